/*
 * ralign.h -- C ABI of the MI355X-native 2-D alignment engine (libralign_hip.so).
 *
 * Two layers, both plain C (pointers and sizes only):
 *
 *  (1) the reference's own ctypes surface, symbol for symbol
 *      (/root/reference/cuda/gpu_aln_noref.h:52-113, cuda/gpu_aln_common.h:62-83,
 *       ctypes mirrors at test_mref_gpu_align.py:91-149), so that the reference drivers can
 *      load this library in place of cuda/gpu_aln_pack.so;
 *  (2) a handle-based `ra_*` API with int error codes that takes DEVICE pointers
 *      (inputs already resident in HBM) and an optional HIP stream; this is what the
 *      Python host side (cryo_ralib_amd/) and bench.py call.
 *
 * Results follow the EMAN2 CPU path (Util.multiref_polar_ali_2d / ormq semantics),
 * the API shape follows the reference's CUDA library.  See DESIGN.md.
 */
#ifndef RALIGN_H
#define RALIGN_H

#include <stdbool.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------ PODs */

/* reference: cuda/gpu_aln_common.h:62-74 ; ctypes test_mref_gpu_align.py:112-123 (32 bytes) */
typedef struct AlignConfig {
    unsigned int sbj_num;    /* particles per device batch                       */
    unsigned int ref_num;    /* references                                       */
    unsigned int img_dim;    /* nx (square images)                               */
    unsigned int ring_num;   /* numr[-3]: outer radius `ou` (rings 1..ring_num)  */
    unsigned int ring_len;   /* reference passes 256; informational here: ring lengths follow Numrinit */
    float shift_step;
    float shift_rng_x;
    float shift_rng_y;
} AlignConfig;

/* reference: cuda/gpu_aln_common.h:76-83 ; ctypes test_mref_gpu_align.py:125-134 (24 bytes).
 * shift_x/shift_y hold the accumulated centre offset (== inverse_transform2 of xform.align2d);
 * it is both input and output of every *_run call.  The caller converts to EMAN2 parameters
 * exactly as test_mref_gpu_align.py:578-588 does. */
typedef struct AlignParam {
    int   sbj_id;
    int   ref_id;
    float shift_x;
    float shift_y;
    float angle;
    bool  mirror;
} AlignParam;

/* ------------------------------------------- (1) reference-compatible names */

/* cuda/gpu_aln_noref.h:52 */
void print_gpu_info(const unsigned int device_idx);
/* cuda/gpu_aln_noref.h:58 */
void gpu_clear(void);
/* cuda/gpu_aln_noref.h:62-65.  Returns host-visible (pinned) memory of num_particles entries. */
AlignParam *pre_align_init(const unsigned int num_particles, const AlignConfig *aln_cfg,
                           const unsigned int device_id);
/* cuda/gpu_aln_noref.h:67-72 */
bool pre_align_size_check(const unsigned int num_particles, const AlignConfig *cfg,
                          const unsigned int device_id, const float request, const bool verbose);
/* cuda/gpu_aln_noref.h:74-77 ; batch_type "sbj_batch" | "ref_batch" */
void pre_align_fetch(const float **img_data, const unsigned int img_num, const char *batch_type);
/* cuda/gpu_aln_noref.h:81 : single-reference search, parameters only */
void pre_align_run(const int start_idx, const int stop_idx);
/* cuda/gpu_aln_noref.h:82 : single-reference search + transform; returns DEVICE pointer to the
 * aligned images [stop-start][nx][nx] (borrowed until the next run/fetch) */
void *pre_align_run_m(const int start_idx, const int stop_idx);
/* cuda/gpu_aln_noref.h:83 : multi-reference search + transform; same return */
void *mref_align_run(const int start_idx, const int stop_idx);
/* cuda/gpu_aln_noref.h:84 : multi-reference search + transform + per-class even/odd sums;
 * returns HOST-readable float[2][R][nx][nx] (even block, then odd block;
 * test_mref_cheng_yu_bdb_cuda.py:550-551) */
float *mref_align_run_m(const int start_idx, const int stop_idx);
/* cuda/gpu_aln_noref.h:113 : per-class member counts of the last mref_align_run_m */
int *get_num_ref(void);
/* cuda/gpu_aln_noref.cu:119 (exported, not in the header) */
void reset_shifts(const float shift_range, const float shift_step);

/* class-resident reference-free alignment (GPU-ISAC), cuda/gpu_aln_noref.h:94-109, gpu_aln_noref.cu:559-782:
 * particles sorted by class (sbj_cid_list non-decreasing runs), one reference per class; every call aligns each
 * particle to the average of its own class, transforms it and rebuilds the class averages on the device.
 * cuda/gpu_aln_noref.h:94-99.  Returns host-visible AlignParam[sbj_num]; ref_id holds the class id. */
AlignParam *ref_free_alignment_2D_init(const AlignConfig *aln_cfg, const float **sbj_data_list,
                                       const float **ref_data_list, const int *sbj_cid_list,
                                       const unsigned int device_id);
/* cuda/gpu_aln_noref.h:101-105 */
bool ref_free_alignment_2D_size_check(const AlignConfig *cfg, const unsigned int device_id, const float request,
                                      const bool verbose);
/* cuda/gpu_aln_noref.h:107 */
void ref_free_alignment_2D(void);
/* cuda/gpu_aln_noref.h:109 ; tangent low-pass of every class average (gpu_aln_noref.cu:786-816) */
void ref_free_alignment_2D_filter_references(const float cutoff_freq, const float falloff);

/* ------------------------------------------------------ (2) handle-based API */

#define RA_OK            0
#define RA_ERR_ARG      -1   /* invalid argument / geometry                   */
#define RA_ERR_HIP      -2   /* HIP runtime failure (message via ra_last_error) */
#define RA_ERR_STATE    -3   /* call out of protocol order                    */
#define RA_ERR_NOMEM    -4

#define RA_MODE_MREF     0   /* Util.multiref_polar_ali_2d: Normalize_ring, out-of-range shifts reset */
#define RA_MODE_REFFREE  1   /* sp_alignment.ormq: no Normalize_ring, shifts clamped                 */

typedef struct ra_config {
    int   nx;             /* image size (square)                                   */
    int   first_ring;     /* --ir                                                  */
    int   last_ring;      /* --ou                                                  */
    int   ring_skip;      /* --rs                                                  */
    float xrng, yrng;     /* --xr --yr                                             */
    float step;           /* --ts                                                  */
    int   nref;           /* references (1 in RA_MODE_REFFREE)                     */
    int   mode;           /* RA_MODE_*                                             */
    int   device;         /* HIP ordinal                                           */
    int   chunk;          /* particles per internal pass (0 = auto)                */
} ra_config;

typedef struct ra_engine ra_engine;

/* per-particle result record written by ra_align (device or host memory, 32 bytes) */
typedef struct ra_result {
    float alpha, sx, sy;  /* EMAN2 xform.align2d parameters (combine_params2 output) */
    int   mirror;
    int   ref_id;
    float peak;           /* CCF peak (qn or qm)                                   */
    int   angle_bin;      /* jtot: 1-based integer angular bin of the peak         */
    int   shift_idx;      /* index of the winning search offset (y outer, x inner) */
} ra_result;

/* Hedges for the two choices of the EMAN2 CPU path that the reference tree does not pin (its arithmetic lives in EMAN2 2.31, which
 * is not part of the reference: SURVEY.md Appendix A.3 / A.4; call sites test_mref_gpu_align.py:1015, 1043-1044):
 *   interp          Util::alrl_ms's interpolation.  RA_INTERP_BILINEAR (Util::bilinear, EMAN2 2.31; default) or RA_INTERP_QUADRI
 *                   (Util::quadri, older releases).  Quadri runs through the size-generic kernels (ra_search_path == 2) whatever
 *                   the geometry -- the particle-resident kernels sample bilinearly only --, and the exact re-evaluation of
 *                   ra_set_refine follows the option.
 *   normalize_ring  Util::Normalize_ring between Polar2Dm and Frngs: -1 = by mode (RA_MODE_MREF on, as inside
 *                   Util.multiref_polar_ali_2d; RA_MODE_REFFREE off, as sp_alignment.ormq), 0 = off, 1 = on.  Every kernel family
 *                   honours it; everything else stays the mode's: the search window rule (mref_ali2d resets a shift beyond
 *                   cnx - last_ring - 2 and cuts the windows with its last_ring argument; ali2d_single_iter clamps, with
 *                   ou = numr[-3]) and the scan over offsets and references (Util::multiref_polar_ali_2d compares every candidate
 *                   with its running peak ROUNDED TO FLOAT; ormq keeps a double) -- both reproduced literally, down to float ties. */
#define RA_INTERP_BILINEAR 0
#define RA_INTERP_QUADRI   1
typedef struct ra_options {
    int interp;           /* RA_INTERP_*                      */
    int normalize_ring;   /* -1 by mode (default), 0 off, 1 on */
} ra_options;

const char *ra_last_error(void);
int  ra_create(ra_engine **out, const ra_config *cfg);
/* ra_create with options (NULL: the defaults = ra_create) */
int  ra_create_ex(ra_engine **out, const ra_config *cfg, const ra_options *opt);
/* switch Normalize_ring for subsequent ra_align calls (flag < 0: back to the mode's default); any time, any kernel path */
int  ra_set_normalize_ring(ra_engine *e, int flag);
/* the options in force (normalize_ring resolved to 0 / 1) */
int  ra_get_options(const ra_engine *e, ra_options *opt);
void ra_destroy(ra_engine *e);
/* use `hip_stream` (a hipStream_t) for all subsequent work; NULL = default stream */
int  ra_set_stream(ra_engine *e, void *hip_stream);
/* geometry queries */
int  ra_num_shifts(const ra_engine *e);
int  ra_maxrin(const ra_engine *e);
int  ra_lcirc(const ra_engine *e);
/* which kernels ra_align runs for the current geometry and window: 1 = particle-resident fused / tiled search kernel (four
 * offsets per pass: rings of up to 256 samples, ou <= 36 -- <= 39 with at most 16 references --, in any box: beyond ~93 pixels over a crop of the
 * image that follows the particle's centre), 0 = polar + contraction kernel pair, 2 = size-generic kernels (rings beyond 512
 * samples, more than 64 rings), 3 = particle-resident search with one or two ring buffers next to the image (search_pair_kernel:
 * ou = 40, and 37 .. 39 with more than 16 references; search_solo_kernel / search_duo_kernel: rings of 512 samples, ou = 41 .. 60) */
int  ra_search_path(const ra_engine *e);
/* with ra_search_path == 3: search offsets per pass, 2 (search_duo_kernel, the default) or 1 (search_solo_kernel); 0 otherwise */
int  ra_search_offsets_per_pass(const ra_engine *e);
/* 1 when the search kernels evaluate the IN-WINDOW offsets of a particle only (sp_alignment.search_range, as the CPU path does): the
 * solo / duo / pair kernels and, since round 6, the size-generic kernels (live-offset lists); 0 when every offset of the list is
 * computed and the out-of-window ones are masked afterwards (fused / tiled kernels, kernel pair) */
int  ra_search_skips_offsets(const ra_engine *e);
/* 1 when the particle-resident path is search_tiled_kernel (reference tiles: 15 and more references), 0 otherwise */
int  ra_search_tiled(const ra_engine *e);
/* search_fused_kernel: rings of at most this many samples (64 | 128) read their bilinear taps from the particle's image in global
 * memory, through the vector L1, instead of the LDS image; 0: every tap from LDS (a geometry or window in which a tap of such a
 * ring could leave the image, and every other kernel).  Follows ra_reset_shifts */
int  ra_search_l1_tap_rings(const ra_engine *e);
/* the rule behind it, without an engine or a device: 128 | 64 when no tap of any sample of the rings of at most that many samples
 * can leave an nx x nx image for any search offset of the window and any shift state the window rule admits, else 0 -- whatever
 * kernel an engine would run and however many references it has (an engine also asks for 3 to 10 references) */
int  ra_l1_tap_rule(int nx, int first_ring, int last_ring, int ring_skip, float xrng, float yrng);
/* change the search window without re-allocating (reset_shifts analogue); the number of
 * offsets may not grow beyond what ra_create sized */
int  ra_reset_shifts(ra_engine *e, float xrng, float yrng, float step);

/* a user mask [nx][nx] (device) instead of model_circle(last_ring) for normalize.mask and the masked statistics
 * (the drivers' optional maskfile argument, test_mref_gpu_align.py:317-321): pixels > 0.5 are inside */
int  ra_set_mask(ra_engine *e, const float *d_mask);

/* --nomirror (test_reffree_gpu_align.py:921, passed to ali2d_single_iter -> ormq): only the straight half of
 * Crosrng_ms takes part in the search (Util.Crosrng_ns); flag != 0 switches it on for subsequent ra_align calls */
int  ra_set_nomirror(ra_engine *e, int flag);

/* references: d_refs [nref][nx][nx] device, ALREADY normalised under the mask
 * (test_mref_gpu_align.py:336).  Polar transform, ring FFT and ring weights
 * (Polar2Dm/Frngs/Applyws, :1015-1017) happen on the device. */
int  ra_set_references(ra_engine *e, const float *d_refs);
/* diagnostic: copy the prepared references in EMAN2 packing [nref][lcirc] to host */
int  ra_get_prepared_references(ra_engine *e, float *h_crefim);

/* search: d_particles [n][nx][nx] device; d_state [n][2] device, accumulated centre offset
 * (in/out); d_result [n] device.  cs = average-centre correction (RA_MODE_REFFREE; NULL = 0).
 * Asynchronous on the engine's stream. */
int  ra_align(ra_engine *e, const float *d_particles, int n, float *d_state,
              ra_result *d_result, const float *cs);
/* Sub-bin angle refinement.  The search finds the winning (reference, offset, mirror, angular bin) in f32; Util::prb1d's
 * second difference c3 amplifies the f32-vs-f64 difference of the 7 CCF samples around a FLAT peak into degrees.  Particles
 * whose |c3| < threshold x max |b| get their 7 samples re-evaluated with the CPU path's own arithmetic (bilinear samples,
 * fftr_q's radix-2 ring FFTs in f32, f64 accumulation of the ring products, f64 inverse) and alpha / sx / sy rewritten.
 * With the refinement on (threshold != 0), float ties are decided the same way: a neighbouring angular bin, another search
 * offset or another reference whose f32 peak lies within 3e-6 (relative) of the winner's is re-evaluated too, and the CPU
 * path's ">=" order picks the integer assignment (angle_bin, shift_idx, ref_id, mirror, peak and d_state follow).
 * threshold < 0: every particle (+25 % of a headline iteration); 0: off; default 0.02 -- no measurable cost, no particle
 * beyond 2e-3 degrees of the CPU path on any tested workload (environment RALIGN_REFINE overrides the default).  Call before
 * ra_set_references.  Geometries whose rings exceed the LDS (256 x 256 / ou = 120: 271 KB per offset) run the same kernels on
 * global scratch.  RA_ERR_STATE only when the ring layout has an odd length (never with Numrinit's powers of two). */
int  ra_set_refine(ra_engine *e, float threshold);
/* particles the last search launch re-evaluated (flat peaks and float ties); synchronises the stream (diagnostics) */
int  ra_last_refine_count(ra_engine *e);
/* LDS ledger (diagnostics, tests): one row for every kernel whose dynamic LDS the engine has raised so far -- search kernels
 * included -- with the static LDS of the loaded code object, the dynamic LDS asked for and the device's limit per workgroup.
 * Every such request is checked (static + dynamic <= limit) before anything is launched; one that does not fit fails with the
 * kernel's name and the two numbers in ra_last_error().  Fills up to `cap` rows and returns the number of rows the engine has.
 * The sub-bin refinement appears as refine_winner_kernel<false> (ring buffers in LDS) or refine_winner_kernel<true> (in
 * global scratch: large ring sets, or RALIGN_REFINE_GM=1).  Read-only. */
typedef struct ra_lds_row {
    char kernel[64];
    int  static_bytes, dynamic_bytes, limit_bytes;
} ra_lds_row;
int  ra_lds_report(const ra_engine *e, ra_lds_row *rows, int cap);
/* the reference's state round trip: rebuild the shift the next search starts from (d_state [n][2]) from the float32
 * parameters of the previous iteration in d_result -- inverse_transform2(alpha, sx, sy) in RA_MODE_MREF
 * (test_mref_gpu_align.py:1024-1026), combine_params2(alpha, sx, sy, mirror, 0, -cs[0], -cs[1], 0) then
 * inverse_transform2 in RA_MODE_REFFREE (ali2d_single_iter; cs = host float[2] or NULL).  Call it before ra_align
 * (then without cs) to follow the reference's loop to the rounding of the header values; without it ra_align
 * continues from the exact d_state it left. */
int  ra_state_from_params(ra_engine *e, const ra_result *d_result, int n, const float *cs, float *d_state);
/* the same with the centre correction in device memory (d_cs [2]): no host value in the path, nothing to wait for */
int  ra_state_from_params_dev(ra_engine *e, const ra_result *d_result, int n, const float *d_cs, float *d_state);
/* class-resident alignment (the ISAC mode behind ref_free_alignment_2D, cuda/gpu_aln_noref.cu:559-782): every particle
 * against the average of its own class, all classes in one launch.  ra_set_class_references prepares ncls references
 * (d_refs [ncls][nx][nx] device); ra_align_classes aligns particle i to reference d_cls[i] (device, [n]); results and
 * state as ra_align.  Needs RA_MODE_REFFREE with nref = 1 on a geometry the fused search kernel covers with the whole
 * image in LDS (ra_search_path == 1 and a box of up to ~93 pixels at ou = 36); RA_ERR_STATE otherwise -- loop over the
 * classes with ra_set_references / ra_align then. */
int  ra_set_class_references(ra_engine *e, const float *d_refs, int ncls);
int  ra_align_classes(ra_engine *e, const float *d_particles, int n, float *d_state,
                      ra_result *d_result, const int *d_cls);
/* apply rot_shift2D with the parameters in d_result and write the aligned images
 * (d_aligned [n][nx][nx], may be NULL) and/or add them into the class sums
 * (d_sums [nref][2][nx][nx] +=, d_counts [nref] +=, may be NULL);
 * even/odd = (index0 + i) % 2 (test_mref_gpu_align.py:1056). */
int  ra_transform_accumulate(ra_engine *e, const float *d_particles, int n, int index0,
                             const ra_result *d_result, float *d_aligned,
                             float *d_sums, int *d_counts);
/* new references from the (all-reduced) class sums: (even+odd)/count then
 * normalize.mask(no_sigma=1) under model_circle(last_ring)
 * (test_mref_gpu_align.py:534-535, 563).  Classes with count < min_count are left
 * untouched in d_refs (the caller re-seeds them, :523-528). */
int  ra_update_references(ra_engine *e, const float *d_sums, const int *d_counts,
                          int min_count, float *d_refs);
/* particle preprocessing on device: subtract the mean under model_circle(last_ring)
 * (normalize.mask no_sigma=0, test_mref_gpu_align.py:342), in place */
int  ra_normalize_particles(ra_engine *e, float *d_particles, int n);
/* diagnostic: run only the polar / ring-FFT stage on n <= chunk particles and return the ring
 * spectra of every search offset in EMAN2 packing, h_out [n][num_shifts][lcirc] (what
 * Polar2Dm -> Normalize_ring -> Frngs leave in `cimage` inside Util.multiref_polar_ali_2d) */
int  ra_debug_spectra(ra_engine *e, const float *d_particles, int n, const float *d_state, float *h_out);
/* diagnostics of the decision stage (finalize and the exact replay; tests/test_gpu_decision.py).  They launch the engine's own
 * kernels with its geometry, tables and stream on buffers of their own, change nothing a search uses, and need the sub-bin
 * refinement (ra_set_refine != 0, ra_set_references called): RA_ERR_STATE otherwise, RA_ERR_ARG for a bad argument; either
 * way nothing is launched or written.  The record layouts (40-byte candidate record, 120-byte refine record) are
 * CAND_DTYPE / REFINE_DTYPE of cryo_ralib_amd/api.py.
 * ra_debug_exact_references: the exact reference spectra h_refx [nref][lcirc] (Polar2Dm -> Frngs -> Applyws in the CPU path's
 * arithmetic) and the copy table h_dup [nref][2] = (first copy, next copy or -1); either may be NULL. */
int  ra_debug_exact_references(ra_engine *e, float *h_refx, int *h_dup);
/* ra_debug_finalize: finalize_kernel (kernel = 0) or finalize_wave_kernel (1) over hand-built candidate records of n <= 32768
 * particles with the states h_state [n][2].  live = 0: h_cand [n][ent_stride][nrtile] (ent_stride: the engine's entries per
 * particle, num_shifts rounded up to 4 -- or num_shifts itself on the size-generic path); live = 1: the records of the in-window
 * offsets only, [ent_base[n]][nrtile], laid out by live_scan_kernel on h_state.  refine_thr as ra_set_refine's threshold.
 * Out: h_res [n] results, h_state_out [n][2], and -- h_rlist != NULL, rlist_cap >= n -- the refine list (in the order of the
 * atomic appends) with *h_count entries; h_rlist = NULL: the kernels run without a list and *h_count = 0. */
int  ra_debug_finalize(ra_engine *e, const void *h_cand, int nrtile, int n, const float *h_state, int kernel, int live,
                       float refine_thr, ra_result *h_res, float *h_state_out, void *h_rlist, int rlist_cap, int *h_count);
/* ra_debug_refine: refine_winner_kernel (ring buffers in LDS or in global scratch, as the engine runs it) over the hand-built
 * list h_rlist [count] (count <= 32768, every index inside the engine's tables) against the engine's exact references;
 * d_particles [n][nx][nx], d_state [n][2], d_result [n] as the search leaves them, d_cls [n] (class-resident mode: particle p
 * against reference d_cls[p], copies ignored) or NULL.  Synchronises. */
int  ra_debug_refine(ra_engine *e, const float *d_particles, int n, const void *h_rlist, int count, float *d_state,
                     ra_result *d_result, const int *d_cls);
/* ---- reference update of one iteration on the device (what the reference's main node does on the
 * CPU, test_mref_gpu_align.py:517-564 / test_reffree_gpu_align.py:374-429, default user function) */
/* length of an FSC curve: nx/2 + 1 */
int  ra_fsc_len(const ra_engine *e);
/* sp_statistics.fsc (masked = 0, :531) or fsc_mask (masked = 1, test_reffree_gpu_align.py:384) between
 * the even and odd sums of every class with count >= min_count, averaged over those classes (:537-548).
 * h_fsc [3][ra_fsc_len]: frequencies, fsc, points per shell (host). */
int  ra_class_fsc(ra_engine *e, const float *d_sums, const int *d_counts, int min_count, int masked,
                  float *h_fsc);
/* per-class curves of the last ra_class_fsc: h_all [nref][2][nx/2+1] = {fsc, points per shell} (the reference writes one
 * drm%03d%04d.txt per class and iteration, test_mref_gpu_align.py:533) */
int  ra_last_class_fsc(ra_engine *e, float *h_all);
/* sp_filter.fit_tanh(dres, low=0.1): host arithmetic; fsc is edited in place like the original. */
int  ra_fit_tanh(const float *freq, float *fsc, int n, float *fl, float *aa);
/* ra_class_fsc + the average over the live classes + fit_tanh + the clamps of ref_ali2d (fl_lo <= fl <= fl_hi, aa <= aa_hi) on
 * the DEVICE (test_mref_gpu_align.py:531-548, sp_user_functions.ref_ali2d): d_fit [5] = {fl, aa clamped; fl, aa as fitted;
 * status (1: every class below min_count)}, d_curve [3][nx/2+1] = {frequency, fsc as fit_tanh leaves it, points per shell}.
 * Asynchronous, no host round trip: ra_filter_references_dev reads (fl, aa) from d_fit. */
int  ra_class_fsc_fit(ra_engine *e, const float *d_sums, const int *d_counts, int min_count, int masked, float fl_lo,
                      float fl_hi, float aa_hi, float *d_fit, float *d_curve);
/* (even + odd) / count without normalisation (:534-535); classes below min_count untouched */
int  ra_class_averages(ra_engine *e, const float *d_sums, const int *d_counts, int min_count,
                       float *d_refs);
/* sp_user_functions.ref_ali2d body on nimg device images, in place: filt_tanl(fl, aa) (fl <= 0: no
 * filter), center_2D: center = 1 phase_cog + fshift, center = -1 fshift by -h_cs_in[i] (average-centre
 * rule, test_reffree_gpu_align.py:403-410), center = 0 none; then normalize.mask(no_sigma=1) under
 * model_circle(last_ring) if normalize != 0 (:563).  h_cs_out [nimg][2] (may be NULL) = applied centres. */
int  ra_filter_references(ra_engine *e, float *d_imgs, int nimg, float fl, float aa, int center,
                          const float *h_cs_in, int normalize, float *h_cs_out);
/* the same with every input in device memory: (fl, aa) = d_flaa[0..1] (NULL: no filter), centres of center = -1 from
 * d_cs_in [nimg][2], applied centres to d_cs_out [nimg][2] (device, may be NULL).  Asynchronous. */
int  ra_filter_references_dev(ra_engine *e, float *d_imgs, int nimg, const float *d_flaa, int center,
                              const float *d_cs_in, int normalize, float *d_cs_out);

/* class-resident mode only (extension, no counterpart in the reference header, where the averages stay in
 * device textures): copy the current class averages [ref_num][nx][nx] to host memory */
int  ra_isac_get_references(float *h_out);

/* diagnostic: the device-memory estimate (bytes) behind pre_align_size_check; (size_t)-1 for a bad geometry */
size_t ra_legacy_bytes(const unsigned int num_particles, const AlignConfig *cfg);

/* CTF phase flip of a stack, in place, without an engine: d_images [n][nx][nx] (device); h_ctf [n][9] (HOST, checked before
 * anything is launched) in the utils_ralib.parse_ctf_star layout (D, Apix, DefocusU, DefocusV, DefocusAngle, Voltage, Cs, w,
 * PhaseShift; A, A, A, A, degrees, kV, mm, -, degrees).  Per particle: embed in a P x P zero image (P = 2 nx with pad != 0,
 * nx otherwise) at (P - nx) / 2, real 2-D DFT, multiply by -sign(ctf) (+1 where ctf == 0) with apix_eff = Apix D / nx,
 * inverse DFT, keep the nx x nx window.  RA_ERR_ARG for nx outside 2 .. 1024, pad not 0 / 1, or a
 * row with a non-finite value, D <= 0, Apix <= 0, voltage <= 0 or w outside [0, 1).  Asynchronous on hip_stream (a
 * hipStream_t; NULL = default stream); bitwise reproducible; every particle is independent of the others. */
int  ra_phase_flip(float *d_images, int n, int nx, const float *h_ctf, int pad, void *hip_stream);

/* Fourier resizing of a stack without an engine: d_in [n][nx][nx] -> d_out [n][m][m] (device, float32), either size the larger.
 * Per image y = A x A^T with the real m x nx operator A[j][i] = (1/nx) sum_{|k| <= min(nx, m)/2} w_k cos(2 pi k (t_j - u_i)),
 * t_j = (j - m/2) / m, u_i = (i - nx/2) / nx, w_k = 1/2 at |k| = nx/2 for even nx and 1 otherwise: the centred trigonometric
 * interpolant of x, band-limited to the smaller grid and sampled on the m grid (Fourier cropping for m < nx, zero padding for
 * m > nx; m == nx is the identity; the output pixel is Apix nx / m).  A is built per call in double and rounded to f32; the
 * products run on f32 MFMA.  RA_ERR_ARG, with nothing launched, for n < 0, nx or m outside 1 .. 1024,
 * a null pointer with n > 0, or overlapping d_in / d_out ranges; n == 0 is a no-op.  Asynchronous on hip_stream (a
 * hipStream_t; NULL = default stream), scratch allocated and freed on that stream; bitwise reproducible; every particle is
 * independent of the others and of its place in the batch. */
int  ra_fourier_resize(const float *d_in, int n, int nx, int m, float *d_out, void *hip_stream);

/* Particle preprocessing without an engine, in place on d_images [n][nx][nx] (device, float32); DESIGN.md section 4.17, contract:
 * cryo_ralib_amd/prep.py.  Centre c = nx/2, u = col - c, v = row - c; every particle is independent of the others and of its
 * place in the batch.
 *   ra_prep_normalize  background set B = {u^2 + v^2 > bg_radius^2}.  ramp != 0: (a, b, c) = the least-squares plane of x over B
 *                      (theta = G^-1 m, G = sum_B [1,u,v]^T [1,u,v] inverted in double on the host, m = sum_B x [1,u,v]);
 *                      e = x - (a + b u + c v) on all pixels, theta = 0 without ramp.  mu = sum_B e / |B|, sigma^2 =
 *                      sum_B (e - mu)^2 / |B| (two passes), y = s (e - mu) / sigma with s = -1 for invert != 0, formed in double
 *                      and rounded to float32 once; sigma == 0 gives s (e - mu).  d_stats (may be NULL): [n][5] double
 *                      (a, b, c, mu, sigma).  A particle with a non-finite pixel gets NaN pixels and statistics.  Every sum is
 *                      double in an order fixed by (nx, bg_radius): no atomics, bitwise reproducible call to call and stream to
 *                      stream.  Domain: 4 <= nx <= 1024, 1 <= bg_radius <= nx/2 (finite), ramp and invert 0 or 1.
 *   ra_prep_filter     embed at (P - nx) / 2 in a P x P zero image (P = 2 nx with pad != 0, else nx), real 2-D DFT, multiply by
 *                      g(d) = LP (1 - HP), d = sqrt(ix^2 + iy^2) / P cycles per pixel, inverse DFT, keep the nx x nx window: the
 *                      passes of ra_phase_flip with g read from a table built once per call (g in double, rounded to float32).
 *                      kind 0: absent (LP = 1, HP = 0); kind 1, tanl(fl = a, aa = b): 1/2 [tanh(k (d + fl)) - tanh(k (d - fl))],
 *                      k = pi / (2 aa fl), 0 < fl < 1, aa > 0; kind 2, gauss(sigma = a): exp(-d^2 / (2 sigma^2)), sigma > 0.
 *                      Domain: 2 <= nx <= 1024, pad 0 or 1, at least one of LP and HP present, finite parameters.
 * RA_ERR_ARG, with nothing launched, for anything outside the domains, n < 0 or a null d_images with n > 0; n == 0 is a no-op.
 * Asynchronous on hip_stream (a hipStream_t; NULL = default stream), scratch allocated and freed on that stream. */
int  ra_prep_normalize(float *d_images, int n, int nx, double bg_radius, int ramp, int invert, double *d_stats, void *hip_stream);
int  ra_prep_filter(float *d_images, int n, int nx, int pad, int lp_kind, double lp_a, double lp_b, int hp_kind, double hp_a,
                    double hp_b, void *hip_stream);

/* CTF-corrected (Wiener-filtered) class averages without an engine (contract: cryo_ralib_amd/wiener.py
 * wiener_reference).  Per particle i: Y_i = rfft2 of rot_shift2D(x_i) (d_params[i]: alpha, sx, sy, mirror as ra_rot_shift2d;
 * ref_id = the class) embedded at o = (P - nx) / 2 in a P x P zero image (P = 2 nx with pad = 1, nx with pad = 0); c_i = the CTF
 * of its [9] row (ra_phase_flip's layout) with DefocusAngle - alpha (mirror 0) or alpha - DefocusAngle (mirror 1) as the
 * astigmatism angle; w_i = c_i, or |c_i| with flipped = 1 (phase-flipped particles).
 *   ra_wiener_accumulate  adds N_j += sum w_i Y_i into d_num [k][P][P/2 + 1] (complex, float2), D_j += sum c_i^2 into
 *                         d_den [k][P][P/2 + 1] and the class sizes into d_counts [k]; the caller zeroes them, so a stack can be
 *                         streamed through in chunks and ranks can all-reduce the sums before finalising.  h_ctf [n][9] is
 *                         host memory, checked with ra_phase_flip's rules before anything is launched; a label outside
 *                         0 .. k - 1 or non-finite alpha / sx / sy is found by a check on the device whose verdict is read back
 *                         (a stream synchronisation) before any sum is written.  RA_ERR_ARG, the sums untouched, for those and
 *                         for n < 0, nx outside 2 .. 1024, pad or flipped not 0 / 1, k outside 1 .. 1024 or a null pointer;
 *                         n == 0 is a no-op.  Scratch is bounded by a fixed budget (chunks of particles), not by n.
 *   ra_wiener_finalize    d_out [k][nx][nx] = crop_o(irfft2(N_j / (D_j + 1/snr))); classes with d_counts[j] < min_count are
 *                         zero.  1 <= k <= 1024, 2 <= nx <= 1024, pad 0 / 1, finite snr > 0.
 * Asynchronous on hip_stream (a hipStream_t; NULL = default stream) apart from the verdict above; no floating-point atomics and
 * a fixed order of every sum: the same calls give bitwise-equal results. */
int  ra_wiener_accumulate(const float *d_images, int n, int nx, const ra_result *d_params, const float *h_ctf, int pad, int flipped,
                          int k, float *d_num, float *d_den, int *d_counts, void *hip_stream);
int  ra_wiener_finalize(const float *d_num, const float *d_den, const int *d_counts, int k, int nx, int pad, float snr, int min_count,
                        float *d_out, void *hip_stream);

/* Half-set FRC and SSNR-weighted class averages (contract: cryo_ralib_amd/wiener.py ssnr_reference).  The
 * half sums are ra_wiener_accumulate's with labels 2j + h and 2k classes, h = (index0 + i) % 2 the particle's global even / odd
 * index: d_num2 [k][2][P][P/2 + 1] (complex), d_den2 [k][2][P][P/2 + 1], d_counts2 [k][2].  Shell s = floor(|(kx, ky)| + 0.5) of
 * each rfft-grid element; shells 0 .. P/2 (S = P/2 + 1) are summed with Hermitian weights (1 on column 0 and, for even P, on column
 * P/2; 2 elsewhere), in double and in a fixed order, over several workgroups per class.
 *   ra_wiener_frc            d_frc [k][S] (double): the FRC of the half averages V_h = N_h / (D_h + 1/snr); 0 where either half
 *                            has no power in the shell, and on every shell of a class with fewer than min_count members.
 *                            d_reg [k][S] (float): R = (shell mean of D0 + D1) / max(2F / (1 - F), ssnr_floor), F = min(FRC, 0.999).
 *   ra_wiener_finalize_ssnr  d_out [k][nx][nx] = crop_o(irfft2((N0 + N1) / (D0 + D1 + R(min(s, P/2))))), 0 where that denominator
 *                            is 0; classes with fewer than min_count members are zero.
 * RA_ERR_ARG, nothing launched, for k outside 1 .. 512, nx outside 2 .. 1024, pad not 0 / 1, snr or ssnr_floor not finite and > 0,
 * or a null pointer.  Asynchronous on hip_stream; no floating-point atomics: the same calls give bitwise-equal results. */
int  ra_wiener_frc(const float *d_num2, const float *d_den2, const int *d_counts2, int k, int nx, int pad, float snr, int min_count,
                   float ssnr_floor, double *d_frc, float *d_reg, void *hip_stream);
int  ra_wiener_finalize_ssnr(const float *d_num2, const float *d_den2, const int *d_counts2, const float *d_reg, int k, int nx, int pad,
                             int min_count, float *d_out, void *hip_stream);

/* Per-particle agreement with the class's Wiener estimate (contract: cryo_ralib_amd/wiener.py
 * score_reference).  d_images, d_params, h_ctf, pad, flipped and k as for ra_wiener_accumulate; d_num, d_den, d_counts are sums it
 * left (over all chunks and ranks, so they normally contain the scored particles) and are only read.  For particle i of class j,
 * with Y, c, w as above: N' = N_j - w Y, D' = max(D_j - c^2, 0) with leave_one_out = 1 (N_j, D_j with 0); tau = 1/snr, or
 * d_reg[j][s] (ra_wiener_frc's term [k][P/2 + 1], used with N = N0 + N1, D = D0 + D1) when d_reg is not NULL;
 * M = w N' / (D' + tau), 0 where that denominator is 0 and, with leave_one_out, everywhere when d_counts[j] < 2.
 * d_sums [n][3] (double) = (sum g Re(Y conj M), sum g |Y|^2, sum g |M|^2) over the elements of shells s_lo <= s <= s_hi, shells
 * and Hermitian weights g as for ra_wiener_frc.  cc = X / sqrt(E F) and the amplitude X / F are the caller's to form.
 * RA_ERR_ARG, d_sums untouched, for everything ra_wiener_accumulate refuses (the device's verdict on labels and params
 * included: one stream synchronisation), leave_one_out not 0 / 1, a band outside 0 <= s_lo <= s_hi <= P/2, d_reg NULL and snr not
 * finite and > 0, d_reg given and k > 512 (snr is then ignored), or a null pointer; n == 0 is a no-op.  Scratch as for
 * ra_wiener_accumulate.  The sums are double, reduced in a fixed order with one writer each: the same call gives the same bits,
 * and a particle's three sums depend neither on its place in the batch nor on how a stack is cut into calls. */
int  ra_wiener_score(const float *d_images, int n, int nx, const ra_result *d_params, const float *h_ctf, int pad, int flipped,
                     int k, const float *d_num, const float *d_den, const int *d_counts, float snr, const float *d_reg,
                     int leave_one_out, int s_lo, int s_hi, double *d_sums, void *hip_stream);

/* Two-stage dimension reduction (utils_ralib.py MPCA / TwoSDR) of a stack in device memory, without an engine (DESIGN.md
 * section 4.6).  All pointers are device pointers; every call is asynchronous on hip_stream (a hipStream_t; NULL = default stream)
 * and allocates and frees its scratch on that stream, as ra_phase_flip does.  Images are [n][p][q] float32, centred on load
 * (x - mean in fp32) where a mean is given.  Results are bitwise reproducible call to call.  RA_ERR_ARG for anything outside the
 * documented domain; nothing is launched then.
 *   ra_sdr_mean     d_mean[p q] = per-pixel mean (double sums in a fixed order, rounded once); 1 <= p, q <= 256, n >= 1
 *                   (p == 1: q <= 2048, the mean of [n][q] factors).
 *   ra_sdr_gram     d_gram (double, exactly symmetric):  form 0: sum X_i^T X_i (q x q);  form 1: sum (X_i P)(X_i P)^T (p x p),
 *                   d_proj P [q][k];  form 2: sum (P^T X_i)^T (P^T X_i) (q x q), d_proj P [p][k].  d_mean NULL: no centring.
 *                   1 <= p, q <= 256 (form 0 with p == 1: q <= 2048, the second stage's n x m matrix); forms 1 / 2: 1 <= k <= 64
 *                   and k <= q (form 1) or k <= p (form 2).
 *   ra_sdr_project  d_U [n][p0 q0] = A^T X_i B, row-major (a, b) -> a q0 + b; d_A [p][p0], d_B [q][q0];
 *                   1 <= p0 <= min(p, 64), 1 <= q0 <= min(q, 64), p0 q0 <= 2048.
 *   ra_sdr_factors  d_F [n][r] = U G; d_U [n][m], d_G [m][r]; 1 <= m <= 2048, 1 <= r <= min(256, m).
 *   ra_rot_shift2d  d_out [n][nx][nx] = rot_shift2D of d_in by d_params[i] (alpha, sx, sy, mirror; the other fields unused): the
 *                   kernel and grid of ra_transform_accumulate without sums, so bitwise equal to its aligned images; 2 <= nx <= 1024.
 *   ra_sdr_reconstruct  d_out [n][p][q] = d_mean + A reshape(c_i) B^T with c_i = G f_i (d_F [n][r], d_G [m][r], m = p0 q0) or,
 *                   d_G NULL, c_i = row i of d_F [n][m] (r_or_m == m then); reshape is (a, b) -> a q0 + b; d_mean NULL adds none.
 *                   With d_resid (and d_images, which go together) d_resid[i] = sum over pixels of (x_i - x^_i)^2 in double, x^_i as
 *                   written, summed in an order fixed by (p, q).  One writer per pixel and per residual, no atomics, no scratch:
 *                   an image's bits depend neither on n nor on its place in the batch.  Domain as ra_sdr_project and
 *                   ra_sdr_factors, but n >= 0: n == 0 is a no-op.  A non-finite factor spoils its own image only. */
int  ra_sdr_mean(const float *d_images, int n, int p, int q, float *d_mean, void *hip_stream);
int  ra_sdr_gram(const float *d_images, int n, int p, int q, const float *d_mean, int form, const float *d_proj, int k,
                 double *d_gram, void *hip_stream);
int  ra_sdr_project(const float *d_images, int n, int p, int q, const float *d_mean, const float *d_A, int p0, const float *d_B,
                    int q0, float *d_U, void *hip_stream);
int  ra_sdr_factors(const float *d_U, int n, int m, const float *d_G, int r, float *d_F, void *hip_stream);
int  ra_rot_shift2d(const float *d_in, int n, int nx, const ra_result *d_params, float *d_out, void *hip_stream);
int  ra_sdr_reconstruct(const float *d_F, int n, int r_or_m, const float *d_G /* NULL: d_F is U */, int p0, int q0,
                        const float *d_A, int p, const float *d_B, int q, const float *d_mean /* NULL: no mean */,
                        const float *d_images /* NULL unless d_resid */, float *d_out, double *d_resid /* or NULL */,
                        void *hip_stream);

/* t-SNE (scikit-learn 1.7 TSNE with method="barnes_hut", angle=0, two output dimensions) of X [n][d] in device memory, without an
 * engine.  Pointers are device pointers; every call is asynchronous on hip_stream (a hipStream_t; NULL =
 * default stream) and allocates and frees its scratch on that stream, as ra_phase_flip does.  Results are bitwise reproducible
 * call to call and across streams (no floating-point atomics; every sum in an order fixed by n).  RA_ERR_ARG for anything outside
 * the documented domain; nothing is launched then.  The optimisation loop around ra_tsne_step is cryo_ralib_amd/tsne.py.
 *   ra_tsne_knn       d_idx [n][k], d_dist2 [n][k]: the k nearest neighbours of every row of d_x [n][d] (float32), itself
 *                     excluded, ordered by (squared euclidean distance, index); distances computed in double from x_i - x_j.
 *                     2 <= n <= 262144, 1 <= d <= 2048, 1 <= k <= min(n - 1, 301).
 *   ra_tsne_affinity  d_pcond [n][k] (double): sklearn's _binary_search_perplexity of each row of d_dist2 (rounded to float as
 *                     sklearn does) for the given perplexity, 0 < perplexity <= 100.
 *   ra_tsne_step      one iteration of sklearn's _gradient_descent: gradient of the KL divergence at d_y [n][2] with the CSR
 *                     affinities (d_indptr [n + 1], d_indices, d_p [nnz], float32) times exaggeration and the exact all-pairs
 *                     repulsion, then gains (d_gains [n][2]), update (d_update [n][2]) and d_y_out = d_y + update
 *                     (d_y_out != d_y).  d_stats (may be NULL): [0] the KL error at d_y, [1] the squared norm of the gradient
 *                     times the gains, as sklearn checks them.  0 <= nnz <= 2 n 301; column indices outside 0 .. n - 1 are skipped.
 *   ra_tsne_error     the same gradient at d_y without an update: d_grad [n][2] (may be NULL), d_stats [0] KL error, [1] squared
 *                     gradient norm (may be NULL; not both). */
int  ra_tsne_knn(const float *d_x, int n, int d, int k, int *d_idx, double *d_dist2, void *hip_stream);
int  ra_tsne_affinity(const double *d_dist2, int n, int k, float perplexity, double *d_pcond, void *hip_stream);
int  ra_tsne_step(const float *d_y, float *d_y_out, float *d_update, float *d_gains, int n, const int *d_indptr, const int *d_indices,
                  const float *d_p, int nnz, float exaggeration, float momentum, float learning_rate, double *d_stats,
                  void *hip_stream);
int  ra_tsne_error(const float *d_y, int n, const int *d_indptr, const int *d_indices, const float *d_p, int nnz, float exaggeration,
                   float *d_grad, double *d_stats, void *hip_stream);

/* Out-of-sample t-SNE: n new points placed into a fixed embedding d_yfit [m][2] of fitted rows d_x [m][d] (DESIGN.md section 4.18;
 * the rules are stated at the top of cryo_ralib_amd/tsne.py).  The conventions are those of ra_tsne_* above.  Every value of a new
 * point is a function of that point, the fitted rows and the parameters alone: bitwise the same whatever n, the point's position,
 * the batch or the stream (no floating-point atomics; every sum in an order fixed by m and k).  A non-finite y or p spoils its own
 * point only.  Shape domain: 1 <= n, nq, rows <= 4194304, 1 <= m <= 262144, 1 <= d <= 2048, 1 <= k <= min(m, 301).
 *   ra_tsne_knn_query       d_idx [nq][k], d_dist2 [nq][k]: for every row of d_q [nq][d] the k rows of d_x [m][d] of least squared
 *                           distance, ordered by (distance, index), distances in double from q_i - x_j with the features in order.
 *                           No row is excluded: a query equal to a base row lists it first at distance 0.  The candidates are
 *                           screened by float32 Gram distances with a margin of 32, as in ra_tsne_knn: on data far from the origin
 *                           relative to its spread (uncentred data) the screen can drop a true neighbour; centre such data first.
 *   ra_tsne_affinity_rows   ra_tsne_affinity's search on any `rows` lists of k distances (1 <= k <= 301): it does not tie k to
 *                           the number of rows, which ra_tsne_affinity does.
 *   ra_tsne_place_gradient  at d_y [n][2]: d_grad [n][2] = 4 (e sum_nbr p w (y_i - Y_j) - sum_{j < m} w^2 (y_i - Y_j) / Z_i),
 *                           d_kl [n] = sum_nbr p log(max(p, tiny) / max(w / Z_i, tiny)), d_z [n] = Z_i = sum_{j < m} w_ij,
 *                           w = 1 / (1 + |y_i - Y_j|^2); d_idx [n][k] and d_p [n][k] (float32) are the neighbour lists, entries
 *                           outside 0 .. m - 1 are skipped.  Each output may be NULL, not all three.  exaggeration e >= 1.
 *   ra_tsne_place           n_iter >= 0 iterations of ra_tsne_step's gains / momentum rule on that gradient from update = 0 and
 *                           gains = 1, in place on d_y, in one launch; d_kl (may be NULL) receives KL_i at the final y.
 *                           0 <= momentum < 1, finite learning_rate > 0. */
int  ra_tsne_knn_query(const float *d_q, int nq, const float *d_x, int m, int d, int k, int *d_idx, double *d_dist2, void *hip_stream);
int  ra_tsne_affinity_rows(const double *d_dist2, int rows, int k, float perplexity, double *d_pcond, void *hip_stream);
int  ra_tsne_place_gradient(const float *d_y, int n, const float *d_yfit, int m, const int *d_idx, const float *d_p, int k,
                            float exaggeration, float *d_grad, double *d_kl, double *d_z, void *hip_stream);
int  ra_tsne_place(float *d_y, int n, const float *d_yfit, int m, const int *d_idx, const float *d_p, int k, float exaggeration,
                   float momentum, float learning_rate, int n_iter, double *d_kl, void *hip_stream);

/* k-means (scikit-learn 1.7 KMeans(algorithm="lloyd") with uniform weights) of X [n][d] in device memory, without an engine
 * (DESIGN.md section 4.8).  Pointers are device pointers; every call is asynchronous on hip_stream (a hipStream_t; NULL = default
 * stream) and allocates and frees its scratch on that stream, as ra_phase_flip does.  Results are bitwise reproducible call to
 * call and across streams (no floating-point atomics; every sum in an order fixed by n, d, k and the labels).  Distances are
 * squared euclidean, decided in double from x - c; labels are the first index of least distance.  The shape domain is
 * 1 <= n <= 4194304, 1 <= d <= 2048, 1 <= k <= min(n, 256); RA_ERR_ARG for anything outside the documented domain, and nothing
 * is launched then.  The seeding draws and the loop around these entries are cryo_ralib_amd/kmeans.py.
 *   ra_kmeans_sqnorm  d_nrm [n] = |x_i|^2 of d_x [n][d] (float32; double sums rounded once): the screen's norms.  k is not an argument.
 *   ra_kmeans_labels  E-step for the centres d_centers [k][d] (double): assign != 0 writes d_labels [n]; assign == 0 keeps the
 *                     labels in d_labels (entries clamped to 0 .. k - 1).  d_inertia [1] (may be NULL when assign != 0) = sum of
 *                     |x_i - c_label|^2.  d_nrm from ra_kmeans_sqnorm, or NULL (computed in scratch).
 *   ra_kmeans_lloyd   one Lloyd iteration: labels of d_centers (d_labels in: the previous labels, -1 before the first
 *                     iteration; out: the new ones), member means into d_centers_new [k][d] (!= d_centers), empty clusters
 *                     relocated to the points farthest from their centre (decreasing distance, ties by lower index) as
 *                     sklearn's _relocate_empty_clusters_dense.  d_stats [3] = {sum_c |c_new - c_old|^2, labels changed,
 *                     clusters found empty}.
 *   ra_kmeans_search  d_idx [m] = np.searchsorted(cumsum(d_w), d_vals, side="left") clipped to n - 1, the cumulative sum of
 *                     d_w [n] (double, >= 0) in a fixed order; 1 <= n <= 4194304, 1 <= m <= 16.
 *   ra_kmeans_seed    one k-means++ step over the m candidate rows d_cand [m] (indices into d_x, clamped): potentials
 *                     sum_i min(d_closest_i, |x_i - x_cand|^2), the first candidate of least potential is chosen and folded into
 *                     d_closest [n] (double).  first != 0 (m = 1): the first centre, d_closest is written, not read.
 *                     d_out [m + 2] = {chosen index, its potential, the m potentials}.  1 <= m <= 16, k is not an argument. */
int  ra_kmeans_sqnorm(const float *d_x, int n, int d, float *d_nrm, void *hip_stream);
int  ra_kmeans_labels(const float *d_x, int n, int d, const float *d_nrm, const double *d_centers, int k, int *d_labels, int assign,
                      double *d_inertia, void *hip_stream);
int  ra_kmeans_lloyd(const float *d_x, int n, int d, const float *d_nrm, const double *d_centers, int k, double *d_centers_new,
                     int *d_labels, double *d_stats, void *hip_stream);
int  ra_kmeans_search(const double *d_w, int n, const double *d_vals, int m, int *d_idx, void *hip_stream);
int  ra_kmeans_seed(const float *d_x, int n, int d, const int *d_cand, int m, double *d_closest, int first, double *d_out,
                    void *hip_stream);

/* Cluster validity of labels d_labels [n] (int, values clamped to 0 .. k - 1; some of the k ids may be unused) on X [n][d] in device
 * memory, after scikit-learn 1.7's sklearn.metrics with metric="euclidean" (DESIGN.md section 4.13).  Same conventions as the
 * k-means entries above: asynchronous on hip_stream, scratch allocated and freed on that stream, bitwise reproducible call to
 * call and across streams, RA_ERR_ARG with nothing launched outside the documented domain.
 *   ra_kmeans_silhouette  d_out [n][3] (double) = {s_i, a_i, b_i}, d_nearest [n] = the other cluster of least mean distance (the
 *                         first one on ties; -1, with b = s = 0, when no other cluster has members).  |x_i - x_j| is
 *                         sqrt(sum_t (x_it - x_jt)^2) from differences in float32; every sum over j is double, in member-list
 *                         order.  a_i = D(i, own) / (n_own - 1), b_i = min over the other non-empty clusters of D(i, c) / n_c,
 *                         s_i = (b_i - a_i) / max(a_i, b_i), 0 for a singleton cluster (a_i = 0 then) and for 0 / 0.
 *                         3 <= n <= 262144, 1 <= d <= 2048, 2 <= k <= 256.
 *   ra_kmeans_dispersion  the label-derived centroids d_centroids [k][d] (double; 0 for an unused id), d_counts [k] (int),
 *                         d_sq [k] = sum over the cluster of |x - mu_c|^2 and d_abs [k] = sum of |x - mu_c|, all in double in
 *                         member-list order: what the Calinski-Harabasz and Davies-Bouldin indices are formed from.
 *                         1 <= n <= 4194304, 1 <= d <= 2048, 1 <= k <= 256. */
int  ra_kmeans_silhouette(const float *d_x, int n, int d, const int *d_labels, int k, double *d_out, int *d_nearest, void *hip_stream);
int  ra_kmeans_dispersion(const float *d_x, int n, int d, const int *d_labels, int k, double *d_centroids, int *d_counts, double *d_sq,
                          double *d_abs, void *hip_stream);

/* One E-step and one M-step of a Gaussian mixture on X [n][d] (float32, device memory), after scikit-learn 1.7's GaussianMixture
 * with covariance_type "full" or "diag" (DESIGN.md section 4.14).  All arithmetic is float64; x - mu is formed in double before it
 * is multiplied.  Same conventions as the k-means entries: asynchronous on hip_stream, scratch allocated and freed on that stream,
 * no floating-point atomics, every sum over i in an order fixed by (n, d, k) (bitwise reproducible call to call and across
 * streams), RA_ERR_ARG with nothing launched outside the domain: 1 <= k <= 256, k <= n <= 4194304, n k <= 2^28, 1 <= d <= 256
 * (full) or 2048 (diag).
 *   ra_gmm_estep  log p_ic = d_offset_c - |(x_i - mu_c)^T PC_c|^2 / 2 (diag: sum_t ((x_it - mu_ct) PC_ct)^2), where the caller
 *                 folds log w_c + log det PC_c - d/2 log 2 pi into d_offset [k].  d_prec_chol: full [k][d][d] row-major, upper
 *                 triangular (16 x 16 tiles below the diagonal are skipped, so the lower triangle must hold zeros); diag [k][d].
 *                 d_log_prob [n] = logsumexp_c log p_ic (max-subtracted), d_log_resp [n][k] = log p - d_log_prob (may be NULL),
 *                 d_labels [n] = argmax_c, the first index on ties (may be NULL), d_sum [1] = sum_i d_log_prob_i.
 *   ra_gmm_mstep  d_resp [n][k] are responsibilities (log_domain != 0: their logarithms, exp() is applied).  d_nk [k] =
 *                 sum_i r_ic + 10 eps, d_means [k][d] = sum_i r_ic x_i / nk_c, d_cov full [k][d][d] = sum_i r_ic (x_i - mu_c)
 *                 (x_i - mu_c)^T / nk_c + reg_covar I (exactly symmetric), diag [k][d] = sum_i r_ic x_i^2 / nk_c - mu_c^2 +
 *                 reg_covar.  reg_covar >= 0. */
#define RA_GMM_FULL 0
#define RA_GMM_DIAG 1
int  ra_gmm_estep(const float *d_x, int n, int d, int k, int cov_type, const double *d_means, const double *d_prec_chol,
                  const double *d_offset, double *d_log_resp, double *d_log_prob, int *d_labels, double *d_sum, void *hip_stream);
int  ra_gmm_mstep(const float *d_x, int n, int d, int k, int cov_type, const double *d_resp, int log_domain, double reg_covar,
                  double *d_nk, double *d_means, double *d_cov, void *hip_stream);

/* DBSCAN of X [n][d] (float32, device memory), after scikit-learn 1.7's DBSCAN(eps, min_samples, metric="euclidean") (DESIGN.md
 * section 4.15).  D2(i, j) = sum_t (x_it - x_jt)^2 in double from differences, the features in order (exactly symmetric, 0 on the
 * diagonal); j is a neighbour of i iff D2(i, j) <= eps * eps (the double product), i included.  Every pass recomputes its
 * distances: nothing of size n^2 is stored.  Same conventions as the k-means entries: asynchronous on hip_stream, scratch
 * allocated and freed on that stream, integer atomics only (bitwise reproducible call to call and across streams), RA_ERR_ARG
 * with nothing launched outside the domain: 1 <= n <= 262144, 1 <= d <= 2048, finite eps > 0, min_samples >= 1.
 *   ra_dbscan_count  d_count [n] = the number of neighbours, d_label [n] = i for a core point (count >= min_samples), -1 otherwise.
 *   ra_dbscan_step   one round of component merging over the core points (d_count as ra_dbscan_count left it): m_i = the least
 *                    d_label of i's core neighbours; every core i with m_i < label_i hooks P[label_i] and P[i] down to m_i (P a
 *                    copy of the labels, integer atomicMin); then, in a launch of its own, a core i follows P to its fixed point
 *                    r and d_label_out [n] (!= d_label) gets r; a non-core i gets m_i, or -1 without a core neighbour.
 *                    d_changed [1] = the number of core points whose label moved.  Repeated from ra_dbscan_count's labels until
 *                    d_changed is 0, d_label_out holds for a core point the lowest core index of its component, for a border
 *                    point the least such index among its core neighbours, and -1 for noise.  The loop is cryo_ralib_amd/dbscan.py. */
int  ra_dbscan_count(const float *d_x, int n, int d, double eps, int min_samples, int *d_count, int *d_label, void *hip_stream);
int  ra_dbscan_step(const float *d_x, int n, int d, double eps, const int *d_count, int min_samples, const int *d_label,
                    int *d_label_out, int *d_changed, void *hip_stream);

/* HDBSCAN of X [n][d] (float32, device memory): the two device parts of cryo_ralib_amd/hdbscan.py, whose docstring holds the
 * contract rule by rule.  D2 is ra_dbscan_count's: double, from differences, the features in order,
 * exactly symmetric.  w2(i, j) = max(core2_i, core2_j, D2(i, j)); edges are totally ordered by (w2, min(i, j), max(i, j)), so the
 * minimum spanning tree is unique.  Every pass recomputes its distances: nothing of size n^2 is stored.  Same conventions as the
 * DBSCAN entries: asynchronous on hip_stream, scratch allocated and freed on that stream, integer atomics only (bitwise
 * reproducible call to call and across streams), no workgroup waits for another, RA_ERR_ARG with nothing launched outside the
 * domain: 2 <= n <= 262144, 1 <= d <= 2048, 1 <= min_samples <= min(n, 302).
 *   ra_hdbscan_core   d_core2 [n] (double) = D2 from i to its (min_samples - 1)-th nearest other point, 0 for min_samples = 1.
 *                     The neighbour is the last column of ra_tsne_knn's index list; the value is recomputed by D2's own chain.
 *   ra_hdbscan_round  one Boruvka round.  d_comp [n]: the lowest index of i's component (values are compared, and range-checked
 *                     before they address anything).  A row pass (one workgroup per 64 rows over all n columns, 4 x 4 double
 *                     accumulators per thread) keeps for every row the least (w2, lo, hi) over the columns of other components;
 *                     the minimum per component then comes from integer atomicMin in two launches: the bit pattern of w2, then
 *                     lo << 32 | hi among the rows that hold that w2.  At a root i = d_comp[i]: d_w2 [i], d_lo [i] < d_hi [i] =
 *                     the component's least outgoing edge.  At every other index, and at the root of a component that holds
 *                     every point: +inf, -1, -1.  The loop, the union-find and the tree of clusters are cryo_ralib_amd/hdbscan.py. */
int  ra_hdbscan_core(const float *d_x, int n, int d, int min_samples, double *d_core2, void *hip_stream);
int  ra_hdbscan_round(const float *d_x, int n, int d, const double *d_core2, const int *d_comp, double *d_w2, int *d_lo, int *d_hi,
                      void *hip_stream);

/* Ward (minimum-variance) agglomeration: the two device parts of cryo_ralib_amd/ward.py, whose docstring holds the contract rule
 * by rule.  The state is the cluster table in device memory: d_c [n][d] (double centroids) and d_size [n]
 * (int; a slot with size <= 0 is dead).  D2 is ra_dbscan_count's chain on the centroids; W2(a, b) = (s_a s_b) / (s_a + s_b) D2, the
 * sizes in double, symmetric bit for bit.  Nothing of size n^2 is stored.  Same conventions as the DBSCAN entries: asynchronous on
 * hip_stream, scratch allocated and freed on that stream, no floating-point atomics (bitwise reproducible call to call and across
 * streams), no workgroup waits for another, RA_ERR_ARG with nothing launched outside the domain: 2 <= n <= 262144, 1 <= d <= 2048.
 *   ra_ward_nearest  d_rows [n_rows] (1 <= n_rows <= 262144) lists slots, in any order, repeats allowed.  By list position:
 *                    d_nn = the live slot b != a that minimises (W2(a, b), b) (ties go to the lower slot), d_w2 = that W2.  A
 *                    listed slot that is dead or outside 0 .. n - 1, or the only live one, gives -1 and +inf.  The list of the live
 *                    columns is rebuilt from d_size on the device in every call.
 *   ra_ward_merge    for each of the n_pairs (1 <= n_pairs <= n / 2) disjoint pairs a = d_a[p] < b = d_b[p]:
 *                    c_a <- (s_a c_a + s_b c_b) / (s_a + s_b) (one fma, one divide per feature), s_a <- s_a + s_b, s_b <- 0.  A
 *                    pair outside 0 <= a < b < n or with a dead member changes nothing.  The rounds are cryo_ralib_amd/ward.py. */
int  ra_ward_nearest(const double *d_c, const int *d_size, int n, int d, const int *d_rows, int n_rows, int *d_nn, double *d_w2,
                     void *hip_stream);
int  ra_ward_merge(double *d_c, int *d_size, int n, int d, const int *d_a, const int *d_b, int n_pairs, void *hip_stream);

/* Spectral embedding (Laplacian eigenmaps / diffusion maps) of a symmetric kNN graph: the device parts of
 * cryo_ralib_amd/spectral.py, whose docstring holds the contract rule by rule.  Everything is double.  The
 * operator is a CSR (d_indptr [n + 1], d_indices, d_val) with the columns of a row ascending; the basis is d_V [m + 1][ldv] (vector j
 * is row j, ldv >= n) and d_q0 [n] the known top eigenvector.  Same conventions as the DBSCAN entries: asynchronous on hip_stream
 * (ra_spectral_spmv alone reads one int back), no floating-point atomics, every sum in an order fixed by the sizes alone (bitwise
 * reproducible call to call and across streams), no workgroup waits for another, every column index range-checked before it
 * addresses anything, RA_ERR_ARG with nothing launched outside the domain: n <= 262144, at most 4096 basis vectors, c <= 64.
 *   ra_spectral_spmv        y = A x, 1 <= n.  16 lanes share a row: lane l adds the entries l, l + 16, ... in order by fma, then the
 *                           lanes combine in a fixed tree, so the order of a row's sum depends on its length only; an empty row
 *                           gives 0.  The CSR is checked on the device first: an indptr that does not ascend from 0 or a column
 *                           outside 0 .. n - 1 returns RA_ERR_ARG with d_y untouched.  d_y != d_x.
 *   ra_spectral_work_bytes  the size of ra_spectral_lanczos' d_work for a call with j0 + steps <= basis; 0 outside the domain.
 *   ra_spectral_lanczos     enqueues `steps` Lanczos steps from basis vector j0 (2 <= n, j0 + steps <= 4096) with no host
 *                           synchronisation.  Step j: w = M v_j; twice h = Q^T w (partial dots [runs of 512 rows][j + 2], then
 *                           the runs in run order), w -= Q h (t order) with Q = [q0, v_0 .. v_j]; d_alpha[j] = v_j . w = h[j + 1]
 *                           of the first pass; d_beta[j] = |w|; v_{j+1} = w / d_beta[j], read from device memory by the scaling
 *                           kernel (zeros when d_beta[j] <= 2^-40, so a breakdown leaves finite values behind it).  d_work is
 *                           256-byte aligned.  The operator is not checked: an entry with a column out of range is skipped.
 *   ra_spectral_ritz        d_Y [c][n]: Y_t = sum_j d_S[j][t] V_j in j order (d_S [m][c]), one writer per element.
 *   ra_spectral_components  one round of minimum-label hooking over the CSR plus pointer compression, in place on d_label [n]
 *                           (start from d_label[i] = i), integer atomicMin only; d_changed[0] = the number of labels that moved.
 *                           Call until it is 0: d_label[i] is then the lowest member of i's component. */
int  ra_spectral_spmv(const int *d_indptr, const int *d_indices, const double *d_val, int n, const double *d_x, double *d_y,
                      void *hip_stream);
size_t ra_spectral_work_bytes(int n, int basis);
int  ra_spectral_lanczos(const int *d_indptr, const int *d_indices, const double *d_val, int n, const double *d_q0, double *d_V, int ldv,
                         int j0, int steps, double *d_alpha, double *d_beta, void *d_work, void *hip_stream);
int  ra_spectral_ritz(const double *d_V, int ldv, int m, int n, const double *d_S, int c, double *d_Y, void *hip_stream);
int  ra_spectral_components(const int *d_indptr, const int *d_indices, int n, int *d_label, int *d_changed, void *hip_stream);

/* UMAP of a kNN graph: the device parts of cryo_ralib_amd/umap.py, whose docstring holds the contract rule by rule (DESIGN.md section
 * 4.22).  Positions are float32 [n][2], every sum is double.  Same conventions as the spectral entries: asynchronous on hip_stream
 * (ra_umap_epochs alone reads one int back, before its first launch), no atomics on positions, every sum in an order fixed by the
 * row's length alone, samples from a counter-based generator keyed by (seed, epoch, entry, sample): bitwise reproducible call to call
 * and across streams.  No workgroup waits for another; every index read from memory is range-checked before it addresses anything;
 * RA_ERR_ARG with nothing launched outside the domain.
 *   ra_umap_smooth_knn  rule 2 on d_dist2 [rows][k] (squared distances as ra_tsne_knn / ra_tsne_knn_query write them), 1 <= rows <=
 *                       4194304, 1 <= k <= 301, target log2(n_neighbors), 2 <= n_neighbors <= 302: d_rho [rows], d_sigma [rows],
 *                       d_w [rows][k].  One wave per row; psum adds lane l's entries l, l + 64, ... in order, then the lanes in the
 *                       xor butterfly 1 .. 32; the mean behind sigma's floor is added in list order.
 *   ra_umap_epochs      enqueues the epochs t = epoch0 .. epoch0 + count - 1 (1 <= epoch0, epoch0 + count - 1 <= n_epochs <= 10000)
 *                       of rules 5 and 6 on the symmetric CSR (d_indptr [n + 1], d_indices, d_rate [nnz] = s / max s), 4 <= n <=
 *                       262144, one launch per epoch and no host synchronisation between them.  Epoch s of the call reads d_y for
 *                       even s and d_y_alt for odd s and writes the other: the result is in d_y_alt if count is odd, else in d_y.
 *                       16 lanes share a row: lane l walks the entries l, l + 16, ... in order, then the lanes combine in the xor
 *                       tree 8, 4, 2, 1.  The CSR is checked on the device first: an indptr that does not ascend from 0 to nnz or a
 *                       column outside 0 .. n - 1 returns RA_ERR_ARG with both buffers untouched.  0 <= negatives <= 16.
 *   ra_umap_place       rule 8's optimisation of d_y [n_new][2] (in: the start; out: the result) against the fixed d_yfit [m][2]
 *                       with the lists d_idx [n_new][k], d_rate [n_new][k] (w / max of the row), all n_epochs epochs in one launch.
 *                       row0 is the global index of the call's first row (the samples' key), so a row's result does not depend on
 *                       its batch.  1 <= n_new <= 4194304 rows a call, row0 >= 0 and row0 + n_new <= 2^48 (the key 16 ((row0 + i) k + slot)
 *                       + s is formed in 64 bits), 2 <= m <= 262144, 1 <= k <= min(m, 301). */
int  ra_umap_smooth_knn(const double *d_dist2, int rows, int k, int n_neighbors, double *d_rho, double *d_sigma, double *d_w,
                        void *hip_stream);
int  ra_umap_epochs(float *d_y, float *d_y_alt, int n, const int *d_indptr, const int *d_indices, const double *d_rate, int nnz, double a,
                    double b, double gamma, int neg, double lr, int n_epochs, int epoch0, int count, unsigned long long seed,
                    void *hip_stream);
int  ra_umap_place(float *d_y, int n_new, long long row0, const float *d_yfit, int m, const int *d_idx, const double *d_rate, int k,
                   double a, double b, double gamma, int neg, double lr, int n_epochs, unsigned long long seed, void *hip_stream);

/* Neighbour ranks for trustworthiness and continuity of an embedding (cryo_ralib_amd/quality.py, whose docstring holds the contract
 * rule by rule).  D2 is ra_dbscan_count's: double, from differences, the features in order, exactly
 * symmetric.  In the row of i, column l precedes column j iff (D2(i, l), l) < (D2(i, j), j); rank(i, j) = 1 + the number of columns
 * l != i that precede j, so 1 <= rank <= n - 1 and ties go to the lower index.  One pass over the n^2 distances per 24 list
 * entries: nothing of size n^2 is stored.  Same conventions as the DBSCAN entries: asynchronous on hip_stream, scratch allocated
 * and freed on that stream, integer atomics only (bitwise reproducible call to call and across streams), no workgroup waits for
 * another, RA_ERR_ARG with nothing launched outside the domain: 2 <= n <= 262144, 1 <= d <= 2048, 1 <= k <= 301 (k is not tied to
 * n: a list may come from anywhere and may repeat an entry).
 *   ra_embed_ranks  d_idx [n][k]: a list per row, e.g. ra_tsne_knn's on another space.  d_rank [n][k] = rank(i, d_idx[i][t]); an
 *                   entry outside 0 .. n - 1, or equal to i, is invalid, addresses nothing and gets rank 0.  d_pen [n] =
 *                   sum_t max(0, d_rank[i][t] - k), the penalty of trustworthiness; an invalid entry adds nothing.  Either output
 *                   may be NULL, not both; the other's bits do not depend on it. */
int  ra_embed_ranks(const float *d_x, int n, int d, const int *d_idx, int k, int *d_rank, long long *d_pen, void *hip_stream);

/* block until the engine's stream is idle */
int  ra_sync(ra_engine *e);

/* timing of the dominant kernel with HIP events on the engine's stream:
 * accumulated milliseconds and launch count since the last reset */
int  ra_kernel_time(ra_engine *e, int enable, double *ms_ccf, int *launches_ccf,
                    double *ms_polar, int *launches_polar);

#ifdef __cplusplus
}
#endif
#endif
