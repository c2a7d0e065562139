// libralign_hip.so -- host side of the MI355X 2-D alignment engine and its C ABI
// (include/ralign.h).  Owns geometry tables, workspaces and the kernel schedule; exposes
// the handle-based ra_* API (device pointers in, asynchronous on one HIP stream).  The
// reference's ctypes surface (ralign_legacy.hip) and the engine-less entry points
// (ralign_ctf.hip, ralign_sdr.hip, ralign_embed.hip, ralign_resize.hip) are files of their own.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "ralign_geom.h"
#include "ralign_kernels.h"
#include "ralign_generic.h"
#include "ralign_xform.h"
#include "ralign_zone.h"
#include "ralign_fused.h"
#include "ralign_tiled.h"
#include "ralign_solo.h"
#include "ralign_duo.h"
#include "ralign_pair.h"
#include "ralign_exact.h"
#include "ralign_refine.h"
#include "ralign_host.h"
#include "ralign_plan.h"

using namespace ralign;

static thread_local std::string g_last_error;
void set_error(const std::string &msg) { g_last_error = msg; }

// device workspace of one engine, shared by ra_create and the size checks of the reference surface
// (pre_align_size_check / ref_free_alignment_2D_size_check), so that the estimate cannot drift from what is allocated
#define RA_XS_LDS_MAX ((size_t)80 * 1024)      // padded image copy of transform_sum_kernel: two workgroups of 1024 threads share a CU

// ---- which kernel of ralign_xform.h a box goes to, decided here and nowhere else (no device is asked)

// transform_kernel keeps the image in this much LDS; transform_generic_kernel takes the boxes beyond a workgroup's 160 KB (203 pixels on)
static size_t xf_lds_bytes(int nx) { return (size_t)((nx * nx + 3) & ~3) * sizeof(float); }
static bool xf_in_lds(int nx) { return xf_lds_bytes(nx) <= (size_t)160 * 1024; }

// rot_shift2D + class sums without the aligned stack
typedef void (*xs_fn)(int, const float *, const ra_result *, const float2 *, const int *, const int *, int, float *);
typedef void (*xs_db_fn)(int, const float *, const ra_result *, const float2 *, const int *, const int *, int, float *, XsGrid);
struct XsPlan {
    enum Kind { NONE, TWO_COPY, ONE_COPY, TILE } kind = NONE;
    xs_db_fn dbfn = nullptr;      // TWO_COPY: transform_sum_db_kernel<sweeps per row band>
    xs_fn fn = nullptr;           // ONE_COPY: transform_sum_kernel<sweeps per band, sweeps>; TILE: transform_sum_tile_kernel
    const char *name = "";        // the kernel's row in the LDS ledger
    int threads = 0;
    size_t lds = 0;               // dynamic LDS of a workgroup
    int npf = 0;                  // sweeps of the 1024-thread workgroup over the image (the whole-image kinds)
    int sb0 = 0, nb0 = 0;         // TWO_COPY: sweeps per row band (at most 9 accumulators per thread), row bands
    int nband = 1;                // ONE_COPY: row bands of at most 8 sweeps (9 accumulators and their prefetch registers are what 128 registers hold)
    int ntile = 0;                // TILE: output tiles of 64 x 64 pixels
    bool whole_image() const { return kind == TWO_COPY || kind == ONE_COPY; }
    const void *kernel() const { return kind == TWO_COPY ? (const void *)dbfn : (const void *)fn; }
};
// Two copies of the padded image per workgroup where that still leaves room for two workgroups on a CU (up to 99 pixels); one
// copy while it fits RA_XS_LDS_MAX (up to 141; up to 24 sweeps are instantiated); beyond, output tiles with the source box of
// each in LDS.  NONE (boxes under 8 pixels): the aligned stack + class_sum_kernel.
static XsPlan xs_plan(int nx)
{
    XsPlan p;
    if (nx < 8) return p;
    const size_t copy = (size_t)(nx + 2) * ((nx + 2) | 1) * sizeof(float);
    const int ry = RA_XS_THREADS / std::min(nx, RA_XS_THREADS), npf = (nx + ry - 1) / ry;
    if (nx <= RA_XS_THREADS && npf <= 24 && copy <= RA_XS_LDS_MAX) {
        p.threads = RA_XS_THREADS; p.npf = npf;
        if (2 * copy <= RA_XS_LDS_MAX) {
            p.kind = XsPlan::TWO_COPY; p.name = "transform_sum_db_kernel"; p.lds = 2 * copy;
            p.nb0 = (npf + 8) / 9; p.sb0 = (npf + p.nb0 - 1) / p.nb0;
            p.dbfn = p.sb0 <= 1 ? transform_sum_db_kernel<1> : p.sb0 <= 2 ? transform_sum_db_kernel<2> : p.sb0 <= 4 ? transform_sum_db_kernel<4>
                   : p.sb0 <= 6 ? transform_sum_db_kernel<6> : transform_sum_db_kernel<9>;
        } else {
            p.kind = XsPlan::ONE_COPY; p.name = "transform_sum_kernel"; p.lds = copy;
            p.nband = npf <= 16 ? 2 : 3;
            p.fn = npf <= 12 ? transform_sum_kernel<6, 12> : npf <= 16 ? transform_sum_kernel<8, 16> : npf <= 20 ? transform_sum_kernel<7, 20>
                 : transform_sum_kernel<8, 24>;
        }
    } else if (nx >= RA_XT_BB) {
        p.kind = XsPlan::TILE; p.name = "transform_sum_tile_kernel"; p.fn = transform_sum_tile_kernel; p.threads = RA_XT_THREADS;
        p.lds = (size_t)2 * RA_XT_BB * RA_XT_BB * sizeof(float);
        p.ntile = ((nx + RA_XT_TS - 1) / RA_XT_TS) * ((nx + RA_XT_TS - 1) / RA_XT_TS);
    }
    return p;
}
// runs every (class, parity) list of cn particles is cut into: ~1024 workgroups (TILE: ~2048, ntile of them per run already), at
// least ~8 members per run on average
static int xs_runs(const XsPlan &p, int nseg, int cn)
{
    const int nrun = p.kind == XsPlan::TILE ? std::min(64, 2048 / (nseg * p.ntile)) : std::min(512, (1024 + nseg - 1) / nseg);
    return std::max(1, std::min(nrun, cn / (8 * nseg)));
}

struct WorkspacePlan {
    int chunk;
    size_t a_floats, cand_recs, refspec_floats, b_floats, alscratch_floats, zscr_recs;
    size_t bytes;          // everything ra_create and the first reference update take from the device
};

// one row of the LDS ledger (ra_lds_report): a kernel whose dynamic LDS the engine raised (raise_dynamic_lds)
struct LdsRow {
    std::string kernel;
    int stat, dyn, limit;          // the code object's static LDS, the dynamic LDS asked for, the device's limit per workgroup (bytes)
};

// The kernel of the particle-resident search (ra_align, ra_align_classes, ra_debug_spectra), recorded where its dynamic LDS is raised
// (setup_fused, setup_solo) and cleared where `fused` / `solo` are, so that what is launched is what was prepared.  The two kernel
// types differ in their last argument: const int *cls, the class of every particle (search_fused_kernel, search_tiled_kernel; null
// outside the class-resident mode), or float *raw, the debug output of the polar stage (the solo, duo and pair kernels).
typedef void (*fused_fn)(DevGeom, FusedGeom, const float *, const float *, int, const float *, int, CandT *, const int *);
typedef void (*solo_fn)(DevGeom, FusedGeom, const float *, const float *, int, const float *, int, CandT *, float *);
typedef void (*ccf_fn)(DevGeom, const float *, const float *, int, int, int, CandT *);
struct SearchPlan {
    fused_fn fused = nullptr;      // search_fused_kernel / search_tiled_kernel (over a crop or not) ...
    fused_fn pack = nullptr;       // ... and search_fused_kernel's dense-offset variant where it exists: the launch picks one (pack_ok)
    solo_fn solo = nullptr;        // or search_solo_kernel / search_duo_kernel / search_pair_kernel ...
    solo_fn debug = nullptr;       // ... and the instantiation ra_debug_spectra runs the polar stage through
    size_t lds = 0;                // dynamic LDS of a workgroup (FusedPlanHost::lds_bytes)
};

struct ra_engine {
    ra_config cfg{};
    std::vector<LdsRow> lds_rows;
    Geometry geo;
    DevGeom dg{};
    hipStream_t stream = nullptr;
    int chunk = 0;
    int shift_cap = 0, pad_cap = 0;     // search offsets the tables / workspace were sized for
    int nrtile = 1;
    std::vector<void *> owned;          // device allocations freed at destroy
    float *d_A = nullptr;               // [chunk * ngroup + 2][a_blk]
    CandT *d_cand = nullptr;             // [(chunk * nshift_pad + 8)][nrtile]
    float *d_refspec = nullptr;         // [nref][lring]
    float *d_B = nullptr;               // [nrtile][LBP][16]
    float *d_cs = nullptr;              // [2]
    float *d_alscratch = nullptr;       // [chunk][nx*nx] aligned images of one chunk (deterministic class sums)
    // sub-bin angle refinement with the CPU path's arithmetic (ralign_exact.h)
    float refine_thr = 0.02f;           // flag |c3| < thr x max |b|; < 0: every particle; 0: off
    bool refine_ok = false;             // tables built
    bool refine_gm = false;             // ring buffers of the exact kernels in global memory (2 lcirc floats exceed the LDS: large boxes)
    float *d_rscratch = nullptr;        // [refine_grid][2 lcirc] (refine_gm)
    int refine_grid = 0;                // waves of a refine_winner_kernel launch
    size_t lds_refine = 0;
    float *d_twx = nullptr, *d_refx = nullptr, *d_cls_refx = nullptr;
    unsigned long long *d_refhash = nullptr;        // [nref] hashes of the exact reference spectra (ref_hash_kernel)
    int *d_refdup = nullptr;                        // [2 nref] copies of a reference inside the stack (DevGeom::ref_dup)
    int *d_twxoff = nullptr, *d_rcount = nullptr;
    RefineRec *d_rlist = nullptr;
    // buffers of the class sums (ralign_xform.h), allocated on first use
    struct {
        // through the aligned stack (class_sum_kernel), sized for a chunk at first use
        int *members = nullptr;         // [2 nref][chunk] member lists of a chunk (class_members_wide_kernel)
        int *mcount = nullptr;          // [2 nref] their lengths
        float *sumpart = nullptr;       // [16][2 nref][nx*nx] per-run partial sums (few classes: class_sum_kernel with runs)
        // in one pass with rot_shift2D (transform_sum), grown to the largest batch seen
        int *xs_members = nullptr;      // [2 nref][batch] member lists of a batch
        size_t cap_members = 0;
        int *xs_mcount = nullptr;       // [2 nref] their lengths
        float *xs_partial = nullptr;    // [runs][2 nref][nx*nx] per-run partial sums
        size_t cap_partial = 0;
        float2 *xs_trig = nullptr;      // [batch] (cos, sin) of every particle's angle (transform_trig_kernel)
        size_t cap_trig = 0;
        int xs_slots = 0;               // workgroups of transform_sum_db_kernel resident on the device at once (occupancy query at first use)
    } cs;
    bool atomic_sums = false;           // RALIGN_ATOMIC_SUMS=1: fp32 atomics instead of particle-order sums
    int *d_ring_off = nullptr, *d_numr = nullptr;
    float *d_wr = nullptr;
    size_t lds_polar = 0, lds_ref = 0, lds_ccf = 0;
    bool force_generic = false;         // options that only the size-generic kernels implement (ra_create_ex)
    // the class of this engine's plan (ralign_plan.h), decided once per plan: create_engine, ra_reset_shifts.  What the class
    // wants; fused / tiled / solo / duo / pair below say what the LDS plans then gave.
    struct { bool fused, tiled, solo, duo, pair; } want{};
    bool generic = false;               // size-generic kernels (ralign_generic.h): large boxes, maxrin > 256, > 48 rings
    bool tcrop = false;                 // generic class, but the search runs search_tiled_kernel over a CROP of the image (tcrop_wanted)
    int crop_S = 0;                     // ... whose side was planned for search shifts of up to this many pixels
    int crop_pst = 0;                   // ... and its row stride in LDS (tcrop_wanted)
    float2 *d_zscr = nullptr;           // [RA_GCCF_NWG][maxrin][64 TM TR] CCF spectra scratch of ccf_generic_kernel
    // polar stage with the image in LDS, ring zone by ring zone (ralign_zone.h); the global-tap kernel stays underneath
    ZonePlanHost zplan;
    ZonePlanDev zdev{};
    bool zones = false;
    float2 *d_stats_part = nullptr;     // [chunk * nshift_pad + 8][nquad_total] Normalize_ring partial sums of every (entry, ring quad)
    size_t zone_cap_rows = 0, zone_cap_pix = 0, zone_cap_zones = 0, stats_part_cap = 0;
    int2 *d_zone_rows = nullptr; int *d_zone_pix = nullptr; ZoneDesc *d_zone_desc = nullptr;
    int *d_ent_base = nullptr, *d_ent_total = nullptr;      // live-offset lists of a chunk (size-generic path): [chunk + 1] entry ranges, their total
    float2 *d_gstats = nullptr;         // [chunk * nshift_pad + 8] Normalize_ring {avg, 1/sigma} of every particle-offset (generic path)
    unsigned long long *d_timeline = nullptr;      // profiling builds only (RALIGN_TIMELINE)
    float *d_cls_refspec = nullptr, *d_cls_Bf = nullptr;      // class-resident mode: [cls_cap][lring], [cls_cap][b_floats]
    int cls_cap = 0, cls_ready = 0;
    float *d_gcdc = nullptr;            // [nref] DC weights of the references (generic and fused paths)
    int g_P = 0;
    size_t lds_gpolar = 0, lds_gccf = 0;
    // reference-update workspace (ralign_refine.h), allocated on first use
    int rf_cap = 0;                     // images the workspace holds
    double2 *d_rfT = nullptr, *d_rfF = nullptr, *d_rftw = nullptr;
    float *d_rfmean = nullptr, *d_rffsc = nullptr, *d_rfcs = nullptr;
    const int *d_fsc_off = nullptr, *d_fsc_idx = nullptr;      // coefficients of every Fourier shell (fsc_shell_table)
    bool refs_ready = false;
    // particle-resident search kernel (ralign_fused.h)
    FusedPlanHost fplan;
    std::vector<int> qoff;              // quadrant-table offset per log2(ring length)
    std::vector<float> ringw_h;
    bool fused = false;                 // plan valid and not disabled (RALIGN_FUSED=0)
    bool tiled = false;                 // the plan is search_tiled_kernel's (ralign_tiled.h: reference tiles, more than RF_MAXREF references)
    bool solo = false;                  // search_solo_kernel (ralign_solo.h: maxrin 512, one offset resident per pass) on top of the generic tables
    bool duo = false;                   // ... as search_duo_kernel (ralign_duo.h): two offsets per pass through the one ring buffer
    bool pair = false;                  // ... search_pair_kernel (ralign_pair.h): maxrin 256 in boxes too large for four ring buffers, two per pass
    SearchPlan search;                  // the kernel behind those flags
    ccf_fn ccf = nullptr;               // ccf_kernel<maxrin> of the kernel pair (LDS-resident class)
    float *d_Bf = nullptr;
    int *d_fbsrc = nullptr;
    size_t f_cap_b = 0;
    CandT *d_fcand = nullptr;           // [(fcand_cap * nshift_pad + 8)] one record per particle-offset of a resident-kernel launch
    int fcand_cap = 0, rlist_cap = 0;   // particles the candidate records / the refine list hold (grown on demand: ensure_resident_ws)
    int n_cu = 256;
    bool unfused_ws = false;            // spectra workspace of the two-kernel path allocated
    WorkspacePlan wp{};
    // kernel timing
    bool timing = false;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_ccf, ev_polar;
    size_t ev_used_ccf = 0, ev_used_polar = 0;
};

int raise_dynamic_lds(std::nullptr_t, const void *fn, const char *name, size_t dyn, int *stat_out, int *limit_out)
{
    int dev = 0, limit = 0;
    hipFuncAttributes fa{};
    RA_HIP(hipGetDevice(&dev));
    RA_HIP(hipDeviceGetAttribute(&limit, hipDeviceAttributeMaxSharedMemoryPerBlock, dev));
    RA_HIP(hipFuncGetAttributes(&fa, fn));
    const size_t stat = fa.sharedSizeBytes;
    if (stat + dyn > (size_t)limit) {
        char buf[512];
        snprintf(buf, sizeof(buf), "%s: %zu bytes of static and %zu bytes of dynamic LDS do not fit the %d bytes of a workgroup", name, stat, dyn, limit);
        g_last_error = buf;
        return RA_ERR_HIP;
    }
    hipError_t he = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
    if (he != hipSuccess) {
        g_last_error = std::string("hipFuncSetAttribute(") + name + "): " + hipGetErrorString(he);
        return RA_ERR_HIP;
    }
    if (stat_out) *stat_out = (int)stat;
    if (limit_out) *limit_out = limit;
    return RA_OK;
}

// the engine's form (ralign_host.h has the comment): the same check, then the row of the ledger (ra_lds_report)
static int raise_dynamic_lds(ra_engine *e, const void *fn, const char *name, size_t dyn)
{
    int stat = 0, limit = 0;
    if (const int rc = raise_dynamic_lds(nullptr, fn, name, dyn, &stat, &limit)) return rc;
    auto it = std::find_if(e->lds_rows.begin(), e->lds_rows.end(), [&](const LdsRow &r) { return r.kernel == name; });
    if (it == e->lds_rows.end()) e->lds_rows.push_back(LdsRow{name, stat, (int)dyn, limit});
    else { it->stat = stat; it->dyn = (int)dyn; it->limit = limit; }
    return RA_OK;
}

// a host table in a device buffer of its own (freed at destroy), through the typed pointer the caller keeps (P: T, const T, or a
// vector type over T such as int4)
template <typename T, typename P> static int upload(ra_engine *e, const std::vector<T> &h, P **dptr)
{
    void *d = nullptr;
    size_t bytes = std::max<size_t>(h.size(), 1) * sizeof(T);
    RA_HIP(hipMalloc(&d, bytes));
    e->owned.push_back(d);
    if (!h.empty()) RA_HIP(hipMemcpy(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    *dptr = (P *)d;
    return RA_OK;
}

static bool fft_plan(int h, int &R1, int &R2)
{
    switch (h) {
    case 4: R1 = 4; R2 = 1; return true;
    case 8: R1 = 8; R2 = 1; return true;
    case 16: R1 = 16; R2 = 1; return true;
    case 32: R1 = 8; R2 = 4; return true;
    case 64: R1 = 8; R2 = 8; return true;
    case 128: R1 = 16; R2 = 8; return true;
    case 256: R1 = 16; R2 = 16; return true;
    default: return false;
    }
}

// polar stage of the size-generic class: alrl_ms with Util::bilinear (default) or Util::quadri (ra_create_ex)
typedef void (*gpolar_fn)(DevGeom, const float *, const float *, int, float *, float2 *);
static gpolar_fn gpolar_kernel(const ra_engine *e, bool refs)
{
    const bool q = e->dg.interp == RA_INTERP_QUADRI;
    return refs ? (q ? (gpolar_fn)polar_generic_kernel<true, true> : (gpolar_fn)polar_generic_kernel<true, false>)
                : (q ? (gpolar_fn)polar_generic_kernel<false, true> : (gpolar_fn)polar_generic_kernel<false, false>);
}

static fused_fn select_tiled(int nh, int sbuf);
static fused_fn select_fused(int maxrin, int nref, int nzr, int sbuf, bool pack = false, bool crop = false, int tapl1 = 0);
// search_tiled_kernel for an engine of the size-generic class: rings of 256 samples (ou <= 36) in a box so much larger than the rings
// that the whole image does not fit next to four ring buffers, but a crop around the particle's sampling centre does (crop_plan,
// ralign_solo.h).  Four offsets per pass with every wave in a ring job instead of the pair kernel's two: 1.6 x its rate.
// RALIGN_TCROP=0: the pair kernel
static bool tcrop_wanted(ra_engine *e, const PlanRequest &rq)
{
    const Geometry &g = e->geo;
    if (!tcrop_class(g, e->cfg, rq, e->generic)) return false;
    FusedGeom t{};
    crop_plan(g, t, rq.sw.crop);
    if (!t.s_crop) return false;
    // the job tables and the image stride are laid out for this kernel before its plan is made (build_device_geometry), so the
    // answer has to be the plan's: the same plan on an upper estimate of the polar part's LDS (tables of 4 offset slots)
    const int sbuf = (g.lring + 31) / 32 * 32 + 16;
    FusedPlanHost tmp;
    // row stride of the crop: 101 words -- the stride of the 90 x 90 headline geometry, which the order of the ring jobs' instances was
    // tuned on -- when the crop is narrower and the plan still fits, else the narrowest conflict-poor one (crop_plan).  Measured
    // (search launch per 8192 / 16 384 particles): ou = 36 / 256 x 256: 5.40 ms at 91, 5.35 at 93, 5.39 - 5.41 at 95 - 99, 5.23 at 101;
    // ou = 30 / 160 x 160: 9.56 ms at 73, 9.28 - 9.54 at 75 - 99, 9.35 at 101
    const int pst_min = t.s_pst;
    for (int pst : {pst_min < 101 && !(RA_EXP_ENV("RALIGN_CROP_PST101") && ra_atoi(RA_EXP_ENV("RALIGN_CROP_PST101")) == 0) ? 101 : pst_min, pst_min}) {
    e->crop_pst = pst;
    const size_t polar = (size_t)pst * pst + 4 * (size_t)std::max(sbuf, sbuf <= RF_SBUF_FIXED ? RF_SBUF_FIXED : sbuf) + 2 * g.maxrin + 3000;
    // the kernels' division of the reference counts is that of the 90 x 90 engines: search_fused_kernel up to RT_MINREF - 1
    // references, search_tiled_kernel from there on (RALIGN_TILED=1: from 7 on, the fewest its tile sizes are instantiated for)
    const bool no_tiled = rq.sw.tiled == 0;
    for (int sb : {sbuf <= RF_SBUF_FIXED ? RF_SBUF_FIXED : sbuf, sbuf}) {
        if (tiled_by_count(e->cfg, rq) && build_tiled_plan(g, e->cfg.nref, sb, polar, tmp) && select_tiled(tmp.f.nh, sb)) return true;
        if (e->cfg.nref <= RF_MAXREF && build_fused_plan(g, e->cfg.nref, sb, polar, tmp) && select_fused(g.maxrin, e->cfg.nref, tmp.f.nzr, sb, false, true)) return true;
        if (!no_tiled && build_tiled_plan(g, e->cfg.nref, sb, polar, tmp) && select_tiled(tmp.f.nh, sb)) return true;
    }
    }
    return false;
}

// the class of the engine's plan, once e->generic and e->tcrop stand
static void decide_class(ra_engine *e, const PlanRequest &rq)
{
    const Geometry &g = e->geo;
    e->want.fused = fused_class(g, e->cfg, rq, e->generic);
    e->want.tiled = e->tcrop ? tiled_by_count(e->cfg, rq) : tiled_class(g, e->cfg, rq);
    e->want.solo = solo_class(g, e->cfg, rq, e->generic);
    e->want.duo = duo_class(g, e->cfg, rq, e->generic);
    e->want.pair = pair_class(g, e->cfg, rq, e->generic);
}

static int build_device_geometry(ra_engine *e, const PlanRequest &rq)
{
    const bool resident4 = e->want.fused || e->tcrop;      // four offset slots per pass in the LDS: search_fused_kernel / search_tiled_kernel
    Geometry &g = e->geo;
    DevGeom &d = e->dg;
    d.nx = g.nx; d.cnx = g.nx / 2 + 1;
    d.nring = g.nring; d.maxrin = g.maxrin; d.lcirc = g.lcirc; d.lring = g.lring; d.nbins = g.nbins;
    d.LB = g.LB; d.LBP = g.LBP; d.last_ring = g.last_ring;
    d.win_ring = e->cfg.mode == RA_MODE_MREF ? g.last_ring : g.numr[3 * (g.nring - 1)];
    d.nshift = g.nshift; d.nshift_pad = g.nshift_pad; d.nkx = g.nkx; d.nky = g.nky; d.ent_stride = e->generic ? g.nshift : g.nshift_pad;      // generic class: dense entries
    d.step = g.step; d.xrng = e->cfg.xrng; d.yrng = e->cfg.yrng;
    d.nn_weight = g.nn_weight; d.inv_nn_weight = g.nn_weight > 0.f ? (float)(1.0 / (double)g.nn_weight) : 0.f; d.lg_maxrin = ilog2_floor(g.maxrin); d.mode = e->cfg.mode; d.nomirror = 0; d.norm_ring = e->cfg.mode == RA_MODE_MREF ? 1 : 0; d.interp = RA_INTERP_BILINEAR; d.quad_aligned = g.quad_aligned ? 1 : 0;
#ifdef RALIGN_PROFILE_SWITCHES
    d.dbg = RA_EXP_ENV("RALIGN_DEBUG") ? ra_atoi(RA_EXP_ENV("RALIGN_DEBUG")) : 0;
    d.timeline = nullptr;
    if (RA_EXP_ENV("RALIGN_TIMELINE")) {          // 64 passes x 16 waves x 16 stamps, written by workgroup 0 for its first particle
        if (!e->d_timeline && hipMalloc(&e->d_timeline, 64 * 16 * 16 * sizeof(unsigned long long)) != hipSuccess) e->d_timeline = nullptr;
        if (e->d_timeline) (void)hipMemset(e->d_timeline, 0, 64 * 16 * 16 * sizeof(unsigned long long));
        d.timeline = e->d_timeline;
    }
#else
    d.dbg = 0;
    d.timeline = nullptr;
#endif
    // ring-buffer stride.  Kernel pair: == 8 (mod 32), the 4 offsets of an entry hit disjoint banks in the write-out gather.
    // Fused kernel: == 16 (mod 32), the two offsets a 4x4x1 MFMA A operand reads (16 bins x Re/Im each) sit in disjoint
    // halves of the 32 banks (RALIGN_SBUF_PAD overrides: experiments)
    int sbuf = (g.lring + 31) / 32 * 32 + (RA_EXP_ENV("RALIGN_SBUF_PAD") ? ra_atoi(RA_EXP_ENV("RALIGN_SBUF_PAD")) : (resident4 ? 16 : 8));
    // fused kernel at maxrin 256: pad the stride to the compile-time value of its fixed-stride instantiations when the image
    // and four such buffers (+ 16 KB of tables and records) still fit the LDS (RALIGN_SBUF_FIXED=0: keep the run-time stride)
    if (resident4 && g.maxrin == 256 && sbuf <= RF_SBUF_FIXED && !RA_EXP_ENV("RALIGN_SBUF_PAD") &&
        !(RA_EXP_ENV("RALIGN_SBUF_FIXED") && ra_atoi(RA_EXP_ENV("RALIGN_SBUF_FIXED")) == 0)) {
        const int bd0 = (int)std::ceil(std::max(e->cfg.xrng, e->cfg.yrng)) + 2, pst0 = e->tcrop ? e->crop_pst : g.nx + 2 * bd0 + 3;
        if ((size_t)(pst0 * pst0 + 4 * RF_SBUF_FIXED + 3400) * sizeof(float) <= 160 * 1024) sbuf = RF_SBUF_FIXED;
    }
    d.sbuf = sbuf;
    d.a_blk = g.LBP * 8 + 64;
    // classes of bins with equal ring-slot count
    d.n_class = 0;
    for (int k = 0; k < g.nbins && !e->generic; k++) {
        int ns = (g.bin_offp[k + 1] - g.bin_offp[k]) / 4;
        if (d.n_class == 0 || d.class_ns[d.n_class - 1] != ns) {
            if (d.n_class == 8) { g_last_error = "too many bin classes"; return RA_ERR_ARG; }
            d.class_k0[d.n_class] = k; d.class_ns[d.n_class] = ns; d.n_class++;
        }
    }
    d.class_k0_end = g.nbins;
    if (!e->generic) {   // start wave of every class: greedy choice that keeps the per-wave MFMA count level
        const int NWV = RA_CCF_THREADS / 64;
        std::vector<long> load(NWV, 0);
        for (int c = 0; c < d.n_class; c++) {
            const int nb = ((c + 1 < d.n_class) ? d.class_k0[c + 1] : g.nbins) - d.class_k0[c], w = d.class_ns[c] + 3;
            int best_r = 0; long best_max = -1, best_sq = 0;
            for (int r = 0; r < NWV; r++) {
                long mx = 0, sq = 0;
                for (int wv = 0; wv < NWV; wv++) {
                    const int first = (wv - r + NWV) % NWV;                 // index of this wave's first bin in the class
                    const long t = load[wv] + (first < nb ? (long)((nb - first + NWV - 1) / NWV) * w : 0);
                    mx = std::max(mx, t); sq += t * t;
                }
                if (best_max < 0 || mx < best_max || (mx == best_max && sq < best_sq)) { best_max = mx; best_sq = sq; best_r = r; }
            }
            d.class_rot[c] = best_r;
            for (int wv = 0; wv < NWV; wv++) {
                const int first = (wv - best_r + NWV) % NWV;
                if (first < nb) load[wv] += (long)((nb - first + NWV - 1) / NWV) * w;
            }
        }
    }
    build_operand_tables(g, sbuf);

    // FFT work lists
    std::vector<int4> A, B, C;
    struct RingPlan { int i, R1, R2; };
    std::vector<RingPlan> plans;
    for (int i = 0; i < g.nring && !e->generic; i++) {
        int n = g.numr[3 * i + 2], R1, R2;
        if (!fft_plan(n / 2, R1, R2)) { g_last_error = "unsupported ring length"; return RA_ERR_ARG; }
        plans.push_back({i, R1, R2});
        for (int b = 0; b < R2; b++) A.push_back(make_int4(g.ring_off[i], R1, R2, b));
        int h = n / 2;
        for (int k = 0; k <= h / 2; k++)
            C.push_back(make_int4(g.ring_off[i] + 2 * k, g.ring_off[i] + 2 * (h - k), k * (g.maxrin / n), k == 0));
    }
    std::stable_sort(A.begin(), A.end(), [](const int4 &a, const int4 &b) { return a.y > b.y; });
    std::stable_sort(plans.begin(), plans.end(), [](const RingPlan &a, const RingPlan &b) { return a.R1 > b.R1; });
    for (auto &p : plans)
        if (p.R2 > 1)
            for (int c = 0; c < p.R1; c++) B.push_back(make_int4(g.ring_off[p.i], p.R1, p.R2, c));
    while (B.size() % 16) B.push_back(make_int4(0, 0, 0, 0));
    d.n_itemA = (int)A.size(); d.n_itemB = (int)B.size(); d.n_itemC = (int)C.size();

    // wave-job schedule of the polar kernel: ring instances (offset slot, ring) sorted by ring
    // length (longest first), cut into jobs of 64/LR instances of one length
    std::vector<float2> qtab;
    std::vector<int4> ringinfo(g.nring);
    std::vector<float> ringw(g.nring);
    std::vector<int4> inst;
    std::vector<float> instw;
    std::vector<int4> jobs;
    {
        std::vector<int> &qoff = e->qoff;
        qoff.assign(32, -1);
        const double qpi = 2 * atan(1.0);
        for (int i = 0; i < g.nring; i++) {
            const int n = g.numr[3 * i + 2], lg = ilog2_floor(n);
            if (qoff[lg] < 0) {
                qoff[lg] = (int)qtab.size();
                const int lt = n / 4;
                const double dfi = qpi / lt;
                for (int jt = 0; jt < lt; jt++) {
                    float fi = (float)(dfi * jt);
                    qtab.push_back(make_float2(sinf(fi), cosf(fi)));
                }
            }
            ringinfo[i] = make_int4(g.ring_off[i], g.numr[3 * i], n, qoff[lg]);
            ringw[i] = (float)(g.numr[3 * i] * 2 * M_PI / (float)n);
        }
        auto code_of = [](int n) { switch (n) { case 512: return 10; case 256: return 0; case 128: return 1; case 64: return 2; case 32: return 3; case 16: return 4; case 8: return 5; default: return -1; } };
        for (int i = 0; i < g.nring && !e->generic; i++)
            if (code_of(g.numr[3 * i + 2]) < 0 || g.numr[3 * i + 2] > 256) { g_last_error = "ring length not supported by the polar kernel (8..256)"; return RA_ERR_ARG; }
        // job code 6: 256-sample rings with 8 lanes per ring (16 sample pairs per lane, two 8-point rows per lane in
        // the second FFT pass) instead of 16 lanes with half of them idle there; code 7 does the same for 64-sample rings
        // (4 lanes x 8 pairs).  Measured: polar stage 5.64 -> 5.2 ms per 7143 particles.
        // nslot = 4: the four offset slots of a pass of the LDS-resident kernels; nslot = 1: search_solo_kernel (rings up to 512
        // samples, code 10: 16 lanes per ring)
        auto make_jobs = [&](int nslot, std::vector<int4> &J, std::vector<int4> &I, std::vector<float> &W, bool lightjobs) {
            const int lanes_of[12] = {16, 8, 8, 4, 4, 4, 8, 4, 0, 0, 16, 32};
            const bool solo = nslot == 1, pairj = nslot == 2;
            // solo class, lightjobs: the short, register-light jobs -- code 11 (512-sample rings, 32 lanes per ring, 8 x 8 x 4:
            // ring_job512) and code 0 -- instead of codes 10 / 6 (16 sample pairs per lane).  They keep all 16 waves busy but are
            // SLOWER in search_solo_kernel (295 k against 324 k particles/s at 128 / 60 / nref 10: the ring jobs of a pass are bound
            // by the LDS array, ~10 k cycles of tap reads and transposes per offset, not by the number of waves that issue them);
            // search_duo_kernel needs them for its second offset, whose ring jobs run next to a live A slice
            // rings of 8 .. 32 samples share jobs of code 9 (ring_job_mix: n / 8 lanes per ring, one table entry per lane)
            // (RALIGN_MIX_JOBS=0, one job per ring length, is an experiment switch of the kernel pair: the fused kernel carries
            // the job variants of codes 1, 6, 7 and 9 only)
            const bool mixed = solo || pairj || (nslot == 4 && (resident4 || !(RA_EXP_ENV("RALIGN_MIX_JOBS") && ra_atoi(RA_EXP_ENV("RALIGN_MIX_JOBS")) == 0)));
            for (int lg = solo ? 9 : 8; lg >= (mixed ? 6 : 3); lg--) {
                const int n = 1 << lg;
                const int code = lightjobs && n == 512 ? 11 : lightjobs && n == 256 ? 0 :
                                 (n == 256 && (nslot == 4 || solo || pairj)) ? 6 : ((n == 64 && (nslot == 4 || solo || pairj)) ? 7 : code_of(n));
                std::vector<int4> cls;
                std::vector<float> clsw;
                for (int sft = 0; sft < nslot; sft++)
                    for (int i = 0; i < g.nring; i++)
                        if (g.numr[3 * i + 2] == n) {
                            cls.push_back(make_int4(sft | (i << 8), g.ring_off[i], qoff[lg], g.numr[3 * i]));
                            clsw.push_back(ringw[i]);
                        }
                const int per_job = 64 / lanes_of[code];
                for (size_t b = 0; b < cls.size(); b += per_job) {
                    const int cnt = (int)std::min<size_t>(per_job, cls.size() - b);
                    J.push_back(make_int4(code, (int)I.size(), cnt, 0));
                    for (int c = 0; c < cnt; c++) { I.push_back(cls[b + c]); W.push_back(clsw[b + c]); }
                }
            }
            if (mixed) {
                std::vector<int4> lanes;              // lane entries of the current job (aligned groups: 4-lane rings first)
                std::vector<float> lanew;
                auto flush = [&]() {
                    if (lanes.empty()) return;
                    J.push_back(make_int4(9, (int)I.size(), (int)lanes.size(), 0));
                    for (size_t c = 0; c < lanes.size(); c++) { I.push_back(lanes[c]); W.push_back(lanew[c]); }
                    lanes.clear(); lanew.clear();
                };
                for (int lg = 5; lg >= 3; lg--) {
                    const int LR = 1 << (lg - 3);
                    for (int sft = 0; sft < nslot; sft++)
                        for (int i = 0; i < g.nring; i++)
                            if (g.numr[3 * i + 2] == (1 << lg)) {
                                if (lanes.size() + LR > 64) flush();
                                for (int t = 0; t < LR; t++) {
                                    lanes.push_back(make_int4(sft | (i << 8) | (lg << 16) | (t << 20), g.ring_off[i], qoff[lg], g.numr[3 * i]));
                                    lanew.push_back(ringw[i]);
                                }
                            }
                }
                flush();
            }
        };
        const bool light_only = rq.sw.solo_jobs == 1;
        if (!e->generic) make_jobs(4, jobs, inst, instw, false);
        else if (e->want.solo) {
            // table A (every kernel of the class; the first offset of a duo pass), then -- duo -- table B: the light jobs of the second offset
            make_jobs(1, jobs, inst, instw, light_only);
            d.n_job_b = 0;
            const int na = (int)jobs.size();
            if (e->want.duo && !light_only) { make_jobs(1, jobs, inst, instw, true); d.n_job_b = (int)jobs.size() - na; }
        } else if (e->tcrop) make_jobs(4, jobs, inst, instw, false);
        else if (e->want.pair) make_jobs(2, jobs, inst, instw, false);
        if (const char *po = RA_EXP_ENV("RALIGN_JOB_ORDER")) {       // experiments: wave w of a pass runs job order[w] ("3,2,1,0,...")
            std::vector<int4> perm;
            for (const char *c = po; *c;) {
                const int k = atoi(c);
                if (k >= 0 && k < (int)jobs.size()) perm.push_back(jobs[k]);
                while (*c && *c != ',') c++;
                if (*c == ',') c++;
            }
            if (perm.size() == jobs.size()) jobs = perm;
        }
    }
    if (!e->want.solo) d.n_job_b = 0;
    d.n_job = (int)jobs.size() - d.n_job_b; d.n_qtab = (int)qtab.size(); d.n_inst = (int)inst.size();
    e->ringw_h = ringw;
    d.bd = (int)std::ceil(std::max(e->cfg.xrng, e->cfg.yrng)) + 2;
    d.pst = g.nx + 2 * d.bd;
    if (e->tcrop) {          // borderless crop (search_tiled_kernel: load_image): rows / columns 0 .. side - 1 + one spare
        d.bd = 0; d.pst = e->crop_pst;
    }
    // row stride of the padded LDS image: the lanes of a ring job sit along an arc and across consecutive radii, so
    // bilinear taps step through the image by +-1 column, +-1 row (= pst words) or a diagonal (pst +- 1).  A stride
    // that is a multiple of 32 (96 at nx = 90) puts every vertical neighbour into the same LDS bank; pick the next
    // stride whose residues pst, pst - 1, pst + 1 share at most a factor 4 with the 32 banks.
    if (!(RA_EXP_ENV("RALIGN_PST_RAW") && ra_atoi(RA_EXP_ENV("RALIGN_PST_RAW")) != 0))
        while (!((d.pst & 1) && ((d.pst - 1) & 7) && ((d.pst + 1) & 7))) d.pst++;

    std::vector<float2> tw(g.maxrin);
    for (int k = 0; k < g.maxrin; k++) {
        double a = -2.0 * M_PI * k / g.maxrin;
        tw[k] = make_float2((float)cos(a), (float)sin(a));
    }
    std::vector<float> mask((size_t)g.nx * g.nx);
    {
        float radius = (float)g.last_ring;
        for (int j = 0; j < g.nx; j++)
            for (int i = 0; i < g.nx; i++) {
                float x2 = ((float)i - g.nx / 2) * ((float)i - g.nx / 2) / (radius * radius);
                float y2 = ((float)j - g.nx / 2) * ((float)j - g.nx / 2) / (radius * radius);
                mask[(size_t)j * g.nx + i] = (x2 + y2 <= 1.0f) ? 1.0f : 0.0f;
            }
    }
    int rc;
    if ((rc = upload(e, g.samp_dx, &d.samp_dx))) return rc;
    if ((rc = upload(e, g.samp_dy, &d.samp_dy))) return rc;
    if ((rc = upload(e, g.samp_w, &d.samp_w))) return rc;
    if ((rc = upload(e, g.samp_dst, &d.samp_dst))) return rc;
    if ((rc = upload(e, g.bin_off, &d.bin_off))) return rc;
    if ((rc = upload(e, g.bin_offp, &d.bin_offp))) return rc;
    if ((rc = upload(e, g.ent_src, &d.ent_src))) return rc;
    if ((rc = upload(e, g.ent_wgt, &d.ent_wgt))) return rc;
    if ((rc = upload(e, g.a_src, &d.a_src4))) return rc;
    if ((rc = upload(e, g.b_src, &d.b_src))) return rc;
    if ((rc = upload(e, g.ent_apos, &d.ent_apos))) return rc;
    if ((rc = upload(e, g.bin_first, &d.bin_first))) return rc;
    // shift tables are sized for the create-time window; ra_reset_shifts rewrites them
    std::vector<float> sx(g.shift_x), sy(g.shift_y);
    if ((rc = upload(e, sx, &d.shift_x))) return rc;
    if ((rc = upload(e, sy, &d.shift_y))) return rc;
    if ((rc = upload(e, tw, &d.tw))) return rc;
    if ((rc = upload(e, A, &d.itemA))) return rc;
    if ((rc = upload(e, B, &d.itemB))) return rc;
    if ((rc = upload(e, C, &d.itemC))) return rc;
    if ((rc = upload(e, mask, &d.mask))) return rc;
    if ((rc = upload(e, jobs, &d.jobs))) return rc;
    if ((rc = upload(e, inst, &d.inst))) return rc;
    if ((rc = upload(e, instw, &d.instw))) return rc;
    if ((rc = upload(e, qtab, &d.qtab))) return rc;
    if ((rc = upload(e, ringinfo, &d.ringinfo))) return rc;
    if ((rc = upload(e, ringw, &d.ringw))) return rc;
    if ((rc = upload(e, g.ring_off, &e->d_ring_off))) return rc;
    if ((rc = upload(e, g.numr, &e->d_numr))) return rc;
    if ((rc = upload(e, g.wr, &e->d_wr))) return rc;
    return RA_OK;
}

template <typename T> static int dev_alloc(ra_engine *e, T **p, size_t count, bool zero)
{
    void *d = nullptr;
    RA_HIP(hipMalloc(&d, std::max<size_t>(count, 1) * sizeof(T)));
    e->owned.push_back(d);
    if (zero) RA_HIP(hipMemset(d, 0, std::max<size_t>(count, 1) * sizeof(T)));
    *p = (T *)d;
    return RA_OK;
}

// replace a device buffer by a larger one (the old one is released now, not at destroy)
template <typename T> static int dev_grow(ra_engine *e, T **p, size_t count, bool zero)
{
    if (*p) {
        auto it = std::find(e->owned.begin(), e->owned.end(), (void *)*p);
        if (it != e->owned.end()) e->owned.erase(it);
        (void)hipStreamSynchronize(e->stream);
        (void)hipFree(*p);
        *p = nullptr;
    }
    return dev_alloc(e, p, count, zero);
}

// Will ra_create select a particle-resident kernel (search_fused_kernel / search_tiled_kernel) for this geometry?  The class
// conditions of the engine's plan (ralign_plan.h) and the LDS estimate of build_device_geometry, evaluated without an engine, so
// that the size checks charge what that path allocates (candidate records, the B stream) instead of the spectra panels of
// the two-kernel path, which are then never allocated (ensure_unfused_ws is lazy).  The LDS figures are estimates of its own, made
// before any table exists; it knows nothing of the crop plan over four ring buffers (tcrop) or the tight-ring geometry.
static bool resident_expected(const Geometry &g, const ra_config &cfg, const PlanRequest &rq, bool generic, size_t *b_floats)
{
    if (generic) {
        // search_solo_kernel / search_duo_kernel (setup_solo): rings of 512 samples, image and one ring buffer in the LDS;
        // search_pair_kernel: rings of 256 samples, image and two ring buffers
        const bool c512 = solo_class(g, cfg, rq, generic), c256 = pair_class(g, cfg, rq, generic);
        if (!(c512 || c256)) return false;
        // the LDS image is a crop around the particle's centre when the box is larger than the rings need (crop_plan)
        FusedGeom t{};
        const int cols = crop_plan(g, t, rq.sw.crop), pst = t.s_pst;
        const int nrp = (cfg.nref + 1) / 2, ntile = (nrp + RS_MAXNH - 1) / RS_MAXNH, nh = (nrp + ntile - 1) / ntile;
        const int sbuf = c256 ? 2 * ((g.lring + 31) / 32 * 32 + 16)
                              : std::max((g.lring + 31) / 32 * 32 + 16, 2 * nh * (2 * (g.maxrin + g.maxrin / 16) + 2));
        if ((size_t)((cols + 1) * pst + sbuf + 4600 + 2 * g.nring + 10 * (g.nring + 16)) * sizeof(float) > 160 * 1024) return false;
        if (b_floats) *b_floats = (size_t)nrp * b_stream_quads(g) * 256 + 256;
        return true;
    }
    if (!fused_class(g, cfg, rq, generic)) return false;
    // the estimate charges the tiled plan's tables from RT_MINREF references on and does not know RALIGN_TILED=1 below that count
    // (the engine's tiled_class does): a forced tiled plan is estimated as the fused one, as it always was.  (fused_class holds for
    // such a request either way: RT_MINREF - 1 <= RF_MAXREF.)
    const bool tiled = tiled_class(g, cfg, rq) && cfg.nref >= RT_MINREF;
    if (g.numr[2] < 8 || g.nring > 64) return false;
    const int bd0 = (int)std::ceil(std::max(cfg.xrng, cfg.yrng)) + 2, pst0 = g.nx + 2 * bd0 + 3;
    const int sbuf0 = (g.lring + 31) / 32 * 32 + 16;
    if ((size_t)(pst0 * pst0 + 4 * sbuf0 + 3400 + (tiled ? 1200 : 0)) * sizeof(float) > 160 * 1024) return false;
    if (b_floats) *b_floats = (size_t)((cfg.nref + 1) / 2) * b_stream_quads(g) * 256 + 256;
    return true;
}

// LDS of the exact kernels (ralign_exact.h) with their ring buffers resident: 2 lcirc floats (or lcirc + the 2 maxrin floats of a
// candidate's spectrum, for very short ring sets) + the twiddles and samples of the f64 CCF (RA_EXACT_TABLE_BYTES)
static size_t refine_resident_lds(const Geometry &g)
{
    return (size_t)((std::max(2 * g.lcirc, g.lcirc + 2 * g.maxrin) + 3) & ~3) * sizeof(float) + RA_EXACT_TABLE_BYTES(g.maxrin);
}
// ... and whether they keep those buffers in global scratch instead: when the resident layout and the kernels' static LDS
// (RA_EXACT_STATIC_LDS) exceed the 160 KB of a workgroup, or when RALIGN_REFINE_GM=1 asks for that route (tests).  The one rule of
// plan_workspace (no device: ra_legacy_bytes) and setup_refine.
#define RA_LDS_PER_WORKGROUP ((size_t)160 * 1024)
static bool refine_rings_global(const Geometry &g, const PlanRequest &rq)
{
    // (a candidate's spectrum, maxrin doubles, lies in the second half of a block of global scratch: ring sets shorter than that
    // keep the resident layout, which has room for it)
    if (rq.sw.refine_gm && g.lcirc >= 2 * g.maxrin) return true;
    return refine_resident_lds(g) + RA_EXACT_STATIC_LDS > RA_LDS_PER_WORKGROUP;
}

// The block shape of the size-generic contraction (ralign_generic.h), described here and nowhere else: TM tiles of 8 particle-offsets
// x TR tiles of 8 references per block.  2 x 2; TM x 7 when the reference tiles come in sevens (gccf_wide_blocks), the B stream then
// read once per 8 TM particle-offsets, with TM of gccf_tm (tm: the value of RALIGN_GCCF_TM, 0 when not set) -- up to 2 in
// ccf_generic_kernel<TM, TR>, which contracts and transforms.  split (maxrin 1024, RALIGN_GCCF_SPLIT): ccf_generic_kernel<TM, TR, true>
// contracts a slice of blocks into the scratch and gccf_ifft_kernel<TM, TR> transforms it.
#define RA_GCCF_NWG 512      // persistent workgroups of ccf_generic_kernel (two per CU)
struct GccfShape {
    int TM, TR;
    int nwg;               // workgroups of the contraction; 4 x 7 blocks: one per CU (256 registers)
    int nblk;              // split: blocks per slice, gccf_blocks_per_wg() to a workgroup (the scratch holds a slice)
    size_t zscr_recs;      // the scratch: 64 TM TR spectra of maxrin / 2 + 1 bins of two values per workgroup, sized for 2 x 7 (= 4 x 7 in half
                           // the workgroups) or for 1 x 7 (which holds 2 x 2)
    size_t lds_ifft;       // dynamic LDS of gccf_ifft_kernel
    long long blocks(long long n_mtile, int nrtile) const { return ((n_mtile + TM - 1) / TM) * ((nrtile + TR - 1) / TR); }
};
static GccfShape gccf_shape(int nrtile, int maxrin, bool split, int tm)
{
    const bool wide = gccf_wide_blocks(nrtile);
    GccfShape s{};
    s.TM = !wide ? 2 : split ? gccf_tm(nrtile, maxrin, tm) : std::min(2, gccf_tm(nrtile, maxrin, tm));
    s.TR = wide ? 7 : 2;
    s.nwg = s.TM >= 4 ? RA_GCCF_NWG / 2 : RA_GCCF_NWG;
    s.nblk = s.nwg * gccf_blocks_per_wg();
    s.zscr_recs = (size_t)RA_GCCF_NWG * (s.TM * s.TR >= 14 ? RA_GCCF_ZPAIRS_MAX : RA_GCCF_ZPAIRS_MAX / 2) * (maxrin + 2) * (maxrin == 1024 ? gccf_blocks_per_wg() : 1);
    s.lds_ifft = ((size_t)8 * RA_IFFT3_PSTRIDE + 16 * 16 + 16 * 64) * sizeof(float2);
    return s;
}

static WorkspacePlan plan_workspace(const Geometry &g, const ra_config &cfg, const PlanRequest &rq, bool generic)
{
    WorkspacePlan w{};
    const int a_blk = g.LBP * 8 + 64, nrtile = (cfg.nref + 7) / 8;
    int chunk = cfg.chunk > 0 ? cfg.chunk : 8192;
    chunk = std::min((chunk + 1) & ~1, 32768);      // class_sum_kernel keeps a chunk's member list in LDS
    const int ngroup = g.nshift_pad / 4;
    const GccfShape gs = gccf_shape(nrtile, g.maxrin, g.maxrin == 1024 && rq.sw.gccf_split, rq.sw.gccf_tm);
    {   // keep the spectra workspace of one chunk within ~12 GB (large boxes: tens of MB per particle)
        const size_t per_particle = (size_t)ngroup * a_blk * sizeof(float);
        const size_t cap = std::max<size_t>(2, ((size_t)12 << 30) / per_particle);
        if ((size_t)chunk > cap) chunk = (int)(cap & ~(size_t)1);
    }
    if (generic && g.maxrin == 1024 && rq.sw.gccf_split && cfg.chunk <= 0) {
        // split contraction: a chunk is walked in slices of nblk blocks, one block per workgroup, and a slice takes its time
        // whether it is full or not (341 particles = 2580 blocks of 4 x 7 tiles = 10 slices of 256 + one of 20): take the chunk
        // size, up to 64 particles below the cap, with the most particles per slice
        int best = chunk;
        double best_pps = 0.0;
        for (int cn = chunk; cn >= std::max(2, chunk - 64); cn -= 2) {
            const long long n_mtile = ((long long)cn * g.nshift + 7) / 8;      // (the generic class packs its entries densely)
            const long long ntask = gs.blocks(n_mtile, nrtile), slices = (ntask + gs.nblk - 1) / gs.nblk;
            const double pps = (double)cn / (double)slices;
            if (pps > best_pps) { best_pps = pps; best = cn; }
        }
        chunk = best;
    }
    w.chunk = chunk;
    w.a_floats = ((size_t)chunk * ngroup + 2) * a_blk;
    w.cand_recs = ((size_t)chunk * g.nshift_pad + 8) * nrtile;
    w.refspec_floats = (size_t)cfg.nref * g.lring;
    w.b_floats = (size_t)nrtile * g.LBP * 16;
    w.alscratch_floats = (size_t)chunk * g.nx * g.nx;
    w.zscr_recs = generic ? gs.zscr_recs : 0;      // CCF-spectra scratch of ccf_generic_kernel, allocated on first use of the generic search
    const size_t nxh = g.nx / 2 + 1, rf_cap = 2 * (size_t)cfg.nref;
    const size_t refine = 2 * rf_cap * g.nx * nxh * sizeof(double2) + rf_cap * (nxh + 3) * sizeof(float) + (size_t)g.nx * sizeof(double2);
    const size_t tables = ((size_t)g.LBP * (8 + 16 + 2) + (size_t)g.lcirc * 4 + (size_t)g.nx * g.nx + (size_t)g.maxrin * 8 + (1 << 16)) * sizeof(float);
    // the particle-resident kernels need one candidate record per particle-offset and their B stream; the spectra panels and
    // per-tile candidates of the two-kernel path are allocated on first use only (never, when the resident kernel runs)
    size_t bf = 0;
    const bool resident = resident_expected(g, cfg, rq, generic, &bf);
    const size_t fcand = (size_t)chunk * g.nshift_pad + 8;
    const size_t search_ws = resident ? bf * (sizeof(float) + sizeof(int)) + fcand * sizeof(CandT)      // B stream + its gather table
                                      : w.a_floats * sizeof(float) + (w.cand_recs + fcand) * sizeof(CandT);
    // rot_shift2D + class sums: member lists, per-run partial sums and cos / sin of a batch (transform_sum_kernel), or -- images
    // that do not fit the LDS -- the aligned images of a chunk, their member lists and 16 runs of partial sums.  (The boxes of
    // transform_sum_tile_kernel are counted with the latter, which overestimates them: they write no aligned stack either.)
    const size_t npix = (size_t)g.nx * g.nx, nseg = 2 * (size_t)cfg.nref;
    const bool xs = xs_plan(g.nx).whole_image();
    const size_t sums_ws = xs ? nseg * chunk * sizeof(int) + std::min<size_t>(512, (1024 + nseg - 1) / nseg) * nseg * npix * sizeof(float) + (size_t)chunk * sizeof(float2)
                              : w.alscratch_floats * sizeof(float) + nseg * chunk * sizeof(int) + 16 * nseg * npix * sizeof(float);
    // sub-bin refinement (ralign_exact.h): exact reference spectra, the list of flagged particles, global ring buffers of large boxes
    const size_t exact_ws = (size_t)cfg.nref * g.lcirc * sizeof(float) + (size_t)chunk * sizeof(RefineRec) +
                            (refine_rings_global(g, rq) ? (size_t)std::max(256, cfg.nref) * 2 * g.lcirc * sizeof(float) : 0);
    w.bytes = (w.refspec_floats + w.b_floats + 2) * sizeof(float) + search_ws + sums_ws + exact_ws +
              (resident ? 0 : w.zscr_recs * sizeof(float2)) + refine + tables;
    // every hipMalloc is rounded up to the allocator's granule; ~40 small tables and buffers
    w.bytes += (size_t)48 * (2 << 20);
    return w;
}

extern "C" const char *ra_last_error(void) { return g_last_error.c_str(); }

static ccf_fn select_ccf(int maxrin)
{
    switch (maxrin) {
    case 256: return ccf_kernel<256>;
    case 128: return ccf_kernel<128>;
    case 64: return ccf_kernel<64>;
    case 32: return ccf_kernel<32>;
    default: return nullptr;
    }
}

// the instantiations with the short rings' taps through the vector L1 (TAPL1 = 64 | 128): the family of the 90 x 90 boxes only --
// rings of 256 samples, compile-time ring-buffer stride, one spectra round per pass, the whole image in LDS, up to 10 references
static bool fused_tap_family(int maxrin, int nzr, int sbuf, bool crop) { return maxrin == 256 && nzr == 1 && sbuf == RF_SBUF_FIXED && !crop; }
template <int TAPL1> static fused_fn select_fused_tap(int nrp, bool pack)
{
    switch ((nrp + 1) / 2) {
    case 1: return pack ? search_fused_kernel<256, 1, true, RF_SBUF_FIXED, true, false, TAPL1> : search_fused_kernel<256, 1, true, RF_SBUF_FIXED, false, false, TAPL1>;
    case 2: return pack ? search_fused_kernel<256, 2, true, RF_SBUF_FIXED, true, false, TAPL1> : search_fused_kernel<256, 2, true, RF_SBUF_FIXED, false, false, TAPL1>;
    case 3: return pack ? search_fused_kernel<256, 3, true, RF_SBUF_FIXED, true, false, TAPL1> : search_fused_kernel<256, 3, true, RF_SBUF_FIXED, false, false, TAPL1>;
    default: return nullptr;      // 13 and more references: no gain measured (14), not instantiated (setup_fused does not ask for it)
    }
}

static fused_fn select_fused(int maxrin, int nref, int nzr, int sbuf, bool pack, bool crop, int tapl1)
{
    if (nref > RF_MAXREF) return nullptr;
    const int nrp = (nref + 1) / 2;
    const bool one = nzr == 1;      // one store / inverse-FFT round per pass
    if (tapl1) {
        if (!fused_tap_family(maxrin, nzr, sbuf, crop)) return nullptr;
        return tapl1 == 128 ? select_fused_tap<128>(nrp, pack) : tapl1 == 64 ? select_fused_tap<64>(nrp, pack) : nullptr;
    }
    if (crop) {                     // the image in LDS is a crop (tcrop_wanted): run-time ring-buffer stride only
        if (maxrin != 256 || (pack && !one)) return nullptr;
        switch ((nrp + 1) / 2) {
        case 1: return pack ? search_fused_kernel<256, 1, true, 0, true, true> : one ? search_fused_kernel<256, 1, true, 0, false, true> : search_fused_kernel<256, 1, false, 0, false, true>;
        case 2: return pack ? search_fused_kernel<256, 2, true, 0, true, true> : one ? search_fused_kernel<256, 2, true, 0, false, true> : search_fused_kernel<256, 2, false, 0, false, true>;
        case 3: return pack ? search_fused_kernel<256, 3, true, 0, true, true> : one ? search_fused_kernel<256, 3, true, 0, false, true> : search_fused_kernel<256, 3, false, 0, false, true>;
        default: return pack ? search_fused_kernel<256, 4, true, 0, true, true> : one ? search_fused_kernel<256, 4, true, 0, false, true> : search_fused_kernel<256, 4, false, 0, false, true>;
        }
    }
    if (pack) {                     // dense offset stream over the workgroup's particles (maxrin 256, one round per pass)
        if (maxrin != 256 || !one) return nullptr;
        if (sbuf == RF_SBUF_FIXED)
            switch ((nrp + 1) / 2) {
            case 1: return search_fused_kernel<256, 1, true, RF_SBUF_FIXED, true>;
            case 2: return search_fused_kernel<256, 2, true, RF_SBUF_FIXED, true>;
            case 3: return search_fused_kernel<256, 3, true, RF_SBUF_FIXED, true>;
            default: return search_fused_kernel<256, 4, true, RF_SBUF_FIXED, true>;
            }
        switch ((nrp + 1) / 2) {
        case 1: return search_fused_kernel<256, 1, true, 0, true>;
        case 2: return search_fused_kernel<256, 2, true, 0, true>;
        case 3: return search_fused_kernel<256, 3, true, 0, true>;
        default: return search_fused_kernel<256, 4, true, 0, true>;
        }
    }
    if (maxrin == 256) {
        if (one && sbuf == RF_SBUF_FIXED)      // compile-time ring-buffer stride
            switch ((nrp + 1) / 2) {
            case 1: return search_fused_kernel<256, 1, true, RF_SBUF_FIXED>;
            case 2: return search_fused_kernel<256, 2, true, RF_SBUF_FIXED>;
            case 3: return search_fused_kernel<256, 3, true, RF_SBUF_FIXED>;
            default: return search_fused_kernel<256, 4, true, RF_SBUF_FIXED>;
            }
        switch ((nrp + 1) / 2) {       // 2 waves per 16-bin group
        case 1: return one ? search_fused_kernel<256, 1, true, 0> : search_fused_kernel<256, 1, false, 0>;
        case 2: return one ? search_fused_kernel<256, 2, true, 0> : search_fused_kernel<256, 2, false, 0>;
        case 3: return one ? search_fused_kernel<256, 3, true, 0> : search_fused_kernel<256, 3, false, 0>;
        default: return one ? search_fused_kernel<256, 4, true, 0> : search_fused_kernel<256, 4, false, 0>;
        }
    }
    if (maxrin == 128) {               // 4 waves per group
        if ((nrp + 3) / 4 == 1) return one ? search_fused_kernel<128, 1, true, 0> : search_fused_kernel<128, 1, false, 0>;
        return one ? search_fused_kernel<128, 2, true, 0> : search_fused_kernel<128, 2, false, 0>;
    }
    return nullptr;
}

static fused_fn select_tiled(int nh, int sbuf)
{
    if (sbuf == RF_SBUF_FIXED)
        switch (nh) {
        case 4: return search_tiled_kernel<256, 4, RF_SBUF_FIXED>;
        case 5: return search_tiled_kernel<256, 5, RF_SBUF_FIXED>;
        default: return nullptr;
        }
    switch (nh) {
    case 4: return search_tiled_kernel<256, 4, 0>;
    case 5: return search_tiled_kernel<256, 5, 0>;
    default: return nullptr;
    }
}

template <typename T> static int grow_upload(ra_engine *e, T **dptr, size_t *cap, const std::vector<T> &h)
{
    if (h.size() > *cap || !*dptr) {
        if (const int rc = dev_grow(e, dptr, h.size(), false)) return rc;
        *cap = std::max<size_t>(h.size(), 1);
    }
    if (!h.empty()) RA_HIP(hipMemcpy(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice));
    return RA_OK;
}

// dense offset stream (search_fused_kernel's PACK): pays when the last pass of a particle would carry padding offsets
// (RALIGN_PACK=0: off -- a switch of the LAUNCH, read at every search, not of the plan: both kernels are prepared by setup_fused)
static bool pack_allowed() { return env_int("RALIGN_PACK", 1) != 0; }
static bool pack_ok(const ra_engine *e)
{
    if (!e->search.pack || !pack_allowed()) return false;
    return e->geo.nshift % 4 != 0 && e->geo.nshift >= 4;      // (a pass holds the offsets of at most two particles)
}

// the resident tables of the plan in e->fplan (fused, tiled, solo, duo, pair): the gather table of the B stream, the stream itself and
// the DC weights of the references
static int upload_resident_tables(ra_engine *e)
{
    FusedPlanHost &fp = e->fplan;
    int rc;
    if ((rc = grow_upload(e, &e->d_fbsrc, &e->f_cap_b, fp.bsrc))) return rc;
    if (!e->d_Bf && (rc = dev_alloc(e, &e->d_Bf, (size_t)fp.f.b_floats + 256, true))) return rc;
    if (!e->d_gcdc && (rc = dev_alloc(e, &e->d_gcdc, (size_t)e->cfg.nref, true))) return rc;
    fp.f.bsrc = e->d_fbsrc; fp.f.cdc_w = e->d_gcdc;
    return RA_OK;
}

// plan of the particle-resident search kernel (ralign_fused.h) and its tables.  It covers every search window of a
// geometry the LDS-resident kernels cover, up to RF_MAXREF references; everything else keeps the two-kernel path.
static int setup_fused(ra_engine *e, const PlanRequest &rq)
{
    e->fused = false; e->tiled = false;
    e->search = SearchPlan{};
    e->fplan.f.on = 0;
    if (e->generic && !e->tcrop) return RA_OK;
    if (!rq.sw.fused) return RA_OK;
    const Geometry &g = e->geo;
    FusedPlanHost &fp = e->fplan;
    const bool no_tiled = rq.sw.tiled == 0;
    auto plan_tiled = [&]() { return build_tiled_plan(g, e->cfg.nref, e->dg.sbuf, e->lds_polar / sizeof(float), fp) && select_tiled(fp.f.nh, e->dg.sbuf); };
    auto plan_fused = [&]() { return select_fused(g.maxrin, e->cfg.nref, 1, 0, false, e->tcrop) && build_fused_plan(g, e->cfg.nref, e->dg.sbuf, e->lds_polar / sizeof(float), fp); };
    if (e->want.tiled && plan_tiled()) e->tiled = true;
    else if (plan_fused()) e->tiled = false;
    else if (e->tcrop && !no_tiled && plan_tiled()) e->tiled = true;
    else if (e->tcrop) {
        g_last_error = "particle-resident search over a crop: the plan tcrop_wanted promised does not fit";
        return RA_ERR_STATE;
    } else return RA_OK;
    if (e->tcrop) {
        FusedGeom tcr{};
        crop_plan(g, tcr, rq.sw.crop);
        fp.f.s_crop = tcr.s_crop; fp.f.s_cropm = tcr.s_cropm;
    }
    // tap source of the short rings (l1_tap_rings): decided with every plan -- ra_create and ra_reset_shifts, whose new search range
    // moves the sampling centres -- for the kernel family that has the instantiations
    // (profiling builds: RALIGN_TAPL1 = 0 | 64 caps the setting; the probe of the LDS taps, RALIGN_DEBUG bit 16384, needs them all in LDS)
    fp.tap_l1 = 0;
    const int tap_cap = (e->dg.dbg & 16384) ? 0 : RA_EXP_ENV("RALIGN_TAPL1") ? ra_atoi(RA_EXP_ENV("RALIGN_TAPL1")) : kTapL1Cap;
    // ... and for 2 to 5 reference pairs (3 - 10 references): where it was measured to win.  Against the LDS taps, at the 90 x 90
    // headline geometry (profiles/tap_source_ab.txt): one pair (reference-free search, the class-resident launch) is 1.9 % SLOWER
    // -- its short contraction leaves the pass to the ring jobs, which the waves with the L1 taps end --, 4 - 8 references gain
    // 3 - 4 %, 10 gain 1.3 %, 14 nothing; 11 and 12 were not measured and keep the LDS taps
    if (!e->tiled && fused_tap_family(g.maxrin, fp.f.nzr, e->dg.sbuf, e->tcrop) && fp.f.nrp >= 2 && fp.f.nrp <= 5)
        fp.tap_l1 = l1_tap_rings(g.numr, g.nring, g.nx, g.last_ring, e->cfg.xrng, e->cfg.yrng, std::min(tap_cap, kTapL1Cap));
    int rc;
    if ((rc = upload_resident_tables(e))) return rc;
    for (int pk = 0; pk < (e->tiled ? 1 : 2); pk++) {
        const fused_fn fk = e->tiled ? select_tiled(fp.f.nh, e->dg.sbuf) : select_fused(g.maxrin, e->cfg.nref, fp.f.nzr, e->dg.sbuf, pk != 0, e->tcrop, fp.tap_l1);
        (pk ? e->search.pack : e->search.fused) = fk;
        if (!fk) continue;
        const std::string kn = std::string(e->tiled ? "search_tiled_kernel" : pk ? "search_fused_kernel<pack>" : "search_fused_kernel") + (e->tcrop ? " (crop)" : "");
        if ((rc = raise_dynamic_lds(e, (const void *)fk, kn.c_str(), fp.lds_bytes))) return rc;
    }
    e->search.lds = fp.lds_bytes;
    if (rq.sw.info) fprintf(stderr, "libralign_hip: %s plan: %zu bytes of LDS (polar part %zu), sbuf %d, pst %d, nzr %d, rz %d\n", e->tiled ? "tiled" : "fused", fp.lds_bytes, e->lds_polar, e->dg.sbuf, e->dg.pst, fp.f.nzr, fp.f.rz);
    e->fused = true;
    return RA_OK;
}

static solo_fn select_solo(int maxrin, int nh, int ntile)
{
    if (maxrin != 512) return nullptr;
    if (ntile > 1)       // 3 .. 5 pairs per tile (build_solo_plan)
        return nh == 3 ? search_solo_kernel<512, 3, false> : nh == 4 ? search_solo_kernel<512, 4, false> : nh == 5 ? search_solo_kernel<512, 5, false> : nullptr;
    switch (nh) {
    case 1: return search_solo_kernel<512, 1, true>;
    case 2: return search_solo_kernel<512, 2, true>;
    case 3: return search_solo_kernel<512, 3, true>;
    case 4: return search_solo_kernel<512, 4, true>;
    case 5: return search_solo_kernel<512, 5, true>;
    default: return nullptr;
    }
}

// NQT: the A slice of a wave holds 14 ring quads when no group of rings has more (ou <= 56), 16 otherwise: the slice lives through
// the second offset's ring jobs and every register counts (nb00: 130 k -> 148 k particles/s with the narrower slice)
template <int NQT>
static solo_fn select_duo_t(int nh)
{
    switch (nh) {
    case 1: return search_duo_kernel<512, 1, NQT>;
    case 2: return search_duo_kernel<512, 2, NQT>;
    case 3: return search_duo_kernel<512, 3, NQT>;
    case 4: return search_duo_kernel<512, 4, NQT>;
    default: return nullptr;
    }
}

static int plan_nqmax(const FusedGeom &f)
{
    int m = 0;
    for (int i = 0; i < 16; i++) m = std::max(m, f.grp_nq[i]);
    return m;
}

// (profiling builds: RALIGN_DUO_NQT=16 asks for the wider slice; read when the plan is made -- setup_solo -- and at no launch)
static solo_fn select_duo(int maxrin, int nh, int nqmax)
{
    if (maxrin != 512) return nullptr;
    const bool q14 = nqmax <= 14 && !(RA_EXP_ENV("RALIGN_DUO_NQT") && ra_atoi(RA_EXP_ENV("RALIGN_DUO_NQT")) == 16);
    return q14 ? select_duo_t<14>(nh) : select_duo_t<16>(nh);
}

static solo_fn select_pair(int maxrin, int nhw)
{
    if (maxrin != 256) return nullptr;
    switch (nhw) {
    case 1: return search_pair_kernel<256, 1>;
    case 2: return search_pair_kernel<256, 2>;
    case 3: return search_pair_kernel<256, 3>;
    default: return nullptr;
    }
}

// plan of search_solo_kernel (ralign_solo.h) for an engine of the size-generic class whose rings end at 512 samples; the generic
// kernels stay available underneath (reference preparation, RALIGN_SOLO=0, geometries whose image and one ring buffer exceed
// the LDS)
static int setup_solo(ra_engine *e, const PlanRequest &rq)
{
    e->solo = false; e->duo = false; e->pair = false;
    const Geometry &g = e->geo;
    FusedPlanHost &fp = e->fplan;
    if (e->fused) return RA_OK;          // tcrop: search_tiled_kernel over a crop of the image took this engine of the generic class
    e->search = SearchPlan{};
    if (e->want.pair) {
        // maxrin 256 in a box too large for four ring buffers: two offsets per pass in two (ralign_pair.h)
        if (!build_pair_plan(g, e->cfg.nref, e->dg.n_qtab, e->dg.n_inst, e->dg.n_job, rq.sw.crop, fp)) { fp.f.on = 0; return RA_OK; }
        const solo_fn fk = select_pair(g.maxrin, fp.f.nrpw);
        if (!fk) { fp.f.on = 0; return RA_OK; }
        int rc;
        if ((rc = upload_resident_tables(e))) return rc;
        if ((rc = raise_dynamic_lds(e, (const void *)fk, "search_pair_kernel", fp.lds_bytes)) || (rc = raise_dynamic_lds(e, (const void *)search_pair_kernel<256, 1>, "search_pair_kernel<256, 1>", fp.lds_bytes))) return rc;
        e->search.solo = fk; e->search.debug = search_pair_kernel<256, 1>; e->search.lds = fp.lds_bytes;
        if (rq.sw.info) fprintf(stderr, "libralign_hip: pair plan: %zu bytes of LDS, image %d x %d, 2 ring buffers of %d floats, %d jobs, %d tiles of 2 x %d reference pairs\n",
                                           fp.lds_bytes, fp.f.s_rows, fp.f.s_pst, fp.f.s_sbuf, e->dg.n_job, fp.f.ntile, fp.f.nrpw);
        e->solo = true; e->pair = true;
        return RA_OK;
    }
    if (!e->want.solo) return RA_OK;
    solo_fn fk = nullptr;
    e->duo = e->want.duo && build_duo_plan(g, e->cfg.nref, e->dg.n_qtab, e->dg.n_inst, e->dg.n_job + e->dg.n_job_b, rq.sw.crop, fp) &&
             (fk = select_duo(g.maxrin, fp.f.nh, plan_nqmax(fp.f)));
    if (!e->duo) {
        if (!build_solo_plan(g, e->cfg.nref, e->dg.n_qtab, e->dg.n_inst, e->dg.n_job + e->dg.n_job_b, rq.sw.crop, fp)) { fp.f.on = 0; return RA_OK; }
        fk = select_solo(g.maxrin, fp.f.nh, fp.f.ntile);
    }
    if (!fk) { fp.f.on = 0; return RA_OK; }
    int rc;
    if ((rc = upload_resident_tables(e))) return rc;
    if ((rc = raise_dynamic_lds(e, (const void *)fk, e->duo ? "search_duo_kernel" : "search_solo_kernel", fp.lds_bytes)) ||
        (rc = raise_dynamic_lds(e, (const void *)search_solo_kernel<512, 1, true>, "search_solo_kernel<512, 1, true>", fp.lds_bytes))) return rc;          // ra_debug_spectra: the polar stage through the solo kernel's debug path
    e->search.solo = fk; e->search.debug = search_solo_kernel<512, 1, true>; e->search.lds = fp.lds_bytes;
    if (rq.sw.info) fprintf(stderr, "libralign_hip: %s plan:", e->duo ? "duo" : "solo");
    if (rq.sw.info) fprintf(stderr, " %zu bytes of LDS, image %d x %d, ring buffer %d floats, %d jobs, %d tiles of %d reference pairs\n",
                                       fp.lds_bytes, fp.f.s_rows, fp.f.s_pst, fp.f.s_sbuf, e->dg.n_job, fp.f.ntile, fp.f.nh);
    e->solo = true;
    return RA_OK;
}

// plan and tables of polar_zone_kernel (ralign_zone.h) for an engine that runs the size-generic polar stage: ring zones whose
// annulus (for every search offset of the window) fits the LDS.  RALIGN_ZONES=0: the global-tap kernel.  Quadri sampling (six
// taps, periodic) stays with the global-tap kernel.
static int setup_zones(ra_engine *e, const PlanRequest &rq)
{
    e->zones = false;
    if (!e->generic || e->fused || e->solo || e->dg.interp != RA_INTERP_BILINEAR) return RA_OK;
    if (!rq.sw.zones) return RA_OK;
    const Geometry &g = e->geo;
    const int S = (int)std::ceil(std::max(g.nkx, g.nky) * g.step - 1e-6);
    if (!build_zone_plan(g, S, RA_ZONE_NW, e->dg.n_qtab, e->zplan)) return RA_OK;
    ZonePlanHost &zp = e->zplan;
    if (const char *ev = RA_EXP_ENV("RALIGN_ZONE_CHUNKS")) { const int v = ra_atoi(ev); if (v >= 1 && v <= 64) zp.nchunk = v; }
    zp.nchunk = std::min(zp.nchunk, std::max(1, g.nshift));
    int rc;
    if ((rc = grow_upload(e, &e->d_zone_rows, &e->zone_cap_rows, zp.rowtab)) || (rc = grow_upload(e, &e->d_zone_pix, &e->zone_cap_pix, zp.pixtab)) ||
        (rc = grow_upload(e, &e->d_zone_desc, &e->zone_cap_zones, zp.zones))) return rc;
    const size_t need = ((size_t)e->chunk * e->pad_cap + 8) * zp.nquad_total;
    if (need > e->stats_part_cap) {
        if ((rc = dev_grow(e, &e->d_stats_part, need, true))) return rc;
        e->stats_part_cap = need;
    }
    if ((rc = RA_LDS(e, polar_zone_kernel<RA_ZONE_NW>, zp.lds_bytes))) return rc;
    e->zdev.zones = e->d_zone_desc; e->zdev.rowtab = e->d_zone_rows; e->zdev.pixtab = e->d_zone_pix;
    e->zdev.nzone = (int)zp.zones.size(); e->zdev.nchunk = zp.nchunk; e->zdev.nquad_total = zp.nquad_total; e->zdev.max_rows = zp.max_rows;
    if (rq.sw.info) {
        fprintf(stderr, "libralign_hip: zone plan: %d zones, %zu bytes of LDS, %d offset chunks, S = %d:", e->zdev.nzone, zp.lds_bytes, zp.nchunk, S);
        for (const ZoneDesc &z : zp.zones) fprintf(stderr, " [rings %d..%d: %d px, %d rows]", z.ring0, std::min(z.ring0 + 4 * z.nquad, g.nring) - 1, z.npix, z.nrow);
        fprintf(stderr, "\n");
    }
    e->zones = true;
    return RA_OK;
}

// Live-offset lists (round 6): the size-generic kernels work on the IN-WINDOW search offsets of every particle only -- what
// Util.multiref_polar_ali_2d / ormq loop over (search_range) -- instead of computing all of them and masking in finalize_kernel.  A tight
// box (configs[4]: ou + xr = 125 of 127) leaves a particle that sits 5 pixels off centre 8 of its 11 offsets per axis: 19 % less work
// in all three stages once the states have moved.  The entries of a chunk then depend on its states: live_scan_kernel lays the ranges
// out on the device, the kernels read the total there, the host launches for the full lists (empty slices return at once).
// RALIGN_LIVE_OFFSETS=0: every offset of the list, masked later (as the particle-resident 90 x 90 kernels do).
static int update_live_mode(ra_engine *e, const PlanRequest &rq)
{
    e->dg.ent_base = nullptr; e->dg.ent_total = nullptr;
    if (!e->generic || e->fused || e->solo) return RA_OK;
    if (!rq.sw.live_offsets) return RA_OK;
    int rc;
    if (!e->d_ent_base && ((rc = dev_alloc(e, &e->d_ent_base, (size_t)e->chunk + 8, true)) || (rc = dev_alloc(e, &e->d_ent_total, 4, true)))) return rc;
    e->dg.ent_base = e->d_ent_base; e->dg.ent_total = e->d_ent_total;
    return RA_OK;
}

// tables and buffers of the sub-bin angle refinement (ralign_exact.h): twiddles (float) of the double-precision cos / sin for
// every power-of-two length, as fftr_q's tables; exact reference spectra; the list of flagged particles of a chunk
static int setup_refine(ra_engine *e, const PlanRequest &rq)
{
    const Geometry &g = e->geo;
    e->refine_ok = false;
    if (rq.sw.refine) e->refine_thr = (float)atof(rq.sw.refine);
    e->lds_refine = refine_resident_lds(g);
    if (g.lcirc & 1) return RA_OK;
    // large boxes: one offset's rings exceed the LDS (271 KB at 256 x 256 / ou = 120) -- the same kernels with the ring buffers
    // in global scratch.  The rule reserves RA_EXACT_STATIC_LDS for the kernels' static LDS (reduction scratch, the tie candidates
    // and their replay list: 1280 bytes); the figure of the loaded code object must not exceed the reserve, or the rule -- which
    // plan_workspace shares and applies without a device -- would keep a geometry in LDS that no longer fits.
    for (const void *fn : {(const void *)refine_winner_kernel<false>, (const void *)refspec_exact_kernel<false>}) {
        hipFuncAttributes fa{};
        RA_HIP(hipFuncGetAttributes(&fa, fn));
        if (fa.sharedSizeBytes > RA_EXACT_STATIC_LDS) {
            char buf[256];
            snprintf(buf, sizeof(buf), "the exact kernels have %zu bytes of static LDS, RA_EXACT_STATIC_LDS reserves %zu: update the reserve (ralign_exact.h)",
                     (size_t)fa.sharedSizeBytes, RA_EXACT_STATIC_LDS);
            g_last_error = buf;
            return RA_ERR_HIP;
        }
    }
    e->refine_gm = refine_rings_global(g, rq);
    e->refine_grid = e->refine_gm ? 256 : 2048;
    if (e->refine_gm) e->lds_refine = RA_EXACT_TABLE_BYTES(g.maxrin);
    std::vector<float> tw;
    std::vector<int> off(32, 0);
    for (int l = 1; (1 << l) <= g.maxrin; l++) {
        const int n = 1 << l, h = n / 2;
        off[l] = (int)tw.size();
        for (int k = 0; k < h; k++) {
            const double a = -2.0 * M_PI * k / n;
            tw.push_back((float)cos(a)); tw.push_back((float)sin(a));
        }
    }
    int rc;
    if ((rc = upload(e, tw, &e->d_twx)) || (rc = upload(e, off, &e->d_twxoff))) return rc;
    if ((rc = dev_alloc(e, &e->d_refx, (size_t)e->cfg.nref * g.lcirc, true)) ||
        (rc = dev_alloc(e, &e->d_rlist, (size_t)e->chunk, false)) || (e->rlist_cap = e->chunk, 0) ||
        (rc = dev_alloc(e, &e->d_rcount, 1, true)) ||
        (rc = dev_alloc(e, &e->d_refhash, (size_t)e->cfg.nref, true)) || (rc = dev_alloc(e, &e->d_refdup, (size_t)2 * e->cfg.nref, true))) return rc;
    if (e->refine_gm) {
        if ((rc = dev_alloc(e, &e->d_rscratch, (size_t)std::max(e->refine_grid, e->cfg.nref) * 2 * g.lcirc, false))) return rc;
        // the f64 twiddles and samples stay in LDS (24 maxrin bytes: 96 KB at maxrin 4096, beyond the 64 KB a kernel gets unasked)
        if ((rc = RA_LDS(e, refine_winner_kernel<true>, e->lds_refine))) return rc;
    } else {
        if ((rc = RA_LDS(e, refine_winner_kernel<false>, e->lds_refine)) || (rc = RA_LDS(e, refspec_exact_kernel<false>, e->lds_refine))) return rc;
    }
    e->refine_ok = true;
    return RA_OK;
}

// refine_winner_kernel over the refine list of cn particles, one image per workgroup (ring buffers in LDS, or -- refine_gm -- in the
// global scratch: setup_refine)
static int launch_refine_winner(ra_engine *e, int cn, float *st, ra_result *res, const float *part, const float *refx, const int *cls)
{
    const auto k = e->refine_gm ? refine_winner_kernel<true> : refine_winner_kernel<false>;
    hipLaunchKernelGGL(k, dim3(std::min(cn, e->refine_grid)), dim3(RA_EXACT_THREADS), e->lds_refine, e->stream, e->dg, (const int *)e->d_numr, (const float *)e->d_twx,
                       (const int *)e->d_twxoff, part, refx, (const RefineRec *)e->d_rlist, (const int *)e->d_rcount, res, cls, st, e->d_rscratch);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

// finalize + (flagged particles) refine of one chunk: `cand` records with `nrtile` per particle-offset.
// Chunked paths (kernel pair, size-generic kernels) call it with deferred = 1 for every chunk -- the flagged particles of the whole
// call collect in ONE list, indexed from the call's first particle (p_base = the chunk's offset; st / res / part are the chunk's) --
// and once more with deferred = 2 behind the last chunk (st / res / part the call's, cn its particle count): refine_winner_kernel
// handles one image per workgroup and a chunk flags ~10 of its 330 particles at configs[4], so a launch per chunk left the GPU to ten
// workgroups for 0.94 ms, 2.6 % of the iteration; one launch per call fills it.
static int finalize_and_refine(ra_engine *e, const CandT *cand, int nrtile, int cn, float *st, ra_result *res, const float *part,
                               const float *refx, const int *cls, int deferred = 0, int p_base = 0)
{
    const bool refine = e->refine_ok && e->refine_thr != 0.f && refx;
    if (refine && deferred == 0) RA_HIP(hipMemsetAsync(e->d_rcount, 0, sizeof(int), e->stream));
    if (deferred != 2) {
    if ((size_t)e->geo.nshift * nrtile >= 256)          // many records per particle: one wave each
        hipLaunchKernelGGL(finalize_wave_kernel, dim3(cn), dim3(64), 0, e->stream, e->dg, cand, nrtile, cn, st, res,
                           refine ? e->d_rlist : (RefineRec *)nullptr, e->d_rcount, e->refine_thr, p_base);
    else
        hipLaunchKernelGGL(finalize_kernel, dim3((cn + 127) / 128), dim3(128), 0, e->stream, e->dg, cand, nrtile, cn, st, res, (const float *)e->d_cs,
                           refine ? e->d_rlist : (RefineRec *)nullptr, e->d_rcount, e->refine_thr, p_base);
    RA_HIP(hipGetLastError());
    }
    if (refine && deferred != 1) return launch_refine_winner(e, cn, st, res, part, refx, cls);
    return RA_OK;
}

// One launch of a particle-resident kernel takes up to RA_RESIDENT_BATCH particles (cfg.chunk > 0: that many): every launch
// ends with a tail in which the CUs run dry one by one, ~1 % of a 7 000-particle launch (measured: 7 launches 30.9 ms, 5 launches
// 30.6 ms per 50 000 particles); its candidate records (2 KB per particle at 49 offsets) and the refine list grow on demand.
#define RA_RESIDENT_BATCH 131072
static int resident_batch(const ra_engine *e, int n)
{
    return std::max(1, std::min(n, e->cfg.chunk > 0 ? e->chunk : RA_RESIDENT_BATCH));
}
static int ensure_resident_ws(ra_engine *e, int cn)
{
    int rc;
    if (cn > e->fcand_cap) {
        if ((rc = dev_grow(e, &e->d_fcand, (size_t)cn * e->pad_cap + 8, true))) return rc;
        e->fcand_cap = cn;
    }
    if (e->refine_ok && cn > e->rlist_cap) {
        if ((rc = dev_grow(e, &e->d_rlist, (size_t)cn, false))) return rc;
        e->rlist_cap = cn;
    }
    return RA_OK;
}

// spectra workspace of the two-kernel path, allocated on first use (the fused kernel does not need it)
static int ensure_unfused_ws(ra_engine *e)
{
    if (e->unfused_ws) return RA_OK;
    int rc;
    if ((rc = dev_alloc(e, &e->d_A, e->wp.a_floats, true)) || (rc = dev_alloc(e, &e->d_cand, e->wp.cand_recs, true))) return rc;
    if (e->generic && (rc = dev_alloc(e, &e->d_zscr, e->wp.zscr_recs, false))) return rc;
    e->unfused_ws = true;
    return RA_OK;
}

// the LDS-resident kernels cover <= 48 rings of 8..256 samples and images whose padded copy plus four ring buffers
// fit one CU's LDS; everything else runs the size-generic kernels
static bool fits_specialised_kernels(const Geometry &g0, const ra_config &cfg, const PlanRequest &rq)
{
    bool fast = g0.nring <= 4 * RA_CCF_MAXNS && select_ccf(g0.maxrin) != nullptr && g0.numr[2] >= 8;
    const int bd0 = (int)std::ceil(std::max(cfg.xrng, cfg.yrng)) + 2, pst0 = g0.nx + 2 * bd0;
    const int sbuf0 = (g0.lring + 31) / 32 * 32 + 8;
    if ((size_t)(pst0 * pst0 + 4 * sbuf0 + 2 * g0.maxrin + 4096) * sizeof(float) > 160 * 1024) fast = false;
    int ncls = 0, prev = -1;
    for (int k = 0; k < g0.nbins; k++) {
        const int ns = (g0.bin_offp[k + 1] - g0.bin_offp[k]) / 4;
        if (ns != prev) { ncls++; prev = ns; }
    }
    if (ncls > 8) fast = false;
    if (rq.generic_forced()) fast = false;
    return fast;
}

static int create_engine(ra_engine **out, const ra_config *cfg, const ra_options *opt, const PlanRequest &rq);
extern "C" int ra_create(ra_engine **out, const ra_config *cfg) { return ra_create_ex(out, cfg, nullptr); }
extern "C" int ra_create_ex(ra_engine **out, const ra_config *cfg, const ra_options *opt)
{
    if (opt && (opt->interp != RA_INTERP_BILINEAR && opt->interp != RA_INTERP_QUADRI)) { g_last_error = "bad interpolation"; return RA_ERR_ARG; }
    if (opt && (opt->normalize_ring < -1 || opt->normalize_ring > 1)) { g_last_error = "normalize_ring is -1 (by mode), 0 or 1"; return RA_ERR_ARG; }
    const PlanRequest rq{read_switches(), opt && opt->interp == RA_INTERP_QUADRI, false, true};
    int rc = create_engine(out, cfg, opt, rq);
    // the plan of the four-offset kernels over a crop of the image is promised by tcrop_wanted on an estimate of the tables; should
    // the real tables miss it, the engine is planned again without that path (pair or generic kernels) instead of failing
    if (rc == RA_ERR_STATE) {
        PlanRequest no_crop = rq;
        no_crop.allow_tcrop = false;
        rc = create_engine(out, cfg, opt, no_crop);
    }
    // More than 16 references in a box whose image fits the LDS but leaves no room for the tiled kernel's plan beside it (100 - 128
    // pixels at ou = 21 .. 32) used to fall to the round-1 kernel pair (3.7 MB of HBM per particle): planned in the size-generic
    // class instead, the search runs search_tiled_kernel over a crop of the image.  Kept only when that plan exists.
    if (rc == RA_OK && *out && !(*out)->generic && !(*out)->fused && cfg->nref > RF_MAXREF && (*out)->geo.maxrin == 256 && !rq.generic_forced() &&
        rq.sw.fused) {          // (RALIGN_FUSED=0 asks for the kernel pair)
        ra_engine *alt = nullptr;
        PlanRequest in_class = rq;
        in_class.generic_class = true;
        const int rc2 = create_engine(&alt, cfg, opt, in_class);
        if (rc2 == RA_OK && alt && (alt->fused || alt->solo)) { ra_destroy(*out); *out = alt; }
        else if (alt) ra_destroy(alt);
    }
    return rc;
}
static int create_engine(ra_engine **out, const ra_config *cfg, const ra_options *opt, const PlanRequest &rq)
{
    if (!out || !cfg) { g_last_error = "null argument"; return RA_ERR_ARG; }
    *out = nullptr;
    if (cfg->nx < 8 || cfg->nref < 1 || cfg->nref > 65535) { g_last_error = "bad nx/nref"; return RA_ERR_ARG; }
    // "Shift or radius is too large - particle crosses image boundary" (test_mref_gpu_align.py:314)
    if (cfg->last_ring + std::max(cfg->xrng, cfg->yrng) > (float)((cfg->nx - 1) / 2)) {
        g_last_error = "shift or radius too large: particle crosses image boundary";
        return RA_ERR_ARG;
    }
    if (cfg->mode != RA_MODE_MREF && cfg->mode != RA_MODE_REFFREE) { g_last_error = "bad mode"; return RA_ERR_ARG; }
    int ndev = 0;
    RA_HIP(hipGetDeviceCount(&ndev));
    if (cfg->device < 0 || cfg->device >= ndev) { g_last_error = "no such HIP device"; return RA_ERR_HIP; }
    RA_HIP(hipSetDevice(cfg->device));

    ra_engine *e = new ra_engine();
    e->cfg = *cfg;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0) e->n_cu = prop.multiProcessorCount;
        if (rq.sw.grid > 0) e->n_cu = rq.sw.grid;      // experiments: fewer persistent workgroups
    }
    if (!build_rings(e->geo, cfg->nx, cfg->first_ring, cfg->last_ring, cfg->ring_skip > 0 ? cfg->ring_skip : 1) ||
        !build_shifts(e->geo, cfg->xrng, cfg->yrng, cfg->step)) {
        g_last_error = "bad ring / shift geometry";
        delete e;
        return RA_ERR_ARG;
    }
    e->force_generic = rq.option_generic;
    e->generic = !fits_specialised_kernels(e->geo, *cfg, rq) || rq.generic_class;
    e->tcrop = tcrop_wanted(e, rq);
    if (!e->tcrop && rq.allow_tcrop && e->generic && e->geo.maxrin == 256 && rq.sw.tight_rings) {
        // ou = 37 ... 40: crop + four ring buffers miss the LDS by 4 - 8 KB, of which the 16 padding floats per ring are 10 KB.  With
        // rings 4 floats apart (the in-place real transform needs 2; 4 keeps every ring 16-byte aligned) the four-offset kernels take
        // the class from the pair kernel (RALIGN_TIGHT_RINGS=0: the pair kernel)
        // (RALIGN_TIGHT_RINGS is on / off like every other switch; the distance itself is an experiment of profiling builds,
        // RALIGN_RING_PAD: multiples of 4 only -- 2 would leave the rings 8-byte aligned, a layout no test covers)
        int pad = 4;
        if (const char *rp = RA_EXP_ENV("RALIGN_RING_PAD")) { const int v = atoi(rp); if (v >= 4 && v % 4 == 0 && v < kRingPad) pad = v; }
        Geometry g16 = e->geo, g4;
        if (build_rings(g4, cfg->nx, cfg->first_ring, cfg->last_ring, cfg->ring_skip > 0 ? cfg->ring_skip : 1, pad) &&
            build_shifts(g4, cfg->xrng, cfg->yrng, cfg->step)) {
            e->geo = g4;
            e->tcrop = tcrop_wanted(e, rq);
            if (!e->tcrop) e->geo = g16;
        }
    }
    e->crop_S = (int)std::ceil(std::max(e->geo.nkx, e->geo.nky) * e->geo.step - 1e-6);
    if (e->generic && e->geo.maxrin <= 1024 && !(RA_EXP_ENV("RALIGN_QUAD_ALIGN") && ra_atoi(RA_EXP_ENV("RALIGN_QUAD_ALIGN")) == 0)) align_ring_quads(e->geo);
    if (e->geo.maxrin > 4096) {
        g_last_error = "rings longer than 4096 samples are not supported";
        delete e;
        return RA_ERR_ARG;
    }
    e->nrtile = (cfg->nref + 7) / 8;
    e->dg.rpt = (cfg->nref + e->nrtile - 1) / e->nrtile;      // balanced reference tiles (10 -> 5 + 5)
    decide_class(e, rq);
    int rc = build_device_geometry(e, rq);
    if (rc) { ra_destroy(e); return rc; }
    if (opt) {
        e->dg.interp = opt->interp;
        if (opt->normalize_ring >= 0) e->dg.norm_ring = opt->normalize_ring;
    }

    e->shift_cap = e->geo.nshift; e->pad_cap = e->geo.nshift_pad;
    const Geometry &g = e->geo;
    const int npix_pad = (g.nx * g.nx + 3) & ~3;
    e->lds_polar = (size_t)(((e->dg.pst * e->dg.pst + 3) & ~3) + 4 * e->dg.sbuf + 2 * g.maxrin + 2 * e->dg.n_qtab + 2 + 5 * e->dg.n_inst +
                            4 * e->dg.n_job + 32 + 8 * g.nring) * sizeof(float);
    e->lds_ref = (size_t)(npix_pad + e->dg.sbuf + 8) * sizeof(float);
    e->lds_ccf = (size_t)64 * (2 * (g.maxrin + g.maxrin / 16) + 2) * sizeof(float);
    const size_t lds_max = 160 * 1024;
    if (!e->generic && (e->lds_polar > lds_max || e->lds_ccf > lds_max)) {
        g_last_error = "image / ring geometry does not fit the 160 KB LDS of one CU";
        ra_destroy(e);
        return RA_ERR_ARG;
    }
    // generic contraction: P pairs per inverse-FFT batch, two N-point buffers per pair
    e->g_P = 64;
    while (e->g_P > 1 && (size_t)e->g_P * (g.maxrin + 1) * sizeof(float2) > 66 * 1024) e->g_P >>= 1;      // two workgroups per CU
    e->lds_gccf = ((size_t)e->g_P * (g.maxrin + 1) + g.maxrin) * sizeof(float2);      // pair buffers (in-place transforms) + twiddle table
    e->lds_gpolar = ((size_t)(RA_GEN_THREADS / 64 + 1) * g.maxrin + e->dg.n_qtab) * sizeof(float2);      // per-wave ring buffers + twiddle table + (sinf, cosf) tables
    if (!e->generic) {
        if (!rc) rc = RA_LDS(e, polar_fft_kernel, e->lds_polar);
        if (!rc) rc = RA_LDS(e, ref_polar_fft_kernel, e->lds_ref);
        e->ccf = select_ccf(g.maxrin);
        if (!rc) rc = raise_dynamic_lds(e, (const void *)e->ccf, "ccf_kernel", e->lds_ccf);
    } else {
        if (!rc) rc = raise_dynamic_lds(e, (const void *)gpolar_kernel(e, false), "polar_generic_kernel<false>", e->lds_gpolar);
        if (!rc) rc = raise_dynamic_lds(e, (const void *)gpolar_kernel(e, true), "polar_generic_kernel<true>", e->lds_gpolar);
        if (!rc) rc = raise_dynamic_lds(e, (const void *)ccf_generic_kernel<2, 2>, "ccf_generic_kernel<2, 2>", e->lds_gccf);
        if (!rc) rc = raise_dynamic_lds(e, (const void *)ccf_generic_kernel<1, 7>, "ccf_generic_kernel<1, 7>", e->lds_gccf);
        if (!rc) rc = raise_dynamic_lds(e, (const void *)ccf_generic_kernel<2, 7>, "ccf_generic_kernel<2, 7>", e->lds_gccf);
        if (g.maxrin == 1024) {
            const size_t lds2 = gccf_shape(e->nrtile, g.maxrin, true, 0).lds_ifft;
            if (!rc) rc = raise_dynamic_lds(e, (const void *)gccf_ifft_kernel<1, 7>, "gccf_ifft_kernel<1, 7>", lds2);
            if (!rc) rc = raise_dynamic_lds(e, (const void *)gccf_ifft_kernel<2, 2>, "gccf_ifft_kernel<2, 2>", lds2);
            if (!rc) rc = raise_dynamic_lds(e, (const void *)gccf_ifft_kernel<2, 7>, "gccf_ifft_kernel<2, 7>", lds2);
            if (!rc) rc = raise_dynamic_lds(e, (const void *)gccf_ifft_kernel<4, 7>, "gccf_ifft_kernel<4, 7>", lds2);
        }
    }
    if (!rc && xf_in_lds(g.nx)) rc = RA_LDS(e, transform_kernel, xf_lds_bytes(g.nx));
    if (!rc) rc = RA_LDS(e, class_sum_kernel, (size_t)160 * 1024 - 64);
    if (rc) { ra_destroy(e); return rc; }

    // workspace.  The spectra panels and candidate records of the two-kernel path are allocated on first use only
    // (ensure_unfused_ws); the fused kernel needs candidate records alone.
    const WorkspacePlan wp = plan_workspace(g, *cfg, rq, e->generic);
    e->wp = wp;
    e->chunk = wp.chunk;
    if ((rc = dev_alloc(e, &e->d_refspec, wp.refspec_floats, true)) ||
        (rc = dev_alloc(e, &e->d_B, wp.b_floats, true)) ||
        (rc = dev_alloc(e, &e->d_cs, 2, true)) ||
        (rc = dev_alloc(e, &e->d_fcand, (size_t)wp.chunk * g.nshift_pad + 8, true))) {
        ra_destroy(e);
        return rc;
    }
    e->fcand_cap = wp.chunk;
    if (e->generic) {
        if ((rc = dev_alloc(e, &e->d_gstats, (size_t)wp.chunk * g.nshift_pad + 8, true)) ||
            (rc = dev_alloc(e, &e->d_gcdc, (size_t)cfg->nref, true))) { ra_destroy(e); return rc; }
    }
    if ((rc = setup_fused(e, rq))) { ra_destroy(e); return rc; }
    if ((rc = setup_solo(e, rq))) { ra_destroy(e); return rc; }
    if ((rc = setup_zones(e, rq))) { ra_destroy(e); return rc; }
    if ((rc = update_live_mode(e, rq))) { ra_destroy(e); return rc; }
    if ((rc = setup_refine(e, rq))) { ra_destroy(e); return rc; }
    e->atomic_sums = rq.sw.atomic_sums;
    *out = e;
    return RA_OK;
}

extern "C" void ra_destroy(ra_engine *e)
{
    if (!e) return;
    (void)hipSetDevice(e->cfg.device);
    (void)hipDeviceSynchronize();
#ifdef RALIGN_PROFILE_SWITCHES
    if (e->d_timeline && RA_EXP_ENV("RALIGN_TIMELINE")) {      // profiling builds: dump the wave timeline of the last launch
        std::vector<unsigned long long> h(64 * 16 * 16);
        (void)hipDeviceSynchronize();
        if (hipMemcpy(h.data(), e->d_timeline, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost) == hipSuccess) {
            if (FILE *fp = fopen(RA_EXP_ENV("RALIGN_TIMELINE"), "wb")) { fwrite(h.data(), sizeof(unsigned long long), h.size(), fp); fclose(fp); }
        }
        (void)hipFree(e->d_timeline);
    }
#endif
    if (e->d_cls_refspec) (void)hipFree(e->d_cls_refspec);
    if (e->d_cls_Bf) (void)hipFree(e->d_cls_Bf);
    if (e->d_cls_refx) (void)hipFree(e->d_cls_refx);
    for (void *p : e->owned) (void)hipFree(p);
    for (auto &pr : e->ev_ccf) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto &pr : e->ev_polar) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    delete e;
}

extern "C" int ra_set_stream(ra_engine *e, void *hip_stream)
{
    if (!e) return RA_ERR_ARG;
    e->stream = (hipStream_t)hip_stream;
    return RA_OK;
}

extern "C" int ra_set_mask(ra_engine *e, const float *d_mask)
{
    if (!e || !d_mask) { g_last_error = "null argument"; return RA_ERR_ARG; }
    RA_HIP(hipMemcpyAsync((void *)e->dg.mask, d_mask, (size_t)e->geo.nx * e->geo.nx * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return RA_OK;
}

extern "C" int ra_set_normalize_ring(ra_engine *e, int flag)
{
    if (!e) return RA_ERR_ARG;
    e->dg.norm_ring = flag < 0 ? (e->cfg.mode == RA_MODE_MREF ? 1 : 0) : flag ? 1 : 0;
    return RA_OK;
}
extern "C" int ra_get_options(const ra_engine *e, ra_options *opt)
{
    if (!e || !opt) return RA_ERR_ARG;
    opt->interp = e->dg.interp; opt->normalize_ring = e->dg.norm_ring;
    return RA_OK;
}

extern "C" int ra_set_nomirror(ra_engine *e, int flag)
{
    if (!e) return RA_ERR_ARG;
    e->dg.nomirror = flag ? 1 : 0;
    return RA_OK;
}
extern "C" int ra_set_refine(ra_engine *e, float threshold)
{
    if (!e) return RA_ERR_ARG;
    e->refine_thr = threshold;
    e->refs_ready = false;             // the exact reference spectra are prepared by ra_set_references when the refinement is on
    e->cls_ready = 0;                  // ... and those of the class-resident mode by ra_set_class_references
    return e->refine_ok || threshold == 0.f ? RA_OK : RA_ERR_STATE;
}
// particles the last search launch handed to refine_winner_kernel (flat peaks and float ties); synchronises the stream
extern "C" int ra_last_refine_count(ra_engine *e)
{
    if (!e) return RA_ERR_ARG;
    if (!e->refine_ok || !e->d_rcount) return 0;
    int h = 0;
    if (hipStreamSynchronize(e->stream) != hipSuccess || hipMemcpy(&h, e->d_rcount, sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) return RA_ERR_HIP;
    return h;
}
// the LDS ledger: every kernel whose dynamic LDS this engine raised, with the static LDS of the loaded code object
extern "C" int ra_lds_report(const ra_engine *e, ra_lds_row *rows, int cap)
{
    if (!e || cap < 0 || (cap > 0 && !rows)) return RA_ERR_ARG;
    const int n = (int)e->lds_rows.size();
    for (int i = 0; i < std::min(n, cap); i++) {
        const LdsRow &r = e->lds_rows[i];
        snprintf(rows[i].kernel, sizeof(rows[i].kernel), "%s", r.kernel.c_str());
        rows[i].static_bytes = r.stat; rows[i].dynamic_bytes = r.dyn; rows[i].limit_bytes = r.limit;
    }
    return n;
}
extern "C" int ra_search_tiled(const ra_engine *e) { return !e ? RA_ERR_ARG : (e->fused && e->tiled) ? 1 : 0; }
// the containment rule of ra_search_l1_tap_rings without an engine or a device: l1_tap_rings (ralign_plan.h) on the rings of the
// geometry, whatever kernel family and reference count an engine would have
extern "C" int ra_l1_tap_rule(int nx, int first_ring, int last_ring, int ring_skip, float xrng, float yrng)
{
    Geometry g;
    if (nx < 1 || !build_rings(g, nx, first_ring, last_ring, ring_skip > 0 ? ring_skip : 1) || xrng < 0.f || yrng < 0.f) {
        g_last_error = "bad ring or window arguments";
        return RA_ERR_ARG;
    }
    return l1_tap_rings(g.numr, g.nring, nx, last_ring, xrng, yrng);
}
extern "C" int ra_search_l1_tap_rings(const ra_engine *e) { return !e ? RA_ERR_ARG : (e->fused && !e->tiled) ? e->fplan.tap_l1 : 0; }
extern "C" int ra_search_path(const ra_engine *e) { return !e ? RA_ERR_ARG : e->solo ? 3 : e->fused ? 1 : e->generic ? 2 : 0; }
extern "C" int ra_search_offsets_per_pass(const ra_engine *e) { return !e ? RA_ERR_ARG : !e->solo ? 0 : (e->duo || e->pair) ? 2 : 1; }
extern "C" int ra_search_skips_offsets(const ra_engine *e) { return !e ? RA_ERR_ARG : (e->solo || e->dg.ent_base) ? 1 : 0; }
extern "C" int ra_num_shifts(const ra_engine *e) { return e ? e->geo.nshift : RA_ERR_ARG; }
extern "C" int ra_maxrin(const ra_engine *e) { return e ? e->geo.maxrin : RA_ERR_ARG; }
extern "C" int ra_lcirc(const ra_engine *e) { return e ? e->geo.lcirc : RA_ERR_ARG; }

extern "C" int ra_reset_shifts(ra_engine *e, float xrng, float yrng, float step)
{
    if (!e) return RA_ERR_ARG;
    const PlanRequest rq{read_switches(), e->force_generic, false, false};      // (generic class and crop were decided at create: e->generic, e->tcrop)
    Geometry g2 = e->geo;
    if (!build_shifts(g2, xrng, yrng, step)) { g_last_error = "bad shift window"; return RA_ERR_ARG; }
    // the reference asserts the offset count does not change (gpu_aln_noref.cu:135); we only
    // require that it does not exceed what ra_create sized
    if (g2.nshift_pad > e->pad_cap || g2.nshift > e->shift_cap) {
        g_last_error = "reset_shifts: more search offsets than the engine was created with";
        return RA_ERR_ARG;
    }
    if ((float)e->cfg.last_ring + std::max(xrng, yrng) > (float)((e->cfg.nx - 1) / 2)) {
        g_last_error = "shift or radius too large: particle crosses image boundary";
        return RA_ERR_ARG;
    }
    // the padded LDS image of the polar stage was sized at ra_create for a border of ceil(max range) + 2 pixels;
    // a wider window (possible at a constant offset count, e.g. xr=1,ts=0.5 -> xr=4,ts=2) would let taps leave it
    if (!e->generic && (int)std::ceil(std::max(xrng, yrng)) + 2 > e->dg.bd) {
        g_last_error = "reset_shifts: search range exceeds the image border the engine was created with";
        return RA_ERR_ARG;
    }
    if (e->tcrop && (int)std::ceil(std::max(g2.nkx, g2.nky) * g2.step - 1e-6) > e->crop_S) {
        g_last_error = "reset_shifts: search range exceeds the image crop the engine was created with";
        return RA_ERR_ARG;
    }
    RA_HIP(hipStreamSynchronize(e->stream));
    RA_HIP(hipMemcpy((void *)e->dg.shift_x, g2.shift_x.data(), g2.nshift * sizeof(float), hipMemcpyHostToDevice));
    RA_HIP(hipMemcpy((void *)e->dg.shift_y, g2.shift_y.data(), g2.nshift * sizeof(float), hipMemcpyHostToDevice));
    e->geo.nkx = g2.nkx; e->geo.nky = g2.nky; e->geo.nshift = g2.nshift; e->geo.step = g2.step;
    e->geo.shift_x = g2.shift_x; e->geo.shift_y = g2.shift_y;
    e->geo.nshift_pad = g2.nshift_pad;
    e->cfg.xrng = xrng; e->cfg.yrng = yrng; e->cfg.step = step;
    e->dg.nkx = g2.nkx; e->dg.nky = g2.nky; e->dg.nshift = g2.nshift; e->dg.nshift_pad = g2.nshift_pad; e->dg.ent_stride = e->generic ? g2.nshift : g2.nshift_pad;
    e->dg.step = step; e->dg.xrng = xrng; e->dg.yrng = yrng;
    decide_class(e, rq);
    int rc = setup_fused(e, rq);
    // the solo / duo / pair kernels keep a crop of the image whose side follows the search range: plan again (a wider range at a
    // constant offset count, e.g. xr = 1, ts = 0.5 -> xr = 4, ts = 2, would otherwise let taps leave the crop)
    // (also when the previous window made the plan fall back to the generic kernels: the new one may fit again)
    if (!rc && e->generic && !e->fused && (e->solo || e->want.solo || e->want.pair)) rc = setup_solo(e, rq);
    if (!rc) rc = setup_zones(e, rq);        // the zones' annuli follow the search range
    if (!rc) rc = update_live_mode(e, rq);   // (the plan may have moved between the particle-resident and the size-generic kernels)
    return rc;
}

// refspec_exact_kernel: the spectra of `count` images with the CPU path's arithmetic into out [count][lcirc]; with global ring buffers (refine_gm)
// as many images per launch as the scratch has blocks
static int launch_refspec_exact(ra_engine *e, const float *d_imgs, int count, float *out)
{
    const auto k = e->refine_gm ? refspec_exact_kernel<true> : refspec_exact_kernel<false>;
    const int cap = e->refine_gm ? std::max(e->refine_grid, e->cfg.nref) : count;
    for (int c0 = 0; c0 < count; c0 += cap) {
        const int cnt = std::min(cap, count - c0);
        hipLaunchKernelGGL(k, dim3(cnt), dim3(RA_EXACT_THREADS), e->refine_gm ? 0 : e->lds_refine, e->stream, e->dg, (const int *)e->d_numr, (const float *)e->d_wr,
                           (const float *)e->d_twx, (const int *)e->d_twxoff, d_imgs + (size_t)c0 * e->geo.nx * e->geo.nx, cnt, out + (size_t)c0 * e->geo.lcirc,
                           e->d_rscratch);
    }
    RA_HIP(hipGetLastError());
    return RA_OK;
}

extern "C" int ra_set_references(ra_engine *e, const float *d_refs)
{
    if (!e || !d_refs) { g_last_error = "null argument"; return RA_ERR_ARG; }
    const Geometry &g = e->geo;
    if (e->generic)
        hipLaunchKernelGGL(gpolar_kernel(e, true), dim3(e->cfg.nref), dim3(RA_GEN_THREADS), e->lds_gpolar, e->stream, e->dg,
                           d_refs, (const float *)nullptr, e->cfg.nref, e->d_refspec, (float2 *)nullptr);
    else
        hipLaunchKernelGGL(ref_polar_fft_kernel, dim3(e->cfg.nref), dim3(256), e->lds_ref, e->stream, e->dg, d_refs,
                           e->cfg.nref, e->d_refspec);
    RA_HIP(hipGetLastError());
    int total = e->nrtile * g.LBP * 16;
    hipLaunchKernelGGL(pack_refs_kernel, dim3((total + 255) / 256), dim3(256), 0, e->stream, e->dg, e->d_refspec,
                       e->cfg.nref, e->nrtile, e->d_B);
    RA_HIP(hipGetLastError());
    if (e->d_Bf) {      // the fused kernel's stream does not depend on the search window: keep it current
        FusedGeom f = e->fplan.f;
        if (f.b_floats > 0 && f.bsrc) {
            hipLaunchKernelGGL(pack_refs_fused_kernel, dim3(std::min(2048, (f.b_floats + 255) / 256)), dim3(256), 0, e->stream, e->dg, f,
                               e->d_refspec, e->cfg.nref, e->d_Bf);
            RA_HIP(hipGetLastError());
        }
    }
    if (e->refine_ok && e->refine_thr != 0.f) {        // the same references with the CPU path's arithmetic, for the sub-bin angle refinement
        if (const int rc = launch_refspec_exact(e, d_refs, e->cfg.nref, e->d_refx)) return rc;      // (one launch: the scratch holds nref images)
        // copies of a reference inside the stack: their CCFs are equal to the bit and the CPU scan alone decides among them
        hipLaunchKernelGGL(ref_hash_kernel, dim3(e->cfg.nref), dim3(256), 0, e->stream, (const float *)e->d_refx, g.lcirc, e->d_refhash);
        hipLaunchKernelGGL(ref_groups_kernel, dim3(1), dim3(256), 0, e->stream, (const float *)e->d_refx, g.lcirc, e->cfg.nref,
                           (const unsigned long long *)e->d_refhash, e->d_refdup);
        RA_HIP(hipGetLastError());
        e->dg.ref_dup = e->d_refdup;
    } else e->dg.ref_dup = nullptr;
    if (e->generic || e->fused) {
        hipLaunchKernelGGL(ref_dc_weights_kernel, dim3((e->cfg.nref + 63) / 64), dim3(64), 0, e->stream, e->dg, e->d_refspec, e->cfg.nref, e->d_gcdc);
        RA_HIP(hipGetLastError());
    }
    e->refs_ready = true;
    return RA_OK;
}

extern "C" int ra_get_prepared_references(ra_engine *e, float *h_crefim)
{
    if (!e || !h_crefim) return RA_ERR_ARG;
    if (!e->refs_ready) { g_last_error = "ra_set_references has not been called"; return RA_ERR_STATE; }
    float *d_out = nullptr;
    size_t cnt = (size_t)e->cfg.nref * e->geo.lcirc;
    RA_HIP(hipMalloc((void **)&d_out, cnt * sizeof(float)));
    hipLaunchKernelGGL(unpack_refs_kernel, dim3(e->cfg.nref), dim3(256), 0, e->stream, e->dg, e->d_refspec,
                       e->cfg.nref, e->d_ring_off, e->d_numr, e->d_wr, d_out);
    hipError_t he = hipStreamSynchronize(e->stream);
    if (he == hipSuccess) he = hipMemcpy(h_crefim, d_out, cnt * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    RA_HIP(he);
    return RA_OK;
}

static std::pair<hipEvent_t, hipEvent_t> *next_events(std::vector<std::pair<hipEvent_t, hipEvent_t>> &pool, size_t &used)
{
    if (used == pool.size()) {
        hipEvent_t a, b;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return nullptr;
        pool.push_back({a, b});
    }
    return &pool[used++];
}

// The particle-resident search of n particles with the engine's stored kernel (solo, duo, pair, fused or tiled, over a crop or not,
// class-resident): launches of up to resident_batch particles -- a launch stays a bounded unit of work (timing, candidate
// workspace) -- with one persistent workgroup per CU (its LDS plan fills the CU) that walks over its share, each followed by its
// finalize and refine.  f: the plan's geometry as this launch wants it (FusedGeom::pack); pack: search_fused_kernel's dense-offset
// variant (pack_ok); B / nref_b: the reference stream and the references in one stream; refx: their exact spectra; d_cls: the class
// of every particle, one stream per class (ra_align_classes), or null
static int resident_search(ra_engine *e, const FusedGeom &f, bool pack, const float *B, int nref_b, const float *refx, const float *d_particles,
                           int n, float *d_state, ra_result *d_result, const int *d_cls)
{
    const SearchPlan &sp = e->search;
    const int npix = e->geo.nx * e->geo.nx, rch = resident_batch(e, n);
    if (const int rc = ensure_resident_ws(e, rch)) return rc;
    for (int start = 0; start < n; start += rch) {
        const int cn = std::min(rch, n - start);
        const float *part = d_particles + (size_t)start * npix;
        float *st = d_state + (size_t)start * 2;
        const int *cls = d_cls ? d_cls + start : nullptr;
        const dim3 grid(std::min(cn, e->n_cu)), block(RF_THREADS);
        std::pair<hipEvent_t, hipEvent_t> *evc = e->timing ? next_events(e->ev_ccf, e->ev_used_ccf) : nullptr;
        if (evc) RA_HIP(hipEventRecord(evc->first, e->stream));
        if (sp.solo)
            hipLaunchKernelGGL(sp.solo, grid, block, sp.lds, e->stream, e->dg, f, part, (const float *)st, cn, B, nref_b, e->d_fcand, (float *)nullptr);
        else
            hipLaunchKernelGGL(pack ? sp.pack : sp.fused, grid, block, sp.lds, e->stream, e->dg, f, part, (const float *)st, cn, B, nref_b, e->d_fcand, cls);
        RA_HIP(hipGetLastError());
        if (evc) RA_HIP(hipEventRecord(evc->second, e->stream));
        if (const int rc = finalize_and_refine(e, e->d_fcand, 1, cn, st, d_result + start, part, refx, cls)) return rc;
    }
    return RA_OK;
}

// Polar2Dm + Normalize_ring statistics + Frngs of `cn` particles into the A blocks / d_gstats of the size-generic path
static int launch_generic_polar(ra_engine *e, const float *part, const float *st, int cn, float *Abuf)
{
    const Geometry &g = e->geo;
    if (e->dg.ent_base) {
        hipLaunchKernelGGL(live_scan_kernel, dim3(1), dim3(1024), 0, e->stream, e->dg, st, cn, e->d_ent_base, e->d_ent_total);
        RA_HIP(hipGetLastError());
    }
    if (e->zones) {
        hipLaunchKernelGGL(polar_zone_kernel<RA_ZONE_NW>, dim3((unsigned)cn * e->zdev.nzone * e->zdev.nchunk), dim3(64 * RA_ZONE_NW), e->zplan.lds_bytes, e->stream,
                           e->dg, e->zdev, part, st, cn, Abuf, e->d_stats_part);
        RA_HIP(hipGetLastError());
        const int nent = cn * e->dg.ent_stride;
        hipLaunchKernelGGL(polar_stats_kernel, dim3((nent + 255) / 256), dim3(256), 0, e->stream, e->dg, (const float2 *)e->d_stats_part, nent,
                           e->zdev.nquad_total, e->d_gstats);
    } else
        hipLaunchKernelGGL(gpolar_kernel(e, false), dim3((unsigned)(((long long)cn * e->dg.ent_stride + 3) / 4)), dim3(RA_GEN_THREADS), e->lds_gpolar, e->stream, e->dg,
                           part, st, cn, Abuf, e->d_gstats);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

// Crosrng_ms of n_mtile tiles of 8 particle-offsets against every reference tile, best reference per tile to Cbuf (the size-generic
// path).  split / tm: RALIGN_GCCF_SPLIT at maxrin 1024 and RALIGN_GCCF_TM, as the caller reads them at the launch (gccf_shape)
static int launch_contraction(ra_engine *e, const float *Abuf, CandT *Cbuf, int n_mtile, bool split, int tm)
{
    const GccfShape gs = gccf_shape(e->nrtile, e->geo.maxrin, split, tm);
    hipStream_t sp = e->stream;
    if (!split) {
        const auto k = gs.TR == 2 ? ccf_generic_kernel<2, 2> : gs.TM == 2 ? ccf_generic_kernel<2, 7> : ccf_generic_kernel<1, 7>;
        hipLaunchKernelGGL(k, dim3(std::min((n_mtile + gs.TM - 1) / gs.TM, gs.nwg)), dim3(RA_GCCF_THREADS), e->lds_gccf, sp, e->dg, Abuf, (const float *)e->d_B,
                           n_mtile, e->nrtile, e->cfg.nref, Cbuf, e->d_zscr, e->g_P, (const float2 *)e->d_gstats, (const float *)e->d_gcdc, 0, 0);
        RA_HIP(hipGetLastError());
        return RA_OK;
    }
    // contraction and inverse transforms as two kernels per slice of nblk blocks (the scratch holds one slice)
    const int ntask = (int)gs.blocks(n_mtile, e->nrtile);
    auto launch = [&](auto ccfk, auto ifftk, int task0, int nt, int grid2) {
        hipLaunchKernelGGL(ccfk, dim3(std::min(nt, gs.nwg)), dim3(RA_EXP_ENV("RALIGN_GCCF_WAVES") ? 64 * std::max(1, std::min(8, ra_atoi(RA_EXP_ENV("RALIGN_GCCF_WAVES")))) : RA_GCCF_THREADS), 0, sp, e->dg, Abuf, e->d_B, n_mtile, e->nrtile, e->cfg.nref, Cbuf,
                           e->d_zscr, e->g_P, (const float2 *)e->d_gstats, (const float *)e->d_gcdc, task0, nt);
        if (!(e->dg.dbg & 1))          // (profiling builds, RALIGN_DEBUG=1: the contraction alone)
        hipLaunchKernelGGL(ifftk, dim3(grid2), dim3(RA_GCCF_THREADS), gs.lds_ifft, sp, e->dg, n_mtile, e->nrtile, e->cfg.nref, Cbuf,
                           (const float2 *)e->d_zscr, (const float2 *)e->d_gstats, task0, nt);
    };
    for (int task0 = 0; task0 < ntask; task0 += gs.nblk) {
        const int nt = std::min(gs.nblk, ntask - task0);
        const int grid2 = std::min(nt * gs.TM * gs.TR * 8, (RA_EXP_ENV("RALIGN_IFFT_WGS") ? ra_atoi(RA_EXP_ENV("RALIGN_IFFT_WGS")) : 2) * e->n_cu);
        if (gs.TM == 4) launch(ccf_generic_kernel<4, 7, true>, gccf_ifft_kernel<4, 7>, task0, nt, grid2);
        else if (gs.TR == 7 && gs.TM == 2) launch(ccf_generic_kernel<2, 7, true>, gccf_ifft_kernel<2, 7>, task0, nt, grid2);
        else if (gs.TR == 7) launch(ccf_generic_kernel<1, 7, true>, gccf_ifft_kernel<1, 7>, task0, nt, grid2);
        else launch(ccf_generic_kernel<2, 2, true>, gccf_ifft_kernel<2, 2>, task0, nt, grid2);
        RA_HIP(hipGetLastError());
    }
    return RA_OK;
}

// average-centre correction of ali2d_single_iter: d += R(-alpha) M cs using the previous
// parameters (combine_params2(alpha,sx,sy,mirror, 0,-cs0,-cs1,0) then inverse_transform2)
__global__ void apply_cs_kernel(int n, const float *__restrict__ cs, const ra_result *__restrict__ res,
                                float *__restrict__ state)
{
    int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    double a = (double)res[p].alpha * M_PI / 180.0, c = cos(a), s = sin(a);
    double u = res[p].mirror ? -(double)cs[0] : (double)cs[0], v = (double)cs[1];
    state[2 * p] = (float)((double)state[2 * p] + c * u - s * v);
    state[2 * p + 1] = (float)((double)state[2 * p + 1] + s * u + c * v);
}

// The reference's state round trip (test_mref_gpu_align.py:1024-1026; ali2d_single_iter behind test_reffree_gpu_align.py:844-847):
// the shift a search starts from is rebuilt from the float32 header values (alpha, sx, sy[, mirror]) of the previous
// iteration -- inverse_transform2(alpha, sx, sy) for mref_ali2d, combine_params2(alpha, sx, sy, mirror, 0, -cs0, -cs1, 0)
// then inverse_transform2 for ali2d -- in double, EMAN2 Transform algebra v' = M (R(alpha) v + t), and rounded to float32
// once.  Algebraically d_old + (ix, iy) (what ra_align leaves in d_state); numerically e.g. -6.9999995, which decides
// edge-limited windows (particle_window) the way the reference's loop does.
__device__ __forceinline__ void tf_build_d(double a_deg, double tx, double ty, int m, double T[3][3])
{
    const double a = a_deg * M_PI / 180.0, c = cos(a), s = sin(a), sgn = m ? -1.0 : 1.0;
    T[0][0] = sgn * c; T[0][1] = sgn * s; T[0][2] = sgn * tx;
    T[1][0] = -s; T[1][1] = c; T[1][2] = ty;
    T[2][0] = 0; T[2][1] = 0; T[2][2] = 1;
}
__device__ __forceinline__ void tf_params_d(const double T[3][3], double out[4])
{
#pragma clang fp contract(off)
    const double det = T[0][0] * T[1][1] - T[0][1] * T[1][0];
    const int m = det < 0;
    const double sgn = m ? -1.0 : 1.0, c = sgn * T[0][0], s = sgn * T[0][1];
    double alpha = atan2(s, c) * 180.0 / M_PI;
    alpha = fmod(alpha, 360.0);
    if (alpha < 0) alpha += 360.0;
    if (alpha >= 360.0) alpha -= 360.0;
    out[0] = alpha; out[1] = sgn * T[0][2]; out[2] = T[1][2]; out[3] = m;
}
__global__ void state_from_params_kernel(int n, int mode, const float *__restrict__ cs, const ra_result *__restrict__ res,
                                         float *__restrict__ state)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    double A[3][3], B[3][3], C[3][3], I[3][3], prm[4];
    double alpha = (double)res[p].alpha, tx = (double)res[p].sx, ty = (double)res[p].sy;
    if (mode == RA_MODE_REFFREE) {
        tf_build_d(alpha, tx, ty, res[p].mirror, A);
        tf_build_d(0.0, -(double)cs[0], -(double)cs[1], 0, B);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                C[i][j] = 0;
                for (int k = 0; k < 3; k++) C[i][j] += B[i][k] * A[k][j];
            }
        tf_params_d(C, prm);
        alpha = prm[0]; tx = prm[1]; ty = prm[2];
    }
    tf_build_d(alpha, tx, ty, 0, A);
    const double det = A[0][0] * A[1][1] - A[0][1] * A[1][0];
    I[0][0] = A[1][1] / det; I[0][1] = -A[0][1] / det;
    I[1][0] = -A[1][0] / det; I[1][1] = A[0][0] / det;
    I[0][2] = -(I[0][0] * A[0][2] + I[0][1] * A[1][2]);
    I[1][2] = -(I[1][0] * A[0][2] + I[1][1] * A[1][2]);
    I[2][0] = 0; I[2][1] = 0; I[2][2] = 1;
    tf_params_d(I, prm);
    state[2 * p] = (float)prm[1];
    state[2 * p + 1] = (float)prm[2];
}

extern "C" int ra_state_from_params(ra_engine *e, const ra_result *d_result, int n, const float *cs, float *d_state)
{
    if (!e || n < 0) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (n == 0) return RA_OK;
    if (!d_result || !d_state) { g_last_error = "null argument"; return RA_ERR_ARG; }
    const float zero[2] = {0.f, 0.f};
    RA_HIP(hipMemcpyAsync(e->d_cs, cs ? cs : zero, 2 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    hipLaunchKernelGGL(state_from_params_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, n, e->cfg.mode, (const float *)e->d_cs, d_result, d_state);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

// the same with the centre correction in device memory (d_cs [2], e.g. the reduced shift sums of the average-centre rule
// divided by the particle count on the device): no host value, no copy
extern "C" int ra_state_from_params_dev(ra_engine *e, const ra_result *d_result, int n, const float *d_cs, float *d_state)
{
    if (!e || n < 0) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (n == 0) return RA_OK;
    if (!d_result || !d_state || !d_cs) { g_last_error = "null argument"; return RA_ERR_ARG; }
    hipLaunchKernelGGL(state_from_params_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, n, e->cfg.mode, d_cs, d_result, d_state);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

// Class-resident alignment (gpu_aln_noref.cu:559-782, the ISAC mode): every particle against the average of its own class, all
// classes in ONE launch of the fused search kernel.  ra_set_class_references prepares ncls references (Polar2Dm, Frngs,
// Applyws) and one B stream per class; ra_align_classes aligns particle i to reference d_cls[i].  Needs the fused kernel
// with a single reference (RA_MODE_REFFREE, nref = 1); RA_ERR_STATE otherwise (callers then loop over the classes).
extern "C" int ra_set_class_references(ra_engine *e, const float *d_refs, int ncls)
{
    if (!e || !d_refs || ncls <= 0) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (!e->fused || e->tiled || e->generic || e->cfg.nref != 1 || e->cfg.mode != RA_MODE_REFFREE) { g_last_error = "class-resident launch needs the fused kernel with one reference (and a box its reference preparation holds in LDS)"; return RA_ERR_STATE; }
    const FusedGeom f = e->fplan.f;
    if (ncls > e->cls_cap) {
        if (e->d_cls_refspec) (void)hipFree(e->d_cls_refspec);
        if (e->d_cls_Bf) (void)hipFree(e->d_cls_Bf);
        e->d_cls_refspec = nullptr; e->d_cls_Bf = nullptr; e->cls_cap = 0;
        if (e->d_cls_refx) (void)hipFree(e->d_cls_refx);
        e->d_cls_refx = nullptr;
        if (hipMalloc((void **)&e->d_cls_refspec, (size_t)ncls * e->geo.lring * sizeof(float)) != hipSuccess ||
            hipMalloc((void **)&e->d_cls_Bf, ((size_t)ncls * f.b_floats + 256) * sizeof(float)) != hipSuccess ||
            (e->refine_ok && hipMalloc((void **)&e->d_cls_refx, (size_t)ncls * e->geo.lcirc * sizeof(float)) != hipSuccess)) {
            g_last_error = "out of device memory (class references)";
            return RA_ERR_NOMEM;
        }
        e->cls_cap = ncls;
    }
    hipLaunchKernelGGL(ref_polar_fft_kernel, dim3(ncls), dim3(256), e->lds_ref, e->stream, e->dg, d_refs, ncls, e->d_cls_refspec);
    RA_HIP(hipGetLastError());
    hipLaunchKernelGGL(pack_refs_fused_kernel, dim3(std::min(64, (f.b_floats + 255) / 256), ncls), dim3(256), 0, e->stream, e->dg, f,
                       (const float *)e->d_cls_refspec, 1, e->d_cls_Bf);
    RA_HIP(hipGetLastError());
    if (e->refine_ok && e->refine_thr != 0.f && e->d_cls_refx) {
        if (const int rc = launch_refspec_exact(e, d_refs, ncls, e->d_cls_refx)) return rc;
    }
    e->cls_ready = ncls;
    return RA_OK;
}

extern "C" int ra_align_classes(ra_engine *e, const float *d_particles, int n, float *d_state, ra_result *d_result,
                                const int *d_cls)
{
    if (!e || n < 0) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (n == 0) return RA_OK;
    if (!d_particles || !d_state || !d_result || !d_cls) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (!e->fused || e->tiled || e->generic || e->cfg.nref != 1 || e->cls_ready <= 0) { g_last_error = "ra_set_class_references has not been called"; return RA_ERR_STATE; }
    return resident_search(e, e->fplan.f, false, e->d_cls_Bf, 1, e->d_cls_refx, d_particles, n, d_state, d_result, d_cls);
}

extern "C" int ra_align(ra_engine *e, const float *d_particles, int n, float *d_state, ra_result *d_result,
                        const float *cs)
{
    if (!e || n < 0) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (n == 0) return RA_OK;
    if (!d_particles || !d_state || !d_result) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (!e->refs_ready) { g_last_error = "ra_set_references has not been called"; return RA_ERR_STATE; }
    const Geometry &g = e->geo;
    const int npix = g.nx * g.nx;
    if (cs && (cs[0] != 0.f || cs[1] != 0.f)) {
        RA_HIP(hipMemcpyAsync(e->d_cs, cs, 2 * sizeof(float), hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(apply_cs_kernel, dim3((n + 255) / 256), dim3(256), 0, e->stream, n, e->d_cs, d_result, d_state);
        RA_HIP(hipGetLastError());
    }
    hipStream_t sp = e->stream;
    if (e->solo || e->fused) {
        FusedGeom f = e->fplan.f;
        // dense offset stream: a template parameter of search_fused_kernel, a run-time flag of search_tiled_kernel (RALIGN_PACK=0: off)
        f.pack = e->tiled && g.nshift % 4 != 0 && g.nshift >= 4 && pack_allowed();
        return resident_search(e, f, pack_ok(e), e->d_Bf, e->cfg.nref, e->d_refx, d_particles, n, d_state, d_result, nullptr);
    }
    {
        int rcw = ensure_unfused_ws(e);
        if (rcw) return rcw;
    }
    // the flagged particles of every chunk collect in one list; one refine launch behind the last chunk (finalize_and_refine)
    const bool refine_once = e->refine_ok && e->refine_thr != 0.f && e->d_refx && n > e->chunk;
    if (refine_once) {
        if (n > e->rlist_cap) {
            int rcg = dev_grow(e, &e->d_rlist, (size_t)n, false);
            if (rcg) return rcg;
            e->rlist_cap = n;
        }
        RA_HIP(hipMemsetAsync(e->d_rcount, 0, sizeof(int), e->stream));
    }
    for (int start = 0; start < n; start += e->chunk) {
        const int cn = std::min(e->chunk, n - start);
        float *Abuf = e->d_A;
        CandT *Cbuf = e->d_cand;
        const float *part = d_particles + (size_t)start * npix;
        float *st = d_state + (size_t)start * 2;
        std::pair<hipEvent_t, hipEvent_t> *evp = nullptr, *evc = nullptr;
        if (e->timing) {
            evp = next_events(e->ev_polar, e->ev_used_polar);
            evc = next_events(e->ev_ccf, e->ev_used_ccf);
        }
        if (evp) RA_HIP(hipEventRecord(evp->first, sp));
        if (e->generic) {
            int rcp = launch_generic_polar(e, part, st, cn, Abuf);
            if (rcp) return rcp;
        } else
            hipLaunchKernelGGL(polar_fft_kernel, dim3(cn), dim3(RA_POLAR_THREADS), e->lds_polar, sp, e->dg, part, st, cn, Abuf);
        RA_HIP(hipGetLastError());
        if (evp) RA_HIP(hipEventRecord(evp->second, sp));
        const int n_mtile = (cn * e->dg.ent_stride + 7) / 8;
        if (evc) RA_HIP(hipEventRecord(evc->first, sp));
        if (e->generic) {          // (the block shape's switches are read at the launch)
            int rcc = launch_contraction(e, Abuf, Cbuf, n_mtile, g.maxrin == 1024 && env_int("RALIGN_GCCF_SPLIT", 1) != 0, env_int("RALIGN_GCCF_TM", 0));
            if (rcc) return rcc;
        } else
            hipLaunchKernelGGL(e->ccf, dim3(n_mtile), dim3(RA_CCF_THREADS), e->lds_ccf, sp, e->dg, Abuf, e->d_B, n_mtile,
                               e->nrtile, e->cfg.nref, Cbuf);
        RA_HIP(hipGetLastError());
        if (evc) RA_HIP(hipEventRecord(evc->second, sp));
        int rcf = finalize_and_refine(e, Cbuf, e->nrtile, cn, st, d_result + start, part, e->d_refx, nullptr, refine_once ? 1 : 0, start);
        if (rcf) return rcf;
    }
    if (refine_once) {
        int rcf = finalize_and_refine(e, nullptr, e->nrtile, n, d_state, d_result, d_particles, e->d_refx, nullptr, 2, 0);
        if (rcf) return rcf;
    }
    return RA_OK;
}

extern "C" int ra_debug_spectra(ra_engine *e, const float *d_particles, int n, const float *d_state, float *h_out)
{
    if (!e || !d_particles || !d_state || !h_out || n < 1 || n > e->chunk) { g_last_error = "bad argument"; return RA_ERR_ARG; }
    const Geometry &g = e->geo;
    if (e->search.debug) {
        // the polar stage of search_solo_kernel: ring buffer and statistics of every in-window (particle, offset)
        const size_t rawcnt = (size_t)n * g.nshift * (g.lring + 2), cnt = (size_t)n * g.nshift * g.lcirc;
        float *d_raw = nullptr, *d_out = nullptr;
        RA_HIP(hipMalloc((void **)&d_raw, rawcnt * sizeof(float)));
        hipError_t he = hipMalloc((void **)&d_out, cnt * sizeof(float));
        if (he == hipSuccess) he = hipMemsetAsync(d_raw, 0, rawcnt * sizeof(float), e->stream);
        if (he == hipSuccess) {
            const FusedGeom f = e->fplan.f;
            hipLaunchKernelGGL(e->search.debug, dim3(std::min(n, e->n_cu)), dim3(RF_THREADS), e->search.lds, e->stream, e->dg, f, d_particles,
                               d_state, n, (const float *)e->d_Bf, e->cfg.nref, e->d_fcand, d_raw);
            hipLaunchKernelGGL(unpack_solo_spectra_kernel, dim3(n * g.nshift), dim3(256), 0, e->stream, e->dg, (const float *)d_raw, n,
                               (const int *)e->d_numr, (const int *)e->d_ring_off, d_out);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        if (he == hipSuccess) he = hipMemcpy(h_out, d_out, cnt * sizeof(float), hipMemcpyDeviceToHost);
        (void)hipFree(d_raw);
        if (d_out) (void)hipFree(d_out);
        RA_HIP(he);
        return RA_OK;
    }
    {
        int rcw = ensure_unfused_ws(e);
        if (rcw) return rcw;
    }
    if (e->generic) {
        int rcp = launch_generic_polar(e, d_particles, d_state, n, e->d_A);
        if (rcp) return rcp;
    } else
        hipLaunchKernelGGL(polar_fft_kernel, dim3(n), dim3(RA_POLAR_THREADS), e->lds_polar, e->stream, e->dg, d_particles, d_state, n, e->d_A);
    RA_HIP(hipGetLastError());
    float *d_out = nullptr;
    const size_t cnt = (size_t)n * g.nshift * g.lcirc;
    RA_HIP(hipMalloc((void **)&d_out, cnt * sizeof(float)));
    hipLaunchKernelGGL(unpack_spectra_kernel, dim3(n * g.nshift), dim3(256), 0, e->stream, e->dg, e->d_A, n, e->d_numr, d_out,
                       e->generic ? (const float2 *)e->d_gstats : (const float2 *)nullptr, d_state);
    hipError_t he = hipStreamSynchronize(e->stream);
    if (he == hipSuccess) he = hipMemcpy(h_out, d_out, cnt * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    RA_HIP(he);
    return RA_OK;
}

// ---- rot_shift2D and the class sums (ralign_xform.h; xs_plan at the top of this file)

// rot_shift2D of n images, with fp32-atomic sums and counts where they are not null: the image in LDS while it fits, read from
// global memory beyond.  e == null: no engine, whose create raised transform_kernel's LDS.
static int launch_transform(hipStream_t stream, ra_engine *e, int nx, const float *d_in, int n, int index0, const ra_result *d_res,
                            float *d_aligned, float *d_sums, int *d_counts)
{
    const int npix = nx * nx;
    if (xf_in_lds(nx)) {
        if (!e) { if (const int rc = RA_LDS(nullptr, transform_kernel, xf_lds_bytes(nx))) return rc; }
        hipLaunchKernelGGL(transform_kernel, dim3(n), dim3(RA_XF_THREADS), xf_lds_bytes(nx), stream, nx, d_in, n, index0, d_res, d_aligned,
                           d_sums, d_counts);
    } else
        // (at least 8 row blocks per image; a handful of images -- the references of an update step -- are cut into more: 10 images x 8 blocks left the GPU idle)
        hipLaunchKernelGGL(transform_generic_kernel, dim3(n, std::max(8, std::min((npix + 255) / 256, (2048 + n - 1) / n))), dim3(256), 0, stream,
                           nx, d_in, n, index0, d_res, d_aligned, d_sums, d_counts);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

// (RALIGN_XSUM=0 / RALIGN_XTILE=0, read at the launch: the aligned stack + class_sum_kernel instead, for every box / for the tile boxes)
static bool xs_usable(const ra_engine *e)
{
    if (e->atomic_sums || env_int("RALIGN_XSUM", 1) == 0) return false;
    const XsPlan p = xs_plan(e->geo.nx);
    return p.whole_image() || (p.kind == XsPlan::TILE && env_int("RALIGN_XTILE", 1) != 0);
}

// rot_shift2D + class sums without the aligned stack: member lists of up to RA_XS_BATCH particles at once, every
// (class, parity) list cut into runs (xs_runs)
#define RA_XS_BATCH 65536
static int transform_sum(ra_engine *e, const float *d_particles, int n, int index0, const ra_result *d_result, float *d_sums, int *d_counts)
{
    const int nx = e->geo.nx, npix = nx * nx, nseg = 2 * e->cfg.nref;
    const XsPlan p = xs_plan(nx);
    if (p.kind == XsPlan::NONE) { g_last_error = "transform_sum: no kernel for this box"; return RA_ERR_ARG; }
    auto &cs = e->cs;
    int rc;
    if (p.lds > 64 * 1024 && (rc = raise_dynamic_lds(e, p.kernel(), p.name, p.lds))) return rc;
    if (p.kind == XsPlan::TWO_COPY && !cs.xs_slots) {
        int per_cu = 0;
        RA_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, p.kernel(), p.threads, p.lds));
        cs.xs_slots = std::max(1, per_cu) * std::max(1, e->n_cu);
    }
    auto reserve = [e](auto **buf, size_t *cap, size_t need) {
        if (need <= *cap) return (int)RA_OK;
        const int rcg = dev_grow(e, buf, need, false);
        if (!rcg) *cap = need;
        return rcg;
    };
    for (int start = 0; start < n; start += RA_XS_BATCH) {
        const int cn = std::min(RA_XS_BATCH, n - start), nrun = xs_runs(p, nseg, cn);
        if ((rc = reserve(&cs.xs_members, &cs.cap_members, (size_t)nseg * cn)) || (rc = reserve(&cs.xs_trig, &cs.cap_trig, (size_t)cn)) ||
            (rc = reserve(&cs.xs_partial, &cs.cap_partial, (size_t)nrun * nseg * npix)) ||
            (!cs.xs_mcount && (rc = dev_alloc(e, &cs.xs_mcount, (size_t)nseg, true)))) return rc;
        const float *part = d_particles + (size_t)start * npix;
        const ra_result *res = d_result + start;
        const float2 *trig = cs.xs_trig;
        const int *members = cs.xs_members, *mcount = cs.xs_mcount;
        hipLaunchKernelGGL(transform_trig_kernel, dim3((cn + 255) / 256), dim3(256), 0, e->stream, res, cn, cs.xs_trig);
        RA_HIP(hipGetLastError());
        hipLaunchKernelGGL(class_members_wide_kernel, dim3(nseg), dim3(1024), 0, e->stream, res, cn, index0 + start, cs.xs_members, cs.xs_mcount, cn,
                           d_counts);
        RA_HIP(hipGetLastError());
        if (p.kind == XsPlan::TWO_COPY) {
            // a small surplus of work items over whole rounds of resident workgroups would hold a round of its own: those
            // items run as row bands, a third of the sweeps each, behind the full ones
            const int items = nseg * nrun, over = items % cs.xs_slots;
            XsGrid gr{nseg, nrun, items, p.sb0, p.nb0, p.sb0, 1};
            if (p.nb0 == 1 && p.npf >= 2 && items > cs.xs_slots && over > 0 && over * 8 <= cs.xs_slots) {
                gr.sb1 = (p.npf + 2) / 3; gr.nb1 = (p.npf + gr.sb1 - 1) / gr.sb1; gr.nfull = items - over;
            }
            hipLaunchKernelGGL(p.dbfn, dim3(gr.nfull * gr.nb0 + (items - gr.nfull) * gr.nb1), dim3(p.threads), p.lds, e->stream, nx, part, res, trig,
                               members, mcount, cn, cs.xs_partial, gr);
        } else          // (segment, run, row band | output tile)
            hipLaunchKernelGGL(p.fn, dim3(nseg, nrun, p.kind == XsPlan::TILE ? p.ntile : p.nband), dim3(p.threads), p.lds, e->stream, nx, part, res, trig,
                               members, mcount, cn, cs.xs_partial);
        RA_HIP(hipGetLastError());
        hipLaunchKernelGGL(class_sum_combine_kernel, dim3((unsigned)(((size_t)nseg * npix + 255) / 256)), dim3(256), 0, e->stream, npix, nseg, nrun,
                           (const float *)cs.xs_partial, d_sums);
        RA_HIP(hipGetLastError());
    }
    return RA_OK;
}

extern "C" int ra_transform_accumulate(ra_engine *e, const float *d_particles, int n, int index0,
                                       const ra_result *d_result, float *d_aligned, float *d_sums, int *d_counts)
{
    if (!e || n < 0) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (n == 0) return RA_OK;
    if (!d_particles || !d_result) { g_last_error = "null argument"; return RA_ERR_ARG; }
    const int nx = e->geo.nx, npix = nx * nx;
    if (!d_sums || e->atomic_sums) return launch_transform(e->stream, e, nx, d_particles, n, index0, d_result, d_aligned, d_sums, d_counts);
    if (!d_aligned && xs_usable(e)) return transform_sum(e, d_particles, n, index0, d_result, d_sums, d_counts);
    // aligned images wanted as well (or no one-pass kernel for the box): aligned images of a chunk, then particle-order sums per
    // (class, parity)
    auto &cs = e->cs;
    int rc;
    if (!d_aligned && !e->d_alscratch && (rc = dev_alloc(e, &e->d_alscratch, e->wp.alscratch_floats, false))) return rc;
    // member lists once per chunk; every (class, parity) list is then cut into runs so that ~4000 workgroups share the additions
    const int nseg = 2 * e->cfg.nref, ntile = (npix + 255) / 256;
    const bool glists = (size_t)nseg * e->chunk * sizeof(int) <= ((size_t)256 << 20);
    const int nrun = std::min(16, std::max(1, (glists ? 4096 : 1024) / (nseg * ntile)));
    if (glists && !cs.members &&
        ((rc = dev_alloc(e, &cs.members, (size_t)nseg * e->chunk, false)) || (rc = dev_alloc(e, &cs.mcount, (size_t)nseg, true)))) return rc;
    if (nrun > 1 && !cs.sumpart && (rc = dev_alloc(e, &cs.sumpart, (size_t)16 * nseg * npix, false))) return rc;
    for (int start = 0; start < n; start += e->chunk) {
        const int cn = std::min(e->chunk, n - start);
        float *al = d_aligned ? d_aligned + (size_t)start * npix : e->d_alscratch;
        if ((rc = launch_transform(e->stream, e, nx, d_particles + (size_t)start * npix, cn, index0 + start, d_result + start, al, nullptr, nullptr)))
            return rc;
        if (glists) {          // (the counts are class_sum_kernel's to add on this path)
            hipLaunchKernelGGL(class_members_wide_kernel, dim3(nseg), dim3(1024), 0, e->stream, d_result + start, cn, index0 + start, cs.members,
                               cs.mcount, cn, (int *)nullptr);
            RA_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(class_sum_kernel, dim3(nseg, ntile, nrun), dim3(256), glists ? 0 : (size_t)cn * sizeof(int), e->stream, npix, al,
                           d_result + start, cn, index0 + start, d_sums, d_counts, nrun > 1 ? cs.sumpart : (float *)nullptr,
                           (const int *)cs.members, (const int *)cs.mcount);
        RA_HIP(hipGetLastError());
        if (nrun > 1) {
            hipLaunchKernelGGL(class_sum_combine_kernel, dim3((unsigned)(((size_t)nseg * npix + 255) / 256)), dim3(256), 0, e->stream, npix, nseg, nrun,
                               (const float *)cs.sumpart, d_sums);
            RA_HIP(hipGetLastError());
        }
    }
    return RA_OK;
}

extern "C" int ra_update_references(ra_engine *e, const float *d_sums, const int *d_counts, int min_count,
                                    float *d_refs)
{
    if (!e || !d_sums || !d_counts || !d_refs) { g_last_error = "null argument"; return RA_ERR_ARG; }
    hipLaunchKernelGGL(update_refs_kernel, dim3(e->cfg.nref), dim3(256), 0, e->stream, e->geo.nx, d_sums, d_counts,
                       min_count, e->dg.mask, d_refs);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

extern "C" int ra_normalize_particles(ra_engine *e, float *d_particles, int n)
{
    if (!e || n < 0) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (n == 0) return RA_OK;
    if (!d_particles) { g_last_error = "null argument"; return RA_ERR_ARG; }
    hipLaunchKernelGGL(normalize_particles_kernel, dim3(n), dim3(256), 0, e->stream, e->geo.nx, e->dg.mask,
                       d_particles, n);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

extern "C" int ra_sync(ra_engine *e)
{
    if (!e) return RA_ERR_ARG;
    RA_HIP(hipStreamSynchronize(e->stream));
    return RA_OK;
}

extern "C" int ra_kernel_time(ra_engine *e, int enable, double *ms_ccf, int *launches_ccf, double *ms_polar,
                              int *launches_polar)
{
    if (!e) return RA_ERR_ARG;
    RA_HIP(hipStreamSynchronize(e->stream));
    double a = 0, b = 0;
    for (size_t i = 0; i < e->ev_used_ccf; i++) {
        float ms = 0;
        RA_HIP(hipEventElapsedTime(&ms, e->ev_ccf[i].first, e->ev_ccf[i].second));
        a += ms;
    }
    for (size_t i = 0; i < e->ev_used_polar; i++) {
        float ms = 0;
        RA_HIP(hipEventElapsedTime(&ms, e->ev_polar[i].first, e->ev_polar[i].second));
        b += ms;
    }
    if (ms_ccf) *ms_ccf = a;
    if (launches_ccf) *launches_ccf = (int)e->ev_used_ccf;
    if (ms_polar) *ms_polar = b;
    if (launches_polar) *launches_polar = (int)e->ev_used_polar;
    e->ev_used_ccf = e->ev_used_polar = 0;
    e->timing = enable != 0;
    return RA_OK;
}

// ---------------------------------------------------------------------------------------------
// reference update on the device (kernels in ralign_refine.h)

static int ensure_refine_ws(ra_engine *e, int nimg)
{
    if (nimg <= e->rf_cap) return RA_OK;
    const int nx = e->geo.nx, nxh = nx / 2 + 1;
    const int cap = std::max(nimg, 2 * e->cfg.nref);
    int rc;
    // growing replaces the buffers that hold one call's images (the old ones are released now); the per-class curves are
    // 2 nref rows whatever nimg is and outlive the call (ra_last_class_fsc), so they are allocated once and kept
    e->rf_cap = 0;          // until every buffer is in place again
    if ((rc = dev_grow(e, &e->d_rfT, (size_t)cap * nx * nxh, false)) || (rc = dev_grow(e, &e->d_rfF, (size_t)cap * nx * nxh, false)) ||
        (rc = dev_grow(e, &e->d_rfmean, (size_t)cap, true)) || (rc = dev_grow(e, &e->d_rfcs, (size_t)cap * 2, true)))
        return rc;
    if (!e->d_rffsc && (rc = dev_alloc(e, &e->d_rffsc, (size_t)2 * e->cfg.nref * (nx / 2 + 1), true))) return rc;
    if (!e->d_rftw) {
        std::vector<double2> tw(nx);
        for (int t = 0; t < nx; t++) { const double a = 2.0 * M_PI * t / nx; tw[t] = make_double2(cos(a), sin(a)); }
        if ((rc = upload(e, tw, &e->d_rftw))) return rc;
    }
    e->rf_cap = cap;
    return RA_OK;
}

static int forward_dft(ra_engine *e, const float *d_imgs, int nimg, const float *d_mask, const float *d_mean)
{
    const int nx = e->geo.nx;
    hipLaunchKernelGGL(dft_rows_kernel, dim3(nimg, nx), dim3(64), 0, e->stream, nx, d_imgs, d_mask, d_mean, e->d_rftw, e->d_rfT);
    RA_HIP(hipGetLastError());
    hipLaunchKernelGGL(dft_cols_kernel<-1>, dim3(nimg, nx), dim3(64), 0, e->stream, nx, e->d_rfT, e->d_rftw, e->d_rfF);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

extern "C" int ra_fsc_len(const ra_engine *e) { return e ? e->geo.nx / 2 + 1 : RA_ERR_ARG; }

// fsc / fsc_mask of the even and odd sum of every class: e->d_rffsc [nref][2][nx/2+1] = {fsc, points per shell}
static int class_fsc_kernels(ra_engine *e, const float *d_sums, int masked)
{
    const int R = e->cfg.nref, nx = e->geo.nx;
    int rc = ensure_refine_ws(e, 2 * R);
    if (rc) return rc;
    if (masked) {
        hipLaunchKernelGGL(masked_mean_kernel, dim3(2 * R), dim3(256), 0, e->stream, nx * nx, d_sums, e->dg.mask, e->d_rfmean);
        RA_HIP(hipGetLastError());
    }
    if ((rc = forward_dft(e, d_sums, 2 * R, masked ? e->dg.mask : nullptr, masked ? e->d_rfmean : nullptr))) return rc;
    const int len = nx / 2 + 1;
    if (!e->d_fsc_off) {          // the coefficients of every shell, in scan order
        std::vector<int> off, idx;
        fsc_shell_table(nx, off, idx);
        if ((rc = upload(e, off, &e->d_fsc_off)) || (rc = upload(e, idx, &e->d_fsc_idx))) return rc;
    }
    const int threads = std::min(1024, (RA_FSC_PARTS * len + 63) / 64 * 64);
    const size_t lds = (size_t)RA_FSC_PARTS * len * 4 * sizeof(double);
    if (lds > 64 * 1024 && (rc = RA_LDS(e, fsc_kernel, lds))) return rc;
    hipLaunchKernelGGL(fsc_kernel, dim3(R), dim3(threads), lds, e->stream, nx, e->d_rfF, e->d_fsc_off, e->d_fsc_idx, e->d_rffsc);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

// Average FSC of the live classes and the tangent-filter fit entirely on the device (fsc_fit_kernel): nothing comes back to
// the host, ra_filter_references_dev takes (fl, aa) from d_fit.  d_fit [5] = {fl, aa clamped, fl, aa fitted, status},
// d_curve [3][nx/2+1] = {frequency, fsc as fit_tanh leaves it, points}; the caller copies them to the host when it wants them
// (bookkeeping).  Asynchronous on the engine's stream.
extern "C" int ra_class_fsc_fit(ra_engine *e, const float *d_sums, const int *d_counts, int min_count, int masked, float fl_lo,
                                float fl_hi, float aa_hi, float *d_fit, float *d_curve)
{
    if (!e || !d_sums || !d_counts || !d_fit || !d_curve) { g_last_error = "null argument"; return RA_ERR_ARG; }
    int rc = class_fsc_kernels(e, d_sums, masked);
    if (rc) return rc;
    const int len = e->geo.nx / 2 + 1;
    hipLaunchKernelGGL(fsc_fit_kernel, dim3(1), dim3(64), (size_t)len * (sizeof(double) + 2 * sizeof(float)), e->stream, e->geo.nx, e->cfg.nref,
                       (const float *)e->d_rffsc, d_counts, min_count, fl_lo, fl_hi, aa_hi, d_fit, d_curve);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

extern "C" int ra_class_fsc(ra_engine *e, const float *d_sums, const int *d_counts, int min_count, int masked, float *h_fsc)
{
    if (!e || !d_sums || !d_counts || !h_fsc) { g_last_error = "null argument"; return RA_ERR_ARG; }
    const int R = e->cfg.nref, nx = e->geo.nx, len = nx / 2 + 1;
    int rc = class_fsc_kernels(e, d_sums, masked);
    if (rc) return rc;
    std::vector<float> all((size_t)R * 2 * len);
    std::vector<int> counts(R);
    RA_HIP(hipMemcpyAsync(all.data(), e->d_rffsc, all.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    RA_HIP(hipMemcpyAsync(counts.data(), d_counts, R * sizeof(int), hipMemcpyDeviceToHost, e->stream));
    RA_HIP(hipStreamSynchronize(e->stream));
    // average over the live classes as the reference does (ave_fsc / c_fsc; kept only if its sum is not 0)
    std::vector<double> ave(len, 0.0);
    int live = 0, last = -1;
    for (int j = 0; j < R; j++) {
        if (counts[j] < min_count) continue;
        for (int i = 0; i < len; i++) ave[i] += all[((size_t)j * 2) * len + i];
        live++; last = j;
    }
    if (live == 0) { g_last_error = "ra_class_fsc: every class is below min_count"; return RA_ERR_STATE; }
    double tot = 0;
    for (int i = 0; i < len; i++) tot += ave[i];
    for (int i = 0; i < len; i++) {
        h_fsc[i] = (float)((double)i / (2.0 * (nx / 2)));
        h_fsc[len + i] = (tot != 0.0) ? (float)(ave[i] / live) : all[((size_t)last * 2) * len + i];
        h_fsc[2 * len + i] = all[((size_t)last * 2 + 1) * len + i];
    }
    return RA_OK;
}

// the per-class curves behind the last ra_class_fsc: h_all [nref][2][nx/2+1] = {fsc, points per shell} of every class (what
// the reference writes to drm%03d%04d.txt, test_mref_gpu_align.py:533)
extern "C" int ra_last_class_fsc(ra_engine *e, float *h_all)
{
    if (!e || !h_all) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (!e->d_rffsc) { g_last_error = "ra_class_fsc has not been called"; return RA_ERR_STATE; }
    const size_t cnt = (size_t)e->cfg.nref * 2 * (e->geo.nx / 2 + 1);
    RA_HIP(hipMemcpyAsync(h_all, e->d_rffsc, cnt * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    RA_HIP(hipStreamSynchronize(e->stream));
    return RA_OK;
}

// sp_filter.fit_tanh(dres, low = 0.1) with sp_utilities.amoeba (simplex maximisation); host arithmetic in
// double like the Python original.  fsc is edited in place (zeroed after its first drop below `low`).
namespace {
struct TanhFit {
    const float *freq; float *fsc; int n;
    double operator()(const double *a) const
    {
        double v = 0.0;
        if (fsc[0] < 0.0f) fsc[0] *= -1.0f;
        for (int i = 0; i < n; i++) {
            const double r = fsc[i], f = 2 * r / (1.0 + r);
            double qt = 0;
            if (a[0] != 0 && a[1] != 0)
                qt = f - 0.5 * (tanh(M_PI * (freq[i] + a[0]) / 2.0 / a[1] / a[0]) - tanh(M_PI * (freq[i] - a[0]) / 2.0 / a[1] / a[0]));
            v -= qt * qt;
        }
        return v;
    }
};
}  // namespace

extern "C" int ra_fit_tanh(const float *freq, float *fsc, int n, float *fl, float *aa)
{
    if (!freq || !fsc || !fl || !aa || n < 3) { g_last_error = "bad argument"; return RA_ERR_ARG; }
    const double low = 0.1;
    bool setzero = false;
    for (int i = 1; i < n; i++) {
        if (!setzero && 2 * (double)fsc[i] / (1.0 + fsc[i]) < low) setzero = true;
        if (setzero) fsc[i] = 0.0f;
    }
    double f0 = -1.0;
    for (int i = 1; i < n - 1; i++)
        if (2 * (double)fsc[i] / (1.0 + fsc[i]) < 0.5) { f0 = freq[i - 1]; break; }
    if (f0 < 0.0) {
        if (fsc[n - 1] < 0.5f) { *fl = 0.5f; *aa = 0.2f; } else { *fl = 0.49f; *aa = 0.1f; }
        return RA_OK;
    }
    TanhFit func{freq, fsc, n};
    const double scale[2] = {0.05, 0.05}, ftol = 1.e-4, xtol = 1.e-4;
    double sx[3][2] = {{f0, 0.1}, {f0 + scale[0], 0.1}, {f0, 0.1 + scale[1]}}, fv[3];
    for (int i = 0; i < 3; i++) fv[i] = func(sx[i]);
    int iteration = 0, best = 0;
    while (true) {
        int worst = 0; best = 0;
        for (int i = 0; i < 3; i++) { if (fv[i] > fv[best]) best = i; if (fv[i] < fv[worst]) worst = i; }
        double pavg[2] = {0, 0};
        for (int i = 0; i < 3; i++) if (i != worst) { pavg[0] += sx[i][0]; pavg[1] += sx[i][1]; }
        pavg[0] /= 2; pavg[1] /= 2;
        const double simscale = (fabs(pavg[0] - sx[worst][0]) / scale[0] + fabs(pavg[1] - sx[worst][1]) / scale[1]) / 2;
        const double fscale = (fabs(fv[best]) + fabs(fv[worst])) / 2.0;
        const double frange = fscale != 0.0 ? fabs(fv[best] - fv[worst]) / fscale : 0.0;
        if ((frange < ftol && simscale < xtol) || iteration >= 500) break;
        double pnew[2] = {2.0 * pavg[0] - sx[worst][0], 2.0 * pavg[1] - sx[worst][1]};
        double fnew = func(pnew);
        if (fnew <= fv[worst]) {           // worse than the worst: shrink towards the best
            for (int i = 0; i < 3; i++)
                if (i != best && i != worst) {
                    sx[i][0] = 0.5 * sx[best][0] + 0.5 * sx[i][0]; sx[i][1] = 0.5 * sx[best][1] + 0.5 * sx[i][1];
                    fv[i] = func(sx[i]);
                }
            pnew[0] = 0.5 * sx[best][0] + 0.5 * sx[worst][0]; pnew[1] = 0.5 * sx[best][1] + 0.5 * sx[worst][1];
            fnew = func(pnew);
        } else if (fnew >= fv[best]) {     // better than the best: try to expand
            double p2[2] = {3.0 * pavg[0] - 2.0 * sx[worst][0], 3.0 * pavg[1] - 2.0 * sx[worst][1]};
            const double f2 = func(p2);
            if (f2 > fnew) { pnew[0] = p2[0]; pnew[1] = p2[1]; fnew = f2; }
        }
        sx[worst][0] = pnew[0]; sx[worst][1] = pnew[1]; fv[worst] = fnew;
        iteration++;
    }
    *fl = (float)sx[best][0]; *aa = (float)sx[best][1];
    return RA_OK;
}

extern "C" int ra_class_averages(ra_engine *e, const float *d_sums, const int *d_counts, int min_count, float *d_refs)
{
    if (!e || !d_sums || !d_counts || !d_refs) { g_last_error = "null argument"; return RA_ERR_ARG; }
    hipLaunchKernelGGL(class_average_kernel, dim3(e->cfg.nref), dim3(256), 0, e->stream, e->geo.nx * e->geo.nx, d_sums, d_counts,
                       min_count, d_refs);
    RA_HIP(hipGetLastError());
    return RA_OK;
}

// filt_tanl + center_2D + (normalize.mask) of nimg images in place; fl / aa by value or (d_flaa != null) from device memory;
// centres: center = -1 reads d_cs_in [nimg][2] (device), the applied centres land in e->d_rfcs
static int filter_references_core(ra_engine *e, float *d_imgs, int nimg, float fl, float aa, const float *d_flaa, int center,
                                  const float *d_cs_in, int normalize)
{
    const int nx = e->geo.nx;
    int rc;
    if ((rc = forward_dft(e, d_imgs, nimg, nullptr, nullptr))) return rc;
    hipLaunchKernelGGL(filter_center_kernel, dim3(nimg), dim3(256), 0, e->stream, nx, e->d_rfF, fl, aa, center,
                       center == -1 ? d_cs_in : (const float *)nullptr, e->d_rfcs, d_flaa);
    RA_HIP(hipGetLastError());
    hipLaunchKernelGGL(dft_cols_kernel<1>, dim3(nimg, nx), dim3(64), 0, e->stream, nx, e->d_rfF, e->d_rftw, e->d_rfT);
    RA_HIP(hipGetLastError());
    hipLaunchKernelGGL(idft_rows_kernel, dim3(nimg, nx), dim3(128), 0, e->stream, nx, e->d_rfT, e->d_rftw, d_imgs);
    RA_HIP(hipGetLastError());
    if (normalize) {
        hipLaunchKernelGGL(normalize_mask_kernel, dim3(nimg), dim3(256), 0, e->stream, nx * nx, e->dg.mask, d_imgs);
        RA_HIP(hipGetLastError());
    }
    return RA_OK;
}

extern "C" int ra_filter_references(ra_engine *e, float *d_imgs, int nimg, float fl, float aa, int center,
                                    const float *h_cs_in, int normalize, float *h_cs_out)
{
    if (!e || !d_imgs || nimg < 1) { g_last_error = "bad argument"; return RA_ERR_ARG; }
    if (center == -1 && !h_cs_in) { g_last_error = "center = -1 needs the shift list"; return RA_ERR_ARG; }
    int rc = ensure_refine_ws(e, nimg);
    if (rc) return rc;
    if (center == -1) RA_HIP(hipMemcpyAsync(e->d_rfcs, h_cs_in, (size_t)nimg * 2 * sizeof(float), hipMemcpyHostToDevice, e->stream));
    if ((rc = filter_references_core(e, d_imgs, nimg, fl, aa, nullptr, center, e->d_rfcs, normalize))) return rc;
    if (h_cs_out) {
        RA_HIP(hipMemcpyAsync(h_cs_out, e->d_rfcs, (size_t)nimg * 2 * sizeof(float), hipMemcpyDeviceToHost, e->stream));
        RA_HIP(hipStreamSynchronize(e->stream));
    }
    return RA_OK;
}

// the same without a host value in the path: (fl, aa) = d_flaa[0..1] (ra_class_fsc_fit's d_fit; null: no filter), the centres
// of center = -1 from d_cs_in [nimg][2], the applied centres to d_cs_out [nimg][2] (device, may be null).  Asynchronous.
extern "C" int ra_filter_references_dev(ra_engine *e, float *d_imgs, int nimg, const float *d_flaa, int center,
                                        const float *d_cs_in, int normalize, float *d_cs_out)
{
    if (!e || !d_imgs || nimg < 1) { g_last_error = "bad argument"; return RA_ERR_ARG; }
    if (center == -1 && !d_cs_in) { g_last_error = "center = -1 needs the shift list"; return RA_ERR_ARG; }
    int rc = ensure_refine_ws(e, nimg);
    if (rc) return rc;
    if ((rc = filter_references_core(e, d_imgs, nimg, 0.f, 0.f, d_flaa, center, d_cs_in, normalize))) return rc;
    if (d_cs_out) RA_HIP(hipMemcpyAsync(d_cs_out, e->d_rfcs, (size_t)nimg * 2 * sizeof(float), hipMemcpyDeviceToDevice, e->stream));
    return RA_OK;
}

// ---- what the reference-compatible surface (ralign_legacy.hip) needs of an engine without seeing the struct (ralign_host.h)

void ra_engine_switch_mode(ra_engine *e, int mode)
{
    e->cfg.mode = mode; e->dg.mode = mode; e->dg.norm_ring = mode == RA_MODE_MREF ? 1 : 0;
    e->dg.win_ring = mode == RA_MODE_MREF ? e->geo.last_ring : e->geo.numr[3 * (e->geo.nring - 1)];      // (Normalize_ring follows the entry point: multiref_polar_ali_2d | ormq)
}

size_t ra_planned_workspace_bytes(const ra_config *rc)
{
    Geometry g;
    if (!build_rings(g, rc->nx, rc->first_ring, rc->last_ring, rc->ring_skip) || !build_shifts(g, rc->xrng, rc->yrng, rc->step))
        return (size_t)-1;
    // the FIRST plan of ra_create with default options: the estimate knows nothing of ra_options, the tight-ring geometry or the
    // generic-class second attempt of ra_create_ex
    const PlanRequest rq{read_switches(), false, false, true};
    const bool generic = !fits_specialised_kernels(g, *rc, rq);
    if (generic && g.maxrin <= 1024) align_ring_quads(g);      // as ra_create: the panel size follows the layout
    return plan_workspace(g, *rc, rq, generic).bytes;
}

// ---- rot_shift2D without an engine (it launches the engine's transform kernels)

extern "C" int ra_rot_shift2d(const float *d_in, int n, int nx, const ra_result *d_params, float *d_out, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 0 || nx < 2 || nx > 1024) { g_last_error = "ra_rot_shift2d: need n >= 0 and 2 <= nx <= 1024"; return RA_ERR_ARG; }
    if (n == 0) return RA_OK;
    if (!d_in || !d_params || !d_out) { g_last_error = "ra_rot_shift2d: null argument"; return RA_ERR_ARG; }
    // the kernel and grid ra_transform_accumulate picks for the same box without sums
    return launch_transform(stream, nullptr, nx, d_in, n, 0, d_params, d_out, nullptr, nullptr);
}

// ---- diagnostics of the decision stage (include/ralign.h): the engine's finalize and replay kernels on hand-built records.
// Buffers of their own, the engine's DevGeom by value: nothing a search uses is written.

// the record layouts the numpy dtypes of api.py restate (CAND_DTYPE, REFINE_DTYPE)
static_assert(sizeof(CandT) == 40 && offsetof(CandT, t7) == 12, "CandT: update CAND_DTYPE (api.py)");
static_assert(sizeof(RefineRec) == 120 && offsetof(RefineRec, alt) == 36 && sizeof(RefineAlt) == 12, "RefineRec: update REFINE_DTYPE (api.py)");
#define RA_DEBUG_MAX_N 32768          // live_scan_kernel's bound

namespace {
// device buffers of one diagnostic call, freed when it returns
struct DebugBufs {
    std::vector<void *> ptrs;
    ~DebugBufs() { for (void *p : ptrs) (void)hipFree(p); }
    template <class T> hipError_t get(T **p, size_t count)
    {
        const hipError_t he = hipMalloc((void **)p, std::max<size_t>(count, 1) * sizeof(T));
        if (he == hipSuccess) ptrs.push_back(*p);
        return he;
    }
};
bool debug_refine_ready(const ra_engine *e)
{
    if (e->refine_ok && e->refs_ready && e->refine_thr != 0.f && e->d_refx && e->dg.ref_dup) return true;
    g_last_error = "the decision diagnostics need the sub-bin refinement (ra_set_refine != 0) and ra_set_references";
    return false;
}
}  // namespace

extern "C" int ra_debug_exact_references(ra_engine *e, float *h_refx, int *h_dup)
{
    if (!e) { g_last_error = "null argument"; return RA_ERR_ARG; }
    if (!debug_refine_ready(e)) return RA_ERR_STATE;
    RA_HIP(hipStreamSynchronize(e->stream));
    if (h_refx) RA_HIP(hipMemcpy(h_refx, e->d_refx, (size_t)e->cfg.nref * e->geo.lcirc * sizeof(float), hipMemcpyDeviceToHost));
    if (h_dup) RA_HIP(hipMemcpy(h_dup, e->d_refdup, (size_t)2 * e->cfg.nref * sizeof(int), hipMemcpyDeviceToHost));
    return RA_OK;
}

extern "C" int ra_debug_finalize(ra_engine *e, const void *h_cand, int nrtile, int n, const float *h_state, int kernel, int live,
                                 float refine_thr, ra_result *h_res, float *h_state_out, void *h_rlist, int rlist_cap, int *h_count)
{
    if (!e || !h_cand || !h_state || !h_res || !h_state_out || !h_count || n < 1 || n > RA_DEBUG_MAX_N || nrtile < 1 || nrtile > 4096 ||
        (kernel != 0 && kernel != 1) || (live != 0 && live != 1) || (h_rlist && rlist_cap < n)) {
        g_last_error = "ra_debug_finalize: bad argument";
        return RA_ERR_ARG;
    }
    if (!debug_refine_ready(e)) return RA_ERR_STATE;
    DevGeom dg = e->dg;
    DebugBufs bufs;
    float *d_st = nullptr;
    ra_result *d_res = nullptr;
    int *d_base = nullptr, *d_total = nullptr, *d_cnt = nullptr;
    CandT *d_cand = nullptr;
    RefineRec *d_rl = nullptr;
    RA_HIP(bufs.get(&d_st, (size_t)2 * n));
    RA_HIP(bufs.get(&d_res, (size_t)n));
    RA_HIP(bufs.get(&d_cnt, 1));
    RA_HIP(bufs.get(&d_base, (size_t)n + 8));
    RA_HIP(bufs.get(&d_total, 4));
    if (h_rlist) RA_HIP(bufs.get(&d_rl, (size_t)n));
    RA_HIP(hipMemcpyAsync(d_st, h_state, (size_t)2 * n * sizeof(float), hipMemcpyHostToDevice, e->stream));
    RA_HIP(hipMemsetAsync(d_cnt, 0, sizeof(int), e->stream));
    RA_HIP(hipMemsetAsync(d_res, 0, (size_t)n * sizeof(ra_result), e->stream));
    if (d_rl) RA_HIP(hipMemsetAsync(d_rl, 0, (size_t)n * sizeof(RefineRec), e->stream));          // (alt[nalt ..] is not written: zeros, the same bytes every time)
    size_t entries = (size_t)n * dg.ent_stride;
    dg.ent_base = nullptr; dg.ent_total = nullptr;
    if (live) {          // the entry ranges as the size-generic path lays them out before its kernels
        hipLaunchKernelGGL(live_scan_kernel, dim3(1), dim3(1024), 0, e->stream, dg, (const float *)d_st, n, d_base, d_total);
        RA_HIP(hipGetLastError());
        int total = 0;
        RA_HIP(hipMemcpyAsync(&total, d_total, sizeof(int), hipMemcpyDeviceToHost, e->stream));
        RA_HIP(hipStreamSynchronize(e->stream));
        if (total < 0 || (size_t)total > (size_t)n * e->geo.nshift) { g_last_error = "ra_debug_finalize: live_scan_kernel left an impossible total"; return RA_ERR_HIP; }
        entries = (size_t)total;
        dg.ent_base = d_base; dg.ent_total = d_total;
    }
    RA_HIP(bufs.get(&d_cand, entries * nrtile + 8));
    RA_HIP(hipMemsetAsync(d_cand, 0, (entries * nrtile + 8) * sizeof(CandT), e->stream));
    if (entries) RA_HIP(hipMemcpyAsync(d_cand, h_cand, entries * nrtile * sizeof(CandT), hipMemcpyHostToDevice, e->stream));
    if (kernel == 1)
        hipLaunchKernelGGL(finalize_wave_kernel, dim3(n), dim3(64), 0, e->stream, dg, (const CandT *)d_cand, nrtile, n, d_st, d_res, d_rl, d_cnt, refine_thr, 0);
    else
        hipLaunchKernelGGL(finalize_kernel, dim3((n + 127) / 128), dim3(128), 0, e->stream, dg, (const CandT *)d_cand, nrtile, n, d_st, d_res,
                           (const float *)e->d_cs, d_rl, d_cnt, refine_thr, 0);
    RA_HIP(hipGetLastError());
    int count = 0;
    RA_HIP(hipMemcpyAsync(&count, d_cnt, sizeof(int), hipMemcpyDeviceToHost, e->stream));
    RA_HIP(hipMemcpyAsync(h_res, d_res, (size_t)n * sizeof(ra_result), hipMemcpyDeviceToHost, e->stream));
    RA_HIP(hipMemcpyAsync(h_state_out, d_st, (size_t)2 * n * sizeof(float), hipMemcpyDeviceToHost, e->stream));
    RA_HIP(hipStreamSynchronize(e->stream));
    if (count < 0 || count > n) { g_last_error = "ra_debug_finalize: the refine list has an impossible count"; return RA_ERR_HIP; }
    if (h_rlist && count) RA_HIP(hipMemcpy(h_rlist, d_rl, (size_t)count * sizeof(RefineRec), hipMemcpyDeviceToHost));
    *h_count = count;
    return RA_OK;
}

extern "C" int ra_debug_refine(ra_engine *e, const float *d_particles, int n, const void *h_rlist, int count, float *d_state,
                               ra_result *d_result, const int *d_cls)
{
    if (!e || !d_particles || !h_rlist || !d_state || !d_result || n < 1 || count < 1 || count > RA_DEBUG_MAX_N) {
        g_last_error = "ra_debug_refine: bad argument";
        return RA_ERR_ARG;
    }
    if (!debug_refine_ready(e)) return RA_ERR_STATE;
    const int nref = e->cfg.nref, nshift = e->geo.nshift;
    const RefineRec *recs = static_cast<const RefineRec *>(h_rlist);
    for (int i = 0; i < count; i++) {          // every index the kernel follows stays inside the engine's tables
        const RefineRec &r = recs[i];
        bool ok = r.p >= 0 && r.p < n && r.ref >= 0 && r.ref < nref && r.bs >= 0 && r.bs < nshift && r.nalt >= 0 && r.nalt <= RA_TIE_ALTS &&
                  (r.mirror == 0 || r.mirror == 1);
        for (int a = 0; ok && a < r.nalt; a++)
            ok = r.alt[a].bs >= 0 && r.alt[a].bs < nshift && (r.alt[a].refmir & 0xffff) < nref && (r.alt[a].refmir >> 16 == 0 || r.alt[a].refmir >> 16 == 1);
        if (!ok) { g_last_error = "ra_debug_refine: a record points outside the engine's tables"; return RA_ERR_ARG; }
    }
    if (d_cls) {
        std::vector<int> cls((size_t)n);
        RA_HIP(hipStreamSynchronize(e->stream));
        RA_HIP(hipMemcpy(cls.data(), d_cls, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
        for (int c : cls)
            if (c < 0 || c >= nref) { g_last_error = "ra_debug_refine: a class outside the engine's references"; return RA_ERR_ARG; }
    }
    DebugBufs bufs;
    RefineRec *d_rl = nullptr;
    int *d_cnt = nullptr;
    RA_HIP(bufs.get(&d_rl, (size_t)count));
    RA_HIP(bufs.get(&d_cnt, 1));
    RA_HIP(hipMemcpyAsync(d_rl, h_rlist, (size_t)count * sizeof(RefineRec), hipMemcpyHostToDevice, e->stream));
    RA_HIP(hipMemcpyAsync(d_cnt, &count, sizeof(int), hipMemcpyHostToDevice, e->stream));
    const auto k = e->refine_gm ? refine_winner_kernel<true> : refine_winner_kernel<false>;
    hipLaunchKernelGGL(k, dim3(std::min(count, e->refine_grid)), dim3(RA_EXACT_THREADS), e->lds_refine, e->stream, e->dg, (const int *)e->d_numr,
                       (const float *)e->d_twx, (const int *)e->d_twxoff, d_particles, (const float *)e->d_refx, (const RefineRec *)d_rl,
                       (const int *)d_cnt, d_result, d_cls, d_state, e->d_rscratch);
    RA_HIP(hipGetLastError());
    RA_HIP(hipStreamSynchronize(e->stream));
    return RA_OK;
}
