// CTF correction on the caller's stream (ralign_ctf.h, ralign_wiener.h): the engine-less ra_phase_flip and ra_wiener_* entry points
// of libralign_hip.so.  The Wiener path transforms its particles with ra_rot_shift2d through the C ABI.
#include "ralign_host.h"
#include "ralign_wiener.h"

using namespace ralign;

// ---- CTF phase flip (ralign_ctf.h)

// the [n][9] CTF rows (host memory) within the ranges the flip and the Wiener averages accept; sets the last error naming the row
static bool pf_rows_ok(const char *what, const float *ctf, int n)
{
    for (int i = 0; i < n; i++) {
        const float *c = ctf + (size_t)i * 9;
        bool finite = true;
        for (int j = 0; j < 9; j++) finite = finite && std::isfinite(c[j]);
        if (!finite || c[0] <= 0.f || c[1] <= 0.f || c[5] <= 0.f || c[7] < 0.f || c[7] >= 1.f) {
            char buf[256];
            snprintf(buf, sizeof(buf), "%s: CTF row %d out of range (needs finite values, D > 0, Apix > 0, "
                     "voltage > 0, 0 <= w < 1)", what, i);
            set_error(buf);
            return false;
        }
    }
    return true;
}

// The kernels specialised for the boxes (nx, pad) of PF_FIXED_BOXES, for the phase flip and for the Wiener forward transform
// alike; nullptr: any other box runs the kernel that takes the plan as an argument.
static const void *pf_fixed_fn(int nx, int pad, bool wiener)
{
    switch (nx * 2 + pad) {
#define PF_FIXED_CASE(NX, PAD) \
    case NX * 2 + PAD: return wiener ? (const void *)wn_forward_fixed_kernel<NX, PAD> : (const void *)phase_flip_fixed_kernel<NX, PAD>;
    PF_FIXED_BOXES(PF_FIXED_CASE)
#undef PF_FIXED_CASE
    default: return nullptr;
    }
}

extern "C" int ra_phase_flip(float *d_images, int n, int nx, const float *ctf, int pad, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 0 || nx < 2 || nx > 1024 || (pad != 0 && pad != 1)) return arg_error("ra_phase_flip: need n >= 0, 2 <= nx <= 1024 and pad 0 or 1");
    if (n == 0) return RA_OK;
    if (!d_images || !ctf) return arg_error("ra_phase_flip: null argument");
    if (!pf_rows_ok("ra_phase_flip", ctf, n)) return RA_ERR_ARG;
    const PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nb < 1) return arg_error("ra_phase_flip: no plan for this box");
    const void *fk = pf_fixed_fn(nx, pad, false);
    const bool fixed = fk != nullptr;
    if (!fixed) fk = pl.gblk ? (const void *)phase_flip_kernel<true> : (const void *)phase_flip_kernel<false>;
    if (const int rc = raise_dynamic_lds(nullptr, fk, fixed ? "phase_flip_fixed_kernel" : "phase_flip_kernel", (size_t)pl.lds)) return rc;
    const int grid = pl.gblk ? pf_gblk_grid(pl, n) : n;
    StreamScratch scratch(stream);
    float *d_ctf = scratch.get<float>((size_t)n * 9);
    float2 *d_scr = pl.gblk ? scratch.get<float2>((size_t)grid * nx * pl.H) : nullptr;
    hipError_t he = scratch.status();
    // the table is pageable host memory of the caller: hipMemcpyAsync stages such a copy before it returns, so the caller may free
    // it as soon as this call returns (a caller passing PINNED memory must keep it alive until the stream has run the copy)
    if (he == hipSuccess) he = hipMemcpyAsync(d_ctf, ctf, (size_t)n * 9 * sizeof(float), hipMemcpyHostToDevice, stream);
    if (he == hipSuccess) {
        void *args_fixed[] = {&d_images, &n, &d_ctf, &d_scr};
        PfPlan pl_arg = pl;
        void *args_plan[] = {&d_images, &n, &d_ctf, &pl_arg, &d_scr};
        he = hipLaunchKernel(fk, dim3(grid), dim3(PF_THREADS), fixed ? args_fixed : args_plan, pl.lds, stream);
        if (he == hipSuccess) he = hipGetLastError();
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_phase_flip", he);
}

// ---- CTF-corrected (Wiener) class averages (ralign_wiener.h)

// step 1 of ra_wiener_accumulate / ra_wiener_score: the table and the particles' classes, finiteness and CTF constants on the
// device (the caller's scratch); the verdict and the classes come back (a stream synchronisation) before the caller launches anything else
struct WnPrep {
    WnCtf *d_cst = nullptr;
    int *d_lab = nullptr;
    std::vector<int> lab;           // [n] classes, then the lowest offending index (n: none)
};

static int wn_prepare(const char *fn, const ra_result *d_params, const float *h_ctf, int n, int nx, int P, int k, hipStream_t stream,
                      StreamScratch &scratch, WnPrep &w)
{
    w.lab.assign((size_t)n + 1, 0);
    float *d_ctf = scratch.get<float>((size_t)n * 9);
    w.d_cst = scratch.get<WnCtf>(n);
    w.d_lab = scratch.get<int>((size_t)n + 1);
    hipError_t he = scratch.status();
    if (he == hipSuccess) he = hipMemcpyAsync(d_ctf, h_ctf, (size_t)n * 9 * sizeof(float), hipMemcpyHostToDevice, stream);
    if (he == hipSuccess) he = hipMemsetD32Async((hipDeviceptr_t)(w.d_lab + n), n, 1, stream);
    RA_LAUNCH(he, wn_prep_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_params, (const float *)d_ctf, n, nx, P, k,
                  w.d_cst, w.d_lab, w.d_lab + n);
    if (he == hipSuccess) he = hipMemcpyAsync(w.lab.data(), w.d_lab, ((size_t)n + 1) * sizeof(int), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he != hipSuccess) return hip_error(fn, he);
    if (w.lab[n] < n) {
        const int i = w.lab[n];
        char buf[256];
        if (w.lab[i] < 0 || w.lab[i] >= k)
            snprintf(buf, sizeof(buf), "%s: particle %d has class label %d outside 0 .. %d", fn, i, w.lab[i], k - 1);
        else
            snprintf(buf, sizeof(buf), "%s: particle %d has non-finite params (alpha, sx, sy)", fn, i);
        set_error(buf);
        return RA_ERR_ARG;
    }
    return RA_OK;
}

// particles per chunk of ra_wiener_accumulate / ra_wiener_score: the spectra and aligned images of one chunk fit the scratch budget
static int wn_chunk(int n, size_t ph, int npix)
{
    return (int)std::max<size_t>(1, std::min<size_t>((size_t)n, WN_SCRATCH_BYTES / (ph * sizeof(float2) + (size_t)npix * sizeof(float))));
}

// the stable counting sort by class of the chunk [c0, c0 + cnt): start [k + 1] the first rank of every class, perm[c0 + rank] the
// particle (index within the chunk) at that rank
static void wn_sort_chunk(const std::vector<int> &lab, int c0, int cnt, int k, std::vector<int> &start, std::vector<int> &perm)
{
    std::fill(start.begin(), start.end(), 0);
    for (int i = 0; i < cnt; i++) start[lab[c0 + i] + 1]++;
    for (int j = 0; j < k; j++) start[j + 1] += start[j];
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int i = 0; i < cnt; i++) perm[c0 + fill[lab[c0 + i]]++] = i;
}

// what ra_wiener_accumulate and ra_wiener_score walk their chunks with: the forward kernel of the box and the chunk's buffers
struct WnChunk {
    const void *fk = nullptr;
    bool fixed = false;
    int fgrid = 0;                  // workgroups of the global-block route
    float *d_al = nullptr;          // [C][nx][nx] aligned images
    float2 *d_spec = nullptr;       // [C][P][H] their spectra
    float2 *d_gscr = nullptr;
    int *d_perm = nullptr;          // [n] wn_sort_chunk's order, uploaded
};

// RA_OK with w filled for chunks of C particles, else the error
static int wn_chunk_buffers(const char *fn, const PfPlan &pl, int nx, int pad, int n, int C, const std::vector<int> &perm, hipStream_t stream,
                            StreamScratch &scratch, WnChunk &w)
{
    const int npix = nx * nx;
    const size_t ph = (size_t)pl.P * pl.H;
    w.fk = pf_fixed_fn(nx, pad, true);
    w.fixed = w.fk != nullptr;
    if (!w.fk) w.fk = pl.gblk ? (const void *)wn_forward_kernel<true> : (const void *)wn_forward_kernel<false>;
    w.fgrid = pl.gblk ? pf_gblk_grid(pl, C) : 0;
    if (const int rc = raise_dynamic_lds(nullptr, w.fk, "wn_forward_kernel", (size_t)pl.lds)) return rc;
    w.d_al = scratch.get<float>((size_t)C * npix);
    w.d_spec = scratch.get<float2>((size_t)C * ph);
    if (pl.gblk) w.d_gscr = scratch.get<float2>((size_t)w.fgrid * nx * pl.H);
    w.d_perm = scratch.get<int>(n);
    hipError_t he = scratch.status();
    // pageable host source: hipMemcpyAsync stages it before it returns
    if (he == hipSuccess) he = hipMemcpyAsync(w.d_perm, perm.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, stream);
    return he == hipSuccess ? RA_OK : hip_error(fn, he);
}

// rot_shift2D of the chunk's cnt particles from c0 on, then their forward transforms into w.d_spec
static int wn_align_transform(const char *fn, const WnChunk &w, const PfPlan &pl, const float *d_images, int nx, const ra_result *d_params,
                              int c0, int cnt, hipStream_t stream)
{
    if (const int rc = ra_rot_shift2d(d_images + (size_t)c0 * nx * nx, cnt, nx, d_params + c0, w.d_al, stream)) return rc;
    const float *al = w.d_al;
    float2 *d_spec = w.d_spec, *d_gscr = w.d_gscr;
    void *args_fixed[] = {&al, &cnt, &d_spec, &d_gscr};
    PfPlan pl_arg = pl;
    void *args_plan[] = {&al, &cnt, &d_spec, &pl_arg, &d_gscr};
    hipError_t he = hipLaunchKernel(w.fk, dim3(pl.gblk ? std::min(w.fgrid, cnt) : cnt), dim3(PF_THREADS), w.fixed ? args_fixed : args_plan, pl.lds, stream);
    if (he == hipSuccess) he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error(fn, he);
}

extern "C" int ra_wiener_accumulate(const float *d_images, int n, int nx, const ra_result *d_params, const float *h_ctf, int pad,
                                    int flipped, int k, float *d_num, float *d_den, int *d_counts, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 0 || nx < 2 || nx > 1024 || (pad != 0 && pad != 1) || (flipped != 0 && flipped != 1) || k < 1 || k > 1024)
        return arg_error("ra_wiener_accumulate: need n >= 0, 2 <= nx <= 1024, pad and flipped 0 or 1, 1 <= k <= 1024");
    if (n == 0) return RA_OK;
    if (!d_images || !d_params || !h_ctf || !d_num || !d_den || !d_counts) return arg_error("ra_wiener_accumulate: null argument");
    if (!pf_rows_ok("ra_wiener_accumulate", h_ctf, n)) return RA_ERR_ARG;
    const PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nb < 1) return arg_error("ra_wiener_accumulate: no plan for this box");
    const int P = pl.P, H = pl.H, npix = nx * nx;
    const size_t ph = (size_t)P * H;

    // 1. classes, finiteness and CTF constants on the device; the verdict and the classes come back before anything is summed
    StreamScratch scratch(stream);
    WnPrep prep;
    if (const int rc = wn_prepare("ra_wiener_accumulate", d_params, h_ctf, n, nx, P, k, stream, scratch, prep)) return rc;

    // 2. chunks within the scratch budget; per chunk the members of every class in particle order, cut into runs so that the
    //    reduce has enough workgroups (element blocks x runs ~ WN_BLOCKS_TARGET); a class of several runs gets partial slots
    const int eblk = (int)((ph + WN_THREADS - 1) / WN_THREADS);
    const int T = std::max(1, std::min(WN_MAX_RUNS, WN_BLOCKS_TARGET / eblk));
    const int C = wn_chunk(n, ph, npix);
    std::vector<int> perm(n), start(k + 1), run0, seg0;        // run0, seg0: per chunk the first run / seg
    std::vector<WnRun> runs;
    std::vector<int4> segs;
    int slots = 0;
    for (int c0 = 0; c0 < n; c0 += C) {
        const int cnt = std::min(C, n - c0), L = (cnt + T - 1) / T;
        run0.push_back((int)runs.size());
        seg0.push_back((int)segs.size());
        wn_sort_chunk(prep.lab, c0, cnt, k, start, perm);
        int slot = 0;
        for (int j = 0; j < k; j++) {
            const int b = start[j], e = start[j + 1], s = e - b;
            if (s == 0) continue;
            if (s <= L) { runs.push_back(WnRun{j, b, e, -1}); continue; }
            const int s0 = slot;
            for (int r = b; r < e; r += L) runs.push_back(WnRun{j, r, std::min(e, r + L), slot++});
            segs.push_back(make_int4(j, s0, slot, s));
        }
        slots = std::max(slots, slot);
    }
    run0.push_back((int)runs.size());
    seg0.push_back((int)segs.size());

    // 3. per chunk: rot_shift2D, forward transforms, reduce, combine
    WnChunk ch;
    if (const int rc = wn_chunk_buffers("ra_wiener_accumulate", pl, nx, pad, n, C, perm, stream, scratch, ch)) return rc;
    float2 *d_pnum = slots ? scratch.get<float2>((size_t)slots * ph) : nullptr;
    float *d_pden = slots ? scratch.get<float>((size_t)slots * ph) : nullptr;
    WnRun *d_runs = scratch.get<WnRun>(runs.size());
    int4 *d_segs = segs.empty() ? nullptr : scratch.get<int4>(segs.size());
    hipError_t he = scratch.status();
    // pageable host sources: hipMemcpyAsync stages them before it returns
    if (he == hipSuccess) he = hipMemcpyAsync(d_runs, runs.data(), runs.size() * sizeof(WnRun), hipMemcpyHostToDevice, stream);
    if (he == hipSuccess && !segs.empty()) he = hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(int4), hipMemcpyHostToDevice, stream);
    for (int c = 0, c0 = 0; c0 < n && he == hipSuccess; c++, c0 += C) {
        const int cnt = std::min(C, n - c0);
        if (const int rc = wn_align_transform("ra_wiener_accumulate", ch, pl, d_images, nx, d_params, c0, cnt, stream)) return rc;
        const int nrun = run0[c + 1] - run0[c], nseg = seg0[c + 1] - seg0[c];
        hipLaunchKernelGGL(wn_reduce_kernel, dim3(eblk, nrun), dim3(WN_THREADS), 0, stream, (const float2 *)ch.d_spec, P, H,
                           (const WnRun *)(d_runs + run0[c]), (const int *)(ch.d_perm + c0), (const WnCtf *)(prep.d_cst + c0), flipped,
                           (float2 *)d_num, d_den, d_counts, d_pnum, d_pden);
        he = hipGetLastError();
        if (nseg) RA_LAUNCH(he, wn_combine_kernel, dim3(eblk, nseg), dim3(WN_THREADS), 0, stream, P, H, (const int4 *)(d_segs + seg0[c]),
                      (const float2 *)d_pnum, (const float *)d_pden, (float2 *)d_num, d_den, d_counts);
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_wiener_accumulate", he);
}

// a finalize kernel's launch: one workgroup per class, or, when the plan keeps its block in global scratch, a grid of scratch
// blocks that loops over the classes; args(pl_arg, d_gscr) gives the kernel's argument pointers
template <class Args>
static int wn_finalize_launch(const char *what, const PfPlan &pl, const void *fk, int k, hipStream_t stream, Args args)
{
    if (const int rc = raise_dynamic_lds(nullptr, fk, what, (size_t)pl.lds)) return rc;
    const int grid = pl.gblk ? pf_gblk_grid(pl, k) : k;
    StreamScratch scratch(stream);
    float2 *d_gscr = pl.gblk ? scratch.get<float2>((size_t)grid * pl.nx * pl.H) : nullptr;
    hipError_t he = scratch.status();
    if (he == hipSuccess) {
        PfPlan pl_arg = pl;
        std::vector<void *> a = args(pl_arg, d_gscr);
        he = hipLaunchKernel(fk, dim3(grid), dim3(PF_THREADS), a.data(), pl.lds, stream);
        if (he == hipSuccess) he = hipGetLastError();
    }
    return he == hipSuccess ? RA_OK : hip_error(what, he);
}

extern "C" int ra_wiener_finalize(const float *d_num, const float *d_den, const int *d_counts, int k, int nx, int pad, float snr,
                                  int min_count, float *d_out, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (k < 1 || k > 1024 || nx < 2 || nx > 1024 || (pad != 0 && pad != 1) || !(snr > 0.f) || !std::isfinite(snr))
        return arg_error("ra_wiener_finalize: need 1 <= k <= 1024, 2 <= nx <= 1024, pad 0 or 1 and a finite snr > 0");
    if (!d_num || !d_den || !d_counts || !d_out) return arg_error("ra_wiener_finalize: null argument");
    const PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nb < 1) return arg_error("ra_wiener_finalize: no plan for this box");
    const void *fk = pl.gblk ? (const void *)wn_finalize_kernel<true> : (const void *)wn_finalize_kernel<false>;
    const float2 *num = (const float2 *)d_num;
    float inv_snr = 1.0f / snr;
    return wn_finalize_launch("ra_wiener_finalize", pl, fk, k, stream, [&](PfPlan &pl_arg, float2 *&d_gscr) -> std::vector<void *> {
        return {&num, &d_den, &d_counts, &k, &inv_snr, &min_count, &d_out, &pl_arg, &d_gscr};
    });
}

// ---- half-set FRC and SSNR-weighted averages (ralign_wiener.h)

extern "C" int ra_wiener_frc(const float *d_num2, const float *d_den2, const int *d_counts2, int k, int nx, int pad, float snr,
                             int min_count, float ssnr_floor, double *d_frc, float *d_reg, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (k < 1 || k > 512 || nx < 2 || nx > 1024 || (pad != 0 && pad != 1) || !(snr > 0.f) || !std::isfinite(snr) ||
        !(ssnr_floor > 0.f) || !std::isfinite(ssnr_floor))
        return arg_error("ra_wiener_frc: need 1 <= k <= 512, 2 <= nx <= 1024, pad 0 or 1, a finite snr > 0 and a finite ssnr_floor > 0");
    if (!d_num2 || !d_den2 || !d_counts2 || !d_frc || !d_reg) return arg_error("ra_wiener_frc: null argument");
    const int P = pad ? 2 * nx : nx, S = P / 2 + 1;
    // row blocks of `rows` rows, about WN_FRC_BLOCKS workgroups over all classes, none of them empty
    const int want = std::max(1, std::min(std::min(P, WN_FRC_MAX_ROW_BLOCKS), WN_FRC_BLOCKS / k));
    const int rows = (P + want - 1) / want, nb = (P + rows - 1) / rows;
    const int threads = std::min(WN_THREADS, (S + 63) / 64 * 64);
    StreamScratch scratch(stream);
    double *d_part = scratch.get<double>((size_t)k * nb * 5 * S);
    hipError_t he = scratch.status();
    RA_LAUNCH(he, wn_frc_rows_kernel, dim3(nb, k), dim3(threads), 0, stream, (const float2 *)d_num2, d_den2, P, rows,
                  1.0 / (double)snr, d_part);
    RA_LAUNCH(he, wn_frc_combine_kernel, dim3((S + WN_THREADS - 1) / WN_THREADS, k), dim3(WN_THREADS), 0, stream,
                  (const double *)d_part, nb, S, d_counts2, min_count, ssnr_floor, d_frc, d_reg);
    return he == hipSuccess ? RA_OK : hip_error("ra_wiener_frc", he);
}

extern "C" int ra_wiener_finalize_ssnr(const float *d_num2, const float *d_den2, const int *d_counts2, const float *d_reg, int k, int nx,
                                       int pad, int min_count, float *d_out, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (k < 1 || k > 512 || nx < 2 || nx > 1024 || (pad != 0 && pad != 1))
        return arg_error("ra_wiener_finalize_ssnr: need 1 <= k <= 512, 2 <= nx <= 1024 and pad 0 or 1");
    if (!d_num2 || !d_den2 || !d_counts2 || !d_reg || !d_out) return arg_error("ra_wiener_finalize_ssnr: null argument");
    const PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nb < 1) return arg_error("ra_wiener_finalize_ssnr: no plan for this box");
    const void *fk = pl.gblk ? (const void *)wn_finalize_ssnr_kernel<true> : (const void *)wn_finalize_ssnr_kernel<false>;
    const float2 *num2 = (const float2 *)d_num2;
    return wn_finalize_launch("ra_wiener_finalize_ssnr", pl, fk, k, stream, [&](PfPlan &pl_arg, float2 *&d_gscr) -> std::vector<void *> {
        return {&num2, &d_den2, &d_counts2, &d_reg, &k, &min_count, &d_out, &pl_arg, &d_gscr};
    });
}

// ---- per-particle agreement scores (ralign_wiener.h)

extern "C" int ra_wiener_score(const float *d_images, int n, int nx, const ra_result *d_params, const float *h_ctf, int pad, int flipped,
                               int k, const float *d_num, const float *d_den, const int *d_counts, float snr, const float *d_reg,
                               int leave_one_out, int s_lo, int s_hi, double *d_sums, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 0 || nx < 2 || nx > 1024 || (pad != 0 && pad != 1) || (flipped != 0 && flipped != 1) || k < 1 || k > 1024 ||
        (leave_one_out != 0 && leave_one_out != 1))
        return arg_error("ra_wiener_score: need n >= 0, 2 <= nx <= 1024, pad, flipped and leave_one_out 0 or 1, 1 <= k <= 1024");
    if (s_lo < 0 || s_lo > s_hi || s_hi > (pad ? 2 * nx : nx) / 2) return arg_error("ra_wiener_score: need 0 <= s_lo <= s_hi <= P/2");
    if (d_reg ? k > 512 : (!(snr > 0.f) || !std::isfinite(snr)))
        return arg_error("ra_wiener_score: need a finite snr > 0, or a per-shell term with k <= 512");
    if (n == 0) return RA_OK;
    if (!d_images || !d_params || !h_ctf || !d_num || !d_den || !d_counts || !d_sums) return arg_error("ra_wiener_score: null argument");
    if (!pf_rows_ok("ra_wiener_score", h_ctf, n)) return RA_ERR_ARG;
    const PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nb < 1) return arg_error("ra_wiener_score: no plan for this box");
    const int P = pl.P, H = pl.H, npix = nx * nx;
    const size_t ph = (size_t)P * H;

    // 1. as ra_wiener_accumulate: the verdict on labels and params before anything is written
    StreamScratch scratch(stream);
    WnPrep prep;
    if (const int rc = wn_prepare("ra_wiener_score", d_params, h_ctf, n, nx, P, k, stream, scratch, prep)) return rc;

    // 2. the accumulate's chunks; in each the particles in class order (stable), so that a class's sums are read while they are hot
    const int C = wn_chunk(n, ph, npix);
    std::vector<int> perm(n), start(k + 1);
    for (int c0 = 0; c0 < n; c0 += C) wn_sort_chunk(prep.lab, c0, std::min(C, n - c0), k, start, perm);

    // 3. per chunk: rot_shift2D, forward transforms, scores
    WnChunk ch;
    if (const int rc = wn_chunk_buffers("ra_wiener_score", pl, nx, pad, n, C, perm, stream, scratch, ch)) return rc;
    const double tau = d_reg ? 0.0 : 1.0 / (double)snr;
    hipError_t he = hipSuccess;
    for (int c0 = 0; c0 < n && he == hipSuccess; c0 += C) {
        const int cnt = std::min(C, n - c0);
        if (const int rc = wn_align_transform("ra_wiener_score", ch, pl, d_images, nx, d_params, c0, cnt, stream)) return rc;
        hipLaunchKernelGGL(wn_score_kernel, dim3(cnt), dim3(WN_THREADS), 0, stream, (const float2 *)ch.d_spec, P, H,
                           (const int *)(ch.d_perm + c0), (const int *)(prep.d_lab + c0), (const WnCtf *)(prep.d_cst + c0), flipped,
                           (const float2 *)d_num, d_den, d_counts, tau, d_reg, leave_one_out, s_lo, s_hi, d_sums + (size_t)c0 * 3);
        he = hipGetLastError();
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_wiener_score", he);
}
