// CTF-corrected (Wiener-filtered) class averages (ra_wiener_accumulate / ra_wiener_finalize).
//
// Contract (cryo_ralib_amd/wiener.py: wiener_reference): per particle i, y_i = rot_shift2D(x_i), embedded at o = (P - nx) / 2 in a
// P x P zero image, Y_i = rfft2 on the [P][P/2 + 1] grid; c_i = the CTF of the particle's [9] row with the astigmatism angle taken
// into the aligned frame (DefocusAngle - alpha, or alpha - DefocusAngle for a mirrored particle); w_i = c_i, or |c_i| for
// phase-flipped particles.  Per class j: N_j = sum w_i Y_i, D_j = sum c_i^2, A_j = crop_o(irfft2(N_j / (D_j + 1/snr))).
//
// Accumulation, per chunk of particles (its size fixed by a scratch budget, never by n):
//   1. wn_prep_kernel: per particle the CTF constants in the aligned frame (double, kept on the device for the chunk kernels) and
//      its class; labels outside 0 .. k-1 or non-finite alpha / sx / sy are reported (lowest index) before anything is summed;
//   2. ra_rot_shift2d's transform of the chunk into scratch;
//   3. wn_forward_kernel: the phase flip's forward row pass (ralign_ctf.h) and forward column FFTs of the P/2 + 1 columns, the
//      spectrum [H][P] (column-major) of every particle written to scratch unweighted;
//   4. wn_reduce_kernel: one thread per spectrum element and one workgroup row per run of class members (the chunk's particles
//      sorted stably by class on the host): sum w Y and c^2 over the run in double, in particle order, with c recomputed from the
//      constants; a class of one run adds straight into d_num / d_den, the runs of a longer class go to partial slots that
//   5. wn_combine_kernel adds in run order.  Every accumulator element has one owner per launch: no atomics on the sums, a fixed
//      association, bitwise reproducible.
// Finalize: wn_finalize_kernel, one workgroup per class (looping when the block lives in global scratch): N / (D + 1/snr) into
// inverse column FFTs over the full height (N is dense), the nx window rows kept, then the phase flip's inverse row pass.
//
// Half-set FRC and SSNR-weighted finalize (ra_wiener_frc / ra_wiener_finalize_ssnr; contract: wiener.py
// ssnr_reference).  The half sums are ra_wiener_accumulate's with labels 2j + h and 2k classes, so class j's halves are slots 2j and
// 2j + 1 of num2 / den2 / counts2.  Shell s = floor(r + 0.5) of element (iy, ix), r = |(ix, ky)|, ky the signed row frequency;
// shells 0 .. P/2 take part in the sums, with the Hermitian weight g = 1 on column 0 (and P/2 for even P), 2 elsewhere.
//   1. wn_frc_rows_kernel: one workgroup per (row block, class), one thread per shell; the thread walks the block's rows in order
//      and, in each row, the columns of its shell (a contiguous run: s does not decrease along a row), summing in double
//      g Re(V0 conj V1), g |V0|^2, g |V1|^2, g (D0 + D1) and g, V_h = N_h / (D_h + 1/snr), into the block's partial slot;
//   2. wn_frc_combine_kernel: one thread per (class, shell) adds the row blocks' slots in block order, then the FRC and
//      R = mean(D0 + D1) / max(2F / (1 - F), floor), F = min(FRC, 0.999);
//   3. wn_finalize_ssnr_kernel: wn_finalize_kernel's transforms of (N0 + N1) / (D0 + D1 + R(min(s, P/2))).
// One writer per output element and a fixed order of every sum: bitwise reproducible.
//
// Per-particle agreement scores (ra_wiener_score; contract: wiener.py score_reference).  Per chunk, steps
// 1 - 3 of the accumulation (the same kernels), then wn_score_kernel: one workgroup per particle, the chunk's particles in class
// order (a class's N, D stay in L2 while its members are scored; the result does not depend on it).  The workgroup walks the
// spectrum in 16 x 16 tiles (columns kx outer, rows n inner), each wave an 8 x 8 quarter, so that the particle's spectrum ([H][P])
// and the class sums ([P][H]) are both read in 64-byte pieces.  Per element inside the shell band: c from the constants as in
// wn_reduce_kernel, the rest of the class's estimate M = w (N - w Y) / (max(D - c^2, 0) + tau) in double (N, D as they are
// without leave-one-out), and g Re(Y conj M), g |Y|^2, g |M|^2 added to the thread's three double partials in tile order; then a
// fixed shuffle tree per wave and the four waves' sums added in wave order by one thread, which writes the particle's [3].  A
// particle's sums depend on nothing but its own spectrum, constants and class sums: not on its place in the batch or the chunk.
#pragma once

#include <hip/hip_runtime.h>

#include "ralign_ctf.h"
#include "../../include/ralign.h"

namespace ralign {

#define WN_THREADS 256              // reduce / combine workgroup
#define WN_SCRATCH_BYTES ((size_t)1 << 30)      // spectra + aligned images of one chunk
#define WN_BLOCKS_TARGET 2048       // workgroups the reduce aims for: runs per chunk = this / element blocks, within 1 .. 64
#define WN_MAX_RUNS 64
#define WN_FRC_BLOCKS 1024          // workgroups the FRC row pass aims for over all classes: row blocks = this / k, within 1 .. 64
#define WN_FRC_MAX_ROW_BLOCKS 64

// CTF constants of one particle in the aligned frame, doubles; l3 = lam^3 folded in
struct WnCtf {
    double q, dsum, ddif, c2a, s2a, lam, cl3, phi0;
};

__host__ __device__ inline WnCtf wn_constants(const float *row, int nx, int P, float alpha, int mirror)
{
    const double ang = mirror ? (double)alpha - (double)row[4] : (double)row[4] - (double)alpha;
    const PfCtf c = pf_ctf_constants_at(row, nx, P, ang);
    WnCtf w;
    w.q = c.q; w.dsum = c.dsum; w.ddif = c.ddif; w.c2a = c.c2a; w.s2a = c.s2a; w.lam = c.lam;
    w.cl3 = c.cs * c.lam * c.lam * c.lam;
    w.phi0 = c.phi0;
    return w;
}

// ctf(iy, ix) = sin(gamma - asin w) = sin(2 pi u), u as in pf_multiplier, reduced to [-1/2, 1/2) in double before the float sine
__host__ __device__ inline float wn_ctf(const WnCtf &c, int iy, int ix)
{
    const double x = ix, y = iy, r2 = x * x + y * y;
    double df = c.dsum;
    if (r2 > 0.0) df += c.ddif * (((x * x - y * y) * c.c2a + 2.0 * x * y * c.s2a) / r2);
    const double s2 = r2 * c.q;
    const double u = -0.5 * df * c.lam * s2 + 0.25 * c.cl3 * s2 * s2 - c.phi0;
    double fr = u - floor(u);
    if (fr >= 0.5) fr -= 1.0;
    return sinf(6.28318530717958648f * (float)fr);
}

// the forward transform of one aligned image: img [nx][nx] -> spec [H][P] (column kx, then the P row frequencies)
template <class Ctx>
__host__ __device__ inline void wn_forward(const Ctx &cx, const float *img, float2 *spec, const PfPlan &pl, float2 *blk, float2 *work,
                                           const float2 *tw)
{
    const int nx = pl.nx, P = pl.P, H = pl.H, o = pl.o, nb = pl.nb;
    float2 *wa = work, *wb = work + (size_t)nb * P;
    pf_rows_forward(cx, img, pl, blk, work, tw);
    for (int c0 = 0; c0 < H; c0 += nb) {
        const int cnt = H - c0 < nb ? H - c0 : nb;
        for (int it = cx.tid; it < cnt * P; it += cx.nt) {
            const int t = it / P, n = it - t * P, y = n - o;
            wa[it] = (y >= 0 && y < nx) ? blk[(size_t)y * H + c0 + t] : make_float2(0.f, 0.f);
        }
        cx.sync();
        const float2 *z = pf_fft(cx, wa, wb, cnt, pl, tw, -1.f);
        for (int it = cx.tid; it < cnt * P; it += cx.nt) spec[(size_t)c0 * P + it] = z[it];
        cx.sync();
    }
}

// shell of the rfft-grid element at column ix and signed row frequency ky: s = floor(r + 0.5).  In integers, with r2 = r^2:
// (s - 1/2)^2 <= r2 < (s + 1/2)^2 is s (s - 1) < r2 <= s (s + 1) for s >= 1 (r2 = 0 for s = 0), so a float estimate settled by
// these exact tests gives the shell of the float64 contract without a double square root
__host__ __device__ inline int wn_shell(int ix, int ky)
{
    const int r2 = ix * ix + ky * ky;
    int s = (int)(sqrtf((float)r2) + 0.5f);
    while (s * (s + 1) < r2) s++;
    while (s > 0 && s * (s - 1) >= r2) s--;
    return s;
}

// what ra_wiener_finalize transforms: num / (den + 1/snr) at element e = n * H + kx of one class
struct WnConstSrc {
    const float2 *num;
    const float *den;
    float inv_snr;
    __host__ __device__ float2 operator()(size_t e, int, int) const
    {
        const float g = 1.0f / (den[e] + inv_snr);
        return make_float2(num[e].x * g, num[e].y * g);
    }
};

// what ra_wiener_finalize_ssnr transforms: (N0 + N1) / (D0 + D1 + R(min(s, P/2))) of one class's half sums, 0 where that
// denominator is 0; reg [P/2 + 1] the class's per-shell term
struct WnSsnrSrc {
    const float2 *n0, *n1;
    const float *d0, *d1, *reg;
    int P;
    __host__ __device__ float2 operator()(size_t e, int n, int kx) const
    {
        const int s = wn_shell(kx, n <= P / 2 ? n : n - P), h = P / 2;
        const float d = (d0[e] + d1[e]) + reg[s < h ? s : h];
        if (d == 0.f) return make_float2(0.f, 0.f);
        const float g = 1.0f / d;
        const float2 a = n0[e], b = n1[e];
        return make_float2((a.x + b.x) * g, (a.y + b.y) * g);
    }
};

// one class: src(e, n, kx) the divided spectrum at row n, column kx of [P][H] -> img [nx][nx]; inverse column FFTs, the nx window
// rows into blk, the inverse row pass
template <class Ctx, class Src>
__host__ __device__ inline void wn_class_src(const Ctx &cx, const Src &src, float *img, const PfPlan &pl, float2 *blk, float2 *work,
                                             const float2 *tw)
{
    const int nx = pl.nx, P = pl.P, H = pl.H, o = pl.o, nb = pl.nb;
    float2 *wa = work, *wb = work + (size_t)nb * P;
    for (int c0 = 0; c0 < H; c0 += nb) {
        const int cnt = H - c0 < nb ? H - c0 : nb;
        for (int it = cx.tid; it < cnt * P; it += cx.nt) {
            const int t = it / P, n = it - t * P;
            wa[it] = src((size_t)n * H + c0 + t, n, c0 + t);
        }
        cx.sync();
        const float2 *z = pf_fft(cx, wa, wb, cnt, pl, tw, 1.f);
        for (int it = cx.tid; it < cnt * nx; it += cx.nt) {
            const int t = it / nx, y = it - t * nx;
            blk[(size_t)y * H + c0 + t] = z[(size_t)t * P + o + y];
        }
        cx.sync();
    }
    pf_rows_inverse(cx, img, pl, blk, work, tw);
}

// one class of the constant-snr finalize: num [P][H], den [P][H] -> img [nx][nx]
template <class Ctx>
__host__ __device__ inline void wn_class(const Ctx &cx, const float2 *num, const float *den, float inv_snr, float *img, const PfPlan &pl,
                                         float2 *blk, float2 *work, const float2 *tw)
{
    wn_class_src(cx, WnConstSrc{num, den, inv_snr}, img, pl, blk, work, tw);
}

// per particle: class, finiteness, CTF constants in the aligned frame; *bad = the lowest offending index (n: none)
__global__ void wn_prep_kernel(const ra_result *__restrict__ prm, const float *__restrict__ ctf, int n, int nx, int P, int k,
                               WnCtf *__restrict__ cst, int *__restrict__ lab, int *__restrict__ bad)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const ra_result r = prm[i];
    const bool ok = r.ref_id >= 0 && r.ref_id < k && isfinite(r.alpha) && isfinite(r.sx) && isfinite(r.sy);
    lab[i] = r.ref_id;
    if (!ok) {
        atomicMin(bad, i);
        return;
    }
    cst[i] = wn_constants(ctf + (size_t)i * 9, nx, P, r.alpha, r.mirror != 0);
}

template <bool GBLK>
__device__ inline void wn_forward_body(const float *imgs, int n, float2 *spec, const PfPlan &pl, float2 *gscr)
{
    extern __shared__ float2 pf_lds[];
    const int P = pl.P;
    float2 *tw = pf_lds;
    float2 *work = pf_lds + P;
    float2 *blk = GBLK ? gscr + (size_t)blockIdx.x * pl.nx * pl.H : work + (size_t)2 * pl.nb * P;
    PfCtx cx{(int)threadIdx.x, PF_THREADS};
    for (int t = cx.tid; t < P; t += cx.nt) {
        double s, c;
        sincospi(-2.0 * t / P, &s, &c);
        tw[t] = make_float2((float)c, (float)s);
    }
    __syncthreads();
    for (int p = blockIdx.x; p < n; p += gridDim.x)
        wn_forward(cx, imgs + (size_t)p * pl.nx * pl.nx, spec + (size_t)p * pl.H * P, pl, blk, work, tw);
}

template <bool GBLK>
__global__ __launch_bounds__(PF_THREADS) void wn_forward_kernel(const float *__restrict__ imgs, int n, float2 *__restrict__ spec, PfPlan pl,
                                                                float2 *__restrict__ gscr)
{
    wn_forward_body<GBLK>(imgs, n, spec, pl, gscr);
}

// the boxes the benchmarks know: the plan is a compile-time constant, as for phase_flip_fixed_kernel
template <int NX, int PAD>
__global__ __launch_bounds__(PF_THREADS) void wn_forward_fixed_kernel(const float *__restrict__ imgs, int n, float2 *__restrict__ spec,
                                                                      float2 *__restrict__ gscr)
{
    constexpr PfPlan pl = pf_make_plan(NX, PAD);
    static_assert(pl.nb > 0, "no plan");
    wn_forward_body<pl.gblk != 0>(imgs, n, spec, pl, gscr);
}

// one run of class members: run r = (class, first, end) into perm (chunk-local particle indices sorted by class, stable), dst < 0:
// the class's only run this chunk, added into num / den (and its size into counts); else partial slot dst
struct WnRun {
    int cls, b, e, dst;
};

__global__ __launch_bounds__(WN_THREADS) void wn_reduce_kernel(const float2 *__restrict__ spec, int P, int H, const WnRun *__restrict__ runs,
                                                               const int *__restrict__ perm, const WnCtf *__restrict__ cst, int flipped,
                                                               float2 *__restrict__ num, float *__restrict__ den, int *__restrict__ counts,
                                                               float2 *__restrict__ pnum, float *__restrict__ pden)
{
    const WnRun run = runs[blockIdx.y];
    const size_t ph = (size_t)P * H;
    const int e = blockIdx.x * WN_THREADS + threadIdx.x;
    if (run.dst < 0 && blockIdx.x == 0 && threadIdx.x == 0) counts[run.cls] += run.e - run.b;
    if (e >= (int)ph) return;
    const int kx = e / P, n = e - kx * P;
    const int iy = n < (P + 1) / 2 ? n : n - P;
    double ax = 0.0, ay = 0.0, d = 0.0;
    for (int m = run.b; m < run.e; m++) {
        const int p = perm[m];
        const float c = wn_ctf(cst[p], iy, kx);
        const float w = flipped ? fabsf(c) : c;
        const float2 y = spec[(size_t)p * ph + e];
        ax += (double)(w * y.x);
        ay += (double)(w * y.y);
        d += (double)(c * c);
    }
    if (run.dst < 0) {
        const size_t o = (size_t)run.cls * ph + (size_t)n * H + kx;
        num[o] = make_float2(num[o].x + (float)ax, num[o].y + (float)ay);
        den[o] += (float)d;
    } else {
        const size_t o = (size_t)run.dst * ph + e;
        pnum[o] = make_float2((float)ax, (float)ay);
        pden[o] = (float)d;
    }
}

// a class of several runs: its partial slots [s0, s1) added in order; seg = (class, s0, s1, members)
__global__ __launch_bounds__(WN_THREADS) void wn_combine_kernel(int P, int H, const int4 *__restrict__ segs, const float2 *__restrict__ pnum,
                                                                const float *__restrict__ pden, float2 *__restrict__ num, float *__restrict__ den,
                                                                int *__restrict__ counts)
{
    const int4 s = segs[blockIdx.y];
    const size_t ph = (size_t)P * H;
    const int e = blockIdx.x * WN_THREADS + threadIdx.x;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[s.x] += s.w;
    if (e >= (int)ph) return;
    double ax = 0.0, ay = 0.0, d = 0.0;
    for (int r = s.y; r < s.z; r++) {
        const float2 v = pnum[(size_t)r * ph + e];
        ax += v.x;
        ay += v.y;
        d += pden[(size_t)r * ph + e];
    }
    const int kx = e / P, n = e - kx * P;
    const size_t o = (size_t)s.x * ph + (size_t)n * H + kx;
    num[o] = make_float2(num[o].x + (float)ax, num[o].y + (float)ay);
    den[o] += (float)d;
}

// the finalize of classes blockIdx.x, blockIdx.x + gridDim.x, ...: zeros where live(j) is false, else src(j) (a WnConstSrc or
// WnSsnrSrc) through wn_class_src
template <bool GBLK, class Live, class Src>
__device__ inline void wn_finalize_body(int k, const Live &live, const Src &src, float *out, const PfPlan &pl, float2 *gscr)
{
    extern __shared__ float2 pf_lds[];
    const int P = pl.P, nx = pl.nx;
    float2 *tw = pf_lds;
    float2 *work = pf_lds + P;
    float2 *blk = GBLK ? gscr + (size_t)blockIdx.x * nx * pl.H : work + (size_t)2 * pl.nb * P;
    PfCtx cx{(int)threadIdx.x, PF_THREADS};
    for (int t = cx.tid; t < P; t += cx.nt) {
        double s, c;
        sincospi(-2.0 * t / P, &s, &c);
        tw[t] = make_float2((float)c, (float)s);
    }
    __syncthreads();
    for (int j = blockIdx.x; j < k; j += gridDim.x) {
        float *img = out + (size_t)j * nx * nx;
        if (!live(j)) {
            for (int i = cx.tid; i < nx * nx; i += cx.nt) img[i] = 0.f;
            continue;
        }
        wn_class_src(cx, src(j), img, pl, blk, work, tw);
    }
}

template <bool GBLK>
__global__ __launch_bounds__(PF_THREADS) void wn_finalize_kernel(const float2 *__restrict__ num, const float *__restrict__ den,
                                                                 const int *__restrict__ counts, int k, float inv_snr, int min_count,
                                                                 float *__restrict__ out, PfPlan pl, float2 *__restrict__ gscr)
{
    const size_t ph = (size_t)pl.P * pl.H;
    wn_finalize_body<GBLK>(
        k, [=](int j) { return counts[j] >= min_count; },
        [=](int j) { return WnConstSrc{num + (size_t)j * ph, den + (size_t)j * ph, inv_snr}; }, out, pl, gscr);
}

// num2 [k][2][P][H], den2 [k][2][P][H], counts2 [k][2], reg [k][P/2 + 1]
template <bool GBLK>
__global__ __launch_bounds__(PF_THREADS) void wn_finalize_ssnr_kernel(const float2 *__restrict__ num2, const float *__restrict__ den2,
                                                                      const int *__restrict__ counts2, const float *__restrict__ reg, int k,
                                                                      int min_count, float *__restrict__ out, PfPlan pl,
                                                                      float2 *__restrict__ gscr)
{
    const int P = pl.P;
    const size_t ph = (size_t)P * pl.H;
    wn_finalize_body<GBLK>(
        k, [=](int j) { return counts2[2 * j] + counts2[2 * j + 1] >= min_count; },
        [=](int j) {
            const size_t a = (size_t)2 * j * ph;
            return WnSsnrSrc{num2 + a, num2 + a + ph, den2 + a, den2 + a + ph, reg + (size_t)j * (P / 2 + 1), P};
        },
        out, pl, gscr);
}

// the five sums of shell s over rows [y0, y1) of one class's halves n0 / n1, d0 / d1 ([P][P/2 + 1]), rows in order and in each row
// the shell's columns in order: a = (g Re(V0 conj V1), g |V0|^2, g |V1|^2, g (D0 + D1), g), V_h = N_h / (D_h + 1/snr)
__host__ __device__ inline void wn_frc_shell_rows(const float2 *n0, const float2 *n1, const float *d0, const float *d1, int P, int y0,
                                                  int y1, int s, double inv_snr, double *a)
{
    const int H = P / 2 + 1;
    double xr = 0.0, a0 = 0.0, a1 = 0.0, dd = 0.0, gg = 0.0;
    for (int iy = y0; iy < y1; iy++) {
        const int ky = iy <= P / 2 ? iy : iy - P;
        if (ky > s || -ky > s) continue;            // r >= |ky| >= s + 1
        // the shell's columns: lo < ix^2 + ky^2 <= hi (wn_shell's bounds; every column from 0 for s = 0); the first one from a
        // float estimate settled by the exact tests
        const int k2 = ky * ky, lo = s * (s - 1), hi = s * (s + 1);
        int ix = 0;
        if (s > 0) {
            ix = lo - k2 > 0 ? (int)sqrtf((float)(lo - k2)) : 0;
            if (ix > H) ix = H;
            while (ix > 0 && (ix - 1) * (ix - 1) + k2 > lo) ix--;
            while (ix < H && ix * ix + k2 <= lo) ix++;
        }
        for (; ix < H && ix * ix + k2 <= hi; ix++) {
            const size_t e = (size_t)iy * H + ix;
            const double g = (ix == 0 || 2 * ix == P) ? 1.0 : 2.0;
            const double q0 = 1.0 / ((double)d0[e] + inv_snr), q1 = 1.0 / ((double)d1[e] + inv_snr);
            const float2 u = n0[e], v = n1[e];
            const double ux = u.x * q0, uy = u.y * q0, vx = v.x * q1, vy = v.y * q1;
            xr += g * (ux * vx + uy * vy);
            a0 += g * (ux * ux + uy * uy);
            a1 += g * (vx * vx + vy * vy);
            dd += g * ((double)d0[e] + (double)d1[e]);
            gg += g;
        }
    }
    a[0] = xr; a[1] = a0; a[2] = a1; a[3] = dd; a[4] = gg;
}

// one shell's FRC and regulariser from its five sums; live: the class has min_count members
__host__ __device__ inline void wn_frc_shell(const double *a, bool live, float ssnr_floor, double *frc, float *reg)
{
    const double f = live && a[1] > 0.0 && a[2] > 0.0 ? a[0] / sqrt(a[1] * a[2]) : 0.0;
    const double F = f < 0.999 ? f : 0.999;
    double rho = F > 0.0 ? 2.0 * F / (1.0 - F) : 0.0;
    if (rho < (double)ssnr_floor) rho = ssnr_floor;
    *frc = f;
    *reg = (float)(a[3] / a[4] / rho);
}

// grid (row blocks, k): part [k][blocks][5][S], S = P/2 + 1
__global__ __launch_bounds__(WN_THREADS) void wn_frc_rows_kernel(const float2 *__restrict__ num2, const float *__restrict__ den2, int P,
                                                                 int rows, double inv_snr, double *__restrict__ part)
{
    const int j = blockIdx.y, b = blockIdx.x, S = P / 2 + 1;
    const size_t ph = (size_t)P * S;
    const float2 *n0 = num2 + (size_t)2 * j * ph;
    const float *d0 = den2 + (size_t)2 * j * ph;
    const int y0 = b * rows, y1 = y0 + rows < P ? y0 + rows : P;
    double *o = part + ((size_t)j * gridDim.x + b) * 5 * S;
    for (int s = threadIdx.x; s < S; s += blockDim.x) {
        double a[5];
        wn_frc_shell_rows(n0, n0 + ph, d0, d0 + ph, P, y0, y1, s, inv_snr, a);
        for (int q = 0; q < 5; q++) o[(size_t)q * S + s] = a[q];
    }
}

// grid (shell blocks, k): the row blocks' sums in block order, then frc [k][S], reg [k][S]
__global__ __launch_bounds__(WN_THREADS) void wn_frc_combine_kernel(const double *__restrict__ part, int nb, int S,
                                                                    const int *__restrict__ counts2, int min_count, float ssnr_floor,
                                                                    double *__restrict__ frc, float *__restrict__ reg)
{
    const int j = blockIdx.y, s = blockIdx.x * WN_THREADS + threadIdx.x;
    if (s >= S) return;
    double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < nb; b++) {
        const double *p = part + ((size_t)j * nb + b) * 5 * S + s;
        for (int q = 0; q < 5; q++) a[q] += p[(size_t)q * S];
    }
    wn_frc_shell(a, counts2[2 * j] + counts2[2 * j + 1] >= min_count, ssnr_floor, frc + (size_t)j * S + s, reg + (size_t)j * S + s);
}

// ---- per-particle agreement scores

#define WN_SCORE_TILE 16            // the score kernel's tile edge: 4 waves of 8 x 8

// one element of one particle's score: y its spectrum, c its CTF, (N, D) its class's sums there, tau the Wiener term, g the
// Hermitian weight; model false: the class has nothing to predict the particle with (M = 0).  a += (g Re(y conj M), g |y|^2, g |M|^2)
__host__ __device__ inline void wn_score_element(float2 y, float c, int flipped, float2 N, float D, bool loo, bool model, double tau,
                                                 double g, double *a)
{
    const double w = flipped ? fabsf(c) : c;
    const double yx = y.x, yy = y.y;
    double mx = 0.0, my = 0.0;
    if (model) {
        double nx = N.x, ny = N.y, d = D;
        if (loo) {
            nx -= w * yx;
            ny -= w * yy;
            d -= (double)c * (double)c;
            if (d < 0.0) d = 0.0;
        }
        const double q = d + tau;
        if (q != 0.0) {
            const double f = w / q;
            mx = f * nx;
            my = f * ny;
        }
    }
    a[0] += g * (yx * mx + yy * my);
    a[1] += g * (yx * yx + yy * yy);
    a[2] += g * (mx * mx + my * my);
}

// element (row n, column kx) of particle spectrum spec [H][P] against its class's num / den [P][H]: skipped outside the band
// s_lo <= s <= s_hi (s_hi <= P/2); reg: the class's per-shell term [P/2 + 1], or null for the constant tau
__host__ __device__ inline void wn_score_at(const float2 *spec, int P, int H, int n, int kx, const WnCtf &cst, int flipped,
                                            const float2 *num, const float *den, bool loo, bool model, double tau, const float *reg,
                                            int s_lo, int s_hi, double *a)
{
    // s_lo <= s <= s_hi by wn_shell's integer bounds, without the shell itself: s >= a is r2 > a (a - 1), s <= b is r2 <= b (b + 1)
    const int ky = n <= P / 2 ? n : n - P, r2 = kx * kx + ky * ky;
    if ((s_lo > 0 && r2 <= s_lo * (s_lo - 1)) || r2 > s_hi * (s_hi + 1)) return;
    const float c = wn_ctf(cst, n < (P + 1) / 2 ? n : n - P, kx);
    const size_t o = (size_t)n * H + kx;
    wn_score_element(spec[(size_t)kx * P + n], c, flipped, num[o], den[o], loo, model, reg ? (double)reg[wn_shell(kx, ky)] : tau,
                     (kx == 0 || 2 * kx == P) ? 1.0 : 2.0, a);
}

// grid: the chunk's particles; perm: chunk-local indices in class order; sums [chunk][3]
__global__ __launch_bounds__(WN_THREADS) void wn_score_kernel(const float2 *__restrict__ spec, int P, int H, const int *__restrict__ perm,
                                                              const int *__restrict__ lab, const WnCtf *__restrict__ cst, int flipped,
                                                              const float2 *__restrict__ num, const float *__restrict__ den,
                                                              const int *__restrict__ counts, double tau, const float *__restrict__ reg,
                                                              int loo, int s_lo, int s_hi, double *__restrict__ sums)
{
    static_assert(WN_THREADS == 256 && WN_SCORE_TILE == 16, "four waves of 8 x 8 make one tile");
    __shared__ double part[WN_THREADS / 64][3];
    const int p = perm[blockIdx.x], cls = lab[p];
    const size_t ph = (size_t)P * H;
    const WnCtf c = cst[p];
    const float2 *y = spec + (size_t)p * ph, *N = num + (size_t)cls * ph;
    const float *D = den + (size_t)cls * ph, *R = reg ? reg + (size_t)cls * (P / 2 + 1) : nullptr;
    const bool model = !loo || counts[cls] >= 2;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tn = (wave & 1) * 8 + (lane & 7), tk = (wave >> 1) * 8 + (lane >> 3);
    double a[3] = {0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < H; k0 += WN_SCORE_TILE) {
        const int kx = k0 + tk;
        if (kx >= H) continue;
        for (int n = tn; n < P; n += WN_SCORE_TILE) wn_score_at(y, P, H, n, kx, c, flipped, N, D, loo != 0, model, tau, R, s_lo, s_hi, a);
    }
    for (int q = 0; q < 3; q++) {
        double v = a[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if (lane == 0) part[wave][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        double v = part[0][threadIdx.x];
        for (int w = 1; w < WN_THREADS / 64; w++) v += part[w][threadIdx.x];
        sums[(size_t)p * 3 + threadIdx.x] = v;
    }
}

}  // namespace ralign
