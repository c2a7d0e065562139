// Particle preprocessing (ra_prep_normalize, ra_prep_filter; contract: cryo_ralib_amd/prep.py).
//
// N -- background normalisation, one workgroup per image, the image staged in LDS when it fits next to the reduction slots
// (pp_image_in_lds), else re-read from global memory by every pass; the workgroups loop when n exceeds the grid.  Centre c = nx/2,
// u = col - c, v = row - c, B = {u^2 + v^2 > R^2}.  Four passes: the moments m = sum_B x [1, u, v] (ramp only; theta = G^-1 m with
// G^-1 from the host), sum_B e with e = x - (a + b u + c v), sum_B (e - mu)^2, then y = s (e - mu) / sigma written once as float32.
// Every sum is double in an order fixed by (nx, R) alone: thread t takes the pixels t, t + nt, ... in that order, the 64 lanes of
// a wave combine in a fixed tree (lane l with l ^ 32, 16, ... 1), the waves add in order through LDS.  No atomics.
//
// F -- Fourier filter: the phase flip's three passes (ralign_ctf.h) with the multiplier read from a [H][H] float table over
// (ix, |iy|), H = P/2 + 1, that a small kernel fills once per call from g = LP (1 - HP) evaluated in double; |iy| is the fast
// index because the column pass walks a column's rows with consecutive threads.
//
// The pass bodies are templates over an execution context and compile for the host (tests/test_prep_host_passes.py).
#pragma once

#include "ralign_ctf.h"

namespace ralign {

#define PP_THREADS 256
#define PP_WAVE 64
#define PP_MAX_SUMS 3
#define PP_RED_BYTES 128                        // PP_MAX_SUMS x (PP_THREADS / PP_WAVE) doubles, rounded up
// the largest box whose image sits in LDS next to the reduction slots within the flip's budget (201)
__host__ __device__ constexpr bool pp_image_in_lds(int nx) { return (size_t)PP_RED_BYTES + (size_t)nx * nx * 4 <= PF_LDS_BUDGET; }

#define PP_NONE 0
#define PP_TANL 1
#define PP_GAUSS 2

// what the host prepares of the background set B of (nx, R): |B| and the inverse of G = sum_B [1, u, v]^T [1, u, v]
struct PpGeom {
    int nx;
    double r2;              // R^2
    double nb;              // |B|
    double gi[6];           // G^-1, symmetric: (00, 01, 02, 11, 12, 22)
};

// G in exact integers, inverted in double by cofactors; false when B has no three pixels off one line (never inside the domain
// 4 <= nx <= 1024, 1 <= R <= nx/2)
inline bool pp_make_geom(int nx, double R, PpGeom &g)
{
    const int c = nx / 2;
    long long s1 = 0, su = 0, sv = 0, suu = 0, suv = 0, svv = 0;
    g.nx = nx;
    g.r2 = R * R;
    for (int row = 0; row < nx; row++)
        for (int col = 0; col < nx; col++) {
            const long long u = col - c, v = row - c;
            if ((double)(u * u + v * v) > g.r2) { s1++; su += u; sv += v; suu += u * u; suv += u * v; svv += v * v; }
        }
    g.nb = (double)s1;
    const double a = (double)s1, b = (double)su, cc = (double)sv, d = (double)suu, e = (double)suv, f = (double)svv;
    const double c00 = d * f - e * e, c01 = cc * e - b * f, c02 = b * e - cc * d;
    const double det = a * c00 + b * c01 + cc * c02;
    if (s1 < 4 || !(det > 0.0)) return false;
    g.gi[0] = c00 / det;
    g.gi[1] = c01 / det;
    g.gi[2] = c02 / det;
    g.gi[3] = (a * f - cc * cc) / det;
    g.gi[4] = (b * cc - a * e) / det;
    g.gi[5] = (a * d - b * b) / det;
    return true;
}

// f(i, row, col) at the pixels i = t, t + nt, ... < nx^2 of thread t, in that order
template <class F>
__host__ __device__ inline void pp_strided(int t, int nt, int nx, F f)
{
    const int npix = nx * nx, dq = nt / nx, dr = nt - dq * nx;
    int row = t / nx, col = t - row * nx;
    for (int i = t; i < npix; i += nt) {
        f(i, row, col);
        row += dq;
        col += dr;
        if (col >= nx) { col -= nx; row++; }
    }
}

// Execution context of the normalise passes on the device: a workgroup of nt threads (a multiple of 64), red [K][nt / 64] in LDS
struct PpCtx {
    int tid, nt;
    double *red;
    // out[k] = the sum over all pixels of what f adds to acc[k]; the same bits in every thread
    template <int K, class F>
    __device__ void sum(int nx, F f, double *out) const
    {
        double acc[K];
#pragma unroll
        for (int k = 0; k < K; k++) acc[k] = 0.0;
        pp_strided(tid, nt, nx, [&](int i, int row, int col) { f(i, row, col, acc); });
        const int nw = nt / PP_WAVE;
#pragma unroll
        for (int k = 0; k < K; k++) {
#pragma unroll
            for (int o = PP_WAVE / 2; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o);
            if ((tid & (PP_WAVE - 1)) == 0) red[k * nw + tid / PP_WAVE] = acc[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < K; k++) {
            double s = red[k * nw];
            for (int w = 1; w < nw; w++) s += red[k * nw + w];
            out[k] = s;
        }
        __syncthreads();
    }
    template <class F>
    __device__ void each(int nx, F f) const { pp_strided(tid, nt, nx, f); }
};

// The same on the host: nt virtual threads run one after the other, lanes past nt in the last wave add +0
struct PpHostCtx {
    int nt;
    template <int K, class F>
    void sum(int nx, F f, double *out) const
    {
        const int nw = (nt + PP_WAVE - 1) / PP_WAVE;
        for (int k = 0; k < K; k++) out[k] = 0.0;
        for (int w = 0; w < nw; w++) {
            double lane[PP_WAVE][K];
            for (int l = 0; l < PP_WAVE; l++) {
                for (int k = 0; k < K; k++) lane[l][k] = 0.0;
                const int t = w * PP_WAVE + l;
                if (t < nt) pp_strided(t, nt, nx, [&](int i, int row, int col) { f(i, row, col, lane[l]); });
            }
            for (int o = PP_WAVE / 2; o > 0; o >>= 1)
                for (int l = 0; l < o; l++)
                    for (int k = 0; k < K; k++) lane[l][k] += lane[l + o][k];
            for (int k = 0; k < K; k++) out[k] = w ? out[k] + lane[0][k] : lane[0][k];
        }
    }
    template <class F>
    void each(int nx, F f) const { for (int t = 0; t < nt; t++) pp_strided(t, nt, nx, f); }
};

// the four passes over one image: src [nx][nx] (LDS copy or the image itself), dst the image in global memory; sgn -1 to invert;
// stats [5] = (a, b, c, mu, sigma) or null, written by the one thread with `writer`
template <class Ctx>
__host__ __device__ inline void pp_normalize_image(const Ctx &cx, const float *src, float *dst, const PpGeom &g, int ramp, double sgn,
                                                   double *stats, bool writer)
{
    const int nx = g.nx, c = nx / 2;
    const double r2 = g.r2;
    auto in_b = [=](int row, int col) { const int u = col - c, v = row - c; return (double)(u * u + v * v) > r2; };
    double a = 0.0, b = 0.0, cc = 0.0;
    // 1. moments over B, theta = G^-1 m
    if (ramp) {
        double m[3];
        cx.template sum<3>(nx, [=](int i, int row, int col, double *acc) {
            if (in_b(row, col)) {
                const double x = src[i];
                acc[0] += x;
                acc[1] += x * (double)(col - c);
                acc[2] += x * (double)(row - c);
            }
        }, m);
        a = g.gi[0] * m[0] + g.gi[1] * m[1] + g.gi[2] * m[2];
        b = g.gi[1] * m[0] + g.gi[3] * m[1] + g.gi[4] * m[2];
        cc = g.gi[2] * m[0] + g.gi[4] * m[1] + g.gi[5] * m[2];
    }
    auto resid = [=](int i, int row, int col) { return (double)src[i] - (a + b * (double)(col - c) + cc * (double)(row - c)); };
    // 2. sum_B e; x - x over ALL pixels is 0 unless one of them is not finite
    double s[2];
    cx.template sum<2>(nx, [=](int i, int row, int col, double *acc) {
        const double x = src[i];
        acc[1] += x - x;
        if (in_b(row, col)) acc[0] += resid(i, row, col);
    }, s);
    double mu = s[0] / g.nb;
    // 3. sum_B (e - mu)^2
    double q[1];
    cx.template sum<1>(nx, [=](int i, int row, int col, double *acc) {
        if (in_b(row, col)) { const double d = resid(i, row, col) - mu; acc[0] += d * d; }
    }, q);
    double sigma = sqrt(q[0] / g.nb);
    if (s[1] != s[1]) a = b = cc = mu = sigma = s[1];           // a non-finite pixel anywhere: NaN throughout
    // 4. y, rounded once
    const bool unit = sigma == 0.0;
    cx.each(nx, [=](int i, int row, int col) {
        const double d = (double)src[i] - (a + b * (double)(col - c) + cc * (double)(row - c)) - mu;
        dst[i] = (float)(unit ? sgn * d : sgn * d / sigma);
    });
    if (stats && writer) { stats[0] = a; stats[1] = b; stats[2] = cc; stats[3] = mu; stats[4] = sigma; }
}

template <bool IMG_LDS>
__global__ __launch_bounds__(PP_THREADS) void prep_normalize_kernel(float *imgs, int n, PpGeom g, int ramp, float sgn, double *stats)
{
    extern __shared__ double pp_lds[];
    const int npix = g.nx * g.nx;
    float *limg = (float *)((char *)pp_lds + PP_RED_BYTES);
    const PpCtx cx{(int)threadIdx.x, PP_THREADS, pp_lds};
    for (int p = blockIdx.x; p < n; p += gridDim.x) {
        float *img = imgs + (size_t)p * npix;
        // every thread stages, reads and writes only its own pixels (tid, tid + nt, ... as pp_strided): no barrier around the copy
        if (IMG_LDS)
            for (int i = cx.tid; i < npix; i += cx.nt) limg[i] = img[i];
        pp_normalize_image(cx, IMG_LDS ? (const float *)limg : (const float *)img, img, g, ramp, (double)sgn,
                           stats ? stats + (size_t)p * 5 : nullptr, cx.tid == 0);
    }
}

// ---- F: the multiplier and the filter passes

// LP or HP at d cycles / pixel
__host__ __device__ inline double pp_filter_term(int kind, double pa, double pb, double d)
{
    if (kind == PP_TANL) {
        const double k = 3.14159265358979323846 / (2.0 * pb * pa);
        return 0.5 * (tanh(k * (d + pa)) - tanh(k * (d - pa)));
    }
    return exp(-d * d / (2.0 * pa * pa));
}

struct PpFilter {
    int lp_kind, hp_kind;
    double lp_a, lp_b, hp_a, hp_b;
};

// g at the integer frequencies (iy, ix) of a P x P transform, in double, rounded to float32 once
__host__ __device__ inline float pp_filter_gain(const PpFilter &f, int P, int iy, int ix)
{
    const double d = sqrt((double)(ix * ix + iy * iy)) / (double)P;
    const double lp = f.lp_kind ? pp_filter_term(f.lp_kind, f.lp_a, f.lp_b, d) : 1.0;
    const double hp = f.hp_kind ? pp_filter_term(f.hp_kind, f.hp_a, f.hp_b, d) : 0.0;
    return (float)(lp * (1.0 - hp));
}

// tab [H][H] over (ix, |iy|), H = P/2 + 1
__global__ void prep_filter_table_kernel(float *__restrict__ tab, int P, PpFilter f)
{
    const int H = P / 2 + 1, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < H * H) tab[i] = pp_filter_gain(f, P, i % H, i / H);
}

// pf_particle with the multiplier read from tab: img [nx][nx] in place, blk [nx][H], work 2 x nb x P, tw [P]
template <class Ctx>
__host__ __device__ inline void pp_filter_particle(const Ctx &cx, float *img, const float *tab, const PfPlan &pl, float2 *blk, float2 *work,
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
        float2 *z = pf_fft(cx, wa, wb, cnt, pl, tw, -1.f);
        // unrolled so that the table reads of several coefficients are in flight together
#pragma unroll 4
        for (int it = cx.tid; it < cnt * P; it += cx.nt) {
            const int t = it / P, n = it - t * P;
            const int ay = n < (P + 1) / 2 ? n : P - n;          // |iy| of the signed row frequency (numpy.fft.fftfreq order)
            const float m = tab[(size_t)(c0 + t) * H + ay];
            z[it] = make_float2(m * z[it].x, m * z[it].y);
        }
        cx.sync();
        float2 *zb = z == wa ? wb : wa;
        z = pf_fft(cx, z, zb, cnt, pl, tw, 1.f);
        for (int it = cx.tid; it < cnt * nx; it += cx.nt) {
            const int t = it / nx, y = it - t * nx;
            blk[(size_t)y * H + c0 + t] = z[(size_t)t * P + o + y];
        }
        cx.sync();
    }
    pf_rows_inverse(cx, img, pl, blk, work, tw);
}

// pf_kernel_body's layout: twiddles, work and (GBLK = false) the block in dynamic LDS, else the block in gscr and a looping grid
template <bool GBLK>
__device__ inline void pp_filter_kernel_body(float *imgs, int n, const float *tab, const PfPlan &pl, float2 *gscr)
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
    for (int p = blockIdx.x; p < n; p += gridDim.x) pp_filter_particle(cx, imgs + (size_t)p * pl.nx * pl.nx, tab, pl, blk, work, tw);
}

template <bool GBLK>
__global__ __launch_bounds__(PF_THREADS) void prep_filter_kernel(float *__restrict__ imgs, int n, const float *__restrict__ tab, PfPlan pl,
                                                                  float2 *__restrict__ gscr)
{
    pp_filter_kernel_body<GBLK>(imgs, n, tab, pl, gscr);
}

// the flip's fixed boxes (PF_FIXED_BOXES): the plan is a compile-time constant
template <int NX, int PAD>
__global__ __launch_bounds__(PF_THREADS) void prep_filter_fixed_kernel(float *__restrict__ imgs, int n, const float *__restrict__ tab,
                                                                        float2 *__restrict__ gscr)
{
    constexpr PfPlan pl = pf_make_plan(NX, PAD);
    static_assert(pl.nb > 0, "no plan");
    pp_filter_kernel_body<pl.gblk != 0>(imgs, n, tab, pl, gscr);
}

}  // namespace ralign
