// UMAP of 2SDR factors (the contract at the top of cryo_ralib_amd/umap.py): the smooth-kNN calibration, one
// epoch of the layout as a per-vertex gather, and the out-of-sample placement.  Positions are float32, every sum is double.
//
//   umap_smooth_kernel    rule 2 on the k squared distances of a row.  One wave per row, UMAP_SK_ROWS rows a workgroup; lane l holds
//                         the entries l, l + 64, ... (at most UMAP_SK_M = 5) in registers as d = sqrt(D2) and then x = d - rho.
//                         psum adds a lane's kernel values in that order and then the 64 lanes in the xor butterfly 1, 2, .. 32, so
//                         every lane holds the same bits and takes the same branch of the bisection.  rho is a wave minimum (a
//                         selection); the mean of d behind the floor is added in list order by every lane alike.
//   umap_check_kernel     flags a CSR that umap_epoch_kernel would have to patch: an indptr that does not ascend from 0 to nnz, or a
//                         column outside 0 .. n - 1.  Nothing beyond indices[nnz - 1] is read.
//   umap_epoch_kernel     rule 6 for every vertex: UMAP_LANES lanes share a CSR row, UMAP_ROWS rows a workgroup.  Lane l walks the
//                         entries p0 + l, p0 + l + 16, ... in that order and adds, for each firing entry, the attractive move and
//                         then the moves of the negatives s = 0, 1, ... to its own pair of sums; the 16 lanes then combine in the
//                         xor tree 8, 4, 2, 1.  y_out[i] = float(y[i] + alpha sum), one writer per vertex, y never written.
//   umap_place_kernel     rule 8: the same lane layout over the k list slots of a new row, all epochs in the launch; the position
//                         lives in registers (the same float32 bits in the 16 lanes of a row) and is rounded once per epoch.
//
// Determinism: no atomics on positions, every sum in an order fixed by the row's length alone, the samples from a counter-based
// generator keyed by (seed, epoch, entry, sample).  No workgroup waits for another.  Every index read from memory is range-checked
// before it addresses anything.  Contraction to fma is off in the move arithmetic, so the float64 checker (numpy, unfused) differs
// from the device by the roundings of pow alone.
#pragma once

#include <hip/hip_runtime.h>

namespace ralign {

#define UMAP_MAX_N 262144
#define UMAP_MAX_ROWS 4194304       // rows of one calibration or placement call
#define UMAP_MAX_K 301              // list entries of a row
#define UMAP_MAX_ROW0 (1LL << 48)   // global row indices of a placement: 16 ((row0 + i) k + slot) + s stays below 2^62
#define UMAP_MAX_NEG 16             // negatives per firing entry
#define UMAP_MAX_EPOCHS 10000
#define UMAP_TRIPS 64               // trips of the bisection
#define UMAP_SK_ROWS 4              // rows (waves) per workgroup of the calibration
#define UMAP_SK_M ((UMAP_MAX_K + 63) / 64)
#define UMAP_LANES 16               // lanes per CSR row / list
#define UMAP_ROWS 16                // rows per workgroup of the epoch and the placement
#define UMAP_KEY_SEED 0xD1342543DE82EF95ull
#define UMAP_KEY_EPOCH 0xA0761D6478BD642Full

static_assert(UMAP_LANES * UMAP_ROWS == 256 && UMAP_SK_ROWS * 64 == 256 && UMAP_MAX_NEG <= 16, "tile plan");

__device__ __forceinline__ double umap_wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__device__ __forceinline__ double umap_wave_min(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v = fmin(v, __shfl_xor(v, m, 64));
    return v;
}

__global__ __launch_bounds__(256) void umap_smooth_kernel(const double *__restrict__ dist2, int rows, int k, double target,
                                                          double *__restrict__ rho, double *__restrict__ sigma, double *__restrict__ w)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * UMAP_SK_ROWS + (threadIdx.x >> 6);
    if (i >= rows) return;                                  // the whole wave
    const double inf = __builtin_inf();
    double x[UMAP_SK_M];
    double mn = inf;
#pragma unroll
    for (int m = 0; m < UMAP_SK_M; m++) {
        const int j = lane + 64 * m;
        x[m] = j < k ? sqrt(dist2[(size_t)i * k + j]) : 0.0;
        if (j < k && x[m] > 0.0) mn = fmin(mn, x[m]);
    }
    // the floor's mean in list order, every lane the same loop: a floored sigma divides distances hundreds of times its size, so
    // a sum in another order would show in w
    double s = 0.0;
    for (int j = 0; j < k; j++) s += sqrt(dist2[(size_t)i * k + j]);
    const double mean = s / (double)k;
    mn = umap_wave_min(mn);
    const double r = mn == inf ? 0.0 : mn;
#pragma unroll
    for (int m = 0; m < UMAP_SK_M; m++) x[m] -= r;
    double lo = 0.0, hi = inf, mid = 1.0;
    for (int trip = 0; trip < UMAP_TRIPS; trip++) {
        double ps = 0.0;
#pragma unroll
        for (int m = 0; m < UMAP_SK_M; m++)
            if (lane + 64 * m < k) ps += x[m] > 0.0 ? exp(-x[m] / mid) : 1.0;
        const double psum = umap_wave_sum(ps);
        if (fabs(psum - target) < 1e-5) break;              // a NaN runs its 64 trips and ends
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = hi == inf ? mid * 2.0 : (lo + hi) / 2.0;
        }
    }
    const double sg = fmax(mid, 1e-3 * mean);
#pragma unroll
    for (int m = 0; m < UMAP_SK_M; m++) {
        const int j = lane + 64 * m;
        if (j < k) w[(size_t)i * k + j] = (x[m] <= 0.0 || sg == 0.0) ? 1.0 : exp(-x[m] / sg);
    }
    if (lane == 0) {
        rho[i] = r;
        sigma[i] = sg;
    }
}

// bad[0] = 1 unless indptr ascends from 0 to nnz and every column is in 0 .. n - 1 (spec_check_kernel asks for another condition,
// rows of at most n entries: the two stay apart)
__global__ __launch_bounds__(256) void umap_check_kernel(const int *__restrict__ indptr, const int *__restrict__ indices, int n, int nnz,
                                                         int *__restrict__ bad)
{
    const int lane = threadIdx.x & (UMAP_LANES - 1), i = blockIdx.x * UMAP_ROWS + (threadIdx.x >> 4);
    if (i >= n) return;
    const int p0 = indptr[i], p1 = indptr[i + 1];
    bool wrong = p0 < 0 || p1 < p0 || p1 > nnz || (i == 0 && p0 != 0) || (i == n - 1 && p1 != nnz);
    if (!wrong)
        for (int p = p0 + lane; p < p1; p += UMAP_LANES) {
            const int c = indices[p];
            wrong |= c < 0 || c >= n;
        }
    if (wrong) atomicMax(bad, 1);
}

// splitmix64's finaliser (Steele, Lea and Flood 2014; Vigna's constants)
__device__ __forceinline__ unsigned long long umap_mix(unsigned long long z)
{
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// sample s of entry p in the epoch of `key` = seed KEY_SEED + t KEY_EPOCH: an index in 0 .. count - 1
__device__ __forceinline__ int umap_draw(unsigned long long key, unsigned long long p, int s, int count)
{
    const unsigned long long z = umap_mix(key + 16ull * p + (unsigned long long)s);
    return (int)(((z >> 32) * (unsigned long long)count) >> 32);
}

__device__ __forceinline__ double umap_clip(double v) { return v > 4.0 ? 4.0 : (v < -4.0 ? -4.0 : v); }

__device__ __forceinline__ bool umap_fires(double r, int t) { return floor((double)t * r) > floor((double)(t - 1) * r); }

// the parameters of the moves: a, b, m2ab = (-2 a) b, g2b = (2 gamma) b
struct UmapCurve {
    double a, b, m2ab, g2b;
};

// the attractive move of y towards v, times `factor`, added to (sx, sy)
__device__ __forceinline__ void umap_attract(const float2 y, const float2 v, const UmapCurve &c, double factor, double &sx, double &sy)
{
#pragma clang fp contract(off)
    const double dx = (double)y.x - (double)v.x, dy = (double)y.y - (double)v.y;
    const double q = dx * dx + dy * dy;
    if (q > 0.0) {
        const double qb = pow(q, c.b);
        const double coef = (c.m2ab * qb / q) / (1.0 + c.a * qb);
        sx += factor * umap_clip(coef * dx);
        sy += factor * umap_clip(coef * dy);
    }
}

// the repulsive move of y away from v added to (sx, sy); coincident points move by +4
__device__ __forceinline__ void umap_repel(const float2 y, const float2 v, const UmapCurve &c, double &sx, double &sy)
{
#pragma clang fp contract(off)
    const double dx = (double)y.x - (double)v.x, dy = (double)y.y - (double)v.y;
    const double q = dx * dx + dy * dy;
    if (q > 0.0) {
        const double qb = pow(q, c.b);
        const double coef = c.g2b / ((0.001 + q) * (1.0 + c.a * qb));
        sx += umap_clip(coef * dx);
        sy += umap_clip(coef * dy);
    } else if (q == 0.0) {
        sx += 4.0;
        sy += 4.0;
    }
}

// the sum of v over the 16 lanes of a row, the same bits in each
__device__ __forceinline__ double umap_group_sum(double v)
{
#pragma unroll
    for (int m = UMAP_LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

struct UmapEpochArgs {
    const float2 *y;
    float2 *y_out;
    const int *indptr, *indices;
    const double *rate;
    int n, neg, t;
    double alpha;
    unsigned long long key;         // seed KEY_SEED + t KEY_EPOCH (mod 2^64)
    UmapCurve c;
};

__global__ __launch_bounds__(256) void umap_epoch_kernel(const UmapEpochArgs a)
{
    const int lane = threadIdx.x & (UMAP_LANES - 1), i = blockIdx.x * UMAP_ROWS + (threadIdx.x >> 4);
    double sx = 0.0, sy = 0.0;
    float2 yi = float2{0.f, 0.f};
    if (i < a.n) {
        yi = a.y[i];
        const int p0 = a.indptr[i], p1 = a.indptr[i + 1];
        if (p0 >= 0)
            for (int p = p0 + lane; p < p1; p += UMAP_LANES) {
                if (!umap_fires(a.rate[p], a.t)) continue;
                const int j = a.indices[p];
                if (j < 0 || j >= a.n) continue;
                umap_attract(yi, a.y[j], a.c, 2.0, sx, sy);
                for (int s = 0; s < a.neg; s++) {
                    const int kk = umap_draw(a.key, (unsigned long long)p, s, a.n);
                    if (kk != i) umap_repel(yi, a.y[kk], a.c, sx, sy);
                }
            }
    }
    sx = umap_group_sum(sx);
    sy = umap_group_sum(sy);
    if (i < a.n && lane == 0) {
#pragma clang fp contract(off)
        a.y_out[i] = float2{(float)((double)yi.x + a.alpha * sx), (float)((double)yi.y + a.alpha * sy)};
    }
}

struct UmapPlaceArgs {
    float2 *y;                      // [n] in and out
    const float2 *yfit;             // [m]
    const int *idx;                 // [n][k]
    const double *rate;             // [n][k]
    int n, m, k, neg, n_epochs;
    unsigned long long row0, seed_key;      // seed KEY_SEED (mod 2^64)
    double lr;
    UmapCurve c;
};

__global__ __launch_bounds__(256) void umap_place_kernel(const UmapPlaceArgs a)
{
    const int lane = threadIdx.x & (UMAP_LANES - 1), i = blockIdx.x * UMAP_ROWS + (threadIdx.x >> 4);
    const bool live = i < a.n;
    const int kk = live ? a.k : 0;
    const size_t base = live ? (size_t)i * a.k : 0;
    float2 yi = live ? a.y[i] : float2{0.f, 0.f};
    for (int t = 1; t <= a.n_epochs; t++) {
        const unsigned long long key = a.seed_key + (unsigned long long)t * UMAP_KEY_EPOCH;
        double sx = 0.0, sy = 0.0;
        for (int slot = lane; slot < kk; slot += UMAP_LANES) {
            if (!umap_fires(a.rate[base + slot], t)) continue;
            const int j = a.idx[base + slot];
            if (j < 0 || j >= a.m) continue;
            umap_attract(yi, a.yfit[j], a.c, 1.0, sx, sy);
            const unsigned long long p = (a.row0 + (unsigned long long)i) * (unsigned long long)a.k + (unsigned long long)slot;
            for (int s = 0; s < a.neg; s++) umap_repel(yi, a.yfit[umap_draw(key, p, s, a.m)], a.c, sx, sy);
        }
        sx = umap_group_sum(sx);
        sy = umap_group_sum(sy);
        {
#pragma clang fp contract(off)
            const double alpha = a.lr * (1.0 - (double)(t - 1) / (double)a.n_epochs);
            yi = float2{(float)((double)yi.x + alpha * sx), (float)((double)yi.y + alpha * sy)};
        }
    }
    if (live && lane == 0) a.y[i] = yi;
}

}  // namespace ralign
