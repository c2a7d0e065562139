// t-SNE of factors X [n][d] (scikit-learn 1.7 TSNE, method="barnes_hut", angle=0: sparse kNN affinities, exact repulsion).
//
//   tsne_sqnorm_kernel, tsne_knn_kernel, tsne_knn_query_kernel   the exact neighbour lists: ralign_knn.h.
//   tsne_affinity_kernel    sklearn's _binary_search_perplexity on the k neighbours of a row (one wave per row, double).
//   tsne_repulsion_kernel   all-pairs partials over one block of rows x one segment of columns: sum_j w_ij^2 (y_i - y_j) per row
//                           and sum_{j != i} w_ij over the block, w = 1 / (1 + d^2).  The self pair (w = 1) is left out of the
//                           float sum: a row whose other w are small would lose them against it.
//   tsne_update_kernel      Z from the block partials, the row's repulsion from its segment partials, the sparse attraction over
//                           its CSR row, the gradient, then sklearn's gains / momentum update (or the gradient alone).
//   tsne_stats_kernel       KL error and squared gradient norm from the update's per-workgroup partials.
//   tsne_place_kernel       out-of-sample placement of new points into a fixed embedding (at the end).
//
// Determinism: no atomics on floating-point data. Every sum has an order fixed by n alone: the segment length, the row blocks
// and the reduction trees depend on n only, never on the device or on how the grid is scheduled.
// Indices read from data (CSR columns, row pointers) are clamped before they address anything.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "ralign_knn.h"

namespace ralign {

#define TSNE_REP_THREADS 256
#define TSNE_REP_R 4                                   // rows per lane
#define TSNE_REP_ROWS (TSNE_REP_THREADS * TSNE_REP_R)  // rows per workgroup
#define TSNE_REP_CHUNK 512                             // columns staged in LDS at a time
#define TSNE_REP_MAXSEG 64                             // segments per row at most (bounds the partial buffer)
#define TSNE_UPD_THREADS 256

// the column segment length of the repulsion for n points: a multiple of TSNE_REP_ROWS, at most TSNE_REP_MAXSEG segments
__host__ __device__ inline int tsne_segment(int n)
{
    const int per = (n + TSNE_REP_MAXSEG * TSNE_REP_ROWS - 1) / (TSNE_REP_MAXSEG * TSNE_REP_ROWS);
    return TSNE_REP_ROWS * (per > 0 ? per : 1);
}

// fixed-order sum of v over the workgroup (blockDim.x = NT, a power of two); every thread gets the result
template <int NT>
__device__ __forceinline__ double tsne_block_sum(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// one wave per row: sklearn _binary_search_perplexity (_utils.pyx) with the row's k squared distances rounded to float, as
// sklearn hands them over; sums by a fixed butterfly, so every lane holds the same bits
__device__ __forceinline__ double tsne_wave_sum(double v)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void tsne_affinity_kernel(const double *__restrict__ dist2, int n, int k, double desired_entropy,
                                                            double *__restrict__ pcond)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    constexpr int M = (TSNE_MAX_K + 63) / 64;
    double dd[M], pp[M];
#pragma unroll
    for (int m = 0; m < M; m++) {
        const int j = lane + 64 * m;
        dd[m] = j < k ? (double)(float)dist2[(size_t)i * k + j] : 0.0;
        pp[m] = 0.0;
    }
    double beta = 1.0, beta_min = -__builtin_inf(), beta_max = __builtin_inf();
    const double tol = (double)1e-5f, floor_sum = (double)1e-8f;
    for (int step = 0; step < 100; step++) {
        double s = 0.0;
#pragma unroll
        for (int m = 0; m < M; m++) {
            pp[m] = lane + 64 * m < k ? exp(-dd[m] * beta) : 0.0;
            s += pp[m];
        }
        double sum_p = tsne_wave_sum(s);
        if (sum_p == 0.0) sum_p = floor_sum;
        double sd = 0.0;
#pragma unroll
        for (int m = 0; m < M; m++) {
            pp[m] /= sum_p;
            sd += dd[m] * pp[m];
        }
        const double sum_dp = tsne_wave_sum(sd);
        const double diff = log(sum_p) + beta * sum_dp - desired_entropy;
        if (fabs(diff) <= tol) break;       // NaN distances make diff NaN: the search runs its 100 steps and ends
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == __builtin_inf() ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -__builtin_inf() ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
#pragma unroll
    for (int m = 0; m < M; m++) {
        const int j = lane + 64 * m;
        if (j < k) pcond[(size_t)i * k + j] = pp[m];
    }
}

// grid (row blocks, segments). Partials part[s][i] = sum over segment s of w^2 (y_i - y_j); zpart[s * nrb + rb] = sum of w over
// the block's rows and the segment's columns, self pairs left out.
__global__ __launch_bounds__(TSNE_REP_THREADS) void tsne_repulsion_kernel(const float2 *__restrict__ y, int n, int seg,
                                                                          float2 *__restrict__ part, double *__restrict__ zpart)
{
    __shared__ float2 ys[TSNE_REP_CHUNK];
    __shared__ double red[TSNE_REP_THREADS];
    const int rb = blockIdx.x, s = blockIdx.y, nrb = gridDim.x, tid = threadIdx.x;
    float yx[TSNE_REP_R], yy[TSNE_REP_R], fx[TSNE_REP_R], fy[TSNE_REP_R], z[TSNE_REP_R];
#pragma unroll
    for (int r = 0; r < TSNE_REP_R; r++) {
        const int i = rb * TSNE_REP_ROWS + r * TSNE_REP_THREADS + tid;
        const float2 v = i < n ? y[i] : float2{0.f, 0.f};
        yx[r] = v.x; yy[r] = v.y; fx[r] = 0.f; fy[r] = 0.f; z[r] = 0.f;
    }
    const int j0 = s * seg, j1 = min(n, j0 + seg), i0 = rb * TSNE_REP_ROWS;
    for (int jt = j0; jt < j1; jt += TSNE_REP_CHUNK) {
        const int c = min(TSNE_REP_CHUNK, j1 - jt);
        __syncthreads();
        for (int t = tid; t < c; t += TSNE_REP_THREADS) ys[t] = y[jt + t];
        __syncthreads();
        // own: the chunk holds rows of this block, whose self pairs stay out of z (their force term is zero as it is)
        auto pairs = [&](auto own) {
#pragma unroll 4
            for (int j = 0; j < c; j++) {
                const float2 v = ys[j];
#pragma unroll
                for (int r = 0; r < TSNE_REP_R; r++) {
                    const float dx = yx[r] - v.x, dy = yy[r] - v.y;
                    const float w = __builtin_amdgcn_rcpf(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, 1.f)));
                    const float w2 = w * w;
                    if (decltype(own)::value) z[r] += jt + j == i0 + r * TSNE_REP_THREADS + tid ? 0.f : w;
                    else z[r] += w;
                    fx[r] = __builtin_fmaf(w2, dx, fx[r]);
                    fy[r] = __builtin_fmaf(w2, dy, fy[r]);
                }
            }
        };
        if (jt < i0 + TSNE_REP_ROWS && jt + c > i0) pairs(std::true_type{});
        else pairs(std::false_type{});
    }
    double zs = 0.0;
#pragma unroll
    for (int r = 0; r < TSNE_REP_R; r++) {
        const int i = rb * TSNE_REP_ROWS + r * TSNE_REP_THREADS + tid;
        if (i < n) {
            part[(size_t)s * n + i] = float2{fx[r], fy[r]};
            zs += (double)z[r];
        }
    }
    zs = tsne_block_sum<TSNE_REP_THREADS>(zs, red);
    if (tid == 0) zpart[s * nrb + rb] = zs;
}

struct TsneUpdateArgs {
    const float2 *y;                // current embedding [n]
    float2 *y_out, *update, *gains; // mode 0: next embedding, sklearn's update and gains (in place)
    float2 *grad;                   // mode 1: the gradient (may be null)
    const float2 *part;             // [nseg][n]
    const double *zpart;            // [nz]
    const int *indptr, *indices;    // CSR of P, nnz entries
    const float *p;
    int n, nseg, nz, nnz, mode;
    float exaggeration, momentum, learning_rate;
    double *stats_part;             // [gridDim.x][2]: KL error, squared gradient norm (null: not computed)
};

__global__ __launch_bounds__(TSNE_UPD_THREADS) void tsne_update_kernel(TsneUpdateArgs a)
{
    __shared__ double red[TSNE_UPD_THREADS];
    const int tid = threadIdx.x, i = blockIdx.x * TSNE_UPD_THREADS + tid;
    double zs = 0.0;
    for (int t = tid; t < a.nz; t += TSNE_UPD_THREADS) zs += a.zpart[t];
    // every workgroup forms the same Z (the partials hold no self pairs); sklearn floors sum_Q at eps
    const double Z = fmax(tsne_block_sum<TSNE_UPD_THREADS>(zs, red), 2.220446049250313e-16);
    double err = 0.0, gn = 0.0;
    if (i < a.n) {
        double rx = 0.0, ry = 0.0;
        for (int s = 0; s < a.nseg; s++) {
            const float2 v = a.part[(size_t)s * a.n + i];
            rx += (double)v.x;
            ry += (double)v.y;
        }
        const float2 yi = a.y[i];
        const int e0 = min(max(a.indptr[i], 0), a.nnz), e1 = min(max(a.indptr[i + 1], e0), a.nnz);
        float ax = 0.f, ay = 0.f;
        const bool want = a.stats_part != nullptr;
        const float tiny = 1.17549435e-38f;
        for (int e = e0; e < e1; e++) {
            const int j = a.indices[e];
            if ((unsigned)j >= (unsigned)a.n) continue;
            const float2 yj = a.y[j];
            const float dx = yi.x - yj.x, dy = yi.y - yj.y;
            const float w = 1.f / (1.f + (dx * dx + dy * dy));
            const float pij = a.p[e] * a.exaggeration;
            const float f = pij * w;
            ax += f * dx;
            ay += f * dy;
            if (want) {
                const double q = (double)w / Z;
                err += (double)pij * log(fmax((double)pij, (double)tiny) / fmax(q, (double)tiny));
            }
        }
        float gx = (float)((double)ax - rx / Z) * 4.f, gy = (float)((double)ay - ry / Z) * 4.f;
        if (a.mode == 0) {
            float2 u = a.update[i], g = a.gains[i];
            g.x = u.x * gx < 0.f ? g.x + 0.2f : g.x * 0.8f;
            g.y = u.y * gy < 0.f ? g.y + 0.2f : g.y * 0.8f;
            g.x = fmaxf(g.x, 0.01f);
            g.y = fmaxf(g.y, 0.01f);
            gx *= g.x;
            gy *= g.y;
            u.x = a.momentum * u.x - a.learning_rate * gx;
            u.y = a.momentum * u.y - a.learning_rate * gy;
            a.gains[i] = g;
            a.update[i] = u;
            a.y_out[i] = float2{yi.x + u.x, yi.y + u.y};
        } else if (a.grad) {
            a.grad[i] = float2{gx, gy};
        }
        gn = (double)gx * gx + (double)gy * gy;
    }
    if (a.stats_part) {
        err = tsne_block_sum<TSNE_UPD_THREADS>(err, red);
        gn = tsne_block_sum<TSNE_UPD_THREADS>(gn, red);
        if (tid == 0) { a.stats_part[2 * blockIdx.x] = err; a.stats_part[2 * blockIdx.x + 1] = gn; }
    }
}

__global__ __launch_bounds__(256) void tsne_stats_kernel(const double *__restrict__ part, int nb, double *__restrict__ stats)
{
    __shared__ double red[256];
    double e = 0.0, g = 0.0;
    for (int b = threadIdx.x; b < nb; b += 256) { e += part[2 * b]; g += part[2 * b + 1]; }
    e = tsne_block_sum<256>(e, red);
    g = tsne_block_sum<256>(g, red);
    if (threadIdx.x == 0) { stats[0] = e; stats[1] = g; }
}

// ---- out-of-sample placement: new points against a fixed embedding
//
//   tsne_knn_query_kernel   the neighbour lists of the new rows among the fitted rows: ralign_knn.h.
//   tsne_place_kernel       a wave owns TSNE_PLACE_R new points and keeps their y, update and gains in registers over all
//                           iterations; its 64 lanes share the fitted points (lane l takes columns l, l + 64, ... of each staged
//                           chunk) and the neighbour list (entries l, l + 64, ...).  Per chunk a lane sums at most
//                           TSNE_PLACE_CHUNK / 64 columns in float32, then adds the partial to a double; the lanes' doubles are
//                           added by one xor butterfly, so all 64 hold the same bits and each applies the same update.
//
// Order: a point's sums depend on m and k only (the chunk, the lane stride and the butterfly are constants); the four points of a
// wave run the same instructions on separate registers, so neither n, the point's slot nor the grid enters any value.

#define TSNE_PLACE_THREADS 256
#define TSNE_PLACE_R 4                                                 // points per wave
#define TSNE_PLACE_ROWS (TSNE_PLACE_R * TSNE_PLACE_THREADS / 64)       // points per workgroup
#define TSNE_PLACE_CHUNK 2048                                          // fitted points staged in LDS at a time

struct TsnePlaceArgs {
    float2 *y;                      // [n]: read; written after the iterations if n_iter > 0
    const float2 *yfit;             // [m]
    const int *idx;                 // [n][k] neighbour lists; entries outside 0 .. m - 1 are skipped
    const float *p;                 // [n][k]
    int n, m, k, n_iter;
    float exaggeration, momentum, learning_rate;
    float2 *grad;                   // [n] gradient at the final y with the exaggeration (may be null)
    double *kl, *z;                 // [n] KL_i and Z_i at the final y (may be null)
};

// Z_i, the repulsion sum_j w^2 (y_i - Y_j) over all m fitted points, the attraction sum_nbr p w (y_i - Y_j) and (want_kl) KL_i of
// the wave's TSNE_PLACE_R points; on return every lane holds the same values.  Workgroup-uniform: it stages yfit through ys
template <bool KL>
__device__ __forceinline__ void tsne_place_eval(const TsnePlaceArgs &a, float2 *ys, int row0, const float (&yx)[TSNE_PLACE_R],
                                                const float (&yy)[TSNE_PLACE_R], double (&Z)[TSNE_PLACE_R],
                                                double (&rx)[TSNE_PLACE_R], double (&ry)[TSNE_PLACE_R],
                                                double (&ax)[TSNE_PLACE_R], double (&ay)[TSNE_PLACE_R], double (&kl)[TSNE_PLACE_R])
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int r = 0; r < TSNE_PLACE_R; r++) { Z[r] = 0.0; rx[r] = 0.0; ry[r] = 0.0; ax[r] = 0.0; ay[r] = 0.0; kl[r] = 0.0; }
    for (int jt = 0; jt < a.m; jt += TSNE_PLACE_CHUNK) {
        const int c = min(TSNE_PLACE_CHUNK, a.m - jt);
        __syncthreads();
        for (int t = tid; t < c; t += TSNE_PLACE_THREADS) ys[t] = a.yfit[jt + t];
        __syncthreads();
        float fx[TSNE_PLACE_R], fy[TSNE_PLACE_R], z[TSNE_PLACE_R];
#pragma unroll
        for (int r = 0; r < TSNE_PLACE_R; r++) { fx[r] = 0.f; fy[r] = 0.f; z[r] = 0.f; }
#pragma unroll 4
        for (int j = lane; j < c; j += 64) {
            const float2 v = ys[j];
#pragma unroll
            for (int r = 0; r < TSNE_PLACE_R; r++) {
                const float dx = yx[r] - v.x, dy = yy[r] - v.y;
                const float w = __builtin_amdgcn_rcpf(__builtin_fmaf(dx, dx, __builtin_fmaf(dy, dy, 1.f)));
                const float w2 = w * w;
                z[r] += w;
                fx[r] = __builtin_fmaf(w2, dx, fx[r]);
                fy[r] = __builtin_fmaf(w2, dy, fy[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < TSNE_PLACE_R; r++) { Z[r] += (double)z[r]; rx[r] += (double)fx[r]; ry[r] += (double)fy[r]; }
    }
#pragma unroll
    for (int r = 0; r < TSNE_PLACE_R; r++) { Z[r] = tsne_wave_sum(Z[r]); rx[r] = tsne_wave_sum(rx[r]); ry[r] = tsne_wave_sum(ry[r]); }
    const float tiny = 1.17549435e-38f;
#pragma unroll
    for (int r = 0; r < TSNE_PLACE_R; r++) {
        const int i = row0 + r;
        if (i < a.n) {
            for (int e = lane; e < a.k; e += 64) {
                const int j = a.idx[(size_t)i * a.k + e];
                if ((unsigned)j >= (unsigned)a.m) continue;
                const float2 v = a.yfit[j];
                const float pij = a.p[(size_t)i * a.k + e];
                const float dx = yx[r] - v.x, dy = yy[r] - v.y;
                const float w = 1.f / (1.f + (dx * dx + dy * dy));
                const float f = pij * w;
                ax[r] += (double)(f * dx);
                ay[r] += (double)(f * dy);
                if (KL) kl[r] += (double)pij * log(fmax((double)pij, (double)tiny) / fmax((double)w / Z[r], (double)tiny));
            }
        }
        ax[r] = tsne_wave_sum(ax[r]);
        ay[r] = tsne_wave_sum(ay[r]);
        if (KL) kl[r] = tsne_wave_sum(kl[r]);
    }
}

__global__ __launch_bounds__(TSNE_PLACE_THREADS) void tsne_place_kernel(TsnePlaceArgs a)
{
#pragma clang fp contract(off)
    __shared__ float2 ys[TSNE_PLACE_CHUNK];
    const int lane = threadIdx.x & 63;
    const int row0 = blockIdx.x * TSNE_PLACE_ROWS + (threadIdx.x >> 6) * TSNE_PLACE_R;
    float yx[TSNE_PLACE_R], yy[TSNE_PLACE_R], ux[TSNE_PLACE_R], uy[TSNE_PLACE_R], gx[TSNE_PLACE_R], gy[TSNE_PLACE_R];
    double Z[TSNE_PLACE_R], rx[TSNE_PLACE_R], ry[TSNE_PLACE_R], ax[TSNE_PLACE_R], ay[TSNE_PLACE_R], kl[TSNE_PLACE_R];
#pragma unroll
    for (int r = 0; r < TSNE_PLACE_R; r++) {
        const float2 v = row0 + r < a.n ? a.y[row0 + r] : float2{0.f, 0.f};
        yx[r] = v.x; yy[r] = v.y; ux[r] = 0.f; uy[r] = 0.f; gx[r] = 1.f; gy[r] = 1.f;
    }
    const double e = (double)a.exaggeration;
    for (int it = 0; it < a.n_iter; it++) {
        tsne_place_eval<false>(a, ys, row0, yx, yy, Z, rx, ry, ax, ay, kl);
#pragma unroll
        for (int r = 0; r < TSNE_PLACE_R; r++) {
            float dx = (float)(4.0 * (e * ax[r] - rx[r] / Z[r])), dy = (float)(4.0 * (e * ay[r] - ry[r] / Z[r]));
            gx[r] = fmaxf(ux[r] * dx < 0.f ? gx[r] + 0.2f : gx[r] * 0.8f, 0.01f);
            gy[r] = fmaxf(uy[r] * dy < 0.f ? gy[r] + 0.2f : gy[r] * 0.8f, 0.01f);
            dx *= gx[r];
            dy *= gy[r];
            ux[r] = a.momentum * ux[r] - a.learning_rate * dx;
            uy[r] = a.momentum * uy[r] - a.learning_rate * dy;
            yx[r] += ux[r];
            yy[r] += uy[r];
        }
    }
    if (a.grad || a.kl || a.z) {
        if (a.kl) tsne_place_eval<true>(a, ys, row0, yx, yy, Z, rx, ry, ax, ay, kl);
        else tsne_place_eval<false>(a, ys, row0, yx, yy, Z, rx, ry, ax, ay, kl);
    }
#pragma unroll
    for (int r = 0; r < TSNE_PLACE_R; r++) {
        const int i = row0 + r;
        if (i >= a.n || lane != r) continue;
        if (a.n_iter > 0) a.y[i] = float2{yx[r], yy[r]};
        if (a.grad) a.grad[i] = float2{(float)(4.0 * (e * ax[r] - rx[r] / Z[r])), (float)(4.0 * (e * ay[r] - ry[r] / Z[r]))};
        if (a.kl) a.kl[i] = kl[r];
        if (a.z) a.z[i] = Z[r];
    }
}

}  // namespace ralign
