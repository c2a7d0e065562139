// Cluster validity of a labelled X [n][d] (scikit-learn 1.7 sklearn.metrics silhouette_samples, calinski_harabasz_score and
// davies_bouldin_score with metric="euclidean").  The member lists are ralign_kmeans.h's.
//
//   val_pstart_kernel        pstart [k + 1]: the first padded column of each cluster, every cluster's range rounded up to a multiple
//                            of the column tile.
//   val_cols_kernel          cols [pstart[k]]: the member lists (cluster by cluster, index order) copied into their padded ranges;
//                            the padding stays -1, an invalid index that contributes exactly 0.
//   val_silhouette_kernel    one workgroup per VAL_TR rows walks ALL columns, cluster by cluster: |x_i - x_j| from differences in
//                            f32 (4 x 4 pair accumulators per thread over feature chunks staged in LDS), sqrt, and the sum over j
//                            in double.  At a cluster's end the 16 partial sums of a row are combined by a fixed xor butterfly and
//                            folded into the row's own-cluster sum or into the running minimum of the other clusters' means (the
//                            first cluster wins ties).  Per row: s, a, b and the nearest other cluster.  No [n][k] table.
//   val_centroid_kernel      centroid = member sum / count (0 for an empty id), counts as int.
//   val_disp_kernel          one block per cluster: sum of |x - mu_c|^2 and of |x - mu_c| over its member list, each thread a
//                            contiguous share in list order, then the block tree.
//
// Determinism: no floating-point atomics.  A pair's squared distance is summed over the features in order; a thread's share of
// D(i, c) runs over the cluster's tiles in order and its 4 columns in order; the butterfly's order is fixed.  The order depends
// on (n, d, k) and the labels alone: the grid is one workgroup per row tile, never a split of the columns.
#pragma once

#include <hip/hip_runtime.h>

#include "ralign_kmeans.h"

namespace ralign {

#define VAL_MAX_N 262144            // rows of one silhouette call (n^2 pair distances)
#define VAL_TR 64                   // rows per workgroup
#define VAL_TC 64                   // columns per tile: every cluster's column range is padded to a multiple
#define VAL_FC 32                   // features per chunk in LDS
#define VAL_LS 68                   // LDS stride of one feature's 64 values: 16-byte aligned rows; the staging stores of one lane
                                    // group (8 features x 4 rows) hit 32 distinct banks

// one thread: pstart[c] = sum over c' < c of count[c'] rounded up to VAL_TC
__global__ __launch_bounds__(64) void val_pstart_kernel(const int *__restrict__ count, int k, int *__restrict__ pstart)
{
    if (threadIdx.x != 0) return;
    int p = 0;
    for (int c = 0; c < k; c++) {
        pstart[c] = p;
        p += (count[c] + VAL_TC - 1) / VAL_TC * VAL_TC;
    }
    pstart[k] = p;
}

// cols[pstart[c] + r] = members[start[c] + r] for the r-th member of cluster c; cap = the length of cols
__global__ __launch_bounds__(256) void val_cols_kernel(const int *__restrict__ members, const int *__restrict__ start,
                                                       const int *__restrict__ count, const int *__restrict__ pstart, int n, int k, int cap,
                                                       int *__restrict__ cols)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    int lo = 0, hi = k - 1;                 // the last cluster that starts at or before q: the one that holds q (empty ones before
    while (lo < hi) {                       // it share its start, the ones after it start past q)
        const int mid = (lo + hi + 1) >> 1;
        if (start[mid] <= q) lo = mid; else hi = mid - 1;
    }
    const int r = q - start[lo];
    if (r < 0 || r >= count[lo]) return;
    const int p = pstart[lo] + r;
    if (p >= 0 && p < cap) cols[p] = members[q];
}

struct ValSilArgs {
    const float *x;                 // [n][d]
    const int *labels;              // [n], clamped to 0 .. k - 1
    const int *cols;                // padded member lists
    const int *count, *pstart;      // [k], [k + 1]
    int n, d, k;
    double *out;                    // [n][3]: s, a, b
    int *nearest;                   // [n]
};

// one staged chunk: dst[t * VAL_LS + r] = x[row(r)][d0 + t], 0 outside; rows from idx (padded lists) or row0 + r.  A wave stores
// 8 (feature group, row group) pieces of 8 x 8: a lane reads 8 consecutive floats of 8 rows (coalesced by row).
__device__ __forceinline__ void val_stage(float *__restrict__ dst, const float *__restrict__ x, const int *__restrict__ idx, int base, int n,
                                          int d, int d0, int tid)
{
    const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int piece = wave * 8 + u, t = (piece & 3) * 8 + (lane & 7), r = (piece >> 2) * 8 + (lane >> 3);
        const int i = idx ? idx[base + r] : base + r;
        float v = 0.f;
        if (i >= 0 && i < n && d0 + t < d) v = x[(size_t)i * d + d0 + t];
        dst[t * VAL_LS + r] = v;
    }
}

__global__ __launch_bounds__(256) void val_silhouette_kernel(ValSilArgs a)
{
    __shared__ __align__(16) float xs[VAL_FC * VAL_LS];
    __shared__ __align__(16) float cs[VAL_FC * VAL_LS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * VAL_TR;
    int lab[4];
    double own[4], best[4], run[4];
    int nid[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = row0 + 4 * ty + i;
        lab[i] = r < a.n ? km_clamp(a.labels[r], a.k) : 0;
        own[i] = 0.0;
        best[i] = __builtin_inf();
        nid[i] = -1;
    }
    const bool one_chunk = a.d <= VAL_FC;
    bool rows_staged = false;
    for (int c = 0; c < a.k; c++) {
        const int nc = a.count[c];
        if (nc <= 0) continue;
#pragma unroll
        for (int i = 0; i < 4; i++) run[i] = 0.0;
        const int p1 = a.pstart[c + 1];
        for (int p0 = a.pstart[c]; p0 < p1; p0 += VAL_TC) {
            float acc[4][4];
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) acc[i][j] = 0.f;
            for (int d0 = 0; d0 < a.d; d0 += VAL_FC) {
                __syncthreads();
                if (!(one_chunk && rows_staged)) val_stage(xs, a.x, nullptr, row0, a.n, a.d, d0, tid);
                val_stage(cs, a.x, a.cols, p0, a.n, a.d, d0, tid);
                rows_staged = true;
                __syncthreads();
                const int tc = min(VAL_FC, a.d - d0);
                for (int t = 0; t < tc; t++) {
                    const float4 xr = *(const float4 *)&xs[t * VAL_LS + 4 * ty];
                    const float4 cv = *(const float4 *)&cs[t * VAL_LS + 4 * tx];
                    const float xv[4] = {xr.x, xr.y, xr.z, xr.w}, cw[4] = {cv.x, cv.y, cv.z, cv.w};
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 4; j++) {
                            const float df = xv[i] - cw[j];
                            acc[i][j] = fmaf(df, df, acc[i][j]);
                        }
                }
            }
            const int4 ci = *(const int4 *)&a.cols[p0 + 4 * tx];
            const bool ok[4] = {ci.x >= 0, ci.y >= 0, ci.z >= 0, ci.w >= 0};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) run[i] += ok[j] ? (double)sqrtf(acc[i][j]) : 0.0;
        }
        // D(i, c): the 16 threads of a row, a fixed butterfly (every lane ends with the same bits)
#pragma unroll
        for (int i = 0; i < 4; i++) {
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) run[i] += __shfl_xor(run[i], m, 64);
            if (c == lab[i]) {
                own[i] = run[i];
            } else {
                const double mean = run[i] / (double)nc;
                if (mean < best[i]) { best[i] = mean; nid[i] = c; }
            }
        }
    }
    if (tx != 0) return;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = row0 + 4 * ty + i;
        if (r >= a.n) continue;
        const int no = a.count[lab[i]];
        const double av = no > 1 ? own[i] / (double)(no - 1) : 0.0;
        const double bv = nid[i] >= 0 ? best[i] : 0.0;
        const double mx = av > bv ? av : bv;
        // sklearn: 0 for a singleton cluster and where the quotient is 0 / 0 (nan_to_num)
        const double sv = (no > 1 && nid[i] >= 0 && mx > 0.0) ? (bv - av) / mx : 0.0;
        a.out[(size_t)r * 3 + 0] = sv;
        a.out[(size_t)r * 3 + 1] = av;
        a.out[(size_t)r * 3 + 2] = bv;
        a.nearest[r] = nid[i];
    }
}

// one block per cluster: cen[c] = sums[c] / count[c] (0 for an empty id), counts[c] = count[c]
__global__ __launch_bounds__(256) void val_centroid_kernel(const double *__restrict__ sums, const int *__restrict__ count, int d,
                                                           double *__restrict__ cen, int *__restrict__ counts)
{
    const int c = blockIdx.x, nc = count[c];
    for (int t = threadIdx.x; t < d; t += 256) cen[(size_t)c * d + t] = nc > 0 ? sums[(size_t)c * d + t] / (double)nc : 0.0;
    if (threadIdx.x == 0) counts[c] = nc;
}

// one block per cluster: sq[c] = sum of dist over the member list, ab[c] = sum of sqrt(dist) (dist [n] = |x_i - mu_label|^2)
__global__ __launch_bounds__(256) void val_disp_kernel(const double *__restrict__ dist, const int *__restrict__ members, const int *__restrict__ count,
                                                       const int *__restrict__ start, int n, double *__restrict__ sq, double *__restrict__ ab)
{
    __shared__ double red[256];
    const int c = blockIdx.x, nc = count[c], s0 = start[c];
    const int per = (nc + 255) / 256, q0 = min(nc, (int)threadIdx.x * per), q1 = min(nc, q0 + per);
    double s2 = 0.0, s1 = 0.0;
    for (int q = q0; q < q1; q++) {
        const double v = dist[km_clamp(members[km_clamp(s0 + q, n)], n)];
        s2 += v;
        s1 += sqrt(v);
    }
    s2 = tsne_block_sum<256>(s2, red);
    s1 = tsne_block_sum<256>(s1, red);
    if (threadIdx.x == 0) {
        sq[c] = s2;
        ab[c] = s1;
    }
}

}  // namespace ralign
