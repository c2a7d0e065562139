// DBSCAN of X [n][d] (scikit-learn 1.7 DBSCAN(eps, min_samples, metric="euclidean")).  The column lists are
// km_column_lists' (ralign_embed.hip: ralign_kmeans.h's member lists padded by ralign_validity.h's kernels); the pair tiling is val_silhouette_kernel's, in double.
//
//   D2(i, j) = sum_t (x_it - x_jt)^2 in double from differences, the features in order, one fma per feature.  x_i - x_j and
//   x_j - x_i differ in sign alone and the chain's order is the same, so D2(i, j) == D2(j, i) bit for bit and D2(i, i) == 0.
//   j is a neighbour of i iff D2(i, j) <= eps2 (= eps * eps, the double product formed on the host).  No f32 screen.
//
//   dbs_count_kernel     one workgroup per DBS_TR rows walks ALL n columns: count_i = neighbours of i (itself included); label_i = i
//                        for a core point (count_i >= min_samples), -1 otherwise.
//   dbs_flag_kernel      0 for a core point, 1 otherwise: the two "clusters" whose member lists give the core points in index order.
//   dbs_min_kernel       one workgroup per DBS_TR rows walks the CORE columns (the padded list, -1 = no column):
//                        m_i = min{label_j : j core, D2(i, j) <= eps2}, INT_MAX without a core neighbour.
//   dbs_hook_kernel      P starts as a copy of label; every core i with m_i < label_i does P[label_i] = min(P[label_i], m_i) and
//                        P[i] = min(P[i], m_i) by integer atomicMin.
//   dbs_compress_kernel  (a launch of its own after the hooks) a core i follows P from i to the fixed point r = P[r] and writes
//                        label_out_i = r; a non-core i writes m_i, or -1 without a core neighbour.  changed counts the core
//                        points whose label moved.
//
// Invariants: a core point's label is a core index of its own component and label_i <= i (true after dbs_count_kernel: label_i = i;
// kept by a round: m_i and every P value are labels of core points of the same component, and a minimum never rises).  Hence
// P[x] <= x for every core x, the walk of dbs_compress_kernel strictly decreases, stays on core indices and ends.  A round in
// which some core i has m_i < label_i gives label_out_i <= P[i] <= m_i < label_i, so every unfinished round lowers a label; when
// no label moves, labels are equal across every core-core edge, i.e. constant on a component, and the constant is the
// component's lowest core index (that point's label is <= itself and inside the component).
//
// Determinism: no floating-point atomics and no floating-point sum across threads at all (a pair's chain lives in one thread).
// The integer minima are minima of sets: the order of the atomics and of the shuffles cannot change them.  No workgroup waits
// for another: ordering comes from separate launches on one stream.  Indices read from memory are range-checked before they
// address anything.
#pragma once

#include <hip/hip_runtime.h>

#include "ralign_validity.h"

namespace ralign {

#define DBS_MAX_N 262144            // n^2 pair distances per pass
#define DBS_MAX_D 2048
#define DBS_TR 64                   // rows per workgroup
#define DBS_TC 64                   // columns per tile (= VAL_TC: the padding of the column list)
#define DBS_FC 32                   // features per chunk in LDS
#define DBS_LS 68                   // LDS stride (doubles) of one feature's 64 values: 32-byte aligned groups of 4
#define DBS_NONE 0x7fffffff         // "no core neighbour"

static_assert(DBS_TC == VAL_TC, "the column list is padded by val_pstart_kernel / val_cols_kernel");

// one staged chunk: dst[t * DBS_LS + r] = (double)x[row(r)][d0 + t], 0 outside; rows from idx (padded list, -1 = none) or base + r
__device__ __forceinline__ void dbs_stage(double *__restrict__ dst, const float *__restrict__ x, const int *__restrict__ idx, int base, int n,
                                          int d, int d0, int tid)
{
    const int wave = tid >> 6, lane = tid & 63, tc = min(DBS_FC, d - d0);
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int piece = wave * 8 + u, t = (piece & 3) * 8 + (lane & 7), r = (piece >> 2) * 8 + (lane >> 3);
        if ((piece & 3) * 8 >= tc) continue;            // features past the chunk's end are never read
        const int i = idx ? idx[base + r] : base + r;
        double v = 0.0;
        if (i >= 0 && i < n && d0 + t < d) v = (double)x[(size_t)i * d + d0 + t];
        dst[t * DBS_LS + r] = v;
    }
}

// acc[i][j] = D2(row 4 ty + i, column 4 tx + j) of the tile whose columns are cols[p0 ..] (cols null: the points p0 ..).  Every
// thread of the workgroup calls it (it synchronises).  rows_staged: the rows' single chunk (d <= DBS_FC) is already in xs.
__device__ __forceinline__ void dbs_tile(double (&acc)[4][4], double *__restrict__ xs, double *__restrict__ cs, const float *__restrict__ x,
                                         const int *__restrict__ cols, int row0, int p0, int n, int d, bool &rows_staged, int tid, int tx,
                                         int ty)
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    const bool one_chunk = d <= DBS_FC;
    for (int d0 = 0; d0 < d; d0 += DBS_FC) {
        __syncthreads();
        if (!(one_chunk && rows_staged)) dbs_stage(xs, x, nullptr, row0, n, d, d0, tid);
        dbs_stage(cs, x, cols, p0, n, d, d0, tid);
        rows_staged = true;
        __syncthreads();
        const int tc = min(DBS_FC, d - d0);
        for (int t = 0; t < tc; t++) {
            const double2 xa = *(const double2 *)&xs[t * DBS_LS + 4 * ty], xb = *(const double2 *)&xs[t * DBS_LS + 4 * ty + 2];
            const double2 ca = *(const double2 *)&cs[t * DBS_LS + 4 * tx], cb = *(const double2 *)&cs[t * DBS_LS + 4 * tx + 2];
            const double xv[4] = {xa.x, xa.y, xb.x, xb.y}, cw[4] = {ca.x, ca.y, cb.x, cb.y};
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double df = xv[i] - cw[j];
                    acc[i][j] = fma(df, df, acc[i][j]);
                }
        }
    }
}

__global__ __launch_bounds__(256) void dbs_count_kernel(const float *__restrict__ x, int n, int d, double eps2, int min_samples,
                                                        int *__restrict__ count, int *__restrict__ label)
{
    __shared__ __align__(32) double xs[DBS_FC * DBS_LS];
    __shared__ __align__(32) double cs[DBS_FC * DBS_LS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * DBS_TR;
    int cnt[4] = {0, 0, 0, 0};
    bool rows_staged = false;
    for (int p0 = 0; p0 < n; p0 += DBS_TC) {
        double acc[4][4];
        dbs_tile(acc, xs, cs, x, nullptr, row0, p0, n, d, rows_staged, tid, tx, ty);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const bool ok = p0 + 4 * tx + j < n;
#pragma unroll
            for (int i = 0; i < 4; i++) cnt[i] += (ok && acc[i][j] <= eps2) ? 1 : 0;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) cnt[i] += __shfl_xor(cnt[i], m, 64);
        const int r = row0 + 4 * ty + i;
        if (tx == 0 && r < n) {
            count[r] = cnt[i];
            label[r] = cnt[i] >= min_samples ? r : -1;
        }
    }
}

__global__ __launch_bounds__(256) void dbs_flag_kernel(const int *__restrict__ count, int n, int min_samples, int *__restrict__ flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) flag[i] = count[i] >= min_samples ? 0 : 1;
}

// cols: the padded list of the core points (index order), pstart[1] its padded length
__global__ __launch_bounds__(256) void dbs_min_kernel(const float *__restrict__ x, int n, int d, double eps2, const int *__restrict__ cols,
                                                      const int *__restrict__ pstart, const int *__restrict__ label, int *__restrict__ mout)
{
    __shared__ __align__(32) double xs[DBS_FC * DBS_LS];
    __shared__ __align__(32) double cs[DBS_FC * DBS_LS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * DBS_TR;
    int best[4] = {DBS_NONE, DBS_NONE, DBS_NONE, DBS_NONE};
    bool rows_staged = false;
    const int p1 = min(pstart[1], n + DBS_TC);          // the list's capacity is n + 2 DBS_TC
    for (int p0 = 0; p0 < p1; p0 += DBS_TC) {
        double acc[4][4];
        dbs_tile(acc, xs, cs, x, cols, row0, p0, n, d, rows_staged, tid, tx, ty);
        const int4 ci = *(const int4 *)&cols[p0 + 4 * tx];
        const int cj[4] = {ci.x, ci.y, ci.z, ci.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (cj[j] < 0 || cj[j] >= n) continue;
            const int lj = label[cj[j]];
            if (lj < 0) continue;
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (acc[i][j] <= eps2) best[i] = min(best[i], lj);
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) best[i] = min(best[i], __shfl_xor(best[i], m, 64));
        const int r = row0 + 4 * ty + i;
        if (tx == 0 && r < n) mout[r] = best[i];
    }
}

__global__ __launch_bounds__(256) void dbs_hook_kernel(const int *__restrict__ count, int n, int min_samples, const int *__restrict__ label,
                                                       const int *__restrict__ m, int *__restrict__ P)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n || count[i] < min_samples) return;
    const int li = label[i], mi = m[i];
    if (li < 0 || li >= n || mi < 0 || mi >= li) return;
    atomicMin(&P[li], mi);
    atomicMin(&P[i], mi);
}

__global__ __launch_bounds__(256) void dbs_compress_kernel(const int *__restrict__ count, int n, int min_samples, const int *__restrict__ label,
                                                           const int *__restrict__ m, const int *__restrict__ P, int *__restrict__ label_out,
                                                           int *__restrict__ changed)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (i < n) {
        int out;
        if (count[i] >= min_samples) {
            int r = i;
            for (;;) {                      // P[r] <= r on core indices: strictly down to the fixed point
                const int p = P[r];
                if (p < 0 || p >= r) break;
                r = p;
            }
            out = r;
            moved = out != label[i];
        } else {
            const int mi = m[i];
            out = (mi >= 0 && mi < n) ? mi : -1;
        }
        label_out[i] = out;
    }
    const unsigned long long b = __ballot(moved);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(changed, (int)__popcll(b));
}

}  // namespace ralign
