// HDBSCAN of X [n][d] (the contract at the top of cryo_ralib_amd/hdbscan.py): the core distances and one
// Boruvka round of the minimum spanning tree of the mutual-reachability graph.  The pair tiling and the distance chain are
// ralign_dbscan.h's dbs_tile: D2(i, j) = sum_t (x_it - x_jt)^2 in double from differences, the features in order, one fma per
// feature, exactly symmetric and 0 on the diagonal.  hdb_d2 is the same chain for one pair.  Nothing of size n^2 is stored.
//
//   w2(i, j) = max(core2_i, core2_j, D2(i, j)); edges are totally ordered by (w2, min(i, j), max(i, j)).  For a fixed row i that
//   order over the columns j is (w2, j): the columns below i give (j, i), those above (i, j), and every j < i sorts before every
//   j > i.  A row therefore keeps (w2, j) and takes a new column only when its w2 is strictly less: columns are visited upwards.
//
//   hdb_core_kernel  core2_i = D2(i, idx[i][k - 1]), the k-th neighbour of ra_tsne_knn's index list (k = min_samples - 1),
//                    recomputed by hdb_d2; an index outside 0 .. n - 1 gives 0 and addresses nothing.
//   hdb_row_kernel   one workgroup per DBS_TR rows walks ALL n columns: the least (w2, j) of row i over the columns of another
//                    component, reduced across the 16 lanes that share a row.  roww_i = the bits of w2, rowe_i = lo << 32 | hi;
//                    HDB_NONE for both when the row's component holds every point.
//   hdb_minw_kernel  cw[comp_i] = min(cw[comp_i], roww_i) by integer atomicMin (non-negative doubles order as their bits).
//   hdb_mine_kernel  (a launch of its own) among the rows with roww_i == cw[comp_i]: ce[comp_i] = min(ce[comp_i], rowe_i).
//   hdb_out_kernel   (a launch of its own) at a root i = comp_i with an edge: w2_i, lo_i, hi_i; everywhere else +inf, -1, -1.
//
// Determinism: no floating-point atomics and no floating-point sum across threads (a pair's chain lives in one thread); the
// minima are minima of sets, so neither the order of the atomics nor that of the shuffles can change them.  No workgroup waits
// for another: ordering comes from separate launches on one stream.  comp values are compared in hdb_row_kernel and
// range-checked before they address cw / ce.
#pragma once

#include <hip/hip_runtime.h>

#include "ralign_dbscan.h"

namespace ralign {

#define HDB_MAX_N DBS_MAX_N
#define HDB_MAX_D DBS_MAX_D
#define HDB_MAX_MIN_SAMPLES 302                 // ra_tsne_knn's 301 neighbours and the point itself
#define HDB_NONE 0xffffffffffffffffull          // above the bits of every finite double and of every packed edge

// rule 2's chain for one pair: the same operations in the same order as dbs_tile
__device__ __forceinline__ double hdb_d2(const float *__restrict__ x, int d, int i, int j)
{
    const float *xi = x + (size_t)i * d, *xj = x + (size_t)j * d;
    double acc = 0.0;
    for (int t = 0; t < d; t++) {
        const double df = (double)xi[t] - (double)xj[t];
        acc = fma(df, df, acc);
    }
    return acc;
}

__global__ __launch_bounds__(256) void hdb_core_kernel(const float *__restrict__ x, int n, int d, const int *__restrict__ idx, int k,
                                                       double *__restrict__ core2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int j = idx[(size_t)i * k + k - 1];
    core2[i] = (j >= 0 && j < n) ? hdb_d2(x, d, i, j) : 0.0;
}

__global__ __launch_bounds__(256) void hdb_row_kernel(const float *__restrict__ x, int n, int d, const double *__restrict__ core2,
                                                      const int *__restrict__ comp, unsigned long long *__restrict__ roww,
                                                      unsigned long long *__restrict__ rowe)
{
    __shared__ __align__(32) double xs[DBS_FC * DBS_LS];
    __shared__ __align__(32) double cs[DBS_FC * DBS_LS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * DBS_TR;
    double rcore[4], bw[4];
    int rcomp[4], bc[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int r = row0 + 4 * ty + i;
        rcore[i] = r < n ? core2[r] : 0.0;
        rcomp[i] = r < n ? comp[r] : -1;
        bw[i] = 0.0;
        bc[i] = -1;                                     // no column yet
    }
    bool rows_staged = false;
    for (int p0 = 0; p0 < n; p0 += DBS_TC) {
        double acc[4][4];
        dbs_tile(acc, xs, cs, x, nullptr, row0, p0, n, d, rows_staged, tid, tx, ty);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = p0 + 4 * tx + j;
            if (c >= n) continue;
            const double ccore = core2[c];
            const int ccomp = comp[c];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const double w = fmax(fmax(acc[i][j], rcore[i]), ccore);
                if (ccomp != rcomp[i] && (bc[i] < 0 || w < bw[i])) {
                    bw[i] = w;
                    bc[i] = c;
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        // (bits of w2, column): both orders are those of unsigned integers; a lane without a column holds HDB_NONE twice
        unsigned long long kw = bc[i] >= 0 ? (unsigned long long)__double_as_longlong(bw[i]) : HDB_NONE;
        unsigned long long kc = bc[i] >= 0 ? (unsigned long long)bc[i] : HDB_NONE;
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const unsigned long long ow = __shfl_xor(kw, m, 64), oc = __shfl_xor(kc, m, 64);
            if (ow < kw || (ow == kw && oc < kc)) {
                kw = ow;
                kc = oc;
            }
        }
        const int r = row0 + 4 * ty + i;
        if (tx == 0 && r < n) {
            roww[r] = kw;
            const unsigned long long lo = kc < (unsigned long long)r ? kc : (unsigned long long)r;
            const unsigned long long hi = kc < (unsigned long long)r ? (unsigned long long)r : kc;
            rowe[r] = kw == HDB_NONE ? HDB_NONE : (lo << 32 | hi);
        }
    }
}

__global__ __launch_bounds__(256) void hdb_minw_kernel(const int *__restrict__ comp, int n, const unsigned long long *__restrict__ roww,
                                                       unsigned long long *__restrict__ cw)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = comp[i];
    const unsigned long long w = roww[i];
    if (c < 0 || c >= n || w == HDB_NONE) return;
    atomicMin(&cw[c], w);
}

__global__ __launch_bounds__(256) void hdb_mine_kernel(const int *__restrict__ comp, int n, const unsigned long long *__restrict__ roww,
                                                       const unsigned long long *__restrict__ rowe, const unsigned long long *__restrict__ cw,
                                                       unsigned long long *__restrict__ ce)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = comp[i];
    const unsigned long long w = roww[i];
    if (c < 0 || c >= n || w == HDB_NONE || w != cw[c]) return;
    atomicMin(&ce[c], rowe[i]);
}

__global__ __launch_bounds__(256) void hdb_out_kernel(const int *__restrict__ comp, int n, const unsigned long long *__restrict__ cw,
                                                      const unsigned long long *__restrict__ ce, double *__restrict__ w2, int *__restrict__ lo,
                                                      int *__restrict__ hi)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const bool edge = comp[i] == i && cw[i] != HDB_NONE && ce[i] != HDB_NONE;
    w2[i] = edge ? __longlong_as_double((long long)cw[i]) : __longlong_as_double(0x7ff0000000000000ll);
    lo[i] = edge ? (int)(ce[i] >> 32) : -1;
    hi[i] = edge ? (int)(ce[i] & 0xffffffffull) : -1;
}

}  // namespace ralign
