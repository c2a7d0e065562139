// Ward (minimum-variance) agglomeration of X [n][d] (the contract at the top of cryo_ralib_amd/ward.py): the
// nearest-neighbour pass of one round and the update of the merged clusters.  A cluster is (centroid c [d] in double, size s) in a
// slot 0 .. n - 1; a slot with size <= 0 is dead.  The pair tiling is ralign_dbscan.h's: ward_stage / ward_tile are dbs_stage /
// dbs_tile with a double source and an index list on both sides, and the D2 chain is the same: differences in double, the
// features in order, one fma per feature, exactly symmetric.  Nothing of size n^2 is stored.
//
//   W2(a, b) = f D2(c_a, c_b), f = (s_a s_b) / (s_a + s_b) with the sizes in double (s_a s_b < 2^36 is exact): one multiply, one
//   add, one divide and one multiply, each commutative, so W2(a, b) == W2(b, a) bit for bit.
//
//   ward_row_kernel    one workgroup per WARD_TR listed rows walks the padded list of live columns (slot order, -1 = no column) in
//                      64 x 64 tiles: per row the least (W2, slot) over the live columns other than the row's own slot.  A thread
//                      visits its columns upwards and takes one only when W2 is strictly less; the 16 lanes of a row then reduce
//                      (bits of W2, slot) (non-negative doubles order as their bits).  nn and w2 are written by list position.  A
//                      listed row that is dead or outside 0 .. n - 1, or that has no other live cluster, gives (-1, +inf) and
//                      addresses nothing.
//   ward_merge_kernel  one thread per (pair, feature): c_a <- (s_a c_a + s_b c_b) / (s_a + s_b), the sum formed by one fma.  It
//                      reads the sizes and writes centroids only.
//   ward_size_kernel   (a launch of its own) one thread per pair: s_a <- s_a + s_b, s_b <- 0.
//                      Both skip a pair outside 0 <= a < b < n or with a dead member; the pairs of one call are disjoint.
//
// The live column list is the member list of "cluster" 0 of dbs_flag_kernel(size, min_samples = 1), padded by km_column_lists
// (ralign_embed.hip), as DBSCAN's core columns are.
//
// Determinism: no floating-point atomics and no floating-point sum across threads (a pair's chain lives in one thread); the
// minimum is that of a set, so the order of the shuffles cannot change it.  No workgroup waits for another: ordering comes from
// separate launches on one stream.  Indices read from memory are range-checked before they address anything.
#pragma once

#include <hip/hip_runtime.h>

#include "ralign_dbscan.h"

namespace ralign {

#define WARD_MAX_N DBS_MAX_N
#define WARD_MAX_D DBS_MAX_D
#define WARD_TR DBS_TR
#define WARD_NONE 0xffffffffffffffffull         // above the bits of every finite double and of +inf, and above every slot

// one staged chunk: dst[t * DBS_LS + r] = c[idx[base + r]][d0 + t], 0 for a position at or past `len`, for an index outside
// 0 .. n - 1 and for a feature past d
__device__ __forceinline__ void ward_stage(double *__restrict__ dst, const double *__restrict__ c, const int *__restrict__ idx, int base,
                                           int len, int n, int d, int d0, int tid)
{
    const int wave = tid >> 6, lane = tid & 63, tc = min(DBS_FC, d - d0);
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int piece = wave * 8 + u, t = (piece & 3) * 8 + (lane & 7), r = (piece >> 2) * 8 + (lane >> 3);
        if ((piece & 3) * 8 >= tc) continue;            // features past the chunk's end are never read
        const int i = base + r < len ? idx[base + r] : -1;
        double v = 0.0;
        if (i >= 0 && i < n && d0 + t < d) v = c[(size_t)i * d + d0 + t];
        dst[t * DBS_LS + r] = v;
    }
}

// acc[i][j] = D2(row rows[row0 + 4 ty + i], column cols[p0 + 4 tx + j]): dbs_tile's chain on the centroid table.  Every thread
// of the workgroup calls it (it synchronises).  rows_staged: the rows' single chunk (d <= DBS_FC) is already in xs.
__device__ __forceinline__ void ward_tile(double (&acc)[4][4], double *__restrict__ xs, double *__restrict__ cs, const double *__restrict__ c,
                                          const int *__restrict__ rows, int row0, int n_rows, const int *__restrict__ cols, int p0,
                                          int n_cols, int n, int d, bool &rows_staged, int tid, int tx, int ty)
{
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) acc[i][j] = 0.0;
    const bool one_chunk = d <= DBS_FC;
    for (int d0 = 0; d0 < d; d0 += DBS_FC) {
        __syncthreads();
        if (!(one_chunk && rows_staged)) ward_stage(xs, c, rows, row0, n_rows, n, d, d0, tid);
        ward_stage(cs, c, cols, p0, n_cols, n, d, d0, tid);
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

// cols: the padded list of the live slots (slot order), pstart[1] its padded length; nn / w2 [n_rows] by list position
__global__ __launch_bounds__(256) void ward_row_kernel(const double *__restrict__ c, const int *__restrict__ size, int n, int d,
                                                       const int *__restrict__ rows, int n_rows, const int *__restrict__ cols,
                                                       const int *__restrict__ pstart, int *__restrict__ nn, double *__restrict__ w2)
{
    __shared__ __align__(32) double xs[DBS_FC * DBS_LS];
    __shared__ __align__(32) double cs[DBS_FC * DBS_LS];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * WARD_TR;
    int ra[4], bc[4];
    double sa[4], bw[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int q = row0 + 4 * ty + i;
        int a = q < n_rows ? rows[q] : -1;
        int s = 0;
        if (a >= 0 && a < n) s = size[a];
        if (s <= 0) a = -1;                             // dead or out of range: no candidate is ever taken
        ra[i] = a;
        sa[i] = (double)s;
        bw[i] = 0.0;
        bc[i] = -1;                                     // no column yet
    }
    bool rows_staged = false;
    const int p1 = min(pstart[1], n + DBS_TC);          // the list's capacity is n + 2 DBS_TC
    for (int p0 = 0; p0 < p1; p0 += DBS_TC) {
        double acc[4][4];
        ward_tile(acc, xs, cs, c, rows, row0, n_rows, cols, p0, p1, n, d, rows_staged, tid, tx, ty);
        const int4 ci = *(const int4 *)&cols[p0 + 4 * tx];
        const int cj[4] = {ci.x, ci.y, ci.z, ci.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (cj[j] < 0 || cj[j] >= n) continue;
            const int sj = size[cj[j]];
            if (sj <= 0) continue;
            const double sb = (double)sj;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                // equal sizes: s s / (2 s) = s / 2 exactly, the quotient the division rounds to; a wave of such pairs (round 0,
                // where every size is 1) skips the division
                double f = 0.5 * sb;
                if (sa[i] != sb) f = (sa[i] * sb) / (sa[i] + sb);
                const double w = f * acc[i][j];
                if (ra[i] >= 0 && cj[j] != ra[i] && (bc[i] < 0 || w < bw[i])) {
                    bw[i] = w;
                    bc[i] = cj[j];
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        // (bits of W2, slot): both orders are those of unsigned integers; a lane without a column holds WARD_NONE twice
        unsigned long long kw = bc[i] >= 0 ? (unsigned long long)__double_as_longlong(bw[i]) : WARD_NONE;
        unsigned long long kc = bc[i] >= 0 ? (unsigned long long)bc[i] : WARD_NONE;
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) {
            const unsigned long long ow = __shfl_xor(kw, m, 64), oc = __shfl_xor(kc, m, 64);
            if (ow < kw || (ow == kw && oc < kc)) {
                kw = ow;
                kc = oc;
            }
        }
        const int q = row0 + 4 * ty + i;
        if (tx == 0 && q < n_rows) {
            const bool found = kc != WARD_NONE;
            nn[q] = found ? (int)kc : -1;
            w2[q] = __longlong_as_double(found ? (long long)kw : 0x7ff0000000000000ll);
        }
    }
}

__device__ __forceinline__ bool ward_pair_ok(const int *__restrict__ size, int n, int a, int b)
{
    return a >= 0 && a < b && b < n && size[a] > 0 && size[b] > 0;
}

__global__ __launch_bounds__(256) void ward_merge_kernel(double *__restrict__ c, const int *__restrict__ size, int n, int d,
                                                         const int *__restrict__ pa, const int *__restrict__ pb, int n_pairs)
{
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= (size_t)n_pairs * d) return;
    const int p = (int)(g / d), t = (int)(g - (size_t)p * d);
    const int a = pa[p], b = pb[p];
    if (!ward_pair_ok(size, n, a, b)) return;
    const double sa = (double)size[a], sb = (double)size[b];
    const double ca = c[(size_t)a * d + t], cb = c[(size_t)b * d + t];
    c[(size_t)a * d + t] = fma(sa, ca, sb * cb) / (sa + sb);
}

__global__ __launch_bounds__(256) void ward_size_kernel(int *__restrict__ size, int n, const int *__restrict__ pa, const int *__restrict__ pb,
                                                        int n_pairs)
{
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pairs) return;
    const int a = pa[p], b = pb[p];
    if (!ward_pair_ok(size, n, a, b)) return;
    size[a] += size[b];
    size[b] = 0;
}

}  // namespace ralign
