// Neighbour ranks for trustworthiness and continuity of an embedding (sklearn.manifold.trustworthiness; DESIGN.md section 4.19;
// the contract, rule by rule, is at the top of cryo_ralib_amd/quality.py).  The pair tiling is dbs_count_kernel's (ralign_dbscan.h),
// the single-pair chain hdb_d2 (ralign_hdbscan.h).
//
//   D2(i, j) = sum_t (x_it - x_jt)^2 in double from differences, the features in order, one fma per feature: dbs_tile and hdb_d2
//   run the same chain, so a column's D2 in the row pass equals the threshold of the list entry that names it bit for bit.
//   In the row of i, column l precedes column j iff (D2(i, l), l) < (D2(i, j), j); rank(i, j) = 1 + #{l != i : l precedes j}.
//
//   emb_thr_kernel   thr[i][t] = D2(i, idx[i][t]) by hdb_d2; an entry outside 0 .. n - 1, or equal to i, is invalid: thr = -1.
//                    The index is range-checked before it addresses anything.
//   emb_rank_kernel  one workgroup per DBS_TR rows walks ALL n columns through dbs_tile, once per chunk of at most EMB_KC list
//                    entries.  A chunk's entries are sorted by (thr, j) into LDS (a rank sort; list position breaks the ties of a
//                    repeated entry, which leaves equal keys adjacent).  Each thread keeps the largest threshold of its 4 rows in
//                    registers: a column beyond it costs one compare.  Any other column finds, by binary search, the first sorted
//                    entry p it precedes (it then precedes every later one) and bumps the integer LDS counter bin[row][p].  The
//                    running sum of bin over the sorted entries is the number of preceding columns: rank = 1 + sum, 0 for an
//                    invalid entry.  pen_i = sum_t max(0, rank - k) (int64) is kept by the thread that writes the row's ranks and
//                    stored once after the last chunk, so a large rank table need not exist.
//
// LDS: dbs_tile's two static arrays (34816 bytes) and 16 bytes per (row, entry) of dynamic LDS at a row stride of kc + 1 entries
// (kc = min(k, EMB_KC): the threshold 8, the index with the list position packed above it 4, the counter 4).  The odd stride
// spreads the 4 rows a wave searches at a time over the banks; the 16 lanes that share a row read one address (a broadcast).
//
// Determinism: the counts are integers, LDS atomicAdd of 1 in any order gives the same sums; no floating-point atomics and no
// floating-point sum across threads (a pair's chain lives in one thread).  No workgroup waits for another.
#pragma once

#include <hip/hip_runtime.h>

#include "ralign_dbscan.h"
#include "ralign_hdbscan.h"

namespace ralign {

#define EMB_MAX_N DBS_MAX_N
#define EMB_MAX_D DBS_MAX_D
#define EMB_MAX_K 301               // ra_tsne_knn's longest list
#define EMB_KC 24                   // list entries per pass of the row kernel
#define EMB_JBITS 18                // an index below EMB_MAX_N; the entry's position in the chunk sits above it
#define EMB_JMASK ((1 << EMB_JBITS) - 1)

static_assert(EMB_MAX_N <= (1 << EMB_JBITS) && EMB_KC < (1 << (31 - EMB_JBITS)), "index and chunk position share one int");

// dynamic LDS of emb_rank_kernel for chunks of kc entries
inline size_t emb_rank_lds(int kc) { return (size_t)DBS_TR * (kc + 1) * 16; }

__global__ __launch_bounds__(256) void emb_thr_kernel(const float *__restrict__ x, int n, int d, const int *__restrict__ idx, int k,
                                                      double *__restrict__ thr)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)n * k) return;
    const int i = (int)(e / k), j = idx[e];
    double v = -1.0;
    if (j >= 0 && j < n && j != i) {
        v = hdb_d2(x, d, i, j);
        if (!(v >= 0.0)) v = -1.0;          // NaN from non-finite input: invalid, so that the keys stay totally ordered
    }
    thr[e] = v;
}

struct EmbRankArgs {
    const float *x;
    const int *idx;         // [n][k]
    const double *thr;      // [n][k], emb_thr_kernel's
    int n, d, k, kc;        // kc = min(k, EMB_KC)
    int *rank;              // [n][k] or null
    long long *pen;         // [n] or null
};

__global__ __launch_bounds__(256) void emb_rank_kernel(const EmbRankArgs a)
{
    __shared__ __align__(32) double xs[DBS_FC * DBS_LS];
    __shared__ __align__(32) double cs[DBS_FC * DBS_LS];
    extern __shared__ __align__(16) unsigned char emb_dyn[];
    const int n = a.n, k = a.k, kc = a.kc, ks = kc + 1;
    double *sthr = (double *)emb_dyn;           // [DBS_TR][ks] thresholds, ascending by (thr, j)
    int *sjt = (int *)(sthr + DBS_TR * ks);     // [DBS_TR][ks] j | position in the chunk << EMB_JBITS
    int *bin = sjt + DBS_TR * ks;               // [DBS_TR][ks] columns whose first preceded entry is this one
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * DBS_TR;
    long long pen = 0;                          // of row row0 + tid (tid < DBS_TR)
    bool rows_staged = false;
    for (int c0 = 0; c0 < k; c0 += kc) {
        const int kcur = min(kc, k - c0);
        __syncthreads();                        // the last chunk's ranks are out
        for (int item = tid; item < DBS_TR * kcur; item += 256) {
            const int r = item / kcur, e = item - r * kcur, row = row0 + r;
            bin[r * ks + e] = 0;
            if (row >= n) {
                sthr[r * ks + e] = -1.0;
                sjt[r * ks + e] = e << EMB_JBITS;
                continue;
            }
            const double *tr = a.thr + (size_t)row * k + c0;
            const int *ir = a.idx + (size_t)row * k + c0;
            const double te = tr[e];
            const int je = te < 0.0 ? 0 : (ir[e] & EMB_JMASK);
            int pos = 0;
            for (int f = 0; f < kcur; f++) {
                const double tf = tr[f];
                const int jf = tf < 0.0 ? 0 : (ir[f] & EMB_JMASK);
                pos += (tf < te || (tf == te && (jf < je || (jf == je && f < e)))) ? 1 : 0;
            }
            sthr[r * ks + pos] = te;
            sjt[r * ks + pos] = je | (e << EMB_JBITS);
        }
        __syncthreads();
        double mx[4];                           // the row's largest threshold; -1 (below every D2) without a valid entry
#pragma unroll
        for (int i = 0; i < 4; i++) mx[i] = sthr[(4 * ty + i) * ks + kcur - 1];
        for (int p0 = 0; p0 < n; p0 += DBS_TC) {
            double acc[4][4];
            dbs_tile(acc, xs, cs, a.x, nullptr, row0, p0, n, a.d, rows_staged, tid, tx, ty);
#pragma unroll
            for (int i = 0; i < 4; i++) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double v = acc[i][j];
                    const int col = p0 + 4 * tx + j;
                    if (!(v <= mx[i]) || col >= n || col == row0 + 4 * ty + i) continue;
                    const double *st = sthr + (4 * ty + i) * ks;
                    const int *sj = sjt + (4 * ty + i) * ks;
                    int lo = 0, hi = kcur;      // the first entry with (thr, j) > (v, col)
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        const double t = st[mid];
                        if (t > v || (t == v && (sj[mid] & EMB_JMASK) > col)) hi = mid;
                        else lo = mid + 1;
                    }
                    if (lo < kcur) atomicAdd(&bin[(4 * ty + i) * ks + lo], 1);
                }
            }
        }
        __syncthreads();
        if (tid < DBS_TR && row0 + tid < n) {
            const size_t out = (size_t)(row0 + tid) * k + c0;
            int cum = 0;
            for (int s = 0; s < kcur; s++) {
                cum += bin[tid * ks + s];
                const int e = min(sjt[tid * ks + s] >> EMB_JBITS, kcur - 1);
                const int rk = sthr[tid * ks + s] < 0.0 ? 0 : 1 + cum;
                if (a.rank) a.rank[out + e] = rk;
                pen += max(0, rk - k);
            }
        }
    }
    if (a.pen && tid < DBS_TR && row0 + tid < n) a.pen[row0 + tid] = pen;
}

}  // namespace ralign
