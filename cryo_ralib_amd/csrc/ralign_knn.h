// Exact k nearest neighbours of rows q [nq][d] among rows x [m][d]: the lists under t-SNE, UMAP, spectral embedding, embedding
// quality, DBSCAN's k-distances and HDBSCAN's core distances (ra_tsne_knn, ra_tsne_knn_query in ralign_embed.hip).
//
//   tsne_sqnorm_kernel      |x_i|^2 per row (double sum, rounded once), for the Gram distances here and for k-means' E-step.
//   tsne_knn_body<SELF>     the one body: Gram distance tiles |q_i|^2 + |x_j|^2 - 2 q_i.x_j on v_mfma_f32_16x16x4_f32, a streaming
//                           per-row top-C selection in LDS, then the C survivors re-ranked by squared distances computed in double
//                           from q_i - x_j (the features in order); writes the k best by (distance, index).
//   tsne_knn_kernel         SELF: the rows against themselves, row i left out of its own list; C = min(m - 1, k + TSNE_KNN_MARGIN).
//   tsne_knn_query_kernel   separate query rows, nothing left out; C = min(m, k + TSNE_KNN_MARGIN).
//
// The list's append order varies (an LDS integer counter), but only its set is used: every cut is by the total order (distance,
// index).
#pragma once

#include <hip/hip_runtime.h>

namespace ralign {

#define TSNE_KNN_THREADS 256        // 4 waves; the workgroup owns 16 query rows, a wave 16 candidate columns of each tile
#define TSNE_KNN_TILE 64            // candidate columns per tile
#define TSNE_KNN_MARGIN 32          // survivors kept beyond k for the double re-rank
#define TSNE_KNN_SLACK 256          // list capacity beyond C: a compaction every >= 192 accepted candidates
#define TSNE_MAX_K 301              // k = int(3 perplexity + 1) at perplexity 100
#define TSNE_MAX_N 262144
#define TSNE_MAX_D 2048
#define TSNE_MAX_NQ 4194304

__device__ __forceinline__ const float *x_row_or_null(const float *x, int i, int n, int d)
{
    return i < n ? x + (size_t)i * d : nullptr;
}

__device__ __forceinline__ float tsne_not_nan(float v) { return v != v ? __builtin_inff() : v; }

__device__ __forceinline__ bool tsne_key_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

__device__ __forceinline__ bool tsne_key_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

__global__ __launch_bounds__(256) void tsne_sqnorm_kernel(const float *__restrict__ x, int n, int d, float *__restrict__ nrm)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *xi = x + (size_t)i * d;
    double s = 0.0;
    for (int t = 0; t < d; t++) s += (double)xi[t] * (double)xi[t];
    nrm[i] = (float)s;
}

struct TsneKnnArgs {
    const float *q, *qnrm;          // query rows [nq][d] and their squared norms; tsne_knn_kernel reads x, xnrm and m in their place
    const float *x, *xnrm;          // base rows [m][d]
    int nq, m, d, k, C, cap;        // C survivors per row, cap list capacity (C + TSNE_KNN_SLACK)
    int *idx;                       // [nq][k]
    double *dist2;                  // [nq][k]
};

// LDS: exact distances [16][C] double, tile [16][64] float, list distances [16][cap] float, list indices [16][cap] int.
// SELF: the query rows are the base rows (taken from x, xnrm and m, so the compiler knows they are equal) and column i is left out
// of row i
template <bool SELF>
__device__ __forceinline__ void tsne_knn_body(const TsneKnnArgs &a)
{
    const float *q = SELF ? a.x : a.q, *qnrm = SELF ? a.xnrm : a.qnrm;
    const int nq = SELF ? a.m : a.nq;

    extern __shared__ __align__(16) unsigned char tsne_smem[];
    double *ex = (double *)tsne_smem;
    float *tile = (float *)(ex + 16 * a.C);
    float *ld = tile + 16 * TSNE_KNN_TILE;
    int *li = (int *)(ld + 16 * a.cap);
    __shared__ int cnt[16], full[16], thr_i[16];
    __shared__ float thr_d[16];

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.x * 16;
    const int row = tid >> 4, sub = tid & 15, gi = i0 + row;   // selection: 16 lanes per query row
    if (tid < 16) { cnt[tid] = 0; full[tid] = 0; thr_d[tid] = __builtin_inff(); thr_i[tid] = 0; }
    __syncthreads();

    // keep the C smallest (distance, index) of the rows whose list holds more than `limit`; workgroup-uniform
    auto compact = [&](int limit) {
        const int c = cnt[row];
        const bool act = gi < nq && c > limit;
        float *rd = ld + row * a.cap;
        int *ri = li + row * a.cap;
        if (act) {
            for (int e = sub; e < c; e += 16) {
                const float de = rd[e];
                const int ie = ri[e];
                int rank = 0;
                for (int f = 0; f < c; f++) rank += tsne_key_less(rd[f], ri[f], de, ie) ? 1 : 0;
                if (rank == a.C - 1) { thr_d[row] = de; thr_i[row] = ie; }
            }
        }
        __syncthreads();
        if (act) {
            const float td = thr_d[row];
            const int ti = thr_i[row];
            int base = 0;
            // in-place stream compaction, 16 entries at a time: all lanes of the row read their entry before any write, and
            // every write lands below the next chunk
            for (int c0 = 0; c0 < c; c0 += 16) {
                const int e = c0 + sub;
                float dv = 0.f;
                int iv = 0;
                bool keep = false;
                if (e < c) { dv = rd[e]; iv = ri[e]; keep = !tsne_key_less(td, ti, dv, iv); }
                const unsigned long long b = __ballot(keep);
                const unsigned grp = (unsigned)(b >> (lane & 48)) & 0xffffu;
                const int pre = __popc(grp & ((1u << sub) - 1u));
                if (keep) { rd[base + pre] = dv; ri[base + pre] = iv; }
                base += __popc(grp);
            }
            if (sub == 0) { cnt[row] = base; full[row] = 1; }
        }
        __syncthreads();
    };

    const int qi = i0 + lr;
    const float *xq = x_row_or_null(q, qi, nq, a.d);
    for (int j0 = 0; j0 < a.m; j0 += TSNE_KNN_TILE) {
        // Gram tile: rows i0 .. i0 + 15 x columns j0 + 16 wave .. + 15
        const int cj = j0 + wave * 16 + lr;
        const float *xc = x_row_or_null(a.x, cj, a.m, a.d);
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int k0 = 0; k0 < a.d; k0 += 4) {
            const int kk = k0 + lk;
            const float av = (xq && kk < a.d) ? xq[kk] : 0.f;
            const float bv = (xc && kk < a.d) ? xc[kk] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
        const float nc = cj < a.m ? a.xnrm[cj] : 0.f;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int orow = lk * 4 + r;
            const float nr = i0 + orow < nq ? qnrm[i0 + orow] : 0.f;
            tile[orow * TSNE_KNN_TILE + wave * 16 + lr] = tsne_not_nan(nr + nc - 2.f * acc[r]);
        }
        __syncthreads();
        if (gi < nq) {
            const bool fl = full[row] != 0;
            const float td = thr_d[row];
#pragma unroll
            for (int t = 0; t < TSNE_KNN_TILE / 16; t++) {
                const int col = sub + 16 * t, j = j0 + col;
                if (j >= a.m || (SELF && j == gi)) continue;
                const float dv = tile[row * TSNE_KNN_TILE + col];
                // columns arrive in increasing index order, so a distance equal to the cut loses to the kept entry
                if (!fl || dv < td) {
                    const int pos = atomicAdd(&cnt[row], 1);
                    ld[row * a.cap + pos] = dv;
                    li[row * a.cap + pos] = j;
                }
            }
        }
        __syncthreads();
        bool over = false;
#pragma unroll
        for (int r = 0; r < 16; r++) over |= cnt[r] > a.cap - TSNE_KNN_TILE;
        if (over) compact(a.cap - TSNE_KNN_TILE);
    }
    compact(a.C);

    // re-rank the survivors by the exact squared distance (double, from q_i - x_j, the features in order)
    const int c = gi < nq ? cnt[row] : 0;
    const float *xi = q + (size_t)min(gi, nq - 1) * a.d;
    double *rx = ex + row * a.C;
    const int *ri = li + row * a.cap;
    for (int e = sub; e < c; e += 16) {
        const float *xj = a.x + (size_t)ri[e] * a.d;
        double s = 0.0;
        for (int t = 0; t < a.d; t++) {
            const double df = (double)xi[t] - (double)xj[t];
            s += df * df;
        }
        rx[e] = s != s ? __builtin_inf() : s;
    }
    __syncthreads();
    for (int e = sub; e < c; e += 16) {
        const double de = rx[e];
        const int ie = ri[e];
        int rank = 0;
        for (int f = 0; f < c; f++) rank += tsne_key_less(rx[f], ri[f], de, ie) ? 1 : 0;
        if (rank < a.k) {
            a.idx[(size_t)gi * a.k + rank] = ie;
            a.dist2[(size_t)gi * a.k + rank] = de;
        }
    }
}

__global__ __launch_bounds__(TSNE_KNN_THREADS) void tsne_knn_kernel(TsneKnnArgs a) { tsne_knn_body<true>(a); }

__global__ __launch_bounds__(TSNE_KNN_THREADS) void tsne_knn_query_kernel(TsneKnnArgs a) { tsne_knn_body<false>(a); }

} // namespace ralign
