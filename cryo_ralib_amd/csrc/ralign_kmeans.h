// k-means of X [n][d] (scikit-learn 1.7 KMeans(algorithm="lloyd") with uniform weights).
//
//   km_prep_kernel           the f32 copy of the double centres and its squared norms, for the screen.
//   km_assign_small_kernel   d <= KM_SMALL_D: every point-centre distance in double from x - c; first index on ties.
//   km_assign_mfma_kernel    d > KM_SMALL_D: Gram tiles |x|^2 + |c|^2 - 2 x.c on v_mfma_f32_16x16x4_f32 screen the centres; every
//                            centre whose f32 distance lies within the proven error bound of the row's minimum is re-evaluated in
//                            double from x - c (a fixed butterfly over the wave), and the label is the (distance, index) minimum.
//   km_hist_kernel / km_offsets_kernel / km_starts_kernel / km_scatter_kernel
//                            stable member lists: per-block label counts (integer LDS atomics), per-cluster offsets, then every
//                            point placed at its rank in index order (ballot ranks inside a wave, wave counts inside a block).
//   km_runsum_kernel         double sums of runs of KM run length members (index order) of one cluster.
//   km_combine_kernel        the runs of a cluster added in run order: its member sum and weight.
//   km_relocate_kernel       sklearn's _relocate_empty_clusters_dense: the points farthest from their centre (decreasing
//                            distance, ties by lower index) become the empty clusters' sums; the donors lose them.
//   km_update_kernel         centre = sum * (1 / weight) (weight 0: sklearn's copy of the heaviest cluster), |c_new - c_old|^2.
//   km_stats_kernel          the centre shift total and the changed-label count of one Lloyd iteration.
//   km_point_dist_kernel     |x - c_label|^2 for given labels (inertia without assignment).
//   km_segsum_kernel / km_segscan_kernel / km_search_kernel
//                            a fixed-order double prefix sum of the k-means++ weights and np.searchsorted (side left) in it.
//   km_cand_dist_kernel / km_pick_kernel / km_commit_kernel
//                            k-means++ candidate potentials sum_i min(closest_i, d^2(x_i, cand)), the first minimum, and the
//                            chosen candidate folded into closest_dist_sq.
//
// Determinism: no atomics on floating-point data. Every floating-point sum has an order fixed by (n, d, k) and the labels alone.
// Integer counters (block histograms, changed labels) use atomics; the candidate lists of the screen are filled in any order but
// only their set is used (the winner is the minimum of the total order (distance, index)). Indices read from data are clamped
// before they address anything.
#pragma once

#include <hip/hip_runtime.h>

#include "ralign_tsne.h"

namespace ralign {

#define KM_MAX_N 4194304
#define KM_MAX_D 2048
#define KM_MAX_K 256
#define KM_MAX_M 16                 // k-means++ candidates per seeding call
#define KM_SMALL_D 8                // d <= 8: every distance in double, no screen
#define KM_WAVES 8
#define KM_ROWS (16 * KM_WAVES)     // rows per workgroup of the screened assignment (16 per wave)
#define KM_KC 32                    // features per centre chunk in LDS
#define KM_KS 36                    // LDS row stride of the chunk (lanes of one MFMA operand read hit distinct banks)
#define KM_CAP 16                   // candidates per row re-evaluated in double (more: every centre)
#define KM_BLOCK 1024               // points per block of the member lists
#define KM_SEG 256                  // prefix-sum segment

// members per run of the cluster sums: a function of n alone (at most ~4096 + k runs)
__host__ __device__ inline int km_run_len(int n)
{
    const int l = (n + 4095) / 4096;
    return l > 256 ? l : 256;
}

__device__ __forceinline__ int km_clamp(int v, int hi) { return v < 0 ? 0 : (v >= hi ? hi - 1 : v); }

// |x - c|^2 in double, features in order (one thread)
__device__ __forceinline__ double km_dist_seq(const float *__restrict__ x, const double *__restrict__ c, int d)
{
    double s = 0.0;
    for (int t = 0; t < d; t++) {
        const double df = (double)x[t] - c[t];
        s += df * df;
    }
    return s;
}

// |x - c|^2 in double over one wave: lane-strided partials, then the xor butterfly (every lane holds the same bits)
__device__ __forceinline__ double km_dist_wave(const float *__restrict__ x, const double *__restrict__ c, int d, int lane)
{
    double s = 0.0;
    for (int t = lane; t < d; t += 64) {
        const double df = (double)x[t] - c[t];
        s += df * df;
    }
    return tsne_wave_sum(s);
}

// one block per centre row: cf [k][d] = (float)c, cnrm [k] = |cf|^2 (double sum, rounded once)
__global__ __launch_bounds__(256) void km_prep_kernel(const double *__restrict__ c, int d, float *__restrict__ cf, float *__restrict__ cnrm)
{
    __shared__ double red[256];
    const int j = blockIdx.x;
    double s = 0.0;
    for (int t = threadIdx.x; t < d; t += 256) {
        const float v = (float)c[(size_t)j * d + t];
        cf[(size_t)j * d + t] = v;
        s += (double)v * (double)v;
    }
    s = tsne_block_sum<256>(s, red);
    if (threadIdx.x == 0) cnrm[j] = (float)s;
}

// label = first argmin over the k centres in double; dist = that distance; changed counts labels that differ from the stored ones
__global__ __launch_bounds__(256) void km_assign_small_kernel(const float *__restrict__ x, int n, int d, const double *__restrict__ c, int k,
                                                              int *__restrict__ labels, double *__restrict__ dist, int *__restrict__ changed)
{
    __shared__ double cs[KM_MAX_K * KM_SMALL_D];
    for (int e = threadIdx.x; e < k * d; e += 256) cs[e] = c[e];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (i < n) {
        double xv[KM_SMALL_D];
#pragma unroll
        for (int t = 0; t < KM_SMALL_D; t++) xv[t] = t < d ? (double)x[(size_t)i * d + t] : 0.0;
        double best = __builtin_inf();
        int bi = 0;
        for (int j = 0; j < k; j++) {
            double s = 0.0;
#pragma unroll
            for (int t = 0; t < KM_SMALL_D; t++) {
                if (t < d) {
                    const double df = xv[t] - cs[j * d + t];
                    s += df * df;
                }
            }
            if (s < best) { best = s; bi = j; }
        }
        moved = labels[i] != bi;
        labels[i] = bi;
        dist[i] = best;
    }
    const unsigned long long b = __ballot(moved);
    if (changed && (threadIdx.x & 63) == 0 && b) atomicAdd(changed, (int)__popcll(b));
}

struct KmAssignArgs {
    const float *x, *nrm;           // [n][d], |x|^2 [n]
    const double *c;                // centres [k][d] (double)
    const float *cf, *cnrm;         // their f32 copy and its squared norms
    int n, d, k;
    int *labels;                    // [n] in: previous labels, out: new labels
    double *dist;                   // [n] |x - c_label|^2 (double)
    int *changed;                   // labels that differ from the previous ones (may be null)
};

// 8 waves x 16 rows; NT tiles of 16 centres per wave (NT * 16 >= k)
template <int NT>
__global__ __launch_bounds__(64 * KM_WAVES) void km_assign_mfma_kernel(KmAssignArgs a)
{
    __shared__ __align__(16) float cs[NT * 16 * KM_KS];
    __shared__ int ccnt[KM_ROWS];
    __shared__ int clist[KM_ROWS * KM_CAP];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int row0 = blockIdx.x * KM_ROWS + wave * 16;
    const int ar = row0 + lr;
    const float *xa = ar < a.n ? a.x + (size_t)ar * a.d : nullptr;
    if (tid < KM_ROWS) ccnt[tid] = 0;
    f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < a.d; d0 += KM_KC) {
        __syncthreads();
        for (int e = tid; e < NT * 16 * KM_KC; e += 64 * KM_WAVES) {
            const int cc = e / KM_KC, t = e - cc * KM_KC;
            cs[cc * KM_KS + t] = (cc < a.k && d0 + t < a.d) ? a.cf[(size_t)cc * a.d + d0 + t] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < KM_KC / 4; s++) {
            const int kk = d0 + 4 * s + lk;
            const float av = (xa && kk < a.d) ? xa[kk] : 0.f;
#pragma unroll
            for (int t = 0; t < NT; t++)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, cs[(t * 16 + lr) * KM_KS + 4 * s + lk], acc[t], 0, 0, 0);
        }
    }

    // screen: acc[t][r] = x_i . c_j for row i = row0 + 4 lk + r, centre j = 16 t + lr. Error of the f32 distance against the double
    // |x - c|^2 (c the double centre): the fmaf chain of the dot product <= d u |x||cf|, the rounded norms and the two operations of
    // the expression <= 3 u (|x| + |cf|)^2, cf against c <= 2 u (|x| + |c|)^2: below (d + 5) u (|x| + |cf|)^2 (1 + O(u)). The bound
    // used is twice that, plus an absolute 1e-30 for underflow; a non-finite screen value makes the centre a candidate.
    const float eb = (float)(2 * (a.d + 16)) * 5.9604645e-8f;
    float nq[4], sq[4], thr[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const int i = row0 + 4 * lk + r;
        nq[r] = i < a.n ? a.nrm[i] : 0.f;
        sq[r] = sqrtf(nq[r]);
        thr[r] = __builtin_inff();
    }
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int j = t * 16 + lr;
        const bool valid = j < a.k;
        const float nc = valid ? a.cnrm[j] : 0.f, sc = sqrtf(nc);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float dt = nq[r] + nc - 2.f * acc[t][r];
            const float s = sq[r] + sc, e = eb * s * s + 1e-30f;
            const float hi = dt + e;
            if (valid && __builtin_isfinite(hi)) thr[r] = fminf(thr[r], hi);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) thr[r] = fminf(thr[r], __shfl_xor(thr[r], m, 64));
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const int j = t * 16 + lr;
        if (j >= a.k) continue;
        const float nc = a.cnrm[j], sc = sqrtf(nc);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const float dt = nq[r] + nc - 2.f * acc[t][r];
            const float s = sq[r] + sc, e = eb * s * s + 1e-30f;
            const float lo = dt - e;
            if (!(lo <= thr[r]) && __builtin_isfinite(lo)) continue;
            const int rl = wave * 16 + 4 * lk + r;
            const int p = atomicAdd(&ccnt[rl], 1);
            if (p < KM_CAP) clist[rl * KM_CAP + p] = j;
        }
    }
    __syncthreads();

    // the candidates of each of the wave's rows in double (the whole wave per distance)
    int moved = 0;
    for (int rr = 0; rr < 16; rr++) {
        const int i = row0 + rr;
        if (i >= a.n) break;
        const int rl = wave * 16 + rr, cnt = ccnt[rl];
        const float *xi = a.x + (size_t)i * a.d;
        double best = __builtin_inf();
        int bi = 0x7fffffff;
        const int m = cnt <= KM_CAP ? cnt : a.k;
        for (int q = 0; q < m; q++) {
            const int j = cnt <= KM_CAP ? km_clamp(clist[rl * KM_CAP + q], a.k) : q;
            const double dv = km_dist_wave(xi, a.c + (size_t)j * a.d, a.d, lane);
            if (dv < best || (dv == best && j < bi)) { best = dv; bi = j; }
        }
        if (bi == 0x7fffffff) bi = 0;
        if (lane == 0) {
            moved += a.labels[i] != bi ? 1 : 0;
            a.labels[i] = bi;
            a.dist[i] = best;
        }
    }
    if (a.changed && lane == 0 && moved) atomicAdd(a.changed, moved);
}

// dist[i] = |x_i - c_label|^2 for the stored labels: one thread per point (d <= KM_SMALL_D) or one wave per point
__global__ __launch_bounds__(256) void km_point_dist_kernel(const float *__restrict__ x, int n, int d, const double *__restrict__ c, int k,
                                                            const int *__restrict__ labels, double *__restrict__ dist)
{
    if (d <= KM_SMALL_D) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        if (i < n) dist[i] = km_dist_seq(x + (size_t)i * d, c + (size_t)km_clamp(labels[i], k) * d, d);
        return;
    }
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const double v = km_dist_wave(x + (size_t)i * d, c + (size_t)km_clamp(labels[i], k) * d, d, lane);
    if (lane == 0) dist[i] = v;
}

// bcnt [nb][k]: label counts of each block of KM_BLOCK points
__global__ __launch_bounds__(KM_BLOCK) void km_hist_kernel(const int *__restrict__ labels, int n, int k, int *__restrict__ bcnt)
{
    __shared__ int h[KM_MAX_K];
    for (int e = threadIdx.x; e < k; e += KM_BLOCK) h[e] = 0;
    __syncthreads();
    const int i = blockIdx.x * KM_BLOCK + threadIdx.x;
    if (i < n) atomicAdd(&h[km_clamp(labels[i], k)], 1);
    __syncthreads();
    for (int e = threadIdx.x; e < k; e += KM_BLOCK) bcnt[(size_t)blockIdx.x * k + e] = h[e];
}

// one block per cluster c: bcnt[b][c] becomes the first position of block b's members of c among the cluster's members (an
// exclusive scan over the blocks: integers, exact in any order); count[c] = the cluster's size
__global__ __launch_bounds__(256) void km_offsets_kernel(int *__restrict__ bcnt, int nb, int k, int *__restrict__ count)
{
    __shared__ int sc[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int per = (nb + 255) / 256, b0 = min(nb, tid * per), b1 = min(nb, b0 + per);
    int s = 0;
    for (int b = b0; b < b1; b++) s += bcnt[(size_t)b * k + c];
    sc[tid] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const int v = tid >= off ? sc[tid - off] : 0;
        __syncthreads();
        sc[tid] += v;
        __syncthreads();
    }
    int run = tid ? sc[tid - 1] : 0;
    for (int b = b0; b < b1; b++) {
        const int v = bcnt[(size_t)b * k + c];
        bcnt[(size_t)b * k + c] = run;
        run += v;
    }
    if (tid == 255) count[c] = sc[255];
}

// one thread: start [k] of each cluster in the member array, run0 [k + 1]: first run of each cluster (run0[k] = runs in all)
__global__ __launch_bounds__(64) void km_starts_kernel(const int *__restrict__ count, int k, int L, int *__restrict__ start,
                                                       int *__restrict__ run0)
{
    if (threadIdx.x != 0) return;
    int s = 0, r = 0;
    for (int j = 0; j < k; j++) {
        start[j] = s;
        run0[j] = r;
        s += count[j];
        r += (count[j] + L - 1) / L;
    }
    run0[k] = r;
}

// members[pos] = i with pos the rank of i among the points of its cluster, in index order
__global__ __launch_bounds__(KM_BLOCK) void km_scatter_kernel(const int *__restrict__ labels, int n, int k, const int *__restrict__ boff,
                                                              const int *__restrict__ start, int *__restrict__ members)
{
    constexpr int NW = KM_BLOCK / 64;
    __shared__ int wc[NW * KM_MAX_K];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int e = tid; e < NW * KM_MAX_K; e += KM_BLOCK) wc[e] = 0;
    __syncthreads();
    const int i = blockIdx.x * KM_BLOCK + tid;
    const int lab = i < n ? km_clamp(labels[i], k) : -1;
    unsigned long long active = __ballot(i < n);
    int rank = 0;
    while (active) {
        const int leader = __builtin_ctzll(active);
        const int l = __shfl(lab, leader, 64);
        const unsigned long long m = __ballot(lab == l);
        if (lab == l) rank = (int)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == leader) wc[wave * KM_MAX_K + l] = (int)__popcll(m);
        active &= ~m;
    }
    __syncthreads();
    if (i < n) {
        int pos = start[lab] + boff[(size_t)blockIdx.x * k + lab] + rank;
        for (int w = 0; w < wave; w++) pos += wc[w * KM_MAX_K + lab];
        members[pos] = i;
    }
}

// one block per run: part[r][d] = sum over the run's members (index order) of x, in double
__global__ __launch_bounds__(256) void km_runsum_kernel(const float *__restrict__ x, int n, int d, int k, int L, const int *__restrict__ members,
                                                        const int *__restrict__ count, const int *__restrict__ start,
                                                        const int *__restrict__ run0, double *__restrict__ part)
{
    const int r = blockIdx.x;
    if (r >= run0[k]) return;
    int lo = 0, hi = k - 1;              // the last cluster whose first run is <= r
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (run0[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int c = lo, j = r - run0[c];
    const int m0 = start[c] + j * L, m1 = min(start[c] + count[c], m0 + L);
    constexpr int U = KM_MAX_D / 256;
    double acc[U];
#pragma unroll
    for (int u = 0; u < U; u++) acc[u] = 0.0;
    int q = m0;
    for (; q + 4 <= m1; q += 4) {            // four rows in flight, added in member order
        const float *xr0 = x + (size_t)km_clamp(members[q], n) * d, *xr1 = x + (size_t)km_clamp(members[q + 1], n) * d;
        const float *xr2 = x + (size_t)km_clamp(members[q + 2], n) * d, *xr3 = x + (size_t)km_clamp(members[q + 3], n) * d;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = threadIdx.x + 256 * u;
            if (t < d) {
                const float v0 = xr0[t], v1 = xr1[t], v2 = xr2[t], v3 = xr3[t];
                acc[u] += (double)v0;
                acc[u] += (double)v1;
                acc[u] += (double)v2;
                acc[u] += (double)v3;
            }
        }
    }
    for (; q < m1; q++) {
        const float *xr = x + (size_t)km_clamp(members[q], n) * d;
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int t = threadIdx.x + 256 * u;
            if (t < d) acc[u] += (double)xr[t];
        }
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int t = threadIdx.x + 256 * u;
        if (t < d) part[(size_t)r * d + t] = acc[u];
    }
}

// one block per cluster: sums[c] = its runs added in run order, wt[c] = its member count
__global__ __launch_bounds__(256) void km_combine_kernel(const double *__restrict__ part, int d, const int *__restrict__ count,
                                                         const int *__restrict__ run0, double *__restrict__ sums, double *__restrict__ wt)
{
    const int c = blockIdx.x, r0 = run0[c], r1 = run0[c + 1];
    for (int t = threadIdx.x; t < d; t += 256) {
        double s = 0.0;
        for (int r = r0; r < r1; r++) s += part[(size_t)r * d + t];
        sums[(size_t)c * d + t] = s;
    }
    if (threadIdx.x == 0) wt[c] = (double)count[c];
}

__device__ __forceinline__ bool km_far_before(double da, int ia, double db, int ib) { return da > db || (da == db && ia < ib); }

// one block: sklearn's _relocate_empty_clusters_dense with the farthest points in decreasing distance, ties by lower index.
// nempty [1] receives the number of empty clusters.
__global__ __launch_bounds__(1024) void km_relocate_kernel(const float *__restrict__ x, int n, int d, int k, const int *__restrict__ labels,
                                                           const double *__restrict__ dist, const int *__restrict__ count,
                                                           double *__restrict__ sums, double *__restrict__ wt, int *__restrict__ nempty)
{
    __shared__ int empty[KM_MAX_K], far[KM_MAX_K];
    __shared__ int ne, stop;
    __shared__ double rd[1024];
    __shared__ int ri[1024];
    const int tid = threadIdx.x;
    if (tid == 0) {
        int e = 0;
        for (int c = 0; c < k; c++)
            if (count[c] == 0) empty[e++] = c;
        ne = e;
        stop = 0;
        if (nempty) nempty[0] = e;
    }
    __syncthreads();
    const int m = ne;
    if (m == 0) return;
    double pd = __builtin_inf();
    int pi = -1;
    for (int q = 0; q < m; q++) {
        double bd = -__builtin_inf();
        int bi = 0x7fffffff;
        for (int i = tid; i < n; i += 1024) {
            const double v = dist[i];
            if (km_far_before(pd, pi, v, i) && km_far_before(v, i, bd, bi)) { bd = v; bi = i; }
        }
        rd[tid] = bd;
        ri[tid] = bi;
        __syncthreads();
        for (int s = 512; s > 0; s >>= 1) {
            if (tid < s && km_far_before(rd[tid + s], ri[tid + s], rd[tid], ri[tid])) { rd[tid] = rd[tid + s]; ri[tid] = ri[tid + s]; }
            __syncthreads();
        }
        pd = rd[0];
        pi = ri[0];
        if (tid == 0) {
            far[q] = km_clamp(pi, n);
            if (q == 0 && pd == 0.0) stop = 1;      // every point sits on its centre: sklearn relocates nothing
        }
        __syncthreads();
        if (stop) return;
    }
    for (int q = 0; q < m; q++) {
        const int nw = empty[q], f = far[q], old = km_clamp(labels[f], k);
        for (int t = tid; t < d; t += 1024) {
            const double xv = (double)x[(size_t)f * d + t];
            sums[(size_t)old * d + t] -= xv;
            sums[(size_t)nw * d + t] = xv;
        }
        if (tid == 0) {
            wt[nw] = 1.0;
            wt[old] -= 1.0;
        }
        __syncthreads();
    }
}

// one block per cluster: sklearn's _average_centers, then |c_new - c_old|^2 per cluster.  weight > 0: c_new = sum * (1 / weight);
// weight 0: the centre of the heaviest cluster a (first maximum), which sklearn's in-order loop has already averaged when a < c
// and not yet (the plain sum) when a > c.
__global__ __launch_bounds__(256) void km_update_kernel(const double *__restrict__ sums, const double *__restrict__ wt, const double *__restrict__ cold,
                                                        int d, int k, double *__restrict__ cnew, double *__restrict__ shift)
{
    __shared__ double red[256];
    __shared__ int heavy;
    const int c = blockIdx.x;
    if (threadIdx.x == 0) {
        int a = 0;
        for (int j = 1; j < k; j++)
            if (wt[j] > wt[a]) a = j;
        heavy = a;
    }
    __syncthreads();
    const double w = wt[c];
    const int src = w > 0.0 ? c : heavy;
    const bool scale = w > 0.0 || heavy < c;
    const double alpha = 1.0 / wt[src];
    double s = 0.0;
    for (int t = threadIdx.x; t < d; t += 256) {
        double v = sums[(size_t)src * d + t];
        if (scale) v *= alpha;
        cnew[(size_t)c * d + t] = v;
        const double df = v - cold[(size_t)c * d + t];
        s += df * df;
    }
    s = tsne_block_sum<256>(s, red);
    if (threadIdx.x == 0) shift[c] = s;
}

// stats [3]: centre shift total, changed labels, empty clusters relocated
__global__ __launch_bounds__(256) void km_stats_kernel(const double *__restrict__ shift, int k, const int *__restrict__ ints, double *__restrict__ stats)
{
    __shared__ double red[256];
    double s = threadIdx.x < k ? shift[threadIdx.x] : 0.0;
    s = tsne_block_sum<256>(s, red);
    if (threadIdx.x == 0) {
        stats[0] = s;
        stats[1] = (double)ints[0];
        stats[2] = (double)ints[1];
    }
}

// part[b] = sum of v over block b of 256 values (tree)
__global__ __launch_bounds__(256) void km_block_sum_kernel(const double *__restrict__ v, int n, double *__restrict__ part)
{
    __shared__ double red[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double s = tsne_block_sum<256>(i < n ? v[i] : 0.0, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// out[0] = sum of part[0 .. nb) (each thread its contiguous share in order, then the tree)
__global__ __launch_bounds__(256) void km_final_sum_kernel(const double *__restrict__ part, int nb, double *__restrict__ out)
{
    __shared__ double red[256];
    const int per = (nb + 255) / 256, b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    double s = 0.0;
    for (int b = b0; b < b1; b++) s += part[b];
    s = tsne_block_sum<256>(s, red);
    if (threadIdx.x == 0) out[0] = s;
}

// ---- k-means++ seeding

// segsum[s] = w[s * KM_SEG] + ... in order (one thread per segment)
__global__ __launch_bounds__(256) void km_segsum_kernel(const double *__restrict__ w, int n, double *__restrict__ segsum)
{
    const int s = blockIdx.x * 256 + threadIdx.x, e0 = s * KM_SEG;
    if (e0 >= n) return;
    const int e1 = min(n, e0 + KM_SEG);
    double v = 0.0;
    for (int e = e0; e < e1; e++) v += w[e];
    segsum[s] = v;
}

// one block: base[s] = the cumulative sum before segment s, end[s] = base[s] + segsum[s] (chunks of segments per thread in
// order, the 256 chunk totals in order by one thread)
__global__ __launch_bounds__(256) void km_segscan_kernel(const double *__restrict__ segsum, int nseg, double *__restrict__ base, double *__restrict__ end)
{
    __shared__ double ct[256];
    const int per = (nseg + 255) / 256, s0 = threadIdx.x * per, s1 = min(nseg, s0 + per);
    double v = 0.0;
    for (int s = s0; s < s1; s++) v += segsum[s];
    ct[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        double run = 0.0;
        for (int t = 0; t < 256; t++) {
            const double c = ct[t];
            ct[t] = run;
            run += c;
        }
    }
    __syncthreads();
    double run = ct[threadIdx.x];
    for (int s = s0; s < s1; s++) {
        base[s] = run;
        run += segsum[s];
        end[s] = run;
    }
}

// one block per value: idx[j] = the first e with cum(e) >= vals[j] (np.searchsorted side left), clipped to n - 1, where
// cum(e) = base[s] + (w[s KM_SEG] + ... + w[e]) (the in-segment prefix in order)
__global__ __launch_bounds__(256) void km_search_kernel(const double *__restrict__ w, int n, const double *__restrict__ base, const double *__restrict__ end,
                                                        int nseg, const double *__restrict__ vals, int *__restrict__ idx)
{
    __shared__ int red[256];
    const double v = vals[blockIdx.x];
    int first = 0x7fffffff;
    for (int s = threadIdx.x; s < nseg; s += 256)
        if (end[s] >= v) { first = s; break; }
    red[threadIdx.x] = first;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = min(red[threadIdx.x], red[threadIdx.x + s]);
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    int r = n;
    const int s = red[0];
    if (s < nseg) {
        const double b = base[s];
        const int e0 = s * KM_SEG, e1 = min(n, e0 + KM_SEG);
        double p = 0.0;
        r = e1 - 1;
        for (int e = e0; e < e1; e++) {
            p += w[e];
            if (b + p >= v) { r = e; break; }
        }
    }
    idx[blockIdx.x] = min(r, n - 1);
}

// grid (blocks, m): part[j][b] = sum over block b of min(closest_i, |x_i - x_cand_j|^2) (closest null: the distance alone)
__global__ __launch_bounds__(256) void km_cand_dist_kernel(const float *__restrict__ x, int n, int d, const int *__restrict__ cand,
                                                           const double *__restrict__ closest, double *__restrict__ part)
{
    __shared__ double cs[KM_MAX_D];
    __shared__ double red[256];
    const int j = blockIdx.y, nb = gridDim.x, ci = km_clamp(cand[j], n);
    for (int t = threadIdx.x; t < d; t += 256) cs[t] = (double)x[(size_t)ci * d + t];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    double v = 0.0;
    if (i < n) {
        v = km_dist_seq(x + (size_t)i * d, cs, d);
        if (closest) v = fmin(closest[i], v);
    }
    v = tsne_block_sum<256>(v, red);
    if (threadIdx.x == 0) part[(size_t)j * nb + blockIdx.x] = v;
}

// one block: pot[j] = sum of part[j][*] (fixed order); out[0] = the chosen point (the first candidate of least potential),
// out[1] = its potential, out[2 + j] = pot[j]
__global__ __launch_bounds__(256) void km_pick_kernel(const double *__restrict__ part, int nb, const int *__restrict__ cand, int m, int n,
                                                      double *__restrict__ out)
{
    __shared__ double red[256];
    __shared__ double pot[KM_MAX_M];
    const int per = (nb + 255) / 256, b0 = threadIdx.x * per, b1 = min(nb, b0 + per);
    for (int j = 0; j < m; j++) {
        double s = 0.0;
        for (int b = b0; b < b1; b++) s += part[(size_t)j * nb + b];
        s = tsne_block_sum<256>(s, red);
        if (threadIdx.x == 0) pot[j] = s;
    }
    if (threadIdx.x != 0) return;
    int best = 0;
    for (int j = 1; j < m; j++)
        if (pot[j] < pot[best]) best = j;
    out[0] = (double)km_clamp(cand[best], n);
    out[1] = pot[best];
    for (int j = 0; j < m; j++) out[2 + j] = pot[j];
}

// closest_i = min(closest_i, |x_i - x_chosen|^2) (first: the distance alone), chosen = out[0] of km_pick_kernel
__global__ __launch_bounds__(256) void km_commit_kernel(const float *__restrict__ x, int n, int d, const double *__restrict__ pick, int first,
                                                        double *__restrict__ closest)
{
    __shared__ double cs[KM_MAX_D];
    const int ci = km_clamp((int)pick[0], n);
    for (int t = threadIdx.x; t < d; t += 256) cs[t] = (double)x[(size_t)ci * d + t];
    __syncthreads();
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double v = km_dist_seq(x + (size_t)i * d, cs, d);
    closest[i] = first ? v : fmin(closest[i], v);
}

}  // namespace ralign
