// Spectral embedding (Laplacian eigenmaps / diffusion maps) of a symmetric kNN graph (the contract at the top of
// cryo_ralib_amd/spectral.py): the sparse operator, the Lanczos step with full reorthogonalisation against
// a growing basis of tall vectors, the Ritz combination and one round of connected components.  Everything is double.
//
// The operator is a CSR (indptr [n + 1], indices, val) with the columns of a row ascending.  The basis is V [m + 1][ldv]: vector j
// is the ldv-strided row j (ldv >= n), and q0 [n] is the known top eigenvector.  Q = [q0, v_0 .. v_j] has j + 2 columns; column 0 is
// q0 and column t >= 1 is v_{t - 1} (spec_col).
//
//   spec_spmv_kernel      y = A x.  SPEC_LANES lanes share a row, SPEC_ROWS rows a workgroup.  Lane l adds the row's entries
//                         l, l + 16, l + 32, ... in that order by fma (SPEC_UNROLL of them are loaded per trip; the order does
//                         not depend on the unroll), then the 16 lanes combine in the xor tree 8, 4, 2, 1: the order of a row's
//                         sum depends on its length only.  An empty row gives 0.  An entry whose column is outside 0 .. n - 1 is
//                         skipped; a row whose indptr pair is not 0 <= p0 <= p1 counts as empty.
//   spec_check_kernel     flags a CSR that spec_spmv_kernel would have to patch (ra_spectral_spmv refuses it).
//   spec_dots_kernel      part[run][t] = sum over the run's SPEC_RUN rows of Q_t[i] w[i].  A wave owns SPEC_CW columns of the
//                         workgroup's SPEC_CT; lane l adds the rows i0 + l, i0 + l + 64, ... of the run in that order by fma, then
//                         the 64 lanes combine in the xor tree 32 .. 1.
//   spec_reduce_kernel    h[t] = part[0][t] + part[1][t] + ... in run order, one thread per column; alpha_j = h[j + 1] of the
//                         first pass (v_j . w before anything was subtracted).
//   spec_update_kernel    w_i <- w_i - (h_0 Q_0[i] + h_1 Q_1[i] + ...), the sum formed by fma in t order, one thread per row.
//                         With `norm` the wave also leaves the sum of its 64 new w_i^2 (xor tree) in npart[wave].
//   spec_norm_kernel      beta_j = sqrt(npart[0] + npart[1] + ...): one workgroup, each thread its contiguous share in order,
//                         then the 256 shares in order (gmm_final_kernel's scheme).
//   spec_scale_kernel     v_{j + 1} = w / beta_j with beta_j read from device memory; beta_j <= SPEC_BREAKDOWN writes zeros, so
//                         every later step of the same enqueue stays finite (alpha = beta = 0) and the host truncates at j.
//   spec_ritz_kernel      Y_t[i] = S[0][t] V_0[i] + S[1][t] V_1[i] + ... by fma in j order; a thread owns SPEC_RT columns of one
//                         row: one writer per element.
//   spec_min_kernel / spec_hook_kernel / spec_compress_kernel
//                         one round of minimum-label hooking with pointer compression, DBSCAN's scheme on a CSR: m_i = the least
//                         label over row i and its neighbours; P starts as a copy of label and every i with m_i < label_i does
//                         P[label_i] = min(.., m_i), P[i] = min(.., m_i) by integer atomicMin; then (a launch of its own) i walks
//                         P down to the fixed point.  label_i <= i always, so the walk strictly decreases and ends.
//
// Determinism: no floating-point atomics; every sum has an order fixed by n, the row length or the number of columns alone.  No
// workgroup waits for another: ordering comes from separate launches on one stream.  Every column index read from memory is
// range-checked before it addresses anything.
#pragma once

#include <hip/hip_runtime.h>

namespace ralign {

#define SPEC_MAX_N 262144
#define SPEC_MAX_M 4096             // basis vectors of one solve
#define SPEC_MAX_C 64               // Ritz vectors of one call
#define SPEC_LANES 16               // lanes per CSR row
#define SPEC_ROWS 16                // CSR rows per workgroup
#define SPEC_UNROLL 4               // entries per lane and trip: 64 entries of a row are in flight
#define SPEC_RUN 512                // rows per run of the dots
#define SPEC_CT 16                  // columns per workgroup of the dots
#define SPEC_CW 4                   // columns per wave of the dots
#define SPEC_UPD 64                 // rows per workgroup of the update (one wave: one partial of the norm)
#define SPEC_RT 4                   // Ritz columns per thread
#define SPEC_BREAKDOWN 9.094947017729282e-13    // 2^-40

static_assert(SPEC_LANES * SPEC_ROWS == 256 && SPEC_CT == 4 * SPEC_CW && SPEC_RUN % 64 == 0, "tile plan");

__device__ __forceinline__ const double *spec_col(const double *__restrict__ q0, const double *__restrict__ V, int ldv, int t)
{
    return t == 0 ? q0 : V + (size_t)(t - 1) * ldv;
}

// the sum of v over the 64 lanes, the same bits in every lane
__device__ __forceinline__ double spec_wave_sum(double v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

__global__ __launch_bounds__(256) void spec_spmv_kernel(const int *__restrict__ indptr, const int *__restrict__ indices,
                                                        const double *__restrict__ val, int n, const double *__restrict__ x,
                                                        double *__restrict__ y)
{
    const int lane = threadIdx.x & (SPEC_LANES - 1), i = blockIdx.x * SPEC_ROWS + (threadIdx.x >> 4);
    double s = 0.0;
    if (i < n) {
        const int p0 = indptr[i], p1 = indptr[i + 1];
        if (p0 >= 0)
            for (int p = p0 + lane; p < p1; p += SPEC_LANES * SPEC_UNROLL) {
                int c[SPEC_UNROLL];
                double v[SPEC_UNROLL];
#pragma unroll
                for (int u = 0; u < SPEC_UNROLL; u++) {
                    const int q = p + u * SPEC_LANES;
                    c[u] = q < p1 ? indices[q] : -1;
                    v[u] = q < p1 ? val[q] : 0.0;
                }
#pragma unroll
                for (int u = 0; u < SPEC_UNROLL; u++)
                    if (c[u] >= 0 && c[u] < n) s = fma(v[u], x[c[u]], s);
            }
    }
#pragma unroll
    for (int m = SPEC_LANES / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    if (i < n && lane == 0) y[i] = s;
}

// bad[0] = 1 unless indptr[0] == 0, every row has 0 <= p0 <= p1 with at most n entries and every column is in 0 .. n - 1
// (umap_check_kernel asks for another condition, an indptr that ascends to nnz: the two stay apart)
__global__ __launch_bounds__(256) void spec_check_kernel(const int *__restrict__ indptr, const int *__restrict__ indices, int n,
                                                         int *__restrict__ bad)
{
    const int lane = threadIdx.x & (SPEC_LANES - 1), i = blockIdx.x * SPEC_ROWS + (threadIdx.x >> 4);
    if (i >= n) return;
    const int p0 = indptr[i], p1 = indptr[i + 1];
    bool wrong = p0 < 0 || p1 < p0 || p1 - p0 > n || (i == 0 && p0 != 0);
    if (!wrong)
        for (int p = p0 + lane; p < p1; p += SPEC_LANES) {
            const int c = indices[p];
            wrong |= c < 0 || c >= n;
        }
    if (wrong) atomicMax(bad, 1);
}

// grid (runs, column tiles); part [runs][cols]
__global__ __launch_bounds__(256) void spec_dots_kernel(const double *__restrict__ q0, const double *__restrict__ V, int ldv, int cols,
                                                        const double *__restrict__ w, int n, double *__restrict__ part)
{
    const int lane = threadIdx.x & 63, t0 = blockIdx.y * SPEC_CT + (threadIdx.x >> 6) * SPEC_CW;
    if (t0 >= cols) return;                                 // the whole wave
    const int i0 = blockIdx.x * SPEC_RUN, i1 = min(n, i0 + SPEC_RUN);
    const double *col[SPEC_CW];
    double acc[SPEC_CW];
#pragma unroll
    for (int c = 0; c < SPEC_CW; c++) {
        col[c] = spec_col(q0, V, ldv, min(t0 + c, cols - 1));
        acc[c] = 0.0;
    }
    for (int i = i0 + lane; i < i1; i += 64) {
        const double wi = w[i];
#pragma unroll
        for (int c = 0; c < SPEC_CW; c++) acc[c] = fma(col[c][i], wi, acc[c]);
    }
#pragma unroll
    for (int c = 0; c < SPEC_CW; c++) {
        const double s = spec_wave_sum(acc[c]);
        if (lane == 0 && t0 + c < cols) part[(size_t)blockIdx.x * cols + t0 + c] = s;
    }
}

__global__ __launch_bounds__(256) void spec_reduce_kernel(const double *__restrict__ part, int runs, int cols, double *__restrict__ h,
                                                          double *__restrict__ alpha_out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= cols) return;
    double s = 0.0;
    for (int r = 0; r < runs; r++) s += part[(size_t)r * cols + t];
    h[t] = s;
    if (alpha_out && t == cols - 1) alpha_out[0] = s;
}

__global__ __launch_bounds__(SPEC_UPD) void spec_update_kernel(const double *__restrict__ q0, const double *__restrict__ V, int ldv,
                                                               int cols, const double *__restrict__ h, double *__restrict__ w, int n,
                                                               double *__restrict__ npart)
{
    const int i = blockIdx.x * SPEC_UPD + threadIdx.x;
    double out = 0.0;
    if (i < n) {
        double s = 0.0;
#pragma unroll 8
        for (int t = 0; t < cols; t++) s = fma(h[t], spec_col(q0, V, ldv, t)[i], s);
        out = w[i] - s;
        w[i] = out;
    }
    if (npart) {
        const double s2 = spec_wave_sum(out * out);
        if (threadIdx.x == 0) npart[blockIdx.x] = s2;
    }
}

__global__ __launch_bounds__(256) void spec_norm_kernel(const double *__restrict__ npart, int nr, double *__restrict__ beta_out)
{
    __shared__ double sh[256];
    const int per = (nr + 255) / 256, b0 = min(nr, (int)threadIdx.x * per), b1 = min(nr, b0 + per);
    double s = 0.0;
    for (int b = b0; b < b1; b++) s += npart[b];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int q = 0; q < 256; q++) t += sh[q];
    beta_out[0] = sqrt(t);
}

__global__ __launch_bounds__(256) void spec_scale_kernel(const double *__restrict__ w, int n, const double *__restrict__ beta,
                                                         double *__restrict__ v)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double b = beta[0];
    v[i] = b > SPEC_BREAKDOWN ? w[i] / b : 0.0;
}

// grid (ceil(n / 256), ceil(c / SPEC_RT)); S [m][c], Y [c][n]
__global__ __launch_bounds__(256) void spec_ritz_kernel(const double *__restrict__ V, int ldv, int m, int n, const double *__restrict__ S,
                                                        int c, double *__restrict__ Y)
{
    const int i = blockIdx.x * 256 + threadIdx.x, t0 = blockIdx.y * SPEC_RT;
    if (i >= n) return;
    double acc[SPEC_RT];
#pragma unroll
    for (int u = 0; u < SPEC_RT; u++) acc[u] = 0.0;
    for (int j = 0; j < m; j++) {
        const double v = V[(size_t)j * ldv + i];
#pragma unroll
        for (int u = 0; u < SPEC_RT; u++) acc[u] = fma(S[(size_t)j * c + min(t0 + u, c - 1)], v, acc[u]);
    }
#pragma unroll
    for (int u = 0; u < SPEC_RT; u++)
        if (t0 + u < c) Y[(size_t)(t0 + u) * n + i] = acc[u];
}

// ---- connected components

__device__ __forceinline__ bool spec_label_ok(int l, int i) { return l >= 0 && l <= i; }

__global__ __launch_bounds__(256) void spec_min_kernel(const int *__restrict__ indptr, const int *__restrict__ indices, int n,
                                                       const int *__restrict__ label, int *__restrict__ mn)
{
    const int lane = threadIdx.x & (SPEC_LANES - 1), i = blockIdx.x * SPEC_ROWS + (threadIdx.x >> 4);
    int best = 0x7fffffff;
    if (i < n) {
        best = label[i];
        const int p0 = indptr[i], p1 = indptr[i + 1];
        if (p0 >= 0)
            for (int p = p0 + lane; p < p1; p += SPEC_LANES) {
                const int c = indices[p];
                if (c >= 0 && c < n) best = min(best, label[c]);
            }
    }
#pragma unroll
    for (int m = SPEC_LANES / 2; m >= 1; m >>= 1) best = min(best, __shfl_xor(best, m, 64));
    if (i < n && lane == 0) mn[i] = best;
}

__global__ __launch_bounds__(256) void spec_hook_kernel(int n, const int *__restrict__ label, const int *__restrict__ mn, int *__restrict__ P)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int li = label[i], mi = mn[i];
    if (!spec_label_ok(li, i) || mi < 0 || mi >= li) return;
    atomicMin(&P[li], mi);
    atomicMin(&P[i], mi);
}

__global__ __launch_bounds__(256) void spec_compress_kernel(int n, const int *__restrict__ P, int *__restrict__ label, int *__restrict__ changed)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool moved = false;
    if (i < n) {
        int r = i;
        for (;;) {                          // P[r] <= r: strictly down to the fixed point
            const int p = P[r];
            if (p < 0 || p >= r) break;
            r = p;
        }
        moved = r != label[i];
        label[i] = r;
    }
    const unsigned long long b = __ballot(moved);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(changed, (int)__popcll(b));
}

}  // namespace ralign
