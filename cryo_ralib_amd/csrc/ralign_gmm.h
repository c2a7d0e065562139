// Gaussian mixture E- and M-step on X [n][d] (scikit-learn 1.7 GaussianMixture, covariance_type "full" and "diag"; DESIGN.md
// section 4.14).  X is float32 and converts exactly; every other number is float64 and x - mu is formed in double before anything
// is multiplied.
//
//   gmm_estep_full_kernel    16 rows of differences per MFMA tile against 16 columns of the upper triangular PC_c on
//                            v_mfma_f64_16x16x4_f64; tiles of PC_c below the diagonal are skipped; sum_j y_j^2, the max-subtracted
//                            running logsumexp, the first argmax and log_resp finish in the kernel.
//   gmm_estep_diag_kernel    log p_ic of 64 rows x 32 components per block on the vector ALU, features in order.
//   gmm_finish_kernel        diag: max, logsumexp, first argmax and log_resp of one row (components in order).
//   gmm_runsum_kernel / gmm_final_kernel
//                            sum_i log_prob_norm_i: runs of GMM_SUM_RUN values in index order, then the runs in run order.
//   gmm_nk_kernel / gmm_msum_kernel
//                            per run of rows (index order): sum_i r_ic, sum_i r_ic x_i and (diag) sum_i r_ic x_i^2.
//   gmm_mcombine_kernel      the runs added in run order: nk (+ 10 eps), means, diag covariances.
//   gmm_cov_kernel           full: sum_i (r_ic diff_i) diff_i^T per run on v_mfma_f64_16x16x4_f64, upper tiles only.
//   gmm_cov_combine_kernel   the runs added in run order, / nk, + reg_covar on the diagonal, mirrored to the lower triangle.
//
// f64 MFMA lane maps (16x16x4): A[row = lane & 15][k = lane >> 4], B[k = lane >> 4][col = lane & 15], and the C/D map that is NOT
// the f32 one: col = lane & 15, row = (lane >> 4) + 4 reg.
//
// Determinism: no floating-point atomics.  Every sum over i runs over a run of rows in index order, then over the runs in run
// order; run lengths depend on (n, d, k) alone (gmm_plan_*).
#pragma once

#include <hip/hip_runtime.h>

namespace ralign {

typedef double f64x4 __attribute__((ext_vector_type(4)));

#define GMM_MAX_N 4194304
#define GMM_MAX_K 256
#define GMM_MAX_D_FULL 256
#define GMM_MAX_D_DIAG 2048
#define GMM_MAX_NK (1 << 28)        // entries of the [n][k] double table
#define GMM_SUM_RUN 64              // values per run of the log-likelihood sum
#define GMM_DR 64                   // diag E-step: rows per block
#define GMM_DC 32                   // diag E-step: components per block (8 per thread)
#define GMM_DT 32                   // diag E-step: features per LDS chunk
#define GMM_MROWS 64                // M-step sums: rows per LDS chunk of responsibilities
#define GMM_CROWS 32                // covariance scatter: rows per LDS chunk
#define GMM_CTILES 8                // covariance scatter: 16 x 16 tiles per wave
#define GMM_CXS 272                 // covariance scatter: largest LDS row stride (16 * 17 floats)

// ---- the fixed run plans (functions of n, d, k alone)

struct GmmPlan { int runs, len; };

// about `want` blocks in all when every run spawns `per_run` blocks; runs of a multiple of `quantum` rows, at most 256 runs
__host__ __device__ inline GmmPlan gmm_plan(int n, int per_run, int quantum, int want)
{
    int runs = (want + per_run - 1) / per_run;
    runs = runs < 1 ? 1 : (runs > 256 ? 256 : runs);
    int len = (n + runs - 1) / runs;
    len = (len + quantum - 1) / quantum * quantum;
    GmmPlan p;
    p.len = len;
    p.runs = (n + len - 1) / len;
    return p;
}

__host__ __device__ inline int gmm_msum_td(int d) { return d <= 64 ? 64 : 256; }              // threads along the features
__host__ __device__ inline int gmm_msum_cb(int d) { return d <= 64 ? 64 : 16; }               // components per block
__host__ __device__ inline int gmm_cov_tiles(int d) { const int dt = (d + 15) >> 4; return dt * (dt + 1) / 2; }
__host__ __device__ inline int gmm_cov_stride(int d) { const int dt = (d + 15) >> 4; return 16 * (dt + 1 + (dt & 1)); }

// ---- E-step, full covariances

struct GmmEArgs {
    const float *x;                 // [n][d]
    const double *means, *pc, *offset;
    double *log_resp, *log_prob;    // [n][k] (may be null), [n]
    int *labels;                    // [n] (may be null)
    int n, d, k;
};

// 4 waves x RT tiles of 16 rows; dynamic LDS: the block's rows as float, row stride 16 DT + 4 (the 64 lanes of one operand read hit
// 64 banks)
template <int RT>
__global__ __launch_bounds__(256) void gmm_estep_full_kernel(GmmEArgs a)
{
    extern __shared__ __align__(16) unsigned char gmm_smem[];
    float *xs = (float *)gmm_smem;
    constexpr int RB = 64 * RT;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int DT = (a.d + 15) >> 4, DP = DT * 16, XS = DP + 4;
    const int row0 = blockIdx.x * RB;
    for (int e = tid; e < RB * DP; e += 256) {
        const int r = e / DP, t = e - r * DP, i = row0 + r;
        xs[r * XS + t] = (i < a.n && t < a.d) ? a.x[(size_t)i * a.d + t] : 0.f;
    }
    __syncthreads();
    const float *xw = xs + (size_t)(wave * 16 * RT + lr) * XS;      // row lr of the wave's tile 0; tile rt: + rt * 16 * XS
    const int mine = lr & 3;                                        // the lane keeps the running state of row lk + 4 * mine
    double M[RT], S[RT];
    int best[RT];
#pragma unroll
    for (int rt = 0; rt < RT; rt++) { M[rt] = -__builtin_inf(); S[rt] = 0.0; best[rt] = 0; }
    for (int c = 0; c < a.k; c++) {
        const double *mu = a.means + (size_t)c * a.d, *pc = a.pc + (size_t)c * a.d * a.d;
        double m[RT][4];
#pragma unroll
        for (int rt = 0; rt < RT; rt++)
#pragma unroll
            for (int r = 0; r < 4; r++) m[rt][r] = 0.0;
        for (int jt = 0; jt < DT; jt++) {
            f64x4 acc[RT];
#pragma unroll
            for (int rt = 0; rt < RT; rt++) acc[rt] = f64x4{0.0, 0.0, 0.0, 0.0};
            const int j = 16 * jt + lr;
            for (int tt = 0; tt <= jt; tt++) {          // PC_c is upper triangular: tiles with tt > jt are zero
#pragma unroll
                for (int s = 0; s < 4; s++) {
                    const int t = 16 * tt + 4 * s + lk;
                    const bool tv = t < a.d;
                    const double muv = tv ? mu[t] : 0.0;
                    const double b = (tv && j < a.d) ? pc[(size_t)t * a.d + j] : 0.0;
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) {
                        const double av = (double)xw[rt * 16 * XS + t] - muv;       // padding: 0 - 0
                        acc[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b, acc[rt], 0, 0, 0);
                    }
                }
            }
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int r = 0; r < 4; r++) m[rt][r] += acc[rt][r] * acc[rt][r];
        }
        const double off = a.offset[c];
#pragma unroll
        for (int rt = 0; rt < RT; rt++) {
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int w = 1; w < 16; w <<= 1) m[rt][r] += __shfl_xor(m[rt][r], w, 64);       // over the 16 columns of the tile
            const double mv = mine == 0 ? m[rt][0] : (mine == 1 ? m[rt][1] : (mine == 2 ? m[rt][2] : m[rt][3]));
            const double lp = off - 0.5 * mv;
            if (lp > M[rt]) {                           // first index on ties
                S[rt] = S[rt] * exp(M[rt] - lp) + 1.0;
                M[rt] = lp;
                best[rt] = c;
            } else {
                S[rt] += exp(lp - M[rt]);
            }
            const int i = row0 + (wave * RT + rt) * 16 + lk + 4 * mine;
            if (a.log_resp && lr < 4 && i < a.n) a.log_resp[(size_t)i * a.k + c] = lp;
        }
    }
    if (lr >= 4) return;
#pragma unroll
    for (int rt = 0; rt < RT; rt++) {
        const int i = row0 + (wave * RT + rt) * 16 + lk + 4 * mine;
        if (i >= a.n) continue;
        const double lpn = M[rt] + log(S[rt]);
        a.log_prob[i] = lpn;
        if (a.labels) a.labels[i] = best[rt];
        if (a.log_resp)
            for (int c = 0; c < a.k; c++) a.log_resp[(size_t)i * a.k + c] -= lpn;       // the lane's own stores, read back
    }
}

// ---- E-step, diagonal covariances

// grid (row blocks, component blocks): lp [n][k] = offset_c - sum_t ((x_it - mu_ct) PC_ct)^2 / 2, features in order
__global__ __launch_bounds__(256) void gmm_estep_diag_kernel(const float *__restrict__ x, int n, int d, int k, const double *__restrict__ means,
                                                             const double *__restrict__ pc, const double *__restrict__ offset,
                                                             double *__restrict__ lp)
{
    __shared__ float xs[GMM_DR][GMM_DT + 1];
    __shared__ double ms[GMM_DC][GMM_DT], ps[GMM_DC][GMM_DT];
    const int tid = threadIdx.x, r = tid & 63, g = tid >> 6;
    const int row0 = blockIdx.x * GMM_DR, cb = blockIdx.y * GMM_DC;
    double acc[8];
#pragma unroll
    for (int u = 0; u < 8; u++) acc[u] = 0.0;
    for (int t0 = 0; t0 < d; t0 += GMM_DT) {
        __syncthreads();
        for (int e = tid; e < GMM_DR * GMM_DT; e += 256) {
            const int rr = e / GMM_DT, t = e % GMM_DT, i = row0 + rr;
            xs[rr][t] = (i < n && t0 + t < d) ? x[(size_t)i * d + t0 + t] : 0.f;
        }
        for (int e = tid; e < GMM_DC * GMM_DT; e += 256) {
            const int cc = e / GMM_DT, t = e % GMM_DT, c = cb + cc;
            const bool ok = c < k && t0 + t < d;
            ms[cc][t] = ok ? means[(size_t)c * d + t0 + t] : 0.0;
            ps[cc][t] = ok ? pc[(size_t)c * d + t0 + t] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int t = 0; t < GMM_DT; t++) {
            const double xv = (double)xs[r][t];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const double y = (xv - ms[g * 8 + u][t]) * ps[g * 8 + u][t];
                acc[u] += y * y;
            }
        }
    }
    const int i = row0 + r;
    if (i >= n) return;
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const int c = cb + g * 8 + u;
        if (c < k) lp[(size_t)i * k + c] = offset[c] - 0.5 * acc[u];
    }
}

// one thread per row: log_prob_norm = max + log(sum_c exp(lp_c - max)), the first argmax, and (normalise) lp -= log_prob_norm
__global__ __launch_bounds__(256) void gmm_finish_kernel(double *__restrict__ lp, int n, int k, int normalise, double *__restrict__ log_prob,
                                                         int *__restrict__ labels)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double *p = lp + (size_t)i * k;
    double mx = p[0];
    int bi = 0;
    for (int c = 1; c < k; c++) {
        const double v = p[c];
        if (v > mx) { mx = v; bi = c; }
    }
    double s = 0.0;
    for (int c = 0; c < k; c++) s += exp(p[c] - mx);
    const double lpn = mx + log(s);
    log_prob[i] = lpn;
    if (labels) labels[i] = bi;
    if (normalise)
        for (int c = 0; c < k; c++) p[c] -= lpn;
}

// ---- fixed-order sum of n doubles

__global__ __launch_bounds__(256) void gmm_runsum_kernel(const double *__restrict__ v, int n, double *__restrict__ part)
{
    const int r = blockIdx.x * 256 + threadIdx.x, e0 = r * GMM_SUM_RUN;
    if (e0 >= n) return;
    const int e1 = min(n, e0 + GMM_SUM_RUN);
    double s = 0.0;
    for (int e = e0; e < e1; e++) s += v[e];
    part[r] = s;
}

// out[0] = part[0] + part[1] + ... in run order (one block: each thread its contiguous share in order, the 256 shares in order)
__global__ __launch_bounds__(256) void gmm_final_kernel(const double *__restrict__ part, int nr, double *__restrict__ out)
{
    __shared__ double sh[256];
    const int per = (nr + 255) / 256, b0 = min(nr, (int)threadIdx.x * per), b1 = min(nr, b0 + per);
    double s = 0.0;
    for (int b = b0; b < b1; b++) s += part[b];
    sh[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int q = 0; q < 256; q++) t += sh[q];
    out[0] = t;
}

// ---- M-step

__device__ __forceinline__ double gmm_resp(const double *__restrict__ resp, size_t e, int log_domain)
{
    const double v = resp[e];
    return log_domain ? exp(v) : v;
}

// grid (runs, ceil(k / 256)): part_nk [run][k] = sum over the run's rows (index order) of r_ic
__global__ __launch_bounds__(256) void gmm_nk_kernel(const double *__restrict__ resp, int n, int k, int log_domain, int len,
                                                     double *__restrict__ part_nk)
{
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= k) return;
    const int i0 = blockIdx.x * len, i1 = min(n, i0 + len);
    double s = 0.0;
    for (int i = i0; i < i1; i++) s += gmm_resp(resp, (size_t)i * k + c, log_domain);
    part_nk[(size_t)blockIdx.x * k + c] = s;
}

// grid (runs, component blocks, feature blocks), TD threads along the features and 256 / TD groups of 16 components:
// part_x [run][k][d] = sum over the run's rows (index order) of r_ic x_i; SQ: part_q likewise of r_ic x_i^2
template <int TD, bool SQ>
__global__ __launch_bounds__(256) void gmm_msum_kernel(const float *__restrict__ x, int n, int d, int k, const double *__restrict__ resp,
                                                       int log_domain, int len, double *__restrict__ part_x, double *__restrict__ part_q)
{
    constexpr int CB = 16 * (256 / TD);
    __shared__ double rs[GMM_MROWS][CB];
    const int tid = threadIdx.x, tx = tid % TD, cg = tid / TD;
    const int t = blockIdx.z * TD + tx, cbase = blockIdx.y * CB;
    const int i0 = blockIdx.x * len, i1 = min(n, i0 + len);
    double sx[16], sq[16];
#pragma unroll
    for (int u = 0; u < 16; u++) { sx[u] = 0.0; sq[u] = 0.0; }
    for (int ch = i0; ch < i1; ch += GMM_MROWS) {
        __syncthreads();
        for (int e = tid; e < GMM_MROWS * CB; e += 256) {
            const int rr = e / CB, cc = e % CB, i = ch + rr, c = cbase + cc;
            rs[rr][cc] = (i < i1 && c < k) ? gmm_resp(resp, (size_t)i * k + c, log_domain) : 0.0;
        }
        __syncthreads();
        const int rows = min(GMM_MROWS, i1 - ch);
#pragma unroll 4
        for (int rr = 0; rr < rows; rr++) {
            const double xv = t < d ? (double)x[(size_t)(ch + rr) * d + t] : 0.0;
            const double xq = xv * xv;
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const double r = rs[rr][cg * 16 + u];
                sx[u] += r * xv;
                if (SQ) sq[u] += r * xq;
            }
        }
    }
    if (t >= d) return;
#pragma unroll
    for (int u = 0; u < 16; u++) {
        const int c = cbase + cg * 16 + u;
        if (c >= k) continue;
        const size_t o = ((size_t)blockIdx.x * k + c) * d + t;
        part_x[o] = sx[u];
        if (SQ) part_q[o] = sq[u];
    }
}

// one block per component: nk = the runs in run order + 10 eps, means = sum / nk, diag (part_q): cov = sum_q / nk - mean^2 + reg
__global__ __launch_bounds__(256) void gmm_mcombine_kernel(const double *__restrict__ part_nk, const double *__restrict__ part_x,
                                                           const double *__restrict__ part_q, int runs, int d, int k, double reg,
                                                           double *__restrict__ nk, double *__restrict__ means, double *__restrict__ cov)
{
    __shared__ double nks;
    const int c = blockIdx.x;
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int r = 0; r < runs; r++) s += part_nk[(size_t)r * k + c];
        s += 10.0 * 2.220446049250313e-16;
        nks = s;
        nk[c] = s;
    }
    __syncthreads();
    const double w = nks;
    for (int t = threadIdx.x; t < d; t += 256) {
        double s = 0.0, q = 0.0;
        for (int r = 0; r < runs; r++) {
            const size_t o = ((size_t)r * k + c) * d + t;
            s += part_x[o];
            if (part_q) q += part_q[o];
        }
        const double mu = s / w;
        means[(size_t)c * d + t] = mu;
        if (part_q) cov[(size_t)c * d + t] = q / w - mu * mu + reg;
    }
}

// tile p of the upper triangle in row-major order: (ta, tb) with ta <= tb < dt
__device__ __forceinline__ void gmm_tile_of(int p, int dt, int &ta, int &tb)
{
    int a = 0;
    while (a < dt - 1 && p >= dt - a) { p -= dt - a; a++; }
    ta = a;
    tb = a + p;
}

// grid (runs, k, tile groups): part [run][c][tile][16][16] = sum over the run's rows of (r_ic diff_i[16 ta + row]) diff_i[16 tb + col];
// 4 waves x GMM_CTILES tiles, tile p = 32 z + wave + 4 q
__global__ __launch_bounds__(256) void gmm_cov_kernel(const float *__restrict__ x, int n, int d, int k, const double *__restrict__ resp,
                                                      int log_domain, const double *__restrict__ means, int len, double *__restrict__ part)
{
    __shared__ __align__(16) float xs[GMM_CROWS * GMM_CXS];
    __shared__ double rs[GMM_CROWS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    const int DT = (d + 15) >> 4, DP = DT * 16, XS = gmm_cov_stride(d), T = gmm_cov_tiles(d);
    const int c = blockIdx.y;
    const int i0 = blockIdx.x * len, i1 = min(n, i0 + len);
    const double *mu = means + (size_t)c * d;
    int ca[GMM_CTILES], cbb[GMM_CTILES];
    double mua[GMM_CTILES], mub[GMM_CTILES];
    f64x4 acc[GMM_CTILES];
#pragma unroll
    for (int q = 0; q < GMM_CTILES; q++) {
        const int p = blockIdx.z * 4 * GMM_CTILES + wave + 4 * q;
        int ta = 0, tb = 0;
        if (p < T) gmm_tile_of(p, DT, ta, tb);
        ca[q] = 16 * ta + lr;
        cbb[q] = 16 * tb + lr;
        mua[q] = ca[q] < d ? mu[ca[q]] : 0.0;
        mub[q] = cbb[q] < d ? mu[cbb[q]] : 0.0;
        acc[q] = f64x4{0.0, 0.0, 0.0, 0.0};
    }
    for (int ch = i0; ch < i1; ch += GMM_CROWS) {
        __syncthreads();
        for (int e = tid; e < GMM_CROWS * DP; e += 256) {
            const int rr = e / DP, t = e - rr * DP, i = ch + rr;
            xs[rr * XS + t] = (i < i1 && t < d) ? x[(size_t)i * d + t] : 0.f;
        }
        if (tid < GMM_CROWS) rs[tid] = ch + tid < i1 ? gmm_resp(resp, (size_t)(ch + tid) * k + c, log_domain) : 0.0;
        __syncthreads();
#pragma unroll
        for (int s = 0; s < GMM_CROWS / 4; s++) {
            const int rr = 4 * s + lk;
            const double r = rs[rr];
#pragma unroll
            for (int q = 0; q < GMM_CTILES; q++) {
                if (blockIdx.z * 4 * GMM_CTILES + wave + 4 * q >= T) break;         // the same for the whole wave
                const double da = (double)xs[rr * XS + ca[q]] - mua[q], db = (double)xs[rr * XS + cbb[q]] - mub[q];
                acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(r * da, db, acc[q], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < GMM_CTILES; q++) {
        const int p = blockIdx.z * 4 * GMM_CTILES + wave + 4 * q;
        if (p >= T) break;
        double *o = part + (((size_t)blockIdx.x * k + c) * T + p) * 256;
#pragma unroll
        for (int g = 0; g < 4; g++) o[(lk + 4 * g) * 16 + lr] = acc[q][g];
    }
}

// grid (k, tiles): cov_c[ja][jb] = (the runs in run order) / nk_c (+ reg on the diagonal) for ja <= jb, copied to [jb][ja]
__global__ __launch_bounds__(256) void gmm_cov_combine_kernel(const double *__restrict__ part, int runs, int d, int k, const double *__restrict__ nk,
                                                              double reg, double *__restrict__ cov)
{
    const int c = blockIdx.x, p = blockIdx.y, DT = (d + 15) >> 4, T = gmm_cov_tiles(d);
    int ta, tb;
    gmm_tile_of(p, DT, ta, tb);
    const int ja = 16 * ta + (threadIdx.x >> 4), jb = 16 * tb + (threadIdx.x & 15);
    if (ja >= d || jb >= d || ja > jb) return;
    double s = 0.0;
    for (int r = 0; r < runs; r++) s += part[(((size_t)r * k + c) * T + p) * 256 + threadIdx.x];
    double v = s / nk[c];
    if (ja == jb) v += reg;
    cov[((size_t)c * d + ja) * d + jb] = v;
    cov[((size_t)c * d + jb) * d + ja] = v;
}

}  // namespace ralign
