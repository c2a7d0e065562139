// Two-stage dimension reduction (2SDR / MPCA, utils_ralib.py MPCA / TwoSDR) of an image stack in HBM.
//
//   sdr_mean_partial_kernel / sdr_mean_combine_kernel   per-pixel mean: double sums over fixed runs of SDR_MEAN_RUN images,
//                                                       then the runs in order; rounded to float once.
//   sdr_gram_kernel<FORM>                               Gram partials of one run of images x one output tile:
//                                                         FORM 0: sum_i X_i^T X_i                  (q x q)
//                                                         FORM 1: sum_i (X_i P)(X_i P)^T, P q x k   (p x p)
//                                                         FORM 2: sum_i (P^T X_i)^T (P^T X_i), P p x k (q x q)
//                                                       X_i = images[i] - mean (fp32, on load; no centring without a mean).
//   sdr_gram_combine_kernel                             adds the run partials in a fixed order in double; writes both halves.
//   sdr_project_kernel                                  U_i = A^T X_i B, [n][p0 q0] row-major (a, b) -> a q0 + b.
//   sdr_factors_kernel                                  F = U G, [n][r].
//   sdr_reconstruct_kernel                              x^_i = mean + A reshape(G f_i) B^T, [n][p][q], and |x_i - x^_i|^2.
//
// Every product is v_mfma_f32_16x16x4_f32 (exact f32 products, a k-ordered f32 fma chain). Operand maps (16x16x4): A[i][k] at
// lane (i = l & 15, k = l >> 4), B[k][j] at lane (k = l >> 4, j = l & 15), C/D row = (l >> 4) * 4 + reg, column = l & 15.
//
// Gram layout. The products are all Grams of a row stream Z (Z^T Z): the image rows (FORM 0), the rows of W_i = P^T X_i^T
// (FORM 1, k x p) or of W_i = P^T X_i (FORM 2, k x q). W_i is made by MFMA from the image in HBM and lives in LDS only. The d x d
// output is cut into nb x nb tiles of TD = 16 ns <= 128; only tiles ta <= tb are computed. A workgroup owns one tile and one
// run of images (run length fixed by the shape: SDR_RUN0_ROWS flattened rows for FORM 0, SDR_RUN_IMAGES images otherwise,
// never by the device), accumulates in f32 registers and writes its partial to scratch [run][tile][TD][TD]. The combine adds the
// partials in run order in double, so the result is bitwise reproducible and independent of how the grid is scheduled, and it
// writes G[a][b] and G[b][a] from one sum, so the Gram is exactly symmetric.
#pragma once

#include <hip/hip_runtime.h>

namespace ralign {

#define SDR_THREADS 256            // 4 waves
#define SDR_RUN0_ROWS 2048         // FORM 0: rows of the flattened [n p][q] stack per run (whole images: max(1, 2048 / p) images)
#define SDR_RUN_IMAGES 32          // FORMS 1, 2: images per run
#define SDR_MEAN_RUN 64            // images per partial of the mean
#define SDR_COMBINE_WAVES 16       // waves of a combine workgroup: wave w adds its contiguous share of the runs

__device__ __forceinline__ f32x4 sdr_mfma(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// W[j][wc] = sum_kk P[kk][j] Xc[kk][col(wc)] (FORM 2) or sum_kk P[kk][j] Xc[col(wc)][kk] (FORM 1), for j < 16 kt (zero for j >= k)
// and wc < 16 ncs; col(wc) = ta TD + wc below TD, tb TD + wc - TD above; zero where col >= d. Xc = image - mean.
// Wave w owns the column subtiles w, w + 4, w + 8, w + 12 and every row subtile, so each image element is loaded once per workgroup.
template <int FORM>
__device__ __forceinline__ void sdr_w_compute(const float *__restrict__ xi, const float *__restrict__ mean, int p, int q,
                                              const float *__restrict__ P, int k, int kt, int ncs, int TD, int ta, int tb,
                                              int d, float *W, int ws)
{
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int K = FORM == 1 ? q : p;
    f32x4 w[4][4];
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
        for (int jt = 0; jt < 4; jt++) w[u][jt] = f32x4{0.f, 0.f, 0.f, 0.f};
    int col[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int wc = (wave + 4 * u) * 16 + lr;
        col[u] = wc < TD ? ta * TD + wc : tb * TD + wc - TD;
    }
#pragma unroll 2
    for (int k0 = 0; k0 < K; k0 += 4) {
        const int kk = k0 + lk;
        float pa[4];
#pragma unroll
        for (int jt = 0; jt < 4; jt++) {
            const int j = jt * 16 + lr;
            pa[jt] = (jt < kt && kk < K && j < k) ? P[(size_t)kk * k + j] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (wave + 4 * u >= ncs) continue;
            float xv = 0.f;
            if (kk < K && col[u] < d) {
                const int idx = FORM == 1 ? col[u] * q + kk : kk * q + col[u];
                xv = mean ? xi[idx] - mean[idx] : xi[idx];
            }
#pragma unroll
            for (int jt = 0; jt < 4; jt++)
                if (jt < kt) w[u][jt] = sdr_mfma(pa[jt], xv, w[u][jt]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        if (wave + 4 * u >= ncs) continue;
#pragma unroll
        for (int jt = 0; jt < 4; jt++) {
            if (jt >= kt) continue;
#pragma unroll
            for (int r = 0; r < 4; r++) W[(jt * 16 + lk * 4 + r) * ws + (wave + 4 * u) * 16 + lr] = w[u][jt][r];
        }
    }
}

struct SdrGramArgs {
    const float *x, *mean, *proj;
    int n, p, q, k;                 // k: columns of proj (FORMS 1, 2)
    int d, nb, ns, ntile;           // output side, tiles per side, TD / 16, tiles computed (nb (nb + 1) / 2)
    int kt;                         // row subtiles of W: ceil(k / 16) (FORMS 1, 2), 1 (FORM 0: 16 stack rows per step)
    int run;                        // images per run
    float *part;                    // [nrun][ntile][TD][TD]
};

template <int FORM>
__global__ __launch_bounds__(SDR_THREADS) void sdr_gram_kernel(SdrGramArgs g)
{
    extern __shared__ __align__(16) float W[];
    const int TD = 16 * g.ns, ws = 2 * TD + 16;     // LDS row stride: the 4 rows of one operand read fall in distinct banks
    const int run = blockIdx.x, tile = blockIdx.y;
    int ta = 0, rem = tile;
    while (rem >= g.nb - ta) { rem -= g.nb - ta; ta++; }
    const int tb = ta + rem;
    const bool diag = ta == tb;
    const int ncs = diag ? g.ns : 2 * g.ns;         // column subtiles of W: block ta, then block tb
    const int boff = diag ? 0 : TD;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int nsub = g.ns * g.ns;

    // subtile t of this wave: s = wave + 4 t, (row, column) = (s / ns, s % ns); wave-uniform, so the offsets stay scalar
    f32x4 acc[16];
#pragma unroll
    for (int t = 0; t < 16; t++) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto live = [&](int t) {
        const int s = wave + 4 * t, ri = s / g.ns, ci = s - ri * g.ns;
        return s < nsub && (!diag || ri <= ci);
    };
    auto gram_step = [&](int rows) {
        for (int j0 = 0; j0 < rows; j0 += 4) {
            const float *wr = W + (j0 + lk) * ws + lr;
#pragma unroll
            for (int t = 0; t < 16; t++) {
                const int s = wave + 4 * t, ri = s / g.ns, ci = s - ri * g.ns;
                if (live(t)) acc[t] = sdr_mfma(wr[ri * 16], wr[boff + ci * 16], acc[t]);
            }
        }
    };

    const int i0 = run * g.run, i1 = min(g.n, i0 + g.run);
    if (FORM == 0) {
        const size_t r0 = (size_t)i0 * g.p, r1 = (size_t)i1 * g.p;
        const int wcols = ncs * 16;
        for (size_t rb = r0; rb < r1; rb += 16) {
            for (int e = threadIdx.x; e < 16 * wcols; e += SDR_THREADS) {
                const int jr = e / wcols, wc = e - jr * wcols;
                const int c = wc < TD ? ta * TD + wc : tb * TD + wc - TD;
                const size_t row = rb + jr;
                float v = 0.f;
                if (row < r1 && c < g.d) {
                    v = g.x[row * g.q + c];
                    if (g.mean) v = v - g.mean[(int)(row % (size_t)g.p) * g.q + c];
                }
                W[jr * ws + wc] = v;
            }
            __syncthreads();
            gram_step(16);
            __syncthreads();
        }
    } else {
        const int rows = (g.k + 3) & ~3;            // W rows at and above k are zero
        for (int i = i0; i < i1; i++) {
            sdr_w_compute<FORM>(g.x + (size_t)i * g.p * g.q, g.mean, g.p, g.q, g.proj, g.k, g.kt, ncs, TD, ta, tb, g.d, W, ws);
            __syncthreads();
            gram_step(rows);
            __syncthreads();
        }
    }
    float *dst = g.part + ((size_t)run * g.ntile + tile) * TD * TD;
#pragma unroll
    for (int t = 0; t < 16; t++) {
        if (!live(t)) continue;
        const int s = wave + 4 * t, ri = s / g.ns, ci = s - ri * g.ns;
#pragma unroll
        for (int r = 0; r < 4; r++) dst[(ri * 16 + lk * 4 + r) * TD + ci * 16 + lr] = acc[t][r];
    }
}

// G[a][b] = G[b][a] = sum over runs of the partials, for a <= b. 64 consecutive elements a d + b per workgroup; wave w adds runs
// [w C, (w + 1) C) in order, C = ceil(nrun / 16), then wave 0 adds the 16 wave sums in order: a fixed association for a given
// shape.
__global__ __launch_bounds__(64 * SDR_COMBINE_WAVES) void sdr_gram_combine_kernel(const float *__restrict__ part, int nrun, int ntile,
                                                                                 int nb, int ns, int d, double *__restrict__ gram)
{
    __shared__ double red[SDR_COMBINE_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, TD = 16 * ns;
    const size_t e = (size_t)blockIdx.x * 64 + lane;
    const int a = (int)(e / (size_t)d), b = (int)(e - (size_t)a * d);
    const bool valid = e < (size_t)d * d && a <= b;
    double s = 0.0;
    if (valid) {
        const int ta = a / TD, tb = b / TD;
        const int tile = ta * nb - ta * (ta - 1) / 2 + (tb - ta);
        const size_t local = (size_t)(a - ta * TD) * TD + (b - tb * TD), tstride = (size_t)TD * TD;
        const int C = (nrun + SDR_COMBINE_WAVES - 1) / SDR_COMBINE_WAVES;
        const int r1 = min(nrun, (wave + 1) * C);
        for (int r = wave * C; r < r1; r++) s += (double)part[((size_t)r * ntile + tile) * tstride + local];
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && valid) {
        double t = red[0][lane];
        for (int w = 1; w < SDR_COMBINE_WAVES; w++) t += red[w][lane];
        gram[(size_t)a * d + b] = t;
        gram[(size_t)b * d + a] = t;
    }
}

__global__ __launch_bounds__(256) void sdr_mean_partial_kernel(const float *__restrict__ x, int n, int npix, double *__restrict__ part)
{
    const int px = blockIdx.x * 256 + threadIdx.x, ch = blockIdx.y;
    if (px >= npix) return;
    const int i1 = min(n, (ch + 1) * SDR_MEAN_RUN);
    double s = 0.0;
    for (int i = ch * SDR_MEAN_RUN; i < i1; i++) s += (double)x[(size_t)i * npix + px];
    part[(size_t)ch * npix + px] = s;
}

__global__ __launch_bounds__(64 * SDR_COMBINE_WAVES) void sdr_mean_combine_kernel(const double *__restrict__ part, int nch, int npix,
                                                                                 int n, float *__restrict__ mean)
{
    __shared__ double red[SDR_COMBINE_WAVES][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, px = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (px < npix) {
        const int C = (nch + SDR_COMBINE_WAVES - 1) / SDR_COMBINE_WAVES, c1 = min(nch, (wave + 1) * C);
        for (int c = wave * C; c < c1; c++) s += part[(size_t)c * npix + px];
    }
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && px < npix) {
        double t = red[0][lane];
        for (int w = 1; w < SDR_COMBINE_WAVES; w++) t += red[w][lane];
        mean[px] = (float)(t / (double)n);
    }
}

// One image per workgroup. Stage 1: W[b][r] = sum_c B[c][b] Xc[r][c] (= (X_i B)^T, q0 x p, LDS). Stage 2: U[a][b] = sum_r A[r][a] W[b][r];
// wave w owns row subtile a in [16 w, 16 w + 16) and every column subtile.
__global__ __launch_bounds__(SDR_THREADS) void sdr_project_kernel(const float *__restrict__ x, const float *__restrict__ mean, int p, int q,
                                                                  const float *__restrict__ A, int p0, const float *__restrict__ B, int q0,
                                                                  float *__restrict__ U)
{
    extern __shared__ __align__(16) float W[];
    const int img = blockIdx.x, m = p0 * q0;
    const int ncs = (p + 15) / 16, ws = ncs * 16 + 4;        // +4: the 16 rows of one operand read fall in distinct banks
    const int kt = (q0 + 15) / 16, nbt = kt;
    sdr_w_compute<1>(x + (size_t)img * p * q, mean, p, q, B, q0, kt, ncs, 256, 0, 0, p, W, ws);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    if (wave * 16 >= p0) return;
    f32x4 acc[4];
#pragma unroll
    for (int bi = 0; bi < 4; bi++) acc[bi] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int a = wave * 16 + lr;
    for (int k0 = 0; k0 < p; k0 += 4) {
        const int kk = k0 + lk;
        const float av = (kk < p && a < p0) ? A[(size_t)kk * p0 + a] : 0.f;
#pragma unroll
        for (int bi = 0; bi < 4; bi++)
            if (bi < nbt) acc[bi] = sdr_mfma(av, kk < p ? W[(bi * 16 + lr) * ws + kk] : 0.f, acc[bi]);
    }
    float *u = U + (size_t)img * m;
#pragma unroll
    for (int bi = 0; bi < 4; bi++) {
        if (bi >= nbt) continue;
        const int b = bi * 16 + lr;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int ar = wave * 16 + lk * 4 + r;
            if (ar < p0 && b < q0) u[ar * q0 + b] = acc[bi][r];
        }
    }
}

// F = U G: U [n][m], G [m][r] (row-major), F [n][r]. 64 x 64 outputs per workgroup; wave w owns rows [16 w, 16 w + 16) of them.
__global__ __launch_bounds__(SDR_THREADS) void sdr_factors_kernel(const float *__restrict__ U, int n, int m, const float *__restrict__ G,
                                                                  int r, float *__restrict__ F)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int i0 = blockIdx.x * 64 + wave * 16, j0 = blockIdx.y * 64;
    f32x4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; u++) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int row = i0 + lr;
    for (int k0 = 0; k0 < m; k0 += 4) {
        const int kk = k0 + lk;
        const float a = (row < n && kk < m) ? U[(size_t)row * m + kk] : 0.f;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int col = j0 + u * 16 + lr;
            acc[u] = sdr_mfma(a, (kk < m && col < r) ? G[(size_t)kk * r + col] : 0.f, acc[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int col = j0 + u * 16 + lr;
#pragma unroll
        for (int rr = 0; rr < 4; rr++) {
            const int orow = i0 + lk * 4 + rr;
            if (orow < n && col < r) F[(size_t)orow * r + col] = acc[u][rr];
        }
    }
}

// Reconstruction. A workgroup owns a run of SDR_REC_RUN images (fixed, so an image's bits do not depend on n or on the grid).
//   stage 0, once per run:  c = F G^T as one [run][r] x [r][m] product: F's rows and 64 rows of G at a time are staged in LDS with
//                           coalesced loads, wave w owns 16 of the 64 columns; c lands in LDS as C_s[a][b], row stride qs.
//                           Without G the rows of F are C already.
//   A and B:                the operands of the tiles a wave owns (row tiles w, w + 4, .. of x^ for A, column tiles w, w + 4, ..
//                           of T for B) are loaded once into registers and serve every image of the run: NU tiles x KS steps
//                           of 4 columns, NU = ceil(max(p, q) / 64), KS = 4 ceil(max(p0, q0) / 16) (templates: the product loops
//                           carry no branch, a tile or step past its matrix multiplies selected zeros and is never stored).
//                           The steps run in the same order in every plan, so the plan does not show in the bits.
//   stage 1, per image:     T[a][y] = sum_b C[a][b] B[y][b]  ([p0][q], LDS, row stride ts).
//   stage 2, per image:     x^[x][y] = sum_a A[x][a] T[a][y], + mean, stored once; with resid the image is read at the same
//                           pixel and (x - x^)^2 summed in double: per lane in tile order, the lanes of a wave by halving
//                           shuffles, the four waves in order -- one writer, an order fixed by (p, q).
// c, C and T never leave LDS.  Strides: qs, rs = 4 mod 8 and ts = 16 mod 32, so the 16 rows (C, F, G) or the 4 rows (T) of one
// MFMA operand read fall in distinct banks.  Every operand outside its matrix is a selected 0, never a product with what LDS held.
#define SDR_REC_RUN 8

struct SdrRecPlan {
    int qs, rs, ts;                 // row strides of C, of the staged F and G rows, of T (floats)
    size_t floats;                  // dynamic LDS: C of the run, then the larger of T and the stage-0 staging
};

__host__ __device__ inline int sdr_rec_pad(int k) { k = (k + 3) & ~3; return (k & 4) ? k : k + 4; }

__host__ __device__ inline SdrRecPlan sdr_rec_plan(int r, bool has_g, int p0, int q0, int q)
{
    SdrRecPlan pl;
    pl.qs = sdr_rec_pad(q0);
    pl.rs = sdr_rec_pad(r);
    pl.ts = 16 * (((q + 15) / 16) | 1);
    const size_t t = (size_t)p0 * pl.ts, stage = has_g ? (size_t)(SDR_REC_RUN + 64) * pl.rs : 0;
    pl.floats = (size_t)SDR_REC_RUN * p0 * pl.qs + (t > stage ? t : stage);
    return pl;
}

struct SdrRecArgs {
    const float *F, *G, *A, *B, *mean, *x;     // G null: F is U; mean null: none added; x: the images, with resid only
    float *out;
    double *resid;
    int n, r, p0, q0, p, q;                     // r: columns of F (p0 q0 without G)
};

template <int KS, int NU>
__global__ __launch_bounds__(SDR_THREADS) void sdr_reconstruct_kernel(SdrRecArgs g)
{
    extern __shared__ __align__(16) float W[];
    __shared__ double red[SDR_THREADS / 64];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int m = g.p0 * g.q0, nxt = (g.p + 15) / 16, nyt = (g.q + 15) / 16, nat = (g.p0 + 15) / 16;
    const SdrRecPlan pl = sdr_rec_plan(g.r, g.G != nullptr, g.p0, g.q0, g.q);
    const int qs = pl.qs, rs = pl.rs, ts = pl.ts;
    float *Cs = W, *T = W + (size_t)SDR_REC_RUN * g.p0 * qs, *Fs = T, *Gs = T + SDR_REC_RUN * rs;
    const int i0 = blockIdx.x * SDR_REC_RUN, cnt = min(SDR_REC_RUN, g.n - i0);

    if (g.G) {
        // consecutive rows of r floats into LDS rows of stride rs: no division per element, four loads in flight per thread
        auto stage = [&](float *dst, const float *src, int count) {
            const int drow = SDR_THREADS / g.r, dcol = SDR_THREADS - drow * g.r;
            int row = threadIdx.x / g.r, col = threadIdx.x - row * g.r;
#pragma unroll 4
            for (int e = threadIdx.x; e < count; e += SDR_THREADS) {
                dst[row * rs + col] = src[e];
                row += drow;
                col += dcol;
                if (col >= g.r) { col -= g.r; row++; }
            }
        };
        stage(Fs, g.F + (size_t)i0 * g.r, cnt * g.r);
        for (int t0 = 0; t0 < m; t0 += 64) {
            const int rows = min(64, m - t0);
            __syncthreads();                    // F is staged; the previous rows of G are consumed
            stage(Gs, g.G + (size_t)t0 * g.r, rows * g.r);
            __syncthreads();
            if (t0 + wave * 16 >= m) continue;
            const int t = t0 + wave * 16 + lr;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < g.r; k0 += 4) {
                const int kk = k0 + lk;
                const float a = (lr < cnt && kk < g.r) ? Fs[lr * rs + kk] : 0.f;
                const float b = (t < m && kk < g.r) ? Gs[(wave * 16 + lr) * rs + kk] : 0.f;
                acc = sdr_mfma(a, b, acc);
            }
            if (t < m) {
                const int ta = t / g.q0, tb = t - ta * g.q0;
#pragma unroll
                for (int reg = 0; reg < 4; reg++)
                    if (lk * 4 + reg < cnt) Cs[((lk * 4 + reg) * g.p0 + ta) * qs + tb] = acc[reg];
            }
        }
    } else {
        for (int e = threadIdx.x; e < cnt * m; e += SDR_THREADS) {
            const int s = e / m, t = e - s * m, ta = t / g.q0;
            Cs[(s * g.p0 + ta) * qs + t - ta * g.q0] = g.F[(size_t)i0 * m + e];
        }
    }
    __syncthreads();                            // C is complete; the staging area becomes T

    float Areg[NU][KS], Breg[NU][KS];
#pragma unroll
    for (int u = 0; u < NU; u++)
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            const int xy = (wave + 4 * u) * 16 + lr, k = 4 * ks + lk;
            Areg[u][ks] = (xy < g.p && k < g.p0) ? g.A[xy * g.p0 + k] : 0.f;
            Breg[u][ks] = (xy < g.q && k < g.q0) ? g.B[xy * g.q0 + k] : 0.f;
        }

#pragma unroll 1
    for (int s = 0; s < cnt; s++) {
        const float *C = Cs + s * g.p0 * qs;
        for (int at = 0; at < nat; at++) {
            f32x4 acc[NU];
#pragma unroll
            for (int u = 0; u < NU; u++) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int a = at * 16 + lr;
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                const int k = 4 * ks + lk;
                const float cv = (a < g.p0 && k < g.q0) ? C[a * qs + k] : 0.f;
#pragma unroll
                for (int u = 0; u < NU; u++) acc[u] = sdr_mfma(cv, Breg[u][ks], acc[u]);
            }
#pragma unroll
            for (int u = 0; u < NU; u++) {
                if (wave + 4 * u >= nyt) continue;
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const int row = at * 16 + lk * 4 + reg;
                    if (row < g.p0) T[row * ts + (wave + 4 * u) * 16 + lr] = acc[u][reg];
                }
            }
        }
        __syncthreads();

        // The mean and the image values of a tile are fetched in front of the tile's products, which hide the loads: out may alias
        // both for the compiler, so a load written next to its use would wait behind the store before it, 16 round trips a tile.
        // Every address is a uniform row pointer plus one 32-bit lane offset, so the 48 of a tile cost no vector registers.
        const size_t base = (size_t)(i0 + s) * g.p * g.q;
        double rsum = 0.0;
#pragma unroll 1
        for (int yt = 0; yt < nyt; yt++) {
            const int y = yt * 16 + lr;
            const unsigned voff = (unsigned)((wave * 16 + lk * 4) * g.q + y);
            float mv[NU][4], xv[NU][4];
#pragma unroll
            for (int u = 0; u < NU; u++)
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    const bool in = (wave + 4 * u) * 16 + lk * 4 + reg < g.p && y < g.q;
                    const size_t row = (size_t)(64 * u + reg) * g.q;
                    mv[u][reg] = (in && g.mean) ? (g.mean + row)[voff] : 0.f;
                    xv[u][reg] = (in && g.resid) ? (g.x + base + row)[voff] : 0.f;
                }
            f32x4 acc[NU];
#pragma unroll
            for (int u = 0; u < NU; u++) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < KS; ks++) {
                const int k = 4 * ks + lk;
                const float tv = k < g.p0 ? T[k * ts + y] : 0.f;
#pragma unroll
                for (int u = 0; u < NU; u++) acc[u] = sdr_mfma(Areg[u][ks], tv, acc[u]);
            }
#pragma unroll
            for (int u = 0; u < NU; u++) {
                if (wave + 4 * u >= nxt) continue;
#pragma unroll
                for (int reg = 0; reg < 4; reg++) {
                    if ((wave + 4 * u) * 16 + lk * 4 + reg >= g.p || y >= g.q) continue;
                    const float v = g.mean ? acc[u][reg] + mv[u][reg] : acc[u][reg];
                    if (g.resid) {
                        const double d = (double)xv[u][reg] - (double)v;
                        rsum += d * d;
                    }
                    (g.out + base + (size_t)(64 * u + reg) * g.q)[voff] = v;
                }
            }
        }
        if (g.resid) {
            for (int off = 32; off > 0; off >>= 1) rsum += __shfl_down(rsum, off);
            if (lane == 0) red[wave] = rsum;
        }
        __syncthreads();                        // T is consumed; the waves' sums are in red
        if (g.resid && threadIdx.x == 0) g.resid[i0 + s] = ((red[0] + red[1]) + red[2]) + red[3];
    }
}


}  // namespace ralign
