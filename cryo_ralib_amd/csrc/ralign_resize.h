// Fourier resizing (binning / upsampling) of square images: y = A x A^T per image, A the real m x nx operator of
// resize.py / include/ralign.h (ra_fourier_resize):
//
//   A[j][i] = (1/nx) sum_{|k| <= s/2} w_k cos(2 pi k (t_j - u_i)),  t_j = (j - m/2) / m,  u_i = (i - nx/2) / nx,  s = min(nx, m),
//   w_k = 1/2 at |k| = nx/2 for even nx, otherwise 1.
//
//   resize_operator_kernel   builds A once per call in double (Dirichlet closed form, arguments reduced as exact integers),
//                            rounds it to f32 into a zero-padded [mp][nxp] block (mp = nt BT rows, nxp = nx rounded up to 64).
//   resize_kernel<NCT>       one workgroup (4 waves) per (image, BT x BT output tile), BT = 16 NCT <= 128:
//                              y[Jb][Cb] = sum over chunks of 64 image rows R:  A[Jb][R] (x[R][:] A[Cb][:]^T).
//                            Step 1: wave w computes T = x[r0 + 16 w .. +15][:] A[Cb][:]^T (16 x BT) with the image rows read
//                            from HBM straight into MFMA operands (each element once per tile), A from L2; T goes to LDS (T^T,
//                            [BT][64 + 4]).  Step 2: the 4 waves split the NCT^2 output subtiles, K = the 64 chunk rows, and
//                            accumulate in f32 registers; x A^T never leaves the workgroup.
//
// Every product is v_mfma_f32_16x16x4_f32 (exact f32 products, k-ordered f32 fma chains). Operand maps: A[i][k] at lane
// (i = l & 15, k = l >> 4), B[k][j] at lane (k = l >> 4, j = l & 15), C/D row = (l >> 4) * 4 + reg, column = l & 15. Each lane
// feeds 8 consecutive k (k0 + 8 (l >> 4) + s, s = 0..7) to 8 successive MFMAs, so a lane's operands are two float4 loads; both
// factors of a product use the same k map. The order of every sum is fixed by the shape alone: no atomics, and a particle's
// output does not depend on the batch it is in.
#pragma once

#include <hip/hip_runtime.h>

namespace ralign {

#define RS_THREADS 256             // 4 waves
#define RS_CHUNK 64                // image rows per step (16 per wave)
#define RS_TS (RS_CHUNK + 4)       // row stride (floats) of T^T in LDS
#define RS_MAX_BOX 1024

struct RsPlan {
    int nt;        // output tiles per axis
    int bt;        // tile edge (multiple of 16, <= 128)
    int mp;        // rows of the padded operand: nt bt
    int nxp;       // columns of the padded operand: nx rounded up to RS_CHUNK
};

static inline RsPlan rs_make_plan(int nx, int m)
{
    RsPlan p;
    p.nt = (m + 127) / 128;
    p.bt = ((m + p.nt - 1) / p.nt + 15) / 16 * 16;
    p.mp = p.nt * p.bt;
    p.nxp = (nx + RS_CHUNK - 1) / RS_CHUNK * RS_CHUNK;
    return p;
}

// Ap[j][i] for j < mp, i < nxp; zero outside j < m, i < nx.  p = (j - m/2) nx - (i - nx/2) m is t_j - u_i in units of 1/L,
// L = m nx; theta / 2 = pi p / L.  sum_{|k| <= h} cos k theta = sin((2h + 1) pi p / L) / sin(pi p / L) (2h + 1 where p = 0 mod L),
// minus cos(2 pi h p / L) when the source's Nyquist pair is in the band with half weights.  Both arguments are reduced modulo 2L
// in integers before the sine / cosine.
__global__ __launch_bounds__(256) void resize_operator_kernel(float *__restrict__ Ap, int nx, int m, int mp, int nxp)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long long)mp * nxp) return;
    const int j = (int)(idx / nxp), i = (int)(idx % nxp);
    if (j >= m || i >= nx) { Ap[idx] = 0.f; return; }
    const long long L = (long long)m * nx, L2 = 2 * L;
    const int s = min(nx, m), h = s / 2;
    const bool half = (nx % 2 == 0) && (nx <= m);           // |k| = nx/2 lies in the band: w = 1/2 there
    const long long p = (long long)(j - m / 2) * nx - (long long)(i - nx / 2) * m;
    auto red = [&](long long a) {                           // a mod 2L in [-L, L)
        long long r = a % L2;
        if (r < -L) r += L2;
        if (r >= L) r -= L2;
        return (double)r / (double)L;
    };
    double d;
    if (p % L == 0) {
        d = 2.0 * h + 1.0;
        if (half) d -= 1.0;
    } else {
        d = sinpi(red((2LL * h + 1) * p)) / sinpi(red(p));
        if (half) d -= cospi(red(2LL * h * p));
    }
    Ap[idx] = (float)(d / nx);
}

// 8 consecutive floats of row `row` from column k (zero at columns >= n).  VEC: the row start and k are 16-byte aligned and
// k + 8 <= n, so two float4 loads.
__device__ __forceinline__ void rs_load8(const float *__restrict__ row, int k, int n, bool vec, float (&v)[8])
{
    if (vec) {
        const float4 a = *(const float4 *)(row + k), b = *(const float4 *)(row + k + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    } else {
#pragma unroll
        for (int s = 0; s < 8; s++) v[s] = k + s < n ? row[k + s] : 0.f;
    }
}

__device__ __forceinline__ f32x4 rs_mfma(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// grid: one workgroup per (image, tile), tile fastest (the tiles of one image run together and share its rows in L2).
// in / out point at the first image of this launch; xvec: nx % 4 == 0 and `in` is 16-byte aligned (image rows load as float4).
template <int NCT>
__global__ __launch_bounds__(RS_THREADS) void resize_kernel(const float *__restrict__ in, float *__restrict__ out, int nx, int m,
                                                            int nt, const float *__restrict__ Ap, int nxp, int xvec)
{
    constexpr int BT = 16 * NCT;
    constexpr int NS = NCT * NCT;                 // output subtiles of the tile
    constexpr int NU = (NS + 3) / 4;              // ... per wave
    __shared__ float tT[BT * RS_TS];              // T^T: [c][chunk row]

    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
    const int tiles = nt * nt;
    const size_t img = blockIdx.x / tiles;
    const int tile = blockIdx.x % tiles, Jb = (tile / nt) * BT, Cb = (tile % nt) * BT;
    const float *__restrict__ x = in + img * (size_t)nx * nx;

    f32x4 acc[NU];
#pragma unroll
    for (int u = 0; u < NU; u++) acc[u] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int r0 = 0; r0 < nx; r0 += RS_CHUNK) {
        // step 1: T[16 w + i][c] = sum_k x[r0 + 16 w + i][k] A[Cb + c][k]
        f32x4 t[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ct++) t[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int r = r0 + 16 * wave + lr;
        const bool rin = r < nx;
        const float *__restrict__ xr = x + (size_t)(rin ? r : 0) * nx;
        for (int k0 = 0; k0 < nx; k0 += 32) {
            const int k = k0 + 8 * lk;
            float xv[8];
            rs_load8(xr, k, rin ? nx : 0, rin && xvec && k + 8 <= nx, xv);
#pragma unroll
            for (int ct = 0; ct < NCT; ct++) {
                float av[8];
                rs_load8(Ap + (size_t)(Cb + ct * 16 + lr) * nxp, k, nxp, true, av);
#pragma unroll
                for (int s = 0; s < 8; s++) t[ct] = rs_mfma(xv[s], av[s], t[ct]);
            }
        }
        __syncthreads();                          // the previous chunk's step 2 is done with tT
#pragma unroll
        for (int ct = 0; ct < NCT; ct++)
            *(f32x4 *)&tT[(ct * 16 + lr) * RS_TS + 16 * wave + 4 * lk] = t[ct];
        __syncthreads();
        // step 2: y[Jb + j][Cb + c] += sum_{q < 64} A[Jb + j][r0 + q] T[q][c]
#pragma unroll
        for (int u = 0; u < NU; u++) {
            const int st = wave + 4 * u;
            if (NS % 4 != 0 && st >= NS) break;
            const int jt = st / NCT, ct = st % NCT;
            const float *__restrict__ arow = Ap + (size_t)(Jb + jt * 16 + lr) * nxp + r0;
            const float *__restrict__ trow = tT + (ct * 16 + lr) * RS_TS;
#pragma unroll
            for (int q0 = 0; q0 < RS_CHUNK; q0 += 32) {
                float av[8], tv[8];
                rs_load8(arow, q0 + 8 * lk, RS_CHUNK, true, av);
                const float4 a = *(const float4 *)(trow + q0 + 8 * lk), b = *(const float4 *)(trow + q0 + 8 * lk + 4);
                tv[0] = a.x; tv[1] = a.y; tv[2] = a.z; tv[3] = a.w; tv[4] = b.x; tv[5] = b.y; tv[6] = b.z; tv[7] = b.w;
#pragma unroll
                for (int s = 0; s < 8; s++) acc[u] = rs_mfma(av[s], tv[s], acc[u]);
            }
        }
    }

    float *__restrict__ y = out + img * (size_t)m * m;
#pragma unroll
    for (int u = 0; u < NU; u++) {
        const int st = wave + 4 * u;
        if (NS % 4 != 0 && st >= NS) break;
        const int jt = st / NCT, ct = st % NCT, c = Cb + ct * 16 + lr;
        if (c >= m) continue;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const int j = Jb + jt * 16 + 4 * lk + e;
            if (j < m) y[(size_t)j * m + c] = acc[u][e];
        }
    }
}

}  // namespace ralign
