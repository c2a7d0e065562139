// CTF phase flip of a particle stack (ra_phase_flip): per particle, embed the nx x nx image at offset o = (P - nx) / 2 in a
// P x P zero image (P = pad * nx), real 2-D DFT, multiply every coefficient by m = -sign(ctf) (+1 where ctf == 0), inverse DFT
// normalised to return the input for m == 1, keep the nx x nx window at o.
//
// One workgroup per particle, three passes over an nx x (P/2 + 1) complex block.  Only the transforms whose input is not all
// zero, or whose output is kept, run (nx rows, P/2 + 1 columns); each of them is a full length-P FFT of its zero-filled input:
//   1. row transforms: two real rows packed into one complex length-P FFT (a + i b), split into their two half spectra;
//   2. column transforms: each kx column of nx non-zero rows, length-P FFT, multiply by m (evaluated in double from the
//      particle's 9 CTF parameters, never stored), inverse FFT, keep the nx window rows, written back in place;
//   3. inverse row transforms: two Hermitian-extended half spectra packed into one complex inverse FFT, the nx window outputs.
// The FFTs are mixed-radix Stockham transforms in LDS (radix 2 / 3 / 4 / 5 butterflies in registers, a direct stage for any
// other prime factor), batched over `nb` rows or columns between barriers.  The block lives in LDS when it fits
// (PF_LDS_BUDGET), otherwise in a per-workgroup slice of global scratch (large boxes; the workgroups then loop over the
// particles).  No atomics, a fixed operation order: bitwise reproducible, and no particle reads another's data.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>

namespace ralign {

#define PF_MAX_RADICES 24
#define PF_THREADS 512
#define PF_LDS_BUDGET ((size_t)160 * 1024 - 1024)
// Rows / columns per FFT batch (profiles/phase_flip_batch_ab.json: batches of 32, 8 and 4, alternated on one MI355X):
//  * block in LDS: the largest batch (<= PF_NB_MAX) with which TWO workgroups share a CU, if that batch is at least
//    PF_NB_TWO_MIN (90 x 90 at 2x: 5 per batch, 10.1 ms per 50 000 against 11.0 ms with one workgroup of 32 per batch), else the
//    largest batch in the whole LDS (100 x 100 at 2x: 25; 90 x 90 at 1x: 32 in 80 KB, two per CU anyway);
//  * block in global scratch: PF_NB_GBLK (130 x 130 at 2x: 5.7 ms per 5 000 against 7.2 ms with 32, 6.1 ms with 4;
//    256 x 256: 15.6 ms per 8 192 against 18.4 ms and 16.2 ms).
// The block goes to global scratch when LDS would leave fewer than PF_LDS_MIN_NB per batch next to it (128, 130, 256 at 2x).
#define PF_NB_MAX 32
#define PF_NB_TWO_MIN 4
#define PF_NB_GBLK 8
#define PF_LDS_MIN_NB 16

struct PfPlan {
    int nx, P, H, o;        // box, padded size, half-spectrum length P/2 + 1, window offset
    int nb;                 // rows / columns per FFT batch (0: no plan)
    int gblk;               // 1: the block lives in global scratch
    int lds;                // dynamic LDS bytes
    int nrad;               // radices of P in stage order
    int rad[PF_MAX_RADICES];
};

// the plan of one box: radices of P (4s first, then 2, 3, 5, then any other prime), the batch and where the block lives.
// constexpr: the kernels specialised for the common boxes fold it into their code (every index division by a constant)
__host__ __device__ constexpr PfPlan pf_make_plan(int nx, int pad)
{
    PfPlan pl{};
    pl.nx = nx;
    pl.P = pad ? 2 * nx : nx;
    pl.H = pl.P / 2 + 1;
    pl.o = (pl.P - nx) / 2;
    int r = pl.P;
    while (r % 4 == 0 && pl.nrad < PF_MAX_RADICES) { pl.rad[pl.nrad++] = 4; r /= 4; }
    for (int f = 2; f <= r && pl.nrad < PF_MAX_RADICES;) {
        if (r % f == 0) { pl.rad[pl.nrad++] = f; r /= f; }
        else f++;
    }
    if (r != 1) return pl;
    const long cap = (long)(PF_LDS_BUDGET / 8), P = pl.P, blk = (long)nx * pl.H;
    pl.gblk = P + 2 * P * PF_LDS_MIN_NB + blk > cap;
    long nb = (cap - P - (pl.gblk ? 0 : blk)) / (2 * P);
    if (pl.gblk) {
        nb = nb < PF_NB_GBLK ? nb : PF_NB_GBLK;
    } else {
        // two workgroups per CU: each within 78 KiB (90 x 90 at 2x with 5 per batch, 81 360 B, ran one per CU: 15.8 ms)
        const long two = ((long)78 * 1024 / 8 - P - blk) / (2 * P);
        if (two >= PF_NB_TWO_MIN) nb = two;
        nb = nb < PF_NB_MAX ? nb : PF_NB_MAX;
    }
    if (nb < 1) return pl;
    pl.nb = (int)nb;
    pl.lds = (int)((P + 2 * P * nb + (pl.gblk ? 0 : blk)) * 8);
    return pl;
}

// The boxes (nx, pad) with kernels specialised for their pf_make_plan plan -- the common ones -- in every kernel family that
// runs these passes (phase flip, Wiener forward transform, particle filter)
#define PF_FIXED_BOXES(X) X(90, 1) X(90, 0) X(100, 1) X(128, 1) X(130, 1) X(256, 1)

#define PF_GBLK_BYTES ((size_t)512 << 20)      // global scratch of the large-box route: the grid is sized to stay within it

// workgroups of the global-block route: as many as fit on the chip at this LDS size (256 CUs), within PF_GBLK_BYTES of scratch
inline int pf_gblk_grid(const PfPlan &pl, int n)
{
    const size_t blk_bytes = (size_t)pl.nx * pl.H * sizeof(float2);
    const size_t resident = (size_t)256 * std::max(1, std::min(4, (int)((size_t)160 * 1024 / pl.lds)));     // <= 32 waves per CU
    return (int)std::min<size_t>((size_t)n, std::max<size_t>(1, std::min<size_t>(resident, PF_GBLK_BYTES / blk_bytes)));
}

// per-particle constants of the CTF sign, from the [9] row (D, Apix, DefocusU, DefocusV, DefocusAngle, Voltage, Cs, w,
// PhaseShift): ctf = sqrt(1 - w^2) sin g - w cos g = sin(g - asin w), so sign(ctf) = sign(sin(2 pi u)) with
// u = (g - asin w) / (2 pi) = -1/2 df lam s^2 + 1/4 Cs lam^3 s^4 - (phase + asin w) / (2 pi): no transcendental per coefficient
struct PfCtf {
    double q;               // s^2 per squared integer frequency: 1 / (P apix_eff)^2
    double dsum, ddif;      // (dfu + dfv) / 2, (dfu - dfv) / 2
    double c2a, s2a;        // cos 2 dfang, sin 2 dfang
    double lam, cs;         // wavelength (A), Cs (A)
    double phi0;            // (phase_shift + asin w) / (2 pi)
};

// the same with the astigmatism angle (degrees) given instead of row[4] (the Wiener averages' aligned frame, ralign_wiener.h)
__host__ __device__ inline PfCtf pf_ctf_constants_at(const float *row, int nx, int P, double dfang_deg)
{
    const double pi = 3.14159265358979323846;
    PfCtf c;
    const double D = row[0], apix = row[1], dfu = row[2], dfv = row[3], ang = dfang_deg * pi / 180.0;
    const double volt = row[5] * 1000.0, w = row[7], ps = row[8] * pi / 180.0;
    const double apix_eff = apix * D / nx;
    const double f = 1.0 / (P * apix_eff);
    c.q = f * f;
    c.dsum = 0.5 * (dfu + dfv);
    c.ddif = 0.5 * (dfu - dfv);
    c.c2a = cos(2.0 * ang);
    c.s2a = sin(2.0 * ang);
    c.lam = 12.2639 / sqrt(volt + 0.97845e-6 * volt * volt);
    c.cs = row[6] * 1.0e7;
    c.phi0 = (ps + asin(w)) / (2.0 * pi);
    return c;
}

__host__ __device__ inline PfCtf pf_ctf_constants(const float *row, int nx, int P) { return pf_ctf_constants_at(row, nx, P, row[4]); }

// m(iy, ix) in {+1, -1} at the signed integer frequencies (iy along the rows, ix along the fast axis)
__host__ __device__ inline float pf_multiplier(const PfCtf &c, int iy, int ix)
{
    const double x = ix, y = iy, r2 = x * x + y * y;
    double df = c.dsum;
    if (r2 > 0.0) {
        // cos 2(theta - dfang) with theta = atan2(y, x): cos 2theta = (x^2 - y^2) / r^2, sin 2theta = 2 x y / r^2
        const double inv = 1.0 / r2;
        df += c.ddif * (((x * x - y * y) * c.c2a + 2.0 * x * y * c.s2a) * inv);
    }
    const double s2 = r2 * c.q, l3 = c.lam * c.lam * c.lam;
    const double u = -0.5 * df * c.lam * s2 + 0.25 * c.cs * l3 * s2 * s2 - c.phi0;
    const double fr = u - floor(u);
    // ctf > 0 <=> 0 < fr < 1/2: then m = -1; ctf < 0 and ctf == 0 give +1
    return (fr > 0.0 && fr < 0.5) ? -1.f : 1.f;
}

__host__ __device__ inline float2 pf_mul(float2 a, float2 b) { return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__host__ __device__ inline float2 pf_add(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__host__ __device__ inline float2 pf_sub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// d * i * a (d = -1 forward, +1 inverse)
__host__ __device__ inline float2 pf_rot(float2 a, float d) { return make_float2(-d * a.y, d * a.x); }

// R-point DFTs in registers, sign d of the exponent
__host__ __device__ inline void pf_dft2(float2 *v, float) { const float2 a = v[0]; v[0] = pf_add(a, v[1]); v[1] = pf_sub(a, v[1]); }

__host__ __device__ inline void pf_dft3(float2 *v, float d)
{
    const float c1 = -0.5f, s1 = 0.866025403784438647f;
    const float2 a = pf_add(v[1], v[2]), b = pf_sub(v[1], v[2]);
    const float2 t = make_float2(v[0].x + c1 * a.x, v[0].y + c1 * a.y);
    const float2 r = pf_rot(make_float2(s1 * b.x, s1 * b.y), d);
    v[0] = pf_add(v[0], a);
    v[1] = pf_add(t, r);
    v[2] = pf_sub(t, r);
}

__host__ __device__ inline void pf_dft4(float2 *v, float d)
{
    const float2 a = pf_add(v[0], v[2]), b = pf_sub(v[0], v[2]), c = pf_add(v[1], v[3]), e = pf_rot(pf_sub(v[1], v[3]), d);
    v[0] = pf_add(a, c);
    v[2] = pf_sub(a, c);
    v[1] = pf_add(b, e);
    v[3] = pf_sub(b, e);
}

__host__ __device__ inline void pf_dft5(float2 *v, float d)
{
    const float c1 = 0.309016994374947424f, c2 = -0.809016994374947424f;
    const float s1 = 0.951056516295153572f, s2 = 0.587785252292473129f;
    const float2 a1 = pf_add(v[1], v[4]), b1 = pf_sub(v[1], v[4]), a2 = pf_add(v[2], v[3]), b2 = pf_sub(v[2], v[3]);
    const float2 t1 = make_float2(v[0].x + c1 * a1.x + c2 * a2.x, v[0].y + c1 * a1.y + c2 * a2.y);
    const float2 t2 = make_float2(v[0].x + c2 * a1.x + c1 * a2.x, v[0].y + c2 * a1.y + c1 * a2.y);
    const float2 r1 = pf_rot(make_float2(s1 * b1.x + s2 * b2.x, s1 * b1.y + s2 * b2.y), d);
    const float2 r2 = pf_rot(make_float2(s2 * b1.x - s1 * b2.x, s2 * b1.y - s1 * b2.y), d);
    v[0] = pf_add(v[0], pf_add(a1, a2));
    v[1] = pf_add(t1, r1);
    v[4] = pf_sub(t1, r1);
    v[2] = pf_add(t2, r2);
    v[3] = pf_sub(t2, r2);
}

template <int R>
__host__ __device__ inline void pf_butterfly(const float2 *in, float2 *out, const float2 *tw, int P, int Ns, int j, float d)
{
    const int M = P / R, k = j % Ns, step = P / (Ns * R);
    float2 v[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        v[r] = in[j + r * M];
        if (r) {
            float2 w = tw[k * r * step];
            if (d > 0) w.y = -w.y;          // tw holds exp(-2 pi i t / P): conjugate for the inverse
            v[r] = pf_mul(v[r], w);
        }
    }
    if (R == 2) pf_dft2(v, d);
    if (R == 3) pf_dft3(v, d);
    if (R == 4) pf_dft4(v, d);
    if (R == 5) pf_dft5(v, d);
    const int o = (j / Ns) * Ns * R + k;
#pragma unroll
    for (int r = 0; r < R; r++) out[o + r * Ns] = v[r];
}

// one output of a direct radix-R stage (any R): out[(j / Ns) Ns R + k + r Ns] = sum_q in[j + q M] w^(k q P / (Ns R) + (r q mod R) M)
__host__ __device__ inline void pf_direct(const float2 *in, float2 *out, const float2 *tw, int P, int R, int Ns, int j, int r, float d)
{
    const int M = P / R, k = j % Ns, step = P / (Ns * R);
    float2 acc = make_float2(0.f, 0.f);
    for (int q = 0; q < R; q++) {
        float2 w = tw[(k * q * step + ((r * q) % R) * M) % P];
        if (d > 0) w.y = -w.y;
        acc = pf_add(acc, pf_mul(in[j + q * M], w));
    }
    out[(j / Ns) * Ns * R + k + r * Ns] = acc;
}

// Execution context of the passes: a workgroup on the device (threads tid, tid + nt, ... of every loop, a barrier between
// stages), one sequential thread on the host (the same arithmetic; tests/test_ctf_host_passes.py checks it without a GPU)
struct PfCtx {
    int tid, nt;
    __host__ __device__ void sync() const
    {
#if defined(__HIP_DEVICE_COMPILE__)
        __syncthreads();
#endif
    }
};

// nb transforms of length P (stride P) in a; ping-pong with b; returns the buffer that holds the result
template <class Ctx>
__host__ __device__ inline float2 *pf_fft(const Ctx &cx, float2 *a, float2 *b, int nb, const PfPlan &pl, const float2 *tw, float d)
{
    const int P = pl.P;
    int Ns = 1;
#pragma unroll
    for (int s = 0; s < pl.nrad; s++) {
        const int R = pl.rad[s], M = P / R;
        if (R <= 5) {
            const int items = nb * M;
            for (int it = cx.tid; it < items; it += cx.nt) {
                const int t = it / M, j = it - t * M;
                const float2 *in = a + (size_t)t * P;
                float2 *out = b + (size_t)t * P;
                switch (R) {
                case 2: pf_butterfly<2>(in, out, tw, P, Ns, j, d); break;
                case 3: pf_butterfly<3>(in, out, tw, P, Ns, j, d); break;
                case 4: pf_butterfly<4>(in, out, tw, P, Ns, j, d); break;
                default: pf_butterfly<5>(in, out, tw, P, Ns, j, d); break;
                }
            }
        } else {
            const int items = nb * P;
            for (int it = cx.tid; it < items; it += cx.nt) {
                const int t = it / P, e = it - t * P, j = e % M, r = e / M;
                pf_direct(a + (size_t)t * P, b + (size_t)t * P, tw, P, R, Ns, j, r, d);
            }
        }
        cx.sync();
        float2 *x = a; a = b; b = x;
        Ns *= R;
    }
    return a;
}

// pass 1: forward row transforms of img [nx][nx] embedded at o, two rows per complex FFT, into blk [nx][H]
template <class Ctx>
__host__ __device__ inline void pf_rows_forward(const Ctx &cx, const float *img, const PfPlan &pl, float2 *blk, float2 *work,
                                                const float2 *tw)
{
    const int nx = pl.nx, P = pl.P, H = pl.H, o = pl.o, nb = pl.nb;
    float2 *wa = work, *wb = work + (size_t)nb * P;
    const int npair = (nx + 1) / 2;
    for (int p0 = 0; p0 < npair; p0 += nb) {
        const int cnt = npair - p0 < nb ? npair - p0 : nb;
        for (int it = cx.tid; it < cnt * P; it += cx.nt) {
            const int t = it / P, n = it - t * P, ya = 2 * (p0 + t), yb = ya + 1, x = n - o;
            float2 v = make_float2(0.f, 0.f);
            if (x >= 0 && x < nx) {
                v.x = img[(size_t)ya * nx + x];
                if (yb < nx) v.y = img[(size_t)yb * nx + x];
            }
            wa[it] = v;
        }
        cx.sync();
        const float2 *z = pf_fft(cx, wa, wb, cnt, pl, tw, -1.f);
        for (int it = cx.tid; it < cnt * H; it += cx.nt) {
            const int t = it / H, k = it - t * H, ya = 2 * (p0 + t), yb = ya + 1;
            const float2 zk = z[(size_t)t * P + k], zm = z[(size_t)t * P + (k ? P - k : 0)];
            // Xa = (Z[k] + conj Z[-k]) / 2, Xb = (Z[k] - conj Z[-k]) / 2i
            blk[(size_t)ya * H + k] = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
            if (yb < nx) blk[(size_t)yb * H + k] = make_float2(0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x));
        }
        cx.sync();
    }
}

// pass 3: inverse row transforms of blk [nx][H] (the window rows), the nx window outputs times 1 / P^2 into img [nx][nx]:
// z = Xa + i Xb on the Hermitian extensions (imaginary parts of DC and Nyquist dropped, as c2r does)
template <class Ctx>
__host__ __device__ inline void pf_rows_inverse(const Ctx &cx, float *img, const PfPlan &pl, const float2 *blk, float2 *work,
                                                const float2 *tw)
{
    const int nx = pl.nx, P = pl.P, H = pl.H, o = pl.o, nb = pl.nb;
    float2 *wa = work, *wb = work + (size_t)nb * P;
    const int npair = (nx + 1) / 2;
    const float scale = 1.0f / ((float)P * (float)P);
    for (int p0 = 0; p0 < npair; p0 += nb) {
        const int cnt = npair - p0 < nb ? npair - p0 : nb;
        for (int it = cx.tid; it < cnt * P; it += cx.nt) {
            const int t = it / P, k = it - t * P, ya = 2 * (p0 + t), yb = ya + 1;
            const bool lo = k < H;
            const int kk = lo ? k : P - k;
            const bool real = kk == 0 || 2 * kk == P;
            float2 a = blk[(size_t)ya * H + kk], b = yb < nx ? blk[(size_t)yb * H + kk] : make_float2(0.f, 0.f);
            if (real) { a.y = 0.f; b.y = 0.f; }
            else if (!lo) { a.y = -a.y; b.y = -b.y; }
            wa[it] = make_float2(a.x - b.y, a.y + b.x);
        }
        cx.sync();
        const float2 *z = pf_fft(cx, wa, wb, cnt, pl, tw, 1.f);
        for (int it = cx.tid; it < cnt * nx; it += cx.nt) {
            const int t = it / nx, x = it - t * nx, ya = 2 * (p0 + t), yb = ya + 1;
            const float2 v = z[(size_t)t * P + o + x];
            img[(size_t)ya * nx + x] = v.x * scale;
            if (yb < nx) img[(size_t)yb * nx + x] = v.y * scale;
        }
        cx.sync();
    }
}

// the three passes over one particle; img [nx][nx] in place, blk [nx][H], work 2 x nb x P, tw [P] = exp(-2 pi i t / P)
template <class Ctx>
__host__ __device__ inline void pf_particle(const Ctx &cx, float *img, const PfCtf &cc, const PfPlan &pl, float2 *blk, float2 *work,
                                            const float2 *tw)
{
    const int nx = pl.nx, P = pl.P, H = pl.H, o = pl.o, nb = pl.nb;
    float2 *wa = work, *wb = work + (size_t)nb * P;
    // 1. forward row transforms, two rows per complex FFT
    pf_rows_forward(cx, img, pl, blk, work, tw);
    // 2. column transforms with the multiplier
    for (int c0 = 0; c0 < H; c0 += nb) {
        const int cnt = H - c0 < nb ? H - c0 : nb;
        for (int it = cx.tid; it < cnt * P; it += cx.nt) {
            const int t = it / P, n = it - t * P, y = n - o;
            wa[it] = (y >= 0 && y < nx) ? blk[(size_t)y * H + c0 + t] : make_float2(0.f, 0.f);
        }
        cx.sync();
        float2 *z = pf_fft(cx, wa, wb, cnt, pl, tw, -1.f);
        for (int it = cx.tid; it < cnt * P; it += cx.nt) {
            const int t = it / P, n = it - t * P;
            const int iy = n < (P + 1) / 2 ? n : n - P;          // signed row frequency (numpy.fft.fftfreq order)
            const float m = pf_multiplier(cc, iy, c0 + t);
            z[it] = make_float2(m * z[it].x, m * z[it].y);
        }
        cx.sync();
        float2 *zb = z == wa ? wb : wa;
        z = pf_fft(cx, z, zb, cnt, pl, tw, 1.f);
        for (int it = cx.tid; it < cnt * nx; it += cx.nt) {
            const int t = it / nx, y = it - t * nx;
            blk[(size_t)y * H + c0 + t] = z[(size_t)t * P + o + y];
        }
        cx.sync();
    }
    // 3. inverse row transforms
    pf_rows_inverse(cx, img, pl, blk, work, tw);
}

// GBLK = false: block, work and twiddles in dynamic LDS, one workgroup per particle.  GBLK = true: the block in global scratch
// (gscr + blockIdx.x * nx * H), the workgroups loop over the particles.
template <bool GBLK>
__device__ inline void pf_kernel_body(float *imgs, int n, const float *ctf, const PfPlan &pl, float2 *gscr)
{
    extern __shared__ float2 pf_lds[];
    const int P = pl.P;
    float2 *tw = pf_lds;
    float2 *work = pf_lds + P;
    float2 *blk = GBLK ? gscr + (size_t)blockIdx.x * pl.nx * pl.H : work + (size_t)2 * pl.nb * P;
    PfCtx cx{(int)threadIdx.x, PF_THREADS};
    for (int t = cx.tid; t < P; t += cx.nt) {
        double s, c;
        sincospi(-2.0 * t / P, &s, &c);
        tw[t] = make_float2((float)c, (float)s);
    }
    __syncthreads();
    for (int p = blockIdx.x; p < n; p += gridDim.x) {
        const PfCtf cc = pf_ctf_constants(ctf + (size_t)p * 9, pl.nx, P);
        pf_particle(cx, imgs + (size_t)p * pl.nx * pl.nx, cc, pl, blk, work, tw);
    }
}

// any box: the plan is a kernel argument
template <bool GBLK>
__global__ __launch_bounds__(PF_THREADS) void phase_flip_kernel(float *__restrict__ imgs, int n, const float *__restrict__ ctf,
                                                                 PfPlan pl, float2 *__restrict__ gscr)
{
    pf_kernel_body<GBLK>(imgs, n, ctf, pl, gscr);
}

// the boxes the benchmarks know (90, 100, 128, 130, 256): the plan is a compile-time constant
template <int NX, int PAD>
__global__ __launch_bounds__(PF_THREADS) void phase_flip_fixed_kernel(float *__restrict__ imgs, int n, const float *__restrict__ ctf,
                                                                       float2 *__restrict__ gscr)
{
    constexpr PfPlan pl = pf_make_plan(NX, PAD);
    static_assert(pl.nb > 0, "no plan");
    pf_kernel_body<pl.gblk != 0>(imgs, n, ctf, pl, gscr);
}

}  // namespace ralign
