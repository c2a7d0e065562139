// K4: rot_shift2D(img, alpha, sx, sy, mirror) ("quadratic", "background") and the per-class even/odd sums
// (test_mref_gpu_align.py:1055-1057; kernel_sum_oe :48-80).  Included by ralign_engine.hip only; needs ra_result and nothing
// of the search path's geometry (every kernel takes the box size nx).
//
//   transform_kernel | transform_generic_kernel   aligned images (image in LDS | in global memory), optionally fp32-atomic sums
//   class_members_wide_kernel + class_sum_kernel  particle-order sums of aligned images, cut into runs
//   transform_trig_kernel + transform_sum_db_kernel | transform_sum_kernel | transform_sum_tile_kernel
//                                                 both in one pass, no aligned stack (two padded copies of the image in LDS |
//                                                 one | the source box of an output tile)
//   class_sum_combine_kernel                      adds the runs in run order
// Every kernel is transform_kernel bit for bit.  The pieces that promise rests on are written once, in the xf_* functions
// below and quadri_background_1b, `__host__ __device__` without contraction: tests/test_xform_host.py runs them on the CPU.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/ralign.h"

namespace ralign {

// ---- the arithmetic, once (the reference tree's own restatement of rot_scale_trans2D_background / quadri_background,
// notebook/02 cell 2)

__host__ __device__ __forceinline__ float2 xf_trig(float alpha)
{
#pragma clang fp contract(off)
    const float ang = alpha * (float)M_PI / 180.0f;
    return make_float2((float)cos((double)ang), (float)sin((double)ang));
}

struct XfPose { float shiftxc, shiftyc, cang, sang; int mirror; };

__host__ __device__ __forceinline__ XfPose xf_pose(int nx, float sx, float sy, float2 cs, int mirror)
{
#pragma clang fp contract(off)
    float delx = sx, dely = sy;
    while (delx >= (float)nx) delx -= nx;
    while (delx <= -(float)nx) delx += nx;
    while (dely >= (float)nx) dely -= nx;
    while (dely <= -(float)nx) dely += nx;
    const int xc = nx / 2, yc = nx / 2;
    return XfPose{xc + delx, yc + dely, cs.x, cs.y, mirror};
}

// xform.mirror(x) reverses columns [1 - nx%2, nx): the column that column c trades places with
__host__ __device__ __forceinline__ int xf_mirror_col(int nx, int mirror, int c)
{
    const int mstart = 1 - nx % 2;
    return (mirror && c >= mstart) ? mstart + (nx - 1) - c : c;
}

// {x cos, x sin} of source column ix
__host__ __device__ __forceinline__ float2 xf_column(const XfPose &p, int ix)
{
#pragma clang fp contract(off)
    const float x = (float)ix - p.shiftxc;
    return make_float2(x * p.cang, x * p.sang);
}

// 1-based source position (xold + 1, yold + 1) of the pixel in row fy (an integer) of the column `col`
__host__ __device__ __forceinline__ float2 xf_source(const XfPose &p, float2 col, float fy, int nx)
{
#pragma clang fp contract(off)
    const int xc = nx / 2, yc = nx / 2;
    const float y = fy - p.shiftyc;
    const float ycang = y * p.cang + yc;
    const float ysang = -y * p.sang + xc;
    const float xold = col.x + ysang;
    const float yold = col.y + ycang;
    return make_float2(xold + 1.0f, yold + 1.0f);
}

__host__ __device__ __forceinline__ float quadri_background_1b(const float *fdata, int nx, int ny, float xx, float yy,
                                                               int xnew, int ynew)
{
#pragma clang fp contract(off)
    float x = xx, y = yy;
    // (written as the negation of "inside": a NaN position -- the parameters of a NaN particle -- takes the background branch too,
    // instead of (int)NaN = 0 indexing one row in front of the image)
    if (!((x >= 1.0f) && (x < (float)(nx + 1)) && (y >= 1.0f) && (y < (float)(ny + 1)))) { x = (float)xnew; y = (float)ynew; }
    int i = (int)x, j = (int)y;
    float dx0 = x - i, dy0 = y - j;
    int ip1 = i + 1, im1 = i - 1, jp1 = j + 1, jm1 = j - 1;
    if (ip1 > nx) ip1 -= nx;
    if (im1 < 1) im1 += nx;
    if (jp1 > ny) jp1 -= ny;
    if (jm1 < 1) jm1 += ny;
#define RA_FD(i_, j_) fdata[((j_) - 1) * nx + ((i_) - 1)]
    float f0 = RA_FD(i, j);
    float c1 = RA_FD(ip1, j) - f0;
    float c2 = (c1 - f0 + RA_FD(im1, j)) * 0.5f;
    float c3 = RA_FD(i, jp1) - f0;
    float c4 = (c3 - f0 + RA_FD(i, jm1)) * 0.5f;
    float dxb = dx0 - 1, dyb = dy0 - 1;
    int hxc = (dx0 >= 0) ? 1 : -1, hyc = (dy0 >= 0) ? 1 : -1;
    int ic = i + hxc, jc = j + hyc;
    if (ic > nx) ic -= nx; else if (ic < 1) ic += nx;
    if (jc > ny) jc -= ny; else if (jc < 1) jc += ny;
    float c5 = ((RA_FD(ic, jc) - f0 - hxc * c1 - (hxc * (hxc - 1.0f)) * c2 - hyc * c3 - (hyc * (hyc - 1.0f)) * c4) * (hxc * hyc));
#undef RA_FD
    return f0 + dx0 * (c1 + dxb * c2 + dy0 * c5) + dy0 * (c3 + dyb * c4);
}

// quadri_background_1b's polynomial on a periodic copy of the image, where the neighbours ip1 / im1 / jp1 / jm1 / (ic, jc) are
// plain offsets from q, the element of pixel (i, j), in rows of st elements.  The float operations are those of
// quadri_background_1b in the same order; two simplifications are exact: hxc = hyc = 1 always (x >= 1 after the background
// rule, so dx0 = x - (int)x >= 0), which turns hxc * c1 into c1 and drops the terms multiplied by hxc (hxc - 1) = 0.
__host__ __device__ __forceinline__ float xf_quadri_poly(const float *q, int st, float dx0, float dy0)
{
#pragma clang fp contract(off)
    const float f0 = q[0];
    const float c1 = q[1] - f0;
    const float c2 = (c1 - f0 + q[-1]) * 0.5f;
    const float c3 = q[st] - f0;
    const float c4 = (c3 - f0 + q[-st]) * 0.5f;
    const float dxb = dx0 - 1, dyb = dy0 - 1;
    const float c5 = q[st + 1] - f0 - c1 - c3;
    return f0 + dx0 * (c1 + dxb * c2 + dy0 * c5) + dy0 * (c3 + dyb * c4);
}

// quadri_background_1b on a copy of the image with a wrap-around border of one pixel (row stride pst, P = pointer to the
// element of 1-based pixel (0, 0)).  Two front ends, both exact, that differ in how the fraction and the range test are
// formed: this one for transform_sum_kernel ...
__host__ __device__ __forceinline__ float quadri_background_wrap(const float *P, int pst, int nx, float xx, float yy, int xnew, int ynew)
{
#pragma clang fp contract(off)
    float x = xx, y = yy;
    if (!((x >= 1.0f) && (x < (float)(nx + 1)) && (y >= 1.0f) && (y < (float)(nx + 1)))) { x = (float)xnew; y = (float)ynew; }          // (NaN: background)
    const int i = (int)x, j = (int)y;
    return xf_quadri_poly(P + j * pst + i, pst, x - i, y - j);
}

// ... and this one for transform_sum_db_kernel, with the fractions from v_fract: x >= 1 after the background rule, so
// x - (float)(int)x is x - floor(x), which v_fract returns exactly (bilinear_pad has the argument)
__host__ __device__ __forceinline__ float quadri_background_wrap1(const float *P, int pst, int nx, float xx, float yy, float xnew, float ynew)
{
#pragma clang fp contract(off)
    // (the four tests joined without short-circuit: selects, not branches; NaN: background)
    const float hi = (float)(nx + 1);
    const bool in = (xx >= 1.0f) & (xx < hi) & (yy >= 1.0f) & (yy < hi);
    const float x = in ? xx : xnew, y = in ? yy : ynew;
#if defined(__HIP_DEVICE_COMPILE__)
    const float dx0 = __builtin_amdgcn_fractf(x), dy0 = __builtin_amdgcn_fractf(y);
    const float *q = (const float *)((const char *)P + (__mul24((int)y, pst * 4) + ((int)x << 2)));          // (24-bit multiply: full rate, exact for these sizes)
#else
    const float dx0 = x - floorf(x), dy0 = y - floorf(y);
    const float *q = P + (int)y * pst + (int)x;
#endif
    return xf_quadri_poly(q, pst, dx0, dy0);
}

// members [j0, j1) of a list of cnt that run `run` of nrun adds
__host__ __device__ __forceinline__ int2 xf_run_range(int cnt, int run, int nrun)
{
    return make_int2((int)((long long)cnt * run / nrun), (int)((long long)cnt * (run + 1) / nrun));
}

// One wave walks particles [lo, hi) and appends those of (cls, par) to mem[base ..] in particle order (ballot + prefix count
// keeps the order); mem == null: counts only.  Returns base + their number.
__device__ __forceinline__ int xf_compact(const ra_result *__restrict__ res, int lo, int hi, int index0, int cls, int par,
                                          int *__restrict__ mem, int base)
{
    const int lane = threadIdx.x & 63;
    for (int i0 = lo; i0 < hi; i0 += 64) {
        const int i = i0 + lane;
        const bool mine = i < hi && res[i].ref_id == cls && ((index0 + i) & 1) == par;
        const unsigned long long m = __ballot(mine);
        if (mine && mem) mem[base + __popcll(m & ((1ull << lane) - 1ull))] = i;
        base += __popcll(m);
    }
    return base;
}

// ---- one image per workgroup

// 512 threads per particle: the image fills a quarter of the LDS, so four workgroups share a CU -- with 256 threads that is four
// waves per SIMD for a kernel paced by its chain of address -> six LDS taps -> interpolate (243 -> 200 us per 7143 particles)
#define RA_XF_THREADS 512
__global__ __launch_bounds__(RA_XF_THREADS) void transform_kernel(int nx, const float *__restrict__ particles, int n,
                                                        int index0, const ra_result *__restrict__ res,
                                                        float *__restrict__ aligned, float *__restrict__ sums,
                                                        int *__restrict__ counts)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float img[];
    const int p = blockIdx.x, tid = threadIdx.x, npix = nx * nx;
    if (p >= n) return;
    __shared__ float trig[2];
    const float *src = particles + (size_t)p * npix;
    for (int i = tid; i < npix; i += blockDim.x) img[i] = src[i];
    const ra_result r = res[p];
    if (tid == 0) { const float2 cs = xf_trig(r.alpha); trig[0] = cs.x; trig[1] = cs.y; }     // once per particle, not per thread
    __syncthreads();
    const XfPose ps = xf_pose(nx, r.sx, r.sy, make_float2(trig[0], trig[1]), r.mirror);
    float *dsum = sums ? sums + ((size_t)r.ref_id * 2 + ((index0 + p) & 1)) * npix : nullptr;
    float *dal = aligned ? aligned + (size_t)p * npix : nullptr;
    const unsigned nx_rcp = 0xFFFFFFFFu / (unsigned)nx + 1u;      // i / nx = (i * nx_rcp) >> 32, exact for i * nx < 2^32
    for (int i = tid; i < npix; i += blockDim.x) {
        const int iy = (int)__umulhi((unsigned)i, nx_rcp), ix = i - iy * nx;
        const float2 s = xf_source(ps, xf_column(ps, ix), (float)iy, nx);
        const float v = quadri_background_1b(img, nx, nx, s.x, s.y, ix + 1, iy + 1);
        const int o = iy * nx + xf_mirror_col(nx, r.mirror, ix);
        if (dal) dal[o] = v;
        if (dsum) atomicAdd(dsum + o, v);
    }
    if (counts && tid == 0) atomicAdd(counts + r.ref_id, 1);
}

// the same for images that do not fit LDS: quadri_background reads global memory
__global__ __launch_bounds__(256) void transform_generic_kernel(int nx, const float *__restrict__ particles, int n,
                                                                int index0, const ra_result *__restrict__ res,
                                                                float *__restrict__ aligned, float *__restrict__ sums,
                                                                int *__restrict__ counts)
{
#pragma clang fp contract(off)
    const int p = blockIdx.x, tid = threadIdx.x, npix = nx * nx;
    if (p >= n) return;
    const float *img = particles + (size_t)p * npix;
    const ra_result r = res[p];
    const XfPose ps = xf_pose(nx, r.sx, r.sy, xf_trig(r.alpha), r.mirror);
    float *dsum = sums ? sums + ((size_t)r.ref_id * 2 + ((index0 + p) & 1)) * npix : nullptr;
    float *dal = aligned ? aligned + (size_t)p * npix : nullptr;
    for (int i = blockIdx.y * blockDim.x + tid; i < npix; i += gridDim.y * blockDim.x) {
        const int iy = i / nx, ix = i - iy * nx;
        const float2 s = xf_source(ps, xf_column(ps, ix), (float)iy, nx);
        const float v = quadri_background_1b(img, nx, nx, s.x, s.y, ix + 1, iy + 1);
        const int o = iy * nx + xf_mirror_col(nx, r.mirror, ix);
        if (dal) dal[o] = v;
        if (dsum) atomicAdd(dsum + o, v);
    }
    if (counts && tid == 0 && blockIdx.y == 0) atomicAdd(counts + r.ref_id, 1);
}

// (float)cos / sin of the angle in double, once per particle, exactly as transform_kernel forms them
__global__ void transform_trig_kernel(const ra_result *__restrict__ res, int n, float2 *__restrict__ trig)
{
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    trig[p] = xf_trig(res[p].alpha);
}

// ---- K4b: per-class even/odd sums in PARTICLE ORDER (the order Util.add_img is called in on the CPU
// path, test_mref_gpu_align.py:1056-1057), hence bitwise reproducible: one workgroup per
// (class, parity, 256-pixel tile) walks the batch and adds the aligned images that belong to it.
// Same scan-all-particles shape as the reference's cu_average_batch_m (gpu_aln_noref.cu:1232-1274).
// With few classes a (class, parity) holds thousands of images and there are only 2 nref x tiles workgroups: the member
// list is then cut into gridDim.z contiguous runs (`partial` != null): workgroup z adds its run in particle order into
// partial[z][class, parity][pixel], and class_sum_combine_kernel adds the runs to the sums in run order -- a fixed
// association ((sums + run0) + run1) + ..., bitwise reproducible run to run like the single-run case.

// member lists of a chunk or a whole batch, once instead of once per workgroup: segment = (class, parity); 16 waves per
// segment, wave w compacts the particles of its contiguous 1/16 of the batch in particle order, after a counting pass that
// gives every wave its offset.  counts (may be null): += members per class (even + odd), added once.
__global__ __launch_bounds__(1024) void class_members_wide_kernel(const ra_result *__restrict__ res, int n, int index0,
                                                                  int *__restrict__ members, int *__restrict__ mcount, int mstride,
                                                                  int *__restrict__ counts)
{
    __shared__ int wcnt[16];
    const int seg = blockIdx.x, cls = seg >> 1, par = seg & 1, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per = ((n + 15) / 16 + 63) & ~63;
    const int lo = min(n, wave * per), hi = min(n, lo + per);
    const int c = xf_compact(res, lo, hi, index0, cls, par, nullptr, 0);
    if (lane == 0) wcnt[wave] = c;
    __syncthreads();
    int base = 0, total = 0;
    for (int w = 0; w < 16; w++) { if (w < wave) base += wcnt[w]; total += wcnt[w]; }
    xf_compact(res, lo, hi, index0, cls, par, members + (size_t)seg * mstride, base);
    if (threadIdx.x == 0) {
        mcount[seg] = total;
        if (counts && total) atomicAdd(counts + cls, total);
    }
}

// gmembers / gcount: the lists of class_members_wide_kernel ([segments][n], [segments]); null: every workgroup compacts its own
// list into LDS (segment counts too large for the list buffer)
__global__ __launch_bounds__(256) void class_sum_kernel(int npix, const float *__restrict__ aligned,
                                                        const ra_result *__restrict__ res, int n, int index0,
                                                        float *__restrict__ sums, int *__restrict__ counts,
                                                        float *__restrict__ partial, const int *__restrict__ gmembers,
                                                        const int *__restrict__ gcount)
{
    extern __shared__ int lmembers[];         // [n] particle indices of this (class, parity), ascending (gmembers == null only)
    __shared__ int nmem;
    const int seg = blockIdx.x, cls = seg >> 1, par = seg & 1;
    const int pix = blockIdx.y * blockDim.x + threadIdx.x;
    const bool live = pix < npix;
    const int *members = gmembers ? gmembers + (size_t)seg * n : lmembers;
    int cnt;
    if (gmembers) {
        cnt = gcount[seg];
    } else {
        if (threadIdx.x < 64) {          // wave 0 compacts the member list
            const int base = xf_compact(res, 0, n, index0, cls, par, lmembers, 0);
            if (threadIdx.x == 0) nmem = base;
        }
        __syncthreads();
        cnt = nmem;
    }
    const int run = blockIdx.z;
    const int2 jr = xf_run_range(cnt, run, gridDim.z);
    if (live) {
        float acc = partial ? 0.f : sums[(size_t)seg * npix + pix];
        int j = jr.x;
        for (; j + 4 <= jr.y; j += 4) {          // four loads in flight, added in particle order
            const float a0 = aligned[(size_t)members[j] * npix + pix], a1 = aligned[(size_t)members[j + 1] * npix + pix];
            const float a2 = aligned[(size_t)members[j + 2] * npix + pix], a3 = aligned[(size_t)members[j + 3] * npix + pix];
            acc += a0; acc += a1; acc += a2; acc += a3;
        }
        for (; j < jr.y; j++) acc += aligned[(size_t)members[j] * npix + pix];
        if (partial) partial[((size_t)run * gridDim.x + seg) * npix + pix] = acc;
        else sums[(size_t)seg * npix + pix] = acc;
    }
    if (counts && blockIdx.y == 0 && run == 0 && threadIdx.x == 0 && cnt) atomicAdd(counts + cls, cnt);
}

__global__ __launch_bounds__(256) void class_sum_combine_kernel(int npix, int nseg, int nrun, const float *__restrict__ partial,
                                                                float *__restrict__ sums)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nseg * npix) return;
    const size_t rst = (size_t)nseg * npix;
    float acc = sums[i];
    int r = 0;
    for (; r + 8 <= nrun; r += 8) {          // eight loads in flight, added in run order
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = partial[(size_t)(r + u) * rst + i];
#pragma unroll
        for (int u = 0; u < 8; u++) acc += v[u];
    }
    for (; r < nrun; r++) acc += partial[r * rst + i];
    sums[i] = acc;
}

// ---- K4c: rot_shift2D and the class sums in one pass: the aligned image is never written.  Workgroup (segment =
// (class, parity), run) walks over its contiguous share of the segment's member list IN PARTICLE ORDER: image -> LDS, every
// thread interpolates its pixels (the arithmetic of transform_kernel, bit for bit) and adds them to accumulators it keeps in
// registers; the next member's image is on its way from HBM meanwhile (register prefetch); cos / sin come from
// transform_trig_kernel.  partial[run][segment][pixel] receives the run's sum; class_sum_combine_kernel adds the runs in run
// order: a fixed association, bitwise reproducible run to run (the same shape as class_sum_kernel's runs).
// Replaces cu_transform_batch + cu_average_batch_m / kernel_sum_oe (cuda/gpu_aln_noref.cu:1145-1197, 1232-1274;
// test_mref_gpu_align.py:48-80, 449-453), which write and re-read the aligned stack.
#define RA_XS_THREADS 1024

// Thread (tx, ty) = (tid % nx, tid / nx) owns column tx of rows ty, ty + RY, ty + 2 RY, .. (RY = 1024 / nx rows per sweep of
// the workgroup, NPT sweeps): the column terms of the rotation -- mirror, x, x cos, x sin -- are formed once per member, pixel
// indices are tid + k RY nx, and nothing per-pixel has to live in registers besides the accumulator and the prefetched value.
// NPF sweeps fill the LDS image (NPF * (1024 / nx) >= nx), NPT sweeps of output rows per workgroup: larger boxes are cut into
// gridDim.z row bands (NPT * gridDim.z >= NPF) so that a thread keeps at most 9 accumulators -- every band loads the whole image
// (any pixel may be a tap), but 16 - 20 accumulators per thread next to their prefetch registers spilled 75 - 126 registers.
// (Launched for boxes of 100 pixels and more, always in row bands; smaller boxes go to transform_sum_db_kernel below.)
template <int NPT, int NPF = NPT>
__global__ __launch_bounds__(RA_XS_THREADS) void transform_sum_kernel(int nx, const float *__restrict__ particles,
                                                                      const ra_result *__restrict__ res, const float2 *__restrict__ trig,
                                                                      const int *__restrict__ members,
                                                                      const int *__restrict__ mcount, int mstride,
                                                                      float *__restrict__ partial)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float img[];          // [(nx + 2)][pst]: rows / columns 0 and nx + 1 repeat nx and 1
    const int seg = blockIdx.x, run = blockIdx.y, tid = threadIdx.x, npix = nx * nx;
    const int pst = (nx + 2) | 1;
    const int2 jr = xf_run_range(mcount[seg], run, gridDim.y);
    const int j0 = jr.x, j1 = jr.y;
    const int *mem = members + (size_t)seg * mstride;
    const unsigned nx_rcp = 0xFFFFFFFFu / (unsigned)nx + 1u;      // i / nx = (i * nx_rcp) >> 32, exact for i * nx < 2^32
    const int RY = RA_XS_THREADS / nx, S = RY * nx;               // rows, pixels per sweep
    const int ty = (int)__umulhi((unsigned)tid, nx_rcp), tx = tid - ty * nx;
    const bool live = tid < S;
    const int band = blockIdx.z * NPT;                            // first output sweep of this workgroup's row band
    float acc[NPT], pre[NPF];
#pragma unroll
    for (int k = 0; k < NPT; k++) acc[k] = 0.f;
    // wrap-around border of the padded copy: 4 nx + 4 elements, one per thread tid < 4 nx + 4 (padded (row, col) <- pixel)
    int bdst = -1, bsrc = 0;
    if (tid < 4 * nx + 4) {
        int pr, pc;
        if (tid < nx + 2) { pr = 0; pc = tid; }
        else if (tid < 2 * nx + 4) { pr = nx + 1; pc = tid - (nx + 2); }
        else if (tid < 3 * nx + 4) { pr = tid - (2 * nx + 4) + 1; pc = 0; }
        else { pr = tid - (3 * nx + 4) + 1; pc = nx + 1; }
        const int sr = pr == 0 ? nx - 1 : pr == nx + 1 ? 0 : pr - 1, sc = pc == 0 ? nx - 1 : pc == nx + 1 ? 0 : pc - 1;
        bdst = pr * pst + pc; bsrc = sr * nx + sc;
    }
    float preb = 0.f;
    // (tid and ty pass through an empty asm in every trip of the member loop: what derives from them per sweep -- pixel
    // indices, LDS addresses, row coordinates -- is then rebuilt with a few instructions instead of being hoisted out of the
    // loop into ~8 registers per sweep, more than the kernel has)
    auto fetch = [&](int j) {
        int t0 = tid;
        asm volatile("" : "+v"(t0));
        const float *src = particles + (size_t)mem[j] * npix;
#pragma unroll
        for (int k = 0; k < NPF; k++) pre[k] = src[min(t0 + k * S, npix - 1)];
        preb = src[bsrc];
    };
    if (j0 < j1) fetch(j0);
#pragma unroll 1
    for (int j = j0; j < j1; j++) {
        __syncthreads();                                  // the previous member's taps are read
        int t1 = tid, tyv = ty;
        asm volatile("" : "+v"(t1), "+v"(tyv));
        float *fill = img + (tyv + 1) * pst + tx + 1;
#pragma unroll
        for (int k = 0; k < NPF; k++)
            if (t1 < S && t1 + k * S < npix) fill[k * RY * pst] = pre[k];
        if (bdst >= 0) img[bdst] = preb;
        const ra_result r = res[mem[j]];
        const float2 cs = trig[mem[j]];
        __syncthreads();
        if (j + 1 < j1) fetch(j + 1);
        const XfPose ps = xf_pose(nx, r.sx, r.sy, cs, r.mirror);
        const int ix = xf_mirror_col(nx, r.mirror, tx);          // destination column tx: its source column
        const float2 col = xf_column(ps, ix);
#pragma unroll
        for (int k = 0; k < NPT; k++) {
            const int iy = min(tyv + (band + k) * RY, nx - 1);     // rows past the image (last sweep, idle threads) shadow the last row
            const float2 s = xf_source(ps, col, (float)iy, nx);
            acc[k] += quadri_background_wrap(img, pst, nx, s.x, s.y, ix + 1, iy + 1);
        }
    }
    float *dst = partial + ((size_t)run * gridDim.x + seg) * npix;
#pragma unroll
    for (int k = 0; k < NPT; k++) { const int o = tid + (band + k) * S; if (live && o < npix) dst[o] = acc[k]; }
}

// K4c': the same pass with TWO copies of the padded image in LDS, for boxes whose two copies still leave room for a second
// workgroup on the CU (nx <= 99).  The next member's image travels global -> LDS without a stop in registers while this one is
// interpolated -- one wave per padded row, the two wrap-around border rows included (they are whole image rows); only the two
// border columns, 2 nx + 4 elements, go through a register of the first threads -- so one barrier per member is left, no
// prefetch registers are held, and the next member's pose (res, trig) is asked for a member ahead.  A wave whose rows of a
// sweep all lie past the image (13 of 16 waves in the ninth sweep of a 90 x 90 box) skips that sweep.  Arithmetic, member
// order and the association of the runs are transform_sum_kernel's to the bit.  (Pairs of sweeps on packed floats were tried:
// 80 vector instructions per pair against 2 x 35 -- the compiler packs seven operations inside one pixel already, and pairs
// across sweeps pay register moves behind ds_read2 --; profiles/step_tail_ab.txt.)
// The grid is one-dimensional: the first nfull work items (segment, run) -- item = run * nseg + seg, the order the 3-D grid
// was dealt in -- come as nb0 row bands of sb0 sweeps each (band-major, nb0 = 1 up to 9 sweeps), the remaining ones, which
// would start another round of resident workgroups for a few items, as nb1 bands of sb1 sweeps behind them.  A band adds the
// same members in the same order to its own rows.
struct XsGrid { int nseg, nrun, nfull, sb0, nb0, sb1, nb1; };

// (amdgpu_waves_per_eu(8, 8): two workgroups of 16 waves per CU need 8 waves per SIMD.  Left to itself the compiler gives <9> 96
// scalar registers, which it counts as 7 waves -- one workgroup per CU, half the residency --; held to 8 waves it keeps up to 26
// scalar values in lanes of a VGPR instead, at most one of them read per sweep, and stays at 44 VGPRs without scratch.)
template <int NPT>
__global__ __launch_bounds__(RA_XS_THREADS) __attribute__((amdgpu_waves_per_eu(8, 8))) void transform_sum_db_kernel(int nx, const float *__restrict__ particles,
                                                                         const ra_result *__restrict__ res, const float2 *__restrict__ trig,
                                                                         const int *__restrict__ members,
                                                                         const int *__restrict__ mcount, int mstride,
                                                                         float *__restrict__ partial, XsGrid gr)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float img[];          // [2][(nx + 2)][pst]: rows / columns 0 and nx + 1 repeat nx and 1
    const int tid = threadIdx.x, npix = nx * nx;
    const int pst = (nx + 2) | 1, nimg = (nx + 2) * pst;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned nx_rcp = 0xFFFFFFFFu / (unsigned)nx + 1u;      // i / nx = (i * nx_rcp) >> 32, exact for i * nx < 2^32
    const int RY = RA_XS_THREADS / nx, S = RY * nx;               // rows, pixels per sweep
    const int npf = (nx + RY - 1) / RY;                           // sweeps over the whole image
    // work item and row band [k0, k0 + kn) of this workgroup
    int item, k0, kn;
    {
        const int b = blockIdx.x, nhead = gr.nfull * gr.nb0;
        if (b < nhead) { const int bd = b / gr.nfull; item = b - bd * gr.nfull; k0 = bd * gr.sb0; kn = gr.sb0; }
        else { const int s = b - nhead, nsur = gr.nseg * gr.nrun - gr.nfull, bd = s / nsur; item = gr.nfull + (s - bd * nsur); k0 = bd * gr.sb1; kn = gr.sb1; }
        kn = min(min(kn, NPT), npf - k0);
    }
    const int run = item / gr.nseg, seg = item - run * gr.nseg;
    const int2 jr = xf_run_range(mcount[seg], run, gr.nrun);
    const int j0 = jr.x, j1 = jr.y;
    const int *mem = members + (size_t)seg * mstride;
    const int ty = (int)__umulhi((unsigned)tid, nx_rcp), tx = tid - ty * nx;
    const int tyw = __builtin_amdgcn_readfirstlane(ty);          // the wave's first row (its lanes' rows ascend)
    const bool live = tid < S;
    float acc[NPT];
#pragma unroll
    for (int k = 0; k < NPT; k++) acc[k] = 0.f;
    // the two border columns of the padded copy: 2 nx + 4 elements, one per thread tid < 2 nx + 4 (padded (row, col) <- pixel)
    int bdst = -1, bsrc = 0;
    if (tid < 2 * nx + 4) {
        const int right = tid >= nx + 2, pr = right ? tid - (nx + 2) : tid;
        const int sr = pr == 0 ? nx - 1 : pr == nx + 1 ? 0 : pr - 1;
        bdst = pr * pst + (right ? nx + 1 : 0); bsrc = sr * nx + (right ? 0 : nx - 1);
    }
    float preb = 0.f;
    // a member's pose as fetched, one member ahead: the shifts are wrapped (xf_pose) when its turn comes
    struct Pose { float sx, sy, cang, sang; int mirror; };
    auto pose_of = [&](int m) { const ra_result r = res[m]; const float2 cs = trig[m]; return Pose{r.sx, r.sy, cs.x, cs.y, r.mirror}; };
    // particle m -> copy `dst`: padded row pr is image row pr - 1 (mod nx) at columns 1 .. nx, pieces of 64 pixels per request
    auto fill = [&](int m, float *dst) {
        const float *src = particles + (size_t)m * npix;
        if (bdst >= 0) preb = src[bsrc];
#pragma unroll 1
        for (int pr = wave; pr < nx + 2; pr += RA_XS_THREADS / 64) {
            const int sr = pr == 0 ? nx - 1 : pr == nx + 1 ? 0 : pr - 1;
            const float *row = src + sr * nx + lane;
            float *drow = dst + pr * pst + 1;
            // (nx <= 99 here: two pieces; the second one through the instruction's offset, which moves source and destination alike)
            if (lane < nx) __builtin_amdgcn_global_load_lds(row, (__attribute__((address_space(3))) void *)drow, 4, 0, 0);
            if (lane + 64 < nx) __builtin_amdgcn_global_load_lds(row, (__attribute__((address_space(3))) void *)drow, 4, 256, 0);
        }
    };
    Pose cur{}, nxt{};
    int mcur = 0, mnxt = 0;
    if (j0 < j1) {
        mcur = mem[j0]; mnxt = mem[min(j0 + 1, j1 - 1)];
        fill(mcur, img);
        cur = pose_of(mcur);
    }
#pragma unroll 1
    for (int j = j0; j < j1; j++) {
        float *buf = img + ((j - j0) & 1) * nimg;
        if (bdst >= 0) buf[bdst] = preb;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                  // this member's copy is complete; the other copy's taps are read
        if (j + 1 < j1) {
            fill(mnxt, img + ((j + 1 - j0) & 1) * nimg);
            nxt = pose_of(mnxt);
            mnxt = mem[min(j + 2, j1 - 1)];
        }
        // (ty passes through an empty asm in every trip: the row coordinates of the sweeps are rebuilt from it with a few
        // instructions instead of being hoisted out of the loop into registers, as in transform_sum_kernel)
        int tyv = ty;
        asm volatile("" : "+v"(tyv));
        const XfPose ps = xf_pose(nx, cur.sx, cur.sy, make_float2(cur.cang, cur.sang), cur.mirror);
        const int ix = xf_mirror_col(nx, cur.mirror, tx);          // destination column tx: its source column
        const float2 col = xf_column(ps, ix);
        const float xnew = (float)ix + 1.0f;              // the pixel's own 1-based position (small integers: exact)
#pragma unroll
        for (int k = 0; k < NPT; k++) {
            // rows past the image (last sweep, idle threads) shadow the last row; a wave whose first row is past it skips the sweep
            if (k < kn && tyw + (k0 + k) * RY < nx) {
                const float yi = (float)min(tyv + (k0 + k) * RY, nx - 1);
                const float2 s = xf_source(ps, col, yi, nx);
                acc[k] += quadri_background_wrap1(buf, pst, nx, s.x, s.y, xnew, yi + 1.0f);
            }
        }
        cur = nxt;
    }
    float *dst = partial + ((size_t)run * gr.nseg + seg) * npix;
#pragma unroll
    for (int k = 0; k < NPT; k++) {
        const int o = tid + (k0 + k) * S;
        if (k < kn && live && o < npix) dst[o] = acc[k];
    }
}

// K4d: the same for boxes whose image does not fit the LDS (transform_sum_kernel stops at ~140 pixels): workgroup = (segment, run,
// OUTPUT TILE of 64 x 64 pixels).  The taps of a tile's pixels lie in the rotated tile's bounding box in the source image, at most
// 63 (|cos| + |sin|) <= 89.1 pixels wide plus the neighbours of quadri and a margin for rounding: a box of 98 x 98 source pixels is brought in per member --
// global -> LDS without a stop in registers, periodic in both directions as quadri's own neighbour rule (ip1 / im1 wrap around), two
// boxes so that the next member's box travels while this one is interpolated -- and every thread adds its 8 pixels (column tx,
// rows ty + 8 k) to accumulators in registers (256 threads: 3.1 ms per 8192 x 256 x 256, 512: 1.9 ms, 1024: 2.6 ms).  A pixel whose source position lies outside the image takes the particle's own
// pixel (quadri_background's rule: the interpolation at the integer position (xnew, ynew) is that pixel, to the bit), read from
// global memory.  Arithmetic and association of the sums are transform_sum_kernel's: partial[run][segment][pixel], runs added in
// run order by class_sum_combine_kernel.
#define RA_XT_TS 64
#define RA_XT_BB 98
#define RA_XT_THREADS 512
// the origin (1-based source coordinates of box element (0, 0)) of the box that holds the taps of the output tile at (tx0, ty0)
__host__ __device__ __forceinline__ int2 xf_tile_origin(const XfPose &q, int nx, int tx0, int ty0)
{
#pragma clang fp contract(off)
    const int xc = nx / 2, yc = nx / 2, mstart = 1 - nx % 2;
    // source columns of the tile's destination columns (mirror reverses [mstart, nx)), rows ty0 .. ty0 + 63
    // (even nx: column 0 is not mirrored and its source lies a box away from its neighbours': it goes through global memory)
    const int c0 = (q.mirror && tx0 < mstart) ? mstart : tx0, c1 = min(tx0 + RA_XT_TS - 1, nx - 1);
    const int ia = q.mirror ? mstart + (nx - 1) - c1 : c0, ib = q.mirror ? mstart + (nx - 1) - c0 : c1;
    const float xa = (float)ia - q.shiftxc, xb = (float)ib - q.shiftxc;
    const float ya = (float)ty0 - q.shiftyc, yb = (float)min(ty0 + RA_XT_TS - 1, nx - 1) - q.shiftyc;
    float lox = 3.0e38f, loy = 3.0e38f;
#pragma unroll
    for (int c = 0; c < 4; c++) {
        const float x = (c & 1) ? xb : xa, y = (c & 2) ? yb : ya;
        lox = fminf(lox, x * q.cang - y * q.sang); loy = fminf(loy, x * q.sang + y * q.cang);
    }
    return make_int2((int)floorf(lox + xc + 1.0f) - 3, (int)floorf(loy + yc + 1.0f) - 3);
}

// source pixel (row, column) of box element (row, col): ((by0 + row - 1) mod nx, (bx0 + col - 1) mod nx), from the reduced
// origin (rb, cb) = ((by0 - 1) mod nx, (bx0 - 1) mod nx)
__host__ __device__ __forceinline__ int xf_box_origin(int b0, int nx) { const int b = (b0 - 1) % nx; return b < 0 ? b + nx : b; }
__host__ __device__ __forceinline__ int xf_box_source(int b, int off, int nx)
{
    int s = b + off;
    if (s >= nx) s -= nx;
    return s >= nx ? s % nx : s;       // boxes wider than the image (nx < 96): not the geometry this kernel is for, but exact
}

__global__ __launch_bounds__(RA_XT_THREADS) void transform_sum_tile_kernel(int nx, const float *__restrict__ particles,
                                                                           const ra_result *__restrict__ res, const float2 *__restrict__ trig,
                                                                           const int *__restrict__ members,
                                                                           const int *__restrict__ mcount, int mstride,
                                                                           float *__restrict__ partial)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) float box[];          // [2][RA_XT_BB * RA_XT_BB]
    constexpr int BB = RA_XT_BB, NB = BB * BB, NW = RA_XT_THREADS / 64, NK = RA_XT_TS / NW;
    const int seg = blockIdx.x, run = blockIdx.y, tid = threadIdx.x, npix = nx * nx;
    const int ntx = (nx + RA_XT_TS - 1) / RA_XT_TS;
    const int tx0 = (blockIdx.z % ntx) * RA_XT_TS, ty0 = (blockIdx.z / ntx) * RA_XT_TS;
    const int2 jr = xf_run_range(mcount[seg], run, gridDim.y);
    const int j0 = jr.x, j1 = jr.y;
    const int *mem = members + (size_t)seg * mstride;
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tx = tx0 + lane, ty = ty0 + wave;            // destination column; first destination row (then + NW k)
    const int mstart = 1 - nx % 2;
    float acc[NK];
#pragma unroll
    for (int k = 0; k < NK; k++) acc[k] = 0.f;
    struct Pose { XfPose p; int bx0, by0; };
    // the member's pose and the origin of its tile's box
    auto pose_of = [&](int j) {
        const ra_result r = res[mem[j]];
        Pose q;
        q.p = xf_pose(nx, r.sx, r.sy, trig[mem[j]], r.mirror);
        const int2 o = xf_tile_origin(q.p, nx, tx0, ty0);
        q.bx0 = o.x; q.by0 = o.y;
        return q;
    };
    auto stage = [&](int j, const Pose &q, float *dstbox) {
        const float *src = particles + (size_t)mem[j] * npix;
        const int cb = xf_box_origin(q.bx0, nx), rb = xf_box_origin(q.by0, nx);
#pragma unroll 1
        for (int e0 = wave * 64; e0 < NB; e0 += RA_XT_THREADS) {
            const int e = min(e0 + lane, NB - 1), row = e / BB, col = e - row * BB;
            const int sr = xf_box_source(rb, row, nx), sc = xf_box_source(cb, col, nx);
            if (e0 + lane < NB)
                __builtin_amdgcn_global_load_lds(src + sr * nx + sc, (__attribute__((address_space(3))) void *)(dstbox + e0), 4, 0, 0);
        }
    };
    Pose cur{}, nxt{};
    if (j0 < j1) { cur = pose_of(j0); stage(j0, cur, box); }
#pragma unroll 1
    for (int j = j0; j < j1; j++) {
        float *bx = box + ((j - j0) & 1) * NB;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                  // this member's box is complete; the other box is free
        if (j + 1 < j1) { nxt = pose_of(j + 1); stage(j + 1, nxt, box + ((j + 1 - j0) & 1) * NB); }
        if (tx < nx) {
            const int ix = xf_mirror_col(nx, cur.p.mirror, tx);
            const float2 col = xf_column(cur.p, ix);
            const float *P = bx - (cur.by0 * BB + cur.bx0);
            const float *own = particles + (size_t)mem[j] * npix + ix;
#pragma unroll
            for (int k = 0; k < NK; k++) {
                const int iy = min(ty + NW * k, nx - 1);
                const float2 s = xf_source(cur.p, col, (float)iy, nx);
                const float X = s.x, Y = s.y;
                float v;
                if (!((X >= 1.0f) && (X < (float)(nx + 1)) && (Y >= 1.0f) && (Y < (float)(nx + 1)))) {          // (NaN: background)
                    v = own[iy * nx];
                } else if (cur.p.mirror && tx < mstart) {
                    v = quadri_background_1b(particles + (size_t)mem[j] * npix, nx, nx, X, Y, ix + 1, iy + 1);
                } else {
                    const int i = (int)X, jj = (int)Y;
                    v = xf_quadri_poly(P + jj * BB + i, BB, X - i, Y - jj);
                }
                acc[k] += v;
            }
        }
        cur = nxt;
    }
    float *dst = partial + ((size_t)run * gridDim.x + seg) * npix;
    if (tx < nx) {
#pragma unroll
        for (int k = 0; k < NK; k++) { const int iy = ty + NW * k; if (iy < nx) dst[iy * nx + tx] = acc[k]; }
    }
}

}  // namespace ralign
