// Fourier resizing (ralign_resize.h): the engine-less ra_fourier_resize of libralign_hip.so, on the caller's stream.
#include <cstdint>

#include "ralign_host.h"
#include "ralign_resize.h"

using namespace ralign;

extern "C" int ra_fourier_resize(const float *d_in, int n, int nx, int m, float *d_out, void *hip_stream)
{
    if (n < 0 || nx < 1 || nx > RS_MAX_BOX || m < 1 || m > RS_MAX_BOX) return arg_error("ra_fourier_resize: need n >= 0 and 1 <= nx, m <= 1024");
    if (n == 0) return RA_OK;
    if (!d_in || !d_out) return arg_error("ra_fourier_resize: null argument");
    const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (size_t)n * nx * nx * sizeof(float);
    const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (size_t)n * m * m * sizeof(float);
    if (i0 < o1 && o0 < i1) return arg_error("ra_fourier_resize: d_in and d_out overlap");
    hipStream_t stream = (hipStream_t)hip_stream;
    const RsPlan pl = rs_make_plan(nx, m);
    const void *fk = nullptr;
    switch (pl.bt / 16) {
    case 1: fk = (const void *)resize_kernel<1>; break;
    case 2: fk = (const void *)resize_kernel<2>; break;
    case 3: fk = (const void *)resize_kernel<3>; break;
    case 4: fk = (const void *)resize_kernel<4>; break;
    case 5: fk = (const void *)resize_kernel<5>; break;
    case 6: fk = (const void *)resize_kernel<6>; break;
    case 7: fk = (const void *)resize_kernel<7>; break;
    default: fk = (const void *)resize_kernel<8>; break;
    }
    const size_t na = (size_t)pl.mp * pl.nxp;
    StreamScratch scratch(stream);
    float *Ap = scratch.get<float>(na);
    if (!Ap) return hip_error("ra_fourier_resize", scratch.status());
    hipLaunchKernelGGL(resize_operator_kernel, dim3((unsigned)((na + 255) / 256)), dim3(256), 0, stream, Ap, nx, m, pl.mp, pl.nxp);
    hipError_t he = hipGetLastError();
    // one workgroup per (image, tile); launches of at most 2^30 workgroups
    const int tiles = pl.nt * pl.nt, per = (1 << 30) / tiles;
    int nt = pl.nt, nxp = pl.nxp, xvec = (nx % 4 == 0) && (i0 % 16 == 0);
    for (int lo = 0; lo < n && he == hipSuccess; lo += per) {
        const int cnt = std::min(per, n - lo);
        const float *src = d_in + (size_t)lo * nx * nx;
        float *dst = d_out + (size_t)lo * m * m;
        int nx_ = nx, m_ = m;
        void *args[] = {&src, &dst, &nx_, &m_, &nt, &Ap, &nxp, &xvec};
        he = hipLaunchKernel(fk, dim3((unsigned)cnt * tiles), dim3(RS_THREADS), args, 0, stream);
        if (he == hipSuccess) he = hipGetLastError();
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_fourier_resize", he);
}
