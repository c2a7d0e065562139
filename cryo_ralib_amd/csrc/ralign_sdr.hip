// Two-stage dimension reduction (ralign_sdr.h): the engine-less ra_sdr_* entry points of libralign_hip.so, each on the caller's stream.
#include "ralign_host.h"
#include "ralign_sdr.h"

using namespace ralign;

extern "C" int ra_sdr_mean(const float *d_images, int n, int p, int q, float *d_mean, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 1 || p < 1 || p > 256 || q < 1 || q > (p == 1 ? 2048 : 256))
        return arg_error("ra_sdr_mean: need n >= 1 and 1 <= p, q <= 256 (p == 1: q <= 2048)");
    if (!d_images || !d_mean) return arg_error("ra_sdr_mean: null argument");
    const int npix = p * q, nch = (n + SDR_MEAN_RUN - 1) / SDR_MEAN_RUN;
    StreamScratch scratch(stream);
    double *d_part = scratch.get<double>((size_t)nch * npix);
    if (!d_part) return hip_error("ra_sdr_mean", scratch.status());
    hipLaunchKernelGGL(sdr_mean_partial_kernel, dim3((npix + 255) / 256, nch), dim3(256), 0, stream, d_images, n, npix, d_part);
    hipError_t he = hipGetLastError();
    RA_LAUNCH(he, sdr_mean_combine_kernel, dim3((npix + 63) / 64), dim3(64 * SDR_COMBINE_WAVES), 0, stream, d_part, nch, npix, n, d_mean);
    return he == hipSuccess ? RA_OK : hip_error("ra_sdr_mean", he);
}

extern "C" int ra_sdr_gram(const float *d_images, int n, int p, int q, const float *d_mean, int form, const float *d_proj, int k,
                           double *d_gram, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (form < 0 || form > 2 || n < 1 || p < 1 || p > 256 || q < 1 || q > (form == 0 && p == 1 ? 2048 : 256))
        return arg_error("ra_sdr_gram: need form 0, 1 or 2, n >= 1, 1 <= p, q <= 256 (form 0 with p == 1: q <= 2048)");
    if (form != 0 && (k < 1 || k > 64 || k > (form == 1 ? q : p) || !d_proj))
        return arg_error("ra_sdr_gram: forms 1 and 2 need a projector with 1 <= k <= 64 columns and k <= q (form 1) or k <= p (form 2)");
    if (!d_images || !d_gram) return arg_error("ra_sdr_gram: null argument");
    SdrGramArgs g;
    g.x = d_images; g.mean = d_mean; g.proj = form ? d_proj : nullptr;
    g.n = n; g.p = p; g.q = q; g.k = form ? k : 0;
    g.d = form == 1 ? p : q;
    g.nb = (g.d + 127) / 128;
    g.ns = ((g.d + g.nb - 1) / g.nb + 15) / 16;
    g.ntile = g.nb * (g.nb + 1) / 2;
    g.kt = form ? (k + 15) / 16 : 1;
    g.run = form ? SDR_RUN_IMAGES : std::max(1, SDR_RUN0_ROWS / p);
    const int nrun = (n + g.run - 1) / g.run, TD = 16 * g.ns;
    const size_t lds = (size_t)16 * g.kt * (2 * TD + 16) * sizeof(float);
    const void *fk = form == 0 ? (const void *)sdr_gram_kernel<0> : form == 1 ? (const void *)sdr_gram_kernel<1> : (const void *)sdr_gram_kernel<2>;
    if (const int rc = raise_dynamic_lds(nullptr, fk, "sdr_gram_kernel", lds)) return rc;
    StreamScratch scratch(stream);
    g.part = scratch.get<float>((size_t)nrun * g.ntile * TD * TD);
    if (!g.part) return hip_error("ra_sdr_gram", scratch.status());
    void *args[] = {&g};
    hipError_t he = hipLaunchKernel(fk, dim3(nrun, g.ntile), dim3(SDR_THREADS), args, lds, stream);
    if (he == hipSuccess) he = hipGetLastError();
    if (he == hipSuccess) {
        const size_t nel = (size_t)g.d * g.d;
        hipLaunchKernelGGL(sdr_gram_combine_kernel, dim3((unsigned)((nel + 63) / 64)), dim3(64 * SDR_COMBINE_WAVES), 0, stream, g.part, nrun,
                           g.ntile, g.nb, g.ns, g.d, d_gram);
        he = hipGetLastError();
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_sdr_gram", he);
}

extern "C" int ra_sdr_project(const float *d_images, int n, int p, int q, const float *d_mean, const float *d_A, int p0, const float *d_B,
                              int q0, float *d_U, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 1 || p < 1 || p > 256 || q < 1 || q > 256 || p0 < 1 || p0 > std::min(p, 64) || q0 < 1 || q0 > std::min(q, 64) || p0 * q0 > 2048)
        return arg_error("ra_sdr_project: need n >= 1, 1 <= p, q <= 256, 1 <= p0 <= min(p, 64), 1 <= q0 <= min(q, 64) and p0 q0 <= 2048");
    if (!d_images || !d_A || !d_B || !d_U) return arg_error("ra_sdr_project: null argument");
    const size_t lds = (size_t)16 * ((q0 + 15) / 16) * (16 * ((p + 15) / 16) + 4) * sizeof(float);
    if (const int rc = RA_LDS(nullptr, sdr_project_kernel, lds)) return rc;
    hipLaunchKernelGGL(sdr_project_kernel, dim3(n), dim3(SDR_THREADS), lds, stream, d_images, d_mean, p, q, d_A, p0, d_B, q0, d_U);
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_sdr_project", he);
}

extern "C" int ra_sdr_factors(const float *d_U, int n, int m, const float *d_G, int r, float *d_F, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 1 || m < 1 || m > 2048 || r < 1 || r > std::min(256, m))
        return arg_error("ra_sdr_factors: need n >= 1, 1 <= m <= 2048 and 1 <= r <= min(256, m)");
    if (!d_U || !d_G || !d_F) return arg_error("ra_sdr_factors: null argument");
    hipLaunchKernelGGL(sdr_factors_kernel, dim3((n + 63) / 64, (r + 63) / 64), dim3(SDR_THREADS), 0, stream, d_U, n, m, d_G, r, d_F);
    hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_sdr_factors", he);
}

// sdr_reconstruct_kernel<4 ks4, nu>: the register plan of a shape (ralign_sdr.h)
template <int KS> static const void *sdr_reconstruct_nu(int nu)
{
    return nu == 1 ? (const void *)sdr_reconstruct_kernel<KS, 1> : nu == 2 ? (const void *)sdr_reconstruct_kernel<KS, 2>
         : nu == 3 ? (const void *)sdr_reconstruct_kernel<KS, 3> : (const void *)sdr_reconstruct_kernel<KS, 4>;
}

static const void *sdr_reconstruct_plan(int ks4, int nu)
{
    return ks4 == 1 ? sdr_reconstruct_nu<4>(nu) : ks4 == 2 ? sdr_reconstruct_nu<8>(nu) : ks4 == 3 ? sdr_reconstruct_nu<12>(nu)
                                                                                                  : sdr_reconstruct_nu<16>(nu);
}

extern "C" int ra_sdr_reconstruct(const float *d_F, int n, int r_or_m, const float *d_G, int p0, int q0, const float *d_A, int p,
                                  const float *d_B, int q, const float *d_mean, const float *d_images, float *d_out, double *d_resid,
                                  void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 0 || p < 1 || p > 256 || q < 1 || q > 256 || p0 < 1 || p0 > std::min(p, 64) || q0 < 1 || q0 > std::min(q, 64) || p0 * q0 > 2048)
        return arg_error("ra_sdr_reconstruct: need n >= 0, 1 <= p, q <= 256, 1 <= p0 <= min(p, 64), 1 <= q0 <= min(q, 64) and p0 q0 <= 2048");
    if (d_G ? (r_or_m < 1 || r_or_m > std::min(256, p0 * q0)) : r_or_m != p0 * q0)
        return arg_error("ra_sdr_reconstruct: need 1 <= r <= min(256, p0 q0) with d_G, and rows of p0 q0 factors without");
    if (n == 0) return RA_OK;
    if (!d_F || !d_A || !d_B || !d_out) return arg_error("ra_sdr_reconstruct: null argument");
    if ((d_images != nullptr) != (d_resid != nullptr)) return arg_error("ra_sdr_reconstruct: d_images and d_resid go together");
    SdrRecArgs g;
    g.F = d_F; g.G = d_G; g.A = d_A; g.B = d_B; g.mean = d_mean; g.x = d_images; g.out = d_out; g.resid = d_resid;
    g.n = n; g.r = r_or_m; g.p0 = p0; g.q0 = q0; g.p = p; g.q = q;
    const size_t lds = sdr_rec_plan(r_or_m, d_G != nullptr, p0, q0, q).floats * sizeof(float);
    const void *fk = sdr_reconstruct_plan((std::max(p0, q0) + 15) / 16, (std::max(p, q) + 63) / 64);
    if (const int rc = raise_dynamic_lds(nullptr, fk, "sdr_reconstruct_kernel", lds)) return rc;
    void *args[] = {&g};
    hipError_t he = hipLaunchKernel(fk, dim3((n + SDR_REC_RUN - 1) / SDR_REC_RUN), dim3(SDR_THREADS), args, lds, stream);
    if (he == hipSuccess) he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_sdr_reconstruct", he);
}
