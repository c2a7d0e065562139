// Gaussian mixture E- and M-step (ralign_gmm.h): the engine-less ra_gmm_* entry points of libralign_hip.so, each on the caller's
// stream.
#include "ralign_host.h"
#include "ralign_gmm.h"

using namespace ralign;

static bool gmm_shape_ok(const char *what, int n, int d, int k, int cov_type)
{
    const bool full = cov_type == RA_GMM_FULL;
    if ((cov_type != RA_GMM_FULL && cov_type != RA_GMM_DIAG) || k < 1 || k > GMM_MAX_K || n < k || n > GMM_MAX_N ||
        (long long)n * k > GMM_MAX_NK || d < 1 || d > (full ? GMM_MAX_D_FULL : GMM_MAX_D_DIAG)) {
        set_error(std::string(what) + ": need cov_type RA_GMM_FULL or RA_GMM_DIAG, 1 <= k <= 256, k <= n <= 4194304, n k <= 2^28 and "
                                      "1 <= d <= 256 (full) or 2048 (diag)");
        return false;
    }
    return true;
}

extern "C" int ra_gmm_estep(const float *d_x, int n, int d, int k, int cov_type, const double *d_means, const double *d_prec_chol,
                            const double *d_offset, double *d_log_resp, double *d_log_prob, int *d_labels, double *d_sum, void *hip_stream)
{
    if (!gmm_shape_ok("ra_gmm_estep", n, d, k, cov_type)) return RA_ERR_ARG;
    if (!d_x || !d_means || !d_prec_chol || !d_offset || !d_log_prob || !d_sum) return arg_error("ra_gmm_estep: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nr = (n + GMM_SUM_RUN - 1) / GMM_SUM_RUN;
    const bool full = cov_type == RA_GMM_FULL;
    const int dp = (d + 15) / 16 * 16, rt = dp <= 64 ? 4 : (dp <= 128 ? 2 : 1);
    const size_t lds = (size_t)64 * rt * (dp + 4) * sizeof(float);
    if (full) {
        const int rc = rt == 4 ? RA_LDS(nullptr, gmm_estep_full_kernel<4>, lds)
                               : (rt == 2 ? RA_LDS(nullptr, gmm_estep_full_kernel<2>, lds) : RA_LDS(nullptr, gmm_estep_full_kernel<1>, lds));
        if (rc) return rc;
    }
    StreamScratch scratch(stream);
    double *part = scratch.get<double>(nr);
    double *table = (full || d_log_resp) ? d_log_resp : scratch.get<double>((size_t)n * k);
    if (!part || (!full && !table)) return hip_error("ra_gmm_estep", scratch.status());
    hipError_t he = hipSuccess;
    if (full) {
        GmmEArgs a;
        a.x = d_x; a.means = d_means; a.pc = d_prec_chol; a.offset = d_offset; a.log_resp = d_log_resp; a.log_prob = d_log_prob;
        a.labels = d_labels; a.n = n; a.d = d; a.k = k;
        const dim3 grid((n + 64 * rt - 1) / (64 * rt)), block(256);
        if (rt == 4) hipLaunchKernelGGL(gmm_estep_full_kernel<4>, grid, block, lds, stream, a);
        else if (rt == 2) hipLaunchKernelGGL(gmm_estep_full_kernel<2>, grid, block, lds, stream, a);
        else hipLaunchKernelGGL(gmm_estep_full_kernel<1>, grid, block, lds, stream, a);
        he = hipGetLastError();
    } else {
        hipLaunchKernelGGL(gmm_estep_diag_kernel, dim3((n + GMM_DR - 1) / GMM_DR, (k + GMM_DC - 1) / GMM_DC), dim3(256), 0, stream, d_x, n, d, k,
                           d_means, d_prec_chol, d_offset, table);
        he = hipGetLastError();
        RA_LAUNCH(he, gmm_finish_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, table, n, k, d_log_resp ? 1 : 0, d_log_prob, d_labels);
    }
    RA_LAUNCH(he, gmm_runsum_kernel, dim3((nr + 255) / 256), dim3(256), 0, stream, (const double *)d_log_prob, n, part);
    RA_LAUNCH(he, gmm_final_kernel, dim3(1), dim3(256), 0, stream, (const double *)part, nr, d_sum);
    return he == hipSuccess ? RA_OK : hip_error("ra_gmm_estep", he);
}

extern "C" int ra_gmm_mstep(const float *d_x, int n, int d, int k, int cov_type, const double *d_resp, int log_domain, double reg_covar,
                            double *d_nk, double *d_means, double *d_cov, void *hip_stream)
{
    if (!gmm_shape_ok("ra_gmm_mstep", n, d, k, cov_type)) return RA_ERR_ARG;
    if (!(reg_covar >= 0.0) || !std::isfinite(reg_covar)) return arg_error("ra_gmm_mstep: need a finite reg_covar >= 0");
    if (!d_x || !d_resp || !d_nk || !d_means || !d_cov) return arg_error("ra_gmm_mstep: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const bool full = cov_type == RA_GMM_FULL;
    const int td = gmm_msum_td(d), cb = gmm_msum_cb(d), ctiles = (k + cb - 1) / cb, dtiles = (d + td - 1) / td;
    const GmmPlan ps = gmm_plan(n, ctiles * dtiles, GMM_MROWS, 2048);
    const int T = gmm_cov_tiles(d), zt = (T + 4 * GMM_CTILES - 1) / (4 * GMM_CTILES);
    const GmmPlan pc = gmm_plan(n, k * zt, GMM_CROWS, 2048);
    const size_t kd = (size_t)k * d;
    StreamScratch scratch(stream);
    double *part_nk = scratch.get<double>((size_t)ps.runs * k);
    double *part_x = scratch.get<double>((size_t)ps.runs * kd);
    double *part_q = full ? nullptr : scratch.get<double>((size_t)ps.runs * kd);
    double *part_c = full ? scratch.get<double>((size_t)pc.runs * k * T * 256) : nullptr;
    if (!part_nk || !part_x || (full ? !part_c : !part_q)) return hip_error("ra_gmm_mstep", scratch.status());
    hipLaunchKernelGGL(gmm_nk_kernel, dim3(ps.runs, (k + 255) / 256), dim3(256), 0, stream, d_resp, n, k, log_domain, ps.len, part_nk);
    hipError_t he = hipGetLastError();
    const dim3 grid(ps.runs, ctiles, dtiles);
    if (td == 64) {
        if (full) RA_LAUNCH(he, (gmm_msum_kernel<64, false>), grid, dim3(256), 0, stream, d_x, n, d, k, d_resp, log_domain, ps.len, part_x, part_q);
        else RA_LAUNCH(he, (gmm_msum_kernel<64, true>), grid, dim3(256), 0, stream, d_x, n, d, k, d_resp, log_domain, ps.len, part_x, part_q);
    } else {
        if (full) RA_LAUNCH(he, (gmm_msum_kernel<256, false>), grid, dim3(256), 0, stream, d_x, n, d, k, d_resp, log_domain, ps.len, part_x, part_q);
        else RA_LAUNCH(he, (gmm_msum_kernel<256, true>), grid, dim3(256), 0, stream, d_x, n, d, k, d_resp, log_domain, ps.len, part_x, part_q);
    }
    RA_LAUNCH(he, gmm_mcombine_kernel, dim3(k), dim3(256), 0, stream, (const double *)part_nk, (const double *)part_x, (const double *)part_q,
              ps.runs, d, k, reg_covar, d_nk, d_means, d_cov);
    if (full) {
        RA_LAUNCH(he, gmm_cov_kernel, dim3(pc.runs, k, zt), dim3(256), 0, stream, d_x, n, d, k, d_resp, log_domain, (const double *)d_means, pc.len,
                  part_c);
        RA_LAUNCH(he, gmm_cov_combine_kernel, dim3(k, T), dim3(256), 0, stream, (const double *)part_c, pc.runs, d, k, (const double *)d_nk,
                  reg_covar, d_cov);
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_gmm_mstep", he);
}
