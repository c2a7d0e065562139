// t-SNE, k-means, cluster validity, DBSCAN, HDBSCAN, Ward agglomeration, embedding quality, spectral embedding and UMAP of 2SDR
// factors (ralign_tsne.h, ralign_kmeans.h, ralign_validity.h, ralign_dbscan.h, ralign_hdbscan.h, ralign_ward.h, ralign_quality.h,
// ralign_spectral.h, ralign_umap.h): the engine-less ra_tsne_*, ra_kmeans_*, ra_dbscan_*, ra_hdbscan_*, ra_ward_*, ra_embed_*,
// ra_spectral_* and ra_umap_* entry points of libralign_hip.so, each on the caller's stream.
#include "ralign_host.h"
#include "ralign_scratch.h"
#include "ralign_kmeans.h"
#include "ralign_validity.h"
#include "ralign_dbscan.h"
#include "ralign_hdbscan.h"
#include "ralign_ward.h"
#include "ralign_quality.h"
#include "ralign_spectral.h"
#include "ralign_umap.h"

using namespace ralign;

// ---- t-SNE (ralign_tsne.h; the neighbour lists: ralign_knn.h)

// the neighbour lists of q [nq][d] among x [m][d] (ralign_knn.h): the plan (C survivors, list capacity, dynamic LDS), the norms
// and the kernel.  self: q == x and nq == m, row i leaves itself out, and the norms are computed once
static int tsne_knn_run(const char *what, bool self, const float *d_q, int nq, const float *d_x, int m, int d, int k, int *d_idx,
                        double *d_dist2, hipStream_t stream)
{
    TsneKnnArgs a;
    a.q = d_q; a.x = d_x; a.nq = nq; a.m = m; a.d = d; a.k = k;
    a.C = std::min(self ? m - 1 : m, k + TSNE_KNN_MARGIN);
    a.cap = a.C + TSNE_KNN_SLACK;
    a.idx = d_idx; a.dist2 = d_dist2;
    const size_t lds = (size_t)16 * a.C * sizeof(double) + (size_t)16 * TSNE_KNN_TILE * sizeof(float) + (size_t)16 * a.cap * 8;
    if (const int rc = self ? RA_LDS(nullptr, tsne_knn_kernel, lds) : RA_LDS(nullptr, tsne_knn_query_kernel, lds)) return rc;
    StreamScratch scratch(stream);
    float *d_nrm = scratch.get<float>(self ? (size_t)m : (size_t)nq + m);
    if (!d_nrm) return hip_error(what, scratch.status());
    a.qnrm = d_nrm; a.xnrm = self ? d_nrm : d_nrm + nq;
    hipLaunchKernelGGL(tsne_sqnorm_kernel, dim3((nq + 255) / 256), dim3(256), 0, stream, d_q, nq, d, d_nrm);
    hipError_t he = hipGetLastError();
    const dim3 grid((nq + 15) / 16), block(TSNE_KNN_THREADS);
    if (self) {
        RA_LAUNCH(he, tsne_knn_kernel, grid, block, lds, stream, a);
    } else {
        RA_LAUNCH(he, tsne_sqnorm_kernel, dim3((m + 255) / 256), dim3(256), 0, stream, d_x, m, d, d_nrm + nq);
        RA_LAUNCH(he, tsne_knn_query_kernel, grid, block, lds, stream, a);
    }
    return he == hipSuccess ? RA_OK : hip_error(what, he);
}

extern "C" int ra_tsne_knn(const float *d_x, int n, int d, int k, int *d_idx, double *d_dist2, void *hip_stream)
{
    if (n < 2 || n > TSNE_MAX_N || d < 1 || d > TSNE_MAX_D || k < 1 || k > std::min(n - 1, TSNE_MAX_K))
        return arg_error("ra_tsne_knn: need 2 <= n <= 262144, 1 <= d <= 2048 and 1 <= k <= min(n - 1, 301)");
    if (!d_x || !d_idx || !d_dist2) return arg_error("ra_tsne_knn: null argument");
    return tsne_knn_run("ra_tsne_knn", true, d_x, n, d_x, n, d, k, d_idx, d_dist2, (hipStream_t)hip_stream);
}

extern "C" int ra_tsne_affinity(const double *d_dist2, int n, int k, float perplexity, double *d_pcond, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 2 || n > TSNE_MAX_N || k < 1 || k > std::min(n - 1, TSNE_MAX_K) || !(perplexity > 0.f && perplexity <= 100.f))
        return arg_error("ra_tsne_affinity: need 2 <= n <= 262144, 1 <= k <= min(n - 1, 301) and 0 < perplexity <= 100");
    if (!d_dist2 || !d_pcond) return arg_error("ra_tsne_affinity: null argument");
    hipLaunchKernelGGL(tsne_affinity_kernel, dim3((n + 3) / 4), dim3(256), 0, stream, d_dist2, n, k, log((double)perplexity), d_pcond);
    hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_tsne_affinity", he);
}

// repulsion partials, then the update kernel in the given mode, then (if d_stats) the statistics
static int tsne_run(const char *what, const float *d_y, float *d_y_out, float *d_update, float *d_gains, float *d_grad, int n,
                    const int *d_indptr, const int *d_indices, const float *d_p, int nnz, float exaggeration, float momentum,
                    float learning_rate, int mode, double *d_stats, hipStream_t stream)
{
    const int seg = tsne_segment(n), nseg = (n + seg - 1) / seg, nrb = (n + TSNE_REP_ROWS - 1) / TSNE_REP_ROWS;
    const int nub = (n + TSNE_UPD_THREADS - 1) / TSNE_UPD_THREADS, nz = nseg * nrb;
    const size_t part_bytes = (size_t)nseg * n * sizeof(float2), z_bytes = (size_t)nz * sizeof(double);
    const size_t st_bytes = d_stats ? (size_t)nub * 2 * sizeof(double) : 0;
    StreamScratch owner(stream);
    unsigned char *scratch = owner.get<unsigned char>(part_bytes + z_bytes + st_bytes);
    if (!scratch) return hip_error(what, owner.status());
    float2 *part = (float2 *)scratch;
    double *zpart = (double *)(scratch + part_bytes), *st = d_stats ? (double *)(scratch + part_bytes + z_bytes) : nullptr;
    hipLaunchKernelGGL(tsne_repulsion_kernel, dim3(nrb, nseg), dim3(TSNE_REP_THREADS), 0, stream, (const float2 *)d_y, n, seg, part, zpart);
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) {
        TsneUpdateArgs u;
        u.y = (const float2 *)d_y; u.y_out = (float2 *)d_y_out; u.update = (float2 *)d_update; u.gains = (float2 *)d_gains;
        u.grad = (float2 *)d_grad; u.part = part; u.zpart = zpart; u.indptr = d_indptr; u.indices = d_indices; u.p = d_p;
        u.n = n; u.nseg = nseg; u.nz = nz; u.nnz = nnz; u.mode = mode;
        u.exaggeration = exaggeration; u.momentum = momentum; u.learning_rate = learning_rate; u.stats_part = st;
        hipLaunchKernelGGL(tsne_update_kernel, dim3(nub), dim3(TSNE_UPD_THREADS), 0, stream, u);
        he = hipGetLastError();
    }
    if (d_stats) RA_LAUNCH(he, tsne_stats_kernel, dim3(1), dim3(256), 0, stream, st, nub, d_stats);
    return he == hipSuccess ? RA_OK : hip_error(what, he);
}

static bool tsne_csr_ok(const char *what, int n, int nnz, const int *d_indptr, const int *d_indices, const float *d_p)
{
    if (n < 2 || n > TSNE_MAX_N || nnz < 0 || (long long)nnz > 2LL * n * TSNE_MAX_K) {
        set_error(std::string(what) + ": need 2 <= n <= 262144 and 0 <= nnz <= 2 n 301");
        return false;
    }
    if (!d_indptr || (nnz > 0 && (!d_indices || !d_p))) { set_error(std::string(what) + ": null argument"); return false; }
    return true;
}

extern "C" int ra_tsne_step(const float *d_y, float *d_y_out, float *d_update, float *d_gains, int n, const int *d_indptr,
                            const int *d_indices, const float *d_p, int nnz, float exaggeration, float momentum, float learning_rate,
                            double *d_stats, void *hip_stream)
{
    if (!tsne_csr_ok("ra_tsne_step", n, nnz, d_indptr, d_indices, d_p)) return RA_ERR_ARG;
    if (!d_y || !d_y_out || !d_update || !d_gains || d_y_out == d_y)
        return arg_error("ra_tsne_step: null argument, or d_y_out == d_y (the step reads every y_j while it writes)");
    if (!std::isfinite(exaggeration) || !std::isfinite(momentum) || !std::isfinite(learning_rate) || !(learning_rate > 0.f))
        return arg_error("ra_tsne_step: need finite exaggeration and momentum and a finite learning rate > 0");
    return tsne_run("ra_tsne_step", d_y, d_y_out, d_update, d_gains, nullptr, n, d_indptr, d_indices, d_p, nnz, exaggeration, momentum,
                    learning_rate, 0, d_stats, (hipStream_t)hip_stream);
}

extern "C" int ra_tsne_error(const float *d_y, int n, const int *d_indptr, const int *d_indices, const float *d_p, int nnz,
                             float exaggeration, float *d_grad, double *d_stats, void *hip_stream)
{
    if (!tsne_csr_ok("ra_tsne_error", n, nnz, d_indptr, d_indices, d_p)) return RA_ERR_ARG;
    if (!d_y || (!d_grad && !d_stats) || !std::isfinite(exaggeration))
        return arg_error("ra_tsne_error: null embedding, neither gradient nor statistics asked for, or a non-finite exaggeration");
    return tsne_run("ra_tsne_error", d_y, nullptr, nullptr, nullptr, d_grad, n, d_indptr, d_indices, d_p, nnz, exaggeration, 0.f, 0.f, 1,
                    d_stats, (hipStream_t)hip_stream);
}

// ---- t-SNE, out-of-sample placement (ralign_tsne.h)

extern "C" int ra_tsne_knn_query(const float *d_q, int nq, const float *d_x, int m, int d, int k, int *d_idx, double *d_dist2,
                                 void *hip_stream)
{
    if (nq < 1 || nq > TSNE_MAX_NQ || m < 1 || m > TSNE_MAX_N || d < 1 || d > TSNE_MAX_D || k < 1 || k > std::min(m, TSNE_MAX_K))
        return arg_error("ra_tsne_knn_query: need 1 <= nq <= 4194304, 1 <= m <= 262144, 1 <= d <= 2048 and 1 <= k <= min(m, 301)");
    if (!d_q || !d_x || !d_idx || !d_dist2) return arg_error("ra_tsne_knn_query: null argument");
    return tsne_knn_run("ra_tsne_knn_query", false, d_q, nq, d_x, m, d, k, d_idx, d_dist2, (hipStream_t)hip_stream);
}

extern "C" int ra_tsne_affinity_rows(const double *d_dist2, int rows, int k, float perplexity, double *d_pcond, void *hip_stream)
{
    if (rows < 1 || rows > TSNE_MAX_NQ || k < 1 || k > TSNE_MAX_K || !(perplexity > 0.f && perplexity <= 100.f))
        return arg_error("ra_tsne_affinity_rows: need 1 <= rows <= 4194304, 1 <= k <= 301 and 0 < perplexity <= 100");
    if (!d_dist2 || !d_pcond) return arg_error("ra_tsne_affinity_rows: null argument");
    hipLaunchKernelGGL(tsne_affinity_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)hip_stream, d_dist2, rows, k,
                       log((double)perplexity), d_pcond);
    hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_tsne_affinity_rows", he);
}

static bool tsne_place_ok(const char *what, const float *d_y, int n, const float *d_yfit, int m, const int *d_idx, const float *d_p,
                          int k, float exaggeration)
{
    if (n < 1 || n > TSNE_MAX_NQ || m < 1 || m > TSNE_MAX_N || k < 1 || k > std::min(m, TSNE_MAX_K) || !std::isfinite(exaggeration) ||
        !(exaggeration >= 1.f)) {
        set_error(std::string(what) + ": need 1 <= n <= 4194304, 1 <= m <= 262144, 1 <= k <= min(m, 301) and a finite exaggeration >= 1");
        return false;
    }
    if (!d_y || !d_yfit || !d_idx || !d_p) { set_error(std::string(what) + ": null argument"); return false; }
    return true;
}

static int tsne_place_run(const char *what, float *d_y, int n, const float *d_yfit, int m, const int *d_idx, const float *d_p, int k,
                          float exaggeration, float momentum, float learning_rate, int n_iter, float *d_grad, double *d_kl,
                          double *d_z, hipStream_t stream)
{
    TsnePlaceArgs a;
    a.y = (float2 *)d_y; a.yfit = (const float2 *)d_yfit; a.idx = d_idx; a.p = d_p; a.n = n; a.m = m; a.k = k; a.n_iter = n_iter;
    a.exaggeration = exaggeration; a.momentum = momentum; a.learning_rate = learning_rate;
    a.grad = (float2 *)d_grad; a.kl = d_kl; a.z = d_z;
    hipLaunchKernelGGL(tsne_place_kernel, dim3((n + TSNE_PLACE_ROWS - 1) / TSNE_PLACE_ROWS), dim3(TSNE_PLACE_THREADS), 0, stream, a);
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error(what, he);
}

extern "C" int ra_tsne_place_gradient(const float *d_y, int n, const float *d_yfit, int m, const int *d_idx, const float *d_p, int k,
                                      float exaggeration, float *d_grad, double *d_kl, double *d_z, void *hip_stream)
{
    if (!tsne_place_ok("ra_tsne_place_gradient", d_y, n, d_yfit, m, d_idx, d_p, k, exaggeration)) return RA_ERR_ARG;
    if (!d_grad && !d_kl && !d_z) return arg_error("ra_tsne_place_gradient: none of gradient, KL and Z asked for");
    // n_iter = 0: the kernel reads d_y and writes the outputs only
    return tsne_place_run("ra_tsne_place_gradient", const_cast<float *>(d_y), n, d_yfit, m, d_idx, d_p, k, exaggeration, 0.f, 0.f, 0,
                          d_grad, d_kl, d_z, (hipStream_t)hip_stream);
}

extern "C" int ra_tsne_place(float *d_y, int n, const float *d_yfit, int m, const int *d_idx, const float *d_p, int k,
                             float exaggeration, float momentum, float learning_rate, int n_iter, double *d_kl, void *hip_stream)
{
    if (!tsne_place_ok("ra_tsne_place", d_y, n, d_yfit, m, d_idx, d_p, k, exaggeration)) return RA_ERR_ARG;
    if (n_iter < 0 || !(momentum >= 0.f && momentum < 1.f) || !std::isfinite(learning_rate) || !(learning_rate > 0.f))
        return arg_error("ra_tsne_place: need n_iter >= 0, 0 <= momentum < 1 and a finite learning rate > 0");
    if (n_iter == 0 && !d_kl) return RA_OK;
    return tsne_place_run("ra_tsne_place", d_y, n, d_yfit, m, d_idx, d_p, k, exaggeration, momentum, learning_rate, n_iter, nullptr,
                          d_kl, nullptr, (hipStream_t)hip_stream);
}

// ---- k-means (ralign_kmeans.h)

static bool km_shape_ok(const char *what, int n, int d, int k)
{
    if (n < 1 || n > KM_MAX_N || d < 1 || d > KM_MAX_D || k < 1 || k > std::min(n, KM_MAX_K)) {
        set_error(std::string(what) + ": need 1 <= n <= 4194304, 1 <= d <= 2048 and 1 <= k <= min(n, 256)");
        return false;
    }
    return true;
}

// the stable member lists of the labels: count [k], start [k], run0 [k + 1] (runs of L members), members [n]
static hipError_t km_member_lists(const int *labels, int n, int k, int L, const KmLists &M, hipStream_t stream)
{
    const int nb = (n + KM_BLOCK - 1) / KM_BLOCK;
    int *bcnt = M.bcnt(), *cnt = M.cnt(), *start = M.start();
    hipLaunchKernelGGL(km_hist_kernel, dim3(nb), dim3(KM_BLOCK), 0, stream, labels, n, k, bcnt);
    hipError_t he = hipGetLastError();
    RA_LAUNCH(he, km_offsets_kernel, dim3(k), dim3(256), 0, stream, bcnt, nb, k, cnt);
    RA_LAUNCH(he, km_starts_kernel, dim3(1), dim3(64), 0, stream, (const int *)cnt, k, L, start, M.run0());
    RA_LAUNCH(he, km_scatter_kernel, dim3(nb), dim3(KM_BLOCK), 0, stream, labels, n, k, (const int *)bcnt, (const int *)start, M.mem());
    return he;
}

// the padded column lists of the labels (val_pstart_kernel pads to VAL_TC = DBS_TC): cols is -1 wherever no member lands
static hipError_t km_column_lists(const int *labels, int n, int k, const KmColumns &Cl, hipStream_t stream)
{
    const KmLists &M = Cl.M;
    hipError_t he = hipMemsetAsync(Cl.cols(), 0xff, (size_t)Cl.cap * 4, stream);
    if (he == hipSuccess) he = km_member_lists(labels, n, k, km_run_len(n), M, stream);
    RA_LAUNCH(he, val_pstart_kernel, dim3(1), dim3(64), 0, stream, (const int *)M.cnt(), k, Cl.pstart());
    RA_LAUNCH(he, val_cols_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, (const int *)M.mem(), (const int *)M.start(),
              (const int *)M.cnt(), (const int *)Cl.pstart(), n, k, Cl.cap, Cl.cols());
    return he;
}

// the squared norms the MFMA E-step reads (d > KM_SMALL_D): the caller's, or computed into the scratch piece `own`
static hipError_t km_norms(const float *x, int n, int d, const float *&nrm, float *own, hipStream_t stream)
{
    if (nrm || d <= KM_SMALL_D) return hipSuccess;
    nrm = own;
    hipLaunchKernelGGL(tsne_sqnorm_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, x, n, d, own);
    return hipGetLastError();
}

extern "C" int ra_kmeans_sqnorm(const float *d_x, int n, int d, float *d_nrm, void *hip_stream)
{
    if (!km_shape_ok("ra_kmeans_sqnorm", n, d, 1)) return RA_ERR_ARG;
    if (!d_x || !d_nrm) return arg_error("ra_kmeans_sqnorm: null argument");
    hipLaunchKernelGGL(tsne_sqnorm_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)hip_stream, d_x, n, d, d_nrm);
    hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_kmeans_sqnorm", he);
}

// the E-step: labels (in place, changed counted into d_changed if non-null) and the double distance of each point to its centre.
// cf [k][d] / cnrm [k]: scratch of the f32 copy (d > KM_SMALL_D only)
static hipError_t km_assign(const float *x, int n, int d, const float *nrm, const double *c, int k, int *labels, double *dist,
                            int *changed, float *cf, float *cnrm, hipStream_t stream)
{
    if (d <= KM_SMALL_D) {
        hipLaunchKernelGGL(km_assign_small_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, x, n, d, c, k, labels, dist, changed);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(km_prep_kernel, dim3(k), dim3(256), 0, stream, c, d, cf, cnrm);
    hipError_t he = hipGetLastError();
    if (he != hipSuccess) return he;
    KmAssignArgs a;
    a.x = x; a.nrm = nrm; a.c = c; a.cf = cf; a.cnrm = cnrm; a.n = n; a.d = d; a.k = k;
    a.labels = labels; a.dist = dist; a.changed = changed;
    const dim3 grid((n + KM_ROWS - 1) / KM_ROWS), block(64 * KM_WAVES);
    const int nt = (k + 15) / 16;
    if (nt <= 1) hipLaunchKernelGGL(km_assign_mfma_kernel<1>, grid, block, 0, stream, a);
    else if (nt <= 2) hipLaunchKernelGGL(km_assign_mfma_kernel<2>, grid, block, 0, stream, a);
    else if (nt <= 4) hipLaunchKernelGGL(km_assign_mfma_kernel<4>, grid, block, 0, stream, a);
    else if (nt <= 8) hipLaunchKernelGGL(km_assign_mfma_kernel<8>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(km_assign_mfma_kernel<16>, grid, block, 0, stream, a);
    return hipGetLastError();
}

extern "C" int ra_kmeans_labels(const float *d_x, int n, int d, const float *d_nrm, const double *d_centers, int k, int *d_labels,
                                int assign, double *d_inertia, void *hip_stream)
{
    if (!km_shape_ok("ra_kmeans_labels", n, d, k)) return RA_ERR_ARG;
    if (!d_x || !d_centers || !d_labels || (!assign && !d_inertia))
        return arg_error("ra_kmeans_labels: null argument, or neither assignment nor inertia asked for");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nb = (n + 255) / 256;
    KmScratch S;
    const size_t o_dist = S.take((size_t)n * 8), o_part = S.take((size_t)nb * 8);
    const bool big = d > KM_SMALL_D;
    const size_t o_cf = S.take(big ? (size_t)k * d * 4 : 0), o_cn = S.take(big ? (size_t)k * 4 : 0);
    const size_t o_nrm = S.take(big && !d_nrm ? (size_t)n * 4 : 0);
    StreamScratch scratch(stream);
    if (!(S.base = scratch.get<unsigned char>(S.off))) return hip_error("ra_kmeans_labels", scratch.status());
    double *dist = S.at<double>(o_dist);
    const float *nrm = d_nrm;
    hipError_t he = km_norms(d_x, n, d, nrm, S.at<float>(o_nrm), stream);
    if (he == hipSuccess) {
        if (assign) {
            he = km_assign(d_x, n, d, nrm, d_centers, k, d_labels, dist, nullptr, S.at<float>(o_cf), S.at<float>(o_cn), stream);
        } else {
            hipLaunchKernelGGL(km_point_dist_kernel, dim3(big ? (n + 3) / 4 : nb), dim3(256), 0, stream, d_x, n, d, d_centers, k, d_labels, dist);
            he = hipGetLastError();
        }
    }
    if (he == hipSuccess && d_inertia) {
        hipLaunchKernelGGL(km_block_sum_kernel, dim3(nb), dim3(256), 0, stream, dist, n, S.at<double>(o_part));
        he = hipGetLastError();
        RA_LAUNCH(he, km_final_sum_kernel, dim3(1), dim3(256), 0, stream, S.at<double>(o_part), nb, d_inertia);
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_kmeans_labels", he);
}

extern "C" int ra_kmeans_lloyd(const float *d_x, int n, int d, const float *d_nrm, const double *d_centers, int k, double *d_centers_new,
                               int *d_labels, double *d_stats, void *hip_stream)
{
    if (!km_shape_ok("ra_kmeans_lloyd", n, d, k)) return RA_ERR_ARG;
    if (!d_x || !d_centers || !d_centers_new || !d_labels || !d_stats || d_centers_new == d_centers)
        return arg_error("ra_kmeans_lloyd: null argument, or d_centers_new == d_centers");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int L = km_run_len(n), rmax = (n + L - 1) / L + k;
    const bool big = d > KM_SMALL_D;
    KmScratch S;
    const KmLists M(S, n, k, KM_BLOCK);
    const size_t o_dist = S.take((size_t)n * 8), o_ints = S.take(2 * 4), o_part = S.take((size_t)rmax * d * 8);
    const size_t o_sums = S.take((size_t)k * d * 8), o_wt = S.take((size_t)k * 8), o_shift = S.take((size_t)k * 8);
    const size_t o_cf = S.take(big ? (size_t)k * d * 4 : 0), o_cn = S.take(big ? (size_t)k * 4 : 0);
    const size_t o_nrm = S.take(big && !d_nrm ? (size_t)n * 4 : 0);
    StreamScratch scratch(stream);
    if (!(S.base = scratch.get<unsigned char>(S.off))) return hip_error("ra_kmeans_lloyd", scratch.status());
    int *ints = S.at<int>(o_ints), *cnt = M.cnt(), *start = M.start(), *run0 = M.run0(), *mem = M.mem();
    double *dist = S.at<double>(o_dist), *part = S.at<double>(o_part), *sums = S.at<double>(o_sums), *wt = S.at<double>(o_wt);
    double *shift = S.at<double>(o_shift);
    const float *nrm = d_nrm;
    hipError_t he = hipMemsetAsync(ints, 0, 2 * sizeof(int), stream);
    if (he == hipSuccess) he = km_norms(d_x, n, d, nrm, S.at<float>(o_nrm), stream);
    if (he == hipSuccess) he = km_assign(d_x, n, d, nrm, d_centers, k, d_labels, dist, ints, S.at<float>(o_cf), S.at<float>(o_cn), stream);
    if (he == hipSuccess) he = km_member_lists(d_labels, n, k, L, M, stream);
    RA_LAUNCH(he, km_runsum_kernel, dim3(rmax), dim3(256), 0, stream, d_x, n, d, k, L, (const int *)mem, (const int *)cnt, (const int *)start,
                  (const int *)run0, part);
    RA_LAUNCH(he, km_combine_kernel, dim3(k), dim3(256), 0, stream, (const double *)part, d, (const int *)cnt, (const int *)run0, sums, wt);
    RA_LAUNCH(he, km_relocate_kernel, dim3(1), dim3(1024), 0, stream, d_x, n, d, k, (const int *)d_labels, (const double *)dist, (const int *)cnt,
                  sums, wt, ints + 1);
    RA_LAUNCH(he, km_update_kernel, dim3(k), dim3(256), 0, stream, (const double *)sums, (const double *)wt, d_centers, d, k, d_centers_new, shift);
    RA_LAUNCH(he, km_stats_kernel, dim3(1), dim3(256), 0, stream, (const double *)shift, k, (const int *)ints, d_stats);
    return he == hipSuccess ? RA_OK : hip_error("ra_kmeans_lloyd", he);
}

extern "C" int ra_kmeans_search(const double *d_w, int n, const double *d_vals, int m, int *d_idx, void *hip_stream)
{
    if (n < 1 || n > KM_MAX_N || m < 1 || m > KM_MAX_M) return arg_error("ra_kmeans_search: need 1 <= n <= 4194304 and 1 <= m <= 16");
    if (!d_w || !d_vals || !d_idx) return arg_error("ra_kmeans_search: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nseg = (n + KM_SEG - 1) / KM_SEG;
    StreamScratch scratch(stream);
    double *buf = scratch.get<double>((size_t)3 * nseg);
    if (!buf) return hip_error("ra_kmeans_search", scratch.status());
    double *segsum = buf, *base = buf + nseg, *end = buf + 2 * nseg;
    hipLaunchKernelGGL(km_segsum_kernel, dim3((nseg + 255) / 256), dim3(256), 0, stream, d_w, n, segsum);
    hipError_t he = hipGetLastError();
    RA_LAUNCH(he, km_segscan_kernel, dim3(1), dim3(256), 0, stream, (const double *)segsum, nseg, base, end);
    RA_LAUNCH(he, km_search_kernel, dim3(m), dim3(256), 0, stream, d_w, n, (const double *)base, (const double *)end, nseg, d_vals, d_idx);
    return he == hipSuccess ? RA_OK : hip_error("ra_kmeans_search", he);
}

extern "C" int ra_kmeans_seed(const float *d_x, int n, int d, const int *d_cand, int m, double *d_closest, int first, double *d_out,
                              void *hip_stream)
{
    if (!km_shape_ok("ra_kmeans_seed", n, d, 1)) return RA_ERR_ARG;
    if (m < 1 || m > KM_MAX_M || (first && m != 1)) return arg_error("ra_kmeans_seed: need 1 <= m <= 16 candidates (first centre: m = 1)");
    if (!d_x || !d_cand || !d_closest || !d_out) return arg_error("ra_kmeans_seed: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nb = (n + 255) / 256;
    StreamScratch scratch(stream);
    double *part = scratch.get<double>((size_t)m * nb);
    if (!part) return hip_error("ra_kmeans_seed", scratch.status());
    hipLaunchKernelGGL(km_cand_dist_kernel, dim3(nb, m), dim3(256), 0, stream, d_x, n, d, d_cand, first ? (const double *)nullptr : d_closest, part);
    hipError_t he = hipGetLastError();
    RA_LAUNCH(he, km_pick_kernel, dim3(1), dim3(256), 0, stream, (const double *)part, nb, d_cand, m, n, d_out);
    RA_LAUNCH(he, km_commit_kernel, dim3(nb), dim3(256), 0, stream, d_x, n, d, (const double *)d_out, first, d_closest);
    return he == hipSuccess ? RA_OK : hip_error("ra_kmeans_seed", he);
}

// ---- cluster validity (ralign_validity.h)

extern "C" int ra_kmeans_silhouette(const float *d_x, int n, int d, const int *d_labels, int k, double *d_out, int *d_nearest, void *hip_stream)
{
    if (n < 3 || n > VAL_MAX_N || d < 1 || d > KM_MAX_D || k < 2 || k > KM_MAX_K)
        return arg_error("ra_kmeans_silhouette: need 3 <= n <= 262144, 1 <= d <= 2048 and 2 <= k <= 256");
    if (!d_x || !d_labels || !d_out || !d_nearest) return arg_error("ra_kmeans_silhouette: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    KmScratch S;
    const KmColumns Cl(S, n, k, KM_BLOCK, VAL_TC);
    StreamScratch scratch(stream);
    if (!(S.base = scratch.get<unsigned char>(S.off))) return hip_error("ra_kmeans_silhouette", scratch.status());
    hipError_t he = km_column_lists(d_labels, n, k, Cl, stream);
    ValSilArgs a;
    a.x = d_x; a.labels = d_labels; a.cols = Cl.cols(); a.count = Cl.M.cnt(); a.pstart = Cl.pstart(); a.n = n; a.d = d; a.k = k;
    a.out = d_out; a.nearest = d_nearest;
    RA_LAUNCH(he, val_silhouette_kernel, dim3((n + VAL_TR - 1) / VAL_TR), dim3(256), 0, stream, a);
    return he == hipSuccess ? RA_OK : hip_error("ra_kmeans_silhouette", he);
}

extern "C" int ra_kmeans_dispersion(const float *d_x, int n, int d, const int *d_labels, int k, double *d_centroids, int *d_counts, double *d_sq,
                                    double *d_abs, void *hip_stream)
{
    if (n < 1 || n > KM_MAX_N || d < 1 || d > KM_MAX_D || k < 1 || k > KM_MAX_K)
        return arg_error("ra_kmeans_dispersion: need 1 <= n <= 4194304, 1 <= d <= 2048 and 1 <= k <= 256");
    if (!d_x || !d_labels || !d_centroids || !d_counts || !d_sq || !d_abs) return arg_error("ra_kmeans_dispersion: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int L = km_run_len(n), rmax = (n + L - 1) / L + k;
    KmScratch S;
    const KmLists M(S, n, k, KM_BLOCK);
    const size_t o_part = S.take((size_t)rmax * d * 8), o_sums = S.take((size_t)k * d * 8), o_wt = S.take((size_t)k * 8);
    const size_t o_dist = S.take((size_t)n * 8);
    StreamScratch scratch(stream);
    if (!(S.base = scratch.get<unsigned char>(S.off))) return hip_error("ra_kmeans_dispersion", scratch.status());
    int *cnt = M.cnt(), *start = M.start(), *run0 = M.run0(), *mem = M.mem();
    double *part = S.at<double>(o_part), *sums = S.at<double>(o_sums), *dist = S.at<double>(o_dist);
    hipError_t he = km_member_lists(d_labels, n, k, L, M, stream);
    RA_LAUNCH(he, km_runsum_kernel, dim3(rmax), dim3(256), 0, stream, d_x, n, d, k, L, (const int *)mem, (const int *)cnt, (const int *)start,
              (const int *)run0, part);
    RA_LAUNCH(he, km_combine_kernel, dim3(k), dim3(256), 0, stream, (const double *)part, d, (const int *)cnt, (const int *)run0, sums,
              S.at<double>(o_wt));
    RA_LAUNCH(he, val_centroid_kernel, dim3(k), dim3(256), 0, stream, (const double *)sums, (const int *)cnt, d, d_centroids, d_counts);
    RA_LAUNCH(he, km_point_dist_kernel, dim3(d > KM_SMALL_D ? (n + 3) / 4 : (n + 255) / 256), dim3(256), 0, stream, d_x, n, d,
              (const double *)d_centroids, k, d_labels, dist);
    RA_LAUNCH(he, val_disp_kernel, dim3(k), dim3(256), 0, stream, (const double *)dist, (const int *)mem, (const int *)cnt, (const int *)start, n,
              d_sq, d_abs);
    return he == hipSuccess ? RA_OK : hip_error("ra_kmeans_dispersion", he);
}

// ---- DBSCAN (ralign_dbscan.h)

static bool dbs_domain_ok(const char *what, int n, int d, double eps, int min_samples)
{
    if (n < 1 || n > DBS_MAX_N || d < 1 || d > DBS_MAX_D || !std::isfinite(eps) || !(eps > 0.0) || min_samples < 1) {
        set_error(std::string(what) + ": need 1 <= n <= 262144, 1 <= d <= 2048, a finite eps > 0 and min_samples >= 1");
        return false;
    }
    return true;
}

extern "C" int ra_dbscan_count(const float *d_x, int n, int d, double eps, int min_samples, int *d_count, int *d_label, void *hip_stream)
{
    if (!dbs_domain_ok("ra_dbscan_count", n, d, eps, min_samples)) return RA_ERR_ARG;
    if (!d_x || !d_count || !d_label) return arg_error("ra_dbscan_count: null argument");
    hipLaunchKernelGGL(dbs_count_kernel, dim3((n + DBS_TR - 1) / DBS_TR), dim3(256), 0, (hipStream_t)hip_stream, d_x, n, d, eps * eps,
                       min_samples, d_count, d_label);
    hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_dbscan_count", he);
}

extern "C" int ra_dbscan_step(const float *d_x, int n, int d, double eps, const int *d_count, int min_samples, const int *d_label,
                              int *d_label_out, int *d_changed, void *hip_stream)
{
    if (!dbs_domain_ok("ra_dbscan_step", n, d, eps, min_samples)) return RA_ERR_ARG;
    if (!d_x || !d_count || !d_label || !d_label_out || !d_changed || d_label_out == d_label)
        return arg_error("ra_dbscan_step: null argument, or d_label_out == d_label");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nt = (n + 255) / 256;
    KmScratch S;
    const KmColumns Cl(S, n, 2, KM_BLOCK, DBS_TC);
    const size_t o_flag = S.take((size_t)n * 4), o_m = S.take((size_t)n * 4), o_p = S.take((size_t)n * 4);
    StreamScratch scratch(stream);
    if (!(S.base = scratch.get<unsigned char>(S.off))) return hip_error("ra_dbscan_step", scratch.status());
    int *flag = S.at<int>(o_flag), *m = S.at<int>(o_m), *P = S.at<int>(o_p);
    // the core points in index order: the column list of "cluster" 0 of the flags
    hipError_t he = hipMemsetAsync(d_changed, 0, sizeof(int), stream);
    RA_LAUNCH(he, dbs_flag_kernel, dim3(nt), dim3(256), 0, stream, d_count, n, min_samples, flag);
    if (he == hipSuccess) he = km_column_lists(flag, n, 2, Cl, stream);
    RA_LAUNCH(he, dbs_min_kernel, dim3((n + DBS_TR - 1) / DBS_TR), dim3(256), 0, stream, d_x, n, d, eps * eps, (const int *)Cl.cols(),
              (const int *)Cl.pstart(), d_label, m);
    if (he == hipSuccess) he = hipMemcpyAsync(P, d_label, (size_t)n * 4, hipMemcpyDeviceToDevice, stream);
    RA_LAUNCH(he, dbs_hook_kernel, dim3(nt), dim3(256), 0, stream, d_count, n, min_samples, d_label, (const int *)m, P);
    RA_LAUNCH(he, dbs_compress_kernel, dim3(nt), dim3(256), 0, stream, d_count, n, min_samples, d_label, (const int *)m, (const int *)P,
              d_label_out, d_changed);
    return he == hipSuccess ? RA_OK : hip_error("ra_dbscan_step", he);
}

// ---- HDBSCAN (ralign_hdbscan.h)

static bool hdb_shape_ok(const char *what, int n, int d)
{
    if (n < 2 || n > HDB_MAX_N || d < 1 || d > HDB_MAX_D) {
        set_error(std::string(what) + ": need 2 <= n <= 262144 and 1 <= d <= 2048");
        return false;
    }
    return true;
}

extern "C" int ra_hdbscan_core(const float *d_x, int n, int d, int min_samples, double *d_core2, void *hip_stream)
{
    if (!hdb_shape_ok("ra_hdbscan_core", n, d)) return RA_ERR_ARG;
    if (min_samples < 1 || min_samples > std::min(n, HDB_MAX_MIN_SAMPLES))
        return arg_error("ra_hdbscan_core: need 1 <= min_samples <= min(n, 302)");
    if (!d_x || !d_core2) return arg_error("ra_hdbscan_core: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int k = min_samples - 1;
    if (k == 0) {
        const hipError_t he = hipMemsetAsync(d_core2, 0, (size_t)n * sizeof(double), stream);
        return he == hipSuccess ? RA_OK : hip_error("ra_hdbscan_core", he);
    }
    StreamScratch scratch(stream);
    int *idx = scratch.get<int>((size_t)n * k);
    double *dist2 = scratch.get<double>((size_t)n * k);
    if (!idx || !dist2) return hip_error("ra_hdbscan_core", scratch.status());
    if (const int rc = ra_tsne_knn(d_x, n, d, k, idx, dist2, hip_stream)) return rc;
    // the neighbour comes from the list; the stored value is rule 2's chain to it, not the list's distance
    hipLaunchKernelGGL(hdb_core_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_x, n, d, (const int *)idx, k, d_core2);
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_hdbscan_core", he);
}

extern "C" int ra_hdbscan_round(const float *d_x, int n, int d, const double *d_core2, const int *d_comp, double *d_w2, int *d_lo, int *d_hi,
                                void *hip_stream)
{
    if (!hdb_shape_ok("ra_hdbscan_round", n, d)) return RA_ERR_ARG;
    if (!d_x || !d_core2 || !d_comp || !d_w2 || !d_lo || !d_hi) return arg_error("ra_hdbscan_round: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nt = (n + 255) / 256;
    StreamScratch scratch(stream);
    unsigned long long *buf = scratch.get<unsigned long long>((size_t)4 * n);
    if (!buf) return hip_error("ra_hdbscan_round", scratch.status());
    unsigned long long *roww = buf, *rowe = buf + n, *cw = buf + 2 * (size_t)n, *ce = buf + 3 * (size_t)n;
    hipError_t he = hipMemsetAsync(cw, 0xff, (size_t)2 * n * sizeof(unsigned long long), stream);       // HDB_NONE
    RA_LAUNCH(he, hdb_row_kernel, dim3((n + DBS_TR - 1) / DBS_TR), dim3(256), 0, stream, d_x, n, d, d_core2, d_comp, roww, rowe);
    RA_LAUNCH(he, hdb_minw_kernel, dim3(nt), dim3(256), 0, stream, d_comp, n, (const unsigned long long *)roww, cw);
    RA_LAUNCH(he, hdb_mine_kernel, dim3(nt), dim3(256), 0, stream, d_comp, n, (const unsigned long long *)roww,
              (const unsigned long long *)rowe, (const unsigned long long *)cw, ce);
    RA_LAUNCH(he, hdb_out_kernel, dim3(nt), dim3(256), 0, stream, d_comp, n, (const unsigned long long *)cw, (const unsigned long long *)ce,
              d_w2, d_lo, d_hi);
    return he == hipSuccess ? RA_OK : hip_error("ra_hdbscan_round", he);
}

// ---- Ward agglomeration (ralign_ward.h)

static bool ward_shape_ok(const char *what, int n, int d)
{
    if (n < 2 || n > WARD_MAX_N || d < 1 || d > WARD_MAX_D) {
        set_error(std::string(what) + ": need 2 <= n <= 262144 and 1 <= d <= 2048");
        return false;
    }
    return true;
}

extern "C" int ra_ward_nearest(const double *d_c, const int *d_size, int n, int d, const int *d_rows, int n_rows, int *d_nn, double *d_w2,
                               void *hip_stream)
{
    if (!ward_shape_ok("ra_ward_nearest", n, d)) return RA_ERR_ARG;
    if (n_rows < 1 || n_rows > WARD_MAX_N) return arg_error("ra_ward_nearest: need 1 <= n_rows <= 262144");
    if (!d_c || !d_size || !d_rows || !d_nn || !d_w2) return arg_error("ra_ward_nearest: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    KmScratch S;
    const KmColumns Cl(S, n, 2, KM_BLOCK, DBS_TC);
    const size_t o_flag = S.take((size_t)n * 4);
    StreamScratch scratch(stream);
    if (!(S.base = scratch.get<unsigned char>(S.off))) return hip_error("ra_ward_nearest", scratch.status());
    int *flag = S.at<int>(o_flag);
    // the live slots in slot order: the column list of "cluster" 0 of the flags (size >= 1)
    hipLaunchKernelGGL(dbs_flag_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, d_size, n, 1, flag);
    hipError_t he = hipGetLastError();
    if (he == hipSuccess) he = km_column_lists(flag, n, 2, Cl, stream);
    RA_LAUNCH(he, ward_row_kernel, dim3((n_rows + WARD_TR - 1) / WARD_TR), dim3(256), 0, stream, d_c, d_size, n, d, d_rows, n_rows,
              (const int *)Cl.cols(), (const int *)Cl.pstart(), d_nn, d_w2);
    return he == hipSuccess ? RA_OK : hip_error("ra_ward_nearest", he);
}

extern "C" int ra_ward_merge(double *d_c, int *d_size, int n, int d, const int *d_a, const int *d_b, int n_pairs, void *hip_stream)
{
    if (!ward_shape_ok("ra_ward_merge", n, d)) return RA_ERR_ARG;
    if (n_pairs < 1 || n_pairs > n / 2) return arg_error("ra_ward_merge: need 1 <= n_pairs <= n / 2 disjoint pairs");
    if (!d_c || !d_size || !d_a || !d_b) return arg_error("ra_ward_merge: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const size_t work = (size_t)n_pairs * d;
    hipLaunchKernelGGL(ward_merge_kernel, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, stream, d_c, (const int *)d_size, n, d, d_a, d_b,
                       n_pairs);
    hipError_t he = hipGetLastError();
    // the sizes change in a launch of their own: every thread of ward_merge_kernel has read them by then
    RA_LAUNCH(he, ward_size_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, stream, d_size, n, d_a, d_b, n_pairs);
    return he == hipSuccess ? RA_OK : hip_error("ra_ward_merge", he);
}

// ---- embedding quality (ralign_quality.h)

extern "C" int ra_embed_ranks(const float *d_x, int n, int d, const int *d_idx, int k, int *d_rank, long long *d_pen, void *hip_stream)
{
    if (n < 2 || n > EMB_MAX_N || d < 1 || d > EMB_MAX_D || k < 1 || k > EMB_MAX_K)
        return arg_error("ra_embed_ranks: need 2 <= n <= 262144, 1 <= d <= 2048 and 1 <= k <= 301");
    if (!d_x || !d_idx || (!d_rank && !d_pen)) return arg_error("ra_embed_ranks: null argument, or neither ranks nor penalties asked for");
    hipStream_t stream = (hipStream_t)hip_stream;
    EmbRankArgs a;
    a.x = d_x; a.idx = d_idx; a.n = n; a.d = d; a.k = k; a.kc = std::min(k, EMB_KC);
    a.rank = d_rank; a.pen = d_pen;
    const size_t lds = emb_rank_lds(a.kc);
    if (const int rc = RA_LDS(nullptr, emb_rank_kernel, lds)) return rc;
    StreamScratch scratch(stream);
    double *thr = scratch.get<double>((size_t)n * k);
    if (!thr) return hip_error("ra_embed_ranks", scratch.status());
    a.thr = thr;
    hipLaunchKernelGGL(emb_thr_kernel, dim3((unsigned)(((size_t)n * k + 255) / 256)), dim3(256), 0, stream, d_x, n, d, d_idx, k, thr);
    hipError_t he = hipGetLastError();
    RA_LAUNCH(he, emb_rank_kernel, dim3((n + DBS_TR - 1) / DBS_TR), dim3(256), lds, stream, a);
    return he == hipSuccess ? RA_OK : hip_error("ra_embed_ranks", he);
}

// ---- spectral embedding (ralign_spectral.h)

extern "C" int ra_spectral_spmv(const int *d_indptr, const int *d_indices, const double *d_val, int n, const double *d_x, double *d_y,
                                void *hip_stream)
{
    if (n < 1 || n > SPEC_MAX_N) return arg_error("ra_spectral_spmv: need 1 <= n <= 262144");
    if (!d_indptr || !d_indices || !d_val || !d_x || !d_y || d_x == d_y) return arg_error("ra_spectral_spmv: null argument, or d_y == d_x");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nb = (n + SPEC_ROWS - 1) / SPEC_ROWS;
    StreamScratch scratch(stream);
    int *bad = scratch.get<int>(1);
    if (!bad) return hip_error("ra_spectral_spmv", scratch.status());
    // the one entry that reads back: a CSR that the kernel would have to patch is refused before y is touched
    hipError_t he = hipMemsetAsync(bad, 0, sizeof(int), stream);
    RA_LAUNCH(he, spec_check_kernel, dim3(nb), dim3(256), 0, stream, d_indptr, d_indices, n, bad);
    int h_bad = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he != hipSuccess) return hip_error("ra_spectral_spmv", he);
    if (h_bad) return arg_error("ra_spectral_spmv: indptr does not ascend from 0, or a column index is outside 0 .. n - 1");
    hipLaunchKernelGGL(spec_spmv_kernel, dim3(nb), dim3(256), 0, stream, d_indptr, d_indices, d_val, n, d_x, d_y);
    he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_spectral_spmv", he);
}

// the pieces of ra_spectral_lanczos' work buffer for a basis of at most `cols` columns of Q
struct SpecWork {
    KmScratch S;
    int runs, nup;
    size_t o_w, o_part, o_h, o_np;
    SpecWork(int n, int cols)
        : runs((n + SPEC_RUN - 1) / SPEC_RUN), nup((n + SPEC_UPD - 1) / SPEC_UPD), o_w(S.take((size_t)n * 8)),
          o_part(S.take((size_t)runs * cols * 8)), o_h(S.take((size_t)cols * 8)), o_np(S.take((size_t)nup * 8)) {}
};

extern "C" size_t ra_spectral_work_bytes(int n, int basis)
{
    if (n < 2 || n > SPEC_MAX_N || basis < 1 || basis > SPEC_MAX_M) return 0;
    return SpecWork(n, basis + 1).S.off;
}

extern "C" int ra_spectral_lanczos(const int *d_indptr, const int *d_indices, const double *d_val, int n, const double *d_q0, double *d_V,
                                   int ldv, int j0, int steps, double *d_alpha, double *d_beta, void *d_work, void *hip_stream)
{
    if (n < 2 || n > SPEC_MAX_N || ldv < n || j0 < 0 || steps < 1 || j0 > SPEC_MAX_M || steps > SPEC_MAX_M || j0 + steps > SPEC_MAX_M)
        return arg_error("ra_spectral_lanczos: need 2 <= n <= 262144, ldv >= n, j0 >= 0, steps >= 1 and j0 + steps <= 4096");
    if (!d_indptr || !d_indices || !d_val || !d_q0 || !d_V || !d_alpha || !d_beta || !d_work || ((size_t)d_work & 255))
        return arg_error("ra_spectral_lanczos: null argument, or a work buffer that is not 256-byte aligned");
    hipStream_t stream = (hipStream_t)hip_stream;
    SpecWork W(n, j0 + steps + 1);                  // ra_spectral_work_bytes(n, j0 + steps)
    W.S.base = (unsigned char *)d_work;
    double *w = W.S.at<double>(W.o_w), *part = W.S.at<double>(W.o_part), *h = W.S.at<double>(W.o_h), *np = W.S.at<double>(W.o_np);
    const int nb = (n + SPEC_ROWS - 1) / SPEC_ROWS, nt = (n + 255) / 256;
    hipError_t he = hipSuccess;
    for (int j = j0; j < j0 + steps && he == hipSuccess; j++) {
        const int cols = j + 2;
        const double *vj = d_V + (size_t)j * ldv;
        const dim3 gd(W.runs, (cols + SPEC_CT - 1) / SPEC_CT);
        RA_LAUNCH(he, spec_spmv_kernel, dim3(nb), dim3(256), 0, stream, d_indptr, d_indices, d_val, n, vj, w);
        for (int pass = 0; pass < 2; pass++) {
            RA_LAUNCH(he, spec_dots_kernel, gd, dim3(256), 0, stream, d_q0, (const double *)d_V, ldv, cols, (const double *)w, n, part);
            RA_LAUNCH(he, spec_reduce_kernel, dim3((cols + 255) / 256), dim3(256), 0, stream, (const double *)part, W.runs, cols, h,
                      pass == 0 ? d_alpha + j : (double *)nullptr);
            RA_LAUNCH(he, spec_update_kernel, dim3(W.nup), dim3(SPEC_UPD), 0, stream, d_q0, (const double *)d_V, ldv, cols, (const double *)h,
                      w, n, pass == 1 ? np : (double *)nullptr);
        }
        RA_LAUNCH(he, spec_norm_kernel, dim3(1), dim3(256), 0, stream, (const double *)np, W.nup, d_beta + j);
        RA_LAUNCH(he, spec_scale_kernel, dim3(nt), dim3(256), 0, stream, (const double *)w, n, (const double *)(d_beta + j),
                  d_V + (size_t)(j + 1) * ldv);
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_spectral_lanczos", he);
}

extern "C" int ra_spectral_ritz(const double *d_V, int ldv, int m, int n, const double *d_S, int c, double *d_Y, void *hip_stream)
{
    if (n < 1 || n > SPEC_MAX_N || ldv < n || m < 1 || m > SPEC_MAX_M || c < 1 || c > SPEC_MAX_C)
        return arg_error("ra_spectral_ritz: need 1 <= n <= 262144, ldv >= n, 1 <= m <= 4096 and 1 <= c <= 64");
    if (!d_V || !d_S || !d_Y) return arg_error("ra_spectral_ritz: null argument");
    hipLaunchKernelGGL(spec_ritz_kernel, dim3((n + 255) / 256, (c + SPEC_RT - 1) / SPEC_RT), dim3(256), 0, (hipStream_t)hip_stream, d_V, ldv,
                       m, n, d_S, c, d_Y);
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_spectral_ritz", he);
}

extern "C" int ra_spectral_components(const int *d_indptr, const int *d_indices, int n, int *d_label, int *d_changed, void *hip_stream)
{
    if (n < 1 || n > SPEC_MAX_N) return arg_error("ra_spectral_components: need 1 <= n <= 262144");
    if (!d_indptr || !d_indices || !d_label || !d_changed) return arg_error("ra_spectral_components: null argument");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nt = (n + 255) / 256;
    KmScratch S;
    const size_t o_m = S.take((size_t)n * 4), o_p = S.take((size_t)n * 4);
    StreamScratch scratch(stream);
    if (!(S.base = scratch.get<unsigned char>(S.off))) return hip_error("ra_spectral_components", scratch.status());
    int *m = S.at<int>(o_m), *P = S.at<int>(o_p);
    hipError_t he = hipMemsetAsync(d_changed, 0, sizeof(int), stream);
    RA_LAUNCH(he, spec_min_kernel, dim3((n + SPEC_ROWS - 1) / SPEC_ROWS), dim3(256), 0, stream, d_indptr, d_indices, n, (const int *)d_label, m);
    if (he == hipSuccess) he = hipMemcpyAsync(P, d_label, (size_t)n * 4, hipMemcpyDeviceToDevice, stream);
    RA_LAUNCH(he, spec_hook_kernel, dim3(nt), dim3(256), 0, stream, n, (const int *)d_label, (const int *)m, P);
    RA_LAUNCH(he, spec_compress_kernel, dim3(nt), dim3(256), 0, stream, n, (const int *)P, d_label, d_changed);
    return he == hipSuccess ? RA_OK : hip_error("ra_spectral_components", he);
}

// ---- UMAP (ralign_umap.h)

extern "C" int ra_umap_smooth_knn(const double *d_dist2, int rows, int k, int n_neighbors, double *d_rho, double *d_sigma, double *d_w,
                                  void *hip_stream)
{
    if (rows < 1 || rows > UMAP_MAX_ROWS || k < 1 || k > UMAP_MAX_K || n_neighbors < 2 || n_neighbors > UMAP_MAX_K + 1)
        return arg_error("ra_umap_smooth_knn: need 1 <= rows <= 4194304, 1 <= k <= 301 and 2 <= n_neighbors <= 302");
    if (!d_dist2 || !d_rho || !d_sigma || !d_w) return arg_error("ra_umap_smooth_knn: null argument");
    hipLaunchKernelGGL(umap_smooth_kernel, dim3((rows + UMAP_SK_ROWS - 1) / UMAP_SK_ROWS), dim3(256), 0, (hipStream_t)hip_stream, d_dist2,
                       rows, k, std::log2((double)n_neighbors), d_rho, d_sigma, d_w);
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_umap_smooth_knn", he);
}

static bool umap_curve_ok(const char *what, double a, double b, double gamma, int neg, double lr, int n_epochs, UmapCurve &c)
{
    if (!std::isfinite(a) || !(a > 0.0) || !std::isfinite(b) || !(b > 0.0) || !std::isfinite(gamma) || !(gamma >= 0.0) || neg < 0 ||
        neg > UMAP_MAX_NEG || !std::isfinite(lr) || !(lr > 0.0) || n_epochs < 1 || n_epochs > UMAP_MAX_EPOCHS) {
        set_error(std::string(what) + ": need finite a > 0, b > 0, gamma >= 0 and lr > 0, 0 <= negatives <= 16 and 1 <= n_epochs <= 10000");
        return false;
    }
    c.a = a; c.b = b; c.m2ab = (-2.0 * a) * b; c.g2b = (2.0 * gamma) * b;
    return true;
}

extern "C" int ra_umap_epochs(float *d_y, float *d_y_alt, int n, const int *d_indptr, const int *d_indices, const double *d_rate, int nnz,
                              double a, double b, double gamma, int neg, double lr, int n_epochs, int epoch0, int count,
                              unsigned long long seed, void *hip_stream)
{
    UmapEpochArgs e;
    if (n < 4 || n > UMAP_MAX_N || nnz < 0 || (long long)nnz > 2LL * n * UMAP_MAX_K)
        return arg_error("ra_umap_epochs: need 4 <= n <= 262144 and 0 <= nnz <= 2 n 301");
    if (!umap_curve_ok("ra_umap_epochs", a, b, gamma, neg, lr, n_epochs, e.c)) return RA_ERR_ARG;
    if (epoch0 < 1 || count < 1 || epoch0 > n_epochs || count > n_epochs - epoch0 + 1)
        return arg_error("ra_umap_epochs: need epoch0 >= 1, count >= 1 and epoch0 + count - 1 <= n_epochs");
    if (!d_y || !d_y_alt || d_y == d_y_alt || !d_indptr || (nnz > 0 && (!d_indices || !d_rate)))
        return arg_error("ra_umap_epochs: null argument, or d_y_alt == d_y (an epoch reads every y_j while it writes)");
    hipStream_t stream = (hipStream_t)hip_stream;
    const int nb = (n + UMAP_ROWS - 1) / UMAP_ROWS;
    StreamScratch scratch(stream);
    int *bad = scratch.get<int>(1);
    if (!bad) return hip_error("ra_umap_epochs", scratch.status());
    // the one read of the call: a CSR that the kernel would have to patch is refused before a position is written
    hipError_t he = hipMemsetAsync(bad, 0, sizeof(int), stream);
    RA_LAUNCH(he, umap_check_kernel, dim3(nb), dim3(256), 0, stream, d_indptr, d_indices, n, nnz, bad);
    int h_bad = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&h_bad, bad, sizeof(int), hipMemcpyDeviceToHost, stream);
    if (he == hipSuccess) he = hipStreamSynchronize(stream);
    if (he != hipSuccess) return hip_error("ra_umap_epochs", he);
    if (h_bad) return arg_error("ra_umap_epochs: indptr does not ascend from 0 to nnz, or a column index is outside 0 .. n - 1");
    e.indptr = d_indptr; e.indices = d_indices; e.rate = d_rate; e.n = n; e.neg = neg;
    for (int s = 0; s < count && he == hipSuccess; s++) {
        const int t = epoch0 + s;
        e.y = (const float2 *)(s % 2 ? d_y_alt : d_y);
        e.y_out = (float2 *)(s % 2 ? d_y : d_y_alt);
        e.t = t;
        e.alpha = lr * (1.0 - (double)(t - 1) / (double)n_epochs);
        e.key = seed * UMAP_KEY_SEED + (unsigned long long)t * UMAP_KEY_EPOCH;
        RA_LAUNCH(he, umap_epoch_kernel, dim3(nb), dim3(256), 0, stream, e);
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_umap_epochs", he);
}

extern "C" int ra_umap_place(float *d_y, int n_new, long long row0, const float *d_yfit, int m, const int *d_idx, const double *d_rate, int k,
                             double a, double b, double gamma, int neg, double lr, int n_epochs, unsigned long long seed, void *hip_stream)
{
    UmapPlaceArgs p;
    if (n_new < 1 || n_new > UMAP_MAX_ROWS || row0 < 0 || row0 > UMAP_MAX_ROW0 - n_new || m < 2 || m > UMAP_MAX_N || k < 1 ||
        k > std::min(m, UMAP_MAX_K))
        return arg_error("ra_umap_place: need 1 <= n_new <= 4194304, row0 >= 0, row0 + n_new <= 2^48, 2 <= m <= 262144 and 1 <= k <= min(m, 301)");
    if (!umap_curve_ok("ra_umap_place", a, b, gamma, neg, lr, n_epochs, p.c)) return RA_ERR_ARG;
    if (!d_y || !d_yfit || !d_idx || !d_rate) return arg_error("ra_umap_place: null argument");
    p.y = (float2 *)d_y; p.yfit = (const float2 *)d_yfit; p.idx = d_idx; p.rate = d_rate;
    p.n = n_new; p.m = m; p.k = k; p.neg = neg; p.n_epochs = n_epochs;
    p.row0 = (unsigned long long)row0; p.seed_key = seed * UMAP_KEY_SEED; p.lr = lr;
    hipLaunchKernelGGL(umap_place_kernel, dim3((n_new + UMAP_ROWS - 1) / UMAP_ROWS), dim3(256), 0, (hipStream_t)hip_stream, p);
    const hipError_t he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_umap_place", he);
}
