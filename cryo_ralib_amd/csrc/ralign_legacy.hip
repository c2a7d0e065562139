// The reference-compatible surface of libralign_hip.so (cuda/gpu_aln_noref.h:52-113) on top of the ra_* API: one
// process-global engine on the default stream, synchronous calls, print + abort on failure like the reference
// (gpu_aln_common.cu:89-103).  It sees the engine through include/ralign.h and the two hidden calls of ralign_host.h only.
#include <cstdlib>
#include <cstring>

#include "ralign_host.h"

namespace {
struct Legacy {
    ra_engine *eng = nullptr;
    AlignConfig cfg{};
    unsigned num_particles = 0;
    int device = -1;
    AlignParam *h_param = nullptr;       // pinned, caller reads / writes in place
    float *d_sbj = nullptr, *d_ref = nullptr, *d_aligned = nullptr, *d_state = nullptr, *d_sums = nullptr;
    int *d_counts = nullptr;
    ra_result *d_res = nullptr, *h_res = nullptr;
    float *h_stage = nullptr, *h_state = nullptr, *h_sums = nullptr;
    int *h_counts = nullptr;
    size_t stage_imgs = 0;
    unsigned sbj_loaded = 0;
    // class-resident (ISAC) mode: particles sorted by class, one reference per class
    bool isac = false;
    std::vector<unsigned> cid_idx;       // [ref_num + 1] first particle of every class
    unsigned *d_cid_idx = nullptr;
    int *d_cls = nullptr;                // [sbj_num] class of every particle (class-resident single launch)
} L;
const hipStream_t kStream = nullptr;     // the stream of L.eng: nothing here calls ra_set_stream, so it stays the default one

void die(const char *what)
{
    fprintf(stderr, "libralign_hip: %s: %s\n", what, ra_last_error());
    exit(EXIT_FAILURE);
}
void hip_or_die(hipError_t e, const char *what)
{
    if (e != hipSuccess) { fprintf(stderr, "libralign_hip: %s: %s\n", what, hipGetErrorString(e)); exit(EXIT_FAILURE); }
}

ra_config legacy_config(const AlignConfig *c, unsigned device, int mode)
{
    ra_config rc{};
    rc.nx = (int)c->img_dim; rc.first_ring = 1; rc.last_ring = (int)c->ring_num; rc.ring_skip = 1;
    rc.xrng = c->shift_rng_x; rc.yrng = c->shift_rng_y; rc.step = c->shift_step;
    rc.nref = (int)c->ref_num; rc.mode = mode; rc.device = (int)device; rc.chunk = 0;
    return rc;
}

size_t legacy_bytes(unsigned num_particles, const AlignConfig *c)
{
    // everything pre_align_init takes from the device: the engine's workspace (same plan as ra_create) plus the
    // resident batch (particles, aligned images, state, results), the references and the class sums
    if (c->img_dim < 8 || c->ref_num < 1) return (size_t)-1;
    ra_config rc = legacy_config(c, 0, RA_MODE_MREF);
    rc.chunk = (int)std::min<unsigned>(8192, std::max(2u, c->sbj_num));
    const size_t ws = ra_planned_workspace_bytes(&rc);
    if (ws == (size_t)-1) return ws;
    const size_t npix = (size_t)c->img_dim * c->img_dim, B = c->sbj_num, R = c->ref_num;
    const size_t batch = B * npix * 4 * 2 + B * (2 * sizeof(float) + sizeof(ra_result)) + R * npix * 4 * 3 + R * 4;
    (void)num_particles;     // the AlignParam array lives in pinned host memory
    return ws + batch + (size_t)8 * (2 << 20);
}

void run_search(int start, int stop, int mode)
{
    if (!L.eng) { fprintf(stderr, "libralign_hip: *_run before pre_align_init\n"); exit(EXIT_FAILURE); }
    const int n = stop - start;
    if (n <= 0 || (unsigned)n > L.cfg.sbj_num || (unsigned)stop > L.num_particles) {
        fprintf(stderr, "libralign_hip: bad index range [%d,%d)\n", start, stop);
        exit(EXIT_FAILURE);
    }
    ra_engine_switch_mode(L.eng, mode);
    for (int i = 0; i < n; i++) { L.h_state[2 * i] = L.h_param[start + i].shift_x; L.h_state[2 * i + 1] = L.h_param[start + i].shift_y; }
    hip_or_die(hipMemcpy(L.d_state, L.h_state, sizeof(float) * 2 * n, hipMemcpyHostToDevice), "state upload");
    if (ra_align(L.eng, L.d_sbj, n, L.d_state, L.d_res, nullptr)) die("ra_align");
}

void fetch_results(int start, int stop)
{
    const int n = stop - start;
    if (ra_sync(L.eng)) die("sync");
    hip_or_die(hipMemcpy(L.h_res, L.d_res, sizeof(ra_result) * n, hipMemcpyDeviceToHost), "result download");
    hip_or_die(hipMemcpy(L.h_state, L.d_state, sizeof(float) * 2 * n, hipMemcpyDeviceToHost), "state download");
    for (int i = 0; i < n; i++) {
        AlignParam &a = L.h_param[start + i];
        a.ref_id = L.h_res[i].ref_id;
        a.shift_x = L.h_state[2 * i]; a.shift_y = L.h_state[2 * i + 1];
        a.angle = L.h_res[i].alpha;
        a.mirror = L.h_res[i].mirror != 0;
    }
}

// `need` bytes ((size_t)-1: bad geometry) against `request` of the current device's free memory
bool size_check(size_t need, unsigned device_id, float request, bool verbose)
{
    size_t fr = 0, tot = 0;
    if (need == (size_t)-1 || hipMemGetInfo(&fr, &tot) != hipSuccess) return false;
    if (verbose)
        printf("GPU[%u] SIZE CHECK: need %zu MB of %zu MB free (request %.2f)\n", device_id, need >> 20, fr >> 20, request);
    return (double)need <= (double)fr * request;
}
}  // namespace

extern "C" void print_gpu_info(const unsigned int device_idx)
{
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, (int)device_idx) != hipSuccess) { printf("GPU[%u]: not available\n", device_idx); return; }
    size_t fr = 0, tot = 0;
    (void)hipSetDevice((int)device_idx);
    (void)hipMemGetInfo(&fr, &tot);
    printf("GPU[%u]: %s (%s), %d CUs, %.1f GiB total, %.1f GiB free, LDS/CU %zu KB, wave %d\n", device_idx, p.name,
           p.gcnArchName, p.multiProcessorCount, tot / 1073741824.0, fr / 1073741824.0,
           (size_t)p.maxSharedMemoryPerMultiProcessor / 1024, p.warpSize);
}

extern "C" void gpu_clear(void)
{
    if (L.eng) { ra_destroy(L.eng); L.eng = nullptr; }
    if (L.h_param) (void)hipHostFree(L.h_param);
    if (L.h_stage) (void)hipHostFree(L.h_stage);
    if (L.h_state) (void)hipHostFree(L.h_state);
    if (L.h_sums) (void)hipHostFree(L.h_sums);
    if (L.h_counts) (void)hipHostFree(L.h_counts);
    if (L.h_res) (void)hipHostFree(L.h_res);
    for (void *p : {(void *)L.d_sbj, (void *)L.d_ref, (void *)L.d_aligned, (void *)L.d_state, (void *)L.d_sums,
                    (void *)L.d_counts, (void *)L.d_res, (void *)L.d_cid_idx, (void *)L.d_cls})
        if (p) (void)hipFree(p);
    int dev = L.device;
    L = Legacy();
    L.device = dev;   // the reference pins the process to one device id (gpu_aln_noref.cu:105)
}

extern "C" AlignParam *pre_align_init(const unsigned int num_particles, const AlignConfig *aln_cfg,
                                      const unsigned int device_id)
{
    if (!aln_cfg) { fprintf(stderr, "libralign_hip: pre_align_init: null config\n"); exit(EXIT_FAILURE); }
    if (L.device != -1 && L.device != (int)device_id) {
        fprintf(stderr, "libralign_hip: device id may not change within a process\n");
        exit(EXIT_FAILURE);
    }
    if (L.eng) gpu_clear();
    L.device = (int)device_id;
    L.cfg = *aln_cfg;
    L.num_particles = num_particles;
    ra_config rc = legacy_config(aln_cfg, device_id, RA_MODE_MREF);
    rc.chunk = (int)std::min<unsigned>(8192, std::max(2u, aln_cfg->sbj_num));
    if (ra_create(&L.eng, &rc)) die("pre_align_init");
    const size_t npix = (size_t)aln_cfg->img_dim * aln_cfg->img_dim;
    const size_t B = aln_cfg->sbj_num, R = aln_cfg->ref_num;
    hip_or_die(hipHostMalloc((void **)&L.h_param, sizeof(AlignParam) * std::max(1u, num_particles)), "param alloc");
    for (unsigned i = 0; i < num_particles; i++) {
        L.h_param[i].sbj_id = -1; L.h_param[i].ref_id = 0; L.h_param[i].shift_x = 0; L.h_param[i].shift_y = 0;
        L.h_param[i].angle = 0; L.h_param[i].mirror = false;
    }
    L.stage_imgs = std::max(B, R);
    hip_or_die(hipHostMalloc((void **)&L.h_stage, L.stage_imgs * npix * sizeof(float)), "stage alloc");
    hip_or_die(hipHostMalloc((void **)&L.h_state, B * 2 * sizeof(float)), "state alloc");
    hip_or_die(hipHostMalloc((void **)&L.h_res, B * sizeof(ra_result)), "res alloc");
    hip_or_die(hipHostMalloc((void **)&L.h_sums, R * 2 * npix * sizeof(float)), "sums alloc");
    hip_or_die(hipHostMalloc((void **)&L.h_counts, R * sizeof(int)), "counts alloc");
    hip_or_die(hipMalloc((void **)&L.d_sbj, B * npix * sizeof(float)), "sbj alloc");
    hip_or_die(hipMalloc((void **)&L.d_aligned, B * npix * sizeof(float)), "aligned alloc");
    hip_or_die(hipMalloc((void **)&L.d_ref, R * npix * sizeof(float)), "ref alloc");
    hip_or_die(hipMalloc((void **)&L.d_state, B * 2 * sizeof(float)), "state alloc");
    hip_or_die(hipMalloc((void **)&L.d_res, B * sizeof(ra_result)), "res alloc");
    hip_or_die(hipMalloc((void **)&L.d_sums, R * 2 * npix * sizeof(float)), "sums alloc");
    hip_or_die(hipMalloc((void **)&L.d_counts, R * sizeof(int)), "counts alloc");
    hip_or_die(hipMemset(L.d_res, 0, B * sizeof(ra_result)), "res clear");
    return L.h_param;
}

extern "C" bool pre_align_size_check(const unsigned int num_particles, const AlignConfig *cfg,
                                     const unsigned int device_id, const float request, const bool verbose)
{
    return cfg && hipSetDevice((int)device_id) == hipSuccess && size_check(legacy_bytes(num_particles, cfg), device_id, request, verbose);
}

extern "C" void pre_align_fetch(const float **img_data, const unsigned int img_num, const char *batch_type)
{
    if (!L.eng) { fprintf(stderr, "libralign_hip: pre_align_fetch before pre_align_init\n"); exit(EXIT_FAILURE); }
    const size_t npix = (size_t)L.cfg.img_dim * L.cfg.img_dim;
    const bool is_sbj = batch_type && strcmp(batch_type, "sbj_batch") == 0;
    const bool is_ref = batch_type && strcmp(batch_type, "ref_batch") == 0;
    if (!is_sbj && !is_ref) {
        // same message and behaviour as gpu_aln_noref.cu:373-376
        printf("ERROR! fetch_data() :: Unknown batch type '%s' specified.\n", batch_type ? batch_type : "(null)");
        return;
    }
    const unsigned cap = is_sbj ? L.cfg.sbj_num : L.cfg.ref_num;
    if (img_num > cap || !img_data) { fprintf(stderr, "libralign_hip: pre_align_fetch: %u images exceed the batch (%u)\n", img_num, cap); exit(EXIT_FAILURE); }
    // gather into one pinned block and ship with a single copy
    for (unsigned i = 0; i < img_num; i++) memcpy(L.h_stage + (size_t)i * npix, img_data[i], npix * sizeof(float));
    float *dst = is_sbj ? L.d_sbj : L.d_ref;
    hip_or_die(hipMemcpy(dst, L.h_stage, (size_t)img_num * npix * sizeof(float), hipMemcpyHostToDevice), "image upload");
    if (is_sbj) L.sbj_loaded = img_num;
    else if (ra_set_references(L.eng, L.d_ref)) die("ra_set_references");
}

extern "C" void pre_align_run(const int start_idx, const int stop_idx)
{
    run_search(start_idx, stop_idx, RA_MODE_REFFREE);
    fetch_results(start_idx, stop_idx);
}

// the search in `mode`, then the aligned images of the range (device memory)
static void *run_and_transform(int start_idx, int stop_idx, int mode)
{
    run_search(start_idx, stop_idx, mode);
    if (ra_transform_accumulate(L.eng, L.d_sbj, stop_idx - start_idx, start_idx, L.d_res, L.d_aligned, nullptr, nullptr)) die("transform");
    fetch_results(start_idx, stop_idx);
    return L.d_aligned;
}
extern "C" void *pre_align_run_m(const int start_idx, const int stop_idx) { return run_and_transform(start_idx, stop_idx, RA_MODE_REFFREE); }
extern "C" void *mref_align_run(const int start_idx, const int stop_idx) { return run_and_transform(start_idx, stop_idx, RA_MODE_MREF); }

extern "C" float *mref_align_run_m(const int start_idx, const int stop_idx)
{
    const size_t npix = (size_t)L.cfg.img_dim * L.cfg.img_dim, R = L.cfg.ref_num;
    run_search(start_idx, stop_idx, RA_MODE_MREF);
    hip_or_die(hipMemsetAsync(L.d_sums, 0, R * 2 * npix * sizeof(float), kStream), "sums clear");
    hip_or_die(hipMemsetAsync(L.d_counts, 0, R * sizeof(int), kStream), "counts clear");
    if (ra_transform_accumulate(L.eng, L.d_sbj, stop_idx - start_idx, start_idx, L.d_res, L.d_aligned, L.d_sums, L.d_counts)) die("transform");
    fetch_results(start_idx, stop_idx);
    // reference layout: all even averages, then all odd ones (test_mref_cheng_yu_bdb_cuda.py:550-551)
    std::vector<float> tmp(R * 2 * npix);
    hip_or_die(hipMemcpy(tmp.data(), L.d_sums, tmp.size() * sizeof(float), hipMemcpyDeviceToHost), "sums download");
    for (size_t r = 0; r < R; r++) {
        memcpy(L.h_sums + r * npix, tmp.data() + (r * 2) * npix, npix * sizeof(float));
        memcpy(L.h_sums + (R + r) * npix, tmp.data() + (r * 2 + 1) * npix, npix * sizeof(float));
    }
    hip_or_die(hipMemcpy(L.h_counts, L.d_counts, R * sizeof(int), hipMemcpyDeviceToHost), "counts download");
    return L.h_sums;
}

extern "C" int *get_num_ref(void) { return L.h_counts; }

extern "C" void reset_shifts(const float shift_range, const float shift_step)
{
    if (!L.eng) { fprintf(stderr, "libralign_hip: reset_shifts before pre_align_init\n"); exit(EXIT_FAILURE); }
    if (ra_reset_shifts(L.eng, shift_range, shift_range, shift_step)) die("reset_shifts");
}

// ---------------------------------------------------------------------------------------------
// class-resident reference-free alignment (cuda/gpu_aln_noref.h:94-109, gpu_aln_noref.cu:559-782; SURVEY.md
// section 8 row f-3): particles arrive sorted by class, every particle is aligned to the average of its own class
// (single-reference search with sp_alignment.ormq semantics), transformed, and the class averages are rebuilt
// on the device from the aligned images; ref_free_alignment_2D_filter_references applies the tangent low-pass.

// mean of the aligned images of the contiguous class range [cid_idx[r], cid_idx[r+1]) in particle order
// (cu_average_batch, gpu_aln_noref.cu:1199-1229); an empty class keeps its previous reference
__global__ __launch_bounds__(256) void class_mean_kernel(int npix, const float *__restrict__ aligned,
                                                         const unsigned *__restrict__ cid_idx, float *__restrict__ refs)
{
    const int r = blockIdx.x;
    const unsigned b = cid_idx[r], e = cid_idx[r + 1];
    if (e <= b) return;
    for (int pix = blockIdx.y * blockDim.x + threadIdx.x; pix < npix; pix += gridDim.y * blockDim.x) {
        float avg = 0.f;
        for (unsigned i = b; i < e; i++) avg += aligned[(size_t)i * npix + pix];
        refs[(size_t)r * npix + pix] = avg / (float)(e - b);
    }
}

static size_t isac_bytes(const AlignConfig *c)
{
    AlignConfig one = *c;
    one.ref_num = 1;
    const size_t npix = (size_t)c->img_dim * c->img_dim;
    size_t need = legacy_bytes(c->sbj_num, &one);
    if (need == (size_t)-1) return need;
    return need + (size_t)c->ref_num * npix * 4 + ((size_t)c->ref_num + 1) * 4;
}

extern "C" AlignParam *ref_free_alignment_2D_init(const AlignConfig *aln_cfg, const float **sbj_data_list,
                                                  const float **ref_data_list, const int *sbj_cid_list,
                                                  const unsigned int device_id)
{
    if (!aln_cfg || !sbj_data_list || !ref_data_list || !sbj_cid_list) {
        fprintf(stderr, "libralign_hip: ref_free_alignment_2D_init: null argument\n");
        exit(EXIT_FAILURE);
    }
    if (L.device != -1 && L.device != (int)device_id) {
        fprintf(stderr, "libralign_hip: device id may not change within a process\n");
        exit(EXIT_FAILURE);
    }
    if (L.eng) gpu_clear();
    L.device = (int)device_id;
    L.cfg = *aln_cfg;
    L.num_particles = aln_cfg->sbj_num;
    L.isac = true;
    const size_t npix = (size_t)aln_cfg->img_dim * aln_cfg->img_dim;
    const size_t B = aln_cfg->sbj_num, R = aln_cfg->ref_num;
    // class index list as the reference builds it (gpu_aln_noref.cu:611-620): a new class starts where the id changes
    L.cid_idx.assign(R + 1, (unsigned)B);
    {
        int cid = -1; size_t idx = 0;
        for (size_t i = 0; i < B; i++)
            if (sbj_cid_list[i] != cid) {
                if (idx >= R) { fprintf(stderr, "libralign_hip: ref_free_alignment_2D_init: more class runs than references\n"); exit(EXIT_FAILURE); }
                L.cid_idx[idx++] = (unsigned)i; cid = sbj_cid_list[i];
            }
    }
    ra_config rc = legacy_config(aln_cfg, device_id, RA_MODE_REFFREE);
    rc.nref = 1;
    rc.chunk = (int)std::min<unsigned>(8192, std::max(2u, aln_cfg->sbj_num));
    if (ra_create(&L.eng, &rc)) die("ref_free_alignment_2D_init");
    hip_or_die(hipHostMalloc((void **)&L.h_param, sizeof(AlignParam) * std::max<size_t>(1, B)), "param alloc");
    for (size_t i = 0; i < B; i++) {
        L.h_param[i].sbj_id = -1; L.h_param[i].ref_id = sbj_cid_list[i]; L.h_param[i].shift_x = 0; L.h_param[i].shift_y = 0;
        L.h_param[i].angle = 0; L.h_param[i].mirror = false;
    }
    L.stage_imgs = std::max(B, R);
    hip_or_die(hipHostMalloc((void **)&L.h_stage, L.stage_imgs * npix * sizeof(float)), "stage alloc");
    hip_or_die(hipHostMalloc((void **)&L.h_state, B * 2 * sizeof(float)), "state alloc");
    hip_or_die(hipHostMalloc((void **)&L.h_res, B * sizeof(ra_result)), "res alloc");
    hip_or_die(hipMalloc((void **)&L.d_sbj, B * npix * sizeof(float)), "sbj alloc");
    hip_or_die(hipMalloc((void **)&L.d_aligned, B * npix * sizeof(float)), "aligned alloc");
    hip_or_die(hipMalloc((void **)&L.d_ref, R * npix * sizeof(float)), "ref alloc");
    hip_or_die(hipMalloc((void **)&L.d_state, B * 2 * sizeof(float)), "state alloc");
    hip_or_die(hipMalloc((void **)&L.d_res, B * sizeof(ra_result)), "res alloc");
    hip_or_die(hipMalloc((void **)&L.d_cid_idx, (R + 1) * sizeof(unsigned)), "cid alloc");
    hip_or_die(hipMemset(L.d_res, 0, B * sizeof(ra_result)), "res clear");
    hip_or_die(hipMemcpy(L.d_cid_idx, L.cid_idx.data(), (R + 1) * sizeof(unsigned), hipMemcpyHostToDevice), "cid upload");
    {
        std::vector<int> cls(B);
        for (unsigned r = 0; r < R; r++)
            for (unsigned i = L.cid_idx[r]; i < L.cid_idx[r + 1]; i++) cls[i] = (int)r;
        hip_or_die(hipMalloc((void **)&L.d_cls, B * sizeof(int)), "class index alloc");
        hip_or_die(hipMemcpy(L.d_cls, cls.data(), B * sizeof(int), hipMemcpyHostToDevice), "class index upload");
    }
    for (size_t i = 0; i < B; i++) memcpy(L.h_stage + i * npix, sbj_data_list[i], npix * sizeof(float));
    hip_or_die(hipMemcpy(L.d_sbj, L.h_stage, B * npix * sizeof(float), hipMemcpyHostToDevice), "image upload");
    for (size_t i = 0; i < R; i++) memcpy(L.h_stage + i * npix, ref_data_list[i], npix * sizeof(float));
    hip_or_die(hipMemcpy(L.d_ref, L.h_stage, R * npix * sizeof(float), hipMemcpyHostToDevice), "reference upload");
    L.sbj_loaded = (unsigned)B;
    return L.h_param;
}

extern "C" bool ref_free_alignment_2D_size_check(const AlignConfig *cfg, const unsigned int device_id, const float request,
                                                 const bool verbose)
{
    return cfg && hipSetDevice((int)device_id) == hipSuccess && size_check(isac_bytes(cfg), device_id, request, verbose);
}

extern "C" void ref_free_alignment_2D(void)
{
    if (!L.eng || !L.isac) { fprintf(stderr, "libralign_hip: ref_free_alignment_2D before ref_free_alignment_2D_init\n"); exit(EXIT_FAILURE); }
    const size_t npix = (size_t)L.cfg.img_dim * L.cfg.img_dim;
    const unsigned B = L.cfg.sbj_num, R = L.cfg.ref_num;
    for (unsigned i = 0; i < B; i++) { L.h_state[2 * i] = L.h_param[i].shift_x; L.h_state[2 * i + 1] = L.h_param[i].shift_y; }
    hip_or_die(hipMemcpy(L.d_state, L.h_state, sizeof(float) * 2 * B, hipMemcpyHostToDevice), "state upload");
    // all classes in one launch where the fused search kernel covers the geometry, class by class otherwise
    if (ra_set_class_references(L.eng, L.d_ref, (int)R) == RA_OK) {
        if (ra_align_classes(L.eng, L.d_sbj, (int)B, L.d_state, L.d_res, L.d_cls)) die("ra_align_classes");
    } else {
        for (unsigned r = 0; r < R; r++) {
            const unsigned b = L.cid_idx[r], e = L.cid_idx[r + 1];
            if (e <= b) continue;
            if (ra_set_references(L.eng, L.d_ref + (size_t)r * npix)) die("ra_set_references");
            if (ra_align(L.eng, L.d_sbj + (size_t)b * npix, (int)(e - b), L.d_state + 2 * (size_t)b, L.d_res + b, nullptr)) die("ra_align");
        }
    }
    if (ra_transform_accumulate(L.eng, L.d_sbj, (int)B, 0, L.d_res, L.d_aligned, nullptr, nullptr)) die("transform");
    hipLaunchKernelGGL(class_mean_kernel, dim3(R, 8), dim3(256), 0, kStream, (int)npix, L.d_aligned, L.d_cid_idx, L.d_ref);
    hip_or_die(hipGetLastError(), "class_mean_kernel");
    if (ra_sync(L.eng)) die("sync");
    hip_or_die(hipMemcpy(L.h_res, L.d_res, sizeof(ra_result) * B, hipMemcpyDeviceToHost), "result download");
    hip_or_die(hipMemcpy(L.h_state, L.d_state, sizeof(float) * 2 * B, hipMemcpyDeviceToHost), "state download");
    for (unsigned i = 0; i < B; i++) {      // ref_id keeps the class id given at init (gpu_aln_noref.cu:607-608)
        AlignParam &a = L.h_param[i];
        a.shift_x = L.h_state[2 * i]; a.shift_y = L.h_state[2 * i + 1];
        a.angle = L.h_res[i].alpha;
        a.mirror = L.h_res[i].mirror != 0;
    }
}

extern "C" void ref_free_alignment_2D_filter_references(const float cutoff_freq, const float falloff)
{
    if (!L.eng || !L.isac) { fprintf(stderr, "libralign_hip: filter_references before ref_free_alignment_2D_init\n"); exit(EXIT_FAILURE); }
    if (ra_filter_references(L.eng, L.d_ref, (int)L.cfg.ref_num, cutoff_freq, falloff, 0, nullptr, 0, nullptr)) die("ra_filter_references");
    if (ra_sync(L.eng)) die("sync");
}

// extension (not in the reference header): copy the current class averages [ref_num][nx][nx] to host memory
extern "C" int ra_isac_get_references(float *h_out)
{
    if (!L.eng || !L.isac || !h_out) { set_error("class-resident mode is not initialised"); return RA_ERR_STATE; }
    const size_t npix = (size_t)L.cfg.img_dim * L.cfg.img_dim;
    RA_HIP(hipMemcpy(h_out, L.d_ref, (size_t)L.cfg.ref_num * npix * sizeof(float), hipMemcpyDeviceToHost));
    return RA_OK;
}

// diagnostic: the device-memory estimate behind pre_align_size_check, in bytes ((size_t)-1 = bad geometry)
extern "C" size_t ra_legacy_bytes(const unsigned int num_particles, const AlignConfig *cfg)
{
    return cfg ? legacy_bytes(num_particles, cfg) : (size_t)-1;
}
