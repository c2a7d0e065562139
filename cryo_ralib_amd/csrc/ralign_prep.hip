// Particle preprocessing on the caller's stream (ralign_prep.h): the engine-less ra_prep_normalize and ra_prep_filter entry
// points of libralign_hip.so.
#include "ralign_host.h"
#include "ralign_prep.h"

using namespace ralign;

// workgroups of the normalisation: one per image up to what the chip holds at this LDS size (256 CUs, <= 32 waves per CU);
// beyond that the workgroups loop over the images
static int pp_normalize_grid(int n, size_t lds)
{
    const int per_cu = std::max(1, std::min(32 * PP_WAVE / PP_THREADS, (int)((size_t)160 * 1024 / lds)));
    return std::min(n, 256 * per_cu);
}

extern "C" int ra_prep_normalize(float *d_images, int n, int nx, double bg_radius, int ramp, int invert, double *d_stats, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 0 || nx < 4 || nx > 1024 || !std::isfinite(bg_radius) || bg_radius < 1.0 || bg_radius > 0.5 * nx ||
        (ramp != 0 && ramp != 1) || (invert != 0 && invert != 1))
        return arg_error("ra_prep_normalize: need n >= 0, 4 <= nx <= 1024, 1 <= bg_radius <= nx/2, ramp and invert 0 or 1");
    if (n == 0) return RA_OK;
    if (!d_images) return arg_error("ra_prep_normalize: null argument");
    PpGeom g;
    if (!pp_make_geom(nx, bg_radius, g)) return arg_error("ra_prep_normalize: the background set does not span a plane");
    const bool in_lds = pp_image_in_lds(nx);
    const size_t lds = PP_RED_BYTES + (in_lds ? (size_t)nx * nx * sizeof(float) : 0);
    const void *fk = in_lds ? (const void *)prep_normalize_kernel<true> : (const void *)prep_normalize_kernel<false>;
    if (const int rc = raise_dynamic_lds(nullptr, fk, "prep_normalize_kernel", lds)) return rc;
    float sgn = invert ? -1.f : 1.f;
    void *args[] = {&d_images, &n, &g, &ramp, &sgn, &d_stats};
    hipError_t he = hipLaunchKernel(fk, dim3(pp_normalize_grid(n, lds)), dim3(PP_THREADS), args, lds, stream);
    if (he == hipSuccess) he = hipGetLastError();
    return he == hipSuccess ? RA_OK : hip_error("ra_prep_normalize", he);
}

static bool pp_term_ok(int kind, double a, double b)
{
    if (kind == PP_NONE) return true;
    if (!std::isfinite(a) || !(a > 0.0)) return false;
    if (kind == PP_GAUSS) return true;
    return kind == PP_TANL && a < 1.0 && std::isfinite(b) && b > 0.0;
}

static const void *pp_filter_fixed_fn(int nx, int pad)
{
    switch (nx * 2 + pad) {
#define PP_FIXED_CASE(NX, PAD) case NX * 2 + PAD: return (const void *)prep_filter_fixed_kernel<NX, PAD>;
    PF_FIXED_BOXES(PP_FIXED_CASE)
#undef PP_FIXED_CASE
    default: return nullptr;
    }
}

extern "C" int ra_prep_filter(float *d_images, int n, int nx, int pad, int lp_kind, double lp_a, double lp_b, int hp_kind, double hp_a,
                              double hp_b, void *hip_stream)
{
    hipStream_t stream = (hipStream_t)hip_stream;
    if (n < 0 || nx < 2 || nx > 1024 || (pad != 0 && pad != 1)) return arg_error("ra_prep_filter: need n >= 0, 2 <= nx <= 1024 and pad 0 or 1");
    if ((lp_kind == PP_NONE && hp_kind == PP_NONE) || !pp_term_ok(lp_kind, lp_a, lp_b) || !pp_term_ok(hp_kind, hp_a, hp_b))
        return arg_error("ra_prep_filter: need a low-pass or a high-pass, each tanl (kind 1: 0 < fl < 1, aa > 0) or gauss (kind 2: sigma > 0)");
    if (n == 0) return RA_OK;
    if (!d_images) return arg_error("ra_prep_filter: null argument");
    const PfPlan pl = pf_make_plan(nx, pad);
    if (pl.nb < 1) return arg_error("ra_prep_filter: no plan for this box");
    const void *fk = pp_filter_fixed_fn(nx, pad);
    const bool fixed = fk != nullptr;
    if (!fixed) fk = pl.gblk ? (const void *)prep_filter_kernel<true> : (const void *)prep_filter_kernel<false>;
    if (const int rc = raise_dynamic_lds(nullptr, fk, fixed ? "prep_filter_fixed_kernel" : "prep_filter_kernel", (size_t)pl.lds)) return rc;
    const int grid = pl.gblk ? pf_gblk_grid(pl, n) : n, H = pl.H;
    StreamScratch scratch(stream);
    float *d_tab = scratch.get<float>((size_t)H * H);
    float2 *d_scr = pl.gblk ? scratch.get<float2>((size_t)grid * nx * pl.H) : nullptr;
    hipError_t he = scratch.status();
    const PpFilter f{lp_kind, hp_kind, lp_a, lp_b, hp_a, hp_b};
    RA_LAUNCH(he, prep_filter_table_kernel, dim3((H * H + 255) / 256), dim3(256), 0, stream, d_tab, pl.P, f);
    if (he == hipSuccess) {
        const float *tab = d_tab;
        void *args_fixed[] = {&d_images, &n, &tab, &d_scr};
        PfPlan pl_arg = pl;
        void *args_plan[] = {&d_images, &n, &tab, &pl_arg, &d_scr};
        he = hipLaunchKernel(fk, dim3(grid), dim3(PF_THREADS), fixed ? args_fixed : args_plan, pl.lds, stream);
        if (he == hipSuccess) he = hipGetLastError();
    }
    return he == hipSuccess ? RA_OK : hip_error("ra_prep_filter", he);
}
