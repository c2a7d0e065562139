// The planner of the search path, host code only: the environment switches of one call (PlanSwitches), what a caller asks of a plan
// (PlanRequest) and the CLASS condition of every kernel family -- ring length, ring-count limit, shortest ring, reference count and
// the family's switches -- written once, for the engine (ra_create_ex, ra_reset_shifts) and for the device-free estimate
// (resident_expected) alike.  Whether a family's LDS plan then fits is decided where its tables are (ralign_engine.hip).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "../../include/ralign.h"
#include "ralign_geom.h"
#include "ralign_fused.h"
#include "ralign_tiled.h"
#include "ralign_solo.h"
#include "ralign_pair.h"

namespace ralign {

inline int env_int(const char *name, int unset) { const char *v = getenv(name); return v ? atoi(v) : unset; }
inline bool env_set(const char *name) { return getenv(name) != nullptr; }

// The user-facing switches (README "Environment"), read ONCE at the start of a call that plans -- ra_create_ex, ra_reset_shifts,
// ra_planned_workspace_bytes -- and passed down; never kept across calls (tests flip them between two engines of a process).
// The experiment switches of profiling builds (RA_EXP_ENV) stay where they are used.
struct PlanSwitches {
    bool generic, fused, solo, pair, duo, tcrop, crop, tight_rings, zones, live_offsets, gccf_split, refine_gm, atomic_sums, info;
    int tiled;              // RALIGN_TILED: < 0 not set, 0 never, > 0 also below RT_MINREF references
    int gccf_tm;            // RALIGN_GCCF_TM (gccf_tm), 0: not set
    int solo_jobs;          // RALIGN_SOLO_JOBS (1: the light ring jobs only)
    int grid;               // RALIGN_GRID: persistent workgroups (experiments), <= 0: one per CU
    const char *refine;     // RALIGN_REFINE: the refinement threshold as text, null: not set
};
inline PlanSwitches read_switches()
{
    PlanSwitches s{};
    s.generic = env_int("RALIGN_GENERIC", 0) != 0;
    s.fused = env_int("RALIGN_FUSED", 1) != 0;
    s.solo = env_int("RALIGN_SOLO", 1) != 0;
    s.pair = env_int("RALIGN_PAIR", 1) != 0;
    s.duo = env_int("RALIGN_DUO", 1) != 0;
    s.tcrop = env_int("RALIGN_TCROP", 1) != 0;
    s.crop = env_int("RALIGN_CROP", 1) != 0;
    s.tight_rings = env_int("RALIGN_TIGHT_RINGS", 1) != 0;
    s.zones = env_int("RALIGN_ZONES", 1) != 0;
    s.live_offsets = env_int("RALIGN_LIVE_OFFSETS", 1) != 0;
    s.gccf_split = env_int("RALIGN_GCCF_SPLIT", 1) != 0;
    s.refine_gm = env_int("RALIGN_REFINE_GM", 0) != 0;
    s.atomic_sums = env_int("RALIGN_ATOMIC_SUMS", 0) != 0;
    s.info = env_set("RALIGN_INFO");
    s.tiled = !env_set("RALIGN_TILED") ? -1 : env_int("RALIGN_TILED", 0) != 0 ? 1 : 0;
    s.gccf_tm = env_int("RALIGN_GCCF_TM", 0);
    s.solo_jobs = env_int("RALIGN_SOLO_JOBS", 0);
    s.grid = env_int("RALIGN_GRID", 0);
    s.refine = getenv("RALIGN_REFINE");
    return s;
}

// What one plan is made for.  ra_create_ex fills it and hands copies to its attempts; ra_reset_shifts fills it from the engine.
struct PlanRequest {
    PlanSwitches sw;
    bool option_generic;    // engine options that only the size-generic kernels implement (RA_INTERP_QUADRI)
    bool generic_class;     // plan in the size-generic CLASS (crop / pair kernels allowed) although the LDS-resident kernels would hold
                            // the image: the second attempt of ra_create_ex for more than RF_MAXREF references
    bool allow_tcrop;       // false: the crop plan missed the real tables once (first retry of ra_create_ex)
    // the size-generic kernels for a geometry the LDS-resident ones cover: the option or RALIGN_GENERIC=1.  Both turn off the pair
    // kernel, the crop plan and the LDS-resident kernels; the 512-sample class (solo / duo) yields to the OPTION alone.
    bool generic_forced() const { return option_generic || sw.generic; }
};

// search_tiled_kernel by the reference count alone: from RT_MINREF on (from 15 references on: search_fused_kernel needs two spectra
// rounds per pass from 12 on and is 4 % slower at 15 and 16), RALIGN_TILED=1 also below, RALIGN_TILED=0 never.  The crop path
// (tcrop_wanted, setup_fused) asks no more than this: the tiled plan decides there.
inline bool tiled_by_count(const ra_config &cfg, const PlanRequest &rq)
{
    return rq.sw.tiled != 0 && (cfg.nref >= RT_MINREF || rq.sw.tiled > 0);
}
// ... and over the whole image: rings of 256 samples, slices of at most 36 rings
inline bool tiled_class(const Geometry &g, const ra_config &cfg, const PlanRequest &rq)
{
    return tiled_by_count(cfg, rq) && g.maxrin == 256 && g.nring <= 4 * RT_NQ && cfg.nref <= 127;
}
// a particle-resident kernel over the whole image (search_fused_kernel up to RF_MAXREF references, or the tiled one)
inline bool fused_class(const Geometry &g, const ra_config &cfg, const PlanRequest &rq, bool generic)
{
    if (generic || !rq.sw.fused) return false;
    return tiled_class(g, cfg, rq) || (cfg.nref <= RF_MAXREF && (g.maxrin == 256 || g.maxrin == 128));
}
// search_solo_kernel / search_duo_kernel: the size-generic class with rings that end at 512 samples (RALIGN_SOLO=0: the generic kernels)
inline bool solo_class(const Geometry &g, const ra_config &cfg, const PlanRequest &rq, bool generic)
{
    return generic && g.maxrin == 512 && g.nring <= 4 * RS_NQ && g.numr[2] >= 8 && cfg.nref <= 127 && !rq.option_generic && rq.sw.solo;
}
// two offsets per pass (search_duo_kernel, ralign_duo.h) for the solo class: the default (measured against search_solo_kernel:
// +4.5 % at 128 / 60 / nref 10, +24 % at 130 / 52 / nref 50); RALIGN_DUO=0: one offset per pass
inline bool duo_class(const Geometry &g, const ra_config &cfg, const PlanRequest &rq, bool generic)
{
    return solo_class(g, cfg, rq, generic) && rq.sw.duo;
}
// search_pair_kernel: the size-generic class with rings that end at 256 samples -- a box too large for the four ring buffers of the
// LDS-resident kernels (RALIGN_PAIR=0: the generic kernels)
inline bool pair_class(const Geometry &g, const ra_config &cfg, const PlanRequest &rq, bool generic)
{
    return generic && g.maxrin == 256 && g.nring <= 4 * RP_NQ && g.numr[2] >= 8 && cfg.nref <= 127 && !rq.generic_forced() && rq.sw.pair;
}
// search_tiled_kernel / search_fused_kernel over a crop of the image for the same class (RALIGN_TCROP=0: the pair kernel)
// (search_tiled_kernel holds slices of at most 36 rings, search_fused_kernel reads its operand from the ring buffers: up to 64)
inline bool tcrop_class(const Geometry &g, const ra_config &cfg, const PlanRequest &rq, bool generic)
{
    return generic && g.maxrin == 256 && g.nring <= 64 && g.numr[2] >= 8 && cfg.nref <= 127 && !rq.generic_forced() &&
           rq.allow_tcrop && rq.sw.tcrop && rq.sw.fused;
}

// Tap source of search_fused_kernel's short rings (its TAPL1): rings of at most 64 or 128 samples may read their taps from the
// particle's image in global memory, which has no zero border -- a tap outside the image would read the neighbouring particle, or
// past the allocation behind the last one.  A ring of radius r qualifies when no tap of any sample can leave the image for any
// search offset and any state the window rule admits: particle_window resets (RA_MODE_MREF) or clamps (RA_MODE_REFFREE) the state to
// |d| <= mashi = cn - win_ring - 2, an offset adds at most ceil(range), a sample at most r, and the right / lower taps of the
// interpolation are x + 1 / y + 1 (the zero-weight tap one past a sample that lands on a pixel counts).  One-based, as integers:
//   cn - mashi - ceil(xr) - r >= 1   and   cn + mashi + ceil(xr) + r + 1 <= nx,   and the same in y with yr.
// mashi: l1_tap_mashi -- the wider of the two modes' windows, since ra_engine_switch_mode changes the mode of a standing plan (at
// ring step 1 both are cn - last_ring - 2).
// The rule is all or nothing per engine: the largest setting T of {128, 64} up to `cap` whose rings of at most T samples ALL
// qualify, else 0.  numr: (radius, offset, length) per ring.
constexpr int kTapL1Cap = 128;      // the largest setting the dispatch instantiates (select_fused)
inline int l1_tap_mashi(const std::vector<int> &numr, int nring, int nx, int last_ring)
{
    const int cn = nx / 2 + 1;
    return std::max(std::abs(cn - last_ring - 2), std::abs(cn - numr[3 * (nring - 1)] - 2));
}
inline bool l1_tap_ring_ok(int nx, int mashi, float xrng, float yrng, int r)
{
    const int cn = nx / 2 + 1, ax = mashi + (int)std::ceil(xrng), ay = mashi + (int)std::ceil(yrng);
    return cn - ax - r >= 1 && cn + ax + r + 1 <= nx && cn - ay - r >= 1 && cn + ay + r + 1 <= nx;
}
inline int l1_tap_rings(const std::vector<int> &numr, int nring, int nx, int last_ring, float xrng, float yrng, int cap = kTapL1Cap)
{
    const int mashi = l1_tap_mashi(numr, nring, nx, last_ring);
    for (int T : {128, 64}) {
        if (T > cap) continue;
        bool ok = true;
        for (int i = 0; i < nring && ok; i++)
            if (numr[3 * i + 2] <= T && !l1_tap_ring_ok(nx, mashi, xrng, yrng, numr[3 * i])) ok = false;
        if (ok) return T;
    }
    return 0;
}

// ring quads of the B stream of the particle-resident kernels, summed over the groups of 16 bins (rf_layout_b lays them out so):
// a group holds the rings long enough to reach its first bin
inline size_t b_stream_quads(const Geometry &g)
{
    size_t quads = 0;
    for (int m = 0; m < g.maxrin / 32; m++) {
        int r0 = 0;
        while (r0 < g.nring) {
            const int n = g.numr[3 * r0 + 2], nbin = (n == g.maxrin) ? n / 2 : n / 2 + 1;
            if (16 * m < nbin) break;
            r0++;
        }
        quads += (g.nring - r0 + 3) / 4;
    }
    return quads;
}

}  // namespace ralign
