"""Inputs and expected outputs of the decision-stage tests (tests/test_decision_cases_cpu.py, tests/test_gpu_decision.py).

The decision stage turns candidate records into an assignment: finalize_kernel / finalize_wave_kernel with finalize_tail
(ralign_kernels.h), the exact reference spectra and their copy table (refspec_exact_kernel, ref_hash_kernel, ref_groups_kernel) and
the replay of float ties in refine_winner_kernel (ralign_exact.h).  This file restates the first as a plain sequential scan and the
last as the literal scan of the CPU path over the listed candidates, evaluated by the oracle; it builds the records and lists at
which the kernels branch.  Everything is seeded; nothing here needs a GPU."""
import functools
import math

import numpy as np

from cryo_ralib_amd import api, geometry, synth
from oracle import oracle as orc

M, F = api.RA_MODE_MREF, api.RA_MODE_REFFREE
f32 = np.float32
NEG = f32(-1.0e23)
TIE_RTOL, TIE_RTOL_OFFSETS, ALTS = f32(3.0e-6), f32(1.0e-5), api.REFINE_ALTS
POISON = f32(3.0e30)          # value of the records no scan may read: offsets outside the window, padding of the dense layout


class Geo:
    """the geometry of one engine as the kernels see it (DevGeom)"""

    def __init__(self, nx, ou, xr, mode, step=1.0, first_ring=1, skip=1, interp=orc.INTERP_BILINEAR):
        self.nx, self.ou, self.xr, self.mode, self.step, self.first_ring, self.skip, self.interp = nx, ou, xr, mode, step, first_ring, skip, interp
        self.rg = orc.rings(first_ring, ou, skip)
        self.numr = self.rg.numr_list()
        self.maxrin, self.lcirc = self.rg.maxrin, self.rg.lcirc
        self.cnx = nx // 2 + 1
        self.win_ring = ou if mode == M else self.numr[-3]          # particle_window: last_ring | the outermost sampled ring
        self.mashi = self.cnx - self.win_ring - 2
        self.shifts = geometry.shift_list(xr, xr, step)             # (ix, iy), y outer
        self.nk = int(xr / step)
        self.nshift = len(self.shifts)
        self.norm_ring = mode == M

    def engine_args(self, nref):
        return dict(nx=self.nx, last_ring=self.ou, xrng=self.xr, yrng=self.xr, step=self.step, nref=nref, mode=self.mode,
                    first_ring=self.first_ring, ring_skip=self.skip, interp=self.interp)

    def window(self, dx, dy):
        """(sxi, syi, lkx, rkx, lky, rky): the reset rule (multi-reference) or the clamp rule (reference-free), then search_range"""
        dx, dy = f32(dx), f32(dy)
        m = f32(self.mashi)
        if self.mode == M:
            if abs(dx) > m or abs(dy) > m:
                dx = dy = f32(0)
        else:
            dx, dy = min(max(dx, -m), m), min(max(dy, -m), m)
        tx = geometry.search_range(self.nx, self.win_ring, float(dx), self.xr)
        ty = geometry.search_range(self.nx, self.win_ring, float(dy), self.xr)
        return f32(dx), f32(dy), int(tx[0] / self.step), int(tx[1] / self.step), int(ty[0] / self.step), int(ty[1] / self.step)

    def live(self, w):
        """list indices of the in-window offsets in scan order (y outer, x inner)"""
        _, _, lkx, rkx, lky, rky = w
        n1 = 2 * self.nk + 1
        return [(iy + self.nk) * n1 + ix + self.nk for iy in range(-lky, rky + 1) for ix in range(-lkx, rkx + 1)]


def ent_stride(eng_path, nshift):
    """entries per particle of the dense layout: num_shifts on the size-generic path (search_path 2), else rounded up to 4"""
    return nshift if eng_path == 2 else (nshift + 3) // 4 * 4


def dense_layout(cand, stride):
    """[n][nshift][nrtile] -> [n][stride][nrtile], the padding offsets poisoned"""
    n, ns, nrt = cand.shape
    out = np.zeros((n, stride, nrt), api.CAND_DTYPE)
    out["val"] = POISON
    out[:, :ns] = cand
    return out


def live_layout(geo, cand, state):
    """the records of the in-window offsets only, particle after particle: [ent_base[n]][nrtile]"""
    return np.concatenate([cand[p, geo.live(geo.window(*state[p]))] for p in range(len(cand))])


# ---------------------------------------------------------------------------------------------------------------- finalize

def tie_threshold(geo, peak):
    """finalize_tail's thr in its float32 steps: peak - tol * |peak|"""
    tol = max(TIE_RTOL_OFFSETS, f32(f32(1.0e-7) * np.sqrt(f32(geo.lcirc)))) if geo.norm_ring else TIE_RTOL
    return f32(peak - f32(f32(tol) * abs(peak)))


def tail_terms(geo, jt, t7, bs, sxi, syi, mirror):
    """(alpha, tx, ty) of finalize_tail in float64 -- prb1d7, ang_n, the shift rotation (float products in the multi-reference
    entry point, doubles in ormq), combine_params2 -- and the magnitude of the terms each is summed from"""
    tot = f32(f32(jt) + f32(orc.prb1d7(np.asarray(t7, np.float64))))
    ang = f32(orc.ang_n(float(tot), geo.maxrin))
    a = float(ang) * math.pi / 180.0
    c, s = math.cos(a), math.sin(a)
    sx, sy = f32(-geo.shifts[bs][0]), f32(-geo.shifts[bs][1])
    if geo.mode == M:
        co, so = f32(c), f32(-s)
        sxs, sys = float(f32(f32(sx * co) - f32(sy * so))), float(f32(f32(sx * so) + f32(sy * co)))
    else:
        sxs, sys = float(sx) * c - float(sy) * -s, float(sx) * -s + float(sy) * c
    alpha, tx, ty, _ = orc.combine_params2(0.0, -float(sxi), -float(syi), 0, float(ang), sxs, sys, int(mirror))
    mag = abs(float(sxi)) + abs(float(syi)) + abs(sxs) + abs(sys)
    return (alpha % 360.0, tx, ty), (360.0, mag, mag)


def finalize_ref(geo, cand, state, thr, ref_dup, with_list=True, flags=None):
    """the sequential restatement of finalize_kernel: cand [n][nshift][nrtile] (CAND_DTYPE), state [n][2].
    Returns (results with float32(alpha, sx, sy), new state, refine list sorted by p, float64 (alpha, sx, sy) [n][3] and the term
    magnitudes [n][3]); flags: a list that receives per particle dict(c3, tie_bin, tie_rec, runner, copies, second, thr, nrec, ntie)"""
    n, _, nrt = cand.shape
    res = np.zeros(n, api.RESULT_DTYPE)
    st = np.zeros((n, 2), np.float32)
    rl = []
    v64, mag = np.zeros((n, 3)), np.zeros((n, 3))
    for p in range(n):
        w = geo.window(*state[p])
        live = geo.live(w)
        peak = second = NEG
        bs = brt = 0
        best = np.zeros((), api.CAND_DTYPE)
        best["val"], best["jtot"] = NEG, 1
        for s in live:
            for rt in range(nrt):
                v = cand[p, s, rt]["val"]
                if v >= peak:
                    second, peak, best, bs, brt = peak, v, cand[p, s, rt], s, rt
                elif v >= second:
                    second = v
        jword = int(best["jtot"])
        jt, ref, mirror = jword & 0x1fff, int(best["refmir"]) & 0xffff, int(best["refmir"]) >> 16
        v64[p], mag[p] = tail_terms(geo, jt, best["t7"], bs, w[0], w[1], mirror)
        res[p] = (f32(v64[p, 0]), f32(v64[p, 1]), f32(v64[p, 2]), mirror, ref, peak, jt, bs)
        st[p] = f32(w[0] + geo.shifts[bs][0]), f32(w[1] + geo.shifts[bs][1])
        if not with_list:
            continue
        b = best["t7"].astype(np.float32)
        c3 = f32(f32(f32(f32(f32(5) * b[0]) - f32(f32(3) * b[2])) - f32(f32(4) * b[3])) - f32(f32(3) * b[4])) + f32(f32(5) * b[6])
        tmax = max(f32(0), *[abs(x) for x in b])
        nb = max(NEG, *[b[k] for k in range(7) if k != 3])
        tie_bin = nb >= f32(b[3] - f32(TIE_RTOL * abs(b[3])))
        tthr = tie_threshold(geo, peak)
        tie_rec = second >= tthr
        runner = (jword >> 13) & 0xff
        copies = ref_dup is not None and (ref_dup[ref][0] != ref or ref_dup[ref][1] >= 0)
        if flags is not None:
            ntie = sum(1 for s in live for rt in range(nrt) if (s, rt) != (bs, brt) and cand[p, s, rt]["val"] >= tthr)
            flags.append(dict(c3=bool(abs(f32(c3)) < f32(f32(thr) * tmax)), tie_bin=bool(tie_bin), tie_rec=bool(tie_rec), runner=bool(runner),
                              copies=bool(copies), second=second, thr=tthr, nrec=len(live) * nrt, ntie=ntie, bs=bs, brt=brt, c3_value=float(c3)))
        if thr < 0 or abs(f32(c3)) < f32(f32(thr) * tmax) or tie_bin or tie_rec or runner or copies:
            rec = np.zeros((), api.REFINE_DTYPE)
            alts = []
            if runner:
                alts.append((bs, brt, (runner - 1) | (((jword >> 21) & 1) << 16)))
            if tie_rec:
                for s in live:
                    for rt in range(nrt):
                        cr = cand[p, s, rt]
                        if (s == bs and rt == brt) or not cr["val"] >= tthr:
                            continue
                        alts.append((s, rt, int(cr["refmir"])))
                        ru = (int(cr["jtot"]) >> 13) & 0xff
                        if ru:
                            alts.append((s, rt, (ru - 1) | (((int(cr["jtot"]) >> 21) & 1) << 16)))
            alts = alts[:ALTS]
            rec["p"], rec["ref"], rec["mirror"], rec["jtot"], rec["bs"], rec["brt"] = p, ref, mirror, jt, bs, brt
            rec["sxi"], rec["syi"], rec["nalt"] = w[0], w[1], len(alts)
            for k, a in enumerate(alts):
                rec["alt"][k] = a
            rl.append(rec)
    return res, st, (np.array(rl, api.REFINE_DTYPE) if rl else np.zeros(0, api.REFINE_DTYPE)), v64, mag


def near_f32_boundary(x, mag, rel=2.0 ** -45):
    """the float64 entries within rel x (the magnitude of their terms) of a float32 rounding boundary: where the device's double
    cos / sin / atan2 (one f64 ulp from the host's) may move the rounded result by one float32 ulp"""
    x = np.asarray(x, np.float64)
    r = x.astype(np.float32)
    out = np.zeros(x.shape, bool)
    for s in (-np.inf, np.inf):
        mid = (r.astype(np.float64) + np.nextafter(r, f32(s)).astype(np.float64)) / 2.0
        out |= np.abs(x - mid) <= rel * np.maximum(np.abs(x), mag)
    return out & (x != 0)          # (an exact zero is a sum of exact zeros on both sides)


def one_ulp_count(got, want):
    """entries of `got` that are not the bits of `want`; each must be one float32 ulp off (anything else fails)"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = got.view(np.int32) != want.view(np.int32)
    bad &= ~((got == 0) & (want == 0))
    one = (got == np.nextafter(want, f32(np.inf))) | (got == np.nextafter(want, f32(-np.inf)))
    assert not np.any(bad & ~one), (got[bad & ~one][:5], want[bad & ~one][:5])
    return int(bad.sum())


def parabola(v, a=0.05):
    """seven samples of a well-conditioned peak of height v: c3 = -84 a v, no neighbour within the tie tolerance"""
    k = np.arange(7) - 3
    return (f32(v) * (1.0 - a * k * k)).astype(np.float32)


# scenario names of the finalize batches, one per particle, repeated along the batch
SCENARIOS = ("plain", "all-equal", "equal-first-last", "equal-adjacent", "equal-cross-lane", "equal-same-lane", "nan", "nan-first",
             "bin-1", "bin-maxrin", "c3-zero", "flag-c3", "flag-tie-bin", "flag-tie-rec", "second-on-thr", "second-below-thr",
             "flag-runner", "flag-copies", "ten-ties", "runner-on-alt", "runner-on-winner-and-ties")
# states of the batch (dyadic: the window rule is exact in float32 and float64): centre, cut on each side, cut twice, beyond mashi
STATES = ((0, 0), (2.5, 0), (-2.5, 0), (0, 2.5), (0, -2.5), (2, 2), (-3, 3), (5, 0), (0.25, -7), (1.5, -2))
COPY_REF, PLAIN_REFS = 3, (0, 1, 2)          # FINALIZE_DUP: reference 3 has a copy (5); references 0 .. 2 have none
FINALIZE_NREF = 6


def finalize_dup():
    """the copy table of the finalize engines' references (finalize_refs): 3 and 5 are copies"""
    d = np.array([[r, -1] for r in range(FINALIZE_NREF)], np.int32)
    d[3], d[5] = (3, 5), (3, -1)
    return d


def finalize_refs(nx, ou):
    refs = synth.make_references(FINALIZE_NREF, nx, ou)
    refs[5] = refs[3]
    return refs


def finalize_batch(geo, n, nrtile, seed=0, states=STATES):
    """(cand [n][nshift][nrtile], state [n][2], scenario of every particle): particle p plays SCENARIOS[p % len] at
    states[(p // len(SCENARIOS) + p) % len(states)]; records outside its window are poisoned"""
    rng = np.random.Generator(np.random.PCG64(seed))
    cand = np.zeros((n, geo.nshift, nrtile), api.CAND_DTYPE)
    state = np.zeros((n, 2), np.float32)
    names = []
    for p in range(n):
        name = SCENARIOS[p % len(SCENARIOS)]
        names.append(name)
        state[p] = states[(p // len(SCENARIOS) + p) % len(states)]
        live = geo.live(geo.window(*state[p]))
        pos = [(s, rt) for s in live for rt in range(nrtile)]          # scan order
        nrec = len(pos)
        vals = (1.0 + rng.permutation(nrec) / max(nrec, 1)).astype(np.float32)          # distinct, 1 / nrec apart
        c = cand[p]
        c["val"] = POISON
        for i, (s, rt) in enumerate(pos):
            c[s, rt] = (vals[i], int(rng.integers(2, geo.maxrin)), int(rng.choice(PLAIN_REFS)) | (int(rng.integers(0, 2)) << 16),
                        parabola(vals[i]))
        order = np.argsort(vals)
        top = pos[order[-1]]                                            # the plain winner

        def put(i, v, t7=None):
            s, rt = pos[i % nrec]
            c[s, rt]["val"] = v
            c[s, rt]["t7"] = parabola(v) if t7 is None else t7

        hi = f32(3.0)
        if name == "all-equal":
            for i in range(nrec):
                put(i, hi)
        elif name == "equal-first-last":
            put(0, hi); put(nrec - 1, hi)
        elif name == "equal-adjacent":
            put(nrec // 2, hi); put(nrec // 2 + 1, hi)
        elif name == "equal-cross-lane":          # different lanes of the wave kernel, the later record in the LOWER lane
            put(5 if nrec <= 64 else 63, hi); put(nrec - 2 if nrec <= 64 else 64, hi); put(nrec // 3 if nrec <= 64 else 7, hi)
        elif name == "equal-same-lane":           # the same lane in two trips (li, li + 64) when there are that many
            put(1, hi); put(65 if nrec > 65 else nrec - 1, hi)
        elif name == "nan":
            put(nrec // 2, f32(np.nan))
        elif name == "nan-first":
            put(0, f32(np.nan)); put(nrec - 1, f32(np.nan))
        elif name == "bin-1":
            c[top]["jtot"] = 1
        elif name == "bin-maxrin":
            c[top]["jtot"] = geo.maxrin
        elif name == "c3-zero":                   # 5 b0 - 3 b2 - 4 b3 - 3 b4 + 5 b6 = 0 exactly, no neighbour near b3
            c[top]["t7"] = np.array([0.5, 0.25, 0, 1.25, 0, 0.25, 0.5], np.float32) * f32(2.0)
            c[top]["val"] = f32(2.5)
        elif name == "flag-c3":                   # |c3| / max |b| = 84e-4 < 0.02, neighbours 1e-4 below
            c[top]["t7"] = parabola(c[top]["val"], 1.0e-4)
        elif name == "flag-tie-bin":
            c[top]["t7"] = (f32(c[top]["val"]) * np.array([0.5, 0.7, 1 - 1e-6, 1, 0.6, 0.4, 0.2])).astype(np.float32)
        elif name in ("flag-tie-rec", "second-on-thr", "second-below-thr", "ten-ties", "runner-on-alt", "runner-on-winner-and-ties"):
            peak = f32(2.5)
            thr = tie_threshold(geo, peak)
            c[top]["val"], c[top]["t7"] = peak, parabola(peak)
            others = [i for i in range(nrec) if pos[i] != top]
            if name == "flag-tie-rec" and others:
                put(others[len(others) // 2], f32(peak - f32(0.3) * f32(peak - thr)))
            elif name == "second-on-thr" and others:
                put(others[0], thr)
            elif name == "second-below-thr" and others:
                put(others[-1], np.nextafter(thr, f32(-np.inf)))
            else:
                for k, i in enumerate(others[:10] if name == "ten-ties" else others[:3]):
                    put(i, f32(peak - f32(0.1 * (k % 5 + 1)) * f32(peak - thr)))
                    s, rt = pos[i]
                    if name != "ten-ties" and k == 1:          # a runner-up word on an alternate: reference 2, mirrored, bin 77
                        c[s, rt]["jtot"] = (int(c[s, rt]["jtot"]) & 0x1fff) | ((2 + 1) << 13) | (1 << 21) | (77 << 22)
                if name == "runner-on-winner-and-ties":
                    c[top]["jtot"] = (int(c[top]["jtot"]) & 0x1fff) | ((1 + 1) << 13) | (0 << 21) | (5 << 22)
        elif name == "flag-runner":               # a runner-up word on the winner: reference 0, mirrored, bin 9
            c[top]["jtot"] = (int(c[top]["jtot"]) & 0x1fff) | ((0 + 1) << 13) | (1 << 21) | (9 << 22)
        elif name == "flag-copies":
            c[top]["refmir"] = COPY_REF | (int(c[top]["refmir"]) >> 16 << 16)
    return cand, state, names


# ---------------------------------------------------------------------------------------------------------------- ref_dup

def dup_table(groups, nref):
    """(first copy, next copy or -1) of every reference; groups: lists of references that are copies of each other"""
    d = np.array([[r, -1] for r in range(nref)], np.int32)
    for g in groups:
        g = sorted(g)
        for k, r in enumerate(g):
            d[r] = g[0], (g[k + 1] if k + 1 < len(g) else -1)
    return d


# name: (nref, groups of copies)
DUP_CASES = {
    "none": (5, []),
    "groups-3-7-9": (23, [[1, 4, 20], [0, 3, 5, 8, 9, 13, 22], [2, 6, 7, 10, 11, 12, 14, 15, 21]]),
    "all-equal": (11, [list(range(11))]),
    "stride-256": (257, [[0, 256]]),
}


def dup_refs(name, nx, ou):
    """distinct seeded images, the members of a group all equal to the group's first"""
    nref, groups = DUP_CASES[name]
    refs = synth.make_references(nref, nx, ou)
    for g in groups:
        for r in g:
            refs[r] = refs[min(g)]
    return refs


# ---------------------------------------------------------------------------------------------------------------- replay

def prepare(geo, refs):
    """(references as the engine takes them, their prepared spectra): normalize.mask under model_circle, Polar2Dm, Frngs, Applyws"""
    return orc.prepare_refs(refs, orc.model_circle(geo.ou, geo.nx, geo.nx), geo.rg, geo.interp)


class Replay:
    """the CPU path's evaluation of the candidates of one engine: references prepared by the oracle, particles as given"""

    def __init__(self, geo, refs, parts, dup=None, prepared=None):
        self.geo, self.parts, self.dup = geo, np.ascontiguousarray(parts, np.float32), dup
        self.refs_n, self.cref = prepared if prepared is not None else prepare(geo, refs)
        self._ev = {}

    def spectrum(self, p, sxi, syi, bs):
        g = self.geo
        cx = f32(f32(f32(g.cnx) + f32(sxi)) + g.shifts[bs][0])
        cy = f32(f32(f32(g.cnx) + f32(syi)) + g.shifts[bs][1])
        circ = orc.polar2dm(self.parts[p], float(cx), float(cy), g.rg, g.interp)
        if g.norm_ring:
            circ = orc.normalize_ring(circ, g.rg)
        return orc.frngs(circ, g.rg)

    def evaluate(self, p, sxi, syi, bs, ref):
        """Crosrng_ms of particle p at offset bs against reference ref: qn, qm, jn, jm, tot, tmt"""
        key = (p, float(sxi), float(syi), bs, ref)
        if key not in self._ev:
            self._ev[key] = orc.crosrng_ms(self.cref[ref], self.spectrum(p, sxi, syi, bs), self.geo.rg)
        return self._ev[key]

    def group(self, ref):
        """the copies of a reference, ascending (itself alone without a table)"""
        if self.dup is None:
            return [ref]
        out, r = [], int(self.dup[ref][0])
        while r >= 0:
            out.append(r)
            r = int(self.dup[r][1])
        return out

    def scan(self, rec, cls=None, listed_only=False, float_peak=None, capacity=None):
        """the literal scan of Util::multiref_polar_ali_2d (float peak) or ormq (double peak) over the (offset, reference) pairs
        the record lists -- copies included -- in ascending order.  listed_only: the orientations the record lists only, as the
        kernel sees them; capacity: the first `capacity` entries of the expansion (the list the kernel had until this test).
        Returns dict(ref, mirror, jtot, bs, tot, q) of the winner"""
        cands = [(int(rec["bs"]), int(rec["ref"]), int(rec["mirror"]))]
        cands += [(int(a["bs"]), int(a["refmir"]) & 0xffff, int(a["refmir"]) >> 16) for a in rec["alt"][:int(rec["nalt"])]]
        p, sxi, syi = int(rec["p"]), rec["sxi"], rec["syi"]
        float_peak = self.geo.mode == M if float_peak is None else float_peak
        entries = []
        for bs, ref, mir in cands:
            for r2 in (self.group(ref) if cls is None else [ref]):
                entries.append((bs, r2, mir))
        if capacity is not None:
            entries = entries[:capacity]
        peak, win = -1.0e23, None
        for bs, r2 in sorted({(e[0], e[1]) for e in entries}):
            ev = self.evaluate(p, sxi, syi, bs, r2 if cls is None else int(cls[p]))
            qn, qm = ev["qn"], ev["qm"]
            if listed_only:
                if (bs, r2, 0) not in entries:
                    qn = -1.0e300
                if (bs, r2, 1) not in entries:
                    qm = -1.0e300
            if qn >= peak or qm >= peak:
                if qn >= qm:
                    win = dict(ref=r2, mirror=0, jtot=ev["jn"], bs=bs, tot=ev["tot"], q=qn)
                else:
                    win = dict(ref=r2, mirror=1, jtot=ev["jm"], bs=bs, tot=ev["tmt"], q=qm)
                peak = float(f32(win["q"])) if float_peak else win["q"]
        return win

    def expected(self, rec, prior, state, cls=None):
        """what refine_winner_kernel leaves for the record: (result record, state [2], float64 (alpha, sx, sy), changed)"""
        g = self.geo
        if int(rec["nalt"]) == 0 and (cls is not None or len(self.group(int(rec["ref"]))) == 1):
            ev = self.evaluate(int(rec["p"]), rec["sxi"], rec["syi"], int(rec["bs"]), int(rec["ref"]) if cls is None else int(cls[int(rec["p"])]))
            m = int(rec["mirror"])          # one candidate: no scan, the record's orientation
            w = dict(ref=int(rec["ref"]), mirror=m, jtot=ev["jm" if m else "jn"], bs=int(rec["bs"]), tot=ev["tmt" if m else "tot"],
                     q=ev["qm" if m else "qn"])
        else:
            w = self.scan(rec, cls)
        ang = f32(orc.ang_n(float(f32(w["tot"])), g.maxrin))
        a = float(ang) * math.pi / 180.0
        c, s = math.cos(a), math.sin(a)
        sx, sy = f32(-g.shifts[w["bs"]][0]), f32(-g.shifts[w["bs"]][1])
        if g.mode == M:
            co, so = f32(c), f32(-s)
            sxs, sys = float(f32(f32(sx * co) - f32(sy * so))), float(f32(f32(sx * so) + f32(sy * co)))
        else:
            sxs, sys = float(sx) * c - float(sy) * -s, float(sx) * -s + float(sy) * c
        alpha, tx, ty, _ = orc.combine_params2(0.0, -float(rec["sxi"]), -float(rec["syi"]), 0, float(ang), sxs, sys, w["mirror"])
        out = prior.copy()
        out["alpha"], out["sx"], out["sy"] = f32(alpha % 360.0), f32(tx), f32(ty)
        changed = (w["jtot"], w["bs"], w["ref"], w["mirror"]) != (int(rec["jtot"]), int(rec["bs"]), int(rec["ref"]), int(rec["mirror"]))
        st = np.array(state, np.float32)
        if changed:
            out["angle_bin"], out["shift_idx"], out["mirror"], out["peak"] = w["jtot"], w["bs"], w["mirror"], f32(w["q"])
            if cls is None:
                out["ref_id"] = w["ref"]
            st = np.array([f32(rec["sxi"] + g.shifts[w["bs"]][0]), f32(rec["syi"] + g.shifts[w["bs"]][1])], np.float32)
        return out, st, (alpha % 360.0, tx, ty), changed, w


def ccf(geo, c1, c2, mirror):
    """the rotational CCF of Crosrng_ms in float64 from two ring sets in EMAN2 packing (float32 products, as the CPU path forms
    them): q (straight) or t (mirrored), all maxrin samples, by direct summation of the inverse real DFT"""
    N = geo.maxrin
    re, im = np.zeros(N // 2 + 1), np.zeros(N // 2 + 1)
    for i in range(len(geo.numr) // 3):
        o, n = geo.numr[3 * i + 1] - 1, geo.numr[3 * i + 2]
        a, d = np.asarray(c1[o:o + n], np.float32), np.asarray(c2[o:o + n], np.float32)
        re[0] += float(a[0] * d[0])
        re[n // 2] += float(a[1] * d[1])
        k = np.arange(1, n // 2)
        p1, p2, p3, p4 = a[2 * k] * d[2 * k], a[2 * k + 1] * d[2 * k + 1], a[2 * k] * d[2 * k + 1], a[2 * k + 1] * d[2 * k]
        if mirror:
            re[k] += (p1 - p2).astype(np.float64); im[k] += (-p3 - p4).astype(np.float64)
        else:
            re[k] += (p1 + p2).astype(np.float64); im[k] += (-p3 + p4).astype(np.float64)
    m = np.arange(N)[:, None]
    k = np.arange(1, N // 2)[None, :]
    w = 2.0 * np.pi * ((k * m) % N) / N
    acc = (re[1:N // 2][None, :] * np.cos(w) - im[1:N // 2][None, :] * np.sin(w)).sum(1)
    return (re[0] + np.where(np.arange(N) % 2, -re[N // 2], re[N // 2]) + 2.0 * acc) / N


def c3_ratio(q, jtot):
    """|c3| / max |b| of prb1d7 on the seven samples around bin jtot (1-based)"""
    b = q[(jtot - 1 + np.arange(-3, 4)) % len(q)]
    return abs(5 * b[0] - 3 * b[2] - 4 * b[3] - 3 * b[4] + 5 * b[6]) / np.abs(b).max()


def make_rec(p, bs, ref, mirror, jtot, alts=(), sxi=0.0, syi=0.0):
    rec = np.zeros((), api.REFINE_DTYPE)
    rec["p"], rec["ref"], rec["mirror"], rec["jtot"], rec["bs"], rec["sxi"], rec["syi"], rec["nalt"] = p, ref, mirror, jtot, bs, sxi, syi, len(alts)
    for k, (abs_, aref, amir) in enumerate(alts):
        rec["alt"][k] = (abs_, 0, aref | (amir << 16))
    return rec


def fourier_shift(img, dx, dy):
    """img moved by (dx, dy) pixels, float64 Fourier interpolation, rounded to float32: a smooth function of the shift"""
    ny, nx = img.shape
    ky, kx = np.fft.fftfreq(ny)[:, None], np.fft.fftfreq(nx)[None, :]
    return np.fft.ifft2(np.fft.fft2(img.astype(np.float64)) * np.exp(-2j * np.pi * (kx * dx + ky * dy))).real.astype(np.float32)


def tuned_tie(geo, prepared, ref, bs_a, bs_b, want, seed=0, iters=40):
    """a particle -- reference `ref` turned by 40 degrees and moved to about half way between the offsets bs_a < bs_b, plus seeded
    noise -- whose straight peaks at the two offsets round to ONE float32 while the doubles differ, found by bisection on the
    sub-pixel shift.  want = "up": float32(qn_a) > qn_b >= qn_a (the float rule keeps a, the doubles take b); "down":
    float32(qn_a) <= qn_b < qn_a (the float rule takes b, the doubles keep a).  Returns the particle, or None for this seed"""
    rng = np.random.Generator(np.random.PCG64(seed))
    refs_n = prepared[0]
    base = synth.rot_shift2d_np(refs_n[ref], 40.0, 0.0, 0.0, 0) + (0.05 * rng.standard_normal(refs_n[ref].shape)).astype(np.float32)
    mid = (geo.shifts[bs_a] + geo.shifts[bs_b]) / 2.0

    def diff(eps):
        part = fourier_shift(base, mid[0] + eps, mid[1])
        rp = Replay(geo, None, part[None], None, prepared)
        return part, rp.evaluate(0, 0.0, 0.0, bs_a, ref)["qn"], rp.evaluate(0, 0.0, 0.0, bs_b, ref)["qn"]

    lo, hi = -0.4, 0.4
    slo, shi = diff(lo), diff(hi)
    slo, shi = slo[2] - slo[1] > 0, shi[2] - shi[1] > 0
    if slo == shi:
        return None
    for _ in range(iters):
        e = 0.5 * (lo + hi)
        part, a, b = diff(e)
        if f32(a) == f32(b):
            fa = float(f32(a))
            if (want == "up" and fa > b >= a and b != a) or (want == "down" and fa <= b < a):
                return part
        if (b - a > 0) == slo:
            lo = e
        else:
            hi = e
    return None


@functools.lru_cache(maxsize=None)
def tie_particle(nx, ou, xr, mode, want, ref=1, bs_a=None, max_seed=64):
    """tuned_tie over seeds 0, 1, ..: (particle, seed, bs_a, bs_b) of the first that has the tie; offsets: the centre and its right
    neighbour"""
    geo = Geo(nx, ou, xr, mode)
    prepared = prepare(geo, synth.make_references(TIE_NREF, nx, ou))
    a = geo.nshift // 2 if bs_a is None else bs_a
    for seed in range(max_seed):
        part = tuned_tie(geo, prepared, ref, a, a + 1, want, seed)
        if part is not None:
            return part, seed, a, a + 1
    return None


TIE_NREF = 4


# the reference stack of the replay engines: a group of 9 copies, a pair, three references without a copy
REPLAY_NREF = 14
GROUP9, PAIR, SINGLE = [1, 3, 4, 5, 7, 8, 10, 11, 13], [2, 9], [0, 6, 12]
PRIOR = dict(alpha=-1.0, sx=-2.0, sy=-3.0, peak=-4.0)          # what the result holds before the replay; state: (-9, -9)
PRIOR_STATE = (-9.0, -9.0)


def replay_refs(nx, ou):
    refs = synth.make_references(REPLAY_NREF, nx, ou)
    for g in (GROUP9, PAIR):
        for r in g:
            refs[r] = refs[g[0]]
    return refs


def replay_dup():
    return dup_table([GROUP9, PAIR], REPLAY_NREF)


def planted(refs_n, ref, seed, ang=None, mirror=0, shift=(0.0, 0.0), sigma=0.05):
    """reference `ref` turned, mirrored and moved, plus seeded noise"""
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    ang = float(rng.uniform(20.0, 340.0)) if ang is None else ang
    img = synth.rot_shift2d_np(refs_n[ref], ang, 0.0, 0.0, mirror)
    return fourier_shift(img + (sigma * rng.standard_normal(img.shape)).astype(np.float32), *shift)


def ranked_offsets(rp, p, ref, sxi=0.0, syi=0.0):
    """the offsets of the full window by the better of (qn, qm) of particle p against `ref`, best first: (bs, mirror, jtot, q)"""
    out = []
    for bs in range(rp.geo.nshift):
        ev = rp.evaluate(p, sxi, syi, bs, ref)
        m = 0 if ev["qn"] >= ev["qm"] else 1
        out.append((bs, m, ev["jm" if m else "jn"], ev["qm" if m else "qn"]))
    return sorted(out, key=lambda t: -t[3])


def rounded_up(q):
    return float(f32(q)) > q


@functools.lru_cache(maxsize=None)
def replay_cases(nx, ou, xr, mode, full=True):
    """(Replay, list of (name, record, class or None)) of one replay engine: particle k belongs to case k.  full = False: the three
    particles of the large geometry (one candidate, two offsets the wrong way round, copies)"""
    geo = Geo(nx, ou, xr, mode)
    prepared = prepare(geo, replay_refs(nx, ou))
    refs_n = prepared[0]
    parts, cases = [], []

    def probe(img):
        return Replay(geo, None, img[None], replay_dup(), prepared)

    def add(name, img, build, cls=None):
        p = len(parts)
        parts.append(img)
        rec = build(p, ranked_offsets(probe(img), 0, cls if cls is not None else build.ref, *build.pre))
        rec["sxi"], rec["syi"] = build.pre
        cases.append((name, rec, cls))

    def case(ref, sxi=0.0, syi=0.0):          # (sxi, syi): the pre-shift of the record, dyadic
        def deco(fn):
            fn.ref, fn.pre = ref, (sxi, syi)
            return fn
        return deco

    def pick(ref, pred, **kw):
        """the first seeded particle of reference `ref` whose ranking satisfies pred"""
        for seed in range(64):
            img = planted(refs_n, ref, seed, **kw)
            if pred(ranked_offsets(probe(img), 0, ref)):
                return img
        raise AssertionError("no particle of reference %d with the wanted property" % ref)

    @case(0)
    def correct(p, rk):
        return make_rec(p, rk[0][0], 0, rk[0][1], rk[0][2])
    add("nalt0-correct", planted(refs_n, 0, 1), correct)

    @case(6, 0.5, -1.0)
    def swapped(p, rk):          # the record holds the second-best offset, the alternate the best
        return make_rec(p, rk[1][0], 6, rk[1][1], rk[1][2], [(rk[0][0], 6, rk[0][1])])
    add("nalt1-swapped", planted(refs_n, 6, 2, mirror=1, shift=(0.3, -0.2)), swapped)

    @case(PAIR[0])
    def copies_down(p, rk):
        return make_rec(p, rk[0][0], PAIR[0], rk[0][1], rk[0][2])
    add("copies-last-wins", pick(PAIR[0], lambda rk: not rounded_up(rk[0][3])), copies_down)
    if not full:
        return Replay(geo, None, np.array(parts), replay_dup(), prepared), cases

    @case(PAIR[0])
    def copies_up(p, rk):          # listed as the LATER copy: the float rule keeps the first
        return make_rec(p, rk[0][0], PAIR[1], rk[0][1], rk[0][2])
    add("copies-first-stays", pick(PAIR[0], lambda rk: rounded_up(rk[0][3])), copies_up)

    @case(0)
    def wrong_jtot(p, rk):
        return make_rec(p, rk[0][0], 0, rk[0][1], (rk[0][2] + 4) % geo.maxrin + 1)
    add("wrong-jtot", planted(refs_n, 0, 3), wrong_jtot)

    @case(12)
    def wrong_mirror(p, rk):          # straight and mirrored entries of one (offset, reference), the record's the wrong one
        return make_rec(p, rk[0][0], 12, 1 - rk[0][1], rk[0][2], [(rk[0][0], 12, rk[0][1])])
    add("wrong-mirror", planted(refs_n, 12, 4, mirror=1), wrong_mirror)

    @case(6)
    def nalt1(p, rk):
        return make_rec(p, rk[0][0], 6, rk[0][1], rk[0][2], [(rk[1][0], 6, rk[1][1])])
    add("nalt1-kept", planted(refs_n, 6, 5, shift=(-0.4, 0.1)), nalt1)

    @case(0, -0.75, 0.25)
    def nalt7(p, rk):          # seven alternates over three references, the best offset last, both orientations of the third offset
        alts = [(rk[3][0], 6, 0), (rk[2][0], 0, rk[2][1]), (rk[2][0], 0, 1 - rk[2][1]), (rk[4][0], 12, 1), (rk[1][0], 0, rk[1][1]),
                (rk[5][0], 0, rk[5][1]), (rk[0][0], 0, rk[0][1])]
        return make_rec(p, rk[6][0], 0, rk[6][1], rk[6][2], alts)
    add("nalt7", planted(refs_n, 0, 6, shift=(0.5, 0.5)), nalt7)

    @case(12)
    def twice(p, rk):          # one candidate listed twice, and the record's own candidate again
        a = (rk[1][0], 12, rk[1][1])
        return make_rec(p, rk[0][0], 12, rk[0][1], rk[0][2], [a, a, (rk[0][0], 12, rk[0][1])])
    add("listed-twice", planted(refs_n, 12, 7), twice)

    for want in ("up", "down"):          # two offsets whose peaks round to one float32 (tuned_tie), the later one in the record
        found = None
        for seed in range(64):
            img = tuned_tie(geo, prepared, 0, geo.nshift // 2, geo.nshift // 2 + 1, want, seed)
            if img is not None:
                found = img
                break
        assert found is not None, want
        a, b = geo.nshift // 2, geo.nshift // 2 + 1

        @case(0)
        def tie(p, rk, a=a, b=b):
            ev = probe(parts[p]).evaluate(0, 0.0, 0.0, b, 0)
            return make_rec(p, b, 0, 0, ev["jn"], [(a, 0, 0)])
        add("tie-rounded-" + want, found, tie)

    @case(GROUP9[4])
    def overflow(p, rk):          # 8 candidates x 9 copies = 72 entries; the best offset is the last alternate
        refs8 = [GROUP9[(3 * k + 4) % 9] for k in range(8)]
        alts = [(rk[7 - k][0], refs8[k], rk[7 - k][1]) for k in range(1, 8)]
        return make_rec(p, rk[7][0], refs8[0], rk[7][1], rk[7][2], alts)
    add("overflow-72", pick(GROUP9[0], lambda rk: not rounded_up(rk[0][3]), shift=(0.5, 0.0)), overflow)

    @case(PAIR[0])
    def resident(p, rk):          # class-resident: the class has a copy in the stack, which takes no part
        return make_rec(p, rk[0][0], PAIR[0], rk[0][1], rk[0][2], [(rk[1][0], PAIR[0], rk[1][1])])
    add("class-resident-copies", pick(PAIR[0], lambda rk: not rounded_up(rk[0][3])), resident, cls=PAIR[0])
    return Replay(geo, None, np.array(parts), replay_dup(), prepared), cases


def replay_prior(rec):
    """the result record and state a replay starts from"""
    r = np.zeros((), api.RESULT_DTYPE)
    r["alpha"], r["sx"], r["sy"], r["peak"] = PRIOR["alpha"], PRIOR["sx"], PRIOR["sy"], PRIOR["peak"]
    r["mirror"], r["ref_id"], r["angle_bin"], r["shift_idx"] = rec["mirror"], rec["ref"], rec["jtot"], rec["bs"]
    return r, np.array(PRIOR_STATE, np.float32)
