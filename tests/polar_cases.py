"""Shared by tests/test_polar_cases_cpu.py and tests/test_gpu_polar_edges.py (no tests here): the case table of the size-generic
polar stage (polar_zone_kernel / polar_generic_kernel), the float64 reference of Polar2Dm -> (Normalize_ring) -> Frngs, the per-ring
error measure and the window rule restated on the host.

The reference takes the sample POSITIONS as the CPU oracle forms them (oracle/ralign_oracle.c: orc_polar2dm) -- float32 sinf / cosf
of a float32 angle, times the radius, plus a float32 centre -- and does everything behind them in float64: the interpolation, the
weighted mean and sigma of Normalize_ring, and every ring's real FFT (numpy.fft.rfft) in EMAN2's packed layout (slot 0 = Re X0,
slot 1 = Re X(n/2), slot 2k = Re Xk, slot 2k + 1 = Im Xk)."""
import ctypes
import ctypes.util
import math

import numpy as np

from cryo_ralib_amd import api, geometry, synth

M, F = api.RA_MODE_MREF, api.RA_MODE_REFFREE
BIL, QUADRI = api.RA_INTERP_BILINEAR, api.RA_INTERP_QUADRI
MARGIN = 4.0        # device against oracle: two float32 evaluations of one operation, other FFT factorisation and summation order
EPS = 2.0 ** -24

_Z2 = ((0, 0), (0, 0))
_Z3 = ((0, 0), (0, 0), (0, 0))
# name, nx, ou, ir, rs, xr, yr, step, mode, interp, states, environment switches
CASES = [
    ("two-zones",               200, 88, 1, 1, 2, 2, 1.0, M, BIL, _Z2, {}),
    ("three-zones-1024",        256, 120, 1, 1, 2, 2, 1.0, M, BIL, _Z2, {}),
    ("mixed-256-512",           176, 80, 3, 2, 2, 2, 1.0, M, BIL, _Z2, {}),
    ("ragged-last-quad",        140, 62, 1, 1, 2, 2, 1.0, M, BIL, _Z2, {}),
    # a half-integer state (what a half-pixel step leaves): cxf = cnx + 0.5, cyf = cnx - 0.5 are truncated to the crop centre
    ("half-pixel",              150, 66, 1, 1, 1, 1, 0.5, M, BIL, ((0.5, -0.5), (0, 0)), {}),
    ("odd-box",                 141, 61, 1, 1, 2, 2, 1.0, M, BIL, _Z2, {}),
    # mashi = 76 - 66 - 2 = 8: windows of 4 x 3, 3 x 3 and (state beyond mashi: reset) 5 x 5 offsets
    ("edge-windows",            150, 66, 1, 1, 2, 2, 1.0, M, BIL, ((7, -8), (8, 8), (9, 0)), {}),
    ("edge-windows-all",        150, 66, 1, 1, 2, 2, 1.0, M, BIL, ((7, -8), (8, 8), (9, 0)), {"RALIGN_LIVE_OFFSETS": "0"}),
    ("reffree",                 200, 88, 1, 1, 2, 2, 1.0, F, BIL, _Z2, {}),
    ("reffree-global-taps",     200, 88, 1, 1, 2, 2, 1.0, F, BIL, _Z2, {"RALIGN_ZONES": "0"}),
    ("global-taps-two-zones",   200, 88, 1, 1, 2, 2, 1.0, M, BIL, _Z2, {"RALIGN_ZONES": "0"}),
    ("global-taps-three-zones", 256, 120, 1, 1, 2, 2, 1.0, M, BIL, _Z2, {"RALIGN_ZONES": "0"}),
    ("quadri-generic",          140, 61, 1, 1, 1, 1, 1.0, M, QUADRI, _Z2, {}),
    # mashi = 101 - 88 - 2 = 11: a window of 3 x 3 next to one of 5 x 5 -- the 4 offset slices of polar_zone_kernel hold 3 3 3 0 and
    # 7 7 7 4 offsets: nlive % nchunk != 0 and an empty last slice.  (The slice count is a constant of the shipped library:
    # RALIGN_ZONE_CHUNKS exists in profiling builds only, so 1 and 3 slices cannot be asked of it.)
    ("zone-chunks",             200, 88, 1, 1, 2, 2, 1.0, M, BIL, ((0, 0), (11, 11)), {}),
    # debug_spectra on an engine whose search runs the fused kernel over a crop
    ("tcrop-160-34",            160, 34, 1, 1, 2, 2, 1.0, M, BIL, _Z3, {}),
    ("tcrop-144-30-reffree",    144, 30, 1, 1, 2, 2, 1.0, F, BIL, _Z3, {}),
]
IDS = [c[0] for c in CASES]
BY_NAME = {c[0]: c for c in CASES}
# cases whose engine runs polar_zone_kernel, the size-generic class (search_path 2), and the cases with every offset in the window
ZONE_CASES = ["two-zones", "three-zones-1024", "mixed-256-512", "ragged-last-quad", "half-pixel", "odd-box", "edge-windows",
              "edge-windows-all", "reffree", "zone-chunks"]
GENERIC_CASES = [n for n in IDS if not n.startswith("tcrop-")]
TCROP_CASES = [n for n in IDS if n.startswith("tcrop-")]
# the switches a case may set: none of them may leak in from the environment of the run
SWITCHES = ["RALIGN_ZONES", "RALIGN_LIVE_OFFSETS"]


def geometry_key(case):
    """what the inputs and the reference depend on: everything but the name and the environment switches"""
    return tuple(case[1:11])


# ---------------------------------------------------------------------------------------------- inputs

_INPUTS = {}


def inputs(case):
    """(particles float32 [n][nx][nx], states float32 [n][2]) of a case, seeded"""
    key = geometry_key(case)
    if key not in _INPUTS:
        _, nx, ou, ir, rs, xr, yr, step, mode, interp, states, _ = case
        n = len(states)
        refs = synth.make_references(2, nx, ou)
        parts, _t = synth.make_particles(refs, n, xr, yr, 0.5, ou=ou)
        _INPUTS[key] = (parts, np.array(states, np.float32).reshape(n, 2))
    return _INPUTS[key]


def numr_of(case):
    return geometry.numrinit(case[3], case[2], case[4])


# ---------------------------------------------------------------------------------------------- the window rule

def window(case, dx, dy):
    """particle_window (csrc/ralign_kernels.h) from geometry.search_range: (sxi, syi, lkx, rkx, lky, rky, reset).  RA_MODE_MREF resets
    a state beyond mashi, RA_MODE_REFFREE clamps it; the radius of the rule is the last_ring ARGUMENT for RA_MODE_MREF and the
    outermost sampled ring for RA_MODE_REFFREE"""
    _, nx, ou, ir, rs, xr, yr, step, mode = case[:9]
    numr = numr_of(case)
    win_ring = ou if mode == M else numr[-3]
    mashi = nx // 2 + 1 - win_ring - 2
    reset = False
    if mode == M:
        if abs(dx) > mashi or abs(dy) > mashi:
            dx, dy, reset = 0.0, 0.0, True
    else:
        dx, dy = min(max(dx, -mashi), mashi), min(max(dy, -mashi), mashi)
    lx, rx = geometry.search_range(nx, win_ring, dx, xr)
    ly, ry = geometry.search_range(nx, win_ring, dy, yr)
    return float(dx), float(dy), int(lx / step), int(rx / step), int(ly / step), int(ry / step), reset


def live_index(case, w, s):
    """live_index: position of offset s of the list among the in-window offsets of window w (y outer, x inner), -1 outside"""
    nkx, nky = int(case[5] / case[7]), int(case[6] / case[7])
    nx1 = 2 * nkx + 1
    iy, ix = s // nx1 - nky, s % nx1 - nkx
    _, _, lkx, rkx, lky, rky, _ = w
    if ix < -lkx or ix > rkx or iy < -lky or iy > rky:
        return -1
    return (iy + lky) * (lkx + rkx + 1) + (ix + lkx)


def in_window(case):
    """bool [n][nshift]: the offsets inside each particle's window"""
    st = np.array(case[10], np.float32).reshape(-1, 2)
    ns = len(geometry.shift_list(case[5], case[6], case[7]))
    out = np.zeros((len(st), ns), bool)
    for p in range(len(st)):
        w = window(case, float(st[p, 0]), float(st[p, 1]))
        out[p] = [live_index(case, w, s) >= 0 for s in range(ns)]
    return out


# the cases with every offset of every particle inside its window
CENTRED_CASES = [c[0] for c in CASES if in_window(c).all()]


# ---------------------------------------------------------------------------------------------- the float64 reference

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = _libm.cosf.restype = ctypes.c_float
_libm.sinf.argtypes = _libm.cosf.argtypes = [ctypes.c_float]


def ring_offsets(numr):
    """float32 (dx, dy) [lcirc] of every sample relative to the sampling centre, orc_polar2dm's arithmetic: the first quadrant from
    the C library's sinf / cosf of the float32 angle (float)(dfi * jt), times the radius in float32, mirrored into the other three"""
    f = np.float32
    nring = len(numr) // 3
    lcirc = numr[-2] + numr[-1] - 1
    dx, dy = np.zeros(lcirc, f), np.zeros(lcirc, f)
    for it in range(nring):
        inr, kc, l = numr[3 * it], numr[3 * it + 1] - 1, numr[3 * it + 2]
        lt = l // 4
        dfi = (2 * math.atan(1.0)) / lt
        x, y = np.zeros(lt, f), np.zeros(lt, f)
        y[0] = f(inr)
        for jt in range(1, lt):
            fi = f(dfi * jt)
            x[jt] = f(_libm.sinf(fi)) * f(inr)
            y[jt] = f(_libm.cosf(fi)) * f(inr)
        dx[kc:kc + l] = np.concatenate([x, y, -x, -y])
        dy[kc:kc + l] = np.concatenate([y, -x, -y, x])
    return dx, dy


def _bilinear64(img, x, y):
    """Util::bilinear at the 1-based float32 positions (x, y), in float64 (taps clamped like the oracle's: a sample that lands on
    the last column / row carries a zero-weight tap one past the image)"""
    ny, nx = img.shape
    ix, iy = x.astype(np.int64), y.astype(np.int64)           # truncation, as (int)
    xd, yd = x.astype(np.float64) - ix, y.astype(np.float64) - iy
    x0 = np.clip(ix, 1, nx); x1 = np.minimum(x0 + 1, nx)
    y0 = np.clip(iy, 1, ny); y1 = np.minimum(y0 + 1, ny)
    f00, f10 = img[y0 - 1, x0 - 1], img[y0 - 1, x1 - 1]
    f01, f11 = img[y1 - 1, x0 - 1], img[y1 - 1, x1 - 1]
    return f00 + yd * (f01 - f00) + xd * (f10 - f00 + yd * (f11 - f10 - f01 + f00))


def _quadri64(img, x, y):
    """Util::quadri (1-based, circulant) at the float32 positions, in float64"""
    ny, nx = img.shape
    f = np.float32
    x, y = x.copy(), y.copy()
    for v, n in ((x, nx), (y, ny)):          # the wrap loops run in float32, as the oracle's
        while (v < f(1.0)).any():
            v[v < f(1.0)] += f(n)
        while (v >= f(n + 1)).any():
            v[v >= f(n + 1)] -= f(n)
    i, j = x.astype(np.int64), y.astype(np.int64)
    dx0, dy0 = x.astype(np.float64) - i, y.astype(np.float64) - j
    ip1 = np.where(i + 1 > nx, i + 1 - nx, i + 1); im1 = np.where(i - 1 < 1, i - 1 + nx, i - 1)
    jp1 = np.where(j + 1 > ny, j + 1 - ny, j + 1); jm1 = np.where(j - 1 < 1, j - 1 + ny, j - 1)
    fd = lambda a, b: img[b - 1, a - 1]
    f0 = fd(i, j)
    c1 = fd(ip1, j) - f0
    c2 = (c1 - f0 + fd(im1, j)) * 0.5
    c3 = fd(i, jp1) - f0
    c4 = (c3 - f0 + fd(i, jm1)) * 0.5
    # dx0, dy0 >= 0: hxc = hyc = 1, the corner is (i + 1, j + 1) and its (h (h - 1)) terms vanish
    c5 = fd(ip1, jp1) - f0 - c1 - c3
    return f0 + dx0 * (c1 + (dx0 - 1) * c2 + dy0 * c5) + dy0 * (c3 + (dy0 - 1) * c4)


def ring_weights(numr):
    """Normalize_ring's weight r 2 pi / n of every sample, float64 [lcirc]"""
    w = np.zeros(numr[-2] + numr[-1] - 1)
    for i in range(len(numr) // 3):
        w[numr[3 * i + 1] - 1:numr[3 * i + 1] - 1 + numr[3 * i + 2]] = numr[3 * i] * 2 * math.pi / numr[3 * i + 2]
    return w


def pack_rfft(circ, numr):
    """Frngs in float64: every ring's numpy.fft.rfft, packed.  circ [..., lcirc]"""
    out = np.zeros(circ.shape, np.float64)
    for i in range(len(numr) // 3):
        o, l = numr[3 * i + 1] - 1, numr[3 * i + 2]
        X = np.fft.rfft(circ[..., o:o + l], axis=-1)
        out[..., o] = X[..., 0].real
        out[..., o + 1] = X[..., l // 2].real
        out[..., o + 2:o + l:2] = X[..., 1:l // 2].real
        out[..., o + 3:o + l:2] = X[..., 1:l // 2].imag
    return out


def sample64(img, cx, cy, rings, interp=BIL, offsets=None):
    """Polar2Dm in float64 at the oracle's float32 positions; cx, cy: the float32 sampling centre (1-based).  float64 [lcirc]"""
    dx, dy = offsets if offsets is not None else ring_offsets(rings)
    x, y = dx + np.float32(cx), dy + np.float32(cy)
    assert x.dtype == np.float32 and y.dtype == np.float32
    img = np.asarray(img, np.float64)
    return _quadri64(img, x, y) if interp == QUADRI else _bilinear64(img, x, y)


def normalize64(circ, rings, weights=None):
    """Normalize_ring in float64: (circ - avg) / sigma, avg, sigma"""
    w = weights if weights is not None else ring_weights(rings)
    nn = w.sum()
    av, sq = (circ * w).sum(), (circ * circ * w).sum()
    avg = av / nn
    sgm = math.sqrt((sq - av * av / nn) / nn)
    return (circ - avg) / sgm, avg, sgm


def reference(img, cx, cy, rings, normalize, interp=BIL):
    """Polar2Dm -> (Normalize_ring) -> Frngs of one image at one sampling centre, float64 [lcirc] in EMAN2's packed ring layout.
    rings: the (radius, 1-based offset, length) triplets of Numrinit"""
    c = sample64(img, cx, cy, rings, interp)
    if normalize:
        c = normalize64(c, rings)[0]
    return pack_rfft(c, rings)


def ring_ratio(got, ref, rings):
    """per ring r of length L_r:  max over the ring's slots of |got - ref| / (2^-24 (1 + log2 L_r) ||ref_r||_2), the 2-norm of the
    ring's own packed spectrum: the size of a float32 FFT's error on that ring.  got, ref [..., lcirc] -> float64 [..., nring]"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    nring = len(rings) // 3
    out = np.zeros(ref.shape[:-1] + (nring,))
    for i in range(nring):
        o, l = rings[3 * i + 1] - 1, rings[3 * i + 2]
        unit = EPS * (1.0 + math.log2(l)) * np.linalg.norm(ref[..., o:o + l], axis=-1)
        out[..., i] = np.abs(got[..., o:o + l] - ref[..., o:o + l]).max(axis=-1) / unit
    return out


def worst(ratio, got, ref, rings):
    """(ratio, entry index, ring, slot) of the largest per-ring ratio of ring_ratio's result [nent][nring]"""
    e, r = np.unravel_index(np.argmax(ratio), ratio.shape)
    o, l = rings[3 * r + 1] - 1, rings[3 * r + 2]
    slot = int(np.argmax(np.abs(np.asarray(got[e, o:o + l], np.float64) - ref[e, o:o + l])))
    return float(ratio[e, r]), int(e), int(r), slot


# ---------------------------------------------------------------------------------------------- per case: reference, oracle

_REFERENCE = {}


def case_reference(case):
    """the float64 reference of every (particle, offset) of a case, in or out of the window:
    dict(ref [n][nshift][lcirc], raw (the same without Normalize_ring), avg, sigma [n][nshift], inwin bool [n][nshift], centre)"""
    key = geometry_key(case)
    if key in _REFERENCE:
        return _REFERENCE[key]
    _, nx, ou, ir, rs, xr, yr, step, mode, interp, _, _ = case
    parts, st = inputs(case)
    numr = numr_of(case)
    sh = geometry.shift_list(xr, yr, step)
    offs, wts = ring_offsets(numr), ring_weights(numr)
    n, ns, lcirc = len(st), len(sh), numr[-2] + numr[-1] - 1
    ref, raw = np.zeros((n, ns, lcirc)), np.zeros((n, ns, lcirc))
    avg, sgm = np.zeros((n, ns)), np.ones((n, ns))
    centre = np.zeros((n, ns, 2), np.float32)
    cnx = np.float32(nx // 2 + 1)
    inwin = in_window(case)
    for p in range(n):
        w = window(case, float(st[p, 0]), float(st[p, 1]))
        for s in range(ns):
            # ((float)cnx + sxi) + offset, in float32: Util.multiref_polar_ali_2d's cnx + ix on the caller's float cnx
            cx, cy = (cnx + np.float32(w[0])) + sh[s, 0], (cnx + np.float32(w[1])) + sh[s, 1]
            centre[p, s] = (cx, cy)
            if not inwin[p, s]:
                continue
            c = sample64(parts[p], cx, cy, numr, interp, offs)
            raw[p, s] = pack_rfft(c, numr)
            if mode == M:
                c, avg[p, s], sgm[p, s] = normalize64(c, numr, wts)
                ref[p, s] = pack_rfft(c, numr)
            else:
                ref[p, s] = raw[p, s]
    _REFERENCE[key] = dict(ref=ref, raw=raw, avg=avg, sigma=sgm, inwin=inwin, centre=centre, numr=numr)
    return _REFERENCE[key]


def recover_stats(got, raw, numr):
    """mean and sigma an implementation applied, from its normalised spectra `got` and the float64 RAW spectra of the same entry:
    got = (raw - [slot 0] avg L_r) / sigma.  1 / sigma: least squares over every slot but the rings' DC slots; avg_r of every ring
    from its DC slot.  -> (avg (the median of avg_r), sigma, avg_r [nring])"""
    got = np.asarray(got, np.float64)
    nring = len(numr) // 3
    dc = np.array([numr[3 * i + 1] - 1 for i in range(nring)])
    L = np.array([numr[3 * i + 2] for i in range(nring)], np.float64)
    sel = np.ones(raw.shape[-1], bool)
    sel[dc] = False
    rsg = float(np.dot(got[sel], raw[sel]) / np.dot(raw[sel], raw[sel]))
    avg_r = (raw[dc] - got[dc] / rsg) / L
    return float(np.median(avg_r)), 1.0 / rsg, avg_r


ORACLE_RATIO = {}       # case name -> largest per-ring ratio of the CPU oracle against the reference: what float32 costs on these inputs
ORACLE_STATS = {}       # MREF cases: (largest relative error of the oracle's mean, of its sigma), recovered by recover_stats
ORACLE_RAW_RATIO = {}   # MREF cases: the oracle's largest per-ring ratio WITHOUT Normalize_ring (taps and transform alone)
_ORACLE = {}


def oracle_figures(case):
    """fills ORACLE_RATIO / ORACLE_STATS of the case (once per geometry) and returns (ratio, (entry, ring, slot), stats or None)"""
    from oracle import oracle as orc
    key = geometry_key(case)
    if key not in _ORACLE:
        _, nx, ou, ir, rs, xr, yr, step, mode, interp, _, _ = case
        R = case_reference(case)
        parts, _st = inputs(case)
        rg = orc.rings(ir, ou, rs)
        numr = R["numr"]
        assert rg.numr_list() == list(numr)
        ent = np.argwhere(R["inwin"])
        got = np.zeros((len(ent), R["ref"].shape[-1]), np.float32)
        graw = np.zeros_like(got)
        for k, (p, s) in enumerate(ent):
            c = orc.polar2dm(parts[p], R["centre"][p, s, 0], R["centre"][p, s, 1], rg, interp)
            if mode == M:
                graw[k] = orc.frngs(c, rg)
                c = orc.normalize_ring(c, rg)
            got[k] = orc.frngs(c, rg)
        ref = R["ref"][R["inwin"]]
        ratio = ring_ratio(got, ref, numr)
        big, e, r, slot = worst(ratio, got, ref, numr)
        stats = None
        if mode == M:
            raw, avg, sgm = R["raw"][R["inwin"]], R["avg"][R["inwin"]], R["sigma"][R["inwin"]]
            rec = [recover_stats(got[k], raw[k], numr) for k in range(len(ent))]
            stats = (max(abs(rec[k][0] - avg[k]) / abs(avg[k]) for k in range(len(ent))),
                     max(abs(rec[k][1] - sgm[k]) / sgm[k] for k in range(len(ent))),
                     float(ring_ratio(graw, raw, numr).max()))
        _ORACLE[key] = (big, (int(ent[e][0]), int(ent[e][1]), r, slot), stats, bool(np.isfinite(ratio).all()))
    ORACLE_RATIO[case[0]] = _ORACLE[key][0]
    if _ORACLE[key][2] is not None:
        ORACLE_STATS[case[0]] = _ORACLE[key][2][:2]
        ORACLE_RAW_RATIO[case[0]] = _ORACLE[key][2][2]
    return _ORACLE[key]
