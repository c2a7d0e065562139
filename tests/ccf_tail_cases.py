"""Inputs, oracle answers and engine runs of the CCF-tail tests (tests/test_ccf_tail_cpu.py, tests/test_gpu_ccf_tail.py) and of the
generator of their golden records (tests/golden/make_ccf_tail_records.py).

The CCF tail of a search pass is the store of the contracted spectra into LDS plus the inverse FFT and argmax (ifft_argmax of
ralign_kernels.h).  Every case below is the smallest geometry that reaches one way into that code; all inputs are seeded."""
import os

import numpy as np

from cryo_ralib_amd import api, synth
from oracle import oracle as orc

M, F = api.RA_MODE_MREF, api.RA_MODE_REFFREE
N_PART, SIGMA = 48, 0.5

# the reference count from which search_fused_kernel needs two store / inverse-FFT rounds at ou 36 (build_fused_plan of
# ralign_fused.h: rz_max = min(16, sbuf / zstride) references per round, zstride = 2 (maxrin + maxrin / 16) + 2 floats per
# spectrum, sbuf = 6432 floats of ring buffer at 36 rings of up to 256 samples)
FUSED_SBUF_OU36, MAXRIN_OU36 = 6432, 256


def fused_rounds(nref, sbuf=FUSED_SBUF_OU36, maxrin=MAXRIN_OU36):
    zstride = 2 * (maxrin + maxrin // 16) + 2
    rzmax = max(1, min(16, sbuf // zstride))
    return (nref + rzmax - 1) // rzmax


TWO_ROUND_NREF = next(r for r in range(1, 15) if fused_rounds(r) == 2)

# name: nx, ou, nref, mode, xr, n, shard (seed of the particles), environment switches, kernel family (search_path, tiled, offsets per pass)
# shards: the first for which the oracle's best and second-best peak of every particle differ by more than 1e-5 (test_ccf_tail_cpu.py)
CASES = {
    "fused-32-R3":       (32, 12, 3, M, 2, N_PART, 5, {}, (1, 0, 0)),                    # maxrin 128, one round
    "fused-90-R3":       (90, 36, 3, M, 3, N_PART, 0, {}, (1, 0, 0)),                    # maxrin 256, one round
    "fused-90-reffree":  (90, 36, 1, F, 3, N_PART, 0, {}, (1, 0, 0)),                    # one reference, no Normalize_ring
    "fused-90-2rounds":  (90, 36, TWO_ROUND_NREF, M, 3, N_PART, 0, {}, (1, 0, 0)),       # ONE = false
    "fused-90-R10":      (90, 36, 10, M, 3, N_PART, 0, {}, (1, 0, 0)),                   # five pairs: the last share holds a pair less
    "tiled-90-R17":      (90, 36, 17, M, 3, N_PART, 0, {}, (1, 1, 0)),                   # search_tiled_kernel
    "pair-100-R3":       (100, 40, 3, M, 3, N_PART, 3, {}, (3, 0, 2)),                   # search_pair_kernel
    "kernelpair-90-R3":  (90, 36, 3, M, 3, N_PART, 0, {"RALIGN_FUSED": "0"}, (0, 0, 0)), # ccf_kernel
    "pack-90-R3-n5":     (90, 36, 3, M, 3, 5, 1, {}, (1, 0, 0)),                         # 5 x 49 slots: one live offset in the last pass
}
# the kernel pair calls ifft_argmax<N, 2> only in builds with RA_CCF_THREADS < 1024, which no shipped build is: NP = 2 has no case

NOMIRROR = "nomirror-90-reffree"        # reference-free, nomirror set: straight half only
CONSTANT = "constant-90-reffree"        # constant particles: both sequences constant and equal
PLANTED = "planted-90-reffree"          # winners at angle bins 1, 2, 3, N - 2, N - 1, N (1-based): the 7-point neighbourhood wraps
PLANTED_BINS = (1, 2, 3, 254, 255, 256)
PLANTED_ROT = (1, 256, 255, 4, 3, 2)    # a particle turned by the angle of bin b peaks at bin 258 - b (mod 256)
NOMIRROR_SHARD = 4
ALL = list(CASES) + [NOMIRROR, CONSTANT, PLANTED]


def geometry_of(name):
    if name in CASES:
        return CASES[name]
    n = {NOMIRROR: N_PART, CONSTANT: 4, PLANTED: len(PLANTED_BINS)}[name]
    return (90, 36, 1, F, 3, n, NOMIRROR_SHARD, {}, (1, 0, 0))


def planted_angle(jbin, maxrin=MAXRIN_OU36):
    """the angle of a whole bin `jbin` (1-based), ang_n"""
    return float(orc.ang_n(float(jbin), maxrin))


_INPUTS = {}


def inputs(name):
    """(references as the engine takes them, particles), seeded, computed once"""
    if name not in _INPUTS:
        nx, ou, nref, mode, xr, n, shard, _, _ = geometry_of(name)
        refs = synth.make_references(nref, nx, ou)
        if name == CONSTANT:
            parts = np.full((n, nx, nx), 1.5, np.float32)
        elif name == PLANTED:
            parts = np.stack([synth.rot_shift2d_np(refs[0], planted_angle(b), 0.0, 0.0, 0) for b in PLANTED_ROT]).astype(np.float32)
        else:
            parts, _ = synth.make_particles(refs, n, xr, xr, SIGMA, shard=shard, ou=ou)
        if mode == M:
            refs, _ = orc.prepare_refs(refs, orc.model_circle(ou, nx, nx), orc.rings(1, ou, 1))
        _INPUTS[name] = (np.ascontiguousarray(refs, np.float32), np.ascontiguousarray(parts, np.float32))
    return _INPUTS[name]


def _cref(name):
    nx, ou, nref, mode = geometry_of(name)[:4]
    refs, _ = inputs(name)
    rg = orc.rings(1, ou, 1)
    if mode == M:
        return rg, orc.prepare_refs(synth.make_references(nref, nx, ou), orc.model_circle(ou, nx, nx), rg)[1]
    return rg, orc.prepare_refs(refs, None, rg)[1]


_ORACLE = {}


def oracle(name):
    """(params [n][6], jtot [n], d [n][2]) of orc.mref_iteration / orc.reffree_iteration from a zero shift state, computed once"""
    if name not in _ORACLE:
        nx, ou, nref, mode, xr, n = geometry_of(name)[:6]
        _, parts = inputs(name)
        rg, cref = _cref(name)
        d = np.zeros((n, 2), np.float32)
        if mode == M:
            params, infos, _, _ = orc.mref_iteration(parts, cref, rg, xr, xr, 1.0, d, nthreads=8)
        else:
            orc.set_nomirror(name == NOMIRROR)
            try:
                params, infos, _, _ = orc.reffree_iteration(parts, cref[0], rg, xr, xr, 1.0, (0, 0), d, np.zeros((n, 6), np.float32), nthreads=8)
            finally:
                orc.set_nomirror(False)
        _ORACLE[name] = (params, np.array([infos[i].jtot for i in range(n)]), d)
    return _ORACLE[name]


def ccf_sequences(c_ref, c_img, rg):
    """the straight and the mirrored sequence of Util::Crosrng_ms over the angle bins, in double: the accumulation of
    orc_crosrng_ms restated in numpy (packed spectra: [0] DC, [1] the Nyquist term of a full-length ring -- of a shorter one
    the coefficient at its own length --, then Re, Im pairs); callers check it against orc.crosrng_ms"""
    maxrin, numr = rg.maxrin, rg.numr_list()
    q = np.zeros(maxrin + 2, np.float64); t = np.zeros(maxrin + 2, np.float64)
    for i in range(rg.nring):
        o, n = numr[3 * i + 1] - 1, numr[3 * i + 2]
        c = c_ref[o:o + n].astype(np.float32); d = c_img[o:o + n].astype(np.float32)
        t1 = np.float32(c[0] * d[0]); q[0] += t1; t[0] += t1
        t1 = np.float32(c[1] * d[1]); q[n] += t1; t[n] += t1          # n == maxrin: the Nyquist term, q[maxrin]
        c1, c2, d1, d2 = c[2::2], c[3::2], d[2::2], d[3::2]
        p1, p2, p3, p4 = c1 * d1, c2 * d2, c1 * d2, c2 * d1            # float32 products, as the C code
        q[2:n:2] += (p1 + p2).astype(np.float32); q[3:n:2] += (-p3 + p4).astype(np.float32)
        t[2:n:2] += (p1 - p2).astype(np.float32); t[3:n:2] += (-p3 - p4).astype(np.float32)

    def inverse(a):
        spec = a[0:maxrin + 2:2] + 1j * a[1:maxrin + 2:2]
        spec[0] = a[0]; spec[maxrin // 2] = a[maxrin]
        return np.fft.irfft(spec, maxrin)

    return inverse(q), inverse(t)


def peak_gap(name, i, straight_only=False):
    """relative gap between the best and the second-best CCF value of particle i over (reference, offset, mirror, angle bin),
    and the best value: every (reference, offset) goes through orc.crosrng_ms for the maxima of its two sequences; the angle
    bins of the winning sequence come from ccf_sequences (checked against orc.crosrng_ms on the way)"""
    nx, ou, nref, mode, xr = geometry_of(name)[:5]
    _, parts = inputs(name)
    rg, cref = _cref(name)
    cnx = nx // 2 + 1
    cands = []
    for iy in range(-xr, xr + 1):
        for ix in range(-xr, xr + 1):
            c = orc.polar2dm(parts[i], cnx + ix, cnx + iy, rg)
            if mode == M:
                c = orc.normalize_ring(c, rg)
            c = orc.frngs(c, rg)
            for r in range(nref):
                m = orc.crosrng_ms(cref[r], c, rg)
                cands.append((m["qn"], m["jn"], r, c, 0))
                if not straight_only:
                    cands.append((m["qm"], m["jm"], r, c, 1))
    cands.sort(key=lambda x: -x[0])
    best, jbest, r, c, mir = cands[0]
    seq = ccf_sequences(cref[r], c, rg)[mir]
    assert abs(seq.max() - best) <= 1e-9 * abs(best) and int(np.argmax(seq)) + 1 == jbest, (seq.max(), best, np.argmax(seq), jbest)
    second_angle = np.sort(seq)[-2]
    second = max(cands[1][0], second_angle)
    return (best - second) / abs(best), best


def run_engine(name):
    """one search of the case on the GPU from a zero shift state: (records as RESULT_DTYPE, shift state, kernel family)"""
    import torch
    nx, ou, nref, mode, xr, n, _, env, _ = geometry_of(name)
    refs, parts = inputs(name)
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        eng = api.Engine(nx, ou, xr, xr, 1.0, nref, mode)
    finally:
        for k, v in saved.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        family = (eng.search_path, int(eng.search_tiled), eng.search_offsets_per_pass)
        if name == NOMIRROR:
            eng.set_nomirror(True)
        eng.set_references(torch.from_numpy(refs).to(eng.dev))
        st, res = eng.new_state(n), eng.new_result(n)
        eng.align(torch.from_numpy(parts).to(eng.dev), st, res)
        eng.sync()
        return api.Engine.result_to_numpy(res).copy(), st.cpu().numpy().copy(), family
    finally:
        eng.close()
