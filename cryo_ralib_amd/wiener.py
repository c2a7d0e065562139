"""CTF-corrected (Wiener-filtered) class averages of an aligned particle stack.

    python -m cryo_ralib_amd.wiener STACK PARAMS CTF OUT [--labels labels.npy] [--k K] [--snr S] [--nopad] [--flipped]
                                    [--min_count M] [--apix A] [--ou R] [--device D] [--ssnr [--ssnr_floor F] [--frc FRC.npz]]
                                    [--scores SCORES.npz [--band LO HI] [--no_leave_one_out] [--keep F] [--min_cc T]]

The contract, stated in float64 by `wiener_reference`: inputs are a stack x [n][nx][nx], params [n][4]
(alpha, sx, sy, mirror, as api.rot_shift2d takes them), labels [n] in 0 .. k-1, a CTF table [n][9] in the layout of ctf.py,
snr > 0, pad (P = 2 nx, the default, or P = nx), flipped and min_count.  For each particle i:

  1. y_i = rot_shift2D(x_i, alpha_i, sx_i, sy_i, mirror_i);
  2. Y_i = rfft2 of y_i embedded at o = (P - nx) / 2 in a P x P zero image (the phase flip's embedding), on the [P][P/2 + 1] grid;
  3. c_i = ctf.ctf_grid(row_i', nx, P), row_i' = row_i with DefocusAngle' = DefocusAngle - alpha (mirror 0) or
     alpha - DefocusAngle (mirror 1): the particle's CTF in the aligned frame.  rot_shift2D samples its input at G r + b with G
     orthogonal, so the output spectrum at k is the input's at G k (the shift only changes the phase); `ctf_at` evaluates the
     CTF at explicitly rotated or reflected frequencies and the tests pin the rule against it and against rotated images;
  4. w_i = c_i, or |c_i| when the particles were phase-flipped (flipped=True, as the drivers' particles are).

For each class j with n_j members: N_j = sum w_i Y_i, D_j = sum c_i^2 and A_j = crop_o(irfft2(N_j / (D_j + 1/snr), s=(P, P))), an
nx x nx image; a class with n_j < min_count is all zeros.  With c == 1 and a large snr, A_j is the plain mean of the aligned
particles, so the output is on the scale of an average.  There is no mask, no per-frequency SSNR and no correction of the
damping of rot_shift2D's interpolation.  Signs: particles formed as -c * F (EMAN2's orientation, in which ra_phase_flip leaves
+|c| F) give +F with flipped=True and -F with flipped=False.

The device path is ra_wiener_accumulate / ra_wiener_finalize (csrc/ralign_wiener.h); `accumulate` and `finalize` expose them
for callers that stream a stack in chunks or sum over ranks in between, `wiener_averages` runs both.

SSNR-weighted averages (--ssnr; DESIGN.md section 4.11, stated in float64 by `ssnr_reference`) replace the constant 1/snr with a
per-shell term that the data set.  Particle i of a call goes to half h_i = (index0 + i) % 2 of its class, index0 the global index
of its first image (the engine's even / odd split, so chunks and ranks agree when each passes its own offset); N_jh, D_jh and n_jh
are the sums above over class j's half h.  Shells s = floor(r + 0.5) of the rfft grid (r = |(kx, ky)|, ky the signed row
frequency) run 0 .. P/2; every shell sum carries the Hermitian weight g (1 on column 0 and, for even P, on column P/2; 2
elsewhere), so it equals the sum over the full plane.  V_jh = N_jh / (D_jh + 1/snr) and FRC_j(s) = sum g Re(V_j0 conj V_j1) /
sqrt(sum g |V_j0|^2 sum g |V_j1|^2), 0 where either sum is 0 and for classes with n_j0 + n_j1 < min_count.  With F = min(FRC, 0.999),
rho = max(2F / (1 - F), ssnr_floor) (0 before the floor where F <= 0) and R_j(s) = (sum g (D_j0 + D_j1) / sum g) / rho,
A_j = crop_o(irfft2((N_j0 + N_j1) / (D_j0 + D_j1 + R_j(min(s, P/2))))), 0 where that denominator is 0 (corner elements beyond
shell P/2 take its term).  --snr then only sets the half averages V.  The FRC also gives each class's resolution (`resolution`):
s1 = the first shell s >= 1 with FRC < t (P/2 + 1 if none), P apix / (s1 - 1) A, or pixels without a pixel size.  The device path
is ra_wiener_accumulate with labels 2j + h (`accumulate_halves`), ra_wiener_frc (`frc`) and ra_wiener_finalize_ssnr
(`finalize_ssnr`); `ssnr_averages` runs all three.

Per-particle agreement scores (--scores; DESIGN.md section 4.12, stated in float64 by `score_reference`) hold every particle
against what the rest of its class predicts for it.  Given class sums N, D and sizes (normally over all particles, the scored ones
included), for particle i of class j: N' = N_j - w_i Y_i, D' = max(D_j - c_i^2, 0) (leave-one-out, the default: a particle is part
of the average it is compared with, and in a class of n noise images the plain correlation is about 1/sqrt(n), not 0; without it
N' = N_j, D' = D_j), tau = 1/snr or the per-shell term reg[j][s] of the SSNR path, M_i = w_i N' / (D' + tau) (0 where that
denominator is 0, and everywhere when leave-one-out leaves nobody: n_j < 2), and over the elements of the shell band
s_lo <= s <= s_hi (default 1 .. P/2: no DC, everything up to Nyquist) with the Hermitian weights g:
X_i = sum g Re(Y_i conj M_i), E_i = sum g |Y_i|^2, F_i = sum g |M_i|^2.  cc_i = X / sqrt(E F) (0 where E F = 0) and the
least-squares amplitude scale_i = X / F (0 where F = 0); both nan in a class of fewer than max(min_count, 2) members
(max(min_count, 1) without leave-one-out).  The device path is ra_wiener_score (`score`); `particle_scores` accumulates, runs the FRC
when asked and scores; `select` turns cc into a mask (per class the best fraction --keep and / or cc >= --min_cc; unscored
particles stay).  With --keep / --min_cc the tool writes OUT (and --frc) from the kept particles only, the halves still by the
original particle index, and prints per class its size, the number kept and the kept particles' lowest and median cc.

PARAMS is a driver's params.txt (idx angle sx sy mirror class; the class column gives the labels) or an initial2Dparams.txt
(alpha sx sy mirror; one class); --labels (an int .npy) overrides the classes, e.g. with k-means labels.  CTF is a [n][9] .npy
or a RELION .star (ctf.load_table, --apix where the .star gives no pixel size).  --ou R subtracts the mean under
model_circle(R) from every particle first.  OUT is .hdf, .mrcs or .npy.
"""
import argparse
import sys

import numpy as np

from . import ctf as _ctf
from ._common import Launcher, ptr

MAX_K = 1024


class WienerError(ValueError):
    """shapes, labels, snr or a CTF table outside the contract's domain"""


# ---- the contract in float64 numpy

def ctf_at(row, nx, P, kx, ky):
    """ctf_np of the [9] row at the frequency vectors (kx, ky), in units of 1 / (P apix_eff) (any real values, any shape; kx along
    the fast axis): ctf_grid(row, nx, P) == ctf_at(row, nx, P, ix, iy) on the rfft2 grid's integer frequencies"""
    D, apix, dfu, dfv, dfang, volt, cs, w, ps = [float(v) for v in row]
    a = apix * D / nx
    x = np.asarray(kx, np.float64) / (P * a)
    y = np.asarray(ky, np.float64) / (P * a)
    volt, cs = volt * 1000, cs * 1e7
    dfang, ps = dfang * np.pi / 180, ps * np.pi / 180
    lam = 12.2639 / np.sqrt(volt + 0.97845e-6 * volt ** 2)
    ang = np.arctan2(y, x)
    s2 = x ** 2 + y ** 2
    df = .5 * (dfu + dfv + (dfu - dfv) * np.cos(2 * (ang - dfang)))
    gamma = 2 * np.pi * (-.5 * df * lam * s2 + .25 * cs * lam ** 3 * s2 ** 2) - ps
    return np.sqrt(1 - w ** 2) * np.sin(gamma) - w * np.cos(gamma)


def aligned_table(table, params):
    """the table with DefocusAngle' = DefocusAngle - alpha (mirror 0) or alpha - DefocusAngle (mirror 1), float64"""
    t = np.array(table, np.float64)
    prm = np.asarray(params, np.float64)
    alpha, mir = prm[:, 0], prm[:, 3] != 0
    t[:, 4] = np.where(mir, alpha - t[:, 4], t[:, 4] - alpha)
    return t


def check_inputs(n, nx, params, labels, k, table, snr=1.0):
    """params [n][4] (finite), labels [n] integers in 0 .. k-1, 1 <= k <= 1024, table [n][9] within ra_phase_flip's ranges,
    snr > 0; returns (params float64, labels int64, table float64)"""
    if not 2 <= nx <= 1024:
        raise WienerError("images are [n][nx][nx] with 2 <= nx <= 1024, got nx = %d" % nx)
    prm = np.asarray(params, np.float64)
    if prm.shape != (n, 4) or not np.isfinite(prm).all():
        raise WienerError("params are [%d][4] finite (alpha, sx, sy, mirror), got %s" % (n, prm.shape))
    if not (isinstance(k, (int, np.integer)) and 1 <= k <= MAX_K):
        raise WienerError("need 1 <= k <= %d, got %r" % (MAX_K, k))
    lab = np.asarray(labels)
    if lab.shape != (n,) or (n and not np.issubdtype(lab.dtype, np.integer)):
        raise WienerError("labels are [%d] integers, got %s %s" % (n, lab.dtype, lab.shape))
    lab = lab.astype(np.int64)
    if n and (lab.min() < 0 or lab.max() >= k):
        raise WienerError("labels must lie in 0 .. %d, got %d .. %d" % (k - 1, lab.min(), lab.max()))
    tab = np.asarray(table, np.float64)
    if tab.shape != (n, 9):
        raise WienerError("the CTF table is [%d][9], got %s" % (n, tab.shape))
    try:
        _ctf.check_table(tab)
    except _ctf.CtfTableError as e:
        raise WienerError(str(e))
    if not (np.isfinite(snr) and snr > 0):
        raise WienerError("need a finite snr > 0, got %r" % snr)
    return prm, lab, tab


def _images(x):
    x = np.asarray(x)
    if x.ndim != 3 or x.shape[1] != x.shape[2]:
        raise WienerError("images are [n][nx][nx], got %s" % (x.shape,))
    return x, x.shape[0], x.shape[-1]


def class_sums_reference(x, params, labels, k, table, pad=True, flipped=False, aligned=None):
    """float64 N_j [k][P][P/2 + 1] (complex), D_j [k][P][P/2 + 1] and the class sizes of the contract.  aligned: the rot_shift2D
    images [n][nx][nx] to use in step 1 (e.g. the device's own, to isolate the rest); default synth.rot_shift2d_np of x"""
    from . import synth
    x, n, nx = _images(x)
    prm, lab, tab = check_inputs(n, nx, params, labels, k, table)
    P = 2 * nx if pad else nx
    o = (P - nx) // 2
    tab = aligned_table(tab, prm)
    num = np.zeros((k, P, P // 2 + 1), np.complex128)
    den = np.zeros((k, P, P // 2 + 1))
    counts = np.bincount(lab, minlength=k)[:k]
    for i in range(n):
        if aligned is not None:
            y = np.asarray(aligned[i], np.float64)
        else:
            y = synth.rot_shift2d_np(x[i], prm[i, 0], prm[i, 1], prm[i, 2], int(prm[i, 3] != 0)).astype(np.float64)
        big = np.zeros((P, P))
        big[o:o + nx, o:o + nx] = y
        c = _ctf.ctf_grid(tab[i], nx, P)
        w = np.abs(c) if flipped else c
        num[lab[i]] += w * np.fft.rfft2(big)
        den[lab[i]] += c * c
    return num, den, counts


def wiener_reference(x, params, labels, k, table, snr=1.0, pad=True, flipped=False, min_count=1, aligned=None):
    """float64 statement of the contract: [k][nx][nx] averages and the class sizes.  aligned: the rot_shift2D images [n][nx][nx]
    to use in step 1 (e.g. the device's own, to isolate the rest); default synth.rot_shift2d_np of x"""
    x, n, nx = _images(x)
    check_inputs(n, nx, params, labels, k, table, snr)
    num, den, counts = class_sums_reference(x, params, labels, k, table, pad, flipped, aligned)
    P = 2 * nx if pad else nx
    o = (P - nx) // 2
    out = np.zeros((k, nx, nx))
    for j in range(k):
        if counts[j] >= min_count and counts[j] > 0:
            out[j] = np.fft.irfft2(num[j] / (den[j] + 1.0 / snr), s=(P, P))[o:o + nx, o:o + nx]
    return out, counts


# ---- the SSNR contract in float64 numpy

MAX_K_SSNR = MAX_K // 2
SSNR_FLOOR = 1e-3


def check_ssnr(k, ssnr_floor):
    """the SSNR path's own domain: 1 <= k <= 512 (its half sums are 2k classes), a finite ssnr_floor > 0"""
    if not (isinstance(k, (int, np.integer)) and 1 <= k <= MAX_K_SSNR):
        raise WienerError("the SSNR averages need 1 <= k <= %d, got %r" % (MAX_K_SSNR, k))
    if not (np.isfinite(ssnr_floor) and ssnr_floor > 0):
        raise WienerError("need a finite ssnr_floor > 0, got %r" % ssnr_floor)


def shells(P):
    """(s, g) on the rfft2 grid [P][P/2 + 1] of a P x P image: the shell floor(r + 0.5) of every element (r = |(kx, ky)|, ky the
    signed row frequency) and its Hermitian weight (1 on column 0 and, for even P, on column P/2; 2 elsewhere)"""
    H = P // 2 + 1
    iy = np.arange(P)
    ky = np.where(iy <= P // 2, iy, iy - P).astype(np.float64)[:, None]
    kx = np.arange(H, dtype=np.float64)[None, :]
    s = np.floor(np.sqrt(kx ** 2 + ky ** 2) + 0.5).astype(np.int64)
    g = np.full((P, H), 2.0)
    g[:, 0] = 1.0
    if P % 2 == 0:
        g[:, P // 2] = 1.0
    return s, g


def half_labels(labels, index0=0, index=None):
    """2 j + h per particle, h = (index0 + i) % 2: the labels of the half sums (2k classes).  index: the particles' global indices
    [n] instead of index0 + i (a subset of a stack that keeps its original even / odd split)"""
    lab = np.asarray(labels).astype(np.int64)
    if index is None:
        return 2 * lab + (int(index0) + np.arange(lab.shape[0])) % 2
    idx = np.asarray(index)
    if idx.shape != lab.shape or (idx.size and not np.issubdtype(idx.dtype, np.integer)):
        raise WienerError("index is [%d] integers (the particles' global indices), got %s %s" % (lab.shape[0], idx.dtype, idx.shape))
    return 2 * lab + idx.astype(np.int64) % 2


def frc_from_sums(num2, den2, counts2, nx, pad=True, snr=1.0, min_count=1, ssnr_floor=SSNR_FLOOR):
    """steps 2 - 4 of the SSNR contract in float64 on given half sums: num2 [k][2][P][P/2 + 1] complex (or float pairs
    [..][2]), den2 [k][2][P][P/2 + 1], counts2 [k][2]; returns (frc [k][P/2 + 1], reg [k][P/2 + 1])"""
    num2 = np.asarray(num2)
    if not np.iscomplexobj(num2):
        num2 = num2[..., 0].astype(np.float64) + 1j * num2[..., 1].astype(np.float64)
    num2 = num2.astype(np.complex128)
    den2 = np.asarray(den2, np.float64)
    counts2 = np.asarray(counts2)
    P = 2 * nx if pad else nx
    S = P // 2 + 1
    k = num2.shape[0]
    if num2.shape != (k, 2, P, S) or den2.shape != num2.shape or counts2.shape != (k, 2):
        raise WienerError("half sums are [k][2][%d][%d] and counts [k][2], got %s, %s, %s" % (P, S, num2.shape, den2.shape, counts2.shape))
    s, g = shells(P)
    inside = s <= P // 2
    idx, gw = s[inside], g[inside]
    v = num2 / (den2 + 1.0 / snr)
    gsum = np.bincount(idx, gw, S)
    frc, reg = np.zeros((k, S)), np.zeros((k, S))
    for j in range(k):
        v0, v1 = v[j, 0][inside], v[j, 1][inside]
        xr = np.bincount(idx, gw * (v0 * np.conj(v1)).real, S)
        a0 = np.bincount(idx, gw * np.abs(v0) ** 2, S)
        a1 = np.bincount(idx, gw * np.abs(v1) ** 2, S)
        dbar = np.bincount(idx, gw * (den2[j, 0] + den2[j, 1])[inside], S) / gsum
        ok = (a0 > 0) & (a1 > 0) & (counts2[j].sum() >= min_count)
        f = np.where(ok, xr / np.sqrt(np.where(ok, a0 * a1, 1.0)), 0.0)
        F = np.minimum(f, 0.999)
        rho = np.maximum(np.where(F > 0, 2 * F / (1 - F), 0.0), ssnr_floor)
        frc[j], reg[j] = f, dbar / rho
    return frc, reg


def ssnr_reference(x, params, labels, k, table, snr=1.0, ssnr_floor=SSNR_FLOOR, pad=True, flipped=False, min_count=1, index0=0,
                   aligned=None):
    """float64 statement of the SSNR contract: (averages [k][nx][nx], class sizes [k], frc [k][P/2 + 1], reg [k][P/2 + 1]).
    aligned: as for class_sums_reference"""
    x, n, nx = _images(x)
    check_inputs(n, nx, params, labels, k, table, snr)
    check_ssnr(k, ssnr_floor)
    P = 2 * nx if pad else nx
    o, S = (P - nx) // 2, P // 2 + 1
    num, den, cnt = class_sums_reference(x, params, half_labels(labels, index0), 2 * k, table, pad, flipped, aligned)
    num2, den2, counts2 = num.reshape(k, 2, P, S), den.reshape(k, 2, P, S), cnt.reshape(k, 2)
    frc, reg = frc_from_sums(num2, den2, counts2, nx, pad, snr, min_count, ssnr_floor)
    s, _ = shells(P)
    s = np.minimum(s, P // 2)
    counts = counts2.sum(1)
    out = np.zeros((k, nx, nx))
    for j in range(k):
        if counts[j] >= min_count and counts[j] > 0:
            d = den2[j, 0] + den2[j, 1] + reg[j][s]
            q = np.where(d != 0, (num2[j, 0] + num2[j, 1]) / np.where(d != 0, d, 1.0), 0.0)
            out[j] = np.fft.irfft2(q, s=(P, P))[o:o + nx, o:o + nx]
    return out, counts, frc, reg


def resolution(frc, nx, pad=True, apix=None, threshold=0.143, counts=None, min_count=1):
    """resolution of FRC curves [k][P/2 + 1] (or one curve) at `threshold`: s1 = the smallest shell s >= 1 with FRC < threshold, or
    P/2 + 1 if there is none, s* = s1 - 1; P apix / s* A, or P / s* pixels when apix is None; inf where s* = 0, nan for classes
    with counts < min_count (when counts are given)"""
    f = np.asarray(frc, np.float64)
    one = f.ndim == 1
    f = np.atleast_2d(f)
    P = 2 * nx if pad else nx
    if f.shape[1] != P // 2 + 1:
        raise WienerError("FRC curves have %d shells for P = %d, got %d" % (P // 2 + 1, P, f.shape[1]))
    below = f[:, 1:] < threshold
    star = np.where(below.any(1), below.argmax(1), P // 2)
    res = np.where(star > 0, P * (1.0 if apix is None else float(apix)) / np.maximum(star, 1), np.inf)
    if counts is not None:
        res = np.where(np.asarray(counts) < min_count, np.nan, res)
    return res[0] if one else res


def table_apix(table, nx):
    """the images' pixel size Apix D / nx when every row of the table agrees to a relative 1e-4, else None"""
    t = np.asarray(table, np.float64)
    if t.ndim != 2 or t.shape[0] == 0:
        return None
    a = t[:, 1] * t[:, 0] / nx
    return float(a[0]) if np.all(np.abs(a - a[0]) <= 1e-4 * abs(a[0])) else None


def resolutions(frc, counts, nx, pad=True, apix=None, min_count=1):
    """{"res_05", "res_0143": [k] at FRC 0.5 and 0.143, "units": "A" with a pixel size, else "px"}"""
    return {"res_05": resolution(frc, nx, pad, apix, 0.5, counts, min_count),
            "res_0143": resolution(frc, nx, pad, apix, 0.143, counts, min_count),
            "units": "px" if apix is None else "A"}


# ---- the score contract in float64 numpy

def check_score(nx, pad, k, snr=1.0, reg=None, band=None):
    """the score's own domain: the band 0 <= s_lo <= s_hi <= P/2 (None: 1 .. P/2), and either a finite snr > 0 or reg [k][P/2 + 1]
    finite and >= 0 with k <= 512; returns (s_lo, s_hi, reg float64 or None)"""
    P = 2 * nx if pad else nx
    try:
        lo, hi = (min(1, P // 2), P // 2) if band is None else tuple(band)
    except (TypeError, ValueError):
        raise WienerError("the shell band is (s_lo, s_hi), got %r" % (band,))
    if not all(isinstance(v, (int, np.integer)) for v in (lo, hi)) or not 0 <= lo <= hi <= P // 2:
        raise WienerError("the shell band needs integers 0 <= s_lo <= s_hi <= P/2 = %d, got %r" % (P // 2, band))
    if reg is None:
        if not (np.isfinite(snr) and snr > 0):
            raise WienerError("need a finite snr > 0, got %r" % snr)
        return int(lo), int(hi), None
    check_ssnr(k, SSNR_FLOOR)
    r = np.asarray(reg, np.float64)
    if r.shape != (k, P // 2 + 1) or not np.isfinite(r).all() or (r < 0).any():
        raise WienerError("the per-shell term is [%d][%d], finite and >= 0, got %s" % (k, P // 2 + 1, r.shape))
    return int(lo), int(hi), r


def _host_sums(num, den, counts, k, P):
    num = np.asarray(num)
    if not np.iscomplexobj(num):
        if num.ndim != 4 or num.shape[-1] != 2:
            raise WienerError("class sums are [k][P][P/2 + 1] complex (or float pairs [..][2]), got %s" % (num.shape,))
        num = num[..., 0].astype(np.float64) + 1j * num[..., 1].astype(np.float64)
    num = num.astype(np.complex128)
    den = np.asarray(den, np.float64)
    counts = np.asarray(counts)
    if num.shape != (k, P, P // 2 + 1) or den.shape != num.shape or counts.shape != (k,):
        raise WienerError("class sums are [%d][%d][%d] and counts [%d], got %s, %s, %s"
                          % (k, P, P // 2 + 1, k, num.shape, den.shape, counts.shape))
    return num, den, counts.astype(np.int64)


def scores_from_sums(sums, labels, counts, leave_one_out=True, min_count=1):
    """(cc, scale) [n] from the three sums [n][3] = (X, E, F): cc = X / sqrt(E F) (0 where E F = 0), scale = X / F (0 where F = 0);
    nan for particles of a class with fewer than max(min_count, 2) members (max(min_count, 1) without leave-one-out)"""
    a = np.asarray(sums, np.float64).reshape(-1, 3)
    X, E, F = a[:, 0], a[:, 1], a[:, 2]
    ef = E * F
    cc = np.where(ef > 0, X / np.sqrt(np.where(ef > 0, ef, 1.0)), 0.0)
    scale = np.where(F > 0, X / np.where(F > 0, F, 1.0), 0.0)
    lab = np.asarray(labels).astype(np.int64)
    unscored = np.asarray(counts)[lab] < max(int(min_count), 2 if leave_one_out else 1)
    cc[unscored] = np.nan
    scale[unscored] = np.nan
    return cc, scale


def score_reference(x, params, labels, k, table, num, den, counts, snr=1.0, reg=None, leave_one_out=True, band=None, pad=True,
                    flipped=False, min_count=1, aligned=None):
    """float64 statement of the score contract: {"cc" [n], "scale" [n], "sums" [n][3] = (X, E, F)} of the particles against the
    class sums num [k][P][P/2 + 1] (complex, or float pairs [..][2]), den, counts.  aligned: as for class_sums_reference"""
    from . import synth
    x, n, nx = _images(x)
    prm, lab, tab = check_inputs(n, nx, params, labels, k, table)
    lo, hi, reg = check_score(nx, pad, k, snr, reg, band)
    P = 2 * nx if pad else nx
    o = (P - nx) // 2
    num, den, counts = _host_sums(num, den, counts, k, P)
    tab = aligned_table(tab, prm)
    s, g = shells(P)
    sel = (s >= lo) & (s <= hi)
    gs = g[sel]
    sums = np.zeros((n, 3))
    for i in range(n):
        if aligned is not None:
            y = np.asarray(aligned[i], np.float64)
        else:
            y = synth.rot_shift2d_np(x[i], prm[i, 0], prm[i, 1], prm[i, 2], int(prm[i, 3] != 0)).astype(np.float64)
        big = np.zeros((P, P))
        big[o:o + nx, o:o + nx] = y
        Y = np.fft.rfft2(big)
        c = _ctf.ctf_grid(tab[i], nx, P)
        w = np.abs(c) if flipped else c
        j = lab[i]
        M = np.zeros_like(Y)
        if not leave_one_out or counts[j] >= 2:
            N, D = (num[j] - w * Y, np.maximum(den[j] - c * c, 0.0)) if leave_one_out else (num[j], den[j])
            q = D + (1.0 / snr if reg is None else reg[j][np.minimum(s, P // 2)])
            M = np.where(q != 0, w * N / np.where(q != 0, q, 1.0), 0.0)
        sums[i] = ((gs * (Y * np.conj(M)).real[sel]).sum(), (gs * np.abs(Y[sel]) ** 2).sum(), (gs * np.abs(M[sel]) ** 2).sum())
    cc, scale = scores_from_sums(sums, lab, counts, leave_one_out, min_count)
    return {"cc": cc, "scale": scale, "sums": sums}


def select(cc, labels, k, keep=None, min_cc=None):
    """boolean mask [n] of the particles to keep.  Per class, the scored members by cc descending (ties: the lower index first):
    keep=f (0 < f <= 1) keeps the first ceil(f n_j) of them, min_cc=t those with cc >= t; with both, a particle must pass both.
    Unscored particles (cc nan) are always kept"""
    cc = np.asarray(cc, np.float64)
    lab = np.asarray(labels)
    if cc.ndim != 1 or lab.shape != cc.shape or (cc.size and not np.issubdtype(lab.dtype, np.integer)):
        raise WienerError("cc is [n] and labels [n] integers, got %s and %s %s" % (cc.shape, lab.dtype, lab.shape))
    if not (isinstance(k, (int, np.integer)) and k >= 1) or (cc.size and (lab.min() < 0 or lab.max() >= k)):
        raise WienerError("labels must lie in 0 .. k - 1 with k >= 1, got k = %r" % (k,))
    if keep is not None and not (np.isfinite(keep) and 0 < keep <= 1):
        raise WienerError("need 0 < keep <= 1, got %r" % (keep,))
    if min_cc is not None and np.isnan(min_cc):
        raise WienerError("min_cc is a number, got nan")
    mask = np.ones(cc.shape, bool)
    scored = ~np.isnan(cc)
    if min_cc is not None:
        mask[scored] = cc[scored] >= min_cc
    if keep is not None:
        for j in range(k):
            idx = np.nonzero(scored & (lab == j))[0]
            order = idx[np.argsort(-cc[idx], kind="stable")]
            mask[order[int(np.ceil(keep * len(idx))):]] = False
    return mask


# ---- the device path

def new_sums(k, nx, pad=True, device=0):
    """zeroed (num [k][P][P/2 + 1][2] float32, den [k][P][P/2 + 1] float32, counts [k] int32) CUDA tensors"""
    import torch
    P = 2 * nx if pad else nx
    dev = torch.device("cuda", device) if not isinstance(device, torch.device) else device
    return (torch.zeros((k, P, P // 2 + 1, 2), dtype=torch.float32, device=dev),
            torch.zeros((k, P, P // 2 + 1), dtype=torch.float32, device=dev),
            torch.zeros(k, dtype=torch.int32, device=dev))


def accumulate(images, params, labels, k, table, num, den, counts, pad=True, flipped=False):
    """ra_wiener_accumulate on the current stream: add the weighted spectra of images [n][nx][nx] (contiguous float32 CUDA
    tensor) into num / den / counts (new_sums).  params [n][4], labels [n] and table [n][9] go to the device unchecked apart from
    their shapes: the library refuses bad labels, non-finite params and bad table rows (api.EngineError) and then adds nothing"""
    import torch
    from . import api
    assert images.is_cuda and images.is_contiguous() and images.dtype == torch.float32, "images: contiguous float32 CUDA tensor"
    assert images.dim() == 3 and images.shape[1] == images.shape[2], "images: [n][nx][nx]"
    n, nx = int(images.shape[0]), int(images.shape[-1])
    prm = np.asarray(params, np.float64)
    lab = np.asarray(labels).astype(np.int64)
    tab = np.ascontiguousarray(table, np.float32)
    if prm.shape != (n, 4) or lab.shape != (n,) or tab.shape != (n, 9):
        raise WienerError("need params [%d][4], labels [%d] and a table [%d][9], got %s, %s, %s" % (n, n, n, prm.shape, lab.shape, tab.shape))
    P = 2 * nx if pad else nx
    shp = (k, P, P // 2 + 1)
    for t, s, dt in ((num, shp + (2,), torch.float32), (den, shp, torch.float32), (counts, (k,), torch.int32)):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == s and t.device == images.device, \
            "sums: new_sums(k, nx, pad) on the images' device"
    rec = np.zeros(n, api.RESULT_DTYPE)
    rec["alpha"], rec["sx"], rec["sy"] = prm[:, 0], prm[:, 1], prm[:, 2]
    rec["mirror"] = (prm[:, 3] != 0).astype(np.int32)
    rec["ref_id"] = np.clip(lab, -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    d_rec = torch.from_numpy(rec.view(np.uint8)).to(images.device)
    L = Launcher(images)
    with torch.cuda.device(images.device):
        L.call("ra_wiener_accumulate", ptr(images), n, nx, ptr(d_rec), tab.ctypes.data_as(api.float_ptr), int(bool(pad)),
               int(bool(flipped)), int(k), ptr(num), ptr(den), ptr(counts))


def finalize(num, den, counts, nx, pad=True, snr=1.0, min_count=1, out=None):
    """ra_wiener_finalize on the current stream: [k][nx][nx] float32 CUDA tensor of the averages"""
    import torch
    k = int(counts.shape[0])
    if out is None:
        out = torch.empty((k, nx, nx), dtype=torch.float32, device=num.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (k, nx, nx)
    L = Launcher(num)
    with torch.cuda.device(num.device):
        L.call("ra_wiener_finalize", ptr(num), ptr(den), ptr(counts), k, int(nx), int(bool(pad)), float(snr), int(min_count), ptr(out))
    return out


def new_half_sums(k, nx, pad=True, device=0):
    """zeroed half sums (num2 [k][2][P][P/2 + 1][2] float32, den2 [k][2][P][P/2 + 1] float32, counts2 [k][2] int32) CUDA
    tensors: new_sums(2 k) with class j's half h in slot 2 j + h"""
    num, den, counts = new_sums(2 * k, nx, pad, device)
    P = 2 * nx if pad else nx
    return num.view(k, 2, P, P // 2 + 1, 2), den.view(k, 2, P, P // 2 + 1), counts.view(k, 2)


def _flat_halves(num2, den2, counts2):
    k = int(counts2.shape[0])
    for t in (num2, den2, counts2):
        assert t.is_contiguous(), "half sums: new_half_sums(k, nx, pad)"
    return k, num2.view(2 * k, *num2.shape[2:]), den2.view(2 * k, *den2.shape[2:]), counts2.view(2 * k)


def accumulate_halves(images, params, labels, k, table, num2, den2, counts2, index0=0, pad=True, flipped=False, index=None):
    """accumulate into the half sums (new_half_sums) on the current stream: particle i of images goes to half (index0 + i) % 2 of
    its class, index0 the global index of images[0] (the engine's even / odd split), through ra_wiener_accumulate with labels
    2j + h.  index: the particles' global indices [n] instead of index0 + i (a subset that keeps its original split).  Labels
    outside 0 .. k - 1 are refused here (WienerError), the rest as by `accumulate`"""
    n = int(images.shape[0])
    lab = np.asarray(labels)
    if lab.shape != (n,) or (n and not np.issubdtype(lab.dtype, np.integer)):
        raise WienerError("labels are [%d] integers, got %s %s" % (n, lab.dtype, lab.shape))
    if n and (lab.min() < 0 or lab.max() >= k):
        raise WienerError("labels must lie in 0 .. %d, got %d .. %d" % (k - 1, lab.min(), lab.max()))
    check_ssnr(k, SSNR_FLOOR)
    k2, num, den, counts = _flat_halves(num2, den2, counts2)
    assert k2 == k, "half sums of %d classes for k = %d" % (k2, k)
    accumulate(images, params, half_labels(lab, index0, index), 2 * k, table, num, den, counts, pad, flipped)


def frc(num2, den2, counts2, nx, pad=True, snr=1.0, min_count=1, ssnr_floor=SSNR_FLOOR):
    """ra_wiener_frc on the current stream: (frc [k][P/2 + 1] float64, reg [k][P/2 + 1] float32) CUDA tensors from the half sums"""
    import torch
    k = int(counts2.shape[0])
    _flat_halves(num2, den2, counts2)
    S = (2 * nx if pad else nx) // 2 + 1
    f = torch.empty((k, S), dtype=torch.float64, device=num2.device)
    r = torch.empty((k, S), dtype=torch.float32, device=num2.device)
    L = Launcher(num2)
    with torch.cuda.device(num2.device):
        L.call("ra_wiener_frc", ptr(num2), ptr(den2), ptr(counts2), k, int(nx), int(bool(pad)), float(snr), int(min_count),
               float(ssnr_floor), ptr(f), ptr(r))
    return f, r


def finalize_ssnr(num2, den2, counts2, reg, nx, pad=True, min_count=1, out=None):
    """ra_wiener_finalize_ssnr on the current stream: [k][nx][nx] float32 CUDA tensor of the SSNR-weighted averages"""
    import torch
    k = int(counts2.shape[0])
    _flat_halves(num2, den2, counts2)
    S = (2 * nx if pad else nx) // 2 + 1
    assert reg.is_contiguous() and reg.dtype == torch.float32 and tuple(reg.shape) == (k, S), "reg: frc()'s [k][P/2 + 1]"
    if out is None:
        out = torch.empty((k, nx, nx), dtype=torch.float32, device=num2.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (k, nx, nx)
    L = Launcher(num2)
    with torch.cuda.device(num2.device):
        L.call("ra_wiener_finalize_ssnr", ptr(num2), ptr(den2), ptr(counts2), ptr(reg), k, int(nx), int(bool(pad)), int(min_count), ptr(out))
    return out


def _device_stack(images, params, labels, k, ctf, snr, ou, preprocess, device):
    """(device, contiguous float32 images on it, params, labels, table) checked against the contract; preprocess=True subtracts
    the mean under model_circle(ou) first"""
    import torch
    from . import api
    dev = torch.device("cuda", device) if not isinstance(device, torch.device) else device
    if isinstance(images, np.ndarray):
        images = torch.from_numpy(np.ascontiguousarray(images, np.float32))
    if images.dim() != 3 or images.shape[1] != images.shape[2]:
        raise WienerError("images are [n][nx][nx], got %s" % (tuple(images.shape),))
    n, nx = int(images.shape[0]), int(images.shape[-1])
    unwrap = lambda a: a.detach().cpu().numpy() if hasattr(a, "detach") else a
    prm, lab, tab = check_inputs(n, nx, unwrap(params), unwrap(labels), k, unwrap(ctf), snr)
    with torch.cuda.device(dev):
        x = images.to(dev, dtype=torch.float32).contiguous()
        if preprocess:
            x = x.clone()
            eng = api.Engine(nx, int(ou) if ou is not None else nx // 2 - 2, 0.0, 0.0, 1.0, 1, api.RA_MODE_MREF, device=dev.index)
            try:
                eng.use_current_stream()
                eng.normalize_particles(x)
            finally:
                eng.close()
    return dev, x, prm, lab, tab


def wiener_averages(images, params, labels, k, ctf, snr=1.0, pad=True, flipped=False, min_count=1, ou=None, preprocess=False,
                    device=0):
    """[k][nx][nx] float32 CTF-corrected averages (numpy) and the class sizes [k] of the stack on the device (the contract of
    wiener_reference).  preprocess=True subtracts the mean under model_circle(ou) first (Engine.normalize_particles, as
    kmeans.class_averages does; ou defaults to nx // 2 - 2)."""
    import torch
    dev, x, prm, lab, tab = _device_stack(images, params, labels, k, ctf, snr, ou, preprocess, device)
    nx = int(x.shape[-1])
    with torch.cuda.device(dev):
        num, den, counts = new_sums(k, nx, pad, dev)
        accumulate(x, prm, lab, k, tab, num, den, counts, pad, flipped)
        out = finalize(num, den, counts, nx, pad, snr, min_count)
        return out.cpu().numpy(), counts.cpu().numpy()


def ssnr_averages(images, params, labels, k, ctf, snr=1.0, ssnr_floor=SSNR_FLOOR, pad=True, flipped=False, min_count=1, index0=0,
                  ou=None, preprocess=False, device=0, apix=None, index=None):
    """SSNR-weighted averages of the stack on the device (the contract of ssnr_reference): ([k][nx][nx] float32 averages, class
    sizes [k], frc [k][P/2 + 1] float64, resolutions), all numpy; resolutions = {"res_05", "res_0143", "units"} at FRC 0.5 and
    0.143 in A with apix, or with table_apix(ctf) when the table gives one pixel size, else in pixels.  index0: the global index of
    images[0] (the half split), or index: every particle's global index [n] (a subset that keeps its original split); the other
    arguments as for wiener_averages"""
    import torch
    check_ssnr(k, ssnr_floor)
    dev, x, prm, lab, tab = _device_stack(images, params, labels, k, ctf, snr, ou, preprocess, device)
    nx = int(x.shape[-1])
    with torch.cuda.device(dev):
        num2, den2, counts2 = new_half_sums(k, nx, pad, dev)
        accumulate_halves(x, prm, lab, k, tab, num2, den2, counts2, index0, pad, flipped, index)
        f, reg = frc(num2, den2, counts2, nx, pad, snr, min_count, ssnr_floor)
        out = finalize_ssnr(num2, den2, counts2, reg, nx, pad, min_count)
        counts = counts2.sum(1).cpu().numpy()
        f = f.cpu().numpy()
        res = resolutions(f, counts, nx, pad, apix if apix is not None else table_apix(tab, nx), min_count)
        return out.cpu().numpy(), counts, f, res


def score(images, params, labels, k, table, num, den, counts, snr=1.0, reg=None, leave_one_out=True, band=None, pad=True,
          flipped=False, min_count=1):
    """ra_wiener_score on the current stream: {"cc" [n], "scale" [n], "sums" [n][3] float64} (numpy) of images [n][nx][nx]
    (contiguous float32 CUDA tensor) against the class sums num / den / counts (new_sums' layout, as `accumulate` left them; only
    read).  reg: the per-shell term [k][P/2 + 1] (float32 CUDA tensor, `frc`'s) instead of 1/snr; band: (s_lo, s_hi), default
    (1, P/2).  The band, snr, k and reg's shape are checked here (WienerError) before anything is launched; labels, params and
    table rows as by `accumulate`"""
    import torch
    from . import api
    assert images.is_cuda and images.is_contiguous() and images.dtype == torch.float32, "images: contiguous float32 CUDA tensor"
    assert images.dim() == 3 and images.shape[1] == images.shape[2], "images: [n][nx][nx]"
    n, nx = int(images.shape[0]), int(images.shape[-1])
    prm = np.asarray(params, np.float64)
    lab = np.asarray(labels).astype(np.int64)
    tab = np.ascontiguousarray(table, np.float32)
    if prm.shape != (n, 4) or lab.shape != (n,) or tab.shape != (n, 9):
        raise WienerError("need params [%d][4], labels [%d] and a table [%d][9], got %s, %s, %s" % (n, n, n, prm.shape, lab.shape, tab.shape))
    if not (isinstance(k, (int, np.integer)) and 1 <= k <= MAX_K):
        raise WienerError("need 1 <= k <= %d, got %r" % (MAX_K, k))
    if n and (lab.min() < 0 or lab.max() >= k):
        raise WienerError("labels must lie in 0 .. %d, got %d .. %d" % (k - 1, lab.min(), lab.max()))
    P = 2 * nx if pad else nx
    lo, hi, _ = check_score(nx, pad, k, snr, None if reg is None else np.zeros((k, P // 2 + 1)), band)
    shp = (k, P, P // 2 + 1)
    for t, s, dt in ((num, shp + (2,), torch.float32), (den, shp, torch.float32), (counts, (k,), torch.int32)):
        assert t.is_cuda and t.is_contiguous() and t.dtype == dt and tuple(t.shape) == s and t.device == images.device, \
            "sums: new_sums(k, nx, pad) on the images' device"
    if reg is not None:
        if not (hasattr(reg, "is_cuda") and reg.is_cuda and reg.is_contiguous() and reg.dtype == torch.float32
                and tuple(reg.shape) == (k, P // 2 + 1) and reg.device == images.device):
            raise WienerError("reg: frc()'s contiguous float32 [%d][%d] on the images' device" % (k, P // 2 + 1))
    rec = np.zeros(n, api.RESULT_DTYPE)
    rec["alpha"], rec["sx"], rec["sy"] = prm[:, 0], prm[:, 1], prm[:, 2]
    rec["mirror"] = (prm[:, 3] != 0).astype(np.int32)
    rec["ref_id"] = lab.astype(np.int32)
    d_rec = torch.from_numpy(rec.view(np.uint8)).to(images.device)
    sums = torch.zeros((n, 3), dtype=torch.float64, device=images.device)
    L = Launcher(images)
    with torch.cuda.device(images.device):
        L.call("ra_wiener_score", ptr(images), n, nx, ptr(d_rec), tab.ctypes.data_as(api.float_ptr), int(bool(pad)), int(bool(flipped)),
               int(k), ptr(num), ptr(den), ptr(counts), float(snr), ptr(reg), int(bool(leave_one_out)), lo, hi, ptr(sums))
        h_sums, h_counts = sums.cpu().numpy(), counts.cpu().numpy()
    cc, scale = scores_from_sums(h_sums, lab, h_counts, leave_one_out, min_count)
    return {"cc": cc, "scale": scale, "sums": h_sums}


def particle_scores(images, params, labels, k, ctf, snr=1.0, ssnr=False, ssnr_floor=SSNR_FLOOR, leave_one_out=True, band=None,
                    pad=True, flipped=False, min_count=1, index0=0, ou=None, preprocess=False, device=0):
    """every particle of the stack against its class's Wiener estimate, on the device: ({"cc", "scale", "sums"}, class sizes [k]),
    numpy (the contract of score_reference on the stack's own sums).  ssnr=False: accumulate, then score with 1/snr.  ssnr=True:
    the half sums (index0 as for ssnr_averages), the FRC's per-shell term, and the score against N0 + N1, D0 + D1 with that term;
    snr then only sets the half averages.  The other arguments as for wiener_averages"""
    import torch
    if ssnr:
        check_ssnr(k, ssnr_floor)
    dev, x, prm, lab, tab = _device_stack(images, params, labels, k, ctf, snr, ou, preprocess, device)
    nx = int(x.shape[-1])
    check_score(nx, pad, k, snr, None, band)
    with torch.cuda.device(dev):
        if not ssnr:
            num, den, counts = new_sums(k, nx, pad, dev)
            accumulate(x, prm, lab, k, tab, num, den, counts, pad, flipped)
            reg = None
        else:
            num2, den2, counts2 = new_half_sums(k, nx, pad, dev)
            accumulate_halves(x, prm, lab, k, tab, num2, den2, counts2, index0, pad, flipped)
            _, reg = frc(num2, den2, counts2, nx, pad, snr, min_count, ssnr_floor)
            num, den = (num2[:, 0] + num2[:, 1]).contiguous(), (den2[:, 0] + den2[:, 1]).contiguous()
            counts = counts2.sum(1).to(torch.int32).contiguous()
        res = score(x, prm, lab, k, tab, num, den, counts, snr, reg, leave_one_out, band, pad, flipped, min_count)
        return res, counts.cpu().numpy()


# ---- command line

def read_params_and_labels(path, n):
    """(params [n][4], labels [n] or None) from a params.txt (6 columns, with classes) or an initial2Dparams.txt (4 columns)"""
    from . import kmeans, sdr
    try:
        prm = sdr.read_params(path, n)
        rows = np.loadtxt(path, ndmin=2)
        lab = kmeans.read_truth(path, n) if rows.shape[1] == 6 else None
    except (sdr.SdrError, kmeans.KMeansError, OSError, ValueError) as e:
        raise WienerError(str(e))
    return prm, lab


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.wiener")
    ap.add_argument("stack", help=".hdf, .mrcs or .npy stack")
    ap.add_argument("params", help="params.txt (idx angle sx sy mirror class) or initial2Dparams.txt (alpha sx sy mirror)")
    ap.add_argument("ctf", help="CTF table: [n][9] .npy or RELION .star")
    ap.add_argument("output", help="OUT.{hdf,mrcs,npy}: the k averages")
    ap.add_argument("--labels", default=None, help="[n] int .npy: the classes, instead of the params file's")
    ap.add_argument("--k", type=int, default=None, help="number of classes (default: largest label + 1)")
    ap.add_argument("--snr", type=float, default=1.0, help="the Wiener constant: divide by sum c^2 + 1/snr")
    ap.add_argument("--nopad", action="store_true", help="P = nx instead of the 2x zero-padded P = 2 nx")
    ap.add_argument("--flipped", action="store_true", help="the particles are phase-flipped already: weights |c|")
    ap.add_argument("--min_count", type=int, default=1, help="classes with fewer members are written as zeros")
    ap.add_argument("--apix", type=float, default=None, help="pixel size (A) for a .star file that gives none")
    ap.add_argument("--ou", type=int, default=None, help="subtract the mean under model_circle(ou) from every particle first")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ssnr", action="store_true",
                    help="SSNR-weighted averages: the per-shell term from the half-set FRC replaces 1/snr (--snr then only sets the "
                         "half averages); prints each class's resolution at FRC 0.5 and 0.143")
    ap.add_argument("--ssnr_floor", type=float, default=SSNR_FLOOR, help="lower bound of the per-shell SSNR (with --ssnr)")
    ap.add_argument("--frc", default=None, metavar="FRC.npz",
                    help="with --ssnr: write frc [k][P/2 + 1], freq (cycles/pixel), counts, res_05, res_0143 and units here")
    ap.add_argument("--scores", default=None, metavar="SCORES.npz",
                    help="score every particle against its class's Wiener estimate (with --ssnr: the per-shell term) and write cc, "
                         "scale, sums, labels, counts and the options used here")
    ap.add_argument("--band", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                    help="with --scores: the shells LO .. HI that are compared (default 1 .. P/2)")
    ap.add_argument("--no_leave_one_out", action="store_true",
                    help="with --scores: compare with the class's estimate as it is, the particle's own term included")
    ap.add_argument("--keep", type=float, default=None, metavar="F",
                    help="with --scores: keep the best fraction F of every class by cc; OUT (and --frc) then come from the kept "
                         "particles, and SCORES.npz gets the mask `keep`")
    ap.add_argument("--min_cc", type=float, default=None, metavar="T", help="with --scores: keep the particles with cc >= T")
    args = ap.parse_args(argv)
    if not args.scores:
        for flag, given in (("--keep", args.keep is not None), ("--min_cc", args.min_cc is not None), ("--band", args.band is not None),
                            ("--no_leave_one_out", args.no_leave_one_out)):
            if given:
                ap.error("%s needs --scores" % flag)
    if args.keep is not None and not 0 < args.keep <= 1:
        ap.error("--keep needs 0 < F <= 1, got %g" % args.keep)
    if args.min_cc is not None and np.isnan(args.min_cc):
        ap.error("--min_cc needs a number")
    from . import stackio
    try:
        stack = np.ascontiguousarray(stackio.read_stack(args.stack), np.float32)
        if stack.ndim != 3 or stack.shape[1] != stack.shape[2]:
            raise WienerError("%s: need a stack of square images, got shape %s" % (args.stack, stack.shape))
        n, nx = stack.shape[0], stack.shape[-1]
        prm, lab = read_params_and_labels(args.params, n)
        if args.labels:
            lab = np.load(args.labels)
        if lab is None:
            lab = np.zeros(n, np.int64)
        lab = np.asarray(lab)
        k = args.k if args.k is not None else (int(lab.max()) + 1 if n else 1)
        tab = _ctf.load_table(args.ctf, n, nx, args.apix)
        check_inputs(n, nx, prm, lab, k, tab, args.snr)
        if args.ssnr:
            check_ssnr(k, args.ssnr_floor)
        elif args.frc:
            raise WienerError("--frc needs --ssnr")
    except (WienerError, _ctf.CtfTableError, OSError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    if args.scores:
        try:
            check_score(nx, not args.nopad, k, args.snr, None, args.band)
        except WienerError as e:
            ap.error("--scores: %s" % e)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: the averages run on the device (wiener_reference is the float64 checker)")
    index = None
    if args.scores:
        res, counts = particle_scores(stack, prm, lab, k, tab, args.snr, args.ssnr, args.ssnr_floor, not args.no_leave_one_out,
                                      args.band, not args.nopad, args.flipped, args.min_count, ou=args.ou,
                                      preprocess=args.ou is not None, device=args.device)
        P = 2 * nx if not args.nopad else nx
        band = tuple(args.band) if args.band else (min(1, P // 2), P // 2)
        extra = {}
        pruned = args.keep is not None or args.min_cc is not None
        if pruned:
            mask = select(res["cc"], lab, k, args.keep, args.min_cc)
            extra["keep"] = mask
        np.savez(args.scores, cc=res["cc"], scale=res["scale"], sums=res["sums"], labels=lab.astype(np.int64), counts=counts,
                 band=np.array(band), leave_one_out=not args.no_leave_one_out, snr=args.snr, ssnr=args.ssnr,
                 ssnr_floor=args.ssnr_floor, flipped=args.flipped, pad=not args.nopad, min_count=args.min_count, **extra)
        print("%s: scores of %d particles in %d classes (shells %d .. %d%s%s)"
              % (args.scores, n, k, band[0], band[1], "" if not args.no_leave_one_out else ", no leave-one-out",
                 ", per-shell term" if args.ssnr else ", snr %g" % args.snr))
        if pruned:
            for j in range(k):
                m = lab == j
                c = res["cc"][m & mask]
                c = c[~np.isnan(c)]
                print("  class %3d: %7d particles, %7d kept   min cc %8.4f   median cc %8.4f"
                      % (j, m.sum(), (m & mask).sum(), c.min() if c.size else np.nan, np.median(c) if c.size else np.nan))
            index = np.nonzero(mask)[0]
            stack, prm, lab, tab, n = stack[index], prm[index], lab[index], tab[index], len(index)
    if not args.ssnr:
        avg, counts = wiener_averages(stack, prm, lab, k, tab, args.snr, not args.nopad, args.flipped, args.min_count, ou=args.ou,
                                      preprocess=args.ou is not None, device=args.device)
        stackio.write_stack(args.output, avg)
        print("%s: %d CTF-corrected averages of %d particles (%d x %d, snr %g%s), class sizes %s"
              % (args.output, k, n, nx, nx, args.snr, ", flipped" if args.flipped else "", " ".join(str(int(c)) for c in counts)))
        return 0
    avg, counts, f, res = ssnr_averages(stack, prm, lab, k, tab, args.snr, args.ssnr_floor, not args.nopad, args.flipped,
                                        args.min_count, ou=args.ou, preprocess=args.ou is not None, device=args.device,
                                        apix=args.apix, index=index)
    stackio.write_stack(args.output, avg)
    P = 2 * nx if not args.nopad else nx
    if args.frc:
        np.savez(args.frc, frc=f, freq=np.arange(P // 2 + 1) / P, counts=counts, res_05=res["res_05"], res_0143=res["res_0143"],
                 units=res["units"])
    print("%s: %d SSNR-weighted averages of %d particles (%d x %d, half averages at snr %g, floor %g%s); resolution in %s%s"
          % (args.output, k, n, nx, nx, args.snr, args.ssnr_floor, ", flipped" if args.flipped else "", res["units"],
             "" if res["units"] == "A" else " (no single pixel size: give --apix)"))
    for j in range(k):
        print("  class %3d: %7d particles   FRC 0.5: %8.2f %s   FRC 0.143: %8.2f %s"
              % (j, counts[j], res["res_05"][j], res["units"], res["res_0143"][j], res["units"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
