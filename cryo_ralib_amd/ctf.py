"""CTF parameter tables for the phase flip (api.phase_flip / ra_phase_flip), host only.

A table is float [N][9] in the layout of the reference's utils_ralib.parse_ctf_star:
(D, Apix, DefocusU, DefocusV, DefocusAngle, Voltage, Cs, w, PhaseShift) in A, A, A, A, degrees, kV, mm, -, degrees.
D is the box the parameters belong to: a stack binned from D to nx pixels is flipped with apix_eff = Apix * D / nx.

Sources:
  * `.npy`   the table itself, [N][9];
  * `.star`  RELION 3.0 (one data block with the CTF columns on every particle) or RELION 3.1+ (`data_optics` joined to
             `data_particles` through `_rlnOpticsGroup`).  Pixel size: `_rlnImagePixelSize`, else
             `_rlnDetectorPixelSize * 1e4 / _rlnMagnification` (parse_ctf_star's rule), else the caller's `apix`; none of
             them is an error (parse_ctf_star's silent 1 A is not used).  D: `_rlnImageSize`, else the stack's nx.
             `_rlnPhaseShift` is 0 where absent.

`flip_reference` is the float64 numpy statement of the flip that the tests hold the device against.
"""
import os

import numpy as np

COLUMNS = ("D", "Apix", "DefocusU", "DefocusV", "DefocusAngle", "Voltage", "Cs", "w", "PhaseShift")
_STAR_CTF = ("_rlnDefocusU", "_rlnDefocusV", "_rlnDefocusAngle", "_rlnVoltage", "_rlnSphericalAberration",
             "_rlnAmplitudeContrast", "_rlnPhaseShift")


class CtfTableError(ValueError):
    pass


# ---- STAR files

def read_star(path):
    """{block name: {column: [str values]}} of every loop_ block (and key / value pairs of non-loop blocks)"""
    blocks, name, cols, rows, in_loop = {}, None, [], [], False

    def close():
        if name is not None and cols:
            blocks[name] = {c: [r[i] for r in rows] for i, c in enumerate(cols)}

    with open(path) as f:
        for raw in f:
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            if line.startswith("data_"):
                close()
                name, cols, rows, in_loop = line[5:], [], [], False
                continue
            if line == "loop_":
                in_loop = True
                continue
            if line.startswith("_"):
                parts = line.split()
                if in_loop and not rows:
                    cols.append(parts[0])
                elif not in_loop and len(parts) >= 2:
                    cols.append(parts[0])
                    if not rows:
                        rows.append([])
                    rows[0].append(parts[1])
                continue
            if in_loop:
                vals = line.split()
                if len(vals) != len(cols):
                    raise CtfTableError("%s: block data_%s: a row has %d values for %d columns" % (path, name, len(vals), len(cols)))
                rows.append(vals)
        close()
    return blocks


def _floats(block, key, n, default=None):
    if key in block:
        return np.array([float(v) for v in block[key]], np.float64)
    if default is None:
        return None
    return np.full(n, float(default), np.float64)


def _check_image_names(names, n, path):
    """`k@file` indices of one file must run 1 .. n in order"""
    idx, files = [], set()
    for s in names:
        if "@" not in s:
            return
        k, fn = s.split("@", 1)
        try:
            idx.append(int(k))
        except ValueError:
            return
        files.add(fn)
    if len(files) != 1:
        return
    if idx != list(range(1, n + 1)):
        raise CtfTableError("%s: _rlnImageName indices do not run 1..%d in order: the table rows do not match the stack's "
                            "images one by one" % (path, n))


def star_table(path, nx, apix=None):
    """[N][9] float64 from a RELION 3.0 or 3.1+ STAR file"""
    blocks = read_star(path)
    if "particles" in blocks and "optics" in blocks:
        parts, optics = blocks["particles"], blocks["optics"]
        if "_rlnOpticsGroup" not in parts or "_rlnOpticsGroup" not in optics:
            raise CtfTableError("%s: data_optics and data_particles without _rlnOpticsGroup" % path)
        gid = {g: i for i, g in enumerate(optics["_rlnOpticsGroup"])}
        try:
            rows = [gid[g] for g in parts["_rlnOpticsGroup"]]
        except KeyError as e:
            raise CtfTableError("%s: particle of optics group %s, which data_optics does not list" % (path, e))
        merged = dict(parts)
        for k, v in optics.items():
            if k not in merged:
                merged[k] = [v[r] for r in rows]
        block = merged
    else:
        cands = [b for b in blocks.values() if "_rlnDefocusU" in b]
        if len(cands) != 1:
            raise CtfTableError("%s: expected one data block with _rlnDefocusU, found %d" % (path, len(cands)))
        block = cands[0]
    n = len(block["_rlnDefocusU"])
    for k in _STAR_CTF[:-1]:
        if k not in block:
            raise CtfTableError("%s: no %s column" % (path, k))
    if "_rlnImageName" in block:
        _check_image_names(block["_rlnImageName"], n, path)
    ap = _floats(block, "_rlnImagePixelSize", n)
    if ap is None and "_rlnDetectorPixelSize" in block and "_rlnMagnification" in block:
        ap = _floats(block, "_rlnDetectorPixelSize", n) * 1.0e4 / _floats(block, "_rlnMagnification", n)
    if ap is None and apix is not None:
        ap = np.full(n, float(apix))
    if ap is None:
        raise CtfTableError("%s: no pixel size (_rlnImagePixelSize, _rlnDetectorPixelSize / _rlnMagnification): give --apix" % path)
    D = _floats(block, "_rlnImageSize", n, default=nx)
    t = np.zeros((n, 9), np.float64)
    t[:, 0], t[:, 1] = D, ap
    for i, k in enumerate(_STAR_CTF):
        t[:, i + 2] = _floats(block, k, n, default=0.0 if k == "_rlnPhaseShift" else None)
    return t


# ---- any table

def load_table(path, n, nx, apix=None, lo=0, hi=None):
    """rows lo:hi of the table at `path` for a stack of n images of nx pixels, float32 [hi - lo][9]; the row count must be n"""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".npy":
        t = np.load(path).astype(np.float64)
        if t.ndim != 2 or t.shape[1] != 9:
            raise CtfTableError("%s: a CTF table is [N][9] (%s), got shape %s" % (path, ", ".join(COLUMNS), t.shape))
    elif ext == ".star":
        t = star_table(path, nx, apix)
    else:
        raise CtfTableError("%s: CTF tables are .npy ([N][9]) or RELION .star" % path)
    if t.shape[0] != n:
        raise CtfTableError("%s: %d CTF rows for a stack of %d images" % (path, t.shape[0], n))
    check_table(t, path)
    hi = n if hi is None else hi
    return np.ascontiguousarray(t[lo:hi], np.float32)


def check_table(t, what="CTF table"):
    """the ranges ra_phase_flip accepts, with the row that breaks them"""
    t = np.asarray(t, np.float64)
    bad = ~np.isfinite(t).all(1) | (t[:, 0] <= 0) | (t[:, 1] <= 0) | (t[:, 5] <= 0) | (t[:, 7] < 0) | (t[:, 7] >= 1)
    if bad.any():
        raise CtfTableError("%s: row %d out of range (finite values, D > 0, Apix > 0, voltage > 0, 0 <= w < 1 needed)"
                            % (what, int(np.nonzero(bad)[0][0])))


# ---- the contract in float64 numpy

def ctf_grid(row, nx, P):
    """ctf_np on the rfft2 grid [P][P/2 + 1] of a P x P image of a stack of box nx: x = ix / (P apix_eff) along the fast axis,
    y = the signed row frequency (numpy.fft.fftfreq order), apix_eff = Apix * D / nx"""
    D, apix, dfu, dfv, dfang, volt, cs, w, ps = [float(v) for v in row]
    a = apix * D / nx
    x = np.arange(P // 2 + 1)[None, :] / (P * a)
    y = (np.fft.fftfreq(P) * P)[:, None] / (P * a)
    volt, cs = volt * 1000, cs * 1e7
    dfang, ps = dfang * np.pi / 180, ps * np.pi / 180
    lam = 12.2639 / np.sqrt(volt + 0.97845e-6 * volt ** 2)
    ang = np.arctan2(y, x)
    s2 = x ** 2 + y ** 2
    df = .5 * (dfu + dfv + (dfu - dfv) * np.cos(2 * (ang - dfang)))
    gamma = 2 * np.pi * (-.5 * df * lam * s2 + .25 * cs * lam ** 3 * s2 ** 2) - ps
    return np.sqrt(1 - w ** 2) * np.sin(gamma) - w * np.cos(gamma)


def multiplier(row, nx, P):
    """m = -sign(ctf), +1 where ctf == 0, on the rfft2 grid [P][P/2 + 1]"""
    c = ctf_grid(row, nx, P)
    return np.where(c > 0, -1.0, 1.0)


def flip_reference(images, table, pad=True):
    """float64 phase flip of images [n][nx][nx] with table [n][9]: embed, rfft2, m, irfft2, crop"""
    images = np.asarray(images, np.float64)
    n, nx = images.shape[0], images.shape[-1]
    P = 2 * nx if pad else nx
    o = (P - nx) // 2
    out = np.empty_like(images)
    for i in range(n):
        big = np.zeros((P, P))
        big[o:o + nx, o:o + nx] = images[i]
        f = np.fft.rfft2(big) * multiplier(table[i], nx, P)
        out[i] = np.fft.irfft2(f, s=(P, P))[o:o + nx, o:o + nx]
    return out
