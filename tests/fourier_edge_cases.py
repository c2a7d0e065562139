"""What the entry-by-entry tests of the Fourier image operators share (tests/test_fourier_edges_cpu.py asserts every property
claimed here without a GPU, tests/test_gpu_fourier_edges.py runs the device on the same inputs against the same bounds):

  * ra_fourier_resize (csrc/ralign_resize.h): the launch plan restated, the shapes at its tile, chunk and load edges, the
    inputs (integers for the identity, impulses that read single operator entries, noise with one bright pixel), the entry-wise
    bounds, a numpy float32 replay of the kernel's two product chains in the kernel's own k order, and the mutants that show the
    bounds have teeth;
  * the gain path of ra_prep_filter (csrc/ralign_prep.h): unit impulses that turn one call into a reading of every table entry,
    the bar from an independent single-precision FFT on the CPU, and its mutants.

Bounds come from term counts, the float32 unit roundoff and the float64 reference, never from a device result."""
import functools

import numpy as np

from cryo_ralib_amd import prep, resize

U = 2.0 ** -24                     # float32 unit roundoff
RS_CHUNK = 64                      # csrc/ralign_resize.h

# ---- resize: the plan and the shapes


def rs_plan(nx, m):
    """rs_make_plan of csrc/ralign_resize.h, restated: (nt tiles per axis, bt tile edge, mp = nt bt, nxp, NCT = bt / 16)"""
    nt = (m + 127) // 128
    bt = ((m + nt - 1) // nt + 15) // 16 * 16
    return dict(nt=nt, bt=bt, mp=nt * bt, nxp=(nx + RS_CHUNK - 1) // RS_CHUNK * RS_CHUNK, nct=bt // 16)


def has_half(nx, m):
    """the source's Nyquist pair lies in the band and carries weights 1/2"""
    return nx % 2 == 0 and nx <= m


# every named edge as a predicate of (nx, m, plan)
EDGES = {
    "nct1": lambda nx, m, p: p["nct"] == 1,
    "nct2": lambda nx, m, p: p["nct"] == 2,
    "nct3": lambda nx, m, p: p["nct"] == 3,
    "nct5": lambda nx, m, p: p["nct"] == 5,
    "nct6": lambda nx, m, p: p["nct"] == 6,
    "nct7": lambda nx, m, p: p["nct"] == 7,
    "nct8": lambda nx, m, p: p["nct"] == 8,
    "nt1": lambda nx, m, p: p["nt"] == 1,
    "nt2": lambda nx, m, p: p["nt"] == 2,
    "nt3": lambda nx, m, p: p["nt"] == 3,
    "break": lambda nx, m, p: p["nct"] ** 2 % 4 != 0,                     # NS % 4 != 0: a wave leaves the subtile loop early
    "full_tile": lambda nx, m, p: m == p["mp"],
    "padded": lambda nx, m, p: p["mp"] > m,
    "last_tile_under_two_thirds": lambda nx, m, p: p["nt"] > 1 and 3 * (m - (p["nt"] - 1) * p["bt"]) < 2 * p["bt"],
    "vec_tail": lambda nx, m, p: nx % 4 == 0 and nx % 8 != 0,             # float4 box whose last group of 8 loads one by one
    "vec": lambda nx, m, p: nx % 4 == 0,
    "scalar_everywhere": lambda nx, m, p: nx % 4 != 0,
    "below_one_k_step": lambda nx, m, p: nx < 32,
    "one_live_column": lambda nx, m, p: nx % 32 == 1 and nx > 32,         # a whole k0 step with one column inside the image
    "one_live_row": lambda nx, m, p: nx % 64 == 1 and nx > 64,            # a whole chunk with one row inside the image
    "up": lambda nx, m, p: m > nx,
    "down": lambda nx, m, p: m < nx,
    "half": lambda nx, m, p: has_half(nx, m),
    "even_no_half": lambda nx, m, p: nx % 2 == 0 and not has_half(nx, m),
    "odd_nx": lambda nx, m, p: nx % 2 == 1,
    "odd_m": lambda nx, m, p: m % 2 == 1,
    "near_tile_edge": lambda nx, m, p: 0 < nx - 128 <= 2 and 0 < m - 128 <= 2,
}

# (nx, m, the edges the case is there for).  9 -> 90 and 12 -> 127 are there for NCT 6 and 8 alone, which no other shape reaches.
RESIZE_CASES = [
    (20, 100, ("nct7", "break", "vec_tail", "below_one_k_step", "up", "half", "nt1", "padded")),
    (100, 112, ("nct7", "full_tile", "vec_tail", "half")),
    (24, 330, ("nt3", "nct7", "padded", "vec", "half")),
    (33, 17, ("one_live_column", "odd_nx", "nct2", "padded", "down")),
    (65, 16, ("one_live_row", "nct1", "full_tile", "one_live_column")),
    (64, 129, ("nt2", "nct5", "last_tile_under_two_thirds", "half", "up", "vec")),
    (66, 40, ("scalar_everywhere", "nct3", "even_no_half")),
    (130, 129, ("near_tile_edge", "nt2", "odd_m", "even_no_half", "padded", "nct5")),
    (9, 90, ("nct6", "padded", "odd_nx", "below_one_k_step")),
    (12, 127, ("nct8", "padded", "vec_tail", "half", "odd_m")),
]
RESIZE_SHAPES = [(nx, m) for nx, m, _ in RESIZE_CASES]
IDENTITY = [1, 7, 63, 64, 65, 97, 100, 112, 130, 200]
UNALIGNED = [(20, 100), (64, 129)]          # R4a: nx % 4 == 0 boxes read from a base 4 bytes past a 16-byte boundary
IMPULSE_STEP = 7                            # image i of the impulse stack is 1 at (i, (7 i + 3) mod nx)


@functools.lru_cache(maxsize=None)
def operator64(nx, m):
    A = resize.operator(nx, m)
    A.setflags(write=False)
    return A


def operator_direct(nx, m):
    """A by its defining cosine sum in long double, arguments reduced as exact integers: independent of the closed form"""
    L = m * nx
    h = min(nx, m) // 2
    p = ((np.arange(m, dtype=np.int64) - m // 2) * nx)[:, None] - ((np.arange(nx, dtype=np.int64) - nx // 2) * m)[None, :]
    acc = np.ones((m, nx), np.longdouble)
    two_pi = np.longdouble(2) * np.arccos(np.longdouble(-1))
    for k in range(1, h + 1):
        w = np.longdouble(0.5 if nx % 2 == 0 and 2 * k == nx else 1.0)
        r = np.mod(k * p, L).astype(np.longdouble) / np.longdouble(L)
        acc += 2 * w * np.cos(two_pi * r)
    return acc / np.longdouble(nx)


def nyquist_term(nx, m):
    """cos(2 pi (nx/2) (t_j - u_i)) / nx: what a Nyquist weight of 1 instead of 1/2 adds to A (has_half shapes)"""
    L = m * nx
    p = ((np.arange(m, dtype=np.int64) - m // 2) * nx)[:, None] - ((np.arange(nx, dtype=np.int64) - nx // 2) * m)[None, :]
    r = np.mod((nx // 2) * p, L).astype(np.float64) / L
    return np.cos(2.0 * np.pi * r) / nx


# ---- resize: inputs

def identity_stack(nx):
    """3 images of integers in [-8, 8], about a third of them zero"""
    rng = np.random.default_rng(1000 + nx)
    x = rng.integers(-8, 9, (3, nx, nx))
    x[rng.random((3, nx, nx)) < 1.0 / 3.0] = 0
    return x.astype(np.float32)


def impulse_columns(nx):
    return (IMPULSE_STEP * np.arange(nx) + 3) % nx


def impulse_stack(nx):
    """nx images; image i is 1 at (i, (7 i + 3) mod nx): rows and columns decoupled, so a transposed output fails"""
    x = np.zeros((nx, nx, nx), np.float32)
    i = np.arange(nx)
    x[i, i, impulse_columns(nx)] = 1.0
    return x


def impulse_reference(nx, m):
    """y_ref of the impulse stack: image i is the outer product of columns i and c_i of A"""
    A = operator64(nx, m)
    return np.einsum("ji,li->ijl", A, A[:, impulse_columns(nx)])


def impulse_bound(ref):
    """R2: three roundings (two operator entries, one product) and the absolute error of the closed form near A = 0"""
    return 3.0 * U * np.abs(ref) + 2.0 ** -40


def bright_stack(nx):
    """3 images of standard normal noise with one pixel at 1e4 (a max-norm bar would leave the rest unchecked)"""
    rng = np.random.default_rng(2000 + nx)
    x = rng.standard_normal((3, nx, nx)).astype(np.float32)
    for i in range(3):
        x[i, rng.integers(nx), rng.integers(nx)] = 1e4
    return x


def reference(x, nx, m):
    A = operator64(nx, m)
    return np.einsum("ji,nik,lk->njl", A, x.astype(np.float64), A, optimize=True)


def general_bound(x, nx, m):
    """R3: (K1 + K2 + 3) u |A| |x| |A|^T; K1, K2 the lengths of the two float32 chains as the kernel runs them, padding included"""
    A = np.abs(operator64(nx, m))
    k1, k2 = 32 * ((nx + 31) // 32), 64 * ((nx + 63) // 64)
    return (k1 + k2 + 3) * U * np.einsum("ji,nik,lk->njl", A, np.abs(x).astype(np.float64), A, optimize=True)


def white_stack(nx, m):
    """the input of tests/test_gpu_resize.py::test_matches_the_float64_checker at 5 images"""
    return np.random.default_rng(nx * 7 + m).standard_normal((5, nx, nx)).astype(np.float32)


# ---- resize: the float32 replay

def _fma32(acc, a, b):
    """float32(acc + a b) with the float32 product a b exact in double (one extra rounding to double, 2^-29 of a float32 ulp)"""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def replay(x, A32):
    """y = A32 x A32^T as resize_kernel forms it: T = x A^T over k in steps of 32 (8 MFMAs, each adding k0 + s, k0 + 8 + s,
    k0 + 16 + s, k0 + 24 + s), y accumulated over chunks of 64 rows of T in the same order; zero padding beyond nx included"""
    n, nx = x.shape[0], x.shape[-1]
    m = A32.shape[0]
    nxp = (nx + RS_CHUNK - 1) // RS_CHUNK * RS_CHUNK
    xp = np.zeros((n, nxp, nxp), np.float32)
    xp[:, :nx, :nx] = x
    Ap = np.zeros((m, nxp), np.float32)
    Ap[:, :nx] = A32
    order32 = [8 * b + s for s in range(8) for b in range(4)]
    T = np.zeros((n, nxp, m), np.float32)
    for k0 in range(0, nx, 32):
        for d in order32:
            k = k0 + d
            T = _fma32(T, xp[:, :, k, None], Ap[None, None, :, k])
    y = np.zeros((n, m, m), np.float32)
    for r0 in range(0, nx, RS_CHUNK):
        for q0 in (0, 32):
            for d in order32:
                q = r0 + q0 + d
                y = _fma32(y, Ap[None, :, q, None], T[:, None, q, :])
    return y


def impulse_replay(nx, A32):
    """the replay of the impulse stack in closed form: T holds one column of A32 unchanged, every y is one rounded product"""
    return (A32.astype(np.float64).T[:, :, None] * A32.astype(np.float64)[:, impulse_columns(nx)].T[:, None, :]).astype(np.float32)


# ---- resize: mutants

def far_entry(nx, m):
    """(j, i) of the largest |A| below 1e-3 and above 1e-6, or None where the operator has no such entry"""
    A = np.abs(operator64(nx, m))
    ok = (A < 1e-3) & (A > 1e-6)
    if not ok.any():
        return None
    return tuple(int(v) for v in np.unravel_index(np.argmax(np.where(ok, A, 0.0)), A.shape))


def operator_mutants(nx, m):
    """{name: mutated float32 operator} for the mutants that act on A"""
    A32 = operator64(nx, m).astype(np.float32)
    out = {}
    if nx > 1:
        a = A32.copy()
        a[:, nx - 1] = 0.0
        out["last source column zeroed"] = a
    if has_half(nx, m) and m > 1:
        out["Nyquist weight 1"] = (operator64(nx, m) + nyquist_term(nx, m)).astype(np.float32)
    ji = far_entry(nx, m)
    if ji is not None:
        a = A32.copy()
        a[ji] = np.float32(1.01) * a[ji]
        out["far entry times 1.01"] = a
    return out


def swap_rows(y):
    """rows j and j ^ 4 of every image exchanged where both exist (the f64 MFMA's C/D lane map used by mistake)"""
    m = y.shape[1]
    j = np.arange(m)
    src = np.where((j ^ 4) < m, j ^ 4, j)
    return y[:, src, :]


# ---- filter

FILTERS = [(("tanl", 0.2, 0.1), None), (("gauss", 0.15), None), (("tanl", 0.3, 0.2), ("gauss", 0.03)), (None, ("tanl", 0.05, 0.5))]
# box: the radices pf_make_plan (csrc/ralign_ctf.h) gives it, 4s first, then 2, 3, 5, then any other prime
FILTER_BOXES = {8: (4, 2), 9: (3, 3), 15: (3, 5), 14: (2, 7), 26: (2, 13), 45: (3, 3, 5), 64: (4, 4, 4), 90: (2, 3, 3, 5)}
IMPULSES = [(0, 0), (3, 5)]
PF_FIXED_NOPAD = (90,)             # PF_FIXED_BOXES with pad 0


def pf_radices(P):
    """the radices of pf_make_plan, restated"""
    out, r = [], P
    while r % 4 == 0:
        out.append(4)
        r //= 4
    f = 2
    while f <= r:
        if r % f == 0:
            out.append(f)
            r //= f
        else:
            f += 1
    return tuple(out)


def pf_batch(nx):
    """(nb columns per FFT batch, block in LDS) of pf_make_plan(nx, pad = 0), restated"""
    cap, P, H = (160 * 1024 - 1024) // 8, nx, nx // 2 + 1
    blk = nx * H
    gblk = P + 2 * P * 16 + blk > cap
    nb = (cap - P - (0 if gblk else blk)) // (2 * P)
    if gblk:
        nb = min(nb, 8)
    else:
        two = (78 * 1024 // 8 - P - blk) // (2 * P)
        if two >= 4:
            nb = two
        nb = min(nb, 32)
    return nb, not gblk


def filter_cases():
    return [(nx, f, k) for nx in FILTER_BOXES for f in range(len(FILTERS)) for k in range(len(IMPULSES))]


def impulse_images(nx):
    x = np.zeros((len(IMPULSES), nx, nx), np.float32)
    for k, (r, c) in enumerate(IMPULSES):
        x[k, r, c] = 1.0
    return x


def gain(nx, f, iy, ix):
    """g in float64 at integer frequencies (iy, ix) of the nx grid, iy of any sign or size: prep's profiles, restated"""
    d = np.sqrt((np.asarray(ix, np.int64) ** 2 + np.asarray(iy, np.int64) ** 2).astype(np.float64)) / nx

    def term(spec):
        if spec[0] == "tanl":
            k = np.pi / (2.0 * spec[2] * spec[1])
            return 0.5 * (np.tanh(k * (d + spec[1])) - np.tanh(k * (d - spec[1])))
        return np.exp(-d * d / (2.0 * spec[1] * spec[1]))

    lp, hp = FILTERS[f]
    g = term(lp) if lp else np.ones_like(d)
    return g * (1.0 - term(hp)) if hp else g


def gain32(nx, f):
    """the table as the device rounds it: float32 of prep.filter_multiplier, [nx][nx/2 + 1] over (iy in fftfreq order, ix)"""
    lp, hp = FILTERS[f]
    return prep.filter_multiplier(nx, nx, lp, hp).astype(np.float32)


def expected_spectrum(nx, f):
    """g32 rfft2(x) of the impulse images in float64"""
    return gain32(nx, f).astype(np.float64) * np.fft.rfft2(impulse_images(nx).astype(np.float64))


def spectrum_error(y, nx, f):
    """per image: max over every coefficient, Nyquist row and column included, of |Re| and |Im| of rfft2(float64(y)) - g32 rfft2(x)"""
    d = np.fft.rfft2(np.asarray(y, np.float64)) - expected_spectrum(nx, f)
    return np.maximum(np.abs(d.real), np.abs(d.imag)).reshape(d.shape[0], -1).max(axis=1)


def filter32(x, g):
    """irfft2(g rfft2(x)) in single precision on the CPU (torch.fft on float32 / complex64 tensors): an FFT independent of the
    device's Stockham passes"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32))
    X = torch.fft.rfft2(t) * torch.from_numpy(np.ascontiguousarray(g, np.float32))
    return torch.fft.irfft2(X, s=(x.shape[-2], x.shape[-1])).numpy()


@functools.lru_cache(maxsize=None)
def e32(nx, f):
    """E32 per impulse image: spectrum_error of the single-precision CPU filter"""
    return spectrum_error(filter32(impulse_images(nx), gain32(nx, f)), nx, f)


def filter_bar(nx, f):
    """F1: 16 max(E32, u) per impulse image.  16: the device's direct prime stages add R terms where pocketfft's do not, and its
    twiddles are table entries rounded to float32; nothing else differs"""
    return 16.0 * np.maximum(e32(nx, f), U)


def table_unmirrored(nx, f):
    """the table read with ay = n instead of |iy|: rows past the middle take the gain of the unsigned row index"""
    n = np.arange(nx, dtype=np.int64)[:, None]
    ix = np.arange(nx // 2 + 1, dtype=np.int64)[None, :]
    return gain(nx, f, n, ix).astype(np.float32)


STOP_BAND = (2e-5, 1e-3)           # a doubled gain moves by at least twice the cap (1e-5) that the CPU file asserts for the F1 bar


def stop_band_entry(nx, f):
    """(|iy|, ix) of the smallest table entry with 2e-5 <= g < 1e-3; None where the filter has no such gain on this grid"""
    g = gain32(nx, f).astype(np.float64)[:nx // 2 + 1]
    ok = (g >= STOP_BAND[0]) & (g < STOP_BAND[1])
    if not ok.any():
        return None
    return tuple(int(v) for v in np.unravel_index(np.argmin(np.where(ok, g, np.inf)), g.shape))


def table_stop_band_doubled(nx, f):
    """one table entry doubled: it serves the rows +iy and -iy"""
    at = stop_band_entry(nx, f)
    if at is None:
        return None
    ay, ix = at
    g = gain32(nx, f).copy()
    g[ay, ix] *= np.float32(2.0)
    if 0 < ay and nx - ay != ay:
        g[nx - ay, ix] *= np.float32(2.0)
    return g


def white_images(nx):
    """the input of tests/test_gpu_prep.py::test_filter_matches_the_checker"""
    return np.random.default_rng(nx).standard_normal((3, nx, nx)).astype(np.float32)
