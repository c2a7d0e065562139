"""Particle preprocessing: background normalisation with optional plane (ramp) removal and contrast inversion, and a Fourier
low-pass / high-pass / band-pass filter.

    python -m cryo_ralib_amd.prep IN OUT [--norm_bg R] [--ramp] [--invert] [--ctf TABLE [--apix A] [--nopad]]
        [--lowpass_tanl FL AA | --lowpass_gauss S] [--highpass_tanl FL AA | --highpass_gauss S] [--filter_pad] [--res]
        [--box M] [--stats STATS.npy] [--batch B] [--backend device|numpy] [--device D]

The contract is this project's own statement.  Centre c = nx//2, u = col - c, v = row - c, as model_circle
and rot_shift2D use.  Every particle is independent of the others and of its place in the batch.

N -- background normalisation of an image x of box nx, 4 <= nx <= 1024, with the real radius R, 1 <= R <= nx/2:
  1. B = {(v, u) : u^2 + v^2 > R^2} (at least the 4 corners, never on one line).
  2. ramp: (a, b, c) = argmin sum_B (x - a - b u - c v)^2 = G^-1 m, G = sum_B [1,u,v]^T [1,u,v] (exact integers, inverted in
     double), m = sum_B x [1,u,v] in double; e = x - (a + b u + c v) on ALL pixels.  Without ramp (a, b, c) = 0 and e = x.
  3. mu = (sum_B e) / |B|, sigma^2 = (sum_B (e - mu)^2) / |B|: the population variance, in two passes.
  4. y = s (e - mu) / sigma, s = -1 with invert and +1 otherwise, formed in double and rounded to float32 once; sigma == 0 gives
     y = s (e - mu) and the stored sigma is 0.
  5. statistics [n][5] double: (a, b, c, mu, sigma).
  6. every sum over pixels is double, in an order fixed by (nx, R) alone; no atomics; bitwise reproducible.
  7. a particle with a non-finite pixel gets NaN pixels and NaN statistics; its neighbours are untouched.
This follows the definition of RELION's --norm --bg_radius (plane fit on the background, then background mean 0 and sigma 1);
nothing pins it against RELION.

F -- Fourier filter of an image of box nx, 2 <= nx <= 1024: embed at (P - nx)/2 in a P x P zero image (P = nx, periodic as
filt_tanl, or P = 2 nx with pad), real 2-D DFT, multiply by g(d), d = sqrt(ix^2 + iy^2) / P cycles per pixel (ix = 0 .. P/2, iy
signed in fftfreq order), inverse DFT, keep the nx x nx window.  g = LP (1 - HP), each of LP and HP absent (LP = 1, HP = 0) or
  ("tanl", fl, aa):  1/2 [tanh(k (d + fl)) - tanh(k (d - fl))], k = pi / (2 aa fl), 0 < fl < 1, aa > 0 (filt_tanl's profile);
  ("gauss", s):      exp(-d^2 / (2 s^2)), s > 0;
at least one of them present.  g is evaluated in double and rounded to float32 once per coefficient; the product and the
transforms are float32 on the device (the phase flip's passes, csrc/ralign_ctf.h).

backend="device" runs ra_prep_normalize / ra_prep_filter (csrc/ralign_prep.h) in place on a contiguous float32 CUDA tensor
[n][nx][nx], on the current stream; backend="numpy" is the float64 checker: it copies its input and needs no GPU.
"""
import argparse
import sys
import time

import numpy as np

from ._common import Launcher, is_int, is_real, ptr

NORM_MIN_BOX, FILTER_MIN_BOX, MAX_BOX = 4, 2, 1024
BATCH = 4096
KINDS = {"tanl": 1, "gauss": 2}


class PrepError(ValueError):
    """an argument outside the domains of N and F, or a stack that is not [n][nx][nx]"""


# ---- arguments

def _check_radius(nx, R):
    if not is_int(nx) or not NORM_MIN_BOX <= nx <= MAX_BOX:
        raise PrepError("normalize: the box must be in %d .. %d, got %r" % (NORM_MIN_BOX, MAX_BOX, nx))
    if not is_real(R) or not 1.0 <= R <= nx / 2.0:
        raise PrepError("normalize: bg_radius must be a finite number in 1 .. nx/2 = %g, got %r" % (nx / 2.0, R))
    return float(R)


def _check_flag(v, what):
    if not isinstance(v, (bool, np.bool_)):
        raise PrepError("%s is True or False, got %r" % (what, v))
    return bool(v)


def _check_term(spec, what):
    """(kind, a, b) of None | ("tanl", fl, aa) | ("gauss", s)"""
    if spec is None:
        return 0, 0.0, 0.0
    if not isinstance(spec, (tuple, list)) or not spec or spec[0] not in KINDS:
        raise PrepError('%s is None, ("tanl", fl, aa) or ("gauss", s), got %r' % (what, spec))
    if spec[0] == "tanl":
        if len(spec) != 3 or not is_real(spec[1]) or not is_real(spec[2]) or not 0.0 < spec[1] < 1.0 or not spec[2] > 0.0:
            raise PrepError('%s: ("tanl", fl, aa) needs finite 0 < fl < 1 and aa > 0, got %r' % (what, spec))
        return 1, float(spec[1]), float(spec[2])
    if len(spec) != 2 or not is_real(spec[1]) or not spec[1] > 0.0:
        raise PrepError('%s: ("gauss", s) needs a finite s > 0, got %r' % (what, spec))
    return 2, float(spec[1]), 0.0


def _check_filter(nx, lowpass, highpass):
    if not is_int(nx) or not FILTER_MIN_BOX <= nx <= MAX_BOX:
        raise PrepError("fourier_filter: the box must be in %d .. %d, got %r" % (FILTER_MIN_BOX, MAX_BOX, nx))
    lp, hp = _check_term(lowpass, "lowpass"), _check_term(highpass, "highpass")
    if not lp[0] and not hp[0]:
        raise PrepError("fourier_filter: give a lowpass, a highpass or both")
    return lp, hp


def _stack_numpy(images):
    if hasattr(images, "detach"):
        images = images.detach().cpu().numpy()
    x = np.array(images, np.float64)
    if x.ndim != 3 or x.shape[1] != x.shape[2]:
        raise PrepError("images are [n][nx][nx], got shape %s" % (x.shape,))
    return x


def _stack_device(images):
    """a contiguous float32 CUDA tensor [n][nx][nx] (worked on in place), or a numpy array copied to the current device"""
    import torch
    if isinstance(images, np.ndarray):
        if images.ndim != 3 or images.shape[1] != images.shape[2]:
            raise PrepError("images are [n][nx][nx], got shape %s" % (images.shape,))
        images = torch.from_numpy(np.ascontiguousarray(images, np.float32)).to(torch.device("cuda", torch.cuda.current_device()))
    if not (isinstance(images, torch.Tensor) and images.is_cuda and images.dtype == torch.float32 and images.is_contiguous()):
        raise PrepError("backend 'device' takes a contiguous float32 CUDA tensor [n][nx][nx] (or a numpy array, copied)")
    if images.dim() != 3 or images.shape[1] != images.shape[2]:
        raise PrepError("images are [n][nx][nx], got shape %s" % (tuple(images.shape),))
    return images


def _check_backend(backend):
    if backend not in ("device", "numpy"):
        raise PrepError("backend is 'device' or 'numpy', got %r" % (backend,))


# ---- N

def background(nx, R):
    """the boolean [nx][nx] background set B and the offsets u [nx][nx], v [nx][nx] (int64)"""
    R = _check_radius(nx, R)
    v, u = np.mgrid[0:nx, 0:nx].astype(np.int64) - nx // 2
    return (u * u + v * v).astype(np.float64) > R * R, u, v


def _normalize_numpy(x, R, ramp, invert, order=1):
    """the float64 statement; order = -1 sums the pixels of B the other way round (what the tests size their bars with)"""
    n, nx = x.shape[0], x.shape[-1]
    B, u, v = background(nx, R)
    ub, vb = u[B][::order], v[B][::order]
    nb = ub.size
    A = np.stack([np.ones_like(ub), ub, vb])                        # exact integers
    Ginv = np.linalg.inv((A @ A.T).astype(np.float64))
    uf, vf = u.astype(np.float64), v.astype(np.float64)
    s = -1.0 if invert else 1.0
    y, st = np.empty_like(x), np.zeros((n, 5))
    for i in range(n):
        if not np.all(np.isfinite(x[i])):
            y[i], st[i] = np.nan, np.nan
            continue
        xb = x[i][B][::order]
        theta = Ginv @ np.array([np.sum(xb), np.sum(xb * ub), np.sum(xb * vb)]) if ramp else np.zeros(3)
        e = x[i] - (theta[0] + theta[1] * uf + theta[2] * vf)
        eb = e[B][::order]
        mu = np.sum(eb) / nb
        sigma = np.sqrt(np.sum((eb - mu) ** 2) / nb)
        y[i] = s * (e - mu) if sigma == 0.0 else s * (e - mu) / sigma
        st[i] = theta[0], theta[1], theta[2], mu, sigma
    return y, st


def normalize(images, bg_radius, ramp=False, invert=False, stats=False, backend="device"):
    """N of the module's contract on images [n][nx][nx].  device: in place on a float32 CUDA tensor, returns it (a numpy array is
    copied to the current device and the new tensor returned); numpy: returns a new float64 array.  stats=True returns
    (images, statistics [n][5] double: a, b, c, mu, sigma) -- a CUDA tensor on the device backend."""
    _check_backend(backend)
    ramp, invert, stats = _check_flag(ramp, "ramp"), _check_flag(invert, "invert"), _check_flag(stats, "stats")
    if backend == "numpy":
        x = _stack_numpy(images)
        y, st = _normalize_numpy(x, _check_radius(x.shape[-1], bg_radius), ramp, invert)
        return (y, st) if stats else y
    t = _stack_device(images)
    n, nx = int(t.shape[0]), int(t.shape[-1])
    R = _check_radius(nx, bg_radius)
    L = Launcher(t)
    st = L.torch.empty((n, 5), dtype=L.torch.float64, device=t.device) if stats else None
    with L.torch.cuda.device(t.device):
        L.call("ra_prep_normalize", ptr(t), n, nx, R, int(ramp), int(invert), ptr(st))
    return (t, st) if stats else t


# ---- F

def filter_multiplier(nx, P, lowpass=None, highpass=None):
    """g [P][P/2 + 1] in float64 over (iy in fftfreq order, ix): what multiplies rfft2 of the P x P image; P is nx or 2 nx"""
    lp, hp = _check_filter(nx, lowpass, highpass)
    if not is_int(P) or P not in (nx, 2 * nx):
        raise PrepError("filter_multiplier: P is nx or 2 nx, got %r for nx = %d" % (P, nx))
    iy = np.fft.fftfreq(P, 1.0 / P).round().astype(np.int64)[:, None]
    ix = np.arange(P // 2 + 1, dtype=np.int64)[None, :]
    d = np.sqrt((ix * ix + iy * iy).astype(np.float64)) / P

    def term(kind, a, b):
        if kind == 1:
            k = np.pi / (2.0 * b * a)
            return 0.5 * (np.tanh(k * (d + a)) - np.tanh(k * (d - a)))
        return np.exp(-d * d / (2.0 * a * a))

    g = term(*lp) if lp[0] else np.ones_like(d)
    return g * (1.0 - term(*hp)) if hp[0] else g


def _filter_numpy(x, lowpass, highpass, pad):
    nx = x.shape[-1]
    P = 2 * nx if pad else nx
    o = (P - nx) // 2
    g = filter_multiplier(nx, P, lowpass, highpass).astype(np.float32).astype(np.float64)     # rounded once, as on the device
    big = np.zeros((x.shape[0], P, P))
    big[:, o:o + nx, o:o + nx] = x
    return np.fft.irfft2(np.fft.rfft2(big) * g, s=(P, P))[:, o:o + nx, o:o + nx]


def fourier_filter(images, lowpass=None, highpass=None, pad=False, backend="device"):
    """F of the module's contract on images [n][nx][nx]; lowpass / highpass: None, ("tanl", fl, aa) or ("gauss", s).  device: in
    place on a float32 CUDA tensor, returns it (a numpy array is copied to the current device and the new tensor returned);
    numpy: returns a new float64 array."""
    _check_backend(backend)
    pad = _check_flag(pad, "pad")
    if backend == "numpy":
        x = _stack_numpy(images)
        _check_filter(x.shape[-1], lowpass, highpass)
        return _filter_numpy(x, lowpass, highpass, pad)
    t = _stack_device(images)
    n, nx = int(t.shape[0]), int(t.shape[-1])
    lp, hp = _check_filter(nx, lowpass, highpass)
    L = Launcher(t)
    with L.torch.cuda.device(t.device):
        L.call("ra_prep_filter", ptr(t), n, nx, int(pad), lp[0], lp[1], lp[2], hp[0], hp[1], hp[2])
    return t


# ---- the tool

def _tool_terms(ap, args):
    """(lowpass, highpass) of the command line; --res converts FL and S from Angstrom as apix / value"""
    def conv(v, what):
        if not args.res:
            return v
        if not is_real(v) or not v > 0.0:
            ap.error("%s: with --res the value is a resolution in Angstrom > 0, got %r" % (what, v))
        return args.apix / v

    out = []
    for side in ("lowpass", "highpass"):
        tanl, gauss = getattr(args, side + "_tanl"), getattr(args, side + "_gauss")
        if tanl is not None and gauss is not None:
            ap.error("--%s_tanl and --%s_gauss exclude each other" % (side, side))
        spec = None
        if tanl is not None:
            spec = ("tanl", conv(tanl[0], "--%s_tanl" % side), tanl[1])
        elif gauss is not None:
            spec = ("gauss", conv(gauss, "--%s_gauss" % side))
        try:
            _check_term(spec, "--" + side)
        except PrepError as e:
            ap.error(str(e))
        out.append(spec)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.prep")
    ap.add_argument("input", help="stack (.hdf, .mrcs or .npy)")
    ap.add_argument("output", help="prepared stack (.hdf, .mrcs or .npy)")
    ap.add_argument("--norm_bg", type=float, default=None, metavar="R", help="normalise the background outside radius R to mean 0, sigma 1")
    ap.add_argument("--ramp", action="store_true", help="with --norm_bg: subtract the least-squares plane of the background first")
    ap.add_argument("--invert", action="store_true", help="invert the contrast")
    ap.add_argument("--ctf", default=None, metavar="TABLE", help="phase-flip ([N][9] .npy or RELION .star)")
    ap.add_argument("--apix", type=float, default=None, help="pixel size (A): for --res, and where the .star file gives none")
    ap.add_argument("--nopad", action="store_true", help="flip at the box size instead of in a 2x zero-padded image")
    ap.add_argument("--lowpass_tanl", type=float, nargs=2, default=None, metavar=("FL", "AA"))
    ap.add_argument("--lowpass_gauss", type=float, default=None, metavar="S")
    ap.add_argument("--highpass_tanl", type=float, nargs=2, default=None, metavar=("FL", "AA"))
    ap.add_argument("--highpass_gauss", type=float, default=None, metavar="S")
    ap.add_argument("--filter_pad", action="store_true", help="filter in a 2x zero-padded image instead of periodically")
    ap.add_argument("--res", action="store_true", help="FL and S are resolutions in Angstrom (needs --apix): frequency = apix / value")
    ap.add_argument("--box", type=int, default=None, metavar="M", help="Fourier-resize to box M last (1 .. 1024)")
    ap.add_argument("--stats", default=None, metavar="STATS.npy", help="write the [N][5] statistics (a, b, c, mu, sigma) of --norm_bg")
    ap.add_argument("--batch", type=int, default=BATCH, help="images read and prepared at a time (default %d)" % BATCH)
    ap.add_argument("--backend", default="device", choices=("device", "numpy"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    from . import ctf, resize, stackio
    # everything that can be refused is refused here, with exit status 2, before the device is touched
    if args.res and args.apix is None:
        ap.error("--res needs --apix")
    lowpass, highpass = _tool_terms(ap, args)
    filtering = lowpass is not None or highpass is not None
    if args.norm_bg is None and not args.invert and not args.ctf and not filtering and args.box is None:
        ap.error("no step requested: give --norm_bg, --invert, --ctf, a filter or --box")
    if args.ramp and args.norm_bg is None:
        ap.error("--ramp needs --norm_bg")
    if args.stats and args.norm_bg is None:
        ap.error("--stats needs --norm_bg")
    if args.filter_pad and not filtering:
        ap.error("--filter_pad needs a filter")
    if args.ctf and args.backend == "numpy":
        ap.error("--ctf flips on the GPU: it needs --backend device")
    if args.nopad and not args.ctf:
        ap.error("--nopad goes with --ctf")
    if args.apix is not None and not (args.ctf or args.res):
        ap.error("--apix goes with --ctf or --res")
    if args.batch < 1:
        ap.error("--batch must be >= 1, got %d" % args.batch)
    try:
        m = resize.check_box(args.box, "--box") if args.box is not None else None
        n = stackio.stack_size(args.input)
        if n < 1:
            raise PrepError("%s holds no images" % args.input)
        first = stackio.read_stack(args.input, 0, min(n, args.batch))
        ny, nx = first.shape[-2:]
        if ny != nx:
            raise PrepError("%s: images of %d x %d: preprocessing needs square images" % (args.input, ny, nx))
        if args.norm_bg is not None:
            _check_radius(nx, args.norm_bg)
        if filtering:
            _check_filter(nx, lowpass, highpass)
        resize.check_box(nx, "the input box")
        tab = ctf.load_table(args.ctf, n, nx, args.apix) if args.ctf else None
    except (PrepError, resize.ResizeError, ctf.CtfTableError, OSError, ValueError) as e:
        ap.error(str(e))
    numpy_backend = args.backend == "numpy"
    if not numpy_backend:
        import torch
        from . import api
        if not torch.cuda.is_available():
            raise SystemExit("no GPU visible: use --backend numpy for the CPU checker")
        dev = torch.device("cuda", args.device)
    mo = nx if m is None else m
    t0 = time.time()
    out = np.empty((n, mo, mo), np.float32)
    st = np.empty((n, 5)) if args.stats else None

    def steps(x, lo, hi):
        """the fixed order: normalise, phase flip, filter, resize"""
        if args.norm_bg is not None:
            r = normalize(x, args.norm_bg, ramp=args.ramp, invert=args.invert, stats=st is not None, backend=args.backend)
            if st is not None:
                x, s = r
                st[lo:hi] = s if numpy_backend else s.cpu().numpy()
            else:
                x = r
        elif args.invert:
            x = -x
        if tab is not None:
            x = api.phase_flip(x, tab[lo:hi], pad=not args.nopad)
        if filtering:
            x = fourier_filter(x, lowpass, highpass, pad=args.filter_pad, backend=args.backend)
        if m is not None:
            x = resize.resize(x, m, backend="numpy") if numpy_backend else api.fourier_resize(x, m)
        return x

    for lo in range(0, n, args.batch):
        hi = min(n, lo + args.batch)
        x = first if lo == 0 else stackio.read_stack(args.input, lo, hi)
        first = None
        if x.shape != (hi - lo, nx, nx):
            raise SystemExit("error: %s: images %d..%d are %s, not %d x %d" % (args.input, lo, hi, x.shape[1:], nx, nx))
        if numpy_backend:
            out[lo:hi] = steps(np.asarray(x, np.float64), lo, hi)
            continue
        with torch.cuda.device(dev):
            out[lo:hi] = steps(torch.from_numpy(np.array(x, np.float32)).to(dev), lo, hi).cpu().numpy()
    stackio.write_stack(args.output, out)
    if st is not None:
        np.save(args.stats, st)
    print("wrote %s (%d x %d x %d) in %.2f s" % (args.output, n, mo, mo, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
