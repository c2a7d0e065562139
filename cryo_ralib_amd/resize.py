"""Fourier resizing of square particle stacks: binning by Fourier cropping, upsampling by Fourier padding.

    python -m cryo_ralib_amd.resize IN OUT --box M [--ctf TABLE [--apix A] [--nopad]] [--batch B] [--backend device|numpy] [--device D]

The contract is this project's own statement: images x of box nx become images y of box m, both in
1 .. 1024 and either one the larger, through one real m x nx operator A applied to both axes, y = A x A^T, with

    A[j][i] = (1/nx) sum_{k in K} w_k cos(2 pi k (t_j - u_i)),  t_j = (j - m//2) / m,  u_i = (i - nx//2) / nx,
    s = min(nx, m),  K = {k : |k| <= s/2},  w_k = 1/2 when nx is even and |k| = nx/2, otherwise 1.

That is the trigonometric interpolant of x about its centre (n//2, as model_circle and rot_shift2D), the Nyquist term of an even
nx split half and half between +-nx/2, kept at |k| <= s/2 and sampled on the m grid about its centre.  m == nx is the identity;
up then down (nx -> M -> nx, M > nx) returns x; downsampling keeps the mean and a constant stays the same constant.  The output
pixel is apix nx / m.  No external implementation pins this; it agrees with fftshift(fft2(ifftshift(x))) cropped or zero padded,
the +-m/2 pair folded onto one index, ifft2, times m^2 / nx^2, with the weights w at the source's Nyquist.

backend="device" runs ra_fourier_resize (csrc/ralign_resize.h, f32 MFMA); backend="numpy" is the float64 checker.
"""
import argparse
import sys
import time

import numpy as np

MAX_BOX = 1024
BATCH = 4096


class ResizeError(ValueError):
    """a size outside 1 .. 1024, or a stack that is not [n][nx][nx]"""


def check_box(v, what="box"):
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not 1 <= v <= MAX_BOX:
        raise ResizeError("%s must be an integer in 1 .. %d, got %r" % (what, MAX_BOX, v))
    return int(v)


def operator(nx, m):
    """the float64 m x nx operator A (Dirichlet closed form, O(nx m))"""
    nx, m = check_box(nx, "nx"), check_box(m, "m")
    L = m * nx
    h = min(nx, m) // 2
    half = nx % 2 == 0 and nx <= m
    # p = (t_j - u_i) L exactly, as integers; theta / 2 = pi p / L
    p = ((np.arange(m, dtype=np.int64) - m // 2) * nx)[:, None] - ((np.arange(nx, dtype=np.int64) - nx // 2) * m)[None, :]

    def red(a):                                    # a mod 2L in [-L, L), over L
        r = np.mod(a + L, 2 * L) - L
        return r.astype(np.float64) / L

    zero = np.mod(p, L) == 0
    den = np.sin(np.pi * red(p))
    num = np.sin(np.pi * red((2 * h + 1) * p))
    d = np.where(zero, 2.0 * h + 1.0, num / np.where(zero, 1.0, den))
    if half:
        d -= np.where(zero, 1.0, np.cos(np.pi * red(2 * h * p)))
    return d / nx


def _resize_numpy(x, m):
    x = np.asarray(x)
    squeeze = x.ndim == 2
    x = x[None] if squeeze else x
    if x.ndim != 3 or x.shape[1] != x.shape[2]:
        raise ResizeError("images are [n][nx][nx], got shape %s" % (x.shape,))
    A = operator(x.shape[-1], m)
    y = np.einsum("ji,nik,lk->njl", A, x.astype(np.float64), A, optimize=True)
    return y[0] if squeeze else y


def resize(images, m, backend="device", out=None):
    """images [n][nx][nx] (or one [nx][nx] image) -> [n][m][m].  device: a float32 CUDA tensor (a numpy array is copied to the
    current device) through ra_fourier_resize, returns a tensor; numpy: the float64 checker, returns float64 numpy."""
    m = check_box(m, "m")
    if backend == "numpy":
        if hasattr(images, "detach"):
            images = images.detach().cpu().numpy()
        return _resize_numpy(images, m)
    if backend != "device":
        raise ResizeError("backend is 'device' or 'numpy', got %r" % (backend,))
    import torch
    from . import api
    if not isinstance(images, torch.Tensor):
        images = torch.from_numpy(np.ascontiguousarray(images, np.float32)).to("cuda")
    squeeze = images.dim() == 2
    t = images[None] if squeeze else images
    y = api.fourier_resize(t.contiguous(), m, out=out)
    return y[0] if squeeze else y


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.resize")
    ap.add_argument("input", help="stack (.hdf, .mrcs or .npy)")
    ap.add_argument("output", help="resized stack (.hdf, .mrcs or .npy)")
    ap.add_argument("--box", type=int, required=True, help="output box M (1 .. 1024)")
    ap.add_argument("--ctf", default=None, metavar="TABLE", help="phase-flip at the input box first ([N][9] .npy or RELION .star)")
    ap.add_argument("--apix", type=float, default=None, help="pixel size (A) where the .star file gives none")
    ap.add_argument("--nopad", action="store_true", help="flip at the box size instead of in a 2x zero-padded image")
    ap.add_argument("--batch", type=int, default=BATCH, help="images read and resized at a time (default %d)" % BATCH)
    ap.add_argument("--backend", default="device", choices=("device", "numpy"))
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    from . import ctf, stackio
    try:
        m = check_box(args.box, "--box")
        if args.batch < 1:
            raise ResizeError("--batch must be >= 1, got %d" % args.batch)
        if args.ctf and args.backend == "numpy":
            raise ResizeError("--ctf flips on the GPU: it needs --backend device")
        if (args.apix is not None or args.nopad) and not args.ctf:
            raise ResizeError("--apix and --nopad go with --ctf")
        n = stackio.stack_size(args.input)
        if n < 1:
            raise ResizeError("%s holds no images" % args.input)
        first = stackio.read_stack(args.input, 0, min(n, args.batch))
        ny, nx = first.shape[-2:]
        if ny != nx:
            raise ResizeError("%s: images of %d x %d: resizing needs square images" % (args.input, ny, nx))
        check_box(nx, "the input box")
        tab = ctf.load_table(args.ctf, n, nx, args.apix) if args.ctf else None
    except (ResizeError, ctf.CtfTableError, OSError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    if args.backend == "device":
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("no GPU visible: use --backend numpy for the CPU checker")
        dev = torch.device("cuda", args.device)
    print("%s: %d images, %d -> %d, scale %.6g (output pixel = input pixel x %.6g)" % (args.input, n, nx, m, m / nx, nx / m))
    t0 = time.time()
    out = np.empty((n, m, m), np.float32)
    for lo in range(0, n, args.batch):
        hi = min(n, lo + args.batch)
        x = first if lo == 0 else stackio.read_stack(args.input, lo, hi)
        first = None
        if x.shape != (hi - lo, nx, nx):
            raise SystemExit("error: %s: images %d..%d are %s, not %d x %d" % (args.input, lo, hi, x.shape[1:], nx, nx))
        if args.backend == "numpy":
            out[lo:hi] = resize(x, m, backend="numpy")
            continue
        from . import api
        with torch.cuda.device(dev):
            t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
            if tab is not None:
                api.phase_flip(t, tab[lo:hi], pad=not args.nopad)
            out[lo:hi] = api.fourier_resize(t, m).cpu().numpy()
    stackio.write_stack(args.output, out)
    print("wrote %s (%d x %d x %d) in %.2f s" % (args.output, n, m, m, time.time() - t0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
