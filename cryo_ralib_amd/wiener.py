"""CTF-corrected (Wiener-filtered) class averages of an aligned particle stack.

    python -m cryo_ralib_amd.wiener STACK PARAMS CTF OUT [--labels labels.npy] [--k K] [--snr S] [--nopad] [--flipped]
                                    [--min_count M] [--apix A] [--ou R] [--device D]

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

PARAMS is a driver's params.txt (idx angle sx sy mirror class; the class column gives the labels) or an initial2Dparams.txt
(alpha sx sy mirror; one class); --labels (an int .npy) overrides the classes, e.g. with k-means labels.  CTF is a [n][9] .npy
or a RELION .star (ctf.load_table, --apix where the .star gives no pixel size).  --ou R subtracts the mean under
model_circle(R) from every particle first.  OUT is .hdf, .mrcs or .npy.
"""
import argparse
import sys

import numpy as np

from . import ctf as _ctf

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


def wiener_reference(x, params, labels, k, table, snr=1.0, pad=True, flipped=False, min_count=1, aligned=None):
    """float64 statement of the contract: [k][nx][nx] averages and the class sizes.  aligned: the rot_shift2D images [n][nx][nx]
    to use in step 1 (e.g. the device's own, to isolate the rest); default synth.rot_shift2d_np of x"""
    from . import synth
    x = np.asarray(x)
    if x.ndim != 3 or x.shape[1] != x.shape[2]:
        raise WienerError("images are [n][nx][nx], got %s" % (x.shape,))
    n, nx = x.shape[0], x.shape[-1]
    prm, lab, tab = check_inputs(n, nx, params, labels, k, table, snr)
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
    out = np.zeros((k, nx, nx))
    for j in range(k):
        if counts[j] >= min_count and counts[j] > 0:
            out[j] = np.fft.irfft2(num[j] / (den[j] + 1.0 / snr), s=(P, P))[o:o + nx, o:o + nx]
    return out, counts


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
    import ctypes
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
    stream = torch.cuda.current_stream(images.device)
    with torch.cuda.device(images.device):
        api._check(api.load_library().ra_wiener_accumulate(
            ctypes.c_void_p(images.data_ptr()), n, nx, ctypes.c_void_p(d_rec.data_ptr()), tab.ctypes.data_as(api.float_ptr),
            int(bool(pad)), int(bool(flipped)), int(k), ctypes.c_void_p(num.data_ptr()), ctypes.c_void_p(den.data_ptr()),
            ctypes.c_void_p(counts.data_ptr()), ctypes.c_void_p(stream.cuda_stream)), "ra_wiener_accumulate")


def finalize(num, den, counts, nx, pad=True, snr=1.0, min_count=1, out=None):
    """ra_wiener_finalize on the current stream: [k][nx][nx] float32 CUDA tensor of the averages"""
    import ctypes
    import torch
    from . import api
    k = int(counts.shape[0])
    if out is None:
        out = torch.empty((k, nx, nx), dtype=torch.float32, device=num.device)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (k, nx, nx)
    stream = torch.cuda.current_stream(num.device)
    with torch.cuda.device(num.device):
        api._check(api.load_library().ra_wiener_finalize(
            ctypes.c_void_p(num.data_ptr()), ctypes.c_void_p(den.data_ptr()), ctypes.c_void_p(counts.data_ptr()), k, int(nx),
            int(bool(pad)), float(snr), int(min_count), ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream.cuda_stream)),
            "ra_wiener_finalize")
    return out


def wiener_averages(images, params, labels, k, ctf, snr=1.0, pad=True, flipped=False, min_count=1, ou=None, preprocess=False,
                    device=0):
    """[k][nx][nx] float32 CTF-corrected averages (numpy) and the class sizes [k] of the stack on the device (the contract of
    wiener_reference).  preprocess=True subtracts the mean under model_circle(ou) first (Engine.normalize_particles, as
    kmeans.class_averages does; ou defaults to nx // 2 - 2)."""
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
        num, den, counts = new_sums(k, nx, pad, dev)
        accumulate(x, prm, lab, k, tab, num, den, counts, pad, flipped)
        out = finalize(num, den, counts, nx, pad, snr, min_count)
        return out.cpu().numpy(), counts.cpu().numpy()


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
    args = ap.parse_args(argv)
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
    except (WienerError, _ctf.CtfTableError, OSError, ValueError) as e:
        raise SystemExit("error: %s" % e)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: the averages run on the device (wiener_reference is the float64 checker)")
    avg, counts = wiener_averages(stack, prm, lab, k, tab, args.snr, not args.nopad, args.flipped, args.min_count, ou=args.ou,
                                  preprocess=args.ou is not None, device=args.device)
    stackio.write_stack(args.output, avg)
    print("%s: %d CTF-corrected averages of %d particles (%d x %d, snr %g%s), class sizes %s"
          % (args.output, k, n, nx, nx, args.snr, ", flipped" if args.flipped else "", " ".join(str(int(c)) for c in counts)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
