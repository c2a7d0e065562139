"""Phase-flip a particle stack with a CTF table (SPHIRE's `sp_process.py --phase_flip` step, without EMAN2):

    python -m cryo_ralib_amd.phaseflip IN OUT --ctf TABLE [--apix A] [--nopad]

IN / OUT: any stack format stackio reads / writes (.hdf, .mrcs, .npy); TABLE: [N][9] .npy or RELION .star
(cryo_ralib_amd.ctf).  The flip runs on the GPU (api.phase_flip), in batches that bound the device memory.
"""
import argparse
import sys

import numpy as np

BATCH = 65536


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m cryo_ralib_amd.phaseflip")
    p.add_argument("input"); p.add_argument("output")
    p.add_argument("--ctf", required=True, metavar="TABLE", help="[N][9] .npy or RELION .star CTF table")
    p.add_argument("--apix", type=float, default=None, help="pixel size (A) where the .star file gives none")
    p.add_argument("--nopad", action="store_true", help="flip at the box size instead of in a 2x zero-padded image")
    p.add_argument("--device", type=int, default=0)
    args = p.parse_args(argv)
    import torch
    from . import api, ctf, stackio
    if not torch.cuda.is_available():
        raise SystemExit("no GPU visible: the phase flip has no CPU path")
    data = stackio.read_stack(args.input)
    n, nx = data.shape[0], data.shape[-1]
    if data.shape[1] != nx:
        raise SystemExit("%s: images of %d x %d: the flip needs square images" % (args.input, data.shape[1], nx))
    try:
        tab = ctf.load_table(args.ctf, n, nx, args.apix)
    except (ctf.CtfTableError, OSError) as e:
        raise SystemExit("--ctf: %s" % e)
    dev = torch.device("cuda", args.device)
    out = np.empty_like(data, dtype=np.float32)
    for lo in range(0, n, BATCH):
        hi = min(n, lo + BATCH)
        t = torch.from_numpy(np.array(data[lo:hi], np.float32)).to(dev)
        api.phase_flip(t, tab[lo:hi], pad=not args.nopad)
        out[lo:hi] = t.cpu().numpy()
    stackio.write_stack(args.output, out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
