"""Golden 2SDR / MPCA values from the reference tree's own functions (utils_ralib.MPCA and utils_ralib.TwoSDR).  Run where the
reference tree is mounted:

    python tests/golden/make_sdr_pins.py

Both functions are read out of src/utils_ralib.py with `ast` and executed with np, numpy.linalg as LA and scipy.sparse.linalg's
eigs / svds; only numbers are written.  sdr_ref.npz holds, per case k: `arr_k` (the float32 input [n][p][q]), `p0_k`, `q0_k`,
`r_k`, the TwoSDR outputs `factors_k`, `G_k`, `A_k`, `B_k`, `mean_k` and the MPCA outputs `mfactors_k`, `mA_k`, `mB_k`, `mmean_k`.
ARPACK starts from a random vector, so signs (and, where the problem is degenerate, the vectors themselves) are the reference's
choice: tests compare projectors and sign-aligned columns, and on the noise-dominated case only the captured energy.
"""
import ast
import os
import sys

import numpy as np
import numpy.linalg as LA
from scipy.sparse.linalg import eigs, svds

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def load_reference():
    src = open(os.path.join(REF, "src", "utils_ralib.py")).read()
    fns = [n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name in ("MPCA", "TwoSDR")]
    assert len(fns) == 2, "MPCA / TwoSDR not found"
    ns = {"np": np, "LA": LA, "eigs": eigs, "svds": svds}
    exec(compile(ast.Module(body=fns, type_ignores=[]), "utils_ralib.sdr", "exec"), ns)
    return ns["MPCA"], ns["TwoSDR"]


def low_rank(seed=11):
    """n = 160 images of 20 x 24 = U0 C_i V0^T + 1e-3 noise, rank 3 x 4, coefficient scales distinct: converges early"""
    rng = np.random.default_rng(seed)
    n, p, q = 160, 20, 24
    U0 = LA.qr(rng.standard_normal((p, 3)))[0]
    V0 = LA.qr(rng.standard_normal((q, 4)))[0]
    s, t = np.array([8.0, 3.0, 1.0]), np.array([5.0, 2.2, 1.3, 0.6])
    C = rng.standard_normal((n, 3, 4)) * s[:, None] * t[None, :]
    arr = np.einsum("pa,iab,qb->ipq", U0, C, V0) + 1e-3 * rng.standard_normal((n, p, q)) + 0.5
    return arr.astype(np.float32), 3, 4, 5


def noisy(seed=12):
    """n = 120 images of 16 x 16: 6 smooth classes under unit noise, p0 = 8, q0 = 6: runs all 30 iterations"""
    rng = np.random.default_rng(seed)
    n, p = 120, 16
    yy, xx = np.mgrid[0:p, 0:p] / p
    classes = np.stack([np.sin(2 * np.pi * (k + 1) * xx) * np.cos(np.pi * (k % 3 + 1) * yy) for k in range(6)])
    arr = 0.5 * classes[rng.integers(0, 6, n)] + rng.standard_normal((n, p, p))
    return arr.astype(np.float32), 8, 6, 10


def synth_stack():
    """n = 64 synth particles of 32 x 32 from 6 references, (p0, q0, r) = (6, 6, 10)"""
    from cryo_ralib_amd import synth
    refs = synth.make_references(6, 32, 14)
    parts, _ = synth.make_particles(refs, 64, 2, 2, 0.3, ou=14)
    return parts.astype(np.float32), 6, 6, 10


def main():
    MPCA, TwoSDR = load_reference()
    out = {}
    for k, make in enumerate((low_rank, noisy, synth_stack)):
        np.random.seed(100 + k)                     # ARPACK's start vector is its own; this only pins numpy's state
        arr, p0, q0, r = make()
        factors, G, A, B, mean = TwoSDR(arr, p0, q0, r)
        mf, mA, mB, mm = MPCA(arr, p0, q0)
        out.update({"arr_%d" % k: arr, "p0_%d" % k: np.int64(p0), "q0_%d" % k: np.int64(q0), "r_%d" % k: np.int64(r),
                    "factors_%d" % k: np.asarray(factors.real, np.float64), "G_%d" % k: np.asarray(G.real, np.float64),
                    "A_%d" % k: np.asarray(A, np.float64), "B_%d" % k: np.asarray(B, np.float64),
                    "mean_%d" % k: np.asarray(mean, np.float32), "mfactors_%d" % k: np.asarray(mf.real, np.float64),
                    "mA_%d" % k: np.asarray(mA, np.float64), "mB_%d" % k: np.asarray(mB, np.float64),
                    "mmean_%d" % k: np.asarray(mm, np.float32)})
    out["count"] = np.int64(3)
    np.savez_compressed(os.path.join(HERE, "sdr_ref.npz"), **out)
    print("wrote sdr_ref.npz: 3 cases, %d bytes" % os.path.getsize(os.path.join(HERE, "sdr_ref.npz")))


if __name__ == "__main__":
    main()
