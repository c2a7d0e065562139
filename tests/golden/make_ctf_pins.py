"""Golden CTF values from the reference tree's own formula (utils_ralib.compute_ctf_np).  Run where the reference tree is
mounted:

    python tests/golden/make_ctf_pins.py

The function is read out of src/utils_ralib.py with `ast` and executed at fixture time; only numbers are written.
ctf_ref.npz holds, per parameter set k: `params_k` (the [9] row: D, Apix, DefocusU, DefocusV, DefocusAngle, Voltage, Cs,
w, PhaseShift), `nx_k` (the box of the stack the row is applied to) and `ctf_k` [nx][nx], compute_ctf_np at the integer DFT
frequencies of that box in numpy.fft order: row = fftfreq(nx) * nx as y, column = fftfreq(nx) * nx as x, divided by
(nx * Apix * D / nx) = D * Apix.  x and y are assigned as in plot_ctf (meshgrid(x, y) reshaped to [y][x]); plot_ctf's own
linspace grid is not used, since it leaves the DFT grid for odd sizes.
"""
import ast
import os

import numpy as np

REF = "/root/reference"
HERE = os.path.dirname(os.path.abspath(__file__))

# (D, Apix, dfu, dfv, dfang, kV, Cs, w, phase), box nx
SETS = [
    ((32, 2.0, 15000.0, 15000.0, 0.0, 300.0, 2.7, 0.1, 0.0), 32),
    ((33, 1.5, 12000.0, 9000.0, 30.0, 300.0, 2.7, 0.07, 0.0), 33),
    ((48, 1.2, 25000.0, 21000.0, -62.5, 200.0, 2.0, 0.1, 0.0), 48),
    ((45, 2.5, 8000.0, 7000.0, 117.0, 300.0, 2.7, 0.0, 0.0), 45),
    ((40, 1.1, 6000.0, 5200.0, 15.0, 300.0, 2.7, 0.1, 90.0), 40),
    ((64, 1.0, 20000.0, 18500.0, 75.0, 300.0, 2.7, 0.1, 0.0), 32),        # binned stack: D = 2 nx
    ((37, 3.0, 30000.0, 28000.0, 170.0, 120.0, 1.4, 0.15, 35.0), 37),
    ((90, 3.7, 18000.0, 16000.0, -10.0, 300.0, 2.7, 0.1, 0.0), 90),
]


def load_compute_ctf_np():
    src = open(os.path.join(REF, "src", "utils_ralib.py")).read()
    tree = ast.parse(src)
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_ctf_np"]
    assert len(fn) == 1, "compute_ctf_np not found"
    mod = ast.Module(body=fn, type_ignores=[])
    ns = {"np": np}
    exec(compile(mod, "utils_ralib.compute_ctf_np", "exec"), ns)
    return ns["compute_ctf_np"]


def main():
    f = load_compute_ctf_np()
    out = {}
    for k, (row, nx) in enumerate(SETS):
        D, apix = row[0], row[1]
        fr = np.fft.fftfreq(nx) * nx / (D * apix)
        freqs = np.stack(np.meshgrid(fr, fr), -1).reshape(-1, 2)        # [y][x], x = column 0, as plot_ctf
        c = f(freqs, *row[2:]).reshape(nx, nx)
        out["params_%d" % k] = np.array(row, np.float64)
        out["nx_%d" % k] = np.int64(nx)
        out["ctf_%d" % k] = c.astype(np.float64)
    out["count"] = np.int64(len(SETS))
    np.savez_compressed(os.path.join(HERE, "ctf_ref.npz"), **out)
    print("wrote ctf_ref.npz: %d parameter sets" % len(SETS))


if __name__ == "__main__":
    main()
