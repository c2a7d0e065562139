"""Writes tests/golden/ccf_tail_records.npz: the result records (RESULT_DTYPE, as raw bytes) and shift states of every case of
tests/ccf_tail_cases.py, from one search each on an MI355X.

Run once with the library of the commit BEFORE the CCF-tail diet (RALIGN_LIB=<that build> python tests/golden/make_ccf_tail_records.py):
tests/test_gpu_ccf_tail.py holds every later build to these bytes."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import ccf_tail_cases as cc


def main(out=os.path.join(HERE, "ccf_tail_records.npz")):
    table = {}
    for name in cc.ALL:
        rec, state, family = cc.run_engine(name)
        table[name + "/records"] = rec.view(np.uint8).copy()
        table[name + "/state"] = state.view(np.uint8).reshape(-1).copy()
        table[name + "/family"] = np.array(family, np.int32)
        print(name, family, rec[:2])
    np.savez_compressed(out, **table)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main(*sys.argv[1:])
