"""Records tests/golden/plan_bytes.npz for tests/test_plan_cpu.py: ra_legacy_bytes of every configuration of that test's grid under
each of its environment settings.  The point of the fixture is to hold a CHANGED planner to the answers of the one before it, so it
is recorded from a build of the commit before the change, never from the code under test:

    RALIGN_LIB=/path/to/the/earlier/libralign_hip.so python tests/golden/make_plan_bytes.py

No GPU is needed.  `configs` is the grid ([n][5]: box, outer radius, references, range, step); every other array is named after
its setting ("default", "RALIGN_FUSED=0", ..) and holds the byte counts in grid order (uint64)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from cryo_ralib_amd import api          # noqa: E402
import test_plan_cpu as t               # noqa: E402


def main():
    if not os.environ.get("RALIGN_LIB"):
        sys.exit("set RALIGN_LIB to a build of the commit BEFORE the change under test")
    lib = api.load_library()
    for name in t.SWITCHES:
        os.environ.pop(name, None)
    cfgs = t.grid()
    out = {"configs": cfgs}
    for setting in t.SETTINGS:
        if setting:
            os.environ[setting[0]] = setting[1]
        out[t.key_of(setting)] = t.plan_bytes(lib, cfgs)
        if setting:
            del os.environ[setting[0]]
        assert not (out[t.key_of(setting)] == np.uint64(2 ** 64 - 1)).any()
    np.savez_compressed(os.path.join(HERE, "plan_bytes.npz"), **out)
    print("%d configurations x %d settings from %s" % (len(cfgs), len(t.SETTINGS), api.LIB_PATH))


if __name__ == "__main__":
    main()
