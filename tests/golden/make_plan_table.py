"""Records tests/golden/plan_table.json for tests/test_gpu_plan_table.py: the plan (kernel family, search geometry, LDS ledger) of
every engine of that test's table.  The point of the fixture is to hold a CHANGED planner to the plans of the one before it, so it
is recorded from a build of the commit before the change, never from the code under test.  Needs an MI355X:

    RALIGN_LIB=/path/to/the/earlier/libralign_hip.so python tests/golden/make_plan_table.py [OUT.json]
"""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from cryo_ralib_amd import api          # noqa: E402
import test_gpu_plan_table as t         # noqa: E402


def main():
    if not os.environ.get("RALIGN_LIB"):
        sys.exit("set RALIGN_LIB to a build of the commit BEFORE the change under test")
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "plan_table.json")
    t0 = time.time()
    table = t.build_table(os.environ.__setitem__, lambda n: os.environ.pop(n, None))
    with open(out, "w") as f:
        json.dump(table, f, indent=0, sort_keys=False)
        f.write("\n")
    failed = sum("rc" in r for r in table.values())
    print("%d rows (%d failed creates) in %.1f s from %s -> %s" % (len(table), failed, time.time() - t0, api.LIB_PATH, out))


if __name__ == "__main__":
    main()
