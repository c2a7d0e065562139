"""Every way into the CCF tail of a search pass -- the store of the contracted spectra and ifft_argmax (ralign_kernels.h) -- on the
smallest geometry that reaches it (tests/ccf_tail_cases.py): against the oracle (identical ref_id, mirror, angle_bin and shift
state, peaks to 1e-5 relative: tests/test_ccf_tail_cpu.py shows that no particle of these cases is a nearer tie than that), against
the records of the library before the CCF-tail diet, byte for byte (tests/golden/ccf_tail_records.npz, written by
tests/golden/make_ccf_tail_records.py), and against itself run twice.  One search per case, shared by the tests."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccf_tail_cases as cc

pytestmark = pytest.mark.gpu

PEAK_RTOL = 1e-5        # the bar of the polar-stage checks
ALPHA_ATOL = 2e-3       # degrees: bench.py's bar on the sub-bin angle
SWITCHES = ("RALIGN_FUSED", "RALIGN_TILED", "RALIGN_GENERIC", "RALIGN_PAIR", "RALIGN_SOLO", "RALIGN_DUO", "RALIGN_PACK")

_RUNS = {}


def engine_run(name):
    if name not in _RUNS:
        _RUNS[name] = cc.run_engine(name)
    return _RUNS[name]


def default_path_only():
    on = [sw for sw in SWITCHES if os.environ.get(sw) is not None]
    if on:
        pytest.skip("asserts the default kernel path; %s is set" % ", ".join(on))


def assert_matches_oracle(name, alpha=False):
    rec, state, family = engine_run(name)
    params, jtot, d = cc.oracle(name)
    rel = np.abs(rec["peak"] - params[:, 5]) / np.abs(params[:, 5])
    print("%s: family %s, largest relative peak difference %.3g" % (name, family, rel.max()))
    np.testing.assert_array_equal(rec["ref_id"], params[:, 4].astype(int))
    np.testing.assert_array_equal(rec["mirror"], params[:, 3].astype(int))
    np.testing.assert_array_equal(rec["angle_bin"], jtot)
    np.testing.assert_array_equal(state, d)
    assert rel.max() < PEAK_RTOL, rel.max()
    if alpha:
        da = np.abs(((rec["alpha"] - params[:, 0]) + 180.0) % 360.0 - 180.0)
        print("%s: largest sub-bin angle difference %.3g degrees" % (name, da.max()))
        assert da.max() <= ALPHA_ATOL, da


@pytest.mark.parametrize("name", list(cc.CASES))
def test_path_against_oracle(name):
    default_path_only()
    assert engine_run(name)[2] == cc.CASES[name][8], "kernel family %s, expected %s" % (engine_run(name)[2], cc.CASES[name][8])
    assert_matches_oracle(name)


def test_nomirror_is_straight_only():
    default_path_only()
    assert (engine_run(cc.NOMIRROR)[0]["mirror"] == 0).all()
    assert_matches_oracle(cc.NOMIRROR)


def test_neighbourhood_wraps_at_both_ends_of_the_angle_range():
    """winners at bins 1, 2, 3 and N - 2, N - 1, N: the 7-point neighbourhood of the sub-bin fit comes from both ends of the sequence"""
    default_path_only()
    assert tuple(engine_run(cc.PLANTED)[0]["angle_bin"]) == cc.PLANTED_BINS
    assert_matches_oracle(cc.PLANTED, alpha=True)


def test_constant_image_takes_the_straight_sequence_and_the_last_bin():
    """both sequences constant and equal: straight wins on bq >= bt, and the LAST element equal to the maximum is the winner"""
    default_path_only()
    rec, state, family = engine_run(cc.CONSTANT)
    params, jtot, d = cc.oracle(cc.CONSTANT)
    np.testing.assert_array_equal(rec["mirror"], params[:, 3].astype(int))
    np.testing.assert_array_equal(rec["angle_bin"], jtot)
    assert (rec["mirror"] == 0).all() and (rec["angle_bin"] == cc.MAXRIN_OU36).all()


@pytest.mark.parametrize("name", cc.ALL)
def test_records_are_those_of_the_library_before_the_diet(golden_dir, name):
    default_path_only()
    g = np.load(os.path.join(golden_dir, "ccf_tail_records.npz"))
    rec, state, family = engine_run(name)
    assert tuple(g[name + "/family"]) == family
    assert rec.view(np.uint8).tobytes() == g[name + "/records"].tobytes()
    assert state.view(np.uint8).tobytes() == g[name + "/state"].tobytes()


@pytest.mark.parametrize("name", ["fused-90-R10", "tiled-90-R17", "pair-100-R3", "kernelpair-90-R3", cc.CONSTANT])
def test_same_input_twice_gives_the_same_bytes(name):
    rec, state, _ = engine_run(name)
    rec2, state2, _ = cc.run_engine(name)
    assert rec.tobytes() == rec2.tobytes() and state.tobytes() == state2.tobytes()
