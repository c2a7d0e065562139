"""The inputs of tests/test_gpu_ccf_tail.py, checked without a GPU: every oracle-comparison case is free of near-ties (so the GPU
test leaves no particle out), the fused kernel's two-round threshold is where the case list puts it, and the oracle's own answers
to the tie and edge cases of the argmax are the ones the GPU test asks of the engine."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ccf_tail_cases as cc
from oracle import oracle as orc

GAP = 1e-5      # the peak bar of the GPU test: a winner this far ahead of the runner-up is the winner in f32 too


@pytest.mark.parametrize("name", list(cc.CASES) + [cc.NOMIRROR])
def test_no_particle_is_a_near_tie(name):
    """best and second-best CCF value over (reference, offset, mirror, angle bin) differ by more than 1e-5 relative for every
    particle, and the best one is the peak the oracle's search reports"""
    n = cc.geometry_of(name)[5]
    params = cc.oracle(name)[0]
    gaps = []
    for i in range(n):
        gap, best = cc.peak_gap(name, i, straight_only=(name == cc.NOMIRROR))
        assert abs(best - params[i, 5]) <= 1e-6 * abs(params[i, 5]), (i, best, params[i, 5])
        gaps.append(gap)
    print("%s: smallest gap %.3g" % (name, min(gaps)))
    assert min(gaps) > GAP, (int(np.argmin(gaps)), min(gaps))


def test_two_round_threshold_of_the_fused_plan():
    """12 references are the fewest for which a pass of search_fused_kernel at ou 36 stores its spectra in two rounds (11 spectra
    of 546 floats fit the 6432 floats of a ring buffer); the tiled kernel takes over at 15"""
    assert cc.TWO_ROUND_NREF == 12 and cc.fused_rounds(11) == 1 and cc.fused_rounds(14) == 2
    assert cc.CASES["fused-90-2rounds"][2] == 12


def test_constant_image_answer_of_the_oracle():
    """only DC in every ring: both sequences are constant and equal -- straight wins the tie, and the scan's '>=' keeps the last bin"""
    params, jtot, d = cc.oracle(cc.CONSTANT)
    assert (params[:, 3] == 0).all() and (jtot == cc.MAXRIN_OU36).all()
    assert (params[:, 5] == params[0, 5]).all()


def test_nomirror_answer_of_the_oracle():
    params, jtot, d = cc.oracle(cc.NOMIRROR)
    assert (params[:, 3] == 0).all()
    # the same particles with the mirror search on: some are found mirrored, so the switch is what keeps them straight
    rg, cref = cc._cref(cc.NOMIRROR)
    _, parts = cc.inputs(cc.NOMIRROR)
    n = len(parts)
    p2, _, _, _ = orc.reffree_iteration(parts, cref[0], rg, 3, 3, 1.0, (0, 0), np.zeros((n, 2), np.float32), np.zeros((n, 6), np.float32), nthreads=8)
    assert (p2[:, 3] == 1).any()


def test_planted_winners_sit_at_both_ends_of_the_angle_range():
    params, jtot, d = cc.oracle(cc.PLANTED)
    assert tuple(jtot) == cc.PLANTED_BINS and (params[:, 3] == 0).all()
