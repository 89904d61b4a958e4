"""The optical-flow oracle (oracle/oracle_flow.cpp, a restatement of cv::calcOpticalFlowPyrLK) against pyramidal Lucas-Kanade
in float64 written from the method's definition (tests/lk_reference.py), on the reference's own stereo pair. The two share no
code and no number format, so an error in the oracle's reading of the algorithm -- window centre, level hand-over, bilinear
weights, derivative kernel, stopping rule -- shows here (DESIGN.md section 2 lists the mutations that were tried).

Two assertions per input, over the points both sides track:
  * the median distance is at most 4x the value measured when the test was written (the rule of the gauge tests);
  * at most 5 % of the points lie further than 0.02 px from the float64 result. The few that do converge to another local
    minimum; the cap is a condition, not a measurement.
The measured values are lk_reference.CASES."""
import numpy as np
import pytest

import oracle

import lk_reference
import stereo_fixture as sf

CASES = lk_reference.CASES


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_lk_against_float64_definition(name):
    a, b, pts = lk_reference.inputs(name, oracle)
    nxt, st, _, top = oracle.optical_flow_pyr_lk(a, b, pts)
    assert top == 3
    lk_reference.check(name, a, b, pts, nxt, st)


def test_reference_pyramid_sizes_and_identity():
    """The float64 reference itself: the crop's levels are 167x106, 84x53, 42x27; a constant stays constant; a pair of equal
    images gives zero flow; a whole-pixel shift is found to 1e-3 px."""
    L, _ = sf.pair()
    c = sf.crop(L)
    assert [l.shape[::-1] for l in lk_reference.pyramid(c)] == [(333, 211), (167, 106), (84, 53), (42, 27)]
    assert len(lk_reference.pyramid(np.zeros((64, 96)))) == 2      # 24x16 is not larger than the window
    assert np.allclose(lk_reference.pyr_down(np.full((37, 51), 93.0)), 93.0)
    pts = sf.inner_keys(oracle, c, 60)
    out, ok = lk_reference.track(c, c, pts)
    assert ok.all() and np.abs(out - pts).max() < 1e-9
    out, ok = lk_reference.track(L[40:251, 300:633], L[37:248, 295:628], pts)   # content moves by (+5, +3)
    assert ok.mean() > 0.9 and np.median(np.abs(out[ok] - pts[ok] - [5, 3]).max(1)) < 1e-3
