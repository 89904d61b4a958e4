"""CPU tests of the descriptor kernel's reach (csrc/k_describe.hip blurs 37 x 37 around the keypoint: every rotated, rounded BRIEF
tap must lie within 18 px), and of the inputs tests/test_gpu_describe_reach.py runs: the oracle's keypoints alone hit every case
the kernel's staging, border path and blur can get wrong (tests/describe_reach_cases.py)."""
import numpy as np
import pytest

import oracle
import describe_reach_cases as dc


def test_pattern_norm_is_below_the_rounding_boundary():
    p = dc.pattern().reshape(512, 2).astype(np.float64)
    norm = np.sqrt((p * p).sum(axis=1)).max()
    assert abs(norm - np.sqrt(2.0) * 13) < 1e-12          # (+-13, +-13)
    assert norm + 0.01 < 18.5


def test_rotated_taps_stay_within_18_in_float32():
    """2^16 equally spaced angles and 2^16 random ones, float32 in the kernel's operation order: no rounded coordinate exceeds
    18, 18 occurs in rows and in columns, and the unrounded maximum keeps its distance from 18.5 (a cosf that differs from the
    double-precision one by an ulp cannot move a tap across the boundary)."""
    n = 1 << 16
    ang = np.concatenate([np.arange(n, dtype=np.float64) * (360.0 / n),
                          np.random.RandomState(7).uniform(0.0, 360.0, n)]).astype(np.float32)
    rmax = cmax = 0
    raw = 0.0
    for i in range(0, len(ang), 8192):
        r, c, m = dc.rotated_taps(ang[i:i + 8192])
        rmax, cmax, raw = max(rmax, int(np.abs(r).max())), max(cmax, int(np.abs(c).max())), max(raw, m)
    assert rmax == 18 and cmax == 18
    assert raw < 18.5 - 0.1


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_oracle_keypoints_cover_the_kernel_cases(name):
    w, h, seeds = dc.SETS[name]
    lvs, kps = [], []
    for s in seeds:
        lv, sf = oracle.pyramid(dc.image(s, w, h), dc.NLEVELS, dc.SCALE)
        k, _, _ = oracle.orb_extract(lv, sf, dc.TARGET, dc.INI_TH, dc.MIN_TH)
        assert len(k) >= 200
        lvs.append(lv)
        kps.append(k)
    dc.check_coverage(dc.coverage(lvs, sf, kps))
