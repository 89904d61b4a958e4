"""CPU tests of tb_bow_score, the host form of TemplatedVocabulary::score (TemplatedVocabulary.h:156-162, :1199-1203;
ScoringObject.cpp:23-311), against the sequential restatement tests/bow_score_reference.py: BowVectors of seeded descriptors
through oracle.bow_transform / oracle.bow_containers (both pinned to the reference's own DBoW2 by tests/test_ref_dbow2.py),
hand-built edge cases, and the recorded genuine-DBoW2 BowVectors of tests/golden/ref_dbow2_v1.npz. Codes 0, 1, 2, 4, 5 compare as
64-bit patterns, KL within the derived bound (bow_score_reference.kl_bound). The same vectors feed tests/test_gpu_bow_score.py."""
import ctypes as C
import math

import numpy as np
import pytest

import bow_score_reference as br
from bow_score_inputs import HAND, NFRAMES, SHAPES, _v, vectors
import oracle
import ref_dbow2_cases as cases
from trackingbench_slam_amd import capi, synth

def check(scoring, a, b, what):
    exp = br.score_detail(scoring, a[0], a[1], b[0], b[1])
    got = capi.bow_score(scoring, a[0], a[1], b[0], b[1])
    assert br.same(scoring, got, exp), (what, scoring, got, exp)
    return got


@pytest.mark.parametrize("k,L,n", SHAPES)
@pytest.mark.parametrize("scoring", range(6))
def test_every_ordered_pair_under_every_scoring(k, L, n, scoring):
    vs = vectors(k, L, n, scoring)
    for i, a in enumerate(vs):
        assert np.all(np.diff(a[0]) > 0)
        for j, b in enumerate(vs):
            if i != j:
                assert len(np.intersect1d(a[0], b[0])) >= 1, "a pair without a common word checks nothing"
            got = check(scoring, a, b, (k, L, n, i, j))
            if i == j and scoring == br.KL:
                assert got == 0.0                  # vi * log(vi / vi) = vi * 0
    if scoring in (br.L1_NORM, br.L2_NORM):        # a vector against itself scores 1 up to rounding, others below
        for i, a in enumerate(vs):                 # (L2: 1 - sqrt(1 - s) turns s = 1 - 1e-15 into 1 - 3e-8)
            assert abs(capi.bow_score(scoring, a[0], a[1], a[0], a[1]) - 1.0) < (1e-12 if scoring == br.L1_NORM else 1e-6)
            assert capi.bow_score(scoring, a[0], a[1], vs[(i + 1) % NFRAMES][0], vs[(i + 1) % NFRAMES][1]) < 0.9


def test_kl_is_not_symmetric_and_lower_is_more_similar():
    vs = vectors(10, 3, 500, br.KL)
    ab = capi.bow_score(br.KL, *vs[0], *vs[1]); ba = capi.bow_score(br.KL, *vs[1], *vs[0])
    assert ab != ba and ab > 0 and ba > 0
    assert capi.bow_score(br.KL, *vs[0], *vs[0]) < ab


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_cases(name):
    a, b = HAND[name]
    # "chi zero sum" holds a negative value: KL's log of it is a NaN on both sides, Bhattacharyya's sqrt of a negative product too
    for scoring in range(6):
        check(scoring, a, b, name)
        check(scoring, b, a, name)


def test_the_hand_built_cases_take_the_branches_they_are_named_for():
    a, b = HAND["chi zero sum"]
    assert a[1][1] + b[1][1] == 0.0
    with_term = 2. * (a[1][0] * b[1][0] / (a[1][0] + b[1][0]) + a[1][2] * b[1][2] / (a[1][2] + b[1][2]))
    assert capi.bow_score(br.CHI_SQUARE, *a, *b) == with_term
    a, b = HAND["l2 sum above 1"]
    assert sum(x * y for x, y in zip(a[1], b[1])) >= 1 and capi.bow_score(br.L2_NORM, *a, *b) == 1.0      # :114
    a, b = HAND["kl tail"]
    assert a[0][-1] > b[0][-1] and a[0][-2] > b[0][-1]
    _, _, n, _ = br.score_detail(br.KL, *a, *b)
    assert n == 5                                  # one common-word term, one word before a word of v2, three past v2's end
    for scoring in range(6):
        assert capi.bow_score(scoring, *HAND["both empty"][0], *HAND["both empty"][1]) == 0.0
    assert capi.bow_score(br.KL, *HAND["b empty"][0], *HAND["b empty"][1]) > 0      # all of v1 is tail
    assert capi.bow_score(br.KL, *HAND["a empty"][0], *HAND["a empty"][1]) == 0.0


def recorded_vectors(w, s):
    """the genuine transform's `bow` lines of the fixture under weighting w and scoring s, one vector per tree (and part)"""
    out = []
    for tree in cases.TREES:
        for part in (("a", "b") if (w, s) == (0, 0) else ("a",)):
            rec = cases.recorded("transform", cases.transform_name(tree, w, s, part))
            out.append((rec["bow_ids"].astype(np.int32), rec["bow_bits"].astype(np.uint64).view(np.float64)))
    return out


@pytest.mark.parametrize("w,s", cases.WS_RECORDED)
def test_recorded_genuine_bow_vectors_scored_under_their_own_scoring(w, s):
    vs = recorded_vectors(w, s)
    assert len(vs) >= len(cases.TREES) and all(len(v[0]) > 0 for v in vs)
    common = 0
    for i, a in enumerate(vs):
        for j, b in enumerate(vs):
            check(s, a, b, (w, s, i, j))
            common += len(np.intersect1d(a[0], b[0])) if i != j else 0
    assert common > 0


def test_argument_checks():
    L = capi.lib()
    aw, av = _v([1, 2], [0.5, 0.5])
    out = C.c_double(7.0)
    p = lambda x: x.ctypes.data_as(C.c_void_p)
    good = [0, p(aw), p(av), 2, p(aw), p(av), 2, C.byref(out)]
    assert L.tb_bow_score(*good) == 0 and out.value == 1.0
    for i, v in ((0, -1), (0, 6), (3, -1), (6, -1), (1, None), (2, None), (4, None), (5, None), (7, None)):
        bad = list(good); bad[i] = v
        assert L.tb_bow_score(*bad) == capi.TB_EINVAL, (i, v)
    assert L.tb_bow_score(0, None, None, 0, None, None, 0, C.byref(out)) == 0 and out.value == 0.0      # empty lists may be null
    assert math.isclose(br.LOG_EPS, math.log(2.0 ** -52))
