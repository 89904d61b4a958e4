"""GPU parity tests (pytest -m gpu) of tb_bow_score_batch_dev / k_bow_score, TemplatedVocabulary::score on the device
(TemplatedVocabulary.h:156-162, :1199-1203; ScoringObject.cpp:23-311), against the host form tb_bow_score and the sequential
restatement tests/bow_score_reference.py by one rule: 64-bit patterns for codes 0, 1, 2, 4, 5, the derived bound for KL. The vectors
are those of tests/test_bow_score_reference.py, packed so that a vector nearly fills its pitch (64) or sits in the largest one
(8192), plus vectors at the wavefront's chunk edges (1, 64, 65 entries), empty ones, and a frame of 5 words over 8192 features."""
import ctypes as C

import numpy as np
import pytest
import torch

import bow_score_reference as br
import oracle
from bow_score_inputs import HAND, pack, random_vector as _random_vector, vectors
from trackingbench_slam_amd import capi

pytestmark = pytest.mark.gpu

PITCH = {(4, 3, 300): 64, (10, 3, 500): 1000, (10, 5, 2000): 8192}


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def dev_scores(ctx, scoring, A, B, pa, pb, mode):
    out = ctx.bow_score_batch_dev(scoring, *pack(A, pa, 5), *pack(B, pb, 6), mode=mode)
    ctx.synchronize()
    return out.cpu().numpy()


def check_all_pairs(ctx, scoring, A, B, pa, pb, what):
    """all pairs on the device against the restatement and against the host form"""
    got = dev_scores(ctx, scoring, A, B, pa, pb, capi.TB_SCORE_ALL_PAIRS)
    assert got.shape == (len(A), len(B))
    for i, a in enumerate(A):
        for j, b in enumerate(B):
            exp = br.score_detail(scoring, *a, *b)
            assert br.same(scoring, got[i, j], exp), (what, scoring, i, j, got[i, j], exp)
            assert br.same(scoring, capi.bow_score(scoring, *a, *b), exp), (what, scoring, i, j)
    return got


@pytest.mark.parametrize("shape", sorted(PITCH))
@pytest.mark.parametrize("scoring", range(6))
def test_frames_in_both_modes(ctx, shape, scoring):
    vs = vectors(*shape, scoring)
    pitch = PITCH[shape]
    if pitch == 64:
        assert max(len(v[0]) for v in vs) >= 56       # a vector nearly fills its pitch
    ap = check_all_pairs(ctx, scoring, vs, vs, pitch, pitch, shape)
    if scoring == br.KL:
        assert not np.array_equal(ap, ap.T)           # v1 is the query
    rot = vs[1:] + vs[:1]
    pw = dev_scores(ctx, scoring, vs, rot, pitch, pitch, capi.TB_SCORE_PAIRWISE)
    assert pw.shape == (len(vs),)
    for i in range(len(vs)):                          # the same pair alone, in a pairwise batch and in an all-pairs batch: same bits
        j = (i + 1) % len(vs)
        alone = dev_scores(ctx, scoring, [vs[i]], [vs[j]], pitch, pitch, capi.TB_SCORE_PAIRWISE)
        assert pw[i].view(np.uint64) == ap[i, j].view(np.uint64) == alone[0].view(np.uint64), (shape, scoring, i)


@pytest.mark.parametrize("scoring", range(6))
def test_chunk_edges_empty_vectors_and_unequal_pitches(ctx, scoring):
    """1, 64 and 65 entries (one lane, a full wavefront chunk, one entry into the second chunk), 63 and 128, an empty vector on each
    side of a 3 x 5 all-pairs batch, and pitches that differ between the sides"""
    rng = np.random.default_rng(11)
    A = [_random_vector(rng, n, 150) for n in (64, 65, 1, 63, 128)]
    check_all_pairs(ctx, scoring, A, A, 128, 130, "chunk edges")
    e = (np.zeros(0, np.int32), np.zeros(0))
    A3 = [_random_vector(rng, 40, 90), e, _random_vector(rng, 70, 90)]
    B5 = [_random_vector(rng, 65, 90), _random_vector(rng, 5, 90), e, _random_vector(rng, 90, 90), _random_vector(rng, 1, 90)]
    got = check_all_pairs(ctx, scoring, A3, B5, 70, 90, "3 x 5")
    assert got.shape == (3, 5) and got[1, 2] == 0.0


@pytest.mark.parametrize("scoring", range(6))
def test_a_frame_of_5_words_over_8192_features_and_many_entries(ctx, scoring):
    """the long-run frame of k_bow_vector's tests (5 words over 8192 features) as query and as entry at pitch 8192, and enough
    entries that a workgroup scores more than one per wavefront"""
    rng = np.random.default_rng(100 + scoring)
    table = rng.uniform(1e-3, 3.0, 5)
    wid = rng.integers(0, 5, 8192).astype(np.int32)
    bv, _ = oracle.bow_containers(wid, table[wid], np.zeros(8192, np.int32), weighting=0, scoring=scoring)
    five = (np.array(list(bv), np.int32), np.array(list(bv.values()), np.float64))
    assert 1 <= len(five[0]) <= 5
    full = vectors(10, 5, 2000, scoring)
    lots = [five] + [_random_vector(rng, int(n), 3000) for n in rng.integers(0, 200, 40)]
    got = dev_scores(ctx, scoring, [five, full[0]], lots + [full[1]], 8192, 8192, capi.TB_SCORE_ALL_PAIRS)
    for i, a in enumerate([five, full[0]]):
        for j, b in enumerate(lots + [full[1]]):
            exp = br.score_detail(scoring, *a, *b)
            assert br.same(scoring, got[i, j], exp), (scoring, i, j, got[i, j], exp)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_cases(ctx, name):
    a, b = HAND[name]
    for scoring in range(6):
        check_all_pairs(ctx, scoring, [a, b], [a, b], 8, 8, name)


def test_order_of_the_sum_is_the_references(ctx):
    """terms of very different magnitude: another order of the adds gives other bits, and the restatement itself shows it"""
    rng = np.random.default_rng(3)
    n = 300
    w = np.arange(n, dtype=np.int32)
    a = (w, np.exp(rng.uniform(-30, 30, n)))
    b = (w, np.exp(rng.uniform(-30, 30, n)))
    for scoring in (br.DOT_PRODUCT, br.BHATTACHARYYA, br.CHI_SQUARE, br.L1_NORM):
        check_all_pairs(ctx, scoring, [a], [b], 300, 300, "order")
    fwd = back = 0.0
    for x, y in zip(a[1], b[1]):
        fwd += x * y
    for x, y in zip(a[1][::-1], b[1][::-1]):
        back += x * y
    assert fwd != back


def test_argument_checks(ctx):
    L = capi.lib()
    rng = np.random.default_rng(1)
    aw, av, ac = pack([_random_vector(rng, 10, 30), _random_vector(rng, 20, 30)], 32)
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    good = [ctx._h, 0, capi.TB_SCORE_ALL_PAIRS, 2, p(aw), p(av), p(ac), 32, 2, p(aw), p(av), p(ac), 32, p(out)]
    assert L.tb_bow_score_batch_dev(*good) == 0
    for i in (0, 4, 5, 6, 9, 10, 11, 13):
        bad = list(good); bad[i] = None
        assert L.tb_bow_score_batch_dev(*bad) == capi.TB_EINVAL, i
    for i, v in ((1, -1), (1, 6), (2, 2), (2, -1), (3, -1), (8, -1), (7, 0), (7, 8193), (12, 0), (12, 8193)):
        bad = list(good); bad[i] = v
        assert L.tb_bow_score_batch_dev(*bad) == capi.TB_EINVAL, (i, v)
    bad = list(good); bad[2] = capi.TB_SCORE_PAIRWISE; bad[8] = 1          # pairwise needs na == nb
    assert L.tb_bow_score_batch_dev(*bad) == capi.TB_EINVAL
    bad = list(good); bad[3] = 0                                           # no queries: nothing to do
    assert L.tb_bow_score_batch_dev(*bad) == 0
    ctx.synchronize()
