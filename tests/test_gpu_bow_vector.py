"""GPU parity tests (pytest -m gpu) of tb_bow_vector_batch_dev, the BowVector half of Frame::SetBow on the device
(TemplatedVocabulary::transform, TemplatedVocabulary.h:1124-1188; BowVector::normalize, BowVector.cpp:57-80):

 - against the reference's OWN DBoW2 code, the `bow` lines of the genuine transform (tests/ref_dbow2_cases.py): the live driver
   oracle/_ref/ref_dbow2 where it travelled (every weighting x scoring pair), tests/golden/ref_dbow2_v1.npz otherwise (the recorded
   pairs);
 - against oracle.bow_containers (pinned to the same code by tests/test_ref_dbow2.py) on batches the driver's cases do not reach:
   ragged counts, an empty frame, a frame whose words are all stopped, long runs of one word, desc_pitch 8192.

Words and counts compare exactly, values as 64-bit patterns."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
import ref_dbow2_cases as cases
from oracle import ref_dbow2
from trackingbench_slam_amd import capi, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _transform_then_vector(ctx, h, frames, pitch, levelsup):
    """tb_bow_transform_batch_dev, then tb_bow_vector_batch_dev on the arrays it wrote"""
    F = len(frames)
    D = np.random.default_rng(1).integers(0, 256, (F, pitch, 32), dtype=np.uint8)       # garbage in the padding
    for f, d in enumerate(frames):
        D[f, :len(d)] = d
    dD, dc = _dev(D), _dev(np.array([len(d) for d in frames], np.int32))
    wid = torch.full((F, pitch), -7, dtype=torch.int32, device="cuda")
    wt = torch.full((F, pitch), 5.0, dtype=torch.float64, device="cuda")                # what lies beyond counts[f] is not read
    ctx.check(capi.lib().tb_bow_transform_batch_dev(ctx._h, h, F, C.c_void_p(dD.data_ptr()), C.c_void_p(dc.data_ptr()), pitch, levelsup,
                                                    C.c_void_p(wid.data_ptr()), None, C.c_void_p(wt.data_ptr()), None, None))
    bw, bv, bc = ctx.bow_vector_batch_dev(h, wid, wt, dc)
    ctx.synchronize()
    return bw.cpu().numpy(), bv.cpu().numpy(), bc.cpu().numpy()


@pytest.mark.parametrize("tree", cases.TREES)
def test_bow_vector_vs_the_genuine_transform(ctx, tree):
    pairs = cases.WS_ALL if ref_dbow2.available() else cases.WS_RECORDED
    for w, s in pairs:
        parts = ("a", "b") if (w, s) == (0, 0) else ("a",)
        outs = [cases.genuine("transform", cases.transform_name(tree, w, s, p)) for p in parts]
        ins = [cases.transform_inputs(cases.transform_name(tree, w, s, p)) for p in parts]
        voc, levelsup = ins[0][0], ins[0][2]
        assert (voc.c.weighting, voc.c.scoring) == (w, s)
        frames = [ins[0][1]] + ([np.zeros((0, 32), np.uint8), ins[1][1]] if len(parts) == 2 else [])
        h = ctx.vocab_create(voc)
        try:
            bw, bv, bc = _transform_then_vector(ctx, h, frames, 320, levelsup)
        finally:
            ctx.vocab_destroy(h)
        if len(parts) == 2:
            assert bc[1] == 0
        for f, out in zip((0, 2), outs):
            n = len(out["bow_ids"])
            where = (tree, w, s, f)
            assert n > 0 and int(bc[f]) == n, where
            assert np.array_equal(bw[f, :n], out["bow_ids"]), where
            assert np.array_equal(bv[f, :n].view(np.uint64), out["bow_bits"]), where
    print("%s: %d weighting x scoring pairs (%s)" % (tree, len(pairs), "live driver" if ref_dbow2.available() else "fixture"))


def _plain_vocab(w, s):
    base = synth.vocabulary(2, 3, 2)
    return synth.Vocabulary(base.k, base.L, base.child_start, base.child_items, base.desc, base.word_id, base.weight, w, s)


def _expect(wid, wt, w, s):
    bv, _ = oracle.bow_containers(wid, wt, np.zeros(len(wid), np.int32), weighting=w, scoring=s)
    return np.array(list(bv), np.int32), np.array(list(bv.values()), np.float64)


def _check(ctx, w, s, wid, wt, cnt, what):
    h = ctx.vocab_create(_plain_vocab(w, s))
    try:
        bw, bv, bc = ctx.bow_vector_batch_dev(h, _dev(wid), _dev(wt), _dev(cnt))
        ctx.synchronize()
    finally:
        ctx.vocab_destroy(h)
    bw, bv, bc = bw.cpu().numpy(), bv.cpu().numpy(), bc.cpu().numpy()
    for f in range(len(cnt)):
        ew, ev = _expect(wid[f, :cnt[f]], wt[f, :cnt[f]], w, s)
        assert int(bc[f]) == len(ew), (what, w, s, f)
        assert np.array_equal(bw[f, :len(ew)], ew), (what, w, s, f)
        assert np.array_equal(bv[f, :len(ew)].view(np.uint64), ev.view(np.uint64)), (what, w, s, f)
    return bc


def _batch(pitch, counts, nwords, seed, stop_frac=0.1):
    """word ids and weights as the transform writes them: a weight per word (some stopped), garbage beyond the counts"""
    rng = np.random.default_rng(seed)
    F = len(counts)
    wid = rng.integers(0, 50, (F, pitch)).astype(np.int32)
    wt = rng.uniform(0.1, 3.0, (F, pitch))
    for f, (n, nw) in enumerate(zip(counts, nwords)):
        table = rng.uniform(1e-3, 3.0, nw)
        table[rng.uniform(size=nw) < stop_frac] = 0.0
        wid[f, :n] = rng.integers(0, nw, n)
        wt[f, :n] = table[wid[f, :n]]
    return wid, wt, np.array(counts, np.int32)


@pytest.mark.parametrize("w,s", cases.WS_ALL)
def test_bow_vector_vs_oracle_at_pitch_8192(ctx, w, s):
    """full frames, ragged counts, an empty frame, one feature, a frame whose words are all stopped, long runs (5 words over 8192
    features: the sums of a word run over 1600 terms, whose order shows in the last bits)"""
    pitch = 8192
    counts = [8192, 5000, 0, 1, 3000, 8192, 8191]
    wid, wt, cnt = _batch(pitch, counts, [100000, 700, 1, 5, 300, 5, 4000], 100 + 10 * w + s)
    wt[4, :3000] = 0.0                                                   # every word of frame 4 is stopped
    wt[3, 0] = 1.25
    bc = _check(ctx, w, s, wid, wt, cnt, "pitch 8192")
    assert bc[2] == 0 and bc[4] == 0 and bc[3] == 1 and bc[0] > 6000 and 1 <= bc[5] <= 5


def test_bow_vector_small_pitches_and_a_batch_of_many_frames(ctx):
    for pitch, F in ((1, 3), (2, 2), (63, 5), (2100, 64)):
        rng = np.random.default_rng(pitch)
        counts = rng.integers(0, pitch + 1, F).tolist()
        counts[0] = pitch
        wid, wt, cnt = _batch(pitch, counts, [max(1, pitch // 3)] * F, 7 + pitch)
        for w, s in ((0, 0), (1, 5), (2, 1), (3, 3), (0, 1)):
            _check(ctx, w, s, wid, wt, cnt, "pitch %d" % pitch)


def test_bow_vector_order_of_the_sums_is_the_references(ctx):
    """values chosen so that another order gives other bits: one word whose weights differ by 2^-52 steps could not come from a
    vocabulary, so the word's run uses one weight and the NORM carries the order: many words of very different magnitude"""
    pitch, nw = 4096, 4096
    rng = np.random.default_rng(3)
    wid = rng.permutation(nw).astype(np.int32)[None]
    table = np.exp(rng.uniform(-30, 30, nw))
    wt = table[wid]
    cnt = np.array([pitch], np.int32)
    for w, s in ((0, 0), (0, 1), (2, 0), (2, 1)):
        _check(ctx, w, s, wid, wt, cnt, "norm order")
        # the yardstick itself depends on the order: the same norm summed in descending word order gives other bits (every word
        # occurs once, so the values before normalisation are the table in word order)
        vals = table
        fwd = 0.0
        for v in vals:
            fwd += v * v if s == 1 else abs(v)
        back = 0.0
        for v in vals[::-1]:
            back += v * v if s == 1 else abs(v)
        assert fwd != back


def test_argument_checks(ctx):
    h = ctx.vocab_create(_plain_vocab(0, 0))
    other = capi.Context(0)
    L = capi.lib()
    try:
        wid, wt, cnt = _batch(64, [64, 10], [9, 9], 1)
        dw, dt, dc = _dev(wid), _dev(wt), _dev(cnt)
        ow = torch.zeros_like(dw); ov = torch.zeros_like(dt); oc = torch.zeros_like(dc)
        p = lambda t: C.c_void_p(t.data_ptr())
        good = [ctx._h, h, 2, p(dw), p(dt), p(dc), 64, p(ow), p(ov), p(oc)]
        assert L.tb_bow_vector_batch_dev(*good) == 0
        for i in (0, 1, 3, 4, 5, 7, 8, 9):
            bad = list(good); bad[i] = None
            assert L.tb_bow_vector_batch_dev(*bad) == capi.TB_EINVAL, i
        for i, v in ((2, -1), (6, -1), (6, 8193)):
            bad = list(good); bad[i] = v
            assert L.tb_bow_vector_batch_dev(*bad) == capi.TB_EINVAL, (i, v)
        bad = list(good); bad[0] = other._h                       # the vocabulary belongs to another context
        assert L.tb_bow_vector_batch_dev(*bad) == capi.TB_EINVAL
        bad = list(good); bad[2] = 0                              # no frames: nothing to do
        assert L.tb_bow_vector_batch_dev(*bad) == 0
        ctx.synchronize()
    finally:
        ctx.vocab_destroy(h)
        other.close()
