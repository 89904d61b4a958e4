"""GPU tests of the searchByNN matcher (tb_match_lsh, tb_search_by_nn, tb_search_by_nn_batch_dev) against the numpy restatement
of the rule in tests/lsh_reference.py: match lists, distances by their bits and counts are exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from trackingbench_slam_amd import capi

import lsh_reference as lr

pytestmark = pytest.mark.gpu

PARAMS = ((20, 10, 2), (1, 10, 2), (2, 10, 0), (4, 16, 1), (32, 32, 0), (20, 10, 10))
# 0, 1, 63, 64, 65, 300 and 715 on either side: one lane, a wavefront and a train chunk (128) less / exactly / more than full,
# more than one query tile (256) and several chunks, neither a multiple of 4 nor of 64
SIZES = ((0, 300), (300, 0), (1, 1), (1, 715), (715, 1), (63, 65), (64, 64), (65, 63), (300, 715), (715, 300), (715, 715))
SEED = 11


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _flip(rng, rows, nflip):
    out = rows.copy()
    for r, nf in zip(out, nflip):
        for b in rng.choice(256, nf, replace=False):
            r[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def _sets(rng, n1, n2):
    """train: random rows, some duplicated; queries: train rows with 4 / 8 / 25 / 60 bits flipped and unrelated rows, so that
    every parameter set sees queries with and without candidates (no query at distance 0: min_d = 0 would make the filter
    keep nothing, as in searchByBF)"""
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    if n2 >= 8:
        d2[n2 // 2] = d2[3]; d2[n2 - 1] = d2[3]
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    if n2:
        src = rng.integers(0, n2, n1)
        if n2 >= 8 and n1 >= 8:
            src[:4] = (3, n2 // 2, n2 - 1, 3)
        nflip = rng.choice([4, 8, 25, 60], n1)
        rel = rng.random(n1) < 0.8
        d1[rel] = _flip(rng, d2[src[rel]], nflip[rel])
    return d1, d2


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(5)
    return {s: _sets(rng, *s) for s in SIZES}


@pytest.fixture(scope="module")
def expected(data):
    """the reference's raw lists, computed once: (params, sizes) -> list"""
    out = {}
    for T, k, L in PARAMS:
        bits = lr.draw_bits(T, k, SEED)
        for s, (d1, d2) in data.items():
            out[(T, k, L), s] = lr.match_lsh(d1, d2, bits, L)
    return out


def _filtered(raw, ratio, min_th):
    if len(raw) == 0:
        return raw
    return raw[raw["distance"] < min(np.float32(np.float32(ratio) * raw["distance"].min()), np.float32(min_th))]


@pytest.mark.parametrize("prm", PARAMS)
def test_host_forms_match_the_rule(ctx, data, expected, prm):
    T, k, L = prm
    h = ctx.lsh(T, k, L, seed=SEED)
    try:
        info = h.info()
        assert info[:3] == (T, k, L) and np.array_equal(info[3], lr.draw_bits(T, k, SEED))
        holes = 0
        for s, (d1, d2) in data.items():
            exp = expected[prm, s]
            got = ctx.match_lsh(h, d1, d2)
            assert np.array_equal(_bytes(got), _bytes(exp)), (prm, s)
            if L == k:   # every pair is a candidate: BFMatcher without cross-check, a path written and tested separately
                assert np.array_equal(_bytes(got), _bytes(ctx.bf_match(d1, d2, crosscheck=False))), (prm, s)
                assert len(got) == (s[0] if s[1] else 0)
            q = exp["queryIdx"]
            holes += len(q) > 2 and bool((np.diff(q) > 1).any())   # a query without a candidate in the middle of the list
            for ratio, min_th in ((10.0, 30.0), (3.0, 64.0), (1.0, 30.0), (1000.0, 300.0)):
                want = _filtered(exp, ratio, min_th)
                got = ctx.search_by_nn(h, d1, d2, ratio, min_th)
                assert np.array_equal(_bytes(got), _bytes(want)), (prm, s, ratio, min_th)
        if L < k:
            assert holes, prm
    finally:
        h.close()


def test_a_pair_without_any_candidate(ctx):
    rng = np.random.default_rng(6)
    d1, d2 = rng.integers(0, 256, (70, 32), dtype=np.uint8), rng.integers(0, 256, (130, 32), dtype=np.uint8)
    bits = lr.draw_bits(1, 32, 0)
    assert len(lr.match_lsh(d1, d2, bits, 0)) == 0          # 32 key bits must agree: 2^-32 per pair
    h = ctx.lsh(1, 32, 0, seed=0)
    try:
        assert len(ctx.match_lsh(h, d1, d2)) == 0 and len(ctx.search_by_nn(h, d1, d2, 10.0, 30.0)) == 0
        # one query gets a candidate: a raw list of one match, which the filter keeps iff ratio > 1 (and it is below minTh)
        d1[41] = d2[77]; d1[41, 0] ^= 1 << (int(np.setdiff1d(np.arange(8), bits[0])[0]))
        raw = ctx.match_lsh(h, d1, d2)
        assert np.array_equal(_bytes(raw), _bytes(lr.match_lsh(d1, d2, bits, 0))) and raw.tolist() == [(41, 77, 0, 1.0)]
        assert len(ctx.search_by_nn(h, d1, d2, 1.0, 30.0)) == 0 and len(ctx.search_by_nn(h, d1, d2, 1.5, 30.0)) == 1
        assert len(ctx.search_by_nn(h, d1, d2, 1.5, 1.0)) == 0
    finally:
        h.close()


def test_duplicated_train_rows_give_the_lower_index(ctx, data):
    d2 = data[(715, 715)][1]
    assert np.array_equal(d2[3], d2[357]) and np.array_equal(d2[3], d2[714])
    d1 = np.concatenate([d2[[714, 357, 3]], data[(715, 715)][0][:3]])   # the copies themselves, then flipped copies of them
    h = ctx.lsh(seed=SEED)
    try:
        raw = ctx.match_lsh(h, d1, d2)
        assert raw["queryIdx"].tolist() == list(range(6)) and raw["trainIdx"].tolist() == [3] * 6
        assert raw["distance"][:3].tolist() == [0.0] * 3 and (raw["distance"][3:] > 0).all()
        assert len(ctx.search_by_nn(h, d1, d2, 10.0, 30.0)) == 0        # min_d = 0: the filter keeps nothing
    finally:
        h.close()


def test_explicit_table_equals_the_seed(ctx, data):
    d1, d2 = data[(300, 715)]
    a, b = ctx.lsh(20, 10, 2, seed=SEED), ctx.lsh(20, 10, 2, seed=999, bits=lr.draw_bits(20, 10, SEED))
    c = ctx.lsh(20, 10, 2, seed=SEED + 1)
    try:
        ra, rb, rc = ctx.match_lsh(a, d1, d2), ctx.match_lsh(b, d1, d2), ctx.match_lsh(c, d1, d2)
        assert np.array_equal(_bytes(ra), _bytes(rb))
        assert np.array_equal(b.info()[3], a.info()[3]) and not np.array_equal(c.info()[3], a.info()[3])
        assert np.array_equal(_bytes(rc), _bytes(lr.match_lsh(d1, d2, lr.draw_bits(20, 10, SEED + 1), 2)))
    finally:
        a.close(); b.close(); c.close()


def _batch(ctx, h, sets, pitch_rows, ratio, min_th, cap):
    n = len(sets)
    D1 = np.zeros((n, pitch_rows, 32), np.uint8); D2 = np.full((n, pitch_rows, 32), 0xA5, np.uint8)
    c1 = np.zeros(n, np.int32); c2 = np.zeros(n, np.int32)
    for i, (d1, d2) in enumerate(sets):
        D1[i, :len(d1)] = d1; D2[i, :len(d2)] = d2
        c1[i], c2[i] = len(d1), len(d2)
    t = [torch.from_numpy(x).cuda() for x in (D1, c1, D2, c2)]
    out = torch.zeros((n, cap, 4), dtype=torch.int32, device="cuda")
    cnt = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.search_by_nn_batch_dev(h, n, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), pitch_rows * 32, ratio, min_th,
                                    out.data_ptr(), cap, cnt.data_ptr())
    assert rc == 0, rc
    ctx.synchronize()
    return out.cpu().numpy(), cnt.cpu().numpy()


@pytest.mark.parametrize("prm", ((20, 10, 2), (2, 10, 0), (32, 32, 0)))
def test_ragged_batch_equals_the_single_calls(ctx, data, prm):
    """5 pairs at a pitch of 715 rows (no multiple of 4 or 64, larger than most counts), one of them empty"""
    T, k, L = prm
    sets = [data[s] for s in ((715, 715), (300, 715), (0, 300), (65, 63), (715, 1))]
    sets[2] = (sets[2][0], sets[2][1][:300])
    h = ctx.lsh(T, k, L, seed=SEED)
    try:
        out, cnt = _batch(ctx, h, sets, 715, 3.0, 64.0, 715)
        for i, (d1, d2) in enumerate(sets):
            single = ctx.search_by_nn(h, d1, d2, 3.0, 64.0)
            want = _filtered(lr.match_lsh(d1, d2, lr.draw_bits(T, k, SEED), L), 3.0, 64.0)
            assert np.array_equal(_bytes(single), _bytes(want)), (prm, i)
            assert cnt[i] == len(single), (prm, i)
            assert np.array_equal(out[i, :cnt[i]].reshape(-1).view(np.uint8), _bytes(single).reshape(-1)), (prm, i)
        assert cnt[2] == 0 and cnt[0] > 0
    finally:
        h.close()


def test_capacity(ctx, data):
    d1, d2 = data[(300, 715)]
    h = ctx.lsh(seed=SEED)
    try:
        full = ctx.search_by_nn(h, d1, d2, 1000.0, 300.0)
        assert len(full) > 10
        out = np.zeros(len(full), capi.MATCH)
        n = C.c_int(0)
        L = capi.lib()
        args = (ctx._h, h._h, capi._p(d1), len(d1), capi._p(d2), len(d2), C.c_float(1000.0), C.c_float(300.0), capi._p(out))
        assert L.tb_search_by_nn(*args, len(full) - 1, C.byref(n)) == capi.TB_ECAPACITY and n.value == len(full)
        assert not out.view(np.uint8).any()                                     # out is not written
        assert L.tb_search_by_nn(*args, len(full), C.byref(n)) == 0 and n.value == len(full)
        assert np.array_equal(_bytes(out), _bytes(full))
        # the device form truncates the list and reports the full count, as tb_search_by_bf_batch_dev does
        o, c = _batch(ctx, h, [(d1, d2)], 715, 1000.0, 300.0, 10)
        assert c[0] == len(full) and np.array_equal(o[0].reshape(-1).view(np.uint8), _bytes(full[:10]).reshape(-1))
    finally:
        h.close()


def test_argument_checks(ctx):
    def create(*a, **kw):
        with pytest.raises(capi.TBError) as e:
            ctx.lsh(*a, **kw)
        return e.value.code

    for bad in ((0, 10, 2), (33, 10, 2), (20, 0, 0), (20, 33, 2), (20, 10, -1), (20, 10, 11)):
        assert create(*bad) == capi.TB_EINVAL, bad
    for ok in ((1, 1, 0), (32, 32, 32), (20, 10, 10)):
        ctx.lsh(*ok).close()
    bits = lr.draw_bits(20, 10, 0)
    b = bits.copy(); b[7, 3] = 256
    assert create(bits=b) == capi.TB_EINVAL
    b = bits.copy(); b[7, 3] = b[7, 9]
    assert create(bits=b) == capi.TB_EINVAL
    b = bits.copy(); b[7, 3] = b[8, 3]            # repeated across tables only: allowed
    ctx.lsh(bits=b).close()
    h = ctx.lsh()
    other = capi.Context(0)
    try:
        big = np.zeros((8193, 32), np.uint8)
        one = np.zeros((1, 32), np.uint8)
        for a, bb in ((big, one), (one, big)):
            with pytest.raises(capi.TBError) as e:
                ctx.match_lsh(h, a, bb)
            assert e.value.code == capi.TB_EINVAL
        assert len(ctx.match_lsh(h, big[:8192], one)) == 8192
        with pytest.raises(capi.TBError) as e:    # a handle of another context
            other.match_lsh(h, one, one)
        assert e.value.code == capi.TB_EINVAL
        t = torch.zeros(64, dtype=torch.int32, device="cuda")
        p = t.data_ptr()
        assert ctx.search_by_nn_batch_dev(h, 1, p, p, p, p, 8193 * 32, 10.0, 30.0, p, 1, p) == capi.TB_EINVAL
        assert ctx.search_by_nn_batch_dev(h, 1, p, p, p, p, 16, 10.0, 30.0, p, 1, p) == capi.TB_EINVAL
        assert ctx.search_by_nn_batch_dev(h, 1, p, p, p, p, 64, 10.0, 30.0, p, 0, p) == capi.TB_EINVAL
        assert ctx.search_by_nn_batch_dev(h, -1, p, p, p, p, 64, 10.0, 30.0, p, 1, p) == capi.TB_EINVAL
        assert ctx.search_by_nn_batch_dev(h, 1, 0, p, p, p, 64, 10.0, 30.0, p, 1, p) == capi.TB_EINVAL
        assert ctx.search_by_nn_batch_dev(h, 0, p, p, p, p, 64, 10.0, 30.0, p, 1, p) == 0
    finally:
        other.close()
        h.close()
