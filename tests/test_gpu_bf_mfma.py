"""GPU parity tests (pytest -m gpu): searchByBF's nearest neighbours on the i8 matrix cores (k_bf_nn_mfma) against the scalar
popcount kernel (tb_debug_bf_scalar) and the CPU oracle. Integer results: every comparison is np.array_equal, field by field."""
import ctypes as C

import numpy as np
import pytest

import oracle
from trackingbench_slam_amd import capi

pytestmark = pytest.mark.gpu

EDGES = (1, 31, 32, 33, 63, 64, 65, 127, 129, 257, 513)


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.bf_scalar(False)
    c.close()


def _eq_struct(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), f


def _both(ctx, fn):
    """fn() with the matrix-core kernel and with the scalar one"""
    ctx.bf_scalar(False)
    try:
        new = fn()
        ctx.bf_scalar(True)
        old = fn()
    finally:
        ctx.bf_scalar(False)
    return new, old


def _check_host(ctx, d1, d2):
    """the four host forms on (d1, d2), both kernels, against the oracle"""
    for fn, ref in ((lambda: ctx.bf_match(d1, d2, True), oracle.bf_match(d1, d2, True)),
                    (lambda: ctx.bf_match(d1, d2, False), oracle.bf_match(d1, d2, False)),
                    (lambda: ctx.search_by_bf(d1, d2, 10, 30), oracle.search_by_bf(d1, d2, 10, 30)),
                    (lambda: ctx.search_by_bf(d1, d2, 1.5, 300), oracle.search_by_bf(d1, d2, 1.5, 300))):
        new, old = _both(ctx, fn)
        _eq_struct(new, old)
        _eq_struct(new, ref)


@pytest.fixture(scope="module")
def pool():
    """random descriptors with near neighbours: the second half is the first with a few bits flipped"""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 256, (600, 32), dtype=np.uint8)
    b = a.copy()
    for i in range(len(b)):
        for bit in rng.integers(0, 256, 1 + i % 7):
            b[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    return a, b[rng.permutation(len(b))]


def test_tile_edges(ctx, pool):
    a, b = pool
    for n1 in EDGES:
        for n2 in EDGES:   # every ordered pair: both orientations
            _check_host(ctx, a[:n1], b[:n2])


def _tie_sets(nc, where, nrows=70, seed=3):
    """nc candidates with one descriptor X at the indices `where`; rows: X itself, X with one bit flipped, and random ones"""
    rng = np.random.default_rng(seed)
    cand = rng.integers(0, 256, (nc, 32), dtype=np.uint8)
    x = rng.integers(0, 256, 32, dtype=np.uint8)
    for i in where:
        cand[i] = x
    rows = rng.integers(0, 256, (nrows, 32), dtype=np.uint8)
    rows[0::3] = x
    rows[1::3] = x
    rows[1::3, 7] ^= 0x10
    return rows, cand


@pytest.mark.parametrize("nc,where", [
    (300, (9, 3)),          # two registers of one lane (tile rows 3 and 9: lane half 0)
    (300, (5, 1)),          # the two lane halves of one tile (tile rows 1 and 5)
    (300, (40, 2)),         # two tiles of one chunk
    (300, (200, 7)),        # two chunks
    (300, (299, 131, 130, 64, 36, 17)),
    (2000, (1900, 100)),    # one pair of 2000 candidates: the chunks are split over workgroups
    (2000, (1999, 1023, 1024, 127, 128)),
])
def test_ties_first_index_wins(ctx, nc, where):
    rows, cand = _tie_sets(nc, where)
    first = min(where)
    # rows = the query side without the cross-check, the train side with it
    m = ctx.bf_match(rows, cand, False)
    assert np.all(m["trainIdx"][0::3] == first) and np.all(m["distance"][0::3] == 0)
    assert np.all(m["trainIdx"][1::3] == first) and np.all(m["distance"][1::3] == 1)
    _check_host(ctx, rows, cand)
    _check_host(ctx, cand, rows)


def test_many_rows_one_candidate(ctx):
    rng = np.random.default_rng(4)
    cand = rng.integers(0, 256, (200, 32), dtype=np.uint8)
    rows = np.repeat(cand[137:138], 500, axis=0)
    rows[::2, 0] ^= 1
    _check_host(ctx, rows, cand)
    _check_host(ctx, cand, rows)


def test_extremes_of_d(ctx):
    rng = np.random.default_rng(6)
    zeros, ones = np.zeros((1, 32), np.uint8), np.full((1, 32), 255, np.uint8)
    onebit = np.zeros((8, 32), np.uint8)
    for i in range(8):
        onebit[i, 4 * i + (i & 3)] = 1 << i           # bit i of a byte in k-step i
    nearly = 255 - onebit
    rnd = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    for a, b in ((zeros, ones), (ones, zeros), (zeros, zeros), (ones, ones),
                 (np.repeat(zeros, 40, 0), np.repeat(ones, 40, 0)),      # every distance 256: D = +256 with rows = zeros
                 (np.repeat(ones, 40, 0), np.repeat(zeros, 40, 0)),      # D = 0, popcount 256
                 (np.repeat(ones, 40, 0), np.repeat(ones, 33, 0)),       # D = -256, distance 0
                 (np.concatenate([zeros, ones, onebit, nearly, rnd]), np.concatenate([rnd[:7], nearly, ones, onebit, zeros, rnd[7:]]))):
        _check_host(ctx, a, b)
        _check_host(ctx, b, a)
    # the distances themselves
    m = ctx.bf_match(np.repeat(zeros, 40, 0), np.repeat(ones, 40, 0), False)
    assert np.all(m["distance"] == 256) and np.all(m["trainIdx"] == 0)
    m = ctx.bf_match(np.repeat(ones, 40, 0), np.repeat(ones, 33, 0), False)
    assert np.all(m["distance"] == 0) and np.all(m["trainIdx"] == 0)


def _batch(ctx, pairs, set_pitch, ratio, min_th, cap):
    """tb_search_by_bf_batch_dev on `pairs` of (d1, d2) at `set_pitch` bytes per set, the bytes beyond each count 0xff:
    (matches per pair, counts, the raw output bytes)"""
    import torch
    S = len(pairs)
    D = np.full((2, S, set_pitch), 0xff, np.uint8)
    cnt = np.zeros((2, S), np.int32)
    for i, (d1, d2) in enumerate(pairs):
        for side, d in enumerate((d1, d2)):
            D[side, i, :len(d) * 32] = np.ascontiguousarray(d, np.uint8).reshape(-1)
            cnt[side, i] = len(d)
    tD, tc = torch.from_numpy(D).cuda(), torch.from_numpy(cnt).cuda()
    out = torch.zeros((S, cap, capi.MATCH.itemsize), dtype=torch.uint8, device="cuda")
    oc = torch.zeros(S, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx.check(capi.lib().tb_search_by_bf_batch_dev(ctx._h, S, p(tD[0]), p(tc[0]), p(tD[1]), p(tc[1]), C.c_size_t(set_pitch),
                                                   C.c_float(ratio), C.c_float(min_th), p(out), cap, p(oc)))
    ctx.synchronize()
    counts = oc.cpu().numpy()
    raw = out.cpu().numpy()
    lists = [raw[i].reshape(-1).view(capi.MATCH)[:min(int(counts[i]), cap)].copy() for i in range(S)]
    return lists, counts, np.concatenate([l.view(np.uint8).reshape(-1) for l in lists] + [counts.view(np.uint8)])


def _check_batch(ctx, pairs, set_pitch, ratio, min_th, cap):
    (new, nc, nraw), (old, ocn, _) = _both(ctx, lambda: _batch(ctx, pairs, set_pitch, ratio, min_th, cap))
    assert np.array_equal(nc, ocn)
    for i, (d1, d2) in enumerate(pairs):
        _eq_struct(new[i], old[i])
        ref = oracle.search_by_bf(d1, d2, ratio, min_th) if len(d1) and len(d2) else np.zeros(0, capi.MATCH)
        assert nc[i] == len(ref)
        _eq_struct(new[i], ref)
    return nraw


def test_ragged_batch(ctx, pool):
    a, b = pool
    rng = np.random.default_rng(8)
    n = 733                                  # max_n: no multiple of the tile, the chunk or the row block
    full1 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    full2 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    full2[:200] = full1[300:500]
    e = a[:0]
    pairs = [(e, b[:500]), (a[:500], e), (a[:1], b[:1]), (a[:33], full2[:700]), (full1[:700], b[:33]), (a[:513], b[:257]),
             (full1, full2), (full2, full1)]
    for ratio, min_th in ((10.0, 30.0), (1.5, 300.0)):
        _check_batch(ctx, pairs, n * 32 + 16, ratio, min_th, n)   # 16 bytes of pitch beyond max_n descriptors


def test_many_pairs_store_grid(ctx, pool):
    """enough pairs that a workgroup sweeps every candidate of its rows and stores: no atomics, no fill of the best rows --
    empty sides, ragged counts and a scratch that the scalar kernel's call before it left full of other pairs' results"""
    a, b = pool
    e = a[:0]
    rng = np.random.default_rng(10)
    pairs = [(e, b[:300]), (a[:300], e), (a[:1], b[:1])]
    while len(pairs) < 192:
        n1, n2 = (int(x) for x in rng.integers(1, 521, 2))
        o1, o2 = (int(x) for x in rng.integers(0, 80, 2))
        pairs.append((a[o1:o1 + n1], b[o2:o2 + n2]))
    pairs[5] = (a[:520], b[:520])
    _check_batch(ctx, pairs[::-1], 520 * 32, 1.5, 300.0, 520)
    _check_batch(ctx, pairs, 520 * 32, 1.5, 300.0, 520)


@pytest.mark.parametrize("npairs", [1, 3])
def test_few_pairs_grid(ctx, npairs):
    rng = np.random.default_rng(20 + npairs)
    pairs = []
    for _ in range(npairs):
        d1 = rng.integers(0, 256, (2000, 32), dtype=np.uint8)
        d2 = rng.integers(0, 256, (2000, 32), dtype=np.uint8)
        d2[rng.permutation(2000)[:600]] = d1[rng.permutation(2000)[:600]]
        pairs.append((d1, d2))
    _check_batch(ctx, pairs, 2000 * 32, 1.5, 300.0, 2000)


def test_determinism(ctx, pool):
    a, b = pool
    rng = np.random.default_rng(9)
    big1 = rng.integers(0, 256, (2000, 32), dtype=np.uint8)
    big2 = big1[rng.permutation(2000)].copy()
    big2[::5, 3] ^= 4
    for pairs, pitch in (([(big1, big2)], 2000 * 32), ([(a[:513], b[:257])] * 2 + [(big1[:600], big2[:600])] * 2, 600 * 32)):
        r1 = _batch(ctx, pairs, pitch, 1.5, 300.0, pitch // 32)[2]
        r2 = _batch(ctx, pairs, pitch, 1.5, 300.0, pitch // 32)[2]
        assert np.array_equal(r1, r2)
    m1, m2 = ctx.bf_match(big1, big2, True), ctx.bf_match(big1, big2, True)
    assert m1.tobytes() == m2.tobytes()
