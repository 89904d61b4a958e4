"""CPU tests of the searchByNN rule (tests/lsh_reference.py, include/tb_capi.h): the drawing of the bit table, the library's
tb_lsh_draw_bits against it, and the rule's own properties -- with multi_probe_level = key_size it is the exhaustive nearest
neighbour, below that the index really prunes."""
import ctypes as C

import numpy as np
import pytest

from trackingbench_slam_amd import capi

import lsh_reference as lr


def _rand_desc(rng, n):
    return rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _flip(rng, rows, nflip):
    out = rows.copy()
    for r in out:
        for b in rng.choice(256, nflip, replace=False):
            r[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def test_draw_20_10_uses_200_distinct_bits_of_one_pool():
    b = lr.draw_bits(20, 10, 0)
    assert b.shape == (20, 10) and b.dtype == np.uint16 and b.max() < 256
    assert len(set(b.reshape(-1).tolist())) == 200
    assert np.array_equal(b, lr.draw_bits(20, 10, 0))
    assert not np.array_equal(b, lr.draw_bits(20, 10, 1))
    # a prefix of the tables is the same drawing: table t depends on the stream alone
    assert np.array_equal(lr.draw_bits(7, 10, 0), b[:7])


def test_draw_30_10_refills_before_table_25():
    b = lr.draw_bits(30, 10, 3)
    first, second = b[:25].reshape(-1), b[25:].reshape(-1)
    assert len(set(first.tolist())) == 250 and len(set(second.tolist())) == 50     # each pool's tables are disjoint
    assert set(first.tolist()) & set(second.tolist())                              # 250 + 50 > 256: the second pool is a new shuffle
    for t in range(30):
        assert len(set(b[t].tolist())) == 10
    # (32, 32): a pool serves 8 tables
    b = lr.draw_bits(32, 32, 5)
    for p in range(4):
        assert len(set(b[8 * p:8 * p + 8].reshape(-1).tolist())) == 256


@pytest.mark.parametrize("T,k,seed", [(20, 10, 0), (20, 10, 1), (30, 10, 3), (1, 1, 9), (32, 32, 2 ** 63 + 5), (4, 16, 12345), (2, 10, 7)])
def test_library_draws_the_same_table(T, k, seed):
    assert np.array_equal(capi.lsh_draw_bits(T, k, seed), lr.draw_bits(T, k, seed))


def test_library_draw_refuses_bad_sizes():
    out = np.zeros(64 * 64, np.uint16)
    for T, k in ((0, 10), (33, 10), (20, 0), (20, 33)):
        assert capi.lib().tb_lsh_draw_bits(T, k, C.c_uint64(0), out.ctypes.data_as(C.c_void_p)) == capi.TB_EINVAL
    assert capi.lib().tb_lsh_draw_bits(20, 10, C.c_uint64(0), None) == capi.TB_EINVAL


def test_full_probe_is_the_exhaustive_neighbour():
    rng = np.random.default_rng(0)
    d2 = _rand_desc(rng, 120)
    d2[40] = d2[7]; d2[90] = d2[7]                      # duplicated train rows
    d1 = np.concatenate([_flip(rng, d2[rng.integers(0, 120, 150)], 20), d2[[7, 40, 90]]])
    for T, k in ((20, 10), (1, 3)):
        raw = lr.match_lsh(d1, d2, lr.draw_bits(T, k, 0), k)
        j, dist = lr.exhaustive_nn(d1, d2)
        assert np.array_equal(raw["queryIdx"], np.arange(len(d1))) and np.array_equal(raw["trainIdx"], j)
        assert np.array_equal(raw["distance"], dist.astype(np.float32)) and (raw["imgIdx"] == 0).all()
        assert (raw["trainIdx"][-3:] == 7).all() and (raw["distance"][-3:] == 0).all()   # ties: the lower index


def test_the_index_prunes():
    """(T 2, k 10, L 0): 300 queries = random rows of a 64-row train set with 25 bits flipped. A query's own row is a candidate
    with probability about 1 - (1 - (231/256)^10)^2 = 0.58; an unrelated row with 2 / 1024."""
    rng = np.random.default_rng(1)
    d2 = _rand_desc(rng, 64)
    d1 = _flip(rng, d2[rng.integers(0, 64, 300)], 25)
    bits = lr.draw_bits(2, 10, 0)
    raw = lr.match_lsh(d1, d2, bits, 0)
    j, _ = lr.exhaustive_nn(d1, d2)
    none = 300 - len(raw)
    other = int((raw["trainIdx"] != j[raw["queryIdx"]]).sum())
    print("pruning at (2, 10, 0): %d of 300 queries without a candidate, %d with a neighbour that is not the exhaustive one" % (none, other))
    assert none >= 20 and other >= 5
    assert (np.diff(raw["queryIdx"]) > 0).all()
    # every listed neighbour is a candidate and no candidate beats it
    cand = lr.candidates(d1, d2, bits, 0)
    H = lr.hamming(d1, d2)
    for m in raw:
        q, t = m["queryIdx"], m["trainIdx"]
        assert cand[q, t] and m["distance"] == H[q, t]
        c = np.nonzero(cand[q])[0]
        assert all((H[q, x], x) >= (H[q, t], t) for x in c)
    assert not cand[np.setdiff1d(np.arange(300), raw["queryIdx"])].any()


def test_candidate_fraction_at_the_reference_parameters():
    """two unrelated random sets: P(candidate) = 1 - (1 - 56/1024)^20 = 0.675"""
    rng = np.random.default_rng(2)
    d1, d2 = _rand_desc(rng, 300), _rand_desc(rng, 300)
    frac = float(lr.candidates(d1, d2, lr.draw_bits(20, 10, 0), 2).mean())
    print("candidate fraction at (20, 10, 2) on 300 x 300 random descriptors: %.4f" % frac)
    assert abs(frac - 0.675) <= 0.02


def test_key_bit_addressing():
    """bit b is bit b % 8 of byte b / 8"""
    d = np.zeros((1, 32), np.uint8)
    d[0, 5] = 0x04                        # bit 42
    kb = lr.key_bits(d, np.array([[42, 41, 43]]))
    assert kb.tolist() == [[[1, 0, 0]]]


def test_filter_is_strict_and_float():
    bits = np.array([[0, 1, 2, 3]], np.uint16)                # an explicit table: every row below has these bits clear,
    d2 = np.zeros((3, 32), np.uint8)                          # so every pair is a candidate
    d2[1, 31] = 0x0f; d2[2, 30] = 0xff
    d1 = np.zeros((3, 32), np.uint8)
    d1[0, 29] = 0x03; d1[1, 31] = 0x0f; d1[1, 29] = 0x0f; d1[2, 30] = 0xff; d1[2, 29] = 0xff
    # nearest: q0 -> t0 at 2, q1 -> t1 at 4, q2 -> t2 at 8
    raw = lr.match_lsh(d1, d2, bits, 4)
    assert raw["trainIdx"].tolist() == [0, 1, 2] and raw["distance"].tolist() == [2.0, 4.0, 8.0]
    assert lr.search_by_nn(d1, d2, bits, 4, 2.0, 30.0)["queryIdx"].tolist() == [0]            # 4 < 2 * 2 is false: strict
    assert lr.search_by_nn(d1, d2, bits, 4, 2.5, 30.0)["queryIdx"].tolist() == [0, 1]
    assert lr.search_by_nn(d1, d2, bits, 4, 10.0, 8.0)["queryIdx"].tolist() == [0, 1]          # minTh: 8 < 8 is false
    assert lr.search_by_nn(d1, d2, bits, 4, 10.0, 8.5)["queryIdx"].tolist() == [0, 1, 2]
    # a raw list of one match: min_d is its own distance, so ratio > 1 keeps it and ratio 1 does not
    assert len(lr.search_by_nn(d1[:1], d2, bits, 4, 1.0, 30.0)) == 0
    assert len(lr.search_by_nn(d1[:1], d2, bits, 4, 1.5, 30.0)) == 1
    # min_d = 0 keeps nothing, as in searchByBF
    assert len(lr.search_by_nn(d2, d2, bits, 4, 10.0, 30.0)) == 0


def test_empty_sets():
    bits = lr.draw_bits(20, 10, 0)
    e = np.zeros((0, 32), np.uint8)
    d = _rand_desc(np.random.default_rng(3), 5)
    for a, b in ((e, d), (d, e), (e, e)):
        assert len(lr.match_lsh(a, b, bits, 2)) == 0 and len(lr.search_by_nn(a, b, bits, 2, 10.0, 30.0)) == 0
