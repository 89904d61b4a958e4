"""The cases that tests/test_ref_dbow2_score.py (CPU) and tests/test_gpu_ref_dbow2_score.py (GPU) put beside the reference's own
TemplatedVocabulary::score (oracle/ref_dbow2.py's `score` command runs it), and tools/gen_ref_dbow2_score_golden.py records into
tests/golden/ref_dbow2_score_v1.npz. A case is a list of BowVectors (words ascending, float64 values) and a list of pairs (i, j)
with v1 = vectors[i], v2 = vectors[j]; every pair is scored in both orders under all six scoring codes, each code through a
vocabulary the driver constructs with it. The inputs are seeded and rebuilt here, so the fixture stores results only, plus a
digest of each case's inputs (a fixture read beside other inputs fails with that message, not with a wrong score) -- and, for the
one case whose values go through exp(), the values themselves, since a C library's exp need not give the same last bit everywhere.

live(name) runs the driver, recorded(name) reads the fixture, genuine(name) takes the live driver where it exists and the fixture
otherwise: -> uint64 [6, npairs], the results' bit patterns per scoring code."""
import functools
import hashlib
import os

import numpy as np

import bow_score_reference as br
import oracle
import ref_dbow2_cases as tcases
from oracle import ref_dbow2
from bow_score_inputs import HAND, SHAPES, _v, random_vector, vectors

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_dbow2_score_v1.npz")
PITCHES = (8, 64, 130, 8192)           # the device tests' pitches; MAX_ENTRIES is the kernels' limit
MAX_ENTRIES = 8192


def both_orders(pairs):
    out = []
    for i, j in pairs:
        out.append((i, j))
        if i != j:
            out.append((j, i))
    return out


# ------------------------------------------------------------------ the genuine BowVectors (the transform cases' outputs)
@functools.lru_cache(maxsize=None)
def _transformed(tree, part):
    voc, desc, levelsup = tcases.transform_inputs(tcases.transform_name(tree, 0, 0, part))
    return oracle.bow_transform(voc, desc, levelsup)


def transform_vector(tree, w, s, part):
    """the BowVector of transform case tree-w-s-part through oracle.bow_transform / oracle.bow_containers, which
    tests/test_ref_dbow2.py holds equal to the genuine transform's bit for bit (test_genuine_vectors_* asserts it again)"""
    wid, wt, nid = _transformed(tree, part)
    bv, _ = oracle.bow_containers(wid, wt, nid, weighting=w, scoring=s)
    return np.array(list(bv), np.int32), np.array(list(bv.values()), np.float64)


def _genuine_case(tree):
    """per recorded (weighting, scoring) the two feature sets a and b: a-b in both orders, each against itself; and one pair
    across two normalisations. Vector 2 * q + p is part "ab"[p] under WS_RECORDED[q]."""
    vs = [transform_vector(tree, w, s, part) for w, s in tcases.WS_RECORDED for part in "ab"]
    pairs = []
    for q in range(len(tcases.WS_RECORDED)):
        pairs += [(2 * q, 2 * q + 1), (2 * q, 2 * q), (2 * q + 1, 2 * q + 1)]
    pairs.append((0, 5))              # tf-idf / L1-normalised a against idf / L2-normalised b
    return vs, pairs


# ------------------------------------------------------------------ the existing score inputs
def _frames_case(shape):
    """vectors(k, L, n, scoring) of tests/test_bow_score_reference.py: frames 0 and 1 under each scoring's normalisation"""
    vs, pairs = [], []
    for s in range(6):
        f = vectors(*shape, s)
        vs += [f[0], f[1]]
        pairs += [(2 * s, 2 * s + 1), (2 * s, 2 * s)]
    return vs, pairs


def _hand_case():
    vs, pairs = [], []
    for name in sorted(HAND):
        vs += list(HAND[name])
        pairs.append((len(vs) - 2, len(vs) - 1))
    return vs, pairs


def _chunk_case(sizes):
    rng = np.random.default_rng(11)
    vs = [random_vector(rng, n, 150) for n in sizes]
    return vs, [(i, j) for i in range(len(vs)) for j in range(i, len(vs))]


def _empties_case():
    """the 3 x 5 batch of tests/test_gpu_bow_score.py: an empty vector on either side, and on both"""
    rng = np.random.default_rng(12)
    e = (np.zeros(0, np.int32), np.zeros(0))
    A3 = [random_vector(rng, 40, 90), e, random_vector(rng, 70, 90)]
    B5 = [random_vector(rng, 65, 90), random_vector(rng, 5, 90), e, random_vector(rng, 90, 90), random_vector(rng, 1, 90)]
    return A3 + B5, [(i, 3 + j) for i in range(3) for j in range(5)]


def _five_words_case():
    """per scoring the frame of 5 words over 8192 features: against itself, a frame of 2000 keys and a short random vector"""
    vs, pairs = [], []
    for s in range(6):
        rng = np.random.default_rng(100 + s)
        table = rng.uniform(1e-3, 3.0, 5)
        wid = rng.integers(0, 5, 8192).astype(np.int32)
        bv, _ = oracle.bow_containers(wid, table[wid], np.zeros(8192, np.int32), weighting=0, scoring=s)
        five = (np.array(list(bv), np.int32), np.array(list(bv.values()), np.float64))
        assert 1 <= len(five[0]) <= 5
        at = len(vs)
        vs += [five, vectors(10, 5, 2000, s)[1], random_vector(rng, 37, 60)]
        pairs += [(at, at), (at, at + 1), (at, at + 2)]
    return vs, pairs


def order_of_sum_inputs():
    """terms of very different magnitude, values exp(U(-30, 30)): another order of the adds gives other bits"""
    rng = np.random.default_rng(3)
    n = 300
    w = np.arange(n, dtype=np.int32)
    return [(w, np.exp(rng.uniform(-30, 30, n))), (w, np.exp(rng.uniform(-30, 30, n)))]


def _order_case():
    """the values the fixture was recorded on (see the module's docstring); fresh_inputs() builds them anew for the generator"""
    z = _fixture()
    w = np.arange(300, dtype=np.int32)
    return [(w, z["score/order-of-sum/value_bits"][i].view(np.float64)) for i in range(2)], [(0, 1)]


def _full_pitch_case():
    """a vector that nearly fills the largest pitch against one of 2000 entries and against itself"""
    rng = np.random.default_rng(13)
    return [random_vector(rng, MAX_ENTRIES - 2, 9000), random_vector(rng, 2000, 9000)], [(0, 1), (0, 0)]


# ------------------------------------------------------------------ one case per branch of ScoringObject.cpp
U = 2.0 ** -52
BRANCH = {
    # no common word: only the lower_bound skips run (KL: every word of v1 is added, :204 or the tail); 7 and 8 entries
    "branch-disjoint": ([_v([1, 2, 3, 10, 11, 30, 31], [0.125, 0.25, 0.125, 0.125, 0.125, 0.125, 0.125]),
                         _v([5, 6, 7, 20, 21, 22, 40, 41], [0.125] * 8)], [(0, 1)]),
    # the walk ends because v1 ends (0, 1) / because v2 ends (1, 0), with common words before it and words left on the other side
    "branch-one-side-exhausted": ([_v([1, 4, 6], [0.5, 0.25, 0.25]), _v([1, 4, 6, 9, 12], [0.125, 0.25, 0.125, 0.25, 0.25])], [(0, 1)]),
    # KL :216-218: words 12, 15, 20 of v1 lie past v2's end; 15 holds 0 and is skipped, the others are added
    "branch-kl-tail-with-zero": ([_v([1, 4, 9, 12, 15, 20], [0.125, 0.25, 0.125, 0.25, 0.0, 0.25]), _v([0, 4, 8, 9], [0.25] * 4)], [(0, 1)]),
    # KL :204 has no zero guard: word 2 of v1 holds 0 and lies ahead of v2's word 5 -> 0 * (log 0 - LOG_EPS) = 0 * -inf = NaN
    "branch-kl-204-zero": ([_v([2, 5], [0.0, 1.0]), _v([5, 7], [0.5, 0.5])], [(0, 1)]),
    # KL :195: a zero on a common word, on either side, is skipped
    "branch-kl-common-zero": ([_v([3, 5, 8], [0.0, 0.5, 0.5]), _v([3, 5, 8], [0.25, 0.25, 0.5]), _v([3, 5, 8], [0.5, 0.0, 0.5])],
                              [(0, 1), (1, 2)]),
    # chi-square :148: vi + wi == 0 from +x and -x on word 2; the other words are added
    "branch-chi-zero-sum": ([_v([1, 2, 7], [0.3, 0.7, 0.1]), _v([1, 2, 7], [0.2, -0.7, 0.4])], [(0, 1)]),
    # Bhattacharyya :245: a negative product on word 2 -> sqrt gives NaN
    "branch-bhattacharyya-negative": ([_v([1, 2], [0.5, 0.5]), _v([1, 2], [0.5, -0.5])], [(0, 1)]),
    # L2 :114: unnormalised pairs whose dot product is exactly 1, 1 + 2^-52 and 1 - 2^-53 (each sum is exact)
    "branch-l2-clamp": ([_v([0, 1], [0.5, 0.5]), _v([0, 1], [1.0, 1.0]), _v([0, 1], [1.0, 1.0 + 2 * U]), _v([0, 1], [1.0, 1.0 - U])],
                        [(0, 1), (0, 2), (0, 3)]),
    # L1 :41 with values of mixed sign: |vi - wi| - |vi| - |wi| is 0 where the signs differ
    "branch-l1-mixed-sign": ([_v([1, 2, 3], [0.5, -0.25, 0.25]), _v([1, 2, 3], [-0.5, -0.5, 0.75])], [(0, 1)]),
    # a NaN, a negative zero (KL's `!= 0` guards skip it) and an infinity as values
    "branch-nan-negzero-inf": ([_v([1, 2, 3, 4], [np.nan, 0.5, -0.0, 0.25]), _v([1, 2, 3, 6], [0.5, 0.5, 0.5, 0.5]),
                                _v([2, 3, 4], [0.5, -0.0, np.inf])], [(0, 1), (1, 2), (0, 2)]),
}


# ------------------------------------------------------------------ the keyframe-database rings of the device test
RING_S, RING_CAP, RING_NADD = 2, 4, 7
RING_KF_IDS = [3, 10, 11, 25, 40, 41, 77]


def _ring_case():
    """per sequence s a query (vector s) and RING_NADD entries (vector RING_S + a * RING_S + s for add a), all distinct: the
    query is v1, as in the database; the other order is scored as well"""
    rng = np.random.default_rng(21)
    queries = [random_vector(rng, 400, 700) for _ in range(RING_S)]
    adds = [random_vector(rng, int(rng.integers(300, 501)), 700) for _ in range(RING_NADD * RING_S)]
    return queries + adds, [(s, ring_vector(a, s)) for a in range(RING_NADD) for s in range(RING_S)]


def ring_vector(a, s):
    return RING_S + a * RING_S + s


# ------------------------------------------------------------------ the case table
def _builders():
    b = {}
    for t in tcases.TREES:
        b["genuine-" + t] = functools.partial(_genuine_case, t)
    for shape in SHAPES:
        b["frames-k%d-L%d-n%d" % shape] = functools.partial(_frames_case, shape)
    b["hand"] = _hand_case
    b["chunk-edges-64"] = functools.partial(_chunk_case, (1, 63, 64))
    b["chunk-edges-128"] = functools.partial(_chunk_case, (64, 65, 1, 63, 128))
    b["empties-3x5"] = _empties_case
    b["five-words-of-8192-features"] = _five_words_case
    b["order-of-sum"] = _order_case
    b["full-pitch"] = _full_pitch_case
    for n, c in BRANCH.items():
        b[n] = (lambda c=c: c)
    b["ring"] = _ring_case
    return b


_BUILD = _builders()
NAMES = list(_BUILD)


def _checked(name, built):
    vs, pairs = built
    for w, v in vs:
        assert len(w) == len(v) <= MAX_ENTRIES and np.all(np.diff(w) > 0) and (len(w) == 0 or w[0] >= 0), name
    return list(vs), both_orders(pairs)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """-> (vectors, pairs): every pair in both orders. What the tests use."""
    return _checked(name, _BUILD[name]())


def fresh_inputs(name):
    """the same with nothing read from the fixture: what the generator records on (it passes them on as `inp`)"""
    return _checked(name, (order_of_sum_inputs(), [(0, 1)]) if name == "order-of-sum" else _BUILD[name]())


def digest(name, inp=None):
    vs, pairs = inp or inputs(name)
    h = hashlib.sha256()
    for w, v in vs:
        h.update(np.int64(len(w)).tobytes() + np.ascontiguousarray(w, np.int32).tobytes() + np.ascontiguousarray(v, np.float64).tobytes())
    h.update(np.array(pairs, np.int32).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def live(name, inp=None):
    vs, pairs = inp or inputs(name)
    out = ref_dbow2.score(vs, [pairs] * 6, "score/" + name)
    return np.stack([out["bits%d" % c] for c in range(6)])


def to_record(name, bits, inp=None):
    rec = {"bits": bits, "inputs_sha256": digest(name, inp)}
    if name == "order-of-sum":
        rec["value_bits"] = np.stack([v.view(np.uint64) for _, v in (inp or inputs(name))[0]])
    return rec


@functools.lru_cache(maxsize=None)
def _fixture():
    return np.load(GOLDEN, allow_pickle=False)


def recorded(name):
    z = _fixture()
    assert np.array_equal(z["score/%s/inputs_sha256" % name], digest(name)), \
        "case %s: the inputs rebuilt here are not those tests/golden/ref_dbow2_score_v1.npz was recorded on" % name
    bits = z["score/%s/bits" % name]
    assert bits.shape == (6, len(inputs(name)[1])) and bits.dtype == np.uint64, name
    return bits


def genuine(name):
    return live(name) if ref_dbow2.score_available() else recorded(name)


def detail(name, scoring, p, branches=None):
    """the restatement's score_detail of pair number p of the case"""
    vs, pairs = inputs(name)
    i, j = pairs[p]
    return br.score_detail(scoring, *vs[i], *vs[j], branches=branches)


# ------------------------------------------------------------------ the genuine ranking of the "ring" case
def ring_after(nadds, scoring):
    """per sequence the bow_score_reference.Ring after the first nadds adds of the ring case (the ring's bookkeeping -- which slot
    an add lands in, which slots a query ranks -- is the project's own rule: the vendored DBoW2 has no database class)"""
    vs, _ = inputs("ring")
    rings = [br.Ring(RING_CAP, scoring) for _ in range(RING_S)]
    for a in range(nadds):
        for s in range(RING_S):
            rings[s].add(*vs[ring_vector(a, s)], RING_KF_IDS[a])
    return rings


def ring_genuine_query(bits, scoring, nadds, topk, exclude_newest):
    """-> per sequence (expected per slot: (genuine score, A, n, M) or None where the slot is not ranked; top_slot, top_kf [topk]
    padded with -1; top_count): the order of the GENUINE scores `bits` (the ring case's [6, npairs]) -- better first, ascending
    for KL, ties to the lower kf_id. For KL asserts that neighbouring genuine scores lie more than twice the bound apart, so
    that the order is decided by arithmetic and not by a last bit."""
    vs, pairs = inputs("ring")
    out = []
    for s, ring in enumerate(ring_after(nadds, scoring)):
        exp = [None] * RING_CAP
        for slot in ring.ranked_slots(exclude_newest):
            a = RING_KF_IDS.index(ring.kf_ids[slot])
            p = pairs.index((s, ring_vector(a, s)))
            g = float(bits[scoring, p].view(np.float64))
            assert g == g, "the ring holds no NaN score"
            exp[slot] = (g,) + tuple(detail("ring", scoring, p)[1:])
        ranked = [slot for slot in range(RING_CAP) if exp[slot] is not None]
        sign = 1.0 if scoring == br.KL else -1.0
        order = sorted(ranked, key=lambda slot: (sign * exp[slot][0], ring.kf_ids[slot], slot))
        if scoring == br.KL:
            for x, y in zip(order, order[1:]):
                gap = exp[y][0] - exp[x][0]
                assert gap > 2.0 * max(br.kl_bound(*exp[x][1:]), br.kl_bound(*exp[y][1:])), (s, x, y, gap)
        top = order[:topk]
        pad = [-1] * (topk - len(top))
        out.append((exp, top + pad, [ring.kf_ids[slot] for slot in top] + pad, len(top)))
    return out


RING_QUERY_AFTER = (2, 4, 7)                               # part filled, just full, wrapped
RING_QUERIES = [(4, 0), (2, 1), (4, 2), (1, 0), (3, 5)]    # (topk, exclude_newest): topk above the entries, all excluded
