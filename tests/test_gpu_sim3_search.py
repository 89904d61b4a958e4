"""GPU tests (pytest -m gpu) of tb_search_by_sim3_batch_dev (include/tb_capi.h) against its definition, tests/sim3_search_reference.py:
match1, match2, the pairs with their distances, the counts and the stats are EQUAL, for batches of five pairs at side pitches 1, 5,
64, 67 and 300 (below, at and past one 256-key chunk; the 1024-key LDS tile is crossed at pitch 1100) with an empty side, garbage
beyond the counts, a malformed srt and an octave outside the table.

No tolerance and no boundary case to state: the kernel and the definition perform the same IEEE float64 operations in the same
order (+ - * / sqrt, no contraction), so every comparison is decided on the same bits; what is compared is integers."""
import numpy as np
import pytest
import torch

import sim3_cases as sc
import sim3_search_reference as ss
from trackingbench_slam_amd import capi

pytestmark = pytest.mark.gpu

K, WIDTH, HEIGHT, NLEVELS, SCALE = (360.0, 360.0, 320.0, 120.0), 640, 240, 5, 0.8
SHAPES = [(1, 5), (5, 1), (64, 67), (67, 64), (300, 300), (1100, 260)]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def make_pair(seed, n1, n2, s=1.1):
    """two views of one scene under X1 = s R X2 + t: (side1, side2, srt). Keys are views of random scene points in a random order, with
    pixel noise, a fifth of the descriptors heavily flipped, some keys without a point, some matched already, and a few duplicated
    descriptors (ties)."""
    rng = np.random.default_rng(seed)
    m = max(n1, n2, 1)
    X2 = np.stack([rng.uniform(-8, 8, m), rng.uniform(-3, 3, m), rng.uniform(-2, 30, m)], -1)
    X2[np.abs(X2[:, 2]) < 0.5, 2] = 0.5
    R = sc.rodrigues((0.2, 1.0, 0.1), 0.07)
    t = np.array([0.5, -0.1, 4.0])                 # camera 1 stands 4 m behind camera 2: points between them are behind camera 2
    X1 = s * X2 @ R.T + t
    base = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    # one physical size a point: the octave of its key follows the distance, as an ORB pyramid's does
    o1 = rng.integers(0, NLEVELS, m)
    d1, d2 = np.linalg.norm(X1, axis=1), s * np.linalg.norm(X2, axis=1)
    o2 = np.clip(np.round(o1 + np.log(d1 / d2) / np.log(1.25)), 0, NLEVELS - 1).astype(np.int64)
    sides = []
    for X, n, octv in ((X1, n1, o1), (X2, n2, o2)):
        ids = rng.permutation(m)[:n]
        front = X[ids, 2] > 0.4
        Z = np.where(front, X[ids, 2], 1.0)
        keys = np.zeros(n, capi.KEYPOINT)
        keys["x"] = np.where(front, K[0] * X[ids, 0] / Z + K[2] + rng.normal(0, 0.5, n), rng.uniform(0, WIDTH, n))
        keys["y"] = np.where(front, K[1] * X[ids, 1] / Z + K[3] + rng.normal(0, 0.5, n), rng.uniform(0, HEIGHT, n))
        keys["octave"] = octv[ids]
        keys["size"], keys["angle"], keys["class_id"] = 31.0, 0.0, -1
        bits = np.unpackbits(base[ids], axis=1)
        flips = np.where(rng.uniform(0, 1, (n, 1)) < 0.2, 60, 3)
        desc = np.packbits(bits ^ (rng.integers(0, 256, bits.shape) < flips).astype(np.uint8), axis=1)
        pts = X[ids].astype(np.float32)
        if n > 8:      # two keys of one point with one descriptor, a pixel apart: a tie the lower index has to win
            a, b = rng.permutation(n)[:2]
            keys[b], desc[b], pts[b], front[b] = keys[a], desc[a], pts[a], front[a]
            keys["x"][b] += 1.0
        sides.append(ss.side(keys, desc, pts, (rng.uniform(0, 1, n) < 0.85) & front, rng.uniform(0, 1, n) < 0.2))
    tr = np.trace(R)
    w = np.sqrt(1.0 + tr) / 2.0
    q = np.array([w, (R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w)])
    return sides[0], sides[1], np.concatenate([q / np.linalg.norm(q), t, [s]])


def problems(p1, p2):
    """five pairs for the side pitches p1, p2: full, partly filled, an empty side, a malformed srt (s = 0), an octave outside the table"""
    out = [make_pair(10 * p1 + p2, p1, p2), make_pair(11 * p1 + p2, max(p1 - 3, 0), max(p2 // 2, 1) if p2 > 1 else 1, s=0.9),
           make_pair(12 * p1 + p2, p1, 0), make_pair(13 * p1 + p2, p1, p2), make_pair(14 * p1 + p2, p1, p2)]
    out[3] = (out[3][0], out[3][1], np.concatenate([out[3][2][:7], [0.0]]))
    s2 = dict(out[4][1], keys=out[4][1]["keys"].copy())
    s2["keys"]["octave"][len(s2["keys"]) - 1] = NLEVELS
    out[4] = (out[4][0], s2, out[4][2])
    return out


def pack(probs, p1, p2, seed):
    """device tensors of a batch, garbage beyond the counts: ((keys, desc, pts, valid, matched, counts) x 2, srt)"""
    rng = np.random.default_rng(seed)
    P = len(probs)
    g = lambda shape, dt: rng.integers(0, 256, tuple(shape) + (np.dtype(dt).itemsize,), dtype=np.uint8).view(dt).reshape(shape)
    sides = []
    for k, pitch in ((0, p1), (1, p2)):
        keys, desc = g((P, pitch, 7), np.int32), g((P, pitch, 32), np.uint8)
        pts, val, mat = g((P, pitch, 3), np.float32), g((P, pitch), np.uint8), g((P, pitch), np.uint8)
        cnt = np.zeros(P, np.int32)
        for p, pr in enumerate(probs):
            sd = pr[k]
            n = cnt[p] = len(sd["keys"])
            if n:
                keys[p, :n] = np.ascontiguousarray(sd["keys"]).view(np.int32).reshape(n, 7)
            desc[p, :n], pts[p, :n], val[p, :n], mat[p, :n] = sd["desc"], sd["points"], sd["valid"], sd["matched"]
        sides.append([torch.from_numpy(a).cuda() for a in (keys, desc, pts, val, mat, cnt)])
    srt = torch.from_numpy(np.stack([pr[2] for pr in probs])).cuda()
    return sides[0], sides[1], srt


def run(ctx, probs, p1, p2, cap, seed=5, th=ss.TH, th_high=ss.TH_HIGH):
    s1, s2, srt = pack(probs, p1, p2, seed)
    P = len(probs)
    i32 = lambda *sh: torch.full(sh, -77, dtype=torch.int32, device="cuda")
    m1, m2, pr, pc, st = i32(P, p1), i32(P, p2), i32(P, max(cap, 1), 4), i32(P), i32(P, 8)
    torch.cuda.synchronize()
    rc = ctx.search_by_sim3_dev(P, K, WIDTH, HEIGHT, NLEVELS, SCALE, tuple(t.data_ptr() for t in s1) + (p1,), tuple(t.data_ptr() for t in s2) + (p2,),
                                srt.data_ptr(), th, th_high, m1.data_ptr(), m2.data_ptr(), pr.data_ptr(), cap, pc.data_ptr(), st.data_ptr())
    assert rc == 0, rc
    ctx.synchronize()
    return [x.cpu().numpy() for x in (m1, m2, pr, pc, st)]


@pytest.fixture(scope="module")
def expected():
    return {sh: [ss.search(a, b, srt, K, WIDTH, HEIGHT, NLEVELS, SCALE) for a, b, srt in problems(*sh)] for sh in SHAPES}


@pytest.mark.parametrize("shape", SHAPES)
def test_equal_to_the_definition(ctx, expected, shape):
    p1, p2 = shape
    probs = problems(p1, p2)
    cap = max(min(p1, p2), 1)
    m1, m2, pr, pc, st = run(ctx, probs, p1, p2, cap)
    found = 0
    for p, (e, (a, b, _)) in enumerate(zip(expected[shape], probs)):
        n1, n2 = len(a["keys"]), len(b["keys"])
        assert np.array_equal(m1[p, :n1], e["match1"]) and (m1[p, n1:] == -1).all(), p
        assert np.array_equal(m2[p, :n2], e["match2"]) and (m2[p, n2:] == -1).all(), p
        assert pc[p] == len(e["pairs"]) and np.array_equal(st[p], e["stats"]), (p, st[p], e["stats"])
        got = np.ascontiguousarray(pr[p, :pc[p]]).view(capi.MATCH).reshape(-1)
        assert got.tobytes() == e["pairs"].tobytes(), p
        found += len(e["pairs"])
    assert [e["stats"][7] for e in expected[shape]] == [0, 0, 0, ss.FLAG_MALFORMED, ss.FLAG_MALFORMED]
    if min(p1, p2) >= 64:      # the batch shows something: pairs are found, and keys are refused for every reason
        assert found >= 10
        why = np.concatenate([w for e in expected[shape] for w in e["why"]])
        assert all((why == r).any() for r in (ss.OK, ss.NOT_TRIED, ss.BEHIND, ss.OUTSIDE, ss.RANGE, ss.NO_CANDIDATE, ss.TOO_FAR))


def test_the_same_bits_alone_in_another_slot_and_again(ctx):
    p1, p2 = 67, 64
    probs = problems(p1, p2)
    cap = 64
    first = run(ctx, probs, p1, p2, cap, seed=5)
    again = run(ctx, probs, p1, p2, cap, seed=6)              # other garbage beyond the counts
    order = [4, 2, 0, 3, 1]
    moved = run(ctx, [probs[k] for k in order], p1, p2, cap, seed=7)
    for p in range(len(probs)):
        alone = run(ctx, [probs[p]], p1, p2, cap, seed=8 + p)
        n = first[3][p]
        for k, name in enumerate(("match1", "match2", "pairs", "pair_counts", "stats")):
            ref = first[k][p][:n] if name == "pairs" else first[k][p]
            cut = (lambda x: x[:n]) if name == "pairs" else (lambda x: x)
            assert np.array_equal(ref, cut(again[k][p])), (p, name)
            assert np.array_equal(ref, cut(moved[k][order.index(p)])), (p, name)
            assert np.array_equal(ref, cut(alone[k][0])), (p, name)


def test_truncation_keeps_the_count_and_null_outputs(ctx, expected):
    p1, p2 = 300, 300
    probs = problems(p1, p2)
    e = expected[(p1, p2)]
    full = run(ctx, probs, p1, p2, 300)
    assert full[3][0] > 3
    cut = run(ctx, probs, p1, p2, 3)
    assert np.array_equal(cut[3], full[3]) and np.array_equal(cut[2][0], full[2][0][:3])
    assert np.array_equal(cut[0], full[0]) and np.array_equal(cut[4], full[4])
    # every output nullable: the stats alone, with the lists in the context's work buffer
    s1, s2, srt = pack(probs, p1, p2, 5)
    st = torch.zeros((len(probs), 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = ctx.search_by_sim3_dev(len(probs), K, WIDTH, HEIGHT, NLEVELS, SCALE, tuple(t.data_ptr() for t in s1) + (p1,),
                                tuple(t.data_ptr() for t in s2) + (p2,), srt.data_ptr(), stats_ptr=st.data_ptr())
    assert rc == 0
    ctx.synchronize()
    assert np.array_equal(st.cpu().numpy(), np.stack([x["stats"] for x in e]))


def test_the_host_form_and_other_thresholds(ctx):
    a, b, srt = make_pair(3, 120, 110)
    for th, th_high in ((ss.TH, ss.TH_HIGH), (3.0, 40), (20.0, 256), (7.5, 0)):
        e = ss.search(a, b, srt, K, WIDTH, HEIGHT, NLEVELS, SCALE, th, th_high)
        g = ctx.search_by_sim3(a, b, srt, K, WIDTH, HEIGHT, NLEVELS, SCALE, th=th, th_high=th_high)
        assert np.array_equal(g["match1"], e["match1"]) and np.array_equal(g["match2"], e["match2"])
        assert g["pairs"].tobytes() == e["pairs"].tobytes() and g["pair_count"] == len(e["pairs"]) and np.array_equal(g["stats"], e["stats"])
    lst = ctx.search_by_sim3([a, b], [b, a], np.stack([srt, srt]), K, WIDTH, HEIGHT, NLEVELS, SCALE)
    assert len(lst) == 2 and np.array_equal(lst[0]["match1"], ss.search(a, b, srt, K, WIDTH, HEIGHT, NLEVELS, SCALE)["match1"])


def test_argument_errors(ctx):
    p1 = p2 = 5
    probs = problems(p1, p2)
    s1, s2, srt = pack(probs, p1, p2, 5)
    a1, a2 = tuple(t.data_ptr() for t in s1), tuple(t.data_ptr() for t in s2)
    st = torch.zeros((len(probs), 8), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def rc(K=K, w=WIDTH, h=HEIGHT, nl=NLEVELS, sc_=SCALE, s1=a1 + (p1,), s2=a2 + (p2,), srt=srt.data_ptr(), th=7.5, th_high=100, **kw):
        return ctx.search_by_sim3_dev(len(probs), K, w, h, nl, sc_, s1, s2, srt, th, th_high, stats_ptr=st.data_ptr(), **kw)

    assert rc() == 0
    bad = [rc(srt=0), rc(s1=(0,) + a1[1:] + (p1,)), rc(s2=a2[:4] + (0, a2[5], p2)), rc(s1=a1 + (0,)), rc(s1=a1 + (8193,)), rc(s2=a2 + (0,)),
           rc(s2=a2 + (8193,)), rc(nl=0), rc(nl=17), rc(th=0.0), rc(th=-1.0), rc(th=float("nan")), rc(th_high=-1), rc(th_high=257), rc(w=0), rc(h=0),
           rc(h=-3), rc(K=(0.0, 360.0, 320.0, 120.0)), rc(sc_=0.0)]
    ctx.synchronize()
    assert bad == [capi.TB_EINVAL] * len(bad)
