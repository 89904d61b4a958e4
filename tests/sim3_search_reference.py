"""The definition of tb_search_by_sim3_batch_dev (include/tb_capi.h) in numpy: ORB-SLAM's ORBmatcher::SearchBySim3, statement for
statement as the kernel computes it. Float64 from the float32 inputs, one rounding a statement, only + - * / sqrt.

A side is a dict(keys = KEYPOINT records [n], desc uint8 [n][32], points float32 [n][3] IN THE SIDE'S OWN CAMERA FRAME, valid [n],
matched [n]). srt = (w x y z, t, s): X1 = s R X2 + t, the quaternion taken as it is given (sim3_reference.rotation).

    level table g[l] = tb_scale_factors(nlevels, scale)'s inv_sf: the size of a level-l pixel in level-0 pixels (1.25^l at 0.8)
    1 -> 2    a key i of side 1 that is valid and not matched is TRIED: P = R' (X1 - t) / s; P.z > 0; u = fx (P.x / P.z) + cx, v;
              0 <= u < width, 0 <= v < height; maxD = |X1| g[octave], minD = maxD / g[nlevels - 1]; d = s |P|;
              0.8 minD <= d <= 1.2 maxD; L = the smallest l with g[l] d >= maxD, else nlevels - 1; r = th g[L]; it has then REACHED
              THE SEARCH: candidates j of side 2 with |x_j - u| < r, |y_j - v| < r, octave L - 1 or L; best = min (hamming << 32 | j);
              match1[i] = j if the distance <= th_high else -1
    2 -> 1    P = s (R X2) + t, d = |P| / s, the sides exchanged
    agreement (i, j) where match1[i] = j and match2[j] = i, ascending i

search() also returns why[k][i], the reason a key of side k did not get a match (or OK), for the tests that ask that every
reason occurs, level[k][i], the predicted level of a point that reached the search, and geom[k][i] = (maxD, d) of such a point."""
import numpy as np

import oracle
import sim3_reference as sr

F32 = np.float32
F64 = np.float64
TH, TH_HIGH = 7.5, 100
FLAG_MALFORMED, FLAG_SKIPPED = 1, 2
# why
OK, NOT_TRIED, BEHIND, OUTSIDE, RANGE, NO_CANDIDATE, TOO_FAR = range(7)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def level_px(nlevels, scale):
    return np.asarray(oracle.scale_factors(nlevels, scale)[1], F32)


def hamming(a, B):
    """a uint8 [32], B uint8 [m][32] -> int64 [m]"""
    return _POP[np.bitwise_xor(np.asarray(B, np.uint8).reshape(-1, 32), np.asarray(a, np.uint8).reshape(1, 32))].sum(1)


def _norm(X, Y, Z):
    n = X * X
    n = n + Y * Y
    n = n + Z * Z
    return np.sqrt(n)


def direction(src, dst, srt, K, width, height, g, th, th_high, forward):
    """one direction: forward = 1 -> 2 (src = side 1). -> (match [n_src] int32, why [n_src], level [n_src], geom [n_src][2] = maxD
    and d of a point that reached the search, NaN elsewhere)"""
    n = len(src["keys"])
    match, why, level = np.full(n, -1, np.int32), np.full(n, NOT_TRIED, np.int32), np.full(n, -1, np.int32)
    geom = np.full((n, 2), np.nan)
    srt = np.asarray(srt, F64)
    q, t, s = srt[:4], srt[4:7], srt[7]
    R = sr.rotation([F64(v) for v in q])
    fx, fy, cx, cy = (F64(k) for k in K)
    g = np.asarray(g, F32).astype(F64)
    nl = len(g)
    th = F64(F32(th))
    kx, ky = dst["keys"]["x"].astype(F64), dst["keys"]["y"].astype(F64)
    ko = dst["keys"]["octave"].astype(np.int64)
    idx = np.arange(len(ko), dtype=np.int64)
    with np.errstate(all="ignore"):
        for i in range(n):
            if not src["valid"][i] or src["matched"][i]:
                continue
            X, Y, Z = (F64(c) for c in np.asarray(src["points"][i], F32))
            P = []
            if forward:
                d0, d1, d2 = X - t[0], Y - t[1], Z - t[2]
                for k in range(3):
                    a = R[0][k] * d0
                    a = a + R[1][k] * d1
                    a = a + R[2][k] * d2
                    P.append(a / s)
            else:
                for k in range(3):
                    a = R[k][0] * X
                    a = a + R[k][1] * Y
                    a = a + R[k][2] * Z
                    a = s * a
                    P.append(a + t[k])
            if not P[2] > 0.0:
                why[i] = BEHIND
                continue
            u = P[0] / P[2]
            u = fx * u
            u = u + cx
            v = P[1] / P[2]
            v = fy * v
            v = v + cy
            if not (u >= 0.0 and u < F64(width) and v >= 0.0 and v < F64(height)):
                why[i] = OUTSIDE
                continue
            octv = min(max(int(src["keys"]["octave"][i]), 0), nl - 1)
            maxD = _norm(X, Y, Z) * g[octv]
            minD = maxD / g[nl - 1]
            nP = _norm(P[0], P[1], P[2])
            d = s * nP if forward else nP / s
            lo = F64(0.8) * minD
            hi = F64(1.2) * maxD
            if not (d >= lo and d <= hi):
                why[i] = RANGE
                continue
            L = nl - 1
            for l in range(nl - 2, -1, -1):
                if g[l] * d >= maxD:
                    L = l
            level[i] = L
            geom[i] = (maxD, d)
            r = th * g[L]
            cand = ((ko == L) | (ko == L - 1)) & (np.abs(kx - u) < r) & (np.abs(ky - v) < r)
            if not cand.any():
                why[i] = NO_CANDIDATE
                continue
            packed = (hamming(src["desc"][i], dst["desc"][cand]) << 32) | idx[cand]
            best = int(packed.min())
            if (best >> 32) <= th_high:
                match[i] = best & 0xFFFFFFFF
                why[i] = OK
            else:
                why[i] = TOO_FAR
    return match, why, level, geom


def malformed(side1, side2, srt, nlevels):
    s = F64(np.asarray(srt, F64)[7])
    if not (s > 0.0) or not np.isfinite(s):
        return True
    return any(len(sd["keys"]) and ((sd["keys"]["octave"] < 0) | (sd["keys"]["octave"] >= nlevels)).any() for sd in (side1, side2))


def search(side1, side2, srt, K, width, height, nlevels, scale, th=TH, th_high=TH_HIGH):
    """-> dict(match1, match2, pairs = MATCH records in ascending i, stats [8] int32, why = (why1, why2), level = (level1, level2),
    geom = (geom1, geom2))"""
    n1, n2 = len(side1["keys"]), len(side2["keys"])
    if malformed(side1, side2, srt, nlevels):
        st = np.zeros(8, np.int32)
        st[7] = FLAG_MALFORMED
        return dict(match1=np.full(n1, -1, np.int32), match2=np.full(n2, -1, np.int32), pairs=np.zeros(0, oracle.MATCH), stats=st,
                    why=(np.full(n1, NOT_TRIED, np.int32), np.full(n2, NOT_TRIED, np.int32)),
                    level=(np.full(n1, -1, np.int32), np.full(n2, -1, np.int32)), geom=(np.full((n1, 2), np.nan), np.full((n2, 2), np.nan)))
    g = level_px(nlevels, scale)
    m1, w1, l1, g1 = direction(side1, side2, srt, K, width, height, g, th, th_high, True)
    m2, w2, l2, g2 = direction(side2, side1, srt, K, width, height, g, th, th_high, False)
    sel = [i for i in range(n1) if m1[i] >= 0 and m2[m1[i]] == i]
    pairs = np.zeros(len(sel), oracle.MATCH)
    for k, i in enumerate(sel):
        j = int(m1[i])
        pairs[k] = (i, j, -1, F32(hamming(side1["desc"][i], side2["desc"][j:j + 1])[0]))
    reached = lambda w: int(np.isin(w, (OK, NO_CANDIDATE, TOO_FAR)).sum())
    st = np.array([(w1 != NOT_TRIED).sum(), reached(w1), (w2 != NOT_TRIED).sum(), reached(w2), (m1 >= 0).sum(), (m2 >= 0).sum(), len(sel), 0],
                  np.int32)
    return dict(match1=m1, match2=m2, pairs=pairs, stats=st, why=(w1, w2), level=(l1, l2), geom=(g1, g2))


def side(keys, desc, points, valid, matched=None):
    n = len(keys)
    return dict(keys=keys, desc=np.asarray(desc, np.uint8).reshape(n, 32), points=np.asarray(points, F32).reshape(n, 3),
                valid=np.asarray(valid).astype(bool).reshape(n),
                matched=np.zeros(n, bool) if matched is None else np.asarray(matched).astype(bool).reshape(n))
