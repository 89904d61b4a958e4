"""Python restatement of DBoW2's scoring objects (third_part/DBoW2/DBoW2/ScoringObject.cpp:23-311, reached through
TemplatedVocabulary::score, TemplatedVocabulary.h:156-162 and :1199-1203) in sequential float64, and of the keyframe database's
rule (include/tb_capi.h, tb_bow_db_*): the yardstick of tests/test_bow_score_reference.py (tb_bow_score on the host) and of the
GPU tests of tb_bow_score_batch_dev, tb_bow_db_* and the VO loop's database.

A vector is a pair (words ascending int array, values float64 array): the std::map's order. The walk is the reference's: two
cursors, one term per common word added into one accumulator in word order, std::map::lower_bound to skip, a closing formula.
Python floats are IEEE doubles and every operator is one rounding, math.sqrt is correctly rounded, so codes 0, 1, 2, 4, 5 are
exact restatements. KL's math.log is the C library's, which a device library's log need not equal bit for bit; kl_bound gives
the derived tolerance.

Pinned to genuine DBoW2: tests/test_ref_dbow2_score.py holds score() and the host form tb_bow_score equal to the reference's own
TemplatedVocabulary::score (oracle/ref_dbow2.py's score command, recorded in tests/golden/ref_dbow2_score_v1.npz) on the cases of
tests/ref_dbow2_score_cases.py: bit for bit under codes 0, 1, 2, 4, 5 and, on the machine that recorded the fixture, under KL too
(both sides call the same C library's log); tests/test_gpu_ref_dbow2_score.py holds the device to the same recorded results,
KL within kl_bound. Not pinned, because the vendored DBoW2 has no database class: the Ring's rule (which slots are ranked, better
first, ties to the lower kf_id) is the project's own.

Scoring codes (include/tb_types.h): 0 L1_NORM, 1 L2_NORM, 2 CHI_SQUARE, 3 KL, 4 BHATTACHARYYA, 5 DOT_PRODUCT."""
import bisect
import math
import sys

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
LOG_EPS = math.log(sys.float_info.epsilon)      # GeneralScoring::LOG_EPS = log(DBL_EPSILON), :18


def _log(x):
    """the C library's log on a double, with its values at 0 and below (math.log raises there)"""
    if x != x:
        return x
    if x == 0:
        return -math.inf
    if x < 0:
        return math.nan
    return math.log(x)


# Every branch of the six scoring functions and both sides of every guard, as (scoring, name): what score_detail's `branches`
# argument can count. common / v1 behind / v2 behind are the three arms of the walk; "* ends first" how the walk's loop ended.
_WALK = ("common", "v1 behind", "v2 behind", "v1 ends first", "v2 ends first", "both end")
BRANCHES = {(s, b) for s in range(6) for b in _WALK}
BRANCHES |= {(L2_NORM, "sum = 1"), (L2_NORM, "sum > 1"), (L2_NORM, "sum < 1"),
             (CHI_SQUARE, "vi + wi != 0"), (CHI_SQUARE, "vi + wi == 0"),
             (KL, "common added"), (KL, "common vi == 0"), (KL, "common wi == 0"),
             (KL, ":204 vi != 0"), (KL, ":204 vi == 0"), (KL, "tail added"), (KL, "tail zero"), (KL, "no tail"),
             (BHATTACHARYYA, "product >= 0"), (BHATTACHARYYA, "product < 0")}


def score_detail(scoring, a_words, a_values, b_words, b_values, branches=None):
    """-> (score, A, n, M). v1 = a, v2 = b. For KL: A = sum of |vi| * (|log argument's log| + |LOG_EPS|) over the added terms,
    n = the number of added terms, M = max |partial sum| (kl_bound's inputs); 0 for the other scorings. branches: an optional
    set that receives the members of BRANCHES this call took (test-side coverage; no result depends on it)."""
    took = (lambda name: None) if branches is None else (lambda name: branches.add((scoring, name)))
    aw = [int(w) for w in a_words]; av = [float(v) for v in a_values]
    bw = [int(w) for w in b_words]; bv = [float(v) for v in b_values]
    assert len(aw) == len(av) and len(bw) == len(bv)
    assert all(x < y for x, y in zip(aw, aw[1:])) and all(x < y for x, y in zip(bw, bw[1:])), "words must ascend strictly"
    na, nb = len(aw), len(bw)
    i = j = 0
    score = 0.0
    A, n, M = 0.0, 0, 0.0

    def kl_add(vi, arg, eps):
        nonlocal score, A, n, M
        lg = _log(arg)
        score += vi * (lg - LOG_EPS) if eps else vi * lg
        A += abs(vi) * (abs(lg) + abs(LOG_EPS))
        n += 1
        M = max(M, abs(score))

    while i < na and j < nb:
        vi, wi = av[i], bv[j]
        if aw[i] == bw[j]:
            took("common")
            if scoring == L1_NORM:
                score += abs(vi - wi) - abs(vi) - abs(wi)              # :41
            elif scoring in (L2_NORM, DOT_PRODUCT):
                score += vi * wi                                       # :91, :290
            elif scoring == CHI_SQUARE:
                took("vi + wi != 0" if vi + wi != 0.0 else "vi + wi == 0")
                if vi + wi != 0.0:
                    score += vi * wi / (vi + wi)                       # :148
            elif scoring == KL:
                took("common added" if vi != 0 and wi != 0 else "common vi == 0" if not vi != 0 else "common wi == 0")
                if vi != 0 and wi != 0:
                    kl_add(vi, vi / wi, False)                         # :195
            else:
                p = vi * wi
                took("product >= 0" if p >= 0 else "product < 0")
                score += math.sqrt(p) if p >= 0 else math.nan          # :245
            i += 1; j += 1
        elif aw[i] < bw[j]:
            took("v1 behind")
            if scoring == KL:
                took(":204 vi != 0" if vi != 0 else ":204 vi == 0")
                kl_add(vi, vi, True)                                   # :204, then ++v1_it
                i += 1
            else:
                i = bisect.bisect_left(aw, bw[j], i)                   # v1.lower_bound(v2_it->first)
        else:
            took("v2 behind")
            j = bisect.bisect_left(bw, aw[i], j)                       # v2.lower_bound(v1_it->first)
    took("both end" if i >= na and j >= nb else "v1 ends first" if i >= na else "v2 ends first")
    if scoring == L1_NORM:
        score = -score / 2.0                                           # :65
    elif scoring == L2_NORM:
        took("sum = 1" if score == 1 else "sum > 1" if score > 1 else "sum < 1")
        score = 1.0 if score >= 1 else 1.0 - math.sqrt(1.0 - score)    # :114-117
    elif scoring == CHI_SQUARE:
        score = 2. * score                                             # :167
    elif scoring == KL:
        if i >= na:
            took("no tail")
        while i < na:                                                  # :216-218
            took("tail added" if av[i] != 0 else "tail zero")
            if av[i] != 0:
                kl_add(av[i], av[i], True)
            i += 1
    return score, A, n, M


def score(scoring, a_words, a_values, b_words, b_values):
    return score_detail(scoring, a_words, a_values, b_words, b_values)[0]


def kl_bound(A, n, M):
    """|device KL - this KL| <= 2^-52 (8 A + n M). Each log is within 1 ulp of the true value on both sides, so two logs of one
    argument differ by at most 2 ulp <= 2^-51 |log|; the term vi * (log - LOG_EPS) or vi * log then takes at most two more
    roundings on each side (2^-53 relative each, on a magnitude of at most |vi| (|log| + |LOG_EPS|)), and a quotient vi / wi that
    is the same double on both sides. Per term that is below 2^-52 * 8 * |vi| (|log| + |LOG_EPS|), summed: 2^-52 * 8 A. The sums run
    in the same order; each of the n adds rounds a partial sum of magnitude at most M (and the other side's, which differs from it
    by less than the bound itself): 2^-52 n M covers both."""
    return 2.0 ** -52 * (8.0 * A + n * M)


def same(scoring, got, exp_detail):
    """the comparison rule: 64-bit patterns for codes 0, 1, 2, 4, 5; the derived bound for KL. A NaN equals a NaN: its sign and
    payload are the processor's choice (x86's sqrt of a negative returns the negative default NaN), not arithmetic."""
    exp, A, n, M = exp_detail
    if got != got and exp != exp:
        return True
    if scoring != KL:
        return np.float64(got).view(np.uint64) == np.float64(exp).view(np.uint64)
    if exp != exp or math.isinf(exp):
        return got == exp
    return abs(got - exp) <= kl_bound(A, n, M)


class Ring:
    """The keyframe database of one sequence: add number a goes to slot a % capacity and overwrites the oldest."""

    def __init__(self, capacity, scoring):
        self.capacity, self.scoring = capacity, scoring
        self.slots = [None] * capacity          # (words, values)
        self.kf_ids = [-1] * capacity
        self.nadded = 0

    def clear(self):
        self.__init__(self.capacity, self.scoring)

    def add(self, words, values, kf_id):
        s = self.nadded % self.capacity
        self.slots[s] = (np.array(words, np.int32), np.array(values, np.float64))
        self.kf_ids[s] = int(kf_id)
        self.nadded += 1

    def ranked_slots(self, exclude_newest):
        """slots that hold a vector and are not among the exclude_newest most recent adds"""
        out = []
        for s in range(self.capacity):
            if self.slots[s] is None:
                continue
            age = (self.nadded - 1 - s) % self.capacity       # 0 = the last add
            if age >= exclude_newest:
                out.append(s)
        return out

    def query(self, q_words, q_values, topk, exclude_newest):
        """-> (details per slot: score_detail tuples, None where the slot is not ranked; top_slot, top_kf [topk] with -1 in the
        unused tail; top_count). The query is v1. Better first: descending score, ascending for KL; ties to the lower kf_id."""
        ranked = self.ranked_slots(exclude_newest)
        det = [None] * self.capacity
        for s in ranked:
            det[s] = score_detail(self.scoring, q_words, q_values, *self.slots[s])
        sign = 1.0 if self.scoring == KL else -1.0
        order = sorted(ranked, key=lambda s: (sign * det[s][0], self.kf_ids[s], s))
        top = order[:topk]
        pad = [-1] * (topk - len(top))
        return det, top + pad, [self.kf_ids[s] for s in top] + pad, len(top)
