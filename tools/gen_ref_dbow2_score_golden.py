#!/usr/bin/env python3
"""Writes tests/golden/ref_dbow2_score_v1.npz: the results of the reference's own TemplatedVocabulary::score
(oracle/_ref/ref_dbow2 score, built by `make -C oracle ref_dbow2` where the reference's sources exist) for every case of
tests/ref_dbow2_score_cases.py, as bit patterns: score/<case>/bits uint64 [6 scoring codes, pairs], a digest of the case's inputs,
and for the order-of-sum case the values themselves. The inputs are seeded and rebuilt by the tests.
tests/test_ref_dbow2_score.py::test_fixture_equals_the_live_driver checks the file against the driver wherever the driver exists."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ref_dbow2_score_cases as cases  # noqa: E402
from oracle import ref_dbow2  # noqa: E402


def main():
    if not ref_dbow2.score_available():
        sys.exit(ref_dbow2.SCORE_SKIP_REASON)
    arrays, npairs = {}, 0
    for name in cases.NAMES:
        inp = cases.fresh_inputs(name)
        bits = cases.live(name, inp)
        npairs += bits.size
        for k, v in cases.to_record(name, bits, inp).items():
            arrays["score/%s/%s" % (name, k)] = v
    np.savez_compressed(cases.GOLDEN, **arrays)
    print("%s: %d cases, %d scored pairs, %d bytes" % (cases.GOLDEN, len(cases.NAMES), npairs, os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
