#!/usr/bin/env python3
"""Writes tests/golden/ref_dbow2_v1.npz: the outputs of the reference's own DBoW2 (oracle/_ref/ref_dbow2, built by
`make -C oracle ref_dbow2` where the reference's sources exist) for the recorded subset of tests/ref_dbow2_cases.py. The
inputs are seeded and rebuilt by the tests, so only outputs are stored: arrays named <mode>/<case>/<key>.
tests/test_ref_dbow2.py::test_fixture_equals_the_live_driver checks the file against the driver wherever the driver exists."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import ref_dbow2_cases as cases  # noqa: E402
from oracle import ref_dbow2  # noqa: E402


def main():
    if not ref_dbow2.available():
        sys.exit(ref_dbow2.SKIP_REASON)
    arrays = {}
    for (mode, name), rec in cases.all_cases().items():
        if rec:
            for k, v in cases.to_record(mode, cases.live(mode, name)).items():
                arrays["%s/%s/%s" % (mode, name, k)] = v
    np.savez_compressed(cases.GOLDEN, **arrays)
    print("%s: %d arrays, %d bytes" % (cases.GOLDEN, len(arrays), os.path.getsize(cases.GOLDEN)))


if __name__ == "__main__":
    main()
