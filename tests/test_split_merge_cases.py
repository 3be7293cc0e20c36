"""The cases of tests/split_merge_cases.py reach what they are for: the restatement alone, on the CPU, from the labels
the oracle's DP chain leaves (or the planted ones), with the device's own Philox streams."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import split_merge_cases as cases  # noqa: E402


@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_the_restatement_reaches_what_the_case_is_for(oracle, case):
    X = cases.data(case)
    z1 = cases.start_labels(case, X, oracle)
    assert z1.min() >= 1 and z1.max() <= case.K
    seen = cases.restated(case, X, z1)
    assert len(seen) == cases.steps_of(case)
    cases.check_reached(case, seen)
    if case.name == "scans-changing":
        assert [s for s, _ in case.phases] == [2, 6, 1]  # the sets grow, then a smaller scans inside the larger allocation
    if case.name == "wide-K":
        free = np.flatnonzero(np.bincount(z1 - 1, minlength=case.K) == 0)
        assert free[0] >= 256  # past the first trip of the strided search
