"""The host-side arithmetic of the eject / absorb move (ea_move_draws, lgamma_, lbeta_, ea_log_q of bmm_spec.h) in the
stand-alone program tests/alloc/alloc_host.cpp, built with -fsanitize=address,undefined: the run is clean (any report
aborts it, -fno-sanitize-recover=all) and gives the bits of the plain build.  Nothing loaded into Python is sanitized."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_cases as cases  # noqa: E402
import alloc_checks as chk  # noqa: E402


def _record(d):
    """p_E is NaN for an absorb: compared by its bits, which the record carries beside it"""
    return {k: v for k, v in d.items() if k != "pe"}


def test_host_arithmetic_is_clean_under_asan_and_ubsan(tmp_path):
    plain, san = chk.build_host(tmp_path), chk.build_host(tmp_path, sanitize=True)
    assert plain != san
    # the arguments of test_closed_form_log_q_on_the_host_build
    triples = [(e, n1, n2) for e in (0.5, 1.0, 2.5) for n1 in (0, 1, 2, 7, 300, 10 ** 6) for n2 in (0, 1, 5, 299, 10 ** 6)]
    a, b = chk.host_logq(plain, tmp_path, triples), chk.host_logq(san, tmp_path, triples)
    np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
    # the draws of every GPU case's first moves, at every K the case allows: forced ejects and absorbs included
    n = 0
    for case in cases.CASES:
        for K in sorted({1, 2, case.K0, case.maxK - 1, case.maxK}):
            if not 1 <= K <= case.maxK:
                continue
            for move in range(3):
                args = (case.seed, 1, move, K, case.maxK, case.e)
                assert _record(chk.host_draws(plain, tmp_path, *args)) == _record(chk.host_draws(san, tmp_path, *args))
                n += 1
    assert n >= 3 * len(cases.CASES)

