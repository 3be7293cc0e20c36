"""The host-side arithmetic of the allocation sampler's split-merge move (as_move_draws, as_log_prior of bmm_spec.h) in
the stand-alone program tests/alloc_split/alloc_split_host.cpp, built plain and with -fsanitize=address,undefined: the
run over the arguments of every GPU case is clean (any report aborts it, -fno-sanitize-recover=all) and gives the bits
of the plain build.  Nothing loaded into Python is sanitized."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import alloc_split_cases as cases  # noqa: E402
import alloc_split_checks as chk  # noqa: E402
import alloc_split_ref as ref  # noqa: E402
import split_merge_checks as smchk  # noqa: E402


def test_host_arithmetic_is_clean_under_asan_and_ubsan_and_restated(tmp_path):
    plain, san = chk.build_host(tmp_path), chk.build_host(tmp_path, sanitize=True)
    assert plain != san
    n = 0
    for case in cases.CASES:
        seen = cases.restated_steps(case)
        lp = cases.log_prior_of(case)
        # the draws of every move of the case, and the restated integer parts against them
        keys = [(case.seed, 1, m, case.N) for m in range(case.steps)]
        a, b = chk.host_draws(plain, tmp_path, keys), chk.host_draws(san, tmp_path, keys)
        assert a == b
        for m, (i, j, ub, salt) in enumerate(a):
            dr = ref.PhiloxDraws(case.seed, 1, m)
            assert dr.pair(case.N) == (i, j) and dr.salt == salt and seen[m]["rows"] == (i, j)
            u = float(np.array([ub], dtype=np.uint64).view(np.float64)[0])
            assert abs(dr.log_u() - math.log(u)) <= 1e-12
        # the prior of every move that got as far as a ratio
        args = [r["prior_args"] for r in seen if r["kind"] != ref.SKIPPED]
        if not args:
            continue
        pa, pb = chk.host_prior(plain, tmp_path, args, case.a, lp), chk.host_prior(san, tmp_path, args, case.a, lp)
        np.testing.assert_array_equal(pa, pb)
        want = np.array([r["log_prior"] for r in seen if r["kind"] != ref.SKIPPED])
        # eleven lgamma_ terms of magnitude up to lgamma(K a + N), two logs, twelve additions
        mag = 8.0 * abs(math.lgamma(case.maxK * case.a + case.N) + 1.0) + float(np.max(np.abs(lp))) * 2.0 + 8.0
        bound = 2.0 * (smchk.LGAMMA_ULPS + 12) * smchk.EPS * mag
        assert np.max(np.abs(pa.view(np.float64) - want)) <= bound, (case.name, np.max(np.abs(pa.view(np.float64) - want)), bound)
        n += len(args)
    assert n >= 100
