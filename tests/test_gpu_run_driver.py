"""The layout of what the gibbs_* wrappers return: for about a dozen runs per burn-in, the ordered list of (key path,
type, dtype, shape, memory order) of the result, walked recursively, against tests/golden/run_schema.json -- recorded on
the device at the commit before the four wrappers were folded into one driver.  Values are not stored here: the rest of
the suite pins them to the oracle and to resident chains.  A run that is refused records the refusal instead.

The shape is that of test_gpu_run_options.py: N = 257 is one full 256-row tile and a one-row tile, P = 33 two plane
words with one live bit in the second.  `python tests/test_gpu_run_driver.py --record [FILE]` rewrites the golden file
from the package as it is: only to be run at a commit whose wrappers are known to be right."""
import json
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bmm_mcmc_amd as bm

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "run_schema.json")
N, P, K, M, NS, SEED = 257, 33, 6, 5, 6, 11
BURNINS = (0, 2)


def _data():
    rng = np.random.default_rng(5)
    theta = 0.1 + 0.8 * rng.random((3, P))
    rows = (rng.random((N + M, P)) < theta[rng.integers(0, 3, N + M)]).astype(np.int32)
    return np.asfortranarray(rows[:N]), np.asfortranarray(rows[N:])


X, XNEW = _data()
MISS = np.zeros((N, P), dtype=bool)
MISS[np.random.default_rng(6).integers(0, N, 20), np.random.default_rng(7).integers(0, P, 20)] = True
KNOWN = np.zeros(N, dtype=np.int64)
KNOWN[:6] = [1, 1, 2, 2, 3, 3]
# everything that goes together: the pair check and missing cells exclude each other, so two sets
TOGETHER = dict(newdata=XNEW, partition="binder", partition_search=True, logpost=True, pair_check=[0, 5, 32], known=KNOWN,
                summary=True)
TOGETHER_NA = dict(TOGETHER, pair_check=None, missing=MISS, newdata_missing=XNEW > 0)


def _run(fn, *args, **kw):
    return lambda burnin: getattr(bm, fn)(X, NS, *args, burnin=burnin, seed=SEED, **kw)


CASES = {
    "collapsed_together": _run("gibbs_collapsed", K, **TOGETHER),
    "dp_together": _run("gibbs_dp", maxK=K, **TOGETHER),
    "stickbreaking_together": _run("gibbs_stickbreaking", K, **TOGETHER),
    "full_together": _run("gibbs_full", K, **TOGETHER),
    "collapsed_together_missing": _run("gibbs_collapsed", K, **TOGETHER_NA),
    "dp_together_missing": _run("gibbs_dp", maxK=K, **TOGETHER_NA),
    "stickbreaking_together_missing": _run("gibbs_stickbreaking", K, **TOGETHER_NA),
    "full_together_missing": _run("gibbs_full", K, **TOGETHER_NA),
    "collapsed_stephens_device": _run("gibbs_collapsed", K, relabel=True, burnrelabel=2, stephens="device", newdata=XNEW,
                                      predictive_trace=True, responsibilities=True, loo=True),
    "full_stephens_device": _run("gibbs_full", K, relabel=True, burnrelabel=2, stephens="device", partition="vi"),
    "dp_stephens_hook": _run("gibbs_dp", maxK=K, relabel=True, burnrelabel=2, stephens=bm.DeviceStephens(0), logpost=True),
    "dp_ecr_iterative": _run("gibbs_dp", maxK=K, relabel="ecr", loo="trace"),
    "full_ecr_partition": _run("gibbs_full", K, relabel="ecr", ecr_pivot="partition", partition="binder", similarity_of=[0, 1, 256]),
    "stickbreaking_ecr_map": _run("gibbs_stickbreaking", K, relabel="ecr", ecr_pivot="map", loo=True),
    "collapsed_temper": _run("gibbs_collapsed", K, temper=2, logpost=True),
    "collapsed_kmodes_features": _run("gibbs_collapsed", K, init="kmodes", select_features=True, loo=False),
    "dp_features": _run("gibbs_dp", maxK=K, select_features=True, rho=0.4),
    "dp_split_merge": _run("gibbs_dp", maxK=K, split_merge=1, newdata=XNEW, newdata_missing=XNEW > 0, responsibilities=True),
    "full_keep_trace_false": _run("gibbs_full", K, summary="counts", summary_pivot=None, keep_trace=False, known=KNOWN),
    "collapsed_chains_2": _run("gibbs_collapsed", K, chains=2, init="kmodes", partition="binder", partition_search=True, logpost=True,
                               relabel="ecr", ecr_pivot="partition"),
    "stickbreaking_chains_2": _run("gibbs_stickbreaking", K, chains=2, relabel="ecr", ecr_pivot="map"),
    "allocation": _run("gibbs_allocation", K, partition="vi", logpost=True, split_merge=1),
}


def _order(a):
    return ("C" if a.flags.c_contiguous else "") + ("F" if a.flags.f_contiguous else "") or "-"


def schema(obj, path=""):
    """the ordered (key path, type, dtype, shape, order) rows of a result"""
    if isinstance(obj, dict):
        rows = [[path, "dict", None, len(obj), None]]
        for k, v in obj.items():
            rows += schema(v, "%s/%s" % (path, k))
        return rows
    if isinstance(obj, (list, tuple)):
        rows = [[path, type(obj).__name__, None, len(obj), None]]
        for i, v in enumerate(obj):
            rows += schema(v, "%s[%d]" % (path, i))
        return rows
    if isinstance(obj, np.ndarray):
        return [[path, "ndarray", str(obj.dtype), list(obj.shape), _order(obj)]]
    if isinstance(obj, np.generic):
        return [[path, type(obj).__name__, str(obj.dtype), [], None]]
    return [[path, type(obj).__name__, None, None, None]]


def outcome(case, burnin):
    try:
        return schema(CASES[case](burnin))
    except (ValueError, NotImplementedError, bm.BmmError) as e:  # refused, by the wrapper or by the library
        return [["", "raised", type(e).__name__, str(e), None]]


@pytest.mark.parametrize("burnin", BURNINS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_result_layout_is_the_recorded_one(case, burnin):
    with open(GOLDEN) as f:
        want = json.load(f)["%s/burnin=%d" % (case, burnin)]  # (a case without a record fails here: KeyError)
    assert json.loads(json.dumps(outcome(case, burnin))) == want


if __name__ == "__main__":
    if sys.argv[1:2] != ["--record"]:
        sys.exit("usage: python tests/test_gpu_run_driver.py --record [FILE]")
    rec = {"%s/burnin=%d" % (c, b): outcome(c, b) for c in sorted(CASES) for b in BURNINS}
    with open(sys.argv[2] if len(sys.argv) > 2 else GOLDEN, "w") as f:
        json.dump(rec, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")
    print("recorded %d results" % len(rec))
