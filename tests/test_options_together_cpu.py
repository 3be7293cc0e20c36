"""The table behind tests/test_gpu_options_together.py, checked without a device: every keyword of the five wrappers
and of bm.run_options is classified (a new option cannot be added without entering the matrix), split() takes every
case's keywords apart and puts them back, every group of a case names keywords its wrapper takes, and diff_leaves sees
each kind of difference it is there to see and names where it is."""
import copy
import inspect

import numpy as np
import pytest

import bmm_mcmc_amd as bm
import options_together as OT


def test_every_keyword_is_classified_and_nothing_classified_is_gone():
    names = OT.signature_names()
    assert sorted(names - set(OT.KINDS)) == [], "a keyword outside the matrix: classify it in tests/options_together.py"
    assert sorted(set(OT.KINDS) - names) == [], "classified, but no wrapper takes it"
    assert set(bm._RUN_OPTIONS) <= set(OT.KINDS)
    assert len(OT.CHAIN) + len(OT.OBSERVERS) + len(OT.MODIFIERS) + len(OT.SHAPE) == len(OT.KINDS)  # one kind each
    assert set(OT.KINDS.values()) == {"chain", "observer", "modifier", "shape"}
    for m, owner in OT.MODIFIERS.items():
        assert owner in OT.OBSERVERS, m
        for w in OT.WRAPPERS:  # a modifier is offered wherever its observer is, and nowhere else
            if m in inspect.signature(getattr(bm, w)).parameters:
                assert OT.wrapper_takes(w, owner), (w, m)
    assert set(OT.RESULT_KEYS) == set(OT.OBSERVERS)


def test_the_layout_cases_are_all_here_under_their_names():
    import ast
    import os
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_run_driver.py")).read()
    table = next(n for n in ast.parse(src).body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) == "CASES")
    assert [k.value for k in table.value.keys] == list(OT.DRIVER_CASES)
    for key, node in zip(table.value.keys, table.value.values):  # _run("gibbs_x", [K], kw=...): the same wrapper, the same keywords
        case = OT.CASES[key.value]
        assert node.args[0].value == case.wrapper
        named = sorted(k.arg for k in node.keywords if k.arg is not None and k.arg != "maxK")
        starred = [k.value.id for k in node.keywords if k.arg is None]
        want = sorted(case.kwargs)
        for s in starred:
            named = sorted(named + list(getattr(OT, s)))
        assert named == want, key.value


@pytest.mark.parametrize("name", list(OT.CASES))
def test_split_reassembles_the_keywords_of_every_case(name):
    case = OT.CASES[name]
    base, groups = OT.split(case.kwargs)
    merged = dict(base)
    for g in groups:
        assert not set(g) & set(merged)  # a keyword sits in one place
        merged.update(g)
    assert set(merged) == set(case.kwargs) and all(merged[k] is case.kwargs[k] for k in merged)
    assert all(OT.KINDS[k] in ("chain", "shape") or not OT._on(v) or OT.MODIFIERS.get(k) is not None for k, v in base.items())
    for g in groups:
        assert any(OT.KINDS[k] == "observer" for k in g) and OT.group_keys(g)
        for k in g:
            assert OT.wrapper_takes(case.wrapper, k), (name, k)
    for k in base:
        assert OT.wrapper_takes(case.wrapper, k), (name, k)
    assert set(case.refusals) <= set(case.burnins)


def test_the_shapes_are_the_ones_the_cases_are_there_for():
    assert OT.X.shape == (257, 33) and OT.XNEW.shape == (5, 33) and OT.XG.shape == (257, 130) and OT.XGNEW.shape == (5, 130)
    assert OT.X[:, 32].any() and not OT.X[:, 32].all()  # the live bit of the second plane word
    # 130 features are past the table kernels (128): the masked scorer of new rows says which side a shape is on
    for sampler in ("collapsed", "dp"):
        assert bm.predict_na_plan(sampler, OT.K, OT.P)["form"] == "lds"
        assert bm.predict_na_plan(sampler, OT.K, OT.P_GENERIC)["form"] == "global"
    assert OT.CASES["generic_dp"].data == OT.CASES["generic_collapsed"].data == "generic"
    assert 0 < OT.MISS.sum() <= 20 and (OT.XNEW > 0).any() and (OT.KNOWN > 0).sum() == 6
    for name in ("strides_collapsed", "strides_full"):  # every stride folds at least two sweeps, at either burn-in
        case = OT.CASES[name]
        for b in case.burnins:
            S, first = case.nsamples - b, 0 if b else 1
            for key in ("partition_stride", "pair_check_stride", "summary_stride"):
                assert case.kwargs[key] > 1 and len([s for s in range(S) if s >= first and s % case.kwargs[key] == 0]) >= 2
        assert len({case.kwargs[k] for k in ("partition_stride", "pair_check_stride")}) == 2


def test_what_travels_together():
    base, groups = OT.split(dict(known=OT.KNOWN, partition="vi", partition_search=True, credible_ball=True, logpost=True,
                                 relabel="ecr", ecr_pivot="partition", loo=False, pair_check_stride=2))
    assert list(base) == ["known", "loo", "pair_check_stride"]  # off, and a modifier without its observer: they arm nothing
    assert [sorted(g) for g in groups] == [["credible_ball", "ecr_pivot", "partition", "partition_search", "relabel"], ["logpost"]]
    assert OT.group_keys(groups[0]) == ["partition", "permutations", "z", "theta", "z_original", "theta_original", "ecr"]
    _, groups = OT.split(dict(relabel="ecr", ecr_pivot="map", logpost=True, summary=True, keep_trace=False))
    assert [sorted(g) for g in groups] == [["ecr_pivot", "logpost", "relabel"], ["keep_trace", "summary"]]
    _, groups = OT.split(dict(relabel="ecr", ecr_pivot="map"))
    assert OT.group_keys(groups[0])[-1] == "logpost"  # implied
    _, groups = OT.split(dict(relabel=True, stephens="device", burnrelabel=2))
    assert "ecr" not in OT.group_keys(groups[0])
    with pytest.raises(ValueError):
        OT.split(dict(credible_ball=True))
    with pytest.raises(KeyError):
        OT.split(dict(partition="vi", no_such_option=1))


def _result():
    return {"z": np.arange(12, dtype=np.int32).reshape(3, 4), "theta": np.full((2, 2), 0.25),
            "partition": {"loss": np.array([1.5, np.nan]), "best": 1, "search": {"z": np.ones(4, dtype=np.int32), "moved": [3, 0],
                                                                                   "loss": 0.5}},
            "summary": {"pivot": None, "n_folded": np.int32(4)}, "list": [{"a": np.zeros(2)}, {"a": np.zeros(2)}]}


def test_diff_leaves_finds_each_kind_of_difference_and_names_it():
    a = _result()
    assert OT.diff_leaves(a, _result()) == [] and OT.diff_leaves(a, copy.deepcopy(a)) == []
    b = _result()
    b["theta"].view(np.uint64)[1, 0] ^= 1                                   # one mantissa bit, in a nested array
    b["list"][1]["a"].view(np.uint64)[1] ^= 1
    assert OT.diff_leaves(b, a) == ["/theta", "/list[1]/a"] and np.allclose(b["theta"], a["theta"], rtol=1e-15, atol=0)
    b = _result()
    b["partition"]["loss"].view(np.uint64)[1] ^= 1                          # a NaN with another payload
    assert np.isnan(b["partition"]["loss"][1]) and OT.diff_leaves(b, a) == ["/partition/loss"]
    b = _result()
    b["theta"][0, 0] = -0.0
    c = _result()
    c["theta"][0, 0] = 0.0
    assert OT.diff_leaves(b, c) == ["/theta"]
    b = _result()
    b["z"] = b["z"].astype(np.int64)                                        # a dtype
    b["summary"]["n_folded"] = 4
    assert OT.diff_leaves(b, a) == ["/z", "/summary/n_folded"]
    b = _result()
    b["z"] = b["z"].reshape(4, 3)                                           # a shape, the same bytes
    assert OT.diff_leaves(b, a) == ["/z"]
    b = _result()
    b["partition"] = {k: b["partition"][k] for k in ("best", "loss", "search")}  # a key moved
    assert OT.diff_leaves(b, a) == ["/partition{keys}"]
    b = _result()
    del b["partition"]["search"]["moved"]                                   # a key missing, on either side
    assert OT.diff_leaves(b, a) == ["/partition/search{keys}"] == OT.diff_leaves(a, b)
    b = _result()
    b["summary"]["pivot"] = np.zeros(4, dtype=np.int32)                     # None against an array
    assert OT.diff_leaves(b, a) == ["/summary/pivot"] == OT.diff_leaves(a, b)
    b = _result()
    b["partition"]["search"]["moved"] = [3, 0, 0]                           # a longer list; a list against a tuple
    assert OT.diff_leaves(b, a) == ["/partition/search/moved[len]"]
    b["partition"]["search"]["moved"] = (3, 0)
    assert OT.diff_leaves(b, a) == ["/partition/search/moved"]
    b = _result()
    b["partition"]["best"] = True                                           # True is not 1
    b["partition"]["search"]["loss"] = np.float64(0.5)                      # a NumPy scalar is not a float
    assert OT.diff_leaves(b, a) == ["/partition/best", "/partition/search/loss"]
    big = np.array([1 << 70, 3], dtype=object)                              # exact totals held as Python integers
    assert OT.diff_leaves({"b": big}, {"b": big.copy()}) == []
    assert OT.diff_leaves({"b": big}, {"b": np.array([(1 << 70) + 1, 3], dtype=object)}) == ["/b"]


def test_pick_keeps_the_order_of_the_result():
    assert list(OT.pick({"z": 1, "loo": 2, "partition": 3}, ("partition", "z"))) == ["z", "partition"]
