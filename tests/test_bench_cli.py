"""bench.py's options and its --dump-outputs writer, without a GPU: stand-in chains hold what a resident chain
hands back (bmm_chain_get_labels / get_counts / get_alpha / get_params)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("_bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class FakeChain:
    def __init__(self, sampler, N, P, K, seed):
        rng = np.random.default_rng(seed)
        self.sampler, self.N, self.P, self.K = sampler, N, P, K
        self.z = rng.integers(1, K + 1, N).astype(np.int32)
        self.S = rng.integers(0, 100, (K, P)).astype(np.int32)
        self.pi, self.theta = rng.dirichlet(np.ones(K)), np.asfortranarray(rng.random((K, P)))

    def labels(self):
        return self.z.copy()

    def counts(self):
        return np.bincount(self.z - 1, minlength=self.K).astype(np.int32), self.S.copy()

    def alpha(self):
        return 0.75

    def params(self):
        if self.sampler not in ("stickbreaking", "full"):
            raise RuntimeError("only the stick-breaking and full samplers carry pi/theta")
        return self.pi.copy(), self.theta.copy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_help_names_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout


def test_one_chain_is_dumped_whole(tmp_path):
    b = _bench()
    ch = FakeChain("collapsed", 5000, 7, 4, 1)
    b.dump_outputs(str(tmp_path), [ch])
    got = _load(tmp_path)
    assert set(got) == {"labels", "cluster_sizes", "feature_counts", "alpha"}
    assert got["labels"].dtype == np.float32 and np.array_equal(got["labels"], ch.z)
    assert got["cluster_sizes"].dtype == np.float64 and got["cluster_sizes"].sum() == 5000
    assert np.array_equal(got["feature_counts"], ch.S) and got["alpha"].tolist() == [0.75]


def test_several_chains_with_parameters_are_prefixed(tmp_path):
    b = _bench()
    chains = [FakeChain("stickbreaking", 300, 5, 6, s) for s in (1, 2)]
    b.dump_outputs(str(tmp_path), chains, first=2, total=4)
    got = _load(tmp_path)
    assert set(got) == {"chain%d_%s" % (c, n) for c in (2, 3)
                        for n in ("labels", "cluster_sizes", "feature_counts", "alpha", "pi", "theta")}
    assert np.array_equal(got["chain3_theta"], chains[1].theta) and got["chain2_pi"].dtype == np.float64
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())


def test_labels_beyond_the_budget_are_a_fixed_sample(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_LABEL_BYTES", 4 * 1000)
    chains = [FakeChain("collapsed", 10_000, 3, 5, s) for s in (3, 4)]
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), chains)
    a, c = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == set(c) and all(np.array_equal(a[k], c[k]) for k in a)     # the same sample every run
    idx = a["labels_index"].astype(np.int64)
    assert idx.shape == (500,) and np.all(np.diff(idx) > 0) and idx[-1] < 10_000
    for i, ch in enumerate(chains):
        assert np.array_equal(a["chain%d_labels" % i], ch.z[idx])


def test_a_full_size_dump_stays_within_64_mb(tmp_path):
    b = _bench()
    chains = [FakeChain("collapsed", 10_000_000, 100, 20, 5)]               # C5's shape
    b.dump_outputs(str(tmp_path), chains)
    total = sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path))
    assert total <= 64 << 20
    assert "labels_index" not in _load(tmp_path)                            # 40 MB of labels: kept whole
