"""
The driver parses ONE JSON line from bench.py's stdout.  Round 4's line had grown to 20 406 bytes and BENCH_r04.json recorded
"parsed": null -- the round's headline was unmeasured.  These tests bound the line: bench.slim_line() is a pure function of the full
result dict, fed here with round 4's full record (profiles/r4_lda_k50_bench.json, 20 KB: four configurations with per-iteration
parity dumps) and with a synthetic multi-GPU record; the GPU test tests/test_bench_torchrun_gpu.py asserts the same on a real line.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (imports no torch at module level)
import numpy as np  # noqa: E402


def _full():
    return json.load(open(os.path.join(ROOT, "profiles", "r4_lda_k50_bench.json")))


def test_slim_line_is_small_and_round_trips():
    full = _full()
    assert len(json.dumps(full)) > 15000                      # the canned record really is the oversized one
    line = bench.slim_line(full)
    assert "\n" not in line and len(line) < bench.LINE_LIMIT <= 6000
    r = json.loads(line)
    # the contract fields
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in r, k
    assert r["config"]["workload"].startswith("LDA K=50") and "model" not in r["config"]
    assert abs(r["value"] - full["value"]) / full["value"] < 1e-6
    rf = r["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-6
    assert rf["algorithmic_bytes"] == full["roofline"]["algorithmic_bytes_per_estep"] and rf["traffic"] and rf["estep_ms"] > 0
    cb = r["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and len(cb["sample"]) <= 90
    assert r["parity"]["pass"] is True and r["parity"]["documents"] == 128804 and "per_iteration" not in r["parity"]
    # the side configurations keep their own roofline / cpu_baseline / parity verdicts
    assert set(r["other_configs"]) == {"lda100", "ctm", "ctpf"}
    for name, o in r["other_configs"].items():
        assert o["roofline"]["frac"] > 0 and o["cpu_baseline"]["value"] > 0 and o["parity"]["pass"] is True, name
        assert "per_iteration" not in o["parity"] and "tolerances" not in o["parity"]
    assert r["other_configs"]["ctm"]["roofline"]["bound"] == "valu"
    assert r["elbo_plateau"]["reached"] is True and "elbo_vs_wallclock" not in r["elbo_plateau"]


def test_slim_line_with_multi_gpu_arrays_and_errors():
    full = _full()
    full["n_gpus"] = 8
    full["multi_gpu_check"] = {"iterations": 5, "globals_hash_equal": True, "globals_hash_per_rank": ["%016x" % i for i in range(8)],
                               "elbo_rel_vs_n1": 3e-8, "elbo_rel_tolerance": 2e-6, "elbo_n": [-1.0e8] * 5, "elbo_n1": [-1.0e8] * 5, "pass": True,
                               "form": "fused", "shard_nnz_max_over_min": 1.001}
    full["other_configs"]["ctm"] = {"error": "RuntimeError: " + "x" * 5000}
    full["cpu_baseline"] = None
    full["parity"] = None
    line = bench.slim_line(full)
    assert len(line) < 6000
    r = json.loads(line)
    assert r["multi_gpu_check"]["pass"] is True and "elbo_n" not in r["multi_gpu_check"] and "globals_hash_per_rank" not in r["multi_gpu_check"]
    assert len(r["other_configs"]["ctm"]["error"]) <= 200 and r["cpu_baseline"] is None


def test_slim_line_sheds_before_it_overflows():
    """whatever the side configurations carry, the printed line stays under the limit (they are shed first, the headline never)"""
    full = _full()
    for o in full["other_configs"].values():
        o["parity"]["worst"] = {f"metric_{i}": 1e-7 * i for i in range(120)}
    line = bench.slim_line(full)
    assert len(line) < 6000
    r = json.loads(line)
    assert r["roofline"]["frac"] > 0 and r["cpu_baseline"]["value"] > 0 and r["parity"]["pass"] is True


def test_non_finite_numbers_do_not_break_json():
    full = _full()
    full["roofline"]["estep_ms"] = float("nan")
    r = json.loads(bench.slim_line(full))                      # strict JSON: NaN would not parse everywhere
    assert r["roofline"]["estep_ms"] is None


class _State:
    """what dump_outputs reads of a gpuLDA: update_host! and the host fields it fills (float64, Fortran order, as lda.py has them)"""

    def __init__(self, K, V, M):
        rng = np.random.default_rng(3)
        self.alpha = rng.uniform(0.1, 2.0, K)
        self.beta = np.asfortranarray(rng.dirichlet(np.ones(V), K))
        self.gamma = np.asfortranarray(rng.uniform(0.5, 9.0, (K, M)))
        self.Elogtheta = np.asfortranarray(-rng.uniform(0.5, 9.0, (K, M)))
        self.hosted = 0

    def update_host(self):
        self.hosted += 1


def test_dump_outputs_writes_the_last_state(tmp_path):
    st = _State(5, 40, 30)
    bench.dump_outputs(str(tmp_path / "out"), st)
    assert st.hosted == 1
    got = {n: np.load(tmp_path / "out" / f"{n}.npy") for n in ("alpha", "beta", "gamma", "Elogtheta")}
    assert got["alpha"].dtype == np.float64 and np.array_equal(got["alpha"], st.alpha)
    for n in ("beta", "gamma", "Elogtheta"):
        assert got[n].dtype == np.float32 and np.array_equal(got[n], getattr(st, n).astype(np.float32)), n
    assert got["gamma"].shape == (5, 30) and got["beta"].shape == (5, 40)


def test_dump_outputs_samples_documents_above_the_limit(tmp_path, monkeypatch):
    """above the limit gamma and Elogtheta keep the same seeded documents in every run, and the whole stays within it"""
    st = _State(4, 10, 1000)
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4 * 8 + 4 * 4 * 10 + 2 * 4 * 4 * 100)      # alpha + beta + 100 documents of gamma and Elogtheta
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), st)
    total = 0
    for n in ("alpha", "beta", "gamma", "Elogtheta"):
        a, b = np.load(tmp_path / "a" / f"{n}.npy"), np.load(tmp_path / "b" / f"{n}.npy")
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= bench.DUMP_LIMIT
    g = np.load(tmp_path / "a" / "gamma.npy")
    assert g.shape == (4, 100)
    cols = [int(np.flatnonzero((st.gamma.astype(np.float32) == g[:, [j]]).all(axis=0))[0]) for j in range(100)]
    assert cols == sorted(set(cols))                             # distinct documents, in document order
    assert np.array_equal(np.load(tmp_path / "a" / "Elogtheta.npy"), st.Elogtheta[:, cols].astype(np.float32))
