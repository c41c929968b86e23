"""bench.py's options and its --dump-outputs writer (host side: no GPU needed)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_options():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and a.full is False and a.dump_outputs == ""
    a = bench.parse_args(["--full", "--dump-outputs", "out"])
    assert a.full is True and a.dump_outputs == "out"


def _lists(nq, k, seed=3):
    rng = np.random.default_rng(seed)
    return {"scores": rng.standard_normal((nq, k)).astype(np.float32),
            "rows": rng.integers(0, 1 << 24, (nq, k)).astype(np.float32)}


def test_dump_under_budget_writes_everything(tmp_path):
    arrays = _lists(50, 20)
    info = bench.dump_outputs(str(tmp_path), arrays)
    assert info["files"] == ["rows.npy", "scores.npy"] and info["queries"] == info["of_queries"] == 50
    assert sorted(os.listdir(tmp_path)) == ["rows.npy", "scores.npy"]
    for name, a in arrays.items():
        b = np.load(tmp_path / (name + ".npy"))
        assert b.dtype == a.dtype and np.array_equal(a, b)


def test_dump_over_budget_writes_a_fixed_sample(tmp_path):
    arrays = _lists(1000, 100)                  # 800 kB
    budget = 100_000
    infos = []
    for sub in ("a", "b"):
        infos.append(bench.dump_outputs(str(tmp_path / sub), arrays, budget=budget))
        total = sum(os.path.getsize(tmp_path / sub / f) - 128 for f in infos[-1]["files"])   # (npy headers: 128 bytes)
        assert total <= budget
    assert infos[0] == {**infos[1], "dir": infos[0]["dir"]}
    assert infos[0]["files"] == ["query_index.npy", "rows.npy", "scores.npy"]
    m = infos[0]["queries"]
    assert 0 < m < 1000 and m == budget // (800 + 8)
    sel = np.load(tmp_path / "a" / "query_index.npy")
    assert sel.dtype == np.float64 and np.array_equal(sel, np.load(tmp_path / "b" / "query_index.npy"))
    assert np.all(np.diff(sel) > 0)
    idx = sel.astype(np.int64)
    for name, a in arrays.items():
        b = np.load(tmp_path / "a" / (name + ".npy"))
        assert np.array_equal(b, a[idx]) and np.array_equal(b, np.load(tmp_path / "b" / (name + ".npy")))


def test_dump_prefix_names_the_sample_index(tmp_path):
    arrays = {"beir_nq_" + k: v for k, v in _lists(100, 50).items()}
    info = bench.dump_outputs(str(tmp_path), arrays, budget=10_000)
    assert info["files"] == ["beir_nq_query_index.npy", "beir_nq_rows.npy", "beir_nq_scores.npy"]
