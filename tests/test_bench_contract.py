"""The driver parses ONE JSON line from bench.py — pin the contract
(field names, types, aggregate semantics) on the CPU path so a refactor
cannot silently break the round-end harness."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(tmp_path, *args):
    env = dict(os.environ)
    env["LZY_BENCH_SHARD_MB"] = "2"
    env["LZY_AMD_STORAGE"] = str(tmp_path / "storage")
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.pop("LZY_BENCH_PROFILE", None)
    r = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), *args],
        cwd=ROOT, env=env, capture_output=True, text=True, timeout=300,
    )
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r


def test_bench_json_contract(tmp_path):
    r = _run_bench(tmp_path, "--steps", "2", "--warmup", "1")
    assert "# lzy_dispatch" not in r.stderr  # breakdown table is --full only
    line = r.stdout.strip().splitlines()[-1]
    d = json.loads(line)

    assert d["metric"] == "workflow_makespan_s_8stage_dag"
    assert isinstance(d["value"], float) and d["value"] > 0
    assert d["unit"] == "s"
    assert d["n_gpus"] == 1
    assert d["steps"] == 2 and d["warmup"] == 1
    assert d["higher_is_better"] is False
    assert d["scaling"] == "weak"
    assert d["vs_baseline"] is None  # reference publishes no number
    assert d["data"] == "synthetic"
    assert isinstance(d["ms_per_step"], float)
    cfg = d["config"]
    # steps * ms_per_step reproduces the timed region (driver's check)
    assert abs(d["steps"] * d["ms_per_step"] / 1000.0
               - cfg["timed_region_s"]) < 0.05 * cfg["timed_region_s"] + 1e-6
    # value is the per-DAG makespan of repeats-declared work
    assert cfg["dag_repeats_per_step"] >= 1
    assert abs(cfg["dag_ms"] - d["value"] * 1000.0) < 1e-6
    for key in ("model", "global_batch", "seq_len", "parallelism",
                "shard_mb", "ops_per_dag", "transfers", "stage_ms"):
        assert key in cfg, key
    assert set(cfg["stage_ms"]) >= {"ingest", "preprocess", "augment",
                                    "train_step", "checksum", "evaluate",
                                    "report"}


def test_bench_dump_outputs_reproducible_and_full(tmp_path):
    """--dump-outputs writes the last timed DAG's results as float64
    .npy files, identical from run to run (seeded inputs, fixed DAG
    count per step); --full adds the breakdown table on stderr and keeps
    the one-JSON-line contract on stdout."""
    import numpy as np

    names = {"summary": (1,), "losses": (1,), "eval_score": (1,),
             "checksums": (1, 2)}
    runs = []
    for tag, extra in (("a", ()), ("b", ("--full",))):
        out = tmp_path / tag
        r = _run_bench(tmp_path / ("s" + tag), "--gpus", "1", "--steps", "1",
                       "--warmup", "1", "--dump-outputs", str(out), *extra)
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert d["steps"] == 1 and d["ms_per_step"] > 0
        assert ("# lzy_dispatch" in r.stderr) == bool(extra)
        assert {p.name for p in out.iterdir()} == {n + ".npy" for n in names}
        arrs = {n: np.load(out / (n + ".npy")) for n in names}
        for n, shape in names.items():
            assert arrs[n].dtype == np.float64 and arrs[n].shape == shape, n
            assert np.isfinite(arrs[n]).all(), n
        runs.append((d, arrs))
    (da, a), (db, b) = runs
    assert da["config"]["dag_repeats_per_step"] \
        == db["config"]["dag_repeats_per_step"]
    # the content hash pins the inputs bit for bit; the float results come
    # from the same fp32 CPU kernels on the same data, so only the order
    # of a threaded reduction may differ: a few fp32 ulps (2^-23 each)
    assert np.array_equal(a["checksums"], b["checksums"])
    for n in ("summary", "losses", "eval_score"):
        assert np.allclose(a[n], b[n], rtol=1e-5, atol=0.0), (n, a[n], b[n])
