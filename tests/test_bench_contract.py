"""The driver depends on bench.py's exact output contract: one JSON line
from rank 0 with specific keys. Run it end-to-end (CPU, tiny config) and
validate the schema."""
import json
import os
import subprocess
import sys

import numpy as np

REPO =os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_json_contract():
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--config", "shakespeare_char",
         "--local-batch", "4"],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for key, typ in [("metric", str), ("value", (int, float)), ("unit", str),
                     ("n_gpus", int), ("steps", int), ("warmup", int),
                     ("ms_per_step", (int, float)), ("higher_is_better", bool),
                     ("scaling", str), ("vs_baseline", (int, float)),
                     ("dtype", str), ("data", str), ("config", dict)]:
        assert key in d, key
        assert isinstance(d[key], typ), (key, type(d[key]))
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["data"] == "synthetic"
    assert d["scaling"] == "weak"
    assert d["higher_is_better"] is True
    for k in ["model", "global_batch", "seq_len", "parallelism"]:
        assert k in d["config"], k


def _run_bench(*extra):
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--config", "shakespeare_char",
         "--local-batch", "4", *extra],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's results as float .npy,
    identical between two runs with the same arguments (same inputs, same
    init); --full leaves the result line's keys and the outputs unchanged."""
    a, b = tmp_path / "a", tmp_path / "b"
    da = _run_bench("--dump-outputs", str(a))
    db = _run_bench("--dump-outputs", str(b), "--full")
    assert set(da) == set(db)
    assert da["config"]["last_loss"] == db["config"]["last_loss"]
    names = sorted(f.name for f in a.iterdir())
    assert names == ["grad_sq_sum.npy", "loss.npy", "weights.npy"]
    assert sorted(f.name for f in b.iterdir()) == names
    total = 0
    for n in names:
        xa, xb = np.load(a / n), np.load(b / n)
        assert xa.dtype in (np.float32, np.float64), (n, xa.dtype)
        assert xa.size > 0 and np.isfinite(xa).all(), n
        assert xa.shape == xb.shape, n
        # Same seed, same inputs: the only run-to-run difference allowed is
        # the order of fp32 reductions on the GPU (a few 1e-6 relative on
        # the loss), far below one bf16 ulp (4e-3) of the compute dtype,
        # which is the least that different inputs or init would show.
        np.testing.assert_allclose(xa, xb, rtol=1e-4, atol=1e-6, err_msg=n)
        total += xa.nbytes
    assert total <= 64 * 2**20
    loss = np.load(a / "loss.npy")
    assert loss.shape == (da["config"]["g_accum_iters"],)
    assert abs(float(loss[-1]) - da["config"]["last_loss"]) < 1e-3
