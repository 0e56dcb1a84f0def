"""bench.py's output contract (the driver parses ONE JSON line from rank 0): keys, types and the internal consistency of the
line, on a short run of the headline configuration (--full: every figure the line can carry)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_prints_one_json_line_with_the_contract_keys():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "6", "--warmup", "6",
                        "--full", "--no-cpu-baseline", "--no-peaks"], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    for k, typ in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                   ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str), ("config", dict)):
        assert isinstance(d[k], typ), (k, d[k])
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 6 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None                     # BASELINE.md holds no published number for this metric
    assert d["unit"] == "utterances/s" and d["dtype"] == "bf16" and d["data"] == "synthetic"
    cfg = d["config"]
    assert "BASELINE configs[1]" in cfg["workload"] and cfg["global_batch"] == 32 and cfg["parallelism"] == "dp1"
    assert "model" not in cfg
    # value = utterances of the whole job / time of the timed steps
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    # the timed steps are the reference-complete step: in-step decode + both WERs, monitor read after every optimizer step
    assert cfg["in_step_wer"]["enabled"] is True and 0.0 <= cfg["in_step_wer"]["training_batch_wer"]
    assert cfg["without_wer"]["in_step_wer"] is False and cfg["without_wer"]["ms_per_step"] > 0
    assert cfg["with_h2d_prefetch"]["h2d_bytes_per_step"] > 0
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s")
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) <= 2e-3 and 0.0 < rf["frac"] < 1.0
    assert "traffic" in rf
    assert "cpu_baseline" in d                          # (null here: --no-cpu-baseline; a --full run without it fills it)


def test_plain_bench_times_only_the_headline_and_dumps_the_last_step(tmp_path):
    """The plain run (no --full): exactly --steps timed steps, the headline keys, none of the --full legs or figures, and
    --dump-outputs writes the last timed step's loss, monitor, updated parameters and gradient as float32 / float64 .npy
    files within 64 MB."""
    import numpy as np
    out_dir = tmp_path / "out"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--dump-outputs", str(out_dir)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["unit"] == "utterances/s" and d["dtype"] == "bf16"
    assert d["higher_is_better"] is True and d["ms_per_step"] > 0
    assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert d["config"]["in_step_wer"]["enabled"] is True
    for k in ("roofline", "roofline_mfma", "rooflines", "peaks_measured", "cpu_baseline"):
        assert k not in d, k
    for k in ("without_wer", "with_wer", "with_h2d_prefetch"):
        assert k not in d["config"], k
    files = {f.name: f for f in out_dir.iterdir()}
    assert {"loss.npy", "params.npy", "grads.npy", "monitor_train_loss.npy", "monitor_train_rnnt_loss.npy",
            "monitor_train_ctc_loss.npy", "monitor_training_batch_wer.npy", "monitor_ewc_penalty.npy"} <= set(files), sorted(files)
    assert sum(f.stat().st_size for f in files.values()) <= 64 << 20
    arrays = {n: np.load(f) for n, f in files.items()}
    for n, a in arrays.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
    assert arrays["params.npy"].shape == arrays["grads.npy"].shape == (1 << 22,)     # seeded sample of 17.3 M trainable values
    assert np.abs(arrays["grads.npy"]).max() > 0
    assert abs(float(arrays["loss.npy"]) - d["config"]["final_loss"]) <= 1e-4 * abs(d["config"]["final_loss"]) + 1e-4
    assert abs(float(arrays["loss.npy"]) - float(arrays["monitor_train_loss.npy"])) <= 1e-6 * abs(float(arrays["loss.npy"]))
