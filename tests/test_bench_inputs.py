"""bench.py without a GPU: the inputs of a run are the same from run to run (so that --dump-outputs of two builds can be
compared output for output), and the options of the plain / --full split are there."""
import os
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_synthetic_batch_and_initial_weights_repeat_from_run_to_run():
    import bench
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    (a, la), (b, lb) = bench.synth_batch(4, 2.0, "cpu"), bench.synth_batch(4, 2.0, "cpu")
    assert la == lb and all(torch.equal(x, y) for x, y in zip(a, b))
    states = []
    for _ in range(2):
        torch.manual_seed(1234)       # bench.main's seed in front of the model
        states.append(EncDecHybridRNNTCTCModel(model_config("tiny", compute_dtype="fp32")).state_dict())
    assert states[0].keys() == states[1].keys() and all(torch.equal(states[0][k], states[1][k]) for k in states[0])


def test_bench_offers_full_and_dump_outputs():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=300,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "--full" in p.stdout and "--dump-outputs" in p.stdout
