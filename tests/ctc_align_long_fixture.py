"""Shared by tests/test_ctc_align_long.py and tests/test_ctc_align_long_gpu.py: the long golden cases of
tests/golden/ctc_align_long_cases.npz (written by tests/golden/make_ctc_align_long_golden.py from the reference's aligner,
same layout as ctc_align_cases.npz without the ragged batch), and unquantised inputs with repeats at every third target."""
import os

import numpy as np
import torch

GOLDEN_LONG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_align_long_cases.npz")

_cases = None


def load_long_cases():
    """One dict per utterance, as ctc_align_fixture.load_cases returns them (read once, shared, never modified)."""
    global _cases
    if _cases is None:
        z = np.load(GOLDEN_LONG)
        _cases = []
        for i, name in enumerate(z["name"]):
            step = float(z["step"][i])
            lp = (-(z[f"g{i}"].astype(np.float64)) * step).astype(np.float32)
            lse = (z[f"z{i}"].astype(np.float64) * step).astype(np.float32)
            score = float(z["score"][i])
            _cases.append(dict(name=str(name), lp=lp, lse=lse, logits=lp + lse[:, None], y=z[f"y{i}"].astype(np.int64),
                               V=lp.shape[1], blank=lp.shape[1] - 1, score=score,
                               path=None if score == -np.inf else z[f"path{i}"].astype(np.int64)))
    return _cases


def repeating_targets(g, B, S, V):
    """[B,S] i64 below the blank V - 1; every third target repeats its predecessor: forbidden skips all along the transcript."""
    tg = torch.randint(0, V - 1, (B, S), generator=g)
    for i in range(2, S, 3):
        tg[:, i] = tg[:, i - 1]
    return tg


def min_frames(y):
    """Shortest utterance a transcript fits: its tokens plus one blank between adjacent repeats."""
    y = np.asarray(y)
    return len(y) + int(np.sum(y[1:] == y[:-1]))
