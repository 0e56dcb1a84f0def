"""Writes tests/golden/ctc_align_long_cases.npz: long-transcript CTC forced-alignment cases (256 to 4096 tokens) and what the
reference's aligner returns for them.

Run by hand where the reference tree is at hand; never imported by a test:

    python tests/golden/make_ctc_align_long_golden.py [/path/to/NeMo]        (default /root/reference/NeMo)

The method, the grids and the file layout are those of make_ctc_align_golden.py (whose helpers are imported): NeMo forced
aligner's viterbi_decoding, loaded unchanged and run one utterance at a time, on inputs that lie on a dyadic grid (fine:
step 2^-6 on [-8, 0]; coarse: step 1.0 on [-4, 0], most decisions are ties), the fp64 restatement of the recurrence asserted
equal to the reference before anything is written, grid indices stored as int16.  V = 9 (blank = 8) keeps the file small.

Exactness at these lengths: the longest case has T = 5831 frames of at most 8 / 2^-6 = 512 grid units each, so every partial
sum is an integer below 5831 * 512 < 2^22 grid units (asserted below against 2^24): every fp32 addition is exact in the
reference, in the host routine and in the kernel.  The logits mode adds a synthetic lse of at most 512 units per frame:
logit = log-prob + lse and logit - lse are exact too.

Cases (T, S, mode); the targets of a case are redrawn until T >= minimum feasible length + 37; `below_min` has S = 600 and one
frame too few.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_ctc_align_golden import load_reference, min_frames, restate_fp64, targets_for  # noqa: E402

CASES = [(328, 256, "random"), (754, 512, "repeats"), (1400, 1023, "coarse"), (2342, 2047, "random"), (5831, 4096, "repeats")]
V = 9
MARGIN = 37


def main():
    nemo_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/NeMo"
    viterbi_decoding = load_reference(nemo_root)
    rng = np.random.default_rng(20240911)
    cases = []          # (name, T, y, step)
    for T, S, mode in CASES:
        y = targets_for(rng, S, V, mode)
        while min_frames(y) + MARGIN > T:
            y = targets_for(rng, S, V, mode)
        cases.append((f"{mode}_T{T}_S{S}", T, y, 1.0 if mode == "coarse" else 2.0 ** -6))
    y = targets_for(rng, 600, V, "repeats")
    cases.append(("below_min", min_frames(y) - 1, y, 2.0 ** -6))

    out = {}
    steps, scores, names = [], [], []
    blank = V - 1
    for i, (name, T, y, step) in enumerate(cases):
        units = int((4 if step == 1.0 else 8) / step)
        assert T * units < 2 ** 24, name                  # every partial sum is an exact fp32 integer of grid units
        g = rng.integers(0, units + 1, size=(T, V))
        z = rng.integers(0, int(8 / step) + 1, size=T)
        lp32 = (-(g.astype(np.float64)) * step).astype(np.float32)
        assert np.all(lp32.astype(np.float64) == -(g * step))
        path64, score64 = restate_fp64(lp32.astype(np.float64), y, blank)
        feasible = T >= min_frames(y)
        assert feasible == (path64 is not None) and feasible == (name != "below_min"), name
        if feasible:
            ext = np.full(2 * len(y) + 1, blank, dtype=np.int64)
            ext[1::2] = y
            ref = viterbi_decoding(torch.from_numpy(lp32).unsqueeze(0), torch.from_numpy(ext).unsqueeze(0),
                                   torch.tensor([T]), torch.tensor([len(ext)]), torch.device("cpu"))[0]
            ref = np.array(ref, dtype=np.int64)
            assert ref.shape == (T,) and np.array_equal(ref, path64), f"{name}: reference and fp64 restatement differ"
            rescored = float(np.sum(lp32.astype(np.float64)[np.arange(T), ext[ref]]))
            assert rescored == score64, name
        else:
            ref, rescored = np.zeros(0, dtype=np.int64), -np.inf
        assert ref.max(initial=0) < 2 ** 15 and g.max() < 2 ** 15
        out[f"g{i}"], out[f"z{i}"] = g.astype(np.int16), z.astype(np.int16)
        out[f"y{i}"], out[f"path{i}"] = y.astype(np.int16), ref.astype(np.int16)
        steps.append(step); scores.append(rescored); names.append(name)
        print(f"{name}: T={T} S={len(y)} min_frames={min_frames(y)} score={rescored}")
    out["step"], out["score"] = np.array(steps, dtype=np.float64), np.array(scores, dtype=np.float64)
    out["name"] = np.array(names)
    dst = os.path.join(HERE, "ctc_align_long_cases.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(cases)} utterances (reference == fp64 restatement on every feasible one), {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
