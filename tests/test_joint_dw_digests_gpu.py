"""Bit-identity anchor of the joint's fused weight-gradient kernel (csrc/joint_dw.hip): SHA-256 digests of dW (fp32 [LD, H]),
recorded in tests/golden/joint_dw_digests.json.

The other tests of the kernel compare its step geometries with each other and with a reference to a tolerance; a changed order of
summation passes them.  This file pins the bits.  Every case runs with p = 0 and p = 0.2 (the two DROPOUT instantiations); the
shapes are the smallest that reach every path of the step cursor, the loaders and the two wave-group loops.  The split plan is
S = min(8 * (32 / ceil(H / 128)), B * ceil(T * U1 / 64)) planned splits, steps_per_split = ceil(planned steps / S), Seff =
ceil(planned steps / steps_per_split) launched splits; with length arrays the LIVE steps are shared: ceil(live / Seff) each.

  b3_ld40 (B 3, T 19, U1 11, H 136, LD 40; frames [19, 7, 1], labels [10, 4, 0]): 3 x 4 = 12 planned steps, 12 splits of one.
      tiled (both length arrays): 3 x 2 + 1 + 1 = 8 live 8 x 8 tiles, so splits 8 .. 11 write a zero partial tile; T = 19 and
          U1 = 11 shift the last frame tile and the last label tile back inside the lattice (rows switched off through the hidden
          rows), utterance 2 has one live frame in an 8-frame tile; the second hidden tile has 8 live columns; 64 x 5 = 320 G
          chunks < 512 threads: chunks 1 .. 4 of every thread and chunk 0 of 192 threads land in the dump slot
      flat_lens (frame counts only): 4 + 2 + 1 = 7 live 64-cell steps found by the prefix pass; step 3 of utterance 0 has 17 rows
          (T * U1 = 209): the masked store
      flat (no lengths): 12 steps; the split's start comes from the reciprocal division
  b3_ld272: the same with LD = 272: 64 x 34 = 2176 chunks, all five chunks of a thread live (the fifth for 128 threads)
  b9_full (B 9, T 40, U1 24, H 520, LD 272; full lengths): five hidden tiles, the last with 8 live columns; 48 planned splits, 9 x 15
      = 135 steps, 3 per split, 45 launched.  tiled: 5 x 3 tiles per utterance = 135 live, 3 per split; flat_lens: the same count.
      Waves 4-7 leave their two-steps-per-iteration loop at its `break`
  b9_ragged (frames [40, 35, 21, 40, 9, 28, 40, 16, 33], labels [23, 17, 9, 23, 3, 12, 20, 7, 15]):
      tiled: 15 + 15 + 6 + 15 + 2 + 8 + 15 + 2 + 10 = 88 live tiles, 2 per split; split 7 (tiles 14, 15) straddles utterances 0
          and 1, its prediction rows are reloaded mid-split; split 44 is empty
      flat_lens: 15 + 14 + 8 + 15 + 4 + 11 + 15 + 6 + 13 = 101 live steps, 3 per split, splits 34 .. 44 empty
  streamed (B 2, T 9, U1 131, H 136, LD 40; frames [9, 5], labels [130, 77]): U1 > 128, the prediction rows are fetched per step
      next to the f rows.  38 planned steps and splits; tiled: 2 x 17 + 10 = 44 live tiles, 2 per split; flat_lens: 19 + 11 = 30

Inputs are made on the CPU from one seeded generator and never modified; G is zero outside each utterance's live box and finite
everywhere.  The digests of the inputs are recorded too and checked first: when they differ, torch's generators changed, not the
kernel, and the failure says so.  A missing file or key fails; nothing skips.

`python tests/test_joint_dw_digests_gpu.py` prints the JSON to record (IA_LIB_PATH selects the library that computes it)."""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # when run as a script
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "joint_dw_digests.json")
SEED = 7
B3 = dict(B=3, T=19, U1=11, H=136, frames=[19, 7, 1], labels=[10, 4, 0])
B9 = dict(B=9, T=40, U1=24, H=520, LD=272)
SHAPES = {
    "b3_ld40": dict(B3, LD=40),
    "b3_ld272": dict(B3, LD=272),
    "b9_full": dict(B9, frames=[40] * 9, labels=[23] * 9),
    "b9_ragged": dict(B9, frames=[40, 35, 21, 40, 9, 28, 40, 16, 33], labels=[23, 17, 9, 23, 3, 12, 20, 7, 15]),
    "streamed": dict(B=2, T=9, U1=131, H=136, LD=40, frames=[9, 5], labels=[130, 77]),
}
MODES = {"b3_ld40": ("tiled", "flat_lens", "flat"), "b3_ld272": ("tiled", "flat_lens", "flat"), "b9_full": ("tiled", "flat_lens"),
         "b9_ragged": ("tiled", "flat_lens"), "streamed": ("tiled", "flat_lens")}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def inputs():
    """Every CPU tensor the cases read, drawn in a fixed order from one generator."""
    gen = torch.Generator().manual_seed(20241)
    x = {}
    for name, s in SHAPES.items():
        B, T, U1, H, LD = s["B"], s["T"], s["U1"], s["H"], s["LD"]
        tl, ul = torch.tensor(s["frames"]), torch.tensor(s["labels"])
        live = (torch.arange(T).view(1, T, 1, 1) < tl.view(B, 1, 1, 1)) & (torch.arange(U1).view(1, 1, U1, 1) <= ul.view(B, 1, 1, 1))
        G = torch.randn(B, T, U1, LD, generator=gen) * 0.01
        x[f"G_{name}"] = (G * live).half().view(B * T * U1, LD).contiguous()
        x[f"f_{name}"] = torch.randn(B, T, H, generator=gen).half()
        x[f"g_{name}"] = torch.randn(B, U1, H, generator=gen).half()
        assert bool(torch.isfinite(x[f"G_{name}"]).all())
    return x


@functools.lru_cache(maxsize=None)
def input_digests():
    return {k: sha(v) for k, v in inputs().items()}


def case(name, mode, p):
    """tiled: ia_joint_dw_fused_ex with frame and label counts; flat_lens: ia_joint_dw_fused with the frame counts; flat: without."""
    from indic_cl_asr_amd import _lib
    L, ptr, x, s = _lib.lib(), _lib.ptr, inputs(), SHAPES[name]
    B, T, U1, H, LD = s["B"], s["T"], s["U1"], s["H"], s["LD"]
    G, f, g = x[f"G_{name}"].cuda(), x[f"f_{name}"].cuda(), x[f"g_{name}"].cuda()
    tl = torch.tensor(s["frames"], dtype=torch.long).cuda() if mode != "flat" else None
    ul = torch.tensor(s["labels"], dtype=torch.long).cuda()
    scr = torch.empty(L.ia_joint_dw_fused_scratch_elems(B, T, U1, H, LD), device="cuda")
    dW = torch.full((LD, H), float("nan"), device="cuda")
    if mode == "tiled":
        _lib.check(L.ia_joint_dw_fused_ex(ptr(G), ptr(f), ptr(g), ptr(tl), ptr(ul), B, T, U1, H, LD, p, SEED, ptr(dW), ptr(scr),
                                          _lib.stream_ptr()), "ia_joint_dw_fused_ex")
    else:
        _lib.check(L.ia_joint_dw_fused(ptr(G), ptr(f), ptr(g), ptr(tl), B, T, U1, H, LD, p, SEED, ptr(dW), ptr(scr),
                                       _lib.stream_ptr()), "ia_joint_dw_fused")
    torch.cuda.synchronize()
    return {"dW": sha(dW)}


CASES = {f"{name}_{mode}_p{p}": functools.partial(case, name, mode, p) for name in SHAPES for mode in MODES[name] for p in (0.0, 0.2)}


@functools.lru_cache(maxsize=None)
def golden():
    assert os.path.exists(GOLDEN), f"{GOLDEN} is missing: record it with `python tests/test_joint_dw_digests_gpu.py`"
    with open(GOLDEN) as f:
        return json.load(f)


def test_inputs_are_the_recorded_ones():
    assert "inputs" in golden(), "the inputs are not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernel"


@pytest.mark.parametrize("case_name", list(CASES))
def test_joint_dw_digests(case_name):
    assert "inputs" in golden() and case_name in golden().get("cases", {}), f"{case_name} is not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernel"
    got, want = CASES[case_name](), golden()["cases"][case_name]
    differing = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert not differing, f"{case_name}: {differing} differ from the recorded digests"


if __name__ == "__main__":
    record = {"inputs": input_digests(), "cases": {name: fn() for name, fn in CASES.items()}}
    print(json.dumps(record, indent=1, sort_keys=True))
