"""Bit-identity anchor of the key-tiled rel-pos attention kernels under their LOCAL span (|i - j| <= window): SHA-256 digests of
ctx, lse, dqkv, dpl, dbias_u and dbias_v from fast.relpos_attention_local(..., want_lse=True) and fast.relpos_attention_local_bwd,
recorded in tests/golden/attention_local_digests.json.  The full span is pinned by tests/test_attention_flash_digests_gpu.py.

The other tests of the local span hold it to fp64 within 3e-2 of the largest element, and to the full span's values only where
the window is at least T - 1: a changed order of summation, a flushed chunk that lands one row over, or a dropped clamp can pass
them.  This file pins the bits.  Every case runs with p = 0 and p = 0.25 under one seed.  The shapes are the smallest that reach
every line where the local span differs from the full one (B, T, H, dk; window; lens):

  l64_w1 (1, 64, 1, 64; 1; [64]): the smallest window, pad0 = 6, Rs = 16.  Almost every flushed 16-byte chunk falls outside the
      row [0, Rs) on one side or the other, and so does the final carry: the flush bounds
  l130_w4 (2, 130, 2, 64; 4; [130, 70]): w < 16, pad0 = 3, Rs = 16.  Query tile 1 processes key tile 0, in which queries >= 68 have
      no admissible key: the forward's guard against -inf - -inf.  One length ends inside a tile; one query tile holds two live rows
  l300_w62 (2, 300, 2, 64; 62; [300, 191]): on the diagonal tile waves 1 and 2 take the forward's mask-free branch and waves 0 and 3
      the masked one, inside one workgroup.  Key tiles are skipped on both sides (t_lo > 0 for the last query tiles, t_hi below
      the last tile for the first)
  l321_w100 (2, 321, 1, 64; 100; [321, 64]): the window is no multiple of 8 (pad0 = 3, Rs = 208).  Four-tile walks carry the dS strip
      across tiles.  len = 64 on a tile boundary: the `I0 >= len` and `J0 >= len` early exits give zero rows and zero bias partials
  l200_dk36_w16 (3, 200, 4, 36; 16; [200, 129, 1]): DK64 = false with a half-filled slot.  B * H = 12 > 8: a second round of
      XCD-congruent ids returns at `bh >= B * H`.  One utterance has length 1
  l65_dk48_w64 (1, 65, 2, 48; 64; [65]): window = T - 1 exactly, whole zero-padded slots, position rows clamped at both ends of
      [0, 2w]
  l50_dk8_w1000 (1, 50, 2, 8; 1000; [50]): the window is far beyond T: the host reduces it to w' = T - 1 and advances the table
      pointer by window - w' rows; dpl gets the row0 > 0 memset in front and zero rows behind the band
  l70_empty_w16 (3, 70, 2, 64; 16; [70, 0, 33]): a zero-length utterance in all three kernels

The position projections have 2 * window + 2 rows, one more than is read: the backward's packing pass writes a zero row there.
dpl, dbias_u and dbias_v also pass through the grouped TN GEMM and the partials pass that ia_relpos_attention_local_bwd issues.

Inputs are made on the CPU from one seeded generator and never modified.  The digests of the inputs are recorded too and checked
first: when they differ, torch's generators changed, not the kernels, and the failure says so.  A missing file or key fails;
nothing skips.

`python tests/test_attention_local_digests_gpu.py` prints the JSON to record (IA_LIB_PATH selects the library that computes it)."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_local_digests.json")
SEED = 1234
SHAPES = {
    "l64_w1": dict(B=1, T=64, H=1, dk=64, window=1, lens=[64]),
    "l130_w4": dict(B=2, T=130, H=2, dk=64, window=4, lens=[130, 70]),
    "l300_w62": dict(B=2, T=300, H=2, dk=64, window=62, lens=[300, 191]),
    "l321_w100": dict(B=2, T=321, H=1, dk=64, window=100, lens=[321, 64]),
    "l200_dk36_w16": dict(B=3, T=200, H=4, dk=36, window=16, lens=[200, 129, 1]),
    "l65_dk48_w64": dict(B=1, T=65, H=2, dk=48, window=64, lens=[65]),
    "l50_dk8_w1000": dict(B=1, T=50, H=2, dk=8, window=1000, lens=[50]),
    "l70_empty_w16": dict(B=3, T=70, H=2, dk=64, window=16, lens=[70, 0, 33]),
}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def inputs():
    """Every CPU tensor the cases read, drawn in a fixed order from one generator."""
    gen = torch.Generator().manual_seed(27183)
    x = {}
    for name, s in SHAPES.items():
        B, T, H, dk, w = s["B"], s["T"], s["H"], s["dk"], s["window"]
        d = H * dk
        x[f"qkv_{name}"] = (torch.randn(B * T, 3 * d, generator=gen) * 0.8).bfloat16()
        x[f"pl_{name}"] = (torch.randn(2 * w + 2, d, generator=gen) * 0.8).bfloat16()
        x[f"bu_{name}"] = torch.randn(H, dk, generator=gen) * 0.3
        x[f"bv_{name}"] = torch.randn(H, dk, generator=gen) * 0.3
        x[f"dctx_{name}"] = (torch.randn(B * T, d, generator=gen) * 0.5).bfloat16()
    return x


@functools.lru_cache(maxsize=None)
def input_digests():
    return {k: sha(v) for k, v in inputs().items()}


def case(name, p):
    from indic_cl_asr_amd.ops import fast
    x, s = inputs(), SHAPES[name]
    B, T, H, dk, w = s["B"], s["T"], s["H"], s["dk"], s["window"]
    qkv, pl, bu, bv, dctx = (x[f"{k}_{name}"].cuda() for k in ("qkv", "pl", "bu", "bv", "dctx"))
    lens = torch.tensor(s["lens"], dtype=torch.int64).cuda()
    ctx, lse = fast.relpos_attention_local(qkv, pl, bu, bv, lens, B, T, H, dk, w, dropout_p=p, seed=SEED, want_lse=True)
    dqkv, dpl, du, dv = fast.relpos_attention_local_bwd(qkv, pl, bu, bv, lens, ctx, dctx, lse, B, T, H, dk, w, dropout_p=p, seed=SEED)
    torch.cuda.synchronize()
    return {"ctx": sha(ctx), "lse": sha(lse), "dqkv": sha(dqkv), "dpl": sha(dpl), "dbias_u": sha(du), "dbias_v": sha(dv)}


CASES = {f"{name}_p{p}": functools.partial(case, name, p) for name in SHAPES for p in (0.0, 0.25)}


@functools.lru_cache(maxsize=None)
def golden():
    assert os.path.exists(GOLDEN), f"{GOLDEN} is missing: record it with `python tests/test_attention_local_digests_gpu.py`"
    with open(GOLDEN) as f:
        return json.load(f)


def test_inputs_are_the_recorded_ones():
    assert "inputs" in golden(), "the inputs are not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernels"


@pytest.mark.parametrize("case_name", list(CASES))
def test_attention_local_digests(case_name):
    assert "inputs" in golden() and case_name in golden().get("cases", {}), f"{case_name} is not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernels"
    got, want = CASES[case_name](), golden()["cases"][case_name]
    differing = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert not differing, f"{case_name}: {differing} differ from the recorded digests"


if __name__ == "__main__":
    record = {"inputs": input_digests(), "cases": {name: fn() for name, fn in CASES.items()}}
    print(json.dumps(record, indent=1, sort_keys=True))
