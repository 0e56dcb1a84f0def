"""Bit-identity anchor of the key-tiled rel-pos attention kernels (csrc/attention_flash.hip forward, csrc/attention_flash_bwd.hip
query-owner and key-owner backward, on the shared vocabulary of csrc/attention_flash.h): SHA-256 digests of ctx, lse, dqkv, dpl,
dbias_u and dbias_v, recorded in tests/golden/attention_flash_digests.json.

The other tests of these kernels hold them to fp64 within 2e-2 / 3e-2 of the largest element: a changed order of summation, a
wrong swizzle phase that lands on a neighbouring row's valid data or a dropped clamp at T % 64 != 0 can pass them.  This file pins
the bits.  Every case runs with p = 0 and p = 0.25 under one seed: the two sides of the `a.thr > 0` branches of all three kernels,
and the mask that both backward kernels regenerate from the forward's hash.  The shapes are the smallest that reach every path
(B, T, H, dk; lens):

  t17 (2, 17, 2, 64; [17, 9]): one partial query / key tile.  Waves 2 and 3 hold only rows >= T (the `iqc` / `jc` clamps, no store);
      wave 1 is the partial last wave whose band flush starts left of column 0 (the `gcol < 0` guard); pad0 = 7.  Utterance 1 ends
      inside wave 0's rows: the length mask of the forward, `qvalid` / `kvalid` false in live workgroups
  t64 (2, 64, 1, 64; [64, 63]): exactly one full tile, no clamp anywhere in the K / V / Q staging.  Utterance 0 takes the forward's
      unmasked score branch (`j0 + 64 <= len`), utterance 1 the masked one, in the same launch; pad0 = 0
  t65_dk48 (1, 65, 2, 48; [65]): DK64 = false with whole slots zero-padded (slots 6, 7).  The second tile holds one row: every other
      row of its staging is clamped to T - 1.  The position rows are clamped at both ends (`r_ < 0` in query tile 1 / key tile 0,
      `r_ > 2T - 2` in query tile 0 / key tile 1)
  t126_dk36 (3, 126, 4, 36; [126, 64, 5]): dk no multiple of 8: slot 4 is half filled (`e0 < dk` without `e0 + 4 < dk`), and the
      guarded head-row store stops after dk = 36 (mt = 2: only q4 = 0).  B * H = 12 > 8: a second round of XCD-congruent ids whose
      ids 4 .. 7 return at `bh >= B * H`.  len = 64 on a tile boundary: the second query / key tile leaves early (`I0 >= len`,
      `J0 >= len`) with zero rows and zero bias partials, the first runs exactly one tile.  len = 5: one wave live
  t200 (4, 200, 2, 64; [128, 200, 1, 129]): four tiles.  The register prefetch under compute (`t + 1 < nkt`), the carry of the dS
      band strip across key tiles and its last flush behind tile nkt - 1, lengths on a tile boundary (128), one past it (129: a
      tile with one live key / query), and 1
  t70_empty (3, 70, 2, 64; [70, 0, 33]): a zero-length utterance, which every workgroup of it leaves early in all three kernels
      (zero ctx, lse, D, dq, dk, dv, bias partials; its dBand rows stay the memset's); pad0 = 2

The position projections have 2T rows, one more than the kernels read: the backward's packing pass writes a zero row there.
dpl, dbias_u and dbias_v also pass through the grouped TN GEMM and the partials pass that ia_relpos_attention_flash_bwd issues.

Inputs are made on the CPU from one seeded generator and never modified.  The digests of the inputs are recorded too and checked
first: when they differ, torch's generators changed, not the kernels, and the failure says so.  A missing file or key fails;
nothing skips.

`python tests/test_attention_flash_digests_gpu.py` prints the JSON to record (IA_LIB_PATH selects the library that computes it)."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "attention_flash_digests.json")
SEED = 1234
SHAPES = {
    "t17": dict(B=2, T=17, H=2, dk=64, lens=[17, 9]),
    "t64": dict(B=2, T=64, H=1, dk=64, lens=[64, 63]),
    "t65_dk48": dict(B=1, T=65, H=2, dk=48, lens=[65]),
    "t126_dk36": dict(B=3, T=126, H=4, dk=36, lens=[126, 64, 5]),
    "t200": dict(B=4, T=200, H=2, dk=64, lens=[128, 200, 1, 129]),
    "t70_empty": dict(B=3, T=70, H=2, dk=64, lens=[70, 0, 33]),
}


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def inputs():
    """Every CPU tensor the cases read, drawn in a fixed order from one generator."""
    gen = torch.Generator().manual_seed(31337)
    x = {}
    for name, s in SHAPES.items():
        B, T, H, dk = s["B"], s["T"], s["H"], s["dk"]
        d = H * dk
        x[f"qkv_{name}"] = (torch.randn(B * T, 3 * d, generator=gen) * 0.8).bfloat16()
        x[f"pl_{name}"] = (torch.randn(2 * T, d, generator=gen) * 0.8).bfloat16()
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
    B, T, H, dk = s["B"], s["T"], s["H"], s["dk"]
    qkv, pl, bu, bv, dctx = (x[f"{k}_{name}"].cuda() for k in ("qkv", "pl", "bu", "bv", "dctx"))
    lens = torch.tensor(s["lens"], dtype=torch.int64).cuda()
    ctx, lse = fast.relpos_attention_flash(qkv, pl, bu, bv, lens, B, T, H, dk, dropout_p=p, seed=SEED, want_lse=True)
    dqkv, dpl, du, dv = fast.relpos_attention_flash_bwd(qkv, pl, bu, bv, lens, ctx, dctx, lse, B, T, H, dk, dropout_p=p, seed=SEED)
    torch.cuda.synchronize()
    return {"ctx": sha(ctx), "lse": sha(lse), "dqkv": sha(dqkv), "dpl": sha(dpl), "dbias_u": sha(du), "dbias_v": sha(dv)}


CASES = {f"{name}_p{p}": functools.partial(case, name, p) for name in SHAPES for p in (0.0, 0.25)}


@functools.lru_cache(maxsize=None)
def golden():
    assert os.path.exists(GOLDEN), f"{GOLDEN} is missing: record it with `python tests/test_attention_flash_digests_gpu.py`"
    with open(GOLDEN) as f:
        return json.load(f)


def test_inputs_are_the_recorded_ones():
    assert "inputs" in golden(), "the inputs are not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernels"


@pytest.mark.parametrize("case_name", list(CASES))
def test_attention_flash_digests(case_name):
    assert "inputs" in golden() and case_name in golden().get("cases", {}), f"{case_name} is not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernels"
    got, want = CASES[case_name](), golden()["cases"][case_name]
    differing = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert not differing, f"{case_name}: {differing} differ from the recorded digests"


if __name__ == "__main__":
    record = {"inputs": input_digests(), "cases": {name: fn() for name, fn in CASES.items()}}
    print(json.dumps(record, indent=1, sort_keys=True))
