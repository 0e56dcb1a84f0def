"""Bit-identity anchor of the two joint kernels every training step runs first and longest: joint_fwd_kernel (csrc/joint_fwd.hip,
through ia_joint_fwd_box) and joint_dh_fused_kernel (csrc/joint_dh.hip, through ia_joint_dh_fused_ex).  SHA-256 digests of what
they write, recorded in tests/golden/joint_fwd_dh_digests.json.

tests/test_joint_gpu.py holds both to a reference within a tolerance; a changed order of summation, a clamped row that lands one
cell over or a keep bit taken from the neighbouring group passes there.  This file pins the bits.  Every case runs with p = 0 and
p = 0.2 under one seed (the two DROPOUT instantiations) and under both wave decompositions of its kernel (IA_JFWD_WAVES = 4 | 8,
IA_DH_WAVES = 4 | 10; the libraries read the switch on every call, the test sets it around the call and restores it).  Where the
10-wave hidden gradient is not eligible (H % 32 != 0) only the 4-wave case exists.  The two decompositions of a kernel compute the
same products in the same order per output, so their digests are equal: test_wave_decompositions_agree asserts it on the record.

Forward.  The logits buffer and the whole loss workspace are prefilled with the byte 0xA5 (cells outside the box are never
written).  Digested: the logits, the four side arrays denom / PB / PL / PLa as the kernel leaves them in the workspace (regions by
the layout of csrc/rnnt_ws.h, restated in ws_layout and checked against ia_rnnt_workspace_bytes), and the costs ia_rnnt_lattice
then returns.
  f_h64_v5    (B 3, T 19, U1 11, H 64, V 5, LD 8, blank 0; frames [19, 7, 1], labels [10, 4, 0]): one K chunk, the loop's prefetch
      branch never runs; T = 19 leaves a partial frame tile under JT = 16 and JT = 12; whole tiles return at t0 >= Tx; one
      utterance has a single frame and no label
  f_h192_v257 (B 2, T 33, U1 35, H 192, V 257, LD 264, blank 256; frames [29, 18], labels [34, 13]): three K chunks, three label
      tiles, label rows past U1 zero-staged, columns 257 .. 271 carry the -65504 padding
  f_v272      (B 1, T 16, U1 16, H 64, V 272): all 17 column tiles full, no padding column
  f_box       the f_h192_v257 tensors with boxes (33, 35) and (24, 20), one per utterance as of two sub-batches narrowed to their
      own maxima, each beyond its utterance's valid lattice (29 x 35, 18 x 14): logits stored for t < Tx, u < Ux, the scalars only
      for t < Tb, u < Ub; frame tile 32.. of utterance 0 runs only here

Hidden gradient.  G is zero outside each utterance's live box and finite everywhere; Wt is [H, 288] f16 (columns >= LD zero).
Each shape runs with fp32 outputs (zero_dead_df = 0, outputs prefilled with NaN) and with only the bf16 outputs (zero_dead_df = 1).
  h160_ld8   (B 5, T 19, U1 11, H 160, LD 8; frames [19, 7, 1, 16, 3], labels [10, 4, 0, 10, 7]): 10 workgroup tiles, one hidden
      half; eight tiles in the XCD-congruent order, two in the remainder order; waves 5 .. 9 of the 10-wave form off; frame chunks
      with 1, 3 and 4 live passes; utterance 3 has npt = 4 everywhere and its second frame chunk returns at t0 >= Tb
  h640_ld272 (B 3, T 37, U1 35, H 640, LD 272; frames [37, 22, 9], labels [34, 20, 5]): two hidden halves in both forms whose tiles
      read the same G rows; three label tiles with rows clamped at U1; dgacc reset and stored once per label tile; 34 of the 37
      slots of a G row live
  h480_ld288 (B 2, T 16, U1 16, H 480, LD 288; frames [16, 11], labels [15, 8]): the second half has five of ten (two of four)
      waves on; every column slot but the padding one is loaded
  h80_ld40   (B 2, T 9, U1 8, H 80, LD 40; frames [9, 4], labels [7, 2]): 4-wave form only, one wave on

Inputs are made on the CPU from one seeded generator and never modified.  Their digests are recorded too and checked first: when
they differ, torch's generators changed, not the kernels, and the failure says so.  A missing file or key fails; nothing skips.

`python tests/test_joint_fwd_dh_digests_gpu.py` prints the JSON to record (IA_LIB_PATH selects the library that computes it)."""
import contextlib
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "joint_fwd_dh_digests.json")
SEED = 7
FILL = 0xA5
JVP, DH_K = 272, 288
PS = (0.0, 0.2)
H192 = dict(B=2, T=33, U1=35, H=192, V=257, LD=264, blank=256, frames=[29, 18], labels=[34, 13])
FWD = {
    "f_h64_v5": dict(B=3, T=19, U1=11, H=64, V=5, LD=8, blank=0, frames=[19, 7, 1], labels=[10, 4, 0]),
    "f_h192_v257": H192,
    "f_v272": dict(B=1, T=16, U1=16, H=64, V=272, LD=272, blank=271, frames=[16], labels=[15]),
    "f_box": dict(H192, tensors="f_h192_v257", box_t=[33, 24], box_u=[35, 20]),
}
DH = {
    "h160_ld8": dict(B=5, T=19, U1=11, H=160, LD=8, frames=[19, 7, 1, 16, 3], labels=[10, 4, 0, 10, 7]),
    "h640_ld272": dict(B=3, T=37, U1=35, H=640, LD=272, frames=[37, 22, 9], labels=[34, 20, 5]),
    "h480_ld288": dict(B=2, T=16, U1=16, H=480, LD=288, frames=[16, 11], labels=[15, 8]),
    "h80_ld40": dict(B=2, T=9, U1=8, H=80, LD=40, frames=[9, 4], labels=[7, 2]),
}
FWD_WAVES = (4, 8)


def dh_waves(name):
    return (4, 10) if DH[name]["H"] % 32 == 0 else (4,)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def inputs():
    """Every CPU tensor the cases read, drawn in a fixed order from one generator."""
    gen = torch.Generator().manual_seed(20251)
    x = {}
    for name, s in FWD.items():
        if "tensors" in s:
            continue
        B, T, U1, H, V = s["B"], s["T"], s["U1"], s["H"], s["V"]
        x[f"f_{name}"] = torch.randn(B, T, H, generator=gen).half()
        x[f"g_{name}"] = torch.randn(B, U1, H, generator=gen).half()
        W = torch.zeros(JVP, H)
        W[:V] = torch.randn(V, H, generator=gen) * 0.05
        x[f"W_{name}"] = W.half()
        x[f"bias_{name}"] = torch.randn(V, generator=gen)
        lab = torch.randint(0, V - 1, (B, U1 - 1), generator=gen)     # V - 1 values that skip the blank
        x[f"labels_{name}"] = lab + (lab >= s["blank"]).long()
    for name, s in DH.items():
        B, T, U1, H, LD = s["B"], s["T"], s["U1"], s["H"], s["LD"]
        tl, ul = torch.tensor(s["frames"]), torch.tensor(s["labels"])
        live = (torch.arange(T).view(1, T, 1, 1) < tl.view(B, 1, 1, 1)) & (torch.arange(U1).view(1, 1, U1, 1) <= ul.view(B, 1, 1, 1))
        G = torch.randn(B, T, U1, LD, generator=gen) * 0.01
        x[f"G_{name}"] = (G * live).half().view(B * T * U1, LD).contiguous()
        Wt = torch.zeros(H, DH_K)
        Wt[:, :LD] = torch.randn(H, LD, generator=gen) * 0.05
        x[f"Wt_{name}"] = Wt.half()
        x[f"f_{name}"] = torch.randn(B, T, H, generator=gen).half()
        x[f"g_{name}"] = torch.randn(B, U1, H, generator=gen).half()
        assert bool(torch.isfinite(x[f"G_{name}"]).all())
    return x


@functools.lru_cache(maxsize=None)
def input_digests():
    return {k: sha(v) for k, v in inputs().items()}


def ws_layout(B, T, U1):
    """csrc/rnnt_ws.h: byte offsets of denom, PB, PL, PLa, the end of PLa, and the workspace size."""
    K = 1
    while 64 * K < U1 + 1:
        K <<= 1
    up = lambda n: (n + 255) // 256 * 256  # noqa: E731
    cells, side = B * T * U1, B * (T + U1 + 1 + 2 * 8) * 64 * K * 4
    o = [0]
    for n in (cells * 4, side, side, side, side, side, 2 * B * 4, cells * 16, (cells + 63) // 64):
        o.append(up(o[-1] + n))
    return o[0], o[1], o[2], o[3], o[4], o[-1]


@contextlib.contextmanager
def env(name, value):
    old = os.environ.get(name)
    os.environ[name] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old


def fwd_case(name, p, waves):
    from indic_cl_asr_amd import _lib
    L, ptr, x, s = _lib.lib(), _lib.ptr, inputs(), FWD[name]
    src = s.get("tensors", name)
    B, T, U1, H, V, LD = s["B"], s["T"], s["U1"], s["H"], s["V"], s["LD"]
    f, g, W, bias, lab = (x[f"{k}_{src}"].cuda() for k in ("f", "g", "W", "bias", "labels"))
    tl, ul = torch.tensor(s["frames"], dtype=torch.long).cuda(), torch.tensor(s["labels"], dtype=torch.long).cuda()
    bt = torch.tensor(s["box_t"], dtype=torch.long).cuda() if "box_t" in s else None
    bu = torch.tensor(s["box_u"], dtype=torch.long).cuda() if "box_u" in s else None
    o_denom, o_pb, o_pl, o_pla, o_end, nbytes = ws_layout(B, T, U1)
    assert nbytes == L.ia_rnnt_workspace_bytes(B, T, U1), "ws_layout no longer restates csrc/rnnt_ws.h"
    ws = torch.full((nbytes,), FILL, dtype=torch.uint8, device="cuda")
    logits = torch.full((B * T * U1 * LD * 2,), FILL, dtype=torch.uint8, device="cuda")
    with env("IA_JFWD_WAVES", waves):
        _lib.check(L.ia_joint_fwd_box(ptr(f), ptr(g), ptr(W), ptr(bias), ptr(lab), ptr(tl), ptr(ul), ptr(bt), ptr(bu), B, T, U1, H, V,
                                      s["blank"], p, SEED, ptr(logits), LD, ptr(ws), nbytes, _lib.stream_ptr()), "ia_joint_fwd_box")
    torch.cuda.synchronize()
    got = {"logits": sha(logits), "denom": sha(ws[o_denom:o_pb]), "PB": sha(ws[o_pb:o_pl]), "PL": sha(ws[o_pl:o_pla]),
           "PLa": sha(ws[o_pla:o_end])}
    costs = torch.full((B,), float("nan"), device="cuda")
    _lib.check(L.ia_rnnt_lattice(ptr(tl), ptr(ul), B, T, U1, 0.0, 1, ptr(costs), ptr(ws), nbytes, _lib.stream_ptr()), "ia_rnnt_lattice")
    torch.cuda.synchronize()
    got["costs"] = sha(costs)
    return got


def dh_case(name, out, p, waves):
    """out = "f32": fp32 d f / d g, zero_dead_df = 0; "bf16": only the bf16 images, zero_dead_df = 1."""
    from indic_cl_asr_amd import _lib
    L, ptr, x, s = _lib.lib(), _lib.ptr, inputs(), DH[name]
    B, T, U1, H, LD = s["B"], s["T"], s["U1"], s["H"], s["LD"]
    assert L.ia_joint_dh_k() == DH_K
    G, Wt, f, g = (x[f"{k}_{name}"].cuda() for k in ("G", "Wt", "f", "g"))
    tl, ul = torch.tensor(s["frames"], dtype=torch.long).cuda(), torch.tensor(s["labels"], dtype=torch.long).cuda()
    scr = torch.empty(L.ia_joint_dh_fused_scratch_bytes(B, T, U1, H), dtype=torch.uint8, device="cuda")
    dt = torch.float32 if out == "f32" else torch.bfloat16
    df = torch.full((B, T, H), float("nan"), dtype=dt, device="cuda")
    dg = torch.full((B, U1, H), float("nan"), dtype=dt, device="cuda")
    f32 = out == "f32"
    with env("IA_DH_WAVES", waves):
        _lib.check(L.ia_joint_dh_fused_ex(ptr(G), ptr(Wt), ptr(f), ptr(g), ptr(tl), ptr(ul), ptr(df) if f32 else None,
                                          ptr(dg) if f32 else None, None if f32 else ptr(df), None if f32 else ptr(dg),
                                          0 if f32 else 1, B, T, U1, H, LD, 0.125, p, SEED, ptr(scr), _lib.stream_ptr()),
                   "ia_joint_dh_fused_ex")
    torch.cuda.synchronize()
    return {"df": sha(df), "dg": sha(dg)}


CASES = {}
for _n in FWD:
    for _p in PS:
        for _w in FWD_WAVES:
            CASES[f"{_n}_p{_p}_w{_w}"] = functools.partial(fwd_case, _n, _p, _w)
for _n in DH:
    for _o in ("f32", "bf16"):
        for _p in PS:
            for _w in dh_waves(_n):
                CASES[f"{_n}_{_o}_p{_p}_w{_w}"] = functools.partial(dh_case, _n, _o, _p, _w)
# (case without its wave suffix, the suffixes recorded for it) for every case with two decompositions
PAIRS = sorted({k.rsplit("_w", 1)[0] for k in CASES if sum(c.rsplit("_w", 1)[0] == k.rsplit("_w", 1)[0] for c in CASES) == 2})


@functools.lru_cache(maxsize=None)
def golden():
    assert os.path.exists(GOLDEN), f"{GOLDEN} is missing: record it with `python tests/test_joint_fwd_dh_digests_gpu.py`"
    with open(GOLDEN) as f:
        return json.load(f)


def test_inputs_are_the_recorded_ones():
    assert "inputs" in golden(), "the inputs are not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernels"


@pytest.mark.parametrize("case_name", list(CASES))
def test_joint_fwd_dh_digests(case_name):
    assert "inputs" in golden() and case_name in golden().get("cases", {}), f"{case_name} is not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernels"
    got, want = CASES[case_name](), golden()["cases"][case_name]
    differing = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert not differing, f"{case_name}: {differing} differ from the recorded digests"


@pytest.mark.parametrize("stem", PAIRS)
def test_wave_decompositions_agree(stem):
    """csrc/joint_fwd.hip and csrc/joint_dh.hip: the wave decompositions of a kernel give the same bits (same products, same order of
    summation per output).  Held on the record, which the cases above hold the kernels to."""
    cases = golden().get("cases", {})
    recorded = [cases[k] for k in sorted(CASES) if k.rsplit("_w", 1)[0] == stem and k in cases]
    assert len(recorded) == 2, f"{stem}: both decompositions must be recorded"
    assert recorded[0] == recorded[1], f"{stem}: the two wave decompositions differ"


if __name__ == "__main__":
    record = {"inputs": input_digests(), "cases": {name: fn() for name, fn in CASES.items()}}
    print(json.dumps(record, indent=1, sort_keys=True))
