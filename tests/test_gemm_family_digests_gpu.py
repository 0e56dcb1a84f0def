"""Bit-identity anchor of the projection GEMM family (csrc/gemm_common.h, gemm_bf16.hip, gemm_big.hip, gemm_bnsilu.hip,
gemm_fp8.hip, gemm_mxfp8.hip): SHA-256 digests of every buffer an entry writes, recorded in tests/golden/gemm_family_digests.json.

The other tests of the family compare its kernels with each other (DMA against register-staged, fused against two launches) and
with fp64 references to a tolerance; kernels that share their staging and their main loop would pass the former together and a
changed summation order passes the latter.  This file pins the bits instead.  The epilogue is one function for all of them, so
the cases are not its cross product: they are the smallest shapes that reach every operand-staging path --

  register-staged bf16 kernel (IA_GEMM_DMA=0), 64 / 96 / 128-row tiles: 200 x 136 x 144 (ragged last row tile for all three, a
      second column tile with 8 live columns, two k-tiles and a 16-wide tail), 200 x 136 x 64 (one k-tile: no prefetch),
      70 x 128 x 128 (two k-tiles); each with the full epilogue and bare; GLU (N = 256) per tile size; outPre and act 3 / aux
  ia_gemm_bf16_ln: the 64 x 256 tile (8 weight vectors per thread), K = 144 and 64
  LDS-DMA kernel (K >= 512, 64-row tiles): 200 x 136 x 512, 70 x 128 x 576
  gemm_big_kernel (IA_GEMM_BIG=1): 300 x 256 x 128 and x 192 (two stages; three, which leaves the loop at its `break`)
  ia_subsample_conv2: 2 x 9 x 7 images (odd sizes: every padding edge), C = 24 (taps straddle k-tiles, K = 216 has a tail),
      C = 64 register-staged and by LDS-DMA
  ia_gemm_bnsilu_bf16 / _keep: 200 x 136 x 144 with fp32 batch sums, fixed-point batch sums and in eval mode
  ia_gemm_fp8: K = 144 (a k-tile and a 16-byte tail) and 256, activations 0 and 1;  ia_gemm_mxfp8: K = 128 and 256

Inputs are made on the CPU from one seeded generator, rounded to bf16 where the entry takes bf16, and never modified; the fp8
operands come out of the library's own quantisers and are digested with the outputs.  The digests of the inputs are recorded too
and checked first: when they differ, torch's generators changed, not the kernels, and the failure says so.  A missing file or
key fails; nothing skips.

`python tests/test_gemm_family_digests_gpu.py` prints the JSON to record (IA_LIB_PATH selects the library that computes it)."""
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

GOLDEN = os.path.join(ROOT, "tests", "golden", "gemm_family_digests.json")
SWITCHES = ("IA_GEMM_BM", "IA_GEMM_DMA", "IA_GEMM_BIG", "IA_CONV_DMA")
BF16_SHAPES = [(200, 136, 144), (200, 136, 64), (70, 128, 128)]
DMA_SHAPES = [(200, 136, 512), (70, 128, 576)]
BIG_SHAPES = [(300, 256, 128), (300, 256, 192)]
LN_SHAPES = [(200, 256, 144), (200, 256, 64)]
F8_SHAPES = [(200, 136, 144), (200, 136, 256)]
MX_SHAPES = [(200, 136, 128), (200, 136, 256)]
CONV = dict(B=2, T1=9, F1=7, N=136)
BS = (200, 136, 144)
P, SEED, ALPHA = 0.1, 3, 0.5


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def inputs():
    """Every CPU tensor the cases read, drawn in a fixed order from one generator."""
    g = torch.Generator().manual_seed(20240)
    x = {}

    def draw(name, shape, scale=1.0, shift=0.0, bf16=False):
        if name not in x:
            t = torch.randn(*shape, generator=g) * scale + shift
            x[name] = t.bfloat16() if bf16 else t
        return x[name]

    for M, N, K in BF16_SHAPES + DMA_SHAPES + BIG_SHAPES + LN_SHAPES + F8_SHAPES + MX_SHAPES + [(200, 256, 144)]:
        draw(f"a_{M}x{K}", (M, K), 0.5, bf16=True)
        draw(f"w_{N}x{K}", (N, K), 0.05, bf16=True)
        draw(f"bias_{N}", (N,))
        draw(f"res_{M}x{N}", (M, N))
    draw("aux_200x136", (200, 136), bf16=True)
    draw("ln_g", (256,), 0.2, 1.0)
    draw("ln_b", (256,), 0.2)
    for C in (24, 64):
        x[f"img_{C}"] = draw(f"img_{C}_raw", (CONV["B"] * CONV["T1"] * CONV["F1"], C), bf16=True).abs()   # (after a ReLU)
        del x[f"img_{C}_raw"]
        draw(f"w2_{C}", (CONV["N"], 9 * C), 0.05, bf16=True)
    M, N, K = BS
    z = draw("bn_z", (M, K), 1.5, 0.3)
    draw("bn_gamma", (K,), 0.1, 1.0)
    draw("bn_beta", (K,), 0.1)
    draw("bn_rm", (K,), 0.1)
    x["bn_rv"] = draw("bn_rv_raw", (K,), 0.1, 0.9).abs()
    del x["bn_rv_raw"]
    x["bn_sum"], x["bn_sumsq"] = z.sum(0).contiguous(), (z * z).sum(0).contiguous()
    # the fixed-point accumulators of ia_glu_dwconv_fixed: [copies][sum | sumsq][K] int64 in 2^-24 units; rows r, r + 8, .. in copy r
    zd = z.double()
    x["bn_fixed"] = torch.stack([torch.stack([(zd[r::8].sum(0) * 2.0 ** 24).round().long(), ((zd[r::8] ** 2).sum(0) * 2.0 ** 24).round().long()])
                                 for r in range(8)]).contiguous()
    return x


@functools.lru_cache(maxsize=None)
def input_digests():
    return {k: sha(v) for k, v in inputs().items()}


@contextlib.contextmanager
def switches(**env):
    """The IA_* switches of the dispatch (read per call by the library) set for one case and restored afterwards; the ones a case
    does not name are unset for it."""
    saved = {k: os.environ.get(k) for k in SWITCHES}
    try:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if env.get(k) is not None:
                os.environ[k] = str(env[k])
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def digests(**bufs):
    torch.cuda.synchronize()
    return {k: sha(v) for k, v in bufs.items()}


def case_bf16(M, N, K, variant, **env):
    """ia_gemm_bf16_ex2.  full: bias + SiLU + dropout + alpha + residual, fp32 and bf16 outputs; bare: bf16 output only; glu: act
    4; pre: outPre + ReLU; aux: act 3 against aux."""
    from indic_cl_asr_amd import _lib
    L, p, x = _lib.lib(), _lib.ptr, inputs()
    a, w = x[f"a_{M}x{K}"].cuda(), x[f"w_{N}x{K}"].cuda()
    bias, res = x[f"bias_{N}"].cuda(), x[f"res_{M}x{N}"].cuda()
    outF = torch.zeros(M, N, device="cuda")
    outH = torch.zeros(M, N // 2 if variant == "glu" else N, dtype=torch.bfloat16, device="cuda")
    pre = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    aux = x["aux_200x136"].cuda() if variant == "aux" else None
    none = (None, 0)
    tail = {"full": (p(bias), 1, P, SEED, ALPHA, p(res), N, p(outF), N, p(outH), N, *none, *none),
            "bare": (None, 0, 0.0, 0, 1.0, *none, *none, p(outH), N, *none, *none),
            "glu": (p(bias), 4, 0.0, 0, 1.0, *none, *none, p(outH), N // 2, *none, *none),
            "pre": (p(bias), 2, P, SEED, ALPHA, p(res), N, p(outF), N, p(outH), N, p(pre), N, *none),
            "aux": (p(bias), 3, P, SEED, ALPHA, p(res), N, p(outF), N, p(outH), N, *none, p(aux), N)}[variant]
    with switches(**env):
        _lib.check(L.ia_gemm_bf16_ex2(p(a), K, p(w), K, M, N, K, *tail, 0, _lib.stream_ptr()), "ia_gemm_bf16_ex2")
    return digests(outF=outF, outH=outH, outPre=pre)


def case_ln(M, N, K):
    from indic_cl_asr_amd import _lib
    L, p, x = _lib.lib(), _lib.ptr, inputs()
    a, w, bias = x[f"a_{M}x{K}"].cuda(), x[f"w_{N}x{K}"].cuda(), x[f"bias_{N}"].cuda()
    xr = x[f"res_{M}x{N}"].cuda()          # updated in place, as the blocks do
    g, b = x["ln_g"].cuda(), x["ln_b"].cuda()
    y = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    with switches():
        _lib.check(L.ia_gemm_bf16_ln(p(a), K, p(w), K, M, N, K, p(bias), P, SEED, ALPHA, p(xr), N, p(xr), N, p(g), p(b), 1e-5, p(y), N,
                                     _lib.stream_ptr()), "ia_gemm_bf16_ln")
    return digests(outF=xr, outH=y)


def case_conv2(C, **env):
    from indic_cl_asr_amd import _lib
    L, p, x = _lib.lib(), _lib.ptr, inputs()
    B, T1, F1, N = CONV["B"], CONV["T1"], CONV["F1"], CONV["N"]
    img, w2, b2 = x[f"img_{C}"].cuda(), x[f"w2_{C}"].cuda(), x[f"bias_{N}"].cuda()
    out = torch.zeros(B * ((T1 - 1) // 2 + 1) * ((F1 - 1) // 2 + 1), N, dtype=torch.bfloat16, device="cuda")
    with switches(**env):
        _lib.check(L.ia_subsample_conv2(p(img), B, T1, F1, C, p(w2), p(b2), N, p(out), _lib.stream_ptr()), "ia_subsample_conv2")
    return digests(out=out)


def case_bnsilu(mode):
    """Both entries (with and without the kept operand) in one case: train mode on fp32 sums or on the fixed-point sums, or eval."""
    from indic_cl_asr_amd import _lib
    L, p, x = _lib.lib(), _lib.ptr, inputs()
    M, N, K = BS
    z, w, bias = x["bn_z"].cuda(), x[f"w_{N}x{K}"].cuda(), x[f"bias_{N}"].cuda()
    gamma, beta = x["bn_gamma"].cuda(), x["bn_beta"].cuda()
    s1, s2, fixed = x["bn_sum"].cuda(), x["bn_sumsq"].cuda(), x["bn_fixed"].cuda()
    training = int(mode != "eval")
    sums = (None, None) if mode == "fixed" else (p(s1), p(s2))
    out = {}
    for keep in (False, True):
        rm, rv, nbt = x["bn_rm"].cuda(), x["bn_rv"].cuda(), torch.zeros(1, dtype=torch.long, device="cuda")
        xr = x[f"res_{M}x{N}"].cuda()
        y = torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
        kept = torch.zeros(M, K, dtype=torch.bfloat16, device="cuda")
        head = (p(z), K, M, *sums, p(gamma), p(beta), p(rm), p(rv), p(nbt), 0.1, 1e-5, training, p(w), K, M, N, K, p(bias), P, SEED, ALPHA,
                p(xr), N, p(xr), N, p(y), N, p(fixed) if mode == "fixed" else None)
        with switches():
            if keep:
                _lib.check(L.ia_gemm_bnsilu_bf16_keep(*head, p(kept), K, _lib.stream_ptr()), "ia_gemm_bnsilu_bf16_keep")
            else:
                _lib.check(L.ia_gemm_bnsilu_bf16(*head, _lib.stream_ptr()), "ia_gemm_bnsilu_bf16")
        tag = "keep_" if keep else ""
        out.update({tag + k: v for k, v in digests(outF=xr, outH=y, rm=rm, rv=rv, nbt=nbt, outA=kept).items()})
    return out


def case_fp8(M, N, K, act, mx):
    """ia_gemm_fp8 (per-row scales) or ia_gemm_mxfp8 (block scales) on operands from the library's quantisers."""
    from indic_cl_asr_amd import _lib
    from indic_cl_asr_amd.ops import fast
    L, p, x = _lib.lib(), _lib.ptr, inputs()
    a, w = x[f"a_{M}x{K}"].cuda(), x[f"w_{N}x{K}"].cuda()
    bias, res = x[f"bias_{N}"].cuda(), x[f"res_{M}x{N}"].cuda()
    outF, outH = torch.zeros(M, N, device="cuda"), torch.zeros(M, N, dtype=torch.bfloat16, device="cuda")
    (aq, asc), (wq, wsc) = (fast.quantize_mxfp8(t) if mx else fast.quantize_fp8_rows(t) for t in (a, w))
    tail = (M, N, aq.shape[1], p(bias), act, P, SEED, ALPHA, p(res), N, p(outF), N, p(outH), N, _lib.stream_ptr())
    with switches():
        if mx:
            _lib.check(L.ia_gemm_mxfp8(p(aq), aq.stride(0), p(asc), asc.stride(0), p(wq), wq.stride(0), p(wsc), wsc.stride(0), *tail),
                       "ia_gemm_mxfp8")
        else:
            _lib.check(L.ia_gemm_fp8(p(aq), aq.stride(0), p(asc), p(wq), wq.stride(0), p(wsc), *tail), "ia_gemm_fp8")
    return digests(outF=outF, outH=outH, aq=aq, a_scales=asc, wq=wq, w_scales=wsc)


def _cases():
    c = {}
    staged = dict(IA_GEMM_DMA=0)
    for bm in (64, 96, 128):
        for M, N, K in BF16_SHAPES:
            for variant in ("full", "bare"):
                c[f"bf16_bm{bm}_{M}x{N}x{K}_{variant}"] = functools.partial(case_bf16, M, N, K, variant, IA_GEMM_BM=bm, **staged)
        c[f"bf16_bm{bm}_200x256x144_glu"] = functools.partial(case_bf16, 200, 256, 144, "glu", IA_GEMM_BM=bm, **staged)
    for variant in ("pre", "aux"):
        c[f"bf16_bm64_200x136x144_{variant}"] = functools.partial(case_bf16, 200, 136, 144, variant, IA_GEMM_BM=64, **staged)
    for M, N, K in LN_SHAPES:
        c[f"bf16_ln_{M}x{N}x{K}"] = functools.partial(case_ln, M, N, K)
    for M, N, K in DMA_SHAPES:
        for variant in ("full", "bare"):
            c[f"bf16_dma_{M}x{N}x{K}_{variant}"] = functools.partial(case_bf16, M, N, K, variant, IA_GEMM_BM=64)
    for M, N, K in BIG_SHAPES:
        for variant in ("full", "bare"):
            c[f"bf16_big_{M}x{N}x{K}_{variant}"] = functools.partial(case_bf16, M, N, K, variant, IA_GEMM_BIG=1)
    c["conv2_c24"] = functools.partial(case_conv2, 24)
    c["conv2_c64_staged"] = functools.partial(case_conv2, 64, IA_CONV_DMA=0)
    c["conv2_c64_dma"] = functools.partial(case_conv2, 64, IA_CONV_DMA=1)
    for mode in ("train", "fixed", "eval"):
        c[f"bnsilu_{mode}"] = functools.partial(case_bnsilu, mode)
    for M, N, K in F8_SHAPES:
        for act in (0, 1):
            c[f"fp8_{M}x{N}x{K}_act{act}"] = functools.partial(case_fp8, M, N, K, act, False)
    for M, N, K in MX_SHAPES:
        c[f"mxfp8_{M}x{N}x{K}"] = functools.partial(case_fp8, M, N, K, 1, True)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def golden():
    assert os.path.exists(GOLDEN), f"{GOLDEN} is missing: record it with `python tests/test_gemm_family_digests_gpu.py`"
    with open(GOLDEN) as f:
        return json.load(f)


def test_inputs_are_the_recorded_ones():
    assert "inputs" in golden(), "the inputs are not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernels"


@pytest.mark.parametrize("case", list(CASES))
def test_gemm_family_digests(case):
    assert "inputs" in golden() and case in golden().get("cases", {}), f"{case} is not recorded"
    assert input_digests() == golden()["inputs"], "the INPUTS differ from the recorded ones (torch's generators), not the kernels"
    got, want = CASES[case](), golden()["cases"][case]
    differing = sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))
    assert not differing, f"{case}: {differing} differ from the recorded digests"


if __name__ == "__main__":
    record = {"inputs": input_digests(), "cases": {name: fn() for name, fn in CASES.items()}}
    print(json.dumps(record, indent=1, sort_keys=True))
