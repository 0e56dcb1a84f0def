"""Everything in front of the first Conformer block held to fp64 references (oracle/input_ref.py): the striding subsampling
stage by stage through the C ABI, the feature normalisation, the log-mel front ends and their dither noise.

Notation and bounds of tests/test_block_reference_gpu.py (its C = 4, FLOOR = 2^-20, _check, _dist and keep_mask are imported):
K = the kernel's result, E = exact math in fp64, F64 / F32 = the HIP path's bf16 rounding points emulated in fp64 / fp32
(rounding="kernel").  Every compared tensor is measured in relative L2 and max-abs distance.

Subsampling (csrc/gemm_bf16.hip conv1_relu_cl_kernel, ia_subsample_conv2 in both variants, the permuted Linear):
  (a) d(K, F64) <= C * d(F32, F64) + FLOOR   per stage, each stage on the KERNEL's own input (splice): conv1 on the features,
      conv2 on the kernel's o1, the Linear on the kernel's o2; and every bf16 output element within one bf16 ulp of F64's
      (+ FLOOR * max): fp32 summation noise can only move a value across one rounding boundary
  (b) d(K, E) <= 2 * d(F64, E) + FLOOR       the whole chain
Normalisation and log-mel have no bf16 stage: d(K, E) <= C * d(F32, E) + FLOOR with F32 = the reference's own fp32 arithmetic
on the CPU (input_ref.normalize / input_ref.log_mel run in fp32); mel energies relative to each frame's largest one (the scale
of tests/test_frontend_fft_gpu.py) and the log values themselves.  The worst ratios d(K, ref) / d(other, ref) are printed per
case.

Single-line faults these tests are written to catch: `f < Fm - 1` in conv1's bounds test, the `t1 < cT1` test dropped from the
conv2 gather, `len` for `len - 1` in the normaliser's variance, one bit of 0x68E31DA4 in ff_randn, alpha dropped from the
Linear's call, and the framing rule `n - win / 2` (one sample late for odd window lengths).
"""
import math

import numpy as np
import pytest
import torch

from oracle import input_ref as R
from test_block_reference_gpu import C, FLOOR, _check, _dist, keep_mask

pytestmark = pytest.mark.gpu

GUARD = 2.0 ** -24


def _report(log):
    for bound in ("(a)", "(b)", "(f32)"):
        for metric in ("L2", "max"):
            rows = [r for r in log if bound in r[0] and r[1] == metric]
            if rows:
                worst = max(rows, key=lambda r: r[2])
                print(f"worst {bound} {metric} ratio d(K, ref) / d(other, ref): {worst[2]:.3f} at {worst[0]}")


def _within_one_bf16_ulp(tag, K, F64):
    """|K - F64| <= the bf16 spacing at the larger of the two + FLOOR * max|F64|, element by element."""
    big = torch.maximum(K.abs(), F64.abs())
    _, e = torch.frexp(big)                                       # |v| = m 2^e, m in [0.5, 1): bf16 spacing 2^(e - 8)
    ulp = torch.where(big > 0, torch.ldexp(torch.ones_like(big), e - 8), torch.zeros_like(big))
    over = (K - F64).abs() - ulp - FLOOR * float(F64.abs().max())
    assert float(over.max()) <= 0, (tag, "more than one bf16 ulp", int((over > 0).sum()), float(over.max()))


# ---------------------------------------------------------------------------------------------------- subsampling: C ABI
def _k_conv1(x_btf, w, b):
    """ia_subsample_conv1 on x [B, T, F] (handed over as the [B, F, T] tensor the preprocessor emits) -> [B, T1, F1, C] bf16."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    B, Tm, Fm = x_btf.shape
    Cc = w.shape[0]
    T1, F1 = (Tm - 1) // 2 + 1, (Fm - 1) // 2 + 1
    xk = x_btf.float().transpose(1, 2).contiguous().cuda()
    wk, bk = w.float().reshape(Cc, 9).contiguous().cuda(), b.float().contiguous().cuda()
    o = torch.empty(B, T1, F1, Cc, dtype=torch.bfloat16, device="cuda")
    _lib.check(L.ia_subsample_conv1(_lib.ptr(xk), B, Fm, Tm, Cc, _lib.ptr(wk), _lib.ptr(bk), _lib.ptr(o), _lib.stream_ptr()), "conv1")
    torch.cuda.synchronize()
    return o


def _k_conv2(o1, w, b):
    """ia_subsample_conv2 on channels-last o1 [B, T1, F1, C] bf16 (device) -> [B, T2, F2, N] bf16."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    B, T1, F1, Cc = o1.shape
    N = w.shape[0]
    T2, F2 = (T1 - 1) // 2 + 1, (F1 - 1) // 2 + 1
    wk = w.float().permute(0, 2, 3, 1).reshape(N, 9 * Cc).to(torch.bfloat16).contiguous().cuda()
    bk = b.float().contiguous().cuda()
    o = torch.empty(B, T2, F2, N, dtype=torch.bfloat16, device="cuda")
    _lib.check(L.ia_subsample_conv2(_lib.ptr(o1), B, T1, F1, Cc, _lib.ptr(wk), _lib.ptr(bk), N, _lib.ptr(o), _lib.stream_ptr()), "conv2")
    torch.cuda.synchronize()
    return o


#          name           C    Fm  B  Tm
CONV1 = [("c8_ppb256", 8, 80, 2, 5),          # one channel group: 256 pixel groups per workgroup pass
         ("c144_live252", 144, 81, 2, 4),     # 252 of 256 threads live; last feature group alone (F1 = 41)
         ("c256_f7", 256, 7, 3, 3),           # F1 = 4: one full feature group
         ("c144_f1", 144, 1, 2, 2),           # a single feature
         ("c8_t1", 8, 81, 1, 1),              # a single frame
         ("c256_mid", 256, 80, 2, 77),        # more than one workgroup, partial last pass
         ("c2048_grid_stride", 2048, 2, 4, 4203)]   # 8408 pixel groups on a grid capped at 8192: second trip of the loop


@pytest.mark.parametrize("case", CONV1, ids=[c[0] for c in CONV1])
def test_conv1_matches_rounding_faithful_reference(case):
    name, Cc, Fm, B, Tm = case
    g = torch.Generator().manual_seed(Cc + Fm + Tm)
    x = torch.randn(B, Tm, Fm, generator=g)
    w = torch.randn(Cc, 1, 3, 3, generator=g) / 3.0
    b = torch.randn(Cc, generator=g) * 0.1
    K = _k_conv1(x, w, b).double().cpu()
    E = R.conv1(x.double(), w.double(), b.double(), None)
    F64 = R.conv1(x.double(), w.double(), b.double(), "kernel")
    F32 = R.conv1(x, w, b, "kernel").double()
    assert K.shape == E.shape
    log = []
    _check(f"{name}:o1:(a)", K, F64, F32, C, log=log)
    _within_one_bf16_ulp(name, K, F64)
    _check(f"{name}:o1:(b)", K, E, F64, 2.0, log=log)
    _report(log)


#          name          C    N    B  T1   F1         M = B * T2 * F2
CONV2 = [("m1", 8, 8, 1, 1, 1),                     # 1
         ("m1_dma", 64, 256, 1, 1, 1),              # 1
         ("m127", 64, 256, 1, 253, 1),              # 127
         ("m128", 144, 144, 2, 127, 2),             # 128
         ("m128_even_t1", 256, 256, 2, 128, 2),     # 128, no padding row at the bottom
         ("m129", 176, 176, 1, 85, 5),              # 129
         ("t5_f40", 256, 256, 2, 5, 40),
         ("t4_f41", 256, 256, 2, 4, 41),
         ("t2_f41", 64, 256, 3, 2, 41),
         ("t3_f40", 144, 144, 2, 3, 40),
         ("t4_f2", 176, 176, 3, 4, 2)]


@pytest.mark.parametrize("case", CONV2, ids=[c[0] for c in CONV2])
def test_conv2_matches_rounding_faithful_reference(case, monkeypatch):
    """Random signed bf16 images straight into ia_subsample_conv2; where C % 64 == 0 both IA_CONV_DMA settings, bit-equal.
    These edge shapes have 8 .. 33 k outputs, where fp32 summation noise flips zero, one or two bf16 roundings and a ratio of
    two such counts says nothing.  So the operands are random DYADIC numbers -- image in multiples of 1/8 in [-2, 2), weights
    in multiples of 1/64 in [-1/8, 1/8], bias in multiples of 1/512: every product is a multiple of 2^-9 and every partial sum
    of the <= 2304 products stays below 2^10, 19 significant bits -- so fp32 accumulation is EXACT in any order, F32 equals
    F64, and (a) holds the kernel to F64 within FLOOR: a tap dropped or read at an image edge, or a store that does not round
    to nearest even, has nowhere to hide.  Realistic operands, and with them the summation noise, run through conv2 in
    test_subsampling_chain_stage_by_stage (0.3 M outputs at d = 144 and 256)."""
    name, Cc, N, B, T1, F1 = case
    g = torch.Generator().manual_seed(Cc + T1 + F1)
    x = (torch.randint(-16, 16, (B, T1, F1, Cc), generator=g).float() / 8.0).to(torch.bfloat16)
    w = torch.randint(-8, 9, (N, Cc, 3, 3), generator=g).float() / 64.0
    b = torch.randint(-64, 65, (N,), generator=g).float() / 512.0
    outs = []
    for mode in (("0", "1") if Cc % 64 == 0 else ("0",)):
        monkeypatch.setenv("IA_CONV_DMA", mode)
        outs.append(_k_conv2(x.cuda(), w, b).cpu())
    monkeypatch.delenv("IA_CONV_DMA")
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1]), "the LDS-DMA variant differs from the register-staged one"
    K = outs[0].double()
    xd = x.double()
    E = R.conv2(xd, w.double(), b.double(), None)
    F64 = R.conv2(xd, w.double(), b.double(), "kernel")
    F32 = R.conv2(x.float(), w, b, "kernel").double()
    assert torch.equal(F32, F64) and torch.equal(w.to(torch.bfloat16).float(), w)     # exact operands, exact fp32 sums
    assert K.shape == E.shape and K.shape[0] * K.shape[1] * K.shape[2] == B * ((T1 - 1) // 2 + 1) * ((F1 - 1) // 2 + 1)
    log = []
    _check(f"{name}:o2:(a)", K, F64, F32, C, log=log)
    _within_one_bf16_ulp(name, K, F64)
    _check(f"{name}:o2:(b)", K, E, F64, 2.0, log=log)
    _report(log)


#          name      C = d  feat_in  B  Tm
CHAIN = [("d144", 144, 80, 2, 200),
         ("d256", 256, 80, 3, 77),
         ("d176_t5", 176, 80, 1, 5),
         ("d64_t1", 64, 64, 2, 1),
         ("d256_t2", 256, 80, 2, 2)]


@pytest.mark.parametrize("p", [0.0, 0.1], ids=["p0", "p0.1"])
@pytest.mark.parametrize("case", CHAIN, ids=[c[0] for c in CHAIN])
def test_subsampling_chain_stage_by_stage(case, p, monkeypatch):
    """ops/fast.conv_subsampling with the positional encoding's alpha = sqrt(d) and dropout in the Linear's epilogue.  o1 and o2
    come from the same two C calls made directly (the GEMM's input is captured and must be bit-equal to that o2); the mask is
    restated by keep_mask.  Dropped elements are exactly 0, kept ones obey (a); the whole chain obeys (b)."""
    from indic_cl_asr_amd.encoder import ConvSubsampling
    from indic_cl_asr_amd.ops import fast
    name, d, feat_in, B, Tm = case
    torch.manual_seed(d + Tm)
    m = ConvSubsampling(feat_in, d, d)
    assert fast.subsample_supported(d, d, feat_in)
    x = torch.randn(B, Tm, feat_in)
    seed = 0x5EED0000 + d
    alpha = float(np.float32(math.sqrt(d)))                       # the C ABI takes alpha as a float
    T2 = ((Tm - 1) // 2 + 1 - 1) // 2 + 1
    mask = keep_mask(seed, B * T2, d, p).view(B, T2, d)

    md = m.cuda()
    cap = {}
    orig = fast.gemm

    def spy(a, w, *args, **kw):
        cap["o2"] = a.detach().clone()
        return orig(a, w, *args, **kw)

    monkeypatch.setattr(fast, "gemm", spy)
    with torch.no_grad():
        Ky = fast.conv_subsampling(x.transpose(1, 2).contiguous().cuda(), md.conv[0], md.conv[2], md.out, alpha=alpha,
                                   dropout_p=p, seed=seed)
    torch.cuda.synchronize()
    monkeypatch.setattr(fast, "gemm", orig)
    Ko1 = _k_conv1(x, m.conv[0].weight.detach().cpu(), m.conv[0].bias.detach().cpu())
    Ko2 = _k_conv2(Ko1, m.conv[2].weight.detach().cpu(), m.conv[2].bias.detach().cpu())
    assert torch.equal(cap["o2"].reshape(-1), Ko2.reshape(-1))
    assert Ky.shape == (B, T2, d)
    K = [Ko1.double().cpu(), Ko2.double().cpu(), Ky.double().cpu()]

    P64, P32 = R.params_of(m, torch.float64), R.params_of(m, torch.float32)
    E = R.subsampling(x.double(), P64, None, alpha, mask)
    F64 = R.subsampling(x.double(), P64, "kernel", alpha, mask)
    sp = {"o1": K[0], "o2": K[1]}
    F64s = R.subsampling(x.double(), P64, "kernel", alpha, mask, splice=sp)
    F32s = [t.double() for t in R.subsampling(x, P32, "kernel", alpha, mask, splice=sp)]
    log = []
    for i, st in enumerate(("o1", "o2", "y")):
        _check(f"{name}:{st}:(a)", K[i], F64s[i], F32s[i], C, log=log)
        if st != "y":
            _within_one_bf16_ulp(f"{name}:{st}", K[i], F64s[i])
        _check(f"{name}:{st}:(b)", K[i], E[i], F64[i], 2.0, log=log)
    dropped = mask == 0
    assert torch.equal(K[2][dropped], torch.zeros(int(dropped.sum()), dtype=torch.float64))
    if p > 0:
        assert 0.85 < 1.0 - float(dropped.double().mean()) < 0.95
        assert float((K[2] != 0).double().mean()) > 0.8
    else:
        assert not dropped.any()
    _report(log)


# ---------------------------------------------------------------------------------------------------- normalisation
def _logmel_shaped(B, F_, T, lens, seed):
    """Mean about -10, std about 2; one feature row constant over the valid frames (-10.25: every partial sum is exact in
    fp32, so the std is exactly 0 and eps decides the result)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F_, T, generator=g) * 2.0 - 10.0 + torch.randn(B, F_, 1, generator=g)
    if F_ > 3:
        for b, n in enumerate(lens):
            x[b, 3, :n] = -10.25
    return x


def _compare_normalize(name, x, lens, spans=None, mask_value=0.0):
    from indic_cl_asr_amd import ops
    lens_t = torch.tensor(lens)
    dspans = None if spans is None else tuple(s.int().cuda() for s in spans)
    K = ops.normalize_mask(x.cuda(), lens_t.cuda(), dspans, eps=1e-5, mask_value=mask_value).double().cpu()
    E = R.normalize(x.double(), lens_t, 1e-5, spans, mask_value)
    F32 = R.normalize(x, lens_t, 1e-5, spans, mask_value).double()
    valid = (torch.arange(x.shape[2])[None, :] < lens_t[:, None]).unsqueeze(1).expand_as(x)
    filled = torch.zeros_like(valid)
    if spans is not None:
        filled = torch.isinf(R.normalize(x.double(), lens_t, 1e-5, spans, float("inf")))
        assert filled.any() and torch.equal(K[filled], torch.full((int(filled.sum()),), mask_value, dtype=torch.float64))
    beyond = ~valid & ~filled
    assert torch.equal(K[beyond], torch.zeros(int(beyond.sum()), dtype=torch.float64)), "frames beyond seq_len must be exactly 0"
    nan = torch.isnan(E)
    assert torch.equal(torch.isnan(K), nan), "NaN exactly where torch.std of one frame gives NaN"
    sel = valid & ~filled & ~nan
    log = []
    if sel.any():
        _check(f"{name}:norm:(f32)", K[sel], E[sel], F32[sel], C, log=log)
        if x.shape[1] > 3:
            assert torch.equal(K[:, 3][sel[:, 3]], torch.zeros(int(sel[:, 3].sum()), dtype=torch.float64))   # the constant row
    _report(log)
    return K, nan


#         name       F   T     lens
NORM = [("t76", 80, 76, (76, 40, 2)),
        ("t255", 80, 255, (255, 129, 3)),
        ("t256", 80, 256, (256, 255, 64)),
        ("t257", 80, 257, (257, 256, 130)),            # the second value of thread 0
        ("t4096", 80, 4096, (4096, 4095, 257)),        # all 16 values per thread
        ("f1_t3", 1, 3, (3, 2))]


@pytest.mark.parametrize("case", NORM, ids=[c[0] for c in NORM])
def test_normalize_matches_fp64(case):
    name, F_, T, lens = case
    x = _logmel_shaped(len(lens), F_, T, lens, T)
    _compare_normalize(name, x, lens)


def test_normalize_of_one_frame_is_nan_where_the_reference_is():
    lens = (5, 1, 3)
    x = _logmel_shaped(3, 80, 5, lens, 5)
    K, nan = _compare_normalize("len1", x, lens)
    assert nan[1, :, 0].all() and int(nan.sum()) == 80
    assert torch.equal(K[1, :, 1:], torch.zeros(80, 4, dtype=torch.float64))


def test_normalize_with_spans_and_mask_value():
    lens = (257, 256, 130)
    x = _logmel_shaped(3, 80, 257, lens, 258)
    fs = torch.tensor([[3, 70], [0, 79], [40, 40]]); fw = torch.tensor([[5, 10], [1, 1], [0, 7]])
    ts = torch.tensor([[0, 100, 250], [255, 10, 10], [120, 129, 200]]); tw = torch.tensor([[4, 30, 20], [5, 0, 3], [20, 1, 9]])
    _compare_normalize("spans", x, lens, spans=(fs, fw, ts, tw), mask_value=-1.0)


# ---------------------------------------------------------------------------------------------------- log-mel
def _fb(n_mels, n_fft=512, sr=16000):
    from indic_cl_asr_amd.features import mel_filterbank_slaney
    return torch.as_tensor(mel_filterbank_slaney(sr, n_fft, n_mels)).float()


def _signal(B, L, seed, quiet=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, generator=g) * 0.1
    if quiet:
        x[0, : L // 3] *= 1e-3                                    # a quiet stretch: small powers next to large ones
    return x


def _compare_logmel(tag, K, E, F32, log):
    assert K.shape == E.shape and not torch.isnan(K).any()
    melE = E.exp()
    scale = melE.amax(dim=1, keepdim=True)
    _check(f"{tag}:mel:(f32)", K.exp() / scale, melE / scale, F32.exp() / scale, C, log=log)
    _check(f"{tag}:log:(f32)", K, E, F32, C, log=log)


def _run_logmel(tag, x, window, fb, n_fft, hop, log, monkeypatch, front_ends=("fft", "gemm"), dither=0.0, seed=0, noise=None):
    from indic_cl_asr_amd.ops import frontend
    n64 = None if noise is None else torch.from_numpy(noise)
    E = R.log_mel(x.double(), window, fb, n_fft, hop, 0.97, GUARD, noise=n64)
    F32 = R.log_mel(x, window, fb, n_fft, hop, 0.97, GUARD, noise=None if noise is None else n64.float()).double()
    wd, fd, xd = window.cuda(), fb.cuda(), x.cuda()
    for fe in front_ends:
        if fe == "gemm":
            monkeypatch.setenv("IA_FRONTEND", "gemm")
        else:
            monkeypatch.delenv("IA_FRONTEND", raising=False)
        K = frontend.log_mel(xd, wd, fd, n_fft=n_fft, hop=hop, preemph=0.97, dither=dither, seed=seed, log_guard=GUARD)
        _compare_logmel(f"{tag}:{fe}", K.double().cpu(), E, F32, log)
    monkeypatch.delenv("IA_FRONTEND", raising=False)


@pytest.mark.parametrize("win", [400, 320, 512, 399])
@pytest.mark.parametrize("L", [257, 330, 1279, 1280, 1281, 4001])
def test_logmel_matches_fp64_on_both_front_ends(L, win, monkeypatch):
    """L = 257: the shortest signal torch.stft accepts at n_fft = 512; 1279 / 1280 / 1281: 8 frames, then 9 (the FFT kernel's
    8-frame tile edge, an even and an odd count for its two-frames-per-transform pairing); win = 399: an odd window length.
    n_mels = 128 does not fit the 128 filterbank chunks and runs the GEMM front end either way."""
    window = torch.hann_window(win, periodic=False)
    x = _signal(2, L, L + win)
    log = []
    for n_mels in (80, 128):
        _run_logmel(f"L{L}:w{win}:m{n_mels}", x, window, _fb(n_mels), 512, 160, log, monkeypatch)
    _report(log)


def test_logmel_of_an_all_zero_utterance_is_log_guard(monkeypatch):
    x = _signal(2, 1280, 9)
    x[0] = 0.0
    log = []
    _run_logmel("zero", x, torch.hann_window(400, periodic=False), _fb(80), 512, 160, log, monkeypatch)
    _report(log)
    E = R.log_mel(x.double(), torch.hann_window(400, periodic=False), _fb(80), 512, 160, 0.97, GUARD)
    assert torch.equal(E[0], torch.full_like(E[0], math.log(GUARD)))


def test_logmel_gemm_front_end_at_n_fft_1024_win_551(monkeypatch):
    """The 22.05 kHz recipe: n_fft = 1024 (GEMM front end only) with an odd window."""
    from indic_cl_asr_amd import _lib
    assert not _lib.lib().ia_feat_logmel_fft_supported(1024, 551, 80, 0)
    log = []
    _run_logmel("n1024:w551", _signal(2, 2999, 551), torch.hann_window(551, periodic=False), _fb(80, 1024, 22050), 1024, 220, log,
                monkeypatch, front_ends=("fft",))                 # IA_FRONTEND unset: log_mel itself must pick the GEMM path
    _report(log)


def _chunked_fb(widths):
    """One filter per entry, `widths[i]` consecutive non-zero bins starting at 3 i: ceil(width / 8) chunks each."""
    g = torch.Generator().manual_seed(len(widths) + sum(widths))
    fb = torch.zeros(len(widths), 257)
    for i, w in enumerate(widths):
        fb[i, 3 * i: 3 * i + w] = torch.rand(w, generator=g) * 0.05 + 0.01
    return fb


@pytest.mark.parametrize("widths,fft", [([16] * 64, True), ([17] + [16] * 63, False)], ids=["128_chunks", "129_chunks"])
def test_logmel_filterbank_chunk_limit(widths, fft, monkeypatch):
    """A filterbank that cuts into exactly 128 chunks of 8 bins stays on the FFT front end; 129 chunks fall back to the GEMMs."""
    from indic_cl_asr_amd import _lib
    from indic_cl_asr_amd.ops import frontend
    fb = _chunked_fb(widths)
    L_ = _lib.lib()
    calls = {"fft": 0, "gemm": 0}
    o_fft, o_frames = L_.ia_feat_logmel_fft, L_.ia_feat_frames

    def c_fft(*a):
        calls["fft"] += 1
        return o_fft(*a)

    def c_frames(*a):
        calls["gemm"] += 1
        return o_frames(*a)

    monkeypatch.setattr(L_, "ia_feat_logmel_fft", c_fft)
    monkeypatch.setattr(L_, "ia_feat_frames", c_frames)
    tables = frontend._fft_tables(torch.hann_window(400, periodic=False), fb, 512, "cpu")
    assert (tables is not None) == fft and (tables is None or tables[4] == 128)
    log = []
    _run_logmel("chunks", _signal(2, 1281, 3), torch.hann_window(400, periodic=False), fb, 512, 160, log, monkeypatch,
                front_ends=("fft",))
    assert calls == ({"fft": 1, "gemm": 0} if fft else {"fft": 0, "gemm": 1})
    _report(log)


# ---------------------------------------------------------------------------------------------------- dither
def test_preemph_kernel_noise_equals_the_replica():
    """ia_feat_preemph on x = 0 with dither = 1 and preemph = 0 returns the noise itself.  1e-4 absolute: at the recipes' dither
    of 1e-5 that is 1e-9 on a sample, below the fp32 spacing of +-0.1-scale audio; what it allows is the hardware log / cos
    (csrc/frontend_fft.hip ff_randn: __logf, __cosf) against the replica's fp64 Box-Muller.  A wrong hash constant or swapped
    uniforms give O(1) errors."""
    from indic_cl_asr_amd import _lib
    L_ = _lib.lib()
    B, L, seed = 3, (1 << 18) + 3, 0xC0FFEE
    x = torch.zeros(B, L, device="cuda")
    y = torch.empty_like(x)
    _lib.check(L_.ia_feat_preemph(_lib.ptr(x), B, L, 0.0, 1.0, seed, _lib.ptr(y), _lib.stream_ptr()), "ia_feat_preemph")
    torch.cuda.synchronize()
    want = R.randn_replica(seed, B, L)
    err = np.abs(y.cpu().numpy().astype(np.float64) - want)
    print(f"noise: max |kernel - replica| = {err.max():.3e}")
    assert err.max() < 1e-4


def test_logmel_with_dither_matches_the_replicas_noise(monkeypatch):
    """log_mel(dither = 1e-3, seed) on each front end (ff_randn in the pre-emphasis pass, fe_randn in the framing kernel) against
    input_ref.log_mel(noise = 1e-3 * replica): the same bound as without dither."""
    B, L, seed = 2, 4001, 77
    noise = 1e-3 * R.randn_replica(seed, B, L)
    log = []
    _run_logmel("dither", _signal(B, L, 5, quiet=False), torch.hann_window(400, periodic=False), _fb(80), 512, 160, log, monkeypatch,
                dither=1e-3, seed=seed, noise=noise)
    _report(log)
