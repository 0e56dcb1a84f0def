"""csrc/attention_flash.hip under its local span (local rel-pos attention forward: the key-tile loop on the band |i - j| <= w) against an
fp64 restatement of the reference's RelPositionMultiHeadAttentionLongformer on the kernel's bf16 inputs, against the full
kernel where the window covers everything, and through the encoder (native prefix executor, per-op chain, transcribe, align).

Tolerances are those of the tests of the full kernel and of the encoder's two bf16 paths: the arithmetic is the same.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def _inputs(B, T, H, dk, rows, seed=0, lens=None):
    g = torch.Generator().manual_seed(seed)
    d = H * dk
    qkv = (torch.randn(B * T, 3 * d, generator=g) * 0.8).bfloat16().cuda()
    pl = (torch.randn(rows, d, generator=g) * 0.8).bfloat16().cuda()
    bu = (torch.randn(H, dk, generator=g) * 0.3).cuda()
    bv = (torch.randn(H, dk, generator=g) * 0.3).cuda()
    return qkv, pl, bu, bv, torch.tensor(lens if lens is not None else [T] * B, dtype=torch.int64).cuda()


def _reference(qkv, pl, bu, bv, lens, B, T, H, dk, w):
    """ctx[b,i,h,:] = sum_j softmax_j(((q_i+u).k_j + (q_i+v).p[w-i+j]) / sqrt(dk)) v_j over |i-j| <= w, j < len; 0 for i >= len.
    q+u and q+v rounded to bf16 as the kernel's operands are (tests/test_attention_flash_gpu.py::_reference)."""
    d = H * dk
    x = qkv.double().view(B, T, 3, H, dk)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)   # [B,H,T,dk]
    p = pl.double()[:2 * w + 1].view(2 * w + 1, H, dk).permute(1, 0, 2)                            # [H,2w+1,dk]
    qu = (q + bu.double()[None, :, None, :]).bfloat16().double()
    qv = (q + bv.double()[None, :, None, :]).bfloat16().double()
    ac = qu @ k.transpose(-1, -2)
    i = torch.arange(T, device=qkv.device)[:, None]; j = torch.arange(T, device=qkv.device)[None, :]
    band = (i - j).abs() <= w
    o = torch.zeros(B, H, T, dk, dtype=torch.float64, device=qkv.device)
    for h in range(H):    # (per head: the [B,T,2w+1] position scores of w = 1000 stay small)
        full = qv[:, h] @ p[h].t()                                                                  # [B,T,2w+1]
        bd = full.gather(-1, (w - i + j).clamp(0, 2 * w).expand(B, T, T))
        s = (ac[:, h] + bd) / math.sqrt(dk)
        ok = band[None] & (j[None] < lens[:, None, None])
        s = s.masked_fill(~ok, float("-inf"))
        o[:, h] = torch.softmax(s, -1) @ v[:, h]
    qvalid = (torch.arange(T, device=qkv.device)[None, :] < lens[:, None])[:, None, :, None]
    o = torch.where(qvalid, o, torch.zeros_like(o))
    return o.transpose(1, 2).reshape(B * T, d)


SHAPES = [
    (2, 130, 2, 64, 4, [130, 70]),        # w < 16; queries with an empty tile; len inside a tile
    (1, 64, 1, 64, 1, [64]),              # smallest window
    (1, 65, 2, 48, 64, [65]),             # w = T-1; zero-padded head rows
    (3, 200, 4, 36, 16, [200, 129, 1]),   # dk = 36; len = 1
    (2, 300, 2, 64, 64, [300, 191]),      # the aligner's window; three key tiles
    (2, 321, 1, 64, 100, [321, 64]),      # w not a multiple of 16; len on a tile boundary
    (2, 700, 8, 64, 128, [700, 500]),     # w = 128; tiles skipped on both sides; mask-free interior tiles
    (1, 50, 2, 8, 1000, [50]),            # w >> T
]


@pytest.mark.parametrize("B,T,H,dk,w,lens", SHAPES)
def test_local_attention_matches_fp64_restatement(B, T, H, dk, w, lens):
    from indic_cl_asr_amd.ops import fast
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * w + 1, seed=T + dk + w, lens=lens)
    ref = _reference(qkv, pl, bu, bv, ln, B, T, H, dk, w)
    assert fast.attention_local_supported(T, dk, w)
    ctx = fast.relpos_attention_local(qkv, pl, bu, bv, ln, B, T, H, dk, w)
    assert torch.isfinite(ctx).all()
    out = ctx.double()
    err, scale = (out - ref).abs().max().item(), ref.abs().max().item()
    print(f"(B,T,H,dk,w)=({B},{T},{H},{dk},{w}) lens={lens}: err {err:.3e}, max|ref| {scale:.3f}, bound {2e-2 * scale + 1e-3:.3e}")
    assert err <= 2e-2 * scale + 1e-3, (err, scale)                      # bf16 band, bf16 probabilities
    for b in range(B):                                                  # padded queries are exactly zero
        n = int(ln[b])
        if n < T:
            assert out.view(B, T, -1)[b, n:].abs().max().item() == 0.0


@pytest.mark.parametrize("B,T,H,dk,lens", [(2, 200, 2, 64, [200, 129]), (2, 126, 4, 36, [126, 5])])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_wide_window_gives_the_full_kernels_bits(B, T, H, dk, lens, p):
    """A window >= T-1 admits every key.  The local kernel shares the full kernel's loop -- the same staging, MFMA order, score
    arithmetic, online-softmax update and dropout hash; the band mask removes nothing and the all-masked guard never fires for a
    query that has a key -- so the outputs are compared with torch.equal, not with the 2e-2 bound of the cross-check in
    tests/test_attention_flash_gpu.py.  w = T-1 reads the same 2T-1-row table; w > T-1 reads it as the centre of a longer one."""
    from indic_cl_asr_amd.ops import fast
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=11 + T, lens=lens)
    full = fast.relpos_attention_flash(qkv, pl, bu, bv, ln, B, T, H, dk, dropout_p=p, seed=5)
    loc = fast.relpos_attention_local(qkv, pl, bu, bv, ln, B, T, H, dk, T - 1, dropout_p=p, seed=5)
    diff = (loc.float() - full.float()).abs().max().item()
    print(f"T={T} dk={dk} p={p}: max |local(w=T-1) - full| = {diff:.3e} (max|full| {full.float().abs().max().item():.3f})")
    assert torch.equal(loc, full)
    extra = 40                                                           # w = T-1+40: 40 more rows on either side of the table
    g = torch.Generator().manual_seed(1)
    pad = lambda: (torch.randn(extra, H * dk, generator=g) * 0.8).bfloat16().cuda()
    longer = torch.cat([pad(), pl, pad()], 0).contiguous()
    loc2 = fast.relpos_attention_local(qkv, longer, bu, bv, ln, B, T, H, dk, T - 1 + extra, dropout_p=p, seed=5)
    assert torch.equal(loc2, full)


def test_local_attention_dropout_is_deterministic():
    from indic_cl_asr_amd.ops import fast
    B, T, H, dk, w = 2, 200, 2, 64, 16
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * w + 1, seed=9, lens=[200, 150])
    base = fast.relpos_attention_local(qkv, pl, bu, bv, ln, B, T, H, dk, w)
    d1 = fast.relpos_attention_local(qkv, pl, bu, bv, ln, B, T, H, dk, w, dropout_p=0.25, seed=5)
    d2 = fast.relpos_attention_local(qkv, pl, bu, bv, ln, B, T, H, dk, w, dropout_p=0.25, seed=5)
    d3 = fast.relpos_attention_local(qkv, pl, bu, bv, ln, B, T, H, dk, w, dropout_p=0.25, seed=6)
    assert torch.equal(d1, d2) and not torch.equal(d1, d3) and not torch.equal(d1, base)
    assert torch.isfinite(d1).all() and d1.view(B, T, -1)[1, 150:].abs().max().item() == 0.0


def test_local_attention_argument_validation():
    from indic_cl_asr_amd import _lib
    from indic_cl_asr_amd.ops import fast
    L = _lib.lib()
    B, T, H, dk, w = 1, 64, 1, 64, 4
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * w + 1)
    ctx = torch.full((B * T, H * dk), 7.0, dtype=torch.bfloat16, device="cuda")
    P = _lib.ptr
    call = lambda *a: L.ia_relpos_attention_local(*a, _lib.stream_ptr())
    assert call(P(qkv), P(pl), P(bu), P(bv), P(ln), B, T, H, dk, 0, 0.0, 0, P(ctx)) == -1          # window <= 0: IA_INVALID_VALUE
    assert call(P(qkv), P(pl), P(bu), P(bv), P(ln), B, T, H, dk, -3, 0.0, 0, P(ctx)) == -1
    assert call(P(qkv), P(pl), P(bu), P(bv), P(ln), B, T, 1, 68, w, 0.0, 0, P(ctx)) == -4          # dk > 64: IA_UNSUPPORTED
    assert call(P(qkv), P(pl), P(bu), P(bv), P(ln), B, T, 1, 30, w, 0.0, 0, P(ctx)) == -4          # dk no multiple of 4
    assert call(P(qkv), P(pl), P(bu), P(bv), P(ln), B, T, H, dk, w, 1.0, 0, P(ctx)) == -1          # dropout_p = 1
    for hole in range(5):                                                                         # null pointers
        a = [P(qkv), P(pl), P(bu), P(bv), P(ln)]
        a[hole] = None
        assert call(*a, B, T, H, dk, w, 0.0, 0, P(ctx)) == -1
    assert call(P(qkv), P(pl), P(bu), P(bv), P(ln), B, T, H, dk, w, 0.0, 0, None) == -1
    torch.cuda.synchronize()
    assert (ctx.float() == 7.0).all()                                                             # ... refused before any device work
    assert L.ia_relpos_attention_local_supported(T, dk, 0) == 0 and L.ia_relpos_attention_local_supported(T, dk, 1) == 1
    assert L.ia_relpos_attention_local_supported(T, 68, 4) == 0
    with pytest.raises(ValueError):                                                               # too few position rows
        fast.relpos_attention_local(qkv, pl[:2 * w], bu, bv, ln, B, T, H, dk, w)


# ------------------------------------------------------------------------------------------- front end beyond 41 s of audio
@pytest.mark.parametrize("T,lens", [(4097, (4097, 4096, 300)), (5000, (5000, 4097, 2))])
def test_normalize_of_rows_longer_than_4096_frames(T, lens):
    """Recordings long enough to want local attention have more than 4096 log-mel frames, where ia_feat_normalize switches from
    the register-resident row to the kernel that re-reads it.  Against the fp64 statistics on the same fp32 input.

    Bound, from the fp32 arithmetic: a thread adds ceil(T / 256) values serially and the block adds 256 partial sums in a tree
    of depth 8 + 2, so a sum passes through at most n_add = ceil(T / 256) + 10 roundings of relative size 2^-24: the mean is off
    by at most n_add * 2^-24 * max|x|, the variance by the same relative amount.  Output = (x - mean) / (std + eps):
    |error| <= n_add * 2^-24 * (2 max|x| / std + 2 max|out|), the factors 2 covering the subtraction, the division and the
    rounding of x - mean itself.  Chosen before any run; the measured error is printed."""
    from indic_cl_asr_amd import ops
    g = torch.Generator().manual_seed(T)
    B, F_ = len(lens), 8
    x = torch.randn(B, F_, T, generator=g) * 2.0 - 10.0 + torch.randn(B, F_, 1, generator=g)
    for b, n in enumerate(lens):
        x[b, 3, :n] = -10.25                                             # a constant row: every partial sum is exact, std = 0
    ln = torch.tensor(lens)
    fs = torch.tensor([[1]] * B); fw = torch.tensor([[1]] * B)           # feature 1 filled; frames 4090 .. 4099 where valid
    ts = torch.tensor([[4090]] * B); tw = torch.tensor([[10]] * B)
    spans = tuple(t.int().cuda() for t in (fs, fw, ts, tw))
    K = ops.normalize_mask(x.cuda(), ln.cuda(), spans, eps=1e-5, mask_value=-1.0).double().cpu()
    K0 = ops.normalize_mask(x.cuda(), ln.cuda(), None, eps=1e-5).double().cpu()
    n_add = -(-T // 256) + 10
    for b, n in enumerate(lens):
        xv = x[b, :, :n].double()
        mean, std = xv.mean(1, keepdim=True), xv.std(1, keepdim=True)
        E = (xv - mean) / (std + 1e-5)
        assert torch.equal(K0[b, :, n:], torch.zeros(F_, T - n, dtype=torch.float64))              # zero beyond the length
        assert torch.equal(K0[b, 3, :n], torch.zeros(n, dtype=torch.float64))                      # the constant row
        rows = [f for f in range(F_) if f != 3]
        tol = n_add * 2.0 ** -24 * (2 * float(xv[rows].abs().max()) / float(std[rows].min()) + 2 * float(E[rows].abs().max()))
        err = float((K0[b, rows, :n] - E[rows]).abs().max())
        print(f"T={T} len={n}: max |kernel - fp64| = {err:.3e}, bound {tol:.3e}")
        assert err <= tol
        filled = torch.zeros(F_, T, dtype=torch.bool)
        filled[1] = True
        filled[:, 4090:min(4100, n)] = True
        assert torch.equal(K[b][filled], torch.full((int(filled.sum()),), -1.0, dtype=torch.float64))
        assert torch.equal(K[b][~filled], K0[b][~filled])


# ---------------------------------------------------------------------------------------------------------- encoder level
def _model():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny', d_model=64, n_layers=3, compute_dtype='bf16', dither=0.0))
    with torch.no_grad():
        for l in m.encoder.layers:
            l.self_attn.pos_bias_u.normal_(0, 0.2); l.self_attn.pos_bias_v.normal_(0, 0.2)
            l.conv.batch_norm.weight.uniform_(0.5, 1.5); l.conv.batch_norm.bias.normal_(0, 0.2)
    m.disable_dropout().cuda()
    m.spec_augment_enabled = False
    m.change_attention_model("rel_pos_local_attn", [16, 16])
    return m


def _audio():
    g = torch.Generator().manual_seed(4)
    sig = torch.randn(2, 96000, generator=g) * 0.1                      # T' = 151 and 101
    sl = torch.tensor([96000, 64000])
    sig[1, 64000:] = 0
    return sig.cuda(), sl.cuda()


@pytest.fixture(scope="module")
def local_model():
    return _model()


def _encode(m, fast_path):
    sig, sl = _audio()
    m.encoder.use_fast_path = fast_path
    try:
        with torch.no_grad():
            enc, elen = m(input_signal=sig, input_signal_length=sl)
    finally:
        m.encoder.use_fast_path = True
    return enc.float().cpu(), elen.cpu()


@pytest.mark.parametrize("mode", ["eval", "train", "per_op"])
def test_encoder_fast_path_matches_aten_composition(local_model, mode, monkeypatch):
    """use_fast_path=True (the local kernel through the native prefix executor; `per_op`: through ConformerLayer.forward_fast,
    with fast.attention_flash_supported patched off so that _fast_prefix declines the executor) against use_fast_path=False (the
    ATen composition with the window) within the "two bf16 paths" bound of tests/test_step_gpu.py, 0.04 x the reference scale
    on valid frames.  `train`: train-mode BatchNorm (batch statistics), dropout disabled."""
    from indic_cl_asr_amd.ops import fast
    m = local_model
    m.train(mode == "train")
    calls = {"local": 0, "full": 0, "prefix_window": []}
    orig_local, orig_full, orig_prefix = fast.relpos_attention_local, fast.relpos_attention_flash, fast.conformer_prefix

    def spy_local(*a, **kw):
        calls["local"] += 1
        assert a[9] == 16                                               # the window
        return orig_local(*a, **kw)

    def spy_full(*a, **kw):
        calls["full"] += 1
        return orig_full(*a, **kw)

    def spy_prefix(*a, **kw):
        calls["prefix_window"].append(kw.get("att_window"))
        return orig_prefix(*a, **kw)

    monkeypatch.setattr(fast, "relpos_attention_local", spy_local)
    monkeypatch.setattr(fast, "relpos_attention_flash", spy_full)
    monkeypatch.setattr(fast, "conformer_prefix", spy_prefix)
    state =[(l.conv.batch_norm.running_mean.clone(), l.conv.batch_norm.running_var.clone(),
              l.conv.batch_norm.num_batches_tracked.clone()) for l in m.encoder.layers]
    ref, rlen = _encode(m, False)
    assert calls == {"local": 0, "full": 0, "prefix_window": []}
    for l, (rm, rv, nb) in zip(m.encoder.layers, state):                # both paths start from the same running statistics
        l.conv.batch_norm.running_mean.copy_(rm); l.conv.batch_norm.running_var.copy_(rv)
        l.conv.batch_norm.num_batches_tracked.copy_(nb)
    if mode == "per_op":
        monkeypatch.setattr(fast, "attention_flash_supported", lambda T, dk: False)
    out, olen = _encode(m, True)
    if mode == "per_op":
        assert calls["local"] == 3 and calls["full"] == 0 and calls["prefix_window"] == []    # the new entry point, per layer
    else:
        assert calls["prefix_window"] == [16] and calls["full"] == 0                          # the executor, told the window
    assert torch.equal(olen, rlen) and olen.tolist() == [151, 101] and torch.isfinite(out).all()
    valid = (torch.arange(ref.shape[2])[None, :] < rlen[:, None]).unsqueeze(1)
    scale = (ref * valid).abs().max().item()
    err = ((out - ref) * valid).abs().max().item()
    print(f"{mode}: max |fast - composition| on valid frames = {err:.3e}, reference scale {scale:.3f}, bound {0.04 * scale:.3e}")
    assert err < 0.04 * scale
    m.eval()


def test_full_attention_still_takes_the_full_kernel(local_model, monkeypatch):
    """Switching back: the executor is told window 0 again."""
    from indic_cl_asr_amd.ops import fast
    m = local_model.eval()
    seen = []
    orig = fast.conformer_prefix
    monkeypatch.setattr(fast, "conformer_prefix", lambda *a, **kw: (seen.append(kw.get("att_window")), orig(*a, **kw))[1])
    m.change_attention_model("rel_pos")
    try:
        full, _ = _encode(m, True)
    finally:
        m.change_attention_model("rel_pos_local_attn", [16, 16])
    loc, _ = _encode(m, True)
    assert seen == [0, 16] and not torch.equal(full, loc)


def test_transcribe_and_align_under_local_attention(local_model):
    m = local_model.eval()
    g = torch.Generator().manual_seed(2)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (96000, 40000, 64000)]
    for decoder in ("rnnt", "ctc"):
        m.cur_decoder = decoder
        hyps = m.transcribe(audio, batch_size=2, language_id="hi")[0]
        assert len(hyps) == 3 and all(isinstance(h, str) for h in hyps)
    m.cur_decoder = "rnnt"
    ids = [[3, 3, 7, 1], [], [15, 0, 2, 2, 2, 9]]
    out = m.align(audio, token_ids=ids, language_id="ta", batch_size=2)
    assert len(out) == 3 and all(a.feasible for a in out)
    assert [len(a.frames) for a in out] == [151, 63, 101]
    assert m.encoder.self_attention_model == "rel_pos_local_attn"


def test_recording_beyond_the_position_table_and_the_register_resident_front_end():
    """45 s of audio: 4501 log-mel frames (> 4096, the long-row normalisation) and T' = 1126 encoder frames on a model whose
    full-attention position table stops at pos_emb_max_len = 512 -- local attention does not read it."""
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny', d_model=64, n_layers=3, compute_dtype='bf16', dither=0.0, pos_emb_max_len=512,
                                              self_attention_model="rel_pos_local_attn", att_context_size=[16, 16])).cuda().eval()
    assert m.encoder.pos_enc.local_window == 16
    g = torch.Generator().manual_seed(3)
    audio = [torch.randn(45 * 16000, generator=g) * 0.1]
    with torch.no_grad():
        enc, elen = m(input_signal=audio[0].cuda()[None], input_signal_length=torch.tensor([45 * 16000]).cuda())
    assert elen.tolist() == [1126] and enc.shape[2] == 1126 and torch.isfinite(enc.float()).all()
    m.cur_decoder = "ctc"
    assert len(m.transcribe(audio, batch_size=1, language_id="hi")[0]) == 1
    out = m.align(audio, token_ids=[[3, 7, 1]], language_id="hi", batch_size=1)
    assert len(out) == 1 and out[0].feasible and len(out[0].frames) == 1126
