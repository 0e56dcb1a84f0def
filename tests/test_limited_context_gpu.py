"""csrc/attention_flash.hip under its context span (rel-pos attention with a limited context: att_context_size = [L, R] under
att_context_style 'regular' or 'chunked_limited') against an fp64 restatement of the reference's masked RelPositionMultiHeadAttention
on the kernel's bf16 inputs, against the full kernel where the context admits every pair, against the local kernel where the
context is a symmetric window, and through the encoder (native prefix executor, per-op chain, transcribe, align).

Tolerances are those of tests/test_local_attention_gpu.py: the arithmetic is the same.  tests/test_limited_context.py pins the
pair rule used here to the reference's mask.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_local_attention_gpu import _audio, _inputs, _model  # noqa: E402

STYLE = {"regular": 0, "chunked": 1}
NAME = {"regular": "regular", "chunked": "chunked_limited"}


def _pairs(T, style, L, R, device="cuda"):
    """[T,T] bool: query i (rows) and key j pair.  regular: i - j <= L and j - i <= R; chunked, R >= 0: 0 <= i//C - j//C <= L//C,
    C = R + 1; chunked, R < 0: i - j <= L.  A negative side is unlimited."""
    i = torch.arange(T, device=device)[:, None]; j = torch.arange(T, device=device)[None, :]
    ok = torch.ones(T, T, dtype=torch.bool, device=device)
    if style == "regular" or R < 0:
        if L >= 0:
            ok &= (i - j) <= L
        if R >= 0:
            ok &= (j - i) <= R
        return ok
    C = R + 1
    dc = i // C - j // C
    ok &= dc >= 0
    if L >= 0:
        ok &= dc <= L // C
    return ok


def _reference(qkv, pl, bu, bv, lens, B, T, H, dk, style, L, R):
    """ctx[b,i,h,:] = sum_j softmax_j(((q_i+u).k_j + (q_i+v).p[T-1-i+j]) / sqrt(dk)) v_j over the pairs of _pairs, j < len; 0 for
    i >= len.  q+u and q+v rounded to bf16 as the kernel's operands are (tests/test_attention_flash_gpu.py::_reference)."""
    d = H * dk
    x = qkv.double().view(B, T, 3, H, dk)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)   # [B,H,T,dk]
    p = pl.double()[:2 * T - 1].view(2 * T - 1, H, dk).permute(1, 0, 2)                            # [H,2T-1,dk]
    qu = (q + bu.double()[None, :, None, :]).bfloat16().double()
    qv = (q + bv.double()[None, :, None, :]).bfloat16().double()
    ac = qu @ k.transpose(-1, -2)
    i = torch.arange(T, device=qkv.device)[:, None]; j = torch.arange(T, device=qkv.device)[None, :]
    pairs = _pairs(T, style, L, R, qkv.device)
    o = torch.zeros(B, H, T, dk, dtype=torch.float64, device=qkv.device)
    for h in range(H):
        bd = (qv[:, h] @ p[h].t()).gather(-1, (T - 1 - i + j).expand(B, T, T))
        s = (ac[:, h] + bd) / math.sqrt(dk)
        ok = pairs[None] & (j[None] < lens[:, None, None])
        s = s.masked_fill(~ok, float("-inf"))
        o[:, h] = torch.nan_to_num(torch.softmax(s, -1), nan=0.0) @ v[:, h]                        # (an empty utterance: no key)
    qvalid = (torch.arange(T, device=qkv.device)[None, :] < lens[:, None])[:, None, :, None]
    o = torch.where(qvalid, o, torch.zeros_like(o))
    return o.transpose(1, 2).reshape(B * T, d)


CASES = [  # B, T, H, dk, style, L, R, lens
    (2, 17, 2, 64, "regular", 4, 2, [17, 9]),             # one tile, asymmetric
    (1, 64, 1, 64, "regular", 0, 0, [64]),                # every query sees only itself
    (2, 130, 2, 64, "regular", 16, 0, [130, 70]),         # causal: whole tiles right of the diagonal empty
    (1, 65, 2, 48, "regular", -1, 3, [65]),               # unlimited left, dk < 64, tile boundary
    (1, 65, 1, 64, "regular", 5, -1, [65]),               # unlimited right
    (1, 321, 1, 64, "regular", 100, 37, [321]),           # tiles skipped on both sides, mask-free interior tiles
    (1, 64, 1, 64, "chunked", 0, 0, [64]),                # C = 1
    (2, 200, 4, 36, "chunked", 32, 15, [200, 129]),       # chunk = one wave, n = 2, dk = 36
    (2, 200, 2, 64, "chunked", 70, 69, [200, 128]),       # C = 70 straddles tile edges, n = 1
    (1, 300, 2, 64, "chunked", -1, 12, [300]),            # odd C, unlimited left
    (2, 130, 2, 64, "chunked", 24, -1, [130, 64]),        # the triu-only form
    (3, 70, 2, 64, "regular", 8, 2, [70, 0, 33]),         # an empty utterance: zero context for it
    (1, 751, 8, 64, "chunked", 140, 27, [751]),           # one large shape
]


@pytest.mark.parametrize("B,T,H,dk,style,L,R,lens", CASES)
def test_context_attention_matches_fp64_restatement(B, T, H, dk, style, L, R, lens):
    from indic_cl_asr_amd.ops import fast
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=T + dk + L + R, lens=lens)
    ref = _reference(qkv, pl, bu, bv, ln, B, T, H, dk, style, L, R)
    c = (NAME[style], L, R)
    assert fast.attention_context_supported(T, dk, c)
    ctx = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, c)
    assert torch.isfinite(ctx).all()
    out = ctx.double()
    err, scale = (out - ref).abs().max().item(), ref.abs().max().item()
    print(f"(B,T,H,dk)=({B},{T},{H},{dk}) {style} [{L},{R}] lens={lens}: err {err:.3e}, max|ref| {scale:.3f}, "
          f"bound {2e-2 * scale + 1e-3:.3e}")
    assert err <= 2e-2 * scale + 1e-3, (err, scale)                      # bf16 band, bf16 probabilities
    for b in range(B):                                                  # padded queries are exactly zero
        if lens[b] < T:
            assert out.view(B, T, -1)[b, lens[b]:].abs().max().item() == 0.0
    by_number = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, (STYLE[style], L, R))   # the C style number
    assert torch.equal(by_number, ctx)


@pytest.mark.parametrize("B,T,H,dk,lens", [(2, 200, 2, 64, [200, 129]), (2, 126, 4, 36, [126, 5])])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_all_admitting_context_gives_the_full_kernels_bits(B, T, H, dk, lens, p):
    """Regular [T-1, T-1], [-1, -1] under either style and regular sides beyond T-1 admit every pair: the full kernel's bits,
    context and log-sum-exp."""
    from indic_cl_asr_amd.ops import fast
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=11 + T, lens=lens)
    full, flse = fast.relpos_attention_flash(qkv, pl, bu, bv, ln, B, T, H, dk, dropout_p=p, seed=5, want_lse=True)
    for c in (("regular", T - 1, T - 1), ("regular", -1, -1), ("chunked_limited", -1, -1), ("regular", T + 40, -1)):
        ctx, lse = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, c, dropout_p=p, seed=5, want_lse=True)
        print(f"T={T} dk={dk} p={p} {c}: max |context - full| = {(ctx.float() - full.float()).abs().max().item():.3e}")
        assert torch.equal(ctx, full) and torch.equal(lse, flse), c


@pytest.mark.parametrize("B,T,H,dk,w,lens", [(2, 200, 2, 64, 16, [200, 129]), (1, 300, 4, 36, 70, [300])])
def test_symmetric_regular_context_against_the_local_kernel(B, T, H, dk, w, lens):
    """Regular [w, w] is the local kernel's band; the local kernel reads rows T-1-w .. T-1+w of the full table."""
    from indic_cl_asr_amd.ops import fast
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=3 + T, lens=lens)
    loc = fast.relpos_attention_local(qkv, pl[T - 1 - w:T + w].contiguous(), bu, bv, ln, B, T, H, dk, w)
    ctx = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, ("regular", w, w))
    err, scale = (ctx.double() - loc.double()).abs().max().item(), loc.double().abs().max().item()
    print(f"T={T} dk={dk} w={w}: max |context - local| = {err:.3e} (max|local| {scale:.3f}); bit-equal: {torch.equal(ctx, loc)}")
    assert err <= 2e-2 * scale + 1e-3


def test_context_attention_dropout_is_deterministic():
    from indic_cl_asr_amd.ops import fast
    B, T, H, dk, c = 2, 200, 2, 64, ("chunked_limited", 32, 15)
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=9, lens=[200, 150])
    base = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, c)
    d1 = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, c, dropout_p=0.25, seed=5)
    d2 = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, c, dropout_p=0.25, seed=5)
    d3 = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, c, dropout_p=0.25, seed=6)
    assert torch.equal(d1, d2) and not torch.equal(d1, d3) and not torch.equal(d1, base)
    assert torch.isfinite(d1).all() and d1.view(B, T, -1)[1, 150:].abs().max().item() == 0.0


def test_context_attention_argument_validation():
    from indic_cl_asr_amd import _lib
    from indic_cl_asr_amd.ops import fast
    L = _lib.lib()
    B, T, H, dk = 1, 64, 1, 64
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1)
    ctx = torch.full((B * T, H * dk), 7.0, dtype=torch.bfloat16, device="cuda")
    P = _lib.ptr
    call = lambda *a: L.ia_relpos_attention_context(*a, _lib.stream_ptr())
    ops5 = (P(qkv), P(pl), P(bu), P(bv), P(ln))
    assert call(*ops5, B, T, H, dk, 2, 4, 4, 0.0, 0, P(ctx)) == -1        # unknown style: IA_INVALID_VALUE
    assert call(*ops5, B, T, H, dk, -1, 4, 4, 0.0, 0, P(ctx)) == -1
    assert call(*ops5, B, T, H, dk, 0, -2, 4, 0.0, 0, P(ctx)) == -1       # left < -1
    assert call(*ops5, B, T, H, dk, 0, 4, -2, 0.0, 0, P(ctx)) == -1       # right < -1
    assert call(*ops5, B, T, H, dk, 1, 9, 3, 0.0, 0, P(ctx)) == -1        # chunked: 9 % (3 + 1) != 0
    assert call(*ops5, B, T, 1, 68, 0, 4, 4, 0.0, 0, P(ctx)) == -4        # dk > 64: IA_UNSUPPORTED
    assert call(*ops5, B, T, 1, 30, 1, 8, 3, 0.0, 0, P(ctx)) == -4        # dk no multiple of 4
    assert call(*ops5, B, T, H, dk, 0, 4, 4, 1.0, 0, P(ctx)) == -1        # dropout_p = 1
    for hole in range(5):                                                # null pointers
        a = list(ops5)
        a[hole] = None
        assert call(*a, B, T, H, dk, 0, 4, 4, 0.0, 0, P(ctx)) == -1
    assert call(*ops5, B, T, H, dk, 0, 4, 4, 0.0, 0, None) == -1
    torch.cuda.synchronize()
    assert (ctx.float() == 7.0).all()                                    # ... refused before any device work
    S = L.ia_relpos_attention_context_supported
    assert S(T, dk, 0, 4, 4) == 1 and S(T, dk, 1, 8, 3) == 1 and S(T, dk, 1, 9, 3) == 0 and S(T, dk, 2, 4, 4) == 0
    assert S(T, 68, 0, 4, 4) == 0 and S(T, dk, 0, -1, -1) == 1 and S(T, dk, 1, 12, -1) == 1
    with pytest.raises(ValueError):                                      # too few position rows
        fast.relpos_attention_context(qkv, pl[:2 * T - 2], bu, bv, ln, B, T, H, dk, ("regular", 4, 4))
    with pytest.raises(ValueError):
        fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, ("sliding", 4, 4))


def test_prefix_executor_refuses_a_context_together_with_a_window():
    """ia_block_params: att_style != 0 with att_window > 0, an unknown style and layers that disagree are IA_INVALID_VALUE, before
    the residual stream is touched."""
    from indic_cl_asr_amd import _lib
    from indic_cl_asr_amd.ops import fast
    m = _model().eval()
    layers = list(m.encoder.layers[:2])
    B, T, d = 1, 40, 64
    xr = torch.full((B * T, d), 0.5, device="cuda")
    pe = torch.zeros(2 * T - 1, d, dtype=torch.bfloat16, device="cuda")
    ln = torch.tensor([T], device="cuda")
    with pytest.raises(RuntimeError, match="IA_INVALID_VALUE"):
        fast.conformer_prefix(layers, xr.clone(), pe, ln, B, T, 0, 16, False, att_window=4, att_context=("regular", 4, 4))
    arr = (_lib.BlockParams * 2)(*[fast._block_params(l) for l in layers])
    for i in range(2):
        arr[i].pl_cached = None
        arr[i].att_window, arr[i].att_style, arr[i].att_left, arr[i].att_right = 0, 1, 4, 4
    arr[1].att_right = 5                                                  # layers disagree
    import ctypes
    n = _lib.lib().ia_conformer_prefix_ws_bytes(B, T, d, arr[0].d_ff, arr[0].n_heads, arr[0].ksz, 2 * T - 1)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    x = xr.clone()
    run = lambda: _lib.lib().ia_conformer_prefix_fwd(ctypes.addressof(arr), 2, _lib.ptr(x), _lib.ptr(pe), 2 * T - 1, _lib.ptr(ln), B, T, 0,
                                                     16, 0, _lib.ptr(ws), n, _lib.stream_ptr())
    assert run() == -1
    arr[1].att_right = 4
    arr[0].att_style = arr[1].att_style = 3                               # unknown style
    assert run() == -1
    torch.cuda.synchronize()
    assert torch.equal(x, xr)


# ---------------------------------------------------------------------------------------------------------- encoder level
CONTEXTS = [("chunked_limited", [32, 15]), ("regular", [16, 0])]


@pytest.fixture(scope="module")
def context_model():
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


@pytest.mark.parametrize("style,context", CONTEXTS)
@pytest.mark.parametrize("mode", ["eval", "train", "per_op"])
def test_encoder_fast_path_matches_aten_composition(context_model, mode, style, context, monkeypatch):
    """use_fast_path=True (the context kernel through the native prefix executor; `per_op`: through ConformerLayer.forward_fast,
    with fast.attention_flash_supported patched off so that _fast_prefix declines the executor) against use_fast_path=False (the
    ATen composition with the interval mask) within the "two bf16 paths" bound of tests/test_step_gpu.py, 0.04 x the reference
    scale on valid frames."""
    from indic_cl_asr_amd.ops import fast
    m = context_model
    m.change_attention_model("rel_pos", context, att_context_style=style)
    assert m.cfg.att_context_style == style and m.cfg.att_context_size == context and m.encoder.pos_enc.local_window is None
    want = (style, context[0], context[1])
    m.train(mode == "train")
    calls = {"context": 0, "local": 0, "full": 0, "prefix": []}
    orig_ctx, orig_local, orig_full, orig_prefix = (fast.relpos_attention_context, fast.relpos_attention_local,
                                                    fast.relpos_attention_flash, fast.conformer_prefix)

    def spy_ctx(*a, **kw):
        calls["context"] += 1
        assert tuple(a[9]) == want
        return orig_ctx(*a, **kw)

    def spy(name, orig):
        def f(*a, **kw):
            calls[name] += 1
            return orig(*a, **kw)
        return f

    def spy_prefix(*a, **kw):
        calls["prefix"].append((kw.get("att_window"), tuple(kw.get("att_context") or ())))
        return orig_prefix(*a, **kw)

    monkeypatch.setattr(fast, "relpos_attention_context", spy_ctx)
    monkeypatch.setattr(fast, "relpos_attention_local", spy("local", orig_local))
    monkeypatch.setattr(fast, "relpos_attention_flash", spy("full", orig_full))
    monkeypatch.setattr(fast, "conformer_prefix", spy_prefix)
    state = [(l.conv.batch_norm.running_mean.clone(), l.conv.batch_norm.running_var.clone(),
              l.conv.batch_norm.num_batches_tracked.clone()) for l in m.encoder.layers]
    ref, rlen = _encode(m, False)
    assert calls == {"context": 0, "local": 0, "full": 0, "prefix": []}
    for l, (rm, rv, nb) in zip(m.encoder.layers, state):                # both paths start from the same running statistics
        l.conv.batch_norm.running_mean.copy_(rm); l.conv.batch_norm.running_var.copy_(rv)
        l.conv.batch_norm.num_batches_tracked.copy_(nb)
    if mode == "per_op":
        monkeypatch.setattr(fast, "attention_flash_supported", lambda T, dk: False)
    out, olen = _encode(m, True)
    if mode == "per_op":
        assert calls["context"] == 3 and calls["prefix"] == []         # the new entry point, per layer
    else:
        assert calls["prefix"] == [(0, want)] and calls["context"] == 0   # the executor, told the context
    assert calls["local"] == 0 and calls["full"] == 0
    assert torch.equal(olen, rlen) and olen.tolist() == [151, 101] and torch.isfinite(out).all()
    valid = (torch.arange(ref.shape[2])[None, :] < rlen[:, None]).unsqueeze(1)
    scale = (ref * valid).abs().max().item()
    err = ((out - ref) * valid).abs().max().item()
    print(f"{style} {context} {mode}: max |fast - composition| on valid frames = {err:.3e}, reference scale {scale:.3f}, "
          f"bound {0.04 * scale:.3e}")
    assert err < 0.04 * scale
    m.eval()


def test_context_changes_the_encoding_and_full_attention_returns(context_model):
    """From every style back to full attention with change_attention_model("rel_pos"): the test sets each style itself, so the
    retained style at the moment of return is the one named -- 'chunked_limited' included, directly and by way of local attention,
    and after the multi-look-ahead sequence of INTEGRATION.md -- and the full encoding comes back bit for bit."""
    m = context_model.eval()
    m.change_attention_model("rel_pos")
    full, _ = _encode(m, True)

    def back(was):
        m.change_attention_model("rel_pos")
        assert m.encoder.att_context_size == [-1, -1] and m.encoder.att_context_size_all == [[-1, -1]]
        assert m.cfg.att_context_size == [-1, -1] and m.cfg.self_attention_model == "rel_pos"
        assert all(l.self_attn.att_context is None and l.self_attn.att_window is None for l in m.encoder.layers)
        assert m.encoder.pos_enc.local_window is None
        again, _ = _encode(m, True)
        assert torch.equal(full, again), was

    m.change_attention_model("rel_pos", [16, 0], att_context_style="regular")
    causal, _ = _encode(m, True)
    assert not torch.equal(full, causal)
    back("regular")
    m.change_attention_model("rel_pos", [32, 15], att_context_style="chunked_limited")
    chunked, _ = _encode(m, True)
    assert m.encoder.att_context_style == "chunked_limited" and not torch.equal(full, chunked)
    back("chunked_limited")
    assert m.encoder.att_context_style == "chunked_limited"            # the style stays; [-1, -1] is full attention under it
    m.change_attention_model("rel_pos", [32, 15], att_context_style="chunked_limited")
    m.change_attention_model("rel_pos_local_attn", [16, 16])
    local, _ = _encode(m, True)
    assert not torch.equal(full, local)
    back("chunked_limited, then local attention")
    m.change_attention_model("rel_pos", [[70, 13], [70, 6], [70, 1], [70, 0]], att_context_style="chunked_limited",
                             att_context_probs=[0.25] * 4)
    m.set_default_att_context_size([70, 6])
    look, _ = _encode(m, True)
    assert all(l.self_attn.att_context == ("chunked_limited", 70, 6) for l in m.encoder.layers) and not torch.equal(full, look)
    back("multi-look-ahead chunked_limited")
    assert m.cfg.att_context_probs is None


@pytest.mark.parametrize("style,context", CONTEXTS)
def test_transcribe_and_align_under_a_limited_context(context_model, style, context):
    m = context_model.eval()
    m.change_attention_model("rel_pos", context, att_context_style=style)
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
    assert m.encoder.self_attention_model == "rel_pos" and m.encoder.att_context_size == context
