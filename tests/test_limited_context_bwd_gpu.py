"""csrc/attention_flash_bwd.hip under its context span (rel-pos attention backward with a limited context) against fp64 autograd of
the interval-masked composition on the kernel's bf16 inputs, against the full backward where the context admits every pair,
against the local backward where the context is a symmetric window, and up through the trainable-block node and
model.training_step.

The bound of the kernel tests, max|err| <= 3e-2 max|ref| + 1e-4 per tensor, is the one tests/test_local_attention_bwd_gpu.py and
tests/test_attention_flash_bwd_gpu.py hold the other spans to: the arithmetic is the same (bf16 P / dS operands, bf16 outputs).
tests/test_limited_context.py pins the composition's gradients to the reference's.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from test_limited_context_gpu import CASES, NAME, _pairs  # noqa: E402
from test_local_attention_gpu import _audio, _inputs, _model  # noqa: E402


def _grads64(qkv, pl, bu, bv, lens, dctx, B, T, H, dk, style, L, R, keep=None, keep_scale=1.0):
    """fp64 autograd of  o[b,h,i] = sum_j keep o softmax_j(((q_i+u).k_j + (q_i+v).p[T-1-i+j]) / sqrt(dk)) v_j  over the pairs of
    _pairs, j < len, i < len (a query without a key -- an empty utterance -- gives 0, not NaN)
    -> (dqkv [B*T,3d], dpl [2T-1,d], du, dv)."""
    d = H * dk
    dev = qkv.device
    x = qkv.double().view(B, T, 3, H, dk)
    q, k, v = (x[:, :, n].transpose(1, 2).clone().requires_grad_(True) for n in range(3))
    p = pl.double()[:2 * T - 1].view(2 * T - 1, H, dk).permute(1, 0, 2).clone().requires_grad_(True)
    u, vb = bu.double().clone().requires_grad_(True), bv.double().clone().requires_grad_(True)
    ac = (q + u[None, :, None, :]) @ k.transpose(-1, -2)
    full = torch.einsum("bhid,hrd->bhir", q + vb[None, :, None, :], p)
    i = torch.arange(T, device=dev)[:, None]; j = torch.arange(T, device=dev)[None, :]
    bd = full.gather(-1, (T - 1 - i + j).expand(*ac.shape))
    ok = _pairs(T, style, L, R, dev)[None] & (j[None] < lens[:, None, None]) & (i[None] < lens[:, None, None])
    s = ((ac + bd) / math.sqrt(dk)).masked_fill(~ok[:, None], float("-inf"))
    e = torch.exp(s - s.detach().amax(-1, keepdim=True).clamp(min=-1e300))
    pr = e / e.sum(-1, keepdim=True).clamp(min=1e-100)
    if keep is not None:
        pr = pr * keep * keep_scale
    o = pr @ v
    (o * dctx.double().view(B, T, H, dk).transpose(1, 2)).sum().backward()
    dqkv = torch.stack([t.grad.transpose(1, 2) for t in (q, k, v)], dim=2).reshape(B * T, 3 * d)
    return dqkv, p.grad.permute(1, 0, 2).reshape(2 * T - 1, d), u.grad, vb.grad


def _check(name, got, ref, rel=3e-2):
    err = (got.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"  {name}: max|err| {err:.3e}, max|ref| {scale:.3f}, bound {rel * scale + 1e-4:.3e}")
    assert err <= rel * scale + 1e-4, (name, err, scale)


def _check_all(dqkv, dpl, du, dv, ref, d, T):
    r_qkv, r_pl, r_u, r_v = ref
    _check("dq", dqkv[:, :d], r_qkv[:, :d])
    _check("dk", dqkv[:, d:2 * d], r_qkv[:, d:2 * d])
    _check("dv", dqkv[:, 2 * d:], r_qkv[:, 2 * d:])
    _check("dpl", dpl[:2 * T - 1], r_pl)
    _check("du", du, r_u)
    _check("dv_bias", dv, r_v)


def _dctx(B, T, d, seed):
    return (torch.randn(B * T, d, generator=torch.Generator().manual_seed(seed)) * 0.5).bfloat16().cuda()


def _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, c, p=0.0, seed=0):
    from indic_cl_asr_amd.ops import fast
    ctx, lse = fast.relpos_attention_context(qkv, pl, bu, bv, ln, B, T, H, dk, c, dropout_p=p, seed=seed, want_lse=True)
    return ctx, lse, fast.relpos_attention_context_bwd(qkv, pl, bu, bv, ln, ctx, dctx, lse, B, T, H, dk, c, dropout_p=p, seed=seed)


def _reach(T, style, L, R, maxlen):
    """(lo, hi): the relative positions i - j that an admissible pair of an utterance of maxlen frames can have; regular [-R, L],
    chunked [-R, L + R], an unlimited side and the utterance's end limiting both to maxlen - 1."""
    far = maxlen - 1
    if style == "chunked" and R >= 0:
        left, right = (L + R if L >= 0 else far), R
    else:
        left, right = (L if L >= 0 else far), (R if (R >= 0 and style == "regular") else far)
    return -min(right, far), min(left, far)


@pytest.mark.parametrize("B,T,H,dk,style,L,R,lens", CASES)
def test_context_backward_matches_fp64_autograd(B, T, H, dk, style, L, R, lens):
    d = H * dk
    rows = (2 * T - 1 + 7) // 8 * 8 + 8                                  # a padded table: rows beyond 2T-2 exist
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, rows, seed=T + dk + L + R, lens=lens)
    dctx = _dctx(B, T, d, T)
    ctx, lse, (dqkv, dpl, du, dv) = _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, (NAME[style], L, R))
    assert all(torch.isfinite(t.float()).all() for t in (lse, dqkv, dpl, du, dv))
    print(f"(B,T,H,dk)=({B},{T},{H},{dk}) {style} [{L},{R}] lens={lens}")
    ref = _grads64(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, style, L, R)
    _check_all(dqkv, dpl, du, dv, ref, d, T)
    for b in range(B):                                                   # rows of padded frames carry no gradient at all
        if lens[b] < T:
            assert dqkv.view(B, T, -1)[b, lens[b]:].abs().max().item() == 0.0
            assert ctx.view(B, T, -1)[b, lens[b]:].abs().max().item() == 0.0
    assert dpl[2 * T - 1:].abs().max().item() == 0.0                     # rows beyond the table
    # row r <-> relative position i - j = T - 1 - r: rows no admissible pair reaches are exactly zero, the others are not
    lo, hi = _reach(T, style, L, R, max(lens))
    r0, r1 = T - 1 - hi, T - 1 - lo
    assert dpl[:r0].abs().sum().item() == 0.0 and dpl[r1 + 1:].abs().sum().item() == 0.0
    if (L, R) != (0, 0):   # [0, 0]: one key per query, P = 1 and dS = P (dP - D) = 0 in exact arithmetic -- the true dpl is zero
        # row by row, so that a missing sub-range (the L+1 .. L+R rows of the chunked form, say) shows: every row whose fp64
        # gradient is not negligible (1e-3 of the largest entry: far above what an fp32 sum of bf16 products can lose, far
        # below the tolerance of the comparison above) is nonzero, and the two ends of the reachable range are such rows
        ref_row = ref[1].abs().amax(dim=1)
        live = ref_row >= 1e-3 * ref_row.max()
        assert bool(live[r0]) and bool(live[r1]) and not bool(live[:r0].any()) and not bool(live[r1 + 1:].any())
        got_row = dpl[:2 * T - 1].abs().amax(dim=1)
        dead = torch.nonzero(live & (got_row == 0.0)).flatten().tolist()
        print(f"  dpl rows {r0}..{r1} reachable, {int(live.sum())} of them held to be nonzero, {len(dead)} missing")
        assert not dead, dead


def test_context_backward_with_an_empty_utterance_gives_zero_gradients_for_it():
    B, T, H, dk, c = 3, 70, 2, 64, ("regular", 8, 2)
    d = H * dk
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=2, lens=[70, 0, 33])
    dctx = _dctx(B, T, d, 1)
    ctx, lse, (dqkv, dpl, du, dv) = _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, c)
    assert ctx.view(B, T, -1)[1].abs().max().item() == 0.0
    assert dqkv.view(B, T, -1)[1].abs().max().item() == 0.0
    assert all(torch.isfinite(t.float()).all() for t in (dpl, du, dv))
    r_qkv, r_pl, r_u, r_v = _grads64(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, "regular", 8, 2)
    others = torch.tensor([0, 2], device="cuda")
    _check("dqkv of the other utterances", dqkv.view(B, T, -1)[others], r_qkv.view(B, T, -1)[others])
    _check("dpl", dpl, r_pl); _check("du", du, r_u); _check("dv_bias", dv, r_v)


@pytest.mark.parametrize("B,T,H,dk,lens", [(2, 130, 2, 64, [130, 77]), (3, 126, 4, 36, [126, 64, 5])])
def test_all_admitting_context_gives_the_full_backwards_bits(B, T, H, dk, lens):
    """Regular [T-1, T-1] and [-1, -1] admit every pair: the full backward's bits, the position gradient included (the context
    span keeps the full dBand layout, and these contexts run the full span)."""
    from indic_cl_asr_amd.ops import fast
    d = H * dk
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=11 + T, lens=lens)
    dctx = _dctx(B, T, d, 7)
    for p in (0.0, 0.25):
        fctx, flse = fast.relpos_attention_flash(qkv, pl, bu, bv, ln, B, T, H, dk, dropout_p=p, seed=5, want_lse=True)
        full = fast.relpos_attention_flash_bwd(qkv, pl, bu, bv, ln, fctx, dctx, flse, B, T, H, dk, dropout_p=p, seed=5)
        for c in (("regular", T - 1, T - 1), ("regular", -1, -1), ("chunked_limited", -1, -1)):
            ctx, lse, got = _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, c, p=p, seed=5)
            assert torch.equal(ctx, fctx) and torch.equal(lse, flse)
            for name, a, b in zip(("dqkv", "dpl", "du", "dv"), got, full):
                print(f"p={p} {c} {name}: max |context - full| = {(a.float() - b.float()).abs().max().item():.3e}")
                assert torch.equal(a, b), (c, name)
    assert fast.attention_context_bwd_dims(T, ("regular", 4, 2)) == fast.attention_flash_bwd_dims(T)   # the full dBand layout


@pytest.mark.parametrize("B,T,H,dk,w,lens", [(2, 200, 2, 64, 16, [200, 129]), (1, 300, 4, 36, 70, [300])])
def test_symmetric_regular_context_against_the_local_backward(B, T, H, dk, w, lens):
    """Regular [w, w] is the local kernels' band; they read rows T-1-w .. T-1+w of the full table, and their dpl is those rows'."""
    from indic_cl_asr_amd.ops import fast
    d = H * dk
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=3 + T, lens=lens)
    dctx = _dctx(B, T, d, 4)
    plw = pl[T - 1 - w:T + w].contiguous()
    lctx, llse = fast.relpos_attention_local(qkv, plw, bu, bv, ln, B, T, H, dk, w, want_lse=True)
    l_dqkv, l_dpl, l_du, l_dv = fast.relpos_attention_local_bwd(qkv, plw, bu, bv, ln, lctx, dctx, llse, B, T, H, dk, w)
    ctx, lse, (dqkv, dpl, du, dv) = _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, ("regular", w, w))
    pairs = (("dqkv", dqkv, l_dqkv), ("dpl", dpl[T - 1 - w:T + w], l_dpl), ("du", du, l_du), ("dv", dv, l_dv))
    print(f"T={T} dk={dk} w={w}: bit-equal ctx {torch.equal(ctx, lctx)}, lse {torch.equal(lse, llse)}, "
          + ", ".join(f"{n} {torch.equal(a, b)}" for n, a, b in pairs))
    for n, a, b in pairs:
        _check(n, a, b.double())
    assert dpl[:T - 1 - w].abs().sum().item() == 0.0 and dpl[T + w:].abs().sum().item() == 0.0


def test_context_backward_regenerates_the_forward_dropout_mask_and_is_bit_reproducible():
    B, T, H, dk, c = 3, 300, 4, 36, ("chunked_limited", 32, 15)
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1, seed=8, lens=[300, 170, 64])
    dctx = _dctx(B, T, H * dk, 2)
    a = _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, c, p=0.25, seed=3)[2]
    b = _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, c, p=0.25, seed=3)[2]
    other = _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, c, p=0.25, seed=4)[2]
    for name, x, y, z in zip(("dqkv", "dpl", "du", "dv"), a, b, other):
        assert torch.equal(x, y), name                                   # same seed: same bits
        assert not torch.equal(x, z), name                               # another seed: other bits


def test_context_backward_argument_validation():
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    B, T, H, dk = 1, 64, 1, 64
    d = H * dk
    qkv, pl, bu, bv, ln = _inputs(B, T, H, dk, 2 * T - 1)
    dctx = _dctx(B, T, d, 1)
    ctx, lse, _ = _run(qkv, pl, bu, bv, ln, dctx, B, T, H, dk, ("regular", 4, 4))
    import ctypes
    rs, p0 = ctypes.c_int(), ctypes.c_int()
    assert L.ia_relpos_attention_context_bwd_dims(T, 0, 4, 4, ctypes.byref(rs), ctypes.byref(p0)) == 0
    assert L.ia_relpos_attention_context_bwd_dims(T, 2, 4, 4, ctypes.byref(rs), ctypes.byref(p0)) == -1
    assert L.ia_relpos_attention_context_bwd_dims(T, 1, 9, 3, ctypes.byref(rs), ctypes.byref(p0)) == -1
    assert L.ia_relpos_attention_context_bwd_ws_elems(B, T, H, dk, 0, 4, 4) == L.ia_relpos_attention_flash_bwd_ws_elems(B, T, H, dk) > 0
    assert L.ia_relpos_attention_context_bwd_ws_elems(B, T, H, dk, 0, -2, 4) == 0
    bf = torch.bfloat16
    dqkv = torch.full((B * T, 3 * d), 7.0, dtype=bf, device="cuda")
    dpl = torch.full((2 * T - 1, d), 7.0, dtype=bf, device="cuda")
    dBand = torch.empty(H * B * T * rs.value, dtype=bf, device="cuda")
    QvHM = torch.empty(H * B * T * 64, dtype=bf, device="cuda")
    ws = torch.empty(L.ia_relpos_attention_context_bwd_ws_elems(B, T, H, dk, 0, 4, 4), device="cuda")
    dub = torch.full((2, H, dk), 7.0, device="cuda")
    P = _lib.ptr
    ptrs = [P(qkv), P(pl), P(bu), P(bv), P(ln), P(ctx), P(dctx), P(lse)]
    outs = [P(dqkv), P(dpl), 2 * T - 1, P(dub[0]), P(dub[1]), P(dBand), P(QvHM), P(ws)]
    call = lambda pt, dims, o: L.ia_relpos_attention_context_bwd(*pt, *dims, 0.0, 0, *o, _lib.stream_ptr())
    assert call(ptrs, (B, T, H, dk, 2, 4, 4), outs) == -1                 # unknown style
    assert call(ptrs, (B, T, H, dk, 0, -2, 4), outs) == -1                # left < -1
    assert call(ptrs, (B, T, H, dk, 0, 4, -2), outs) == -1                # right < -1
    assert call(ptrs, (B, T, H, dk, 1, 9, 3), outs) == -1                 # chunked: 9 % 4 != 0
    assert call(ptrs, (B, T, 1, 68, 0, 4, 4), outs) == -4                 # dk > 64: IA_UNSUPPORTED
    for hole in range(8):                                                # null pointers
        a = list(ptrs)
        a[hole] = None
        assert call(a, (B, T, H, dk, 0, 4, 4), outs) == -1
    for hole in (0, 1, 3, 4, 5, 6, 7):
        o = list(outs)
        o[hole] = None
        assert call(ptrs, (B, T, H, dk, 0, 4, 4), o) == -1
    few = list(outs); few[2] = 2 * T - 2                                  # too few position rows
    assert call(ptrs, (B, T, H, dk, 0, 4, 4), few) == -1
    torch.cuda.synchronize()
    assert (dqkv.float() == 7.0).all() and (dpl.float() == 7.0).all() and (dub == 7.0).all()   # refused before any device work


def _structural_zero(name):   # tests/test_step_gpu.py: rounding noise on both sides
    return name.endswith("depthwise_conv.bias") or name.endswith("self_attn.linear_k.bias")


def _step(m, frozen):
    from indic_cl_asr_amd.model import freeze_layer
    sig, sl = _audio()
    g = torch.Generator().manual_seed(6)
    tr = torch.randint(0, m.cfg.vocab_per_lang, (2, 6), generator=g).cuda()
    tl = torch.tensor([6, 4]).cuda()
    m.train()
    freeze_layer(m, frozen)
    for q in m.parameters():
        q.grad = None
    loss, _ = m.training_step((sig, sl, tr, tl), [m.cfg.languages[0]] * 2)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss.detach()), {n: q.grad.float().cpu().clone() for n, q in m.named_parameters()
                                  if n.startswith("encoder.layers.") and q.grad is not None}


@pytest.mark.parametrize("style,context", [("chunked_limited", [32, 15]), ("regular", [16, 0])])
def test_training_step_under_a_limited_context_runs_the_context_backward(style, context, monkeypatch):
    """The tiny model of tests/test_local_attention_gpu.py under a limited context: one training_step + backward with the fused
    trainable blocks (block 0 frozen and encoder_frozen_till = 1: it runs in the no-grad prefix, told the context) and without.  One context backward per
    trainable block, never the full or the local one; loss and every encoder-layer gradient within the fused-against-ATen bounds
    of tests/test_local_attention_bwd_gpu.py's model-level check."""
    from indic_cl_asr_amd.ops import fast
    m = _model()
    m.change_attention_model("rel_pos", context, att_context_style=style)
    m.encoder.encoder_frozen_till = 1                                    # block 0 (frozen by _step) runs in the native prefix
    want = (style, context[0], context[1])
    calls = {"context": 0, "local": 0, "full": 0, "prefix": []}
    o_ctx, o_local, o_full, o_prefix = (fast.relpos_attention_context_bwd, fast.relpos_attention_local_bwd,
                                        fast.relpos_attention_flash_bwd, fast.conformer_prefix)

    def spy_ctx(*a, **kw):
        calls["context"] += 1
        assert tuple(a[12]) == want
        return o_ctx(*a, **kw)

    monkeypatch.setattr(fast, "relpos_attention_context_bwd", spy_ctx)
    monkeypatch.setattr(fast, "relpos_attention_local_bwd", lambda *a, **kw: (calls.__setitem__("local", calls["local"] + 1), o_local(*a, **kw))[1])
    monkeypatch.setattr(fast, "relpos_attention_flash_bwd", lambda *a, **kw: (calls.__setitem__("full", calls["full"] + 1), o_full(*a, **kw))[1])
    monkeypatch.setattr(fast, "conformer_prefix",
                        lambda *a, **kw: (calls["prefix"].append(tuple(kw.get("att_context") or ())), o_prefix(*a, **kw))[1])
    bns = [l.conv.batch_norm for l in m.encoder.layers]
    state = [(b.running_mean.clone(), b.running_var.clone(), b.num_batches_tracked.clone()) for b in bns]

    def restore():
        for b, (rm, rv, nb) in zip(bns, state):
            b.running_mean.copy_(rm); b.running_var.copy_(rv); b.num_batches_tracked.copy_(nb)

    m.encoder.use_fused_blocks = True
    loss_f, grads_f = _step(m, 0)
    assert calls == {"context": 2, "local": 0, "full": 0, "prefix": [want]}
    restore()
    m.encoder.use_fused_blocks = False
    loss_a, grads_a = _step(m, 0)
    assert calls["context"] == 2 and calls["local"] == 0 and calls["full"] == 0      # the ATen composition calls none of them
    m.encoder.use_fused_blocks = True
    print(f"{style} {context}: loss fused {loss_f:.6f}, ATen {loss_a:.6f}")
    assert math.isfinite(loss_f) and math.isclose(loss_f, loss_a, rel_tol=5e-3)
    assert grads_f.keys() == grads_a.keys() and len(grads_f) >= 30 * 2
    for n, a in grads_f.items():
        b = grads_a[n]
        assert torch.isfinite(a).all(), n
        if _structural_zero(n):
            assert a.abs().max().item() < 5e-3 * max(1.0, b.abs().max().item()) + 1e-3, n
            continue
        err = (a - b).norm().item() / (b.norm().item() + 1e-12)
        assert err < 0.04, f"{n}: relative L2 error {err:.3e}"
