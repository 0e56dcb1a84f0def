"""The Conformer block executors held to a rounding-faithful fp64 reference (oracle/block_ref.py).

K = the kernel's result, E = exact math in fp64 (rounding=None), F64 / F32 = the executor's bf16 rounding points emulated in
fp64 / fp32 (rounding="executor").  F32 and F64 differ only in fp32 summation order, so d(F32, F64) is the noise the kernels'
own fp32 accumulation order may add.  Every compared tensor is measured twice -- relative L2 and max-abs distance, both scaled
by the reference tensor's norm / max -- and row tensors separately over valid and padded frames, so that a bug confined to a
few rows cannot hide in an average.  Two bounds, and no other:

  (a) d(K, F64) <= C * d(F32, F64) + FLOOR      C = 4 for the whole file
  (b) d(K, E)   <= 2 * d(F64, E) + FLOOR        the kernel is at most twice as far from exact math as the emulation

C = 4, not 1: beyond its summation order the kernel evaluates sigmoid / SiLU with the hardware exp2 and reciprocal
(csrc/ia_common.h ia_sigmoid_fast, a few fp32 ulps) and the BatchNorm variance in one pass (E[z^2] - mean^2), and every
such fp32-sized difference is amplified exactly like the summation noise: by the values it moves across a bf16 rounding
boundary downstream.  What (a) allows is not small: d(F32, F64) is 0.3-1.2x d(F64, E) (0.3x for the output, ~0.7x for dx,
0.5-0.9x for most parameter gradients), so C = 4 admits an extra error of up to a few times the whole bf16 rounding effect.
The worst ratios d(K, ref) / d(other, ref) are printed per case; observed: up to 3.3 under (a) (relative L2 of a LayerNorm
gamma gradient at d = 256, else <= 1.6) and up to 1.6 under (b).  Single-line faults in the kernels -- the conv pad mask
one frame short, running_var from the biased variance, fc_factor dropped from a branch gradient, bias_u read for bias_v in
the attention backward -- each fail these tests; a keep scale of 1/(1-p) instead of 256/(256-thr) is what the exact mask
checks of the dropout case are for.
FLOOR = 2^-20 (relative): the bound for tensors where F32 equals F64 or both are fp32-exact (the spliced pos_bias gradients,
num_batches_tracked, the structurally zero linear_k / depthwise-conv bias gradients).  It is 8 fp32 ulps, and covers the
fp32 rounding of the add into the pre-filled .grad buffers (<= 2^-24 of |prefill| + |grad|, prefill ~ the gradient's scale).
The structurally zero gradients (their exact value is 0) are scaled by the norm of the same module's weight gradient; the
linear_k bias gradient is pure bf16 noise of the attention core's dK and is held by the derivation written beside it.
Parameter gradients are sums over every row: one bf16 rounding that lands the other way in a single summand (dy, dB, ...)
moves one element by up to 2^-8 of that summand, a quantum d(F32, F64) need not contain.  Their relative L2 distance is held
by (a) and (b), their max-abs distance by (b) only.

The attention core rounds inside its online softmax (bf16 band strip, P in bf16) in ways the emulation does not follow, so
for (a) the kernel's own values are spliced in at the core's boundary: its ctx in the forward, its dqkv / dpl / d bias in the
backward (read from ops/fast.relpos_attention_flash_bwd), and the kernel's dctx is compared with the emulation's under (a).
The core itself is held by (b) end to end and by tests/test_attention_flash*_gpu.py.

The frozen-prefix executor (csrc/block_exec.hip) is held by (b) only.  It rounds at other points than the trainable executor
the emulation follows (the fused feed-forward module and its q|k|v tail, LayerNorm in the linear_out GEMM's epilogue, the GLU
in the pointwise GEMM's epilogue with fixed-point BatchNorm sums), and its one native call leaves no place to splice the
attention core.  The per-op forward_fast chain runs other kernels again, so it is no bit-for-bit partner either.
"""
import numpy as np
import pytest
import torch

from oracle import block_ref as R

pytestmark = pytest.mark.gpu

C = 4.0
FLOOR = 2.0 ** -20
STRUCT_ZERO = {"conv.depthwise_conv.bias": "conv.depthwise_conv.weight", "self_attn.linear_k.bias": "self_attn.linear_k.weight"}

#            name        d   H  d_ff  B    T   lens
CASES = [("configs0", 144, 4, 576, 3, 126, (126, 64, 1)),
         ("configs1-3", 256, 4, 1024, 4, 376, (376, 300, 65, 1)),
         ("configs4", 512, 8, 2048, 2, 751, (751, 500)),
         ("tile_edge", 256, 4, 1024, 3, 65, (65, 64, 63)),
         ("sub_tile", 144, 4, 576, 2, 17, (17, 9))]


def _layer(d, H, d_ff, p, seed):
    from indic_cl_asr_amd.encoder import ConformerLayer
    torch.manual_seed(seed)
    layer = ConformerLayer(d, d_ff, H, 31, p, 0.0).cuda().train()
    with torch.no_grad():
        layer.self_attn.pos_bias_u.normal_(0, 0.2); layer.self_attn.pos_bias_v.normal_(0, 0.2)
        layer.conv.batch_norm.weight.uniform_(0.5, 1.5); layer.conv.batch_norm.bias.normal_(0, 0.2)
        layer.conv.batch_norm.running_mean.normal_(0, 0.1); layer.conv.batch_norm.running_var.uniform_(0.5, 2.0)
        for n in ("norm_feed_forward1", "norm_self_att", "norm_conv", "norm_feed_forward2", "norm_out"):
            ln = getattr(layer, n)
            ln.weight.uniform_(0.7, 1.3); ln.bias.normal_(0, 0.1)
    return layer


def _inputs(d, B, T, lens, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B * T, d, generator=g)
    pe = (torch.randn(2 * T - 1, d, generator=g) * 0.5).to(torch.bfloat16)
    dout = torch.randn(B * T, d, generator=g)
    valid = (torch.arange(T)[None, :] < torch.tensor(lens)[:, None]).reshape(-1)
    return x, pe, dout, valid


# ---------------------------------------------------------------------------------------------------- dropout restated
def _hash32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13)); x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def keep_mask(seed, M, N, p):
    """csrc/dropout_mask.h ia_keep8 + the epilogue's scale (ia_common.h ia_dropout_rule: thr = (unsigned)(p*256 + 0.5) in fp32, keep if the
    byte >= thr, kept values * 256 / (256 - thr)): [M, N] float32 tensor of 0 / keep_scale."""
    thr = int(np.float32(p) * np.float32(256.0) + np.float32(0.5))
    if thr == 0:
        return torch.ones(M, N)
    with np.errstate(over="ignore"):
        gm = np.arange(M, dtype=np.uint32)[:, None]
        gn = np.arange(0, N, 8, dtype=np.uint32)[None, :]
        base = (gm * np.uint32(N) + gn) * np.uint32(0x9E3779B1) + np.uint32(seed & 0xFFFFFFFF)
        r = [_hash32(base), _hash32(base ^ np.uint32(0x68E31DA4))]
    cols = [((r[j // 4] >> np.uint32(8 * (j % 4))) & np.uint32(255)) >= thr for j in range(8)]
    keep = np.stack(cols, axis=-1).reshape(M, N)
    scale = np.float32(256.0) / (np.float32(256.0) - np.float32(thr))
    return torch.from_numpy(keep.astype(np.float32) * scale)


# ---------------------------------------------------------------------------------------------------- distances
def _dist(a, b, scale_l2, scale_max):
    e = (a - b)
    return float(e.norm()) / scale_l2, float(e.abs().max()) / scale_max


def _check(tag, K, ref, other, factor, rows=None, scale=None, log=None, max_abs=True):
    """d(K, ref) <= factor * d(other, ref) + FLOOR, relative L2 and (max_abs) max-abs, over valid and padded rows separately."""
    parts = [("", None)] if rows is None else [("valid", rows), ("padded", ~rows)]
    for pn, sel in parts:
        k, r, o = (t if sel is None else t[sel] for t in (K, ref, other))
        if r.numel() == 0:
            continue
        s2 = scale if scale is not None else max(float(r.norm()), 1e-30)
        sm = scale if scale is not None else max(float(r.abs().max()), 1e-30)
        if scale is not None:
            s2, sm = scale, scale / max(r.numel(), 1) ** 0.5
        kl, km = _dist(k, r, s2, sm)
        ol, om = _dist(o, r, s2, sm)
        if log is not None:   # the ratios the bounds hold (printed per case: the headroom under `factor`)
            log.append((f"{tag}{'/' + pn if pn else ''}", "L2", kl / max(ol, FLOOR)))
            if max_abs:
                log.append((f"{tag}{'/' + pn if pn else ''}", "max", km / max(om, FLOOR)))
        assert kl <= factor * ol + FLOOR, (tag, pn, "rel L2", kl, ol)
        if max_abs:
            assert km <= factor * om + FLOOR, (tag, pn, "max abs", km, om)


# ---------------------------------------------------------------------------------------------------- trainable executor
def _reference(layer, x, pe_pad, dout, lens, B, T, H, dtype, rounding, masks=None, splice=None):
    bn = layer.conv.batch_norm
    state = [bn.running_mean.detach().cpu().to(dtype).clone(), bn.running_var.detach().cpu().to(dtype).clone(),
             bn.num_batches_tracked.cpu().clone()]
    P = R.params_of(layer, dtype)
    m = None if masks is None else {k: v.to(dtype) for k, v in masks.items()}
    out, dx, G = R.run_block(x.to(dtype), P, torch.tensor(lens), pe_pad.float().to(dtype), B, T, H, dout=dout.to(dtype),
                             rounding=rounding, bn_state=state, fc_factor=layer.fc_factor, masks=m, splice=splice)
    res = {"out": out, "dx": dx, "running_mean": state[0], "running_var": state[1], "num_batches_tracked": state[2]}
    res.update({"grad:" + n: g for n, g in G.items()})
    return {k: v.double() for k, v in res.items()}


def _kernel(layer, x, pe_pad, dout, lens, B, T, seed, native, prefill, monkeypatch):
    from indic_cl_asr_amd.ops import block, fast
    cap = {}
    orig = fast.relpos_attention_flash_bwd

    def spy(qkv, pl, bu, bv, lens_, ctx, dctx, lse, *a, **kw):
        r = orig(qkv, pl, bu, bv, lens_, ctx, dctx, lse, *a, **kw)
        cap.update(ctx=ctx.double().cpu(), dctx=dctx.double().cpu(), dqkv=r[0].double().cpu(), dpl=r[1].double().cpu(),
                   du=r[2].double().cpu(), dv=r[3].double().cpu())
        return r

    monkeypatch.setattr(fast, "relpos_attention_flash_bwd", spy)
    monkeypatch.setattr(block, "USE_NATIVE_BLOCKS", native)
    bn = layer.conv.batch_norm
    bn0 = (bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone())
    for n, q in layer.named_parameters():
        q.grad = prefill[n].cuda().clone()              # the executor ADDS into existing .grad buffers
    xg = x.cuda().requires_grad_(True)
    lens_d = torch.tensor(lens, device="cuda")
    out = block.conformer_block(xg, layer, lens_d, pe_pad.cuda(), B, T, seed)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    res = {"out": out.detach().double().cpu(), "dx": xg.grad.double().cpu(), "running_mean": bn.running_mean.double().cpu(),
           "running_var": bn.running_var.double().cpu(), "num_batches_tracked": bn.num_batches_tracked.double().cpu()}
    for n, q in layer.named_parameters():
        res["grad:" + n] = q.grad.double().cpu() - prefill[n].double()
    with torch.no_grad():
        bn.running_mean.copy_(bn0[0]); bn.running_var.copy_(bn0[1]); bn.num_batches_tracked.copy_(bn0[2])
    for q in layer.parameters():
        q.grad = None
    monkeypatch.undo()
    return res, cap


def _prefill(E):
    g = torch.Generator().manual_seed(1)
    out = {}
    for k, v in E.items():
        if k.startswith("grad:"):
            n = k[5:]
            s = E["grad:" + STRUCT_ZERO[n]] if n in STRUCT_ZERO else v
            out[n] = (torch.randn(v.shape, generator=g, dtype=torch.float64) * 0.5 * float(s.pow(2).mean().sqrt())).float()
    return out


def _scale(E, k):
    n = k[5:] if k.startswith("grad:") else None
    return float(E["grad:" + STRUCT_ZERO[n]].norm()) if n in STRUCT_ZERO else None


def _compare_block(layer, x, pe_pad, dout, valid, lens, B, T, H, seed, monkeypatch, masks=None):
    E = _reference(layer, x, pe_pad, dout, lens, B, T, H, torch.float64, None, masks)
    F64 = _reference(layer, x, pe_pad, dout, lens, B, T, H, torch.float64, "executor", masks)
    prefill = _prefill(E)
    log = []
    for native in (True, False):
        K, cap = _kernel(layer, x, pe_pad, dout, lens, B, T, seed, native, prefill, monkeypatch)
        sp64, sp32 = dict(cap), dict(cap)
        F64s = _reference(layer, x, pe_pad, dout, lens, B, T, H, torch.float64, "executor", masks, splice=sp64)
        F32s = _reference(layer, x, pe_pad, dout, lens, B, T, H, torch.float32, "executor", masks, splice=sp32)
        path = "native" if native else "python"
        assert torch.equal(K["num_batches_tracked"], E["num_batches_tracked"])
        for k in K:
            if k == "num_batches_tracked":
                continue
            rows = valid if K[k].shape[0] == B * T and k in ("out", "dx") else None
            if k == "grad:self_attn.linear_k.bias":
                # exactly 0 in E (softmax drops a per-query constant); the kernel's value is the column sum of its bf16-rounded
                # dK rows (each off by <= 2^-9 of itself), so |value| <= 2^-9 * sum |dK| per channel -- bound with 2^-8
                dk_sum = cap["dqkv"][:, layer.norm_out.weight.shape[0]:2 * layer.norm_out.weight.shape[0]].abs().sum(0)
                assert (K[k].abs() <= 2.0 ** -8 * dk_sum + FLOOR * _scale(E, k)).all(), k
                _check(f"{path}:{k}:(a)", K[k], F64s[k], F32s[k], C, None, _scale(E, k), log)
                continue
            grad = k.startswith("grad:")
            _check(f"{path}:{k}:(a)", K[k], F64s[k], F32s[k], C, rows, _scale(E, k), log, max_abs=not grad)
            _check(f"{path}:{k}:(b)", K[k], E[k], F64[k], 2.0, rows, _scale(E, k), log)
        _check(f"{path}:dctx:(a)", cap["dctx"], sp64["dctx_ref"], sp32["dctx_ref"].double(), C, valid, None, log)
    for bound in ("(a)", "(b)"):
        for metric in ("L2", "max"):
            worst = max((r for r in log if bound in r[0] and r[1] == metric), key=lambda r: r[2])
            print(f"worst {bound} {metric} ratio d(K, ref) / d(other, ref): {worst[2]:.3f} at {worst[0]}")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_trainable_block_matches_rounding_faithful_reference(case, monkeypatch):
    name, d, H, d_ff, B, T, lens = case
    layer = _layer(d, H, d_ff, 0.0, d + T)
    x, pe, dout, valid = _inputs(d, B, T, lens, T)
    from indic_cl_asr_amd.ops import block
    pe_pad = block.pad_pos_emb(pe.float().unsqueeze(0), d).cpu()
    _compare_block(layer, x, pe_pad, dout, valid, lens, B, T, H, 1234 + d, monkeypatch)


def test_trainable_block_with_dropout_matches_reference(monkeypatch):
    """The block's dropouts at the config rate (0.1; attention-probability dropout 0, its replay is tested in
    test_attention_flash_bwd_gpu.py): the restated masks reproduce the executor's GEMM-epilogue masks bit for bit, then the
    reference applies them."""
    from indic_cl_asr_amd.ops import block, fast
    d, H, d_ff, B, T, lens, p, seed = 256, 4, 1024, 3, 200, (200, 151, 37), 0.1, 0x7FFFFFF0
    N = B * T
    spec = {"ff1_h": (1, d_ff), "ff1_res": (2, d), "att_res": (3, d), "conv_res": (4, d), "ff2_h": (5, d_ff), "ff2_res": (6, d)}
    masks = {k: keep_mask(seed + s, N, n, p) for k, (s, n) in spec.items()}
    for k, (s, n) in spec.items():   # the epilogue's own masks: ones @ (ones/8)^T = 1 exactly, dropout applied
        a = torch.ones(N, 8, dtype=torch.bfloat16, device="cuda")
        w = torch.full((n, 8), 0.125, dtype=torch.bfloat16, device="cuda")
        out, _ = fast.gemm(a, w, dropout_p=p, seed=(seed + s) & 0xFFFFFFFF, out_f32=torch.empty(N, n, device="cuda"),
                           want_bf16=False)
        assert torch.equal(out.cpu(), masks[k]), k
        assert 0.85 < float((masks[k] > 0).float().mean()) < 0.95
    g = torch.Generator().manual_seed(3)
    for k, (s, n) in spec.items():   # the kernels that regenerate the masks elsewhere
        v = torch.randn(N, n, generator=g)
        # branch gradient of the backward (ia_scale_dropout_bf16; ia_layernorm_bwd_drop emits the same bits, see
        # test_block_native_gpu.py): bf16((v * alpha) * keep_scale) where kept, 0 elsewhere -- values too, not just the pattern
        got = block._branch_grad(v.cuda(), 0.5, p, seed + s).cpu()
        want = torch.where(masks[k] > 0, (v * 0.5) * masks[k], torch.zeros(())).to(torch.bfloat16)
        assert torch.equal(got, want), k
        if n == d_ff:   # SiLU dropout of the per-op path, forward and backward (ia_silu_dropout[_bwd], on [N, d_ff] there)
            hp = v.to(torch.bfloat16).cuda()
            dh = torch.randn(N, n, generator=g).to(torch.bfloat16).cuda()
            assert torch.equal(block._silu_dropout(hp, p, seed + s).cpu() != 0, masks[k] > 0), k
            assert torch.equal(block._silu_dropout_bwd(hp, dh, p, seed + s).cpu() != 0, masks[k] > 0), k
    layer = _layer(d, H, d_ff, p, 7)
    x, pe, dout, valid = _inputs(d, B, T, lens, 8)
    pe_pad = block.pad_pos_emb(pe.float().unsqueeze(0), d).cpu()
    _compare_block(layer, x, pe_pad, dout, valid, lens, B, T, H, seed, monkeypatch, masks=masks)


# ---------------------------------------------------------------------------------------------------- frozen prefix
def _prefix_reference(layers, x, pe, lens, B, T, H, rounding, train):
    xr = x.double()
    states = []
    for layer in layers:
        bn = layer.conv.batch_norm
        st = [bn.running_mean.detach().cpu().double().clone(), bn.running_var.detach().cpu().double().clone(),
              bn.num_batches_tracked.cpu().clone()]
        xr, _, _ = R.run_block(xr, R.params_of(layer, torch.float64), torch.tensor(lens), pe.double(), B, T, H, rounding=rounding,
                               bn_state=st, bn_train=train, fc_factor=layer.fc_factor)
        states.append(st)
    return xr, states


@pytest.mark.parametrize("frozen", [True, False], ids=["frozen", "trainable_params"])
@pytest.mark.parametrize("train", [True, False], ids=["train_bn", "eval_bn"])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_frozen_prefix_matches_reference(case, train, frozen):
    """ops/fast.conformer_prefix (csrc/block_exec.hip, one native call for two chained blocks; at d = 256 through ffn_fused and
    its q|k|v tail) and the per-op forward_fast chain _fast_prefix falls back to: output and running statistics under (b)."""
    from indic_cl_asr_amd.ops import fast
    name, d, H, d_ff, B, T, lens = case
    layers = [_layer(d, H, d_ff, 0.0, d + T + i) for i in range(2)]
    for layer in layers:
        layer.train(train)
        # frozen layers (as in the step) take the executor's cached position projection (fast.pos_proj_cached, pl_cached in
        # block_exec.hip); layers with trainable parameters make it recompute linear_pos itself
        layer.requires_grad_(not frozen)
    x, pe, _, valid = _inputs(d, B, T, lens, T + 1)
    E, E_st = _prefix_reference(layers, x, pe, lens, B, T, H, None, train)
    F64, F_st = _prefix_reference(layers, x, pe, lens, B, T, H, "executor", train)
    lens_d = torch.tensor(lens, device="cuda")
    pe_d = pe.cuda().contiguous()
    for path in ("native", "per_op"):
        saved = [(l.conv.batch_norm.running_mean.clone(), l.conv.batch_norm.running_var.clone(),
                  l.conv.batch_norm.num_batches_tracked.clone()) for l in layers]
        xr = x.cuda().contiguous()
        with torch.no_grad():
            if path == "native":
                fast.conformer_prefix(layers, xr, pe_d, lens_d, B, T, 99, 16, train)
            else:
                y = None
                for i, layer in enumerate(layers):
                    nxt = layers[i + 1].norm_feed_forward1 if i + 1 < len(layers) else None
                    xr, y = layer.forward_fast(xr, y, lens_d, pe_d, B, T, 99 + 16 * i, nxt)
        torch.cuda.synchronize()
        _check(f"{path}:out:(b)", xr.double().cpu(), E, F64, 2.0, valid)
        for i, layer in enumerate(layers):
            bn = layer.conv.batch_norm
            for j, nm in enumerate(("running_mean", "running_var")):
                _check(f"{path}:{i}:{nm}:(b)", getattr(bn, nm).double().cpu(), E_st[i][j], F_st[i][j], 2.0)
            assert int(bn.num_batches_tracked) == int(E_st[i][2])
        with torch.no_grad():
            for layer, (rm, rv, nb) in zip(layers, saved):
                bn = layer.conv.batch_norm
                bn.running_mean.copy_(rm); bn.running_var.copy_(rv); bn.num_batches_tracked.copy_(nb)
