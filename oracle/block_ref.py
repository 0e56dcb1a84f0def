"""Functional fp64 / fp32 reference of ONE ConformerLayer (forward + autograd backward) with selectable rounding.

TEST INFRASTRUCTURE (see oracle/__init__.py): only tests/ import this file.

`conformer_layer(...)` computes the block of step_ref.ConformerLayer (conformer_modules.py:60-214 restated there) as plain
functions of a parameter dict, so that the same arithmetic can run

  rounding=None        plain math: the exact reference E (run it in fp64).  tests/test_block_reference.py pins it to
                       step_ref.ConformerLayer(...).double() -- output, input gradient, every parameter gradient and the
                       BatchNorm running statistics.
  rounding="executor"  rounds to bf16 exactly where the trainable block executor (csrc/block_train.hip) stores or consumes
                       bf16.  Run in fp64 (F64) and in fp32 (F32): the two differ only in summation order, so d(F32, F64)
                       is the noise scale the kernels' own fp32 accumulation order is allowed.

Rounding points of the executor (file:line of the csrc/ call each one mirrors):

  forward (straight-through: value rounded, gradient passed unchanged)
    bf16 weight images of the nine projections ........ ops/fast.py bf16_shadow, consumed by every ia_gemm_bf16 of the block
    y1..y4 = LayerNorm outputs ......................... block_train.hip:301, 306, 312, 328 (ia_layernorm -> bf16)
    h1p / h4p pre-activations, SiLU of the rounded value gemm_common.h:59-64 (outPre rounded, v = (float)bf16) ; :66-68
    h1 / h4 = dropout(SiLU(h_p)) ....................... block_train.hip:302, 329 (outH bf16)
    qkv, pl, ctx ....................................... block_train.hip:307, 308, 309
    c2 (pointwise conv 1), c3 = SiLU(BN(z)) ............ block_train.hip:313, 319 (c3 kept bf16 by the fused BN+SiLU GEMM)
    the residual stream x1..x4, z and the output stay fp32.
  backward (grad-only: the forward value untouched, the gradient rounded)
    dB = bf16(alpha * dropout(d x)) that each LayerNorm backward emits for the branch in front of it
                                                       block_train.hip:385, 393, 420 and 494 (ia_layernorm_bwd_drop)
    d h = bf16(acc) of the act-3 epilogue, d h_p = bf16(bf16(acc) * SiLU'(h_p) * keep)
                                                       gemm_common.h:73-80 ; block_train.hip:389, 497
    dy (into every LayerNorm backward) ................. block_train.hip:392, 419, 482, 507 (dX of the data-gradient GEMM, bf16)
    dc3 ................................................ block_train.hip:396
    dc2 ................................................ block_train.hip:410 (ia_dwconv_glu_bwd -> bf16)
    dctx ............................................... block_train.hip:423
    dqkv, dpl .......................................... attention_flash_bwd.hip (bf16 outputs of the core's backward)

The attention core rounds inside its online softmax in ways not worth emulating (bf16 band strip, P in bf16 against the
running maximum).  `splice=` replaces the core by given values: the forward returns the kernel's ctx and the backward
hands back the kernel's dqkv / dpl / d bias_u / d bias_v, recording the gradient that arrives at the core (the emulation's
dctx) in splice["dctx_ref"].

Dropout: `masks` = {name: keep-scaled [N, n] tensor} for the executor's counter-based masks (a test restates them);
None = no dropout.  Names: "ff1_h" (seed+1), "ff1_res" (seed+2), "att_res" (seed+3), "conv_res" (seed+4), "ff2_h" (seed+5),
"ff2_res" (seed+6).
"""
import math

import torch
import torch.nn.functional as F


PARAM_NAMES = (
    "norm_feed_forward1.weight", "norm_feed_forward1.bias",
    "feed_forward1.linear1.weight", "feed_forward1.linear1.bias", "feed_forward1.linear2.weight", "feed_forward1.linear2.bias",
    "norm_conv.weight", "norm_conv.bias",
    "conv.pointwise_conv1.weight", "conv.pointwise_conv1.bias", "conv.depthwise_conv.weight", "conv.depthwise_conv.bias",
    "conv.batch_norm.weight", "conv.batch_norm.bias", "conv.pointwise_conv2.weight", "conv.pointwise_conv2.bias",
    "norm_self_att.weight", "norm_self_att.bias",
    "self_attn.pos_bias_u", "self_attn.pos_bias_v",
    "self_attn.linear_q.weight", "self_attn.linear_q.bias", "self_attn.linear_k.weight", "self_attn.linear_k.bias",
    "self_attn.linear_v.weight", "self_attn.linear_v.bias", "self_attn.linear_out.weight", "self_attn.linear_out.bias",
    "self_attn.linear_pos.weight",
    "norm_feed_forward2.weight", "norm_feed_forward2.bias",
    "feed_forward2.linear1.weight", "feed_forward2.linear1.bias", "feed_forward2.linear2.weight", "feed_forward2.linear2.bias",
    "norm_out.weight", "norm_out.bias",
)


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


class _RoundFwd(torch.autograd.Function):
    """value rounded to bf16, gradient passed through (a bf16 store whose consumer's gradient is taken w.r.t. the fp32 value)"""

    @staticmethod
    def forward(ctx, x):
        return _bf16(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundGrad(torch.autograd.Function):
    """identity forward, gradient rounded to bf16 (a bf16 store in the backward)"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return _bf16(g)


class _Splice(torch.autograd.Function):
    """attention core replaced by given values (see the module docstring)"""

    @staticmethod
    def forward(ctx, qkv, pl, u, v, holder):
        ctx.holder, ctx.shapes = holder, (qkv.shape, pl.shape, u.shape, v.shape)
        return holder["ctx"].to(qkv.dtype).clone()

    @staticmethod
    def backward(ctx, g):
        h = ctx.holder
        h["dctx_ref"] = g.detach().clone()
        dt = g.dtype
        return tuple(h[k].to(dt).reshape(s) for k, s in zip(("dqkv", "dpl", "du", "dv"), ctx.shapes)) + (None,)


def params_of(module, dtype):
    """{name: detached leaf copy in `dtype`, requires_grad} for the PARAM_NAMES of a ConformerLayer (product or oracle)."""
    sd = dict(module.named_parameters())
    return {n: sd[n].detach().to("cpu", dtype).clone().requires_grad_(True) for n in PARAM_NAMES}


def _layernorm(x, g, b):
    return F.layer_norm(x, (x.shape[-1],), g, b, 1e-5)


def _rel_shift(x):   # step_ref.RelPositionMultiHeadAttention.rel_shift (multi_head_attention.py:184-195)
    b, h, qlen, pos_len = x.size()
    x = F.pad(x, pad=(1, 0))
    x = x.view(b, h, -1, qlen)
    return x[:, :, 1:].view(b, h, qlen, pos_len)


def relpos_attention(qkv, pl, u, v, lens, B, T, H):
    """qkv [B*T, 3d], pl [>= 2T-1, d] -> ctx [B*T, d]: step_ref.RelPositionMultiHeadAttention.forward without its projections
    (-10000 fill of the masked scores, masked probabilities zeroed: padded query rows give ctx = 0)."""
    d = qkv.shape[1] // 3
    dk = d // H
    q, k, vv = (qkv[:, i * d:(i + 1) * d].reshape(B, T, H, dk) for i in range(3))
    k, vv = k.transpose(1, 2), vv.transpose(1, 2)
    p = pl[:2 * T - 1].reshape(1, 2 * T - 1, H, dk).transpose(1, 2)
    q_u = (q + u).transpose(1, 2)
    q_v = (q + v).transpose(1, 2)
    ac = torch.matmul(q_u, k.transpose(-2, -1))
    bd = _rel_shift(torch.matmul(q_v, p.transpose(-2, -1)))[:, :, :, :T]
    scores = (ac + bd) / math.sqrt(dk)
    valid = torch.arange(T)[None, :] < lens.cpu()[:, None]
    m = ~(valid[:, :, None] & valid[:, None, :])
    m = m.unsqueeze(1)
    scores = scores.masked_fill(m, -10000.0)
    attn = torch.softmax(scores, dim=-1).masked_fill(m, 0.0)
    return torch.matmul(attn, vv).transpose(1, 2).reshape(B * T, d)


def conformer_layer(x, P, lens, pe, B, T, H, *, rounding=None, bn_state=None, bn_train=True, momentum=0.1, bn_eps=1e-5,
                    fc_factor=0.5, masks=None, splice=None):
    """x [B*T, d] (residual stream), P = params_of(...), lens [B], pe [>= 2T-1, d] position table (the executor's bf16 values),
    bn_state = [running_mean, running_var, num_batches_tracked] updated in place (train-mode BatchNorm) or read (eval).
    Returns the block output [B*T, d].  Dtype = that of x and P."""
    if rounding not in (None, "executor"):
        raise ValueError(rounding)
    ex = rounding == "executor"
    rf = _RoundFwd.apply if ex else (lambda t: t)
    rg = _RoundGrad.apply if ex else (lambda t: t)
    N, d = x.shape
    dt = x.dtype
    M = masks or {}

    def mask(name):
        m = M.get(name)
        return 1.0 if m is None else m.to(dt)

    def lin(a, w, b=None):
        y = a @ rf(P[w]).reshape(P[w].shape[0], -1).t()
        return y if b is None else y + P[b]

    def ffn(x_in, ln, ff, hm, rm):
        y = rg(rf(_layernorm(x_in, P[ln + ".weight"], P[ln + ".bias"])))
        hp = rg(rf(lin(y, ff + ".linear1.weight", ff + ".linear1.bias")))
        h = rg(rf(F.silu(hp) * mask(hm)))
        return x_in + rg(lin(h, ff + ".linear2.weight", ff + ".linear2.bias")) * (fc_factor * mask(rm))

    x1 = ffn(x, "norm_feed_forward1", "feed_forward1", "ff1_h", "ff1_res")
    # self-attention
    y2 = rg(rf(_layernorm(x1, P["norm_self_att.weight"], P["norm_self_att.bias"])))
    qkv = rg(rf(torch.cat([lin(y2, f"self_attn.linear_{c}.weight", f"self_attn.linear_{c}.bias") for c in "qkv"], dim=1)))
    pl = rg(rf(lin(pe.to(dt), "self_attn.linear_pos.weight")))
    dk = d // H
    u, v = P["self_attn.pos_bias_u"], P["self_attn.pos_bias_v"]
    if splice is not None:
        ctx = _Splice.apply(qkv, pl, u, v, splice)
    else:
        ctx = relpos_attention(qkv, pl, u.reshape(H, dk), v.reshape(H, dk), lens, B, T, H)
    ctx = rg(rf(ctx))
    x2 = x1 + rg(lin(ctx, "self_attn.linear_out.weight", "self_attn.linear_out.bias")) * mask("att_res")
    # convolution module
    y3 = rg(rf(_layernorm(x2, P["norm_conv.weight"], P["norm_conv.bias"])))
    c2 = rg(rf(lin(y3, "conv.pointwise_conv1.weight", "conv.pointwise_conv1.bias")))
    g = c2[:, :d] * torch.sigmoid(c2[:, d:])
    valid = (torch.arange(T)[None, :] < lens.cpu()[:, None]).reshape(N, 1)
    g = g.masked_fill(~valid, 0.0)                                       # conformer_modules.py:351 (pad mask before the conv)
    ksz = P["conv.depthwise_conv.weight"].shape[-1]
    z = F.conv1d(F.pad(g.reshape(B, T, d).transpose(1, 2), ((ksz - 1) // 2, (ksz - 1) // 2)), P["conv.depthwise_conv.weight"],
                 P["conv.depthwise_conv.bias"], groups=d)                 # [B, d, T]
    rm, rv, nbt = bn_state
    if bn_train:   # batch statistics over every frame, padded ones included (BatchNorm1d over [B, d, T])
        mean = z.mean(dim=(0, 2))
        var = z.var(dim=(0, 2), unbiased=False)
        with torch.no_grad():
            n = B * T
            rm.mul_(1 - momentum).add_(momentum * mean.detach().to(rm.dtype))
            rv.mul_(1 - momentum).add_(momentum * (var.detach() * (n / (n - 1))).to(rv.dtype))
            nbt.add_(1)
    else:
        mean, var = rm.to(dt), rv.to(dt)
    zn = (z - mean[None, :, None]) / torch.sqrt(var[None, :, None] + bn_eps)
    zn = zn * P["conv.batch_norm.weight"][None, :, None] + P["conv.batch_norm.bias"][None, :, None]
    c3 = rg(rf(F.silu(zn).transpose(1, 2).reshape(N, d)))
    x3 = x2 + rg(lin(c3, "conv.pointwise_conv2.weight", "conv.pointwise_conv2.bias")) * mask("conv_res")
    x4 = ffn(x3, "norm_feed_forward2", "feed_forward2", "ff2_h", "ff2_res")
    return _layernorm(x4, P["norm_out.weight"], P["norm_out.bias"])


def run_block(x, P, lens, pe, B, T, H, dout=None, **kw):
    """Forward (+ backward of sum(out * dout) when dout is given) of conformer_layer on leaf copies.
    Returns (out, dx or None, {name: grad} or None)."""
    xl = x.detach().clone().requires_grad_(dout is not None)
    if dout is None:
        with torch.no_grad():
            return conformer_layer(xl, P, lens, pe, B, T, H, **kw), None, None
    for q in P.values():
        q.grad = None
    out = conformer_layer(xl, P, lens, pe, B, T, H, **kw)
    out.backward(dout.to(out.dtype))
    return out.detach(), xl.grad.detach(), {n: q.grad.detach().clone() for n, q in P.items()}
