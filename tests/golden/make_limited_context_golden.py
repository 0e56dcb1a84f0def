"""Writes tests/golden/limited_context_cases.npz: rel-pos attention under a limited context, outputs and gradients of the reference.

Run by hand where the reference tree is at hand; never imported by a test:

    python tests/golden/make_limited_context_golden.py /path/to/NeMo

The reference is RelPositionMultiHeadAttention.forward with RelPositionalEncoding
(nemo/collections/asr/parts/submodules/multi_head_attention.py:157-250, :935-979), loaded by file path as
make_local_attention_golden.py loads it, in fp64, dropout 0, eval mode, linear_out = identity (the module's output IS the
attention context, a padded row is exactly zero).  Its `mask` argument is built here as ConformerEncoder._create_masks builds it
(nemo/collections/asr/modules/conformer_encoder.py:686-740) for self_attention_model 'rel_pos': triu / tril of a matrix of ones
for att_context_style 'regular', the chunk-index difference for 'chunked_limited' (left_chunks_num = L // (R + 1), 10000 for
L < 0; only triu(-L) when R == -1), and-ed with the padding of both axes, then inverted.

Cases (style, [L, R]; B, T, H, dk, lens): the seven contexts regular [8,3] [5,0] [-1,4], chunked_limited [8,3] [-1,6] [12,-1]
[70,13], with lengths that include 1 and 64 (a tile boundary of the kernels).  Inputs, weights and biases lie on dyadic grids
(int8 g, value = g / den); the position table is stored as the reference built it (fp32 sin / cos), outputs and gradients in fp64.

Stored per case i: x{i} [B,T,d] int8 (/ 16), wq / wk / wv / wp{i} [d,d] int8 (/ 32), bq / bk / bv{i} [d] int8 (/ 32),
u{i} / v{i} [H,dk] int8 (/ 32), pe{i} [2T-1, d] f32 (row r <-> relative position T-1-r), lens{i} [B] i64, out{i} [B,T,d] f64;
the upstream gradient g{i} [B,T,d] int8 (/ 8) of loss = sum(out o g) and the reference's autograd gradients dx{i} [B,T,d],
dwq / dwk / dwv / dwp{i} [d,d], du / dv{i} [H,dk] f64; per file: shape [n, 7] = (B, T, H, dk, style, L, R) with style 0 =
regular, 1 = chunked_limited, and name [n].

Before writing, the script asserts that an interval-masked fp64 restatement

    ctx[b,i,h,:] = sum_j softmax_j( ((q_i+u_h).k_j + (q_i+v_h).p_h[T-1-i+j]) / sqrt(dk) ) v_j ,   0 for i >= len_b
    regular:  i - L <= j <= i + R;   chunked, C = R + 1, n = L // C:  (i//C - n) C <= j <= (i//C + 1) C - 1;   j < len_b

(an unlimited side drops its bound; masked with -inf, where the reference fills -10000, which underflows to 0 after the softmax)
matches the reference to 1e-12 on valid frames, that padded rows are exactly zero, and that every gradient is finite and non-zero.
"""
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_local_attention_golden import load_reference  # noqa: E402

STYLES = ("regular", "chunked_limited")
CASES = [  # name, style, (L, R), B, T, H, dk, lens
    ("regular_8_3", "regular", (8, 3), 2, 66, 2, 4, [66, 1]),
    ("regular_5_0", "regular", (5, 0), 2, 66, 2, 4, [64, 33]),
    ("regular_m1_4", "regular", (-1, 4), 1, 65, 2, 4, [65]),
    ("chunked_8_3", "chunked_limited", (8, 3), 1, 66, 2, 4, [64]),
    ("chunked_m1_6", "chunked_limited", (-1, 6), 2, 50, 2, 4, [50, 1]),
    ("chunked_12_m1", "chunked_limited", (12, -1), 1, 64, 2, 4, [64]),
    ("chunked_70_13", "chunked_limited", (70, 13), 1, 100, 2, 4, [100]),
]
X_DEN, W_DEN, G_DEN = 16.0, 32.0, 8.0


def create_att_mask(style, L, R, lens, T):
    """ConformerEncoder._create_masks' att_mask [B,T,T] for 'rel_pos' (True = masked), restated."""
    m = torch.ones(1, T, T, dtype=torch.bool)
    if style == "regular":
        if L >= 0:
            m = m.triu(diagonal=-L)
        if R >= 0:
            m = m.tril(diagonal=R)
    elif R == -1:
        if L >= 0:
            m = m.triu(diagonal=-L)
    else:
        chunk = R + 1
        left_chunks = L // chunk if L >= 0 else 10000
        idx = torch.div(torch.arange(T, dtype=torch.int), chunk, rounding_mode="trunc")
        diff = idx.unsqueeze(1) - idx.unsqueeze(0)
        m = torch.logical_and(m, torch.logical_and(diff <= left_chunks, diff >= 0).unsqueeze(0))
    pad = torch.arange(T).expand(len(lens), -1) < torch.tensor(lens).unsqueeze(-1)
    pad2 = pad.unsqueeze(1).repeat([1, T, 1])
    pad2 = torch.logical_and(pad2, pad2.transpose(1, 2))
    return ~torch.logical_and(pad2, m)


def restate_fp64(x, W, lens, H, dk, style, L, R, pe):
    """Interval-masked attention context [B,T,d] in fp64: one interval of keys per query, position row T - 1 - i + j."""
    B, T, d = x.shape
    q = (x @ W["wq"].T + W["bq"]).view(B, T, H, dk).transpose(1, 2)
    k = (x @ W["wk"].T + W["bk"]).view(B, T, H, dk).transpose(1, 2)
    v = (x @ W["wv"].T + W["bv"]).view(B, T, H, dk).transpose(1, 2)
    p = (pe @ W["wp"].T).view(-1, H, dk).transpose(0, 1)                      # [H, 2T-1, dk]
    ok = torch.zeros(B, T, T, dtype=torch.bool)
    for b in range(B):
        for i in range(lens[b]):
            if style == "regular" or R < 0:
                lo = i - L if L >= 0 else 0
                hi = i + R if (R >= 0 and style == "regular") else T - 1
            else:
                C = R + 1
                lo = (i // C - L // C) * C if L >= 0 else 0
                hi = (i // C + 1) * C - 1
            lo, hi = max(lo, 0), min(hi, lens[b] - 1)
            ok[b, i, lo:hi + 1] = True
    i = torch.arange(T).view(T, 1)
    j = torch.arange(T).view(1, T)
    idx = T - 1 - i + j
    ac = (q + W["u"].view(1, H, 1, dk)) @ k.transpose(-2, -1)
    bd = torch.gather((q + W["v"].view(1, H, 1, dk)) @ p.unsqueeze(0).transpose(-2, -1), 3, idx.expand(B, H, T, T))
    s = ((ac + bd) / math.sqrt(dk)).masked_fill(~ok[:, None], -float("inf"))
    a = torch.softmax(s, dim=-1)
    a = torch.where(ok[:, None], a, torch.zeros_like(a))                       # (rows without a key: NaN -> 0)
    return (a @ v).transpose(1, 2).reshape(B, T, d)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    rng = np.random.default_rng(20261020)
    out, shapes, names = {}, [], []
    for ci, (name, style, (L, R), B, T, H, dk, lens) in enumerate(CASES):
        d = H * dk
        g = dict(x=rng.integers(-32, 33, size=(B, T, d)), wq=rng.integers(-16, 17, size=(d, d)), wk=rng.integers(-16, 17, size=(d, d)),
                 wv=rng.integers(-16, 17, size=(d, d)), wp=rng.integers(-16, 17, size=(d, d)), bq=rng.integers(-16, 17, size=d),
                 bk=rng.integers(-16, 17, size=d), bv=rng.integers(-16, 17, size=d), u=rng.integers(-16, 17, size=(H, dk)),
                 v=rng.integers(-16, 17, size=(H, dk)))
        W = {k: torch.from_numpy(a.astype(np.float64) / (X_DEN if k == "x" else W_DEN)) for k, a in g.items()}
        x = W.pop("x").requires_grad_(True)
        enc = ref.RelPositionalEncoding(d_model=d, dropout_rate=0.0, max_len=5000, xscale=None)
        enc.extend_pe(T, torch.device("cpu"))
        _, pe = enc(torch.zeros(1, T, d))
        assert pe.shape == (1, 2 * T - 1, d) and pe.dtype == torch.float32
        att = ref.RelPositionMultiHeadAttention(n_head=H, n_feat=d, dropout_rate=0.0, pos_bias_u=None, pos_bias_v=None).double().eval()
        with torch.no_grad():
            att.linear_q.weight.copy_(W["wq"]); att.linear_q.bias.copy_(W["bq"])
            att.linear_k.weight.copy_(W["wk"]); att.linear_k.bias.copy_(W["bk"])
            att.linear_v.weight.copy_(W["wv"]); att.linear_v.bias.copy_(W["bv"])
            att.linear_pos.weight.copy_(W["wp"])
            att.pos_bias_u.copy_(W["u"]); att.pos_bias_v.copy_(W["v"])
            att.linear_out.weight.copy_(torch.eye(d, dtype=torch.float64)); att.linear_out.bias.zero_()
        mask = create_att_mask(style, L, R, lens, T)
        y = att(x, x, x, mask, pe.double())
        with torch.no_grad():
            mine = restate_fp64(x.detach(), W, lens, H, dk, style, L, R, pe.double()[0])
        valid = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
        err = float((y.detach() - mine)[valid].abs().max())
        assert err <= 1e-12, f"{name}: reference and interval restatement differ by {err:.3e}"
        assert float(y.detach()[~valid].abs().max()) == 0.0 if (~valid).any() else True, f"{name}: padded rows are not zero"
        assert bool((~mask)[:, torch.arange(T), torch.arange(T)][valid].all()), f"{name}: a valid query lost its own key"
        gr = rng.integers(-8, 9, size=(B, T, d))
        (y * torch.from_numpy(gr.astype(np.float64) / G_DEN)).sum().backward()
        grads = dict(dx=x.grad, dwq=att.linear_q.weight.grad, dwk=att.linear_k.weight.grad, dwv=att.linear_v.weight.grad,
                     dwp=att.linear_pos.weight.grad, du=att.pos_bias_u.grad, dv=att.pos_bias_v.grad)
        for k, a in g.items():
            assert np.abs(a).max() <= 127
            out[f"{k}{ci}"] = a.astype(np.int8)
        out[f"pe{ci}"] = pe[0].numpy()
        out[f"lens{ci}"] = np.array(lens, dtype=np.int64)
        out[f"out{ci}"] = y.detach().numpy()
        out[f"g{ci}"] = gr.astype(np.int8)
        for k, t in grads.items():
            assert t is not None and torch.isfinite(t).all() and float(t.abs().max()) > 0.0, (name, k)
            out[f"{k}{ci}"] = t.numpy()
        print(f"{name}: |ref - restatement| = {err:.3e} on outputs up to {float(y.detach()[valid].abs().max()):.3f}; "
              + ", ".join(f"max|{k}| {float(t.abs().max()):.3f}" for k, t in grads.items()))
        shapes.append((B, T, H, dk, STYLES.index(style), L, R)); names.append(name)
    out["shape"], out["name"] = np.array(shapes, dtype=np.int64), np.array(names)
    dst = os.path.join(HERE, "limited_context_cases.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(CASES)} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
