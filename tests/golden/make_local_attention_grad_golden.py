"""Writes tests/golden/local_attention_grad_cases.npz: what the reference's local rel-pos attention gives as GRADIENTS.

Run by hand where the reference tree is at hand; never imported by a test:

    python tests/golden/make_local_attention_grad_golden.py /path/to/NeMo

The four symmetric cases of tests/golden/local_attention_cases.npz (sym_w4, sym_w16, sym_w64_full, sym_w5_len1) are read back
from that file -- inputs, weights, biases and the position table are not stored twice -- and pushed through the reference's
RelPositionMultiHeadAttentionLongformer exactly as make_local_attention_golden.py does (loaded by file path, fp64, eval, dropout
0, linear_out = identity), now with autograd on.  Loss = sum(out o g) with g on a dyadic int8 grid (value = g / 8), so the
upstream gradient is reproduced exactly.

Stored per case i (the index in local_attention_cases.npz): g{i} [B,T,d] int8 (/ 8) and the fp64 gradients dx{i} [B,T,d],
dwq / dwk / dwv / dwp{i} [d,d], du / dv{i} [H,dk]; per file: case [n] = those indices, name [n].

Before writing, the script asserts that the stored forward output is reproduced bit for bit (same module, same inputs) and
that every gradient is finite and non-zero.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_local_attention_golden import load_reference  # noqa: E402

G_DEN = 8.0


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = load_reference(sys.argv[1])
    Z = np.load(os.path.join(HERE, "local_attention_cases.npz"))
    rng = np.random.default_rng(20241021)
    out, cases, names = {}, [], []
    for ci, shape in enumerate(Z["shape"]):
        B, T, H, dk, L, R = (int(v) for v in shape)
        if L != R:
            continue
        d = H * dk
        f = lambda k, den: torch.from_numpy(Z[f"{k}{ci}"].astype(np.float64) / den)
        x = f("x", 16.0).requires_grad_(True)
        lens = Z[f"lens{ci}"].tolist()
        pe = torch.from_numpy(Z[f"pe{ci}"]).double().unsqueeze(0)
        att = ref.RelPositionMultiHeadAttentionLongformer(n_head=H, n_feat=d, dropout_rate=0.0, pos_bias_u=None, pos_bias_v=None,
                                                          att_context_size=[L, R]).double().eval()
        with torch.no_grad():
            att.linear_q.weight.copy_(f("wq", 32.0)); att.linear_q.bias.copy_(f("bq", 32.0))
            att.linear_k.weight.copy_(f("wk", 32.0)); att.linear_k.bias.copy_(f("bk", 32.0))
            att.linear_v.weight.copy_(f("wv", 32.0)); att.linear_v.bias.copy_(f("bv", 32.0))
            att.linear_pos.weight.copy_(f("wp", 32.0))
            att.pos_bias_u.copy_(f("u", 32.0)); att.pos_bias_v.copy_(f("v", 32.0))
            att.linear_out.weight.copy_(torch.eye(d, dtype=torch.float64)); att.linear_out.bias.zero_()
        pad_mask = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
        y = att(x, x, x, pad_mask, pe)
        assert np.array_equal(y.detach().numpy(), Z[f"out{ci}"]), f"{Z['name'][ci]}: the stored forward output is not reproduced"
        g = rng.integers(-8, 9, size=(B, T, d))
        (y * torch.from_numpy(g.astype(np.float64) / G_DEN)).sum().backward()
        grads = dict(dx=x.grad, dwq=att.linear_q.weight.grad, dwk=att.linear_k.weight.grad, dwv=att.linear_v.weight.grad,
                     dwp=att.linear_pos.weight.grad, du=att.pos_bias_u.grad, dv=att.pos_bias_v.grad)
        out[f"g{ci}"] = g.astype(np.int8)
        for k, t in grads.items():
            assert t is not None and torch.isfinite(t).all() and float(t.abs().max()) > 0.0, (str(Z["name"][ci]), k)
            out[f"{k}{ci}"] = t.numpy()
        print(f"{Z['name'][ci]}: " + ", ".join(f"max|{k}| {float(t.abs().max()):.3f}" for k, t in grads.items()))
        cases.append(ci); names.append(str(Z["name"][ci]))
    out["case"], out["name"] = np.array(cases, dtype=np.int64), np.array(names)
    dst = os.path.join(HERE, "local_attention_grad_cases.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(cases)} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
