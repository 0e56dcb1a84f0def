"""Writes tests/golden/local_attention_cases.npz: local (windowed) rel-pos attention cases and what the reference computes.

Run by hand where the reference tree is at hand; never imported by a test:

    python tests/golden/make_local_attention_golden.py [/path/to/NeMo]        (default /root/reference/NeMo)

The reference is RelPositionMultiHeadAttentionLongformer.forward with LocalAttRelPositionalEncoding
(nemo/collections/asr/parts/submodules/multi_head_attention.py:253-470, :982-1026), loaded by file path in fp64 with
nemo.utils.avoid_float16_autocast_context stubbed by contextlib.nullcontext (the only thing that file takes from the package),
no global tokens, dropout 0, eval mode.  linear_out is set to the identity (weight I, bias 0), so the module's output IS the
attention context before linear_out and a padded row (context 0 -> linear_out.bias) is exactly zero.

Cases (B, T, H, dk, [L, R], lens): four symmetric windows and two asymmetric ones.  Inputs, weights and biases lie on dyadic
grids (int8 g, value = g / den), so the file is small and the fp64 inputs are reproduced exactly; the position table is stored
as the reference built it (fp32 sin / cos), the output in fp64.

Stored per case i: x{i} [B,T,d] int8 (/ 16), wq / wk / wv / wp{i} [d,d] int8 (/ 32), bq / bk / bv{i} [d] int8 (/ 32),
u{i} / v{i} [H,dk] int8 (/ 32), pe{i} [L+R+1, d] f32 (row r <-> relative position L - r), lens{i} [B] i64, out{i} [B,T,d] f64;
per file: shape [n, 6] = (B, T, H, dk, L, R), name [n].

Before writing, the script asserts that a band-masked fp64 restatement

    ctx[b,i,h,:] = sum_j softmax_j( ((q_i+u_h).k_j + (q_i+v_h).p_h[w-i+j]) / sqrt(dk) ) v_j ,  |i-j| <= w, j < len_b;  0 for i >= len_b

matches the reference to 1e-12 on the symmetric cases and does NOT match it on the asymmetric ones (restated with the band
-L <= j-i <= R and p_h[L-i+j]): the reference adds the position term of an L != R window to the wrong columns (:355-360), which
this project does not reproduce -- it refuses asymmetric windows.
"""
import contextlib
import importlib.util
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

CASES = [  # name, B, T, H, dk, (L, R), lens
    ("sym_w4", 2, 50, 2, 8, (4, 4), [50, 33]),
    ("sym_w16", 2, 130, 2, 8, (16, 16), [130, 70]),
    ("sym_w64_full", 1, 65, 4, 4, (64, 64), [65]),
    ("sym_w5_len1", 2, 200, 2, 8, (5, 5), [200, 1]),
    ("asym_8_3", 1, 40, 2, 8, (8, 3), [40]),
    ("asym_3_8", 1, 40, 2, 8, (3, 8), [40]),
]
X_DEN, W_DEN = 16.0, 32.0


def load_reference(nemo_root):
    """The reference's multi_head_attention module, by file path, with the one import it takes from the package stubbed."""
    for name in ("nemo", "nemo.utils"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["nemo.utils"].avoid_float16_autocast_context = contextlib.nullcontext
    sys.modules["nemo"].utils = sys.modules["nemo.utils"]
    path = os.path.join(nemo_root, "nemo", "collections", "asr", "parts", "submodules", "multi_head_attention.py")
    spec = importlib.util.spec_from_file_location("ref_multi_head_attention", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def restate_fp64(x, W, lens, H, dk, L, R, pe):
    """Band-masked attention context [B,T,d] in fp64: keys -L <= j - i <= R, j < len; position row L - i + j."""
    B, T, d = x.shape
    q = (x @ W["wq"].T + W["bq"]).view(B, T, H, dk).transpose(1, 2)
    k = (x @ W["wk"].T + W["bk"]).view(B, T, H, dk).transpose(1, 2)
    v = (x @ W["wv"].T + W["bv"]).view(B, T, H, dk).transpose(1, 2)
    p = (pe @ W["wp"].T).view(-1, H, dk).transpose(0, 1)                      # [H, L+R+1, dk]
    i = torch.arange(T).view(T, 1)
    j = torch.arange(T).view(1, T)
    rel = j - i
    band = (rel >= -L) & (rel <= R)
    idx = (L + rel).clamp(0, L + R)
    ac = (q + W["u"].view(1, H, 1, dk)) @ k.transpose(-2, -1)
    bd = torch.gather((q + W["v"].view(1, H, 1, dk)) @ p.unsqueeze(0).transpose(-2, -1), 3, idx.expand(B, H, T, T))
    s = (ac + bd) / math.sqrt(dk)
    valid = torch.arange(T)[None, :] < torch.tensor(lens)[:, None]
    ok = band[None] & valid[:, None, :] & valid[:, :, None]
    s = s.masked_fill(~ok[:, None], -float("inf"))
    a = torch.softmax(s, dim=-1)
    a = torch.where(ok[:, None], a, torch.zeros_like(a))                       # (rows without a key: NaN -> 0)
    return (a @ v).transpose(1, 2).reshape(B, T, d)


def main():
    nemo_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/NeMo"
    ref = load_reference(nemo_root)
    rng = np.random.default_rng(20241020)
    out, shapes, names = {}, [], []
    for ci, (name, B, T, H, dk, (L, R), lens) in enumerate(CASES):
        d = H * dk
        g = dict(x=rng.integers(-32, 33, size=(B, T, d)), wq=rng.integers(-16, 17, size=(d, d)), wk=rng.integers(-16, 17, size=(d, d)),
                 wv=rng.integers(-16, 17, size=(d, d)), wp=rng.integers(-16, 17, size=(d, d)), bq=rng.integers(-16, 17, size=d),
                 bk=rng.integers(-16, 17, size=d), bv=rng.integers(-16, 17, size=d), u=rng.integers(-16, 17, size=(H, dk)),
                 v=rng.integers(-16, 17, size=(H, dk)))
        W = {k: torch.from_numpy(a.astype(np.float64) / (X_DEN if k == "x" else W_DEN)) for k, a in g.items()}
        x = W.pop("x")
        # the reference's position table for this window, as it builds it (fp32), then its module in fp64
        enc = ref.LocalAttRelPositionalEncoding(att_context_size=[L, R], d_model=d, dropout_rate=0.0, max_len=5000, xscale=None)
        enc.extend_pe(T, torch.device("cpu"))
        _, pe = enc(torch.zeros(1, T, d))
        assert pe.shape == (1, L + R + 1, d) and pe.dtype == torch.float32
        att = ref.RelPositionMultiHeadAttentionLongformer(n_head=H, n_feat=d, dropout_rate=0.0, pos_bias_u=None, pos_bias_v=None,
                                                          att_context_size=[L, R]).double().eval()
        with torch.no_grad():
            att.linear_q.weight.copy_(W["wq"]); att.linear_q.bias.copy_(W["bq"])
            att.linear_k.weight.copy_(W["wk"]); att.linear_k.bias.copy_(W["bk"])
            att.linear_v.weight.copy_(W["wv"]); att.linear_v.bias.copy_(W["bv"])
            att.linear_pos.weight.copy_(W["wp"])
            att.pos_bias_u.copy_(W["u"]); att.pos_bias_v.copy_(W["v"])
            att.linear_out.weight.copy_(torch.eye(d, dtype=torch.float64)); att.linear_out.bias.zero_()
            pad_mask = torch.arange(T)[None, :] >= torch.tensor(lens)[:, None]
            y = att(x, x, x, pad_mask, pe.double())
        mine = restate_fp64(x, W, lens, H, dk, L, R, pe.double()[0])
        valid = ~pad_mask
        err = float((y - mine)[valid].abs().max())
        scale = float(y[valid].abs().max())
        if L == R:
            assert err <= 1e-12, f"{name}: reference and band restatement differ by {err:.3e}"
            assert float(y[pad_mask].abs().max()) == 0.0 if pad_mask.any() else True, f"{name}: padded rows are not the bias"
        else:
            assert err > 1e-3, f"{name}: the asymmetric reference unexpectedly matches the band restatement ({err:.3e})"
        print(f"{name}: |ref - restatement| = {err:.3e} on outputs up to {scale:.3f}")
        for k, a in g.items():
            assert np.abs(a).max() <= 127
            out[f"{k}{ci}"] = a.astype(np.int8)
        out[f"pe{ci}"] = pe[0].numpy()
        out[f"lens{ci}"] = np.array(lens, dtype=np.int64)
        out[f"out{ci}"] = y.numpy()
        shapes.append((B, T, H, dk, L, R)); names.append(name)
    out["shape"], out["name"] = np.array(shapes, dtype=np.int64), np.array(names)
    dst = os.path.join(HERE, "local_attention_cases.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(CASES)} cases, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
