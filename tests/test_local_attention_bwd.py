"""Local rel-pos attention backward on the host: the oracle and the entry points' argument checks.

The GPU tests (tests/test_local_attention_bwd_gpu.py) hold csrc/attention_flash_bwd.hip under its local span to fp64 autograd of the band-masked
composition ops.rel_pos_attention(window=w).  Here that composition's own gradients are held to the reference's
(RelPositionMultiHeadAttentionLongformer in fp64, tests/golden/make_local_attention_grad_golden.py) to 1e-10 relative: two fp64
evaluations of the same function in different summation orders.  The C entry points answer every bad argument before a launch.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from indic_cl_asr_amd import _lib, ops

Z = np.load(os.path.join(GOLDEN, "local_attention_cases.npz"))
G = np.load(os.path.join(GOLDEN, "local_attention_grad_cases.npz"))
CASES = [int(c) for c in G["case"]]
NAMES = [str(n) for n in G["name"]]


def test_fixture_holds_the_four_symmetric_cases():
    assert NAMES == ["sym_w4", "sym_w16", "sym_w64_full", "sym_w5_len1"]
    assert [str(Z["name"][c]) for c in CASES] == NAMES
    assert all(int(Z["shape"][c][4]) == int(Z["shape"][c][5]) for c in CASES)


@pytest.mark.parametrize("ci", CASES, ids=NAMES)
def test_composition_gradients_match_reference_fp64(ci):
    B, T, H, dk, w, _ = (int(v) for v in Z["shape"][ci])
    f = lambda k, den: torch.from_numpy(Z[f"{k}{ci}"].astype(np.float64) / den)
    x = f("x", 16.0).requires_grad_(True)
    W = {k: f(k, 32.0).requires_grad_(k in ("wq", "wk", "wv", "wp", "u", "v")) for k in ("wq", "wk", "wv", "wp", "bq", "bk", "bv", "u", "v")}
    pe, lens = torch.from_numpy(Z[f"pe{ci}"]).double(), torch.from_numpy(Z[f"lens{ci}"])
    proj = lambda wn, bn: (x @ W[wn].T + W[bn]).view(B, T, H, dk).transpose(1, 2)
    q, k, v = proj("wq", "bq"), proj("wk", "bk"), proj("wv", "bv")
    p = (pe @ W["wp"].T).view(-1, H, dk).transpose(0, 1)
    ctx = ops.rel_pos_attention(q, k, v, p, W["u"], W["v"], lens, window=w)
    out = ctx.transpose(1, 2).reshape(B, T, H * dk)
    g = torch.from_numpy(G[f"g{ci}"].astype(np.float64) / 8.0)
    (out * g).sum().backward()
    got = dict(dx=x.grad, dwq=W["wq"].grad, dwk=W["wk"].grad, dwv=W["wv"].grad, dwp=W["wp"].grad, du=W["u"].grad, dv=W["v"].grad)
    for name, t in got.items():
        ref = torch.from_numpy(G[f"{name}{ci}"])
        rel = float((t - ref).abs().max()) / float(ref.abs().max())
        print(f"{str(Z['name'][ci])} {name}: max |composition - reference| / max|reference| = {rel:.3e}")
        assert rel <= 1e-10, (name, rel)


def test_new_symbols_exist():
    L = _lib.lib()
    for name in ("ia_relpos_attention_local_lse", "ia_relpos_attention_local_bwd_dims", "ia_relpos_attention_local_bwd_ws_elems",
                 "ia_relpos_attention_local_bwd"):
        assert hasattr(L, name), name
    from indic_cl_asr_amd.ops import fast
    for name in ("attention_local_bwd_dims", "relpos_attention_local_bwd"):
        assert callable(getattr(fast, name))


def test_backward_validates_its_arguments_before_any_launch():
    """Host scratch pointers that are never read (as tests/test_local_attention.py does for the executors): every answer below
    comes before the first launch."""
    L = _lib.lib()
    scratch = ctypes.create_string_buffer(256)
    ptr = ctypes.c_void_p(ctypes.addressof(scratch) // 16 * 16 + 16)
    B, T, H, dk, w = 1, 64, 1, 64, 4

    def call(window=w, pl_rows=2 * w + 1, dk_=dk, dropout=0.0, hole=None):
        a = [ptr] * 8 + [B, T, H, dk_, window, dropout, 0] + [ptr, ptr, pl_rows] + [ptr] * 5 + [None]
        if hole is not None:
            a[hole] = None
        return L.ia_relpos_attention_local_bwd(*a)

    for hole in list(range(8)) + [15, 16, 18, 19, 20, 21, 22]:      # every pointer argument
        assert call(hole=hole) == -1, hole
    assert call(window=0) == -1 and call(window=-2) == -1            # IA_INVALID_VALUE
    assert call(pl_rows=2 * w) == -1                                 # fewer than 2 * window + 1 position rows
    assert call(dk_=68) == -4                                        # IA_UNSUPPORTED
    assert call(dk_=30) == -4
    assert call(dropout=1.0) == -1
    odd = ctypes.c_void_p(ptr.value + 4)                             # misaligned qkv
    assert L.ia_relpos_attention_local_bwd(odd, *([ptr] * 7), B, T, H, dk, w, 0.0, 0, ptr, ptr, 2 * w + 1, *([ptr] * 5), None) == -1
    # the forward with lse: the checks of ia_relpos_attention_local
    assert L.ia_relpos_attention_local_lse(None, None, None, None, None, 1, 64, 1, 64, 4, 0.0, 0, None, None, None) == -1
    assert L.ia_relpos_attention_local_lse(ptr, ptr, ptr, ptr, ptr, 1, 64, 1, 64, 0, 0.0, 0, ptr, ptr, None) == -1
    assert L.ia_relpos_attention_local_lse(ptr, ptr, ptr, ptr, ptr, 1, 64, 1, 68, 4, 0.0, 0, ptr, ptr, None) == -4
    rs, p0 = ctypes.c_int(), ctypes.c_int()
    assert L.ia_relpos_attention_local_bwd_dims(0, 4, ctypes.byref(rs), ctypes.byref(p0)) == -1
    assert L.ia_relpos_attention_local_bwd_dims(64, 0, ctypes.byref(rs), ctypes.byref(p0)) == -1
    assert L.ia_relpos_attention_local_bwd_dims(64, 4, None, ctypes.byref(p0)) == -1
    assert L.ia_relpos_attention_local_bwd_ws_elems(1, 64, 1, 64, 0) == 0


@pytest.mark.parametrize("T", [1, 2, 17, 64, 65, 1000, 3001])
@pytest.mark.parametrize("w", [1, 4, 15, 16, 63, 64, 100, 500, 5000])
def test_dband_row_stride(T, w):
    from indic_cl_asr_amd.ops import fast
    Rs, pad0 = fast.attention_local_bwd_dims(T, w)
    we = min(w, T - 1)
    assert Rs % 8 == 0 and 0 <= pad0 < 8
    assert Rs >= pad0 + 2 * we + 1
    assert Rs < pad0 + 2 * we + 1 + 8                                # ... and no wider than the band needs: no term in T
    assert (we - 15 + pad0) % 8 == 0                                 # every flushed 16-byte chunk is aligned


@pytest.mark.parametrize("B,H,dk,w", [(1, 8, 64, 64), (4, 4, 36, 16), (2, 2, 64, 500)])
def test_workspace_is_linear_in_T(B, H, dk, w):
    """ws(2T) <= 2 ws(T) + c with c independent of T: the layout rounds each of its four parts up to 64 elements (c = 4 * 64)
    and every other term is proportional to T or constant in it."""
    L = _lib.lib()
    ws = lambda T: L.ia_relpos_attention_local_bwd_ws_elems(B, T, H, dk, w)
    c = 4 * 64
    for T in (1000, 2000, 4000):
        a, b = ws(T), ws(2 * T)
        print(f"B={B} H={H} dk={dk} w={w}: ws({T}) = {a}, ws({2 * T}) = {b}")
        assert a > 0 and b <= 2 * a + c
    full = L.ia_relpos_attention_flash_bwd_ws_elems(B, 4000, H, dk)
    assert ws(4000) < full
