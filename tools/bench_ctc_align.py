"""DESIGN.md section 6, "CTC forced alignment": ia_ctc_align against ia_ctc_forward_logits (the loss's alpha/beta launch)
at (B,T,V,S) = (32,376,257,105): same process, device events, alternating windows, after warm-up.  One JSON line."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from indic_cl_asr_amd import _lib  # noqa: E402

L = _lib.lib()
B, T, V, S, ld = 32, 376, 257, 105, 264
g = torch.Generator().manual_seed(0)
logits = (torch.randn(B * T, ld, generator=g) * 3).cuda()
tg = torch.randint(0, V - 1, (B, S), generator=g).cuda()
il = torch.full((B,), T, dtype=torch.long).cuda()
tl = torch.full((B,), S, dtype=torch.long).cuda()
lse = torch.empty(B * T, device="cuda")
_lib.check(L.ia_ctc_row_lse(_lib.ptr(logits), ld, B * T, V, _lib.ptr(lse), _lib.stream_ptr()), "lse")
n_loss = L.ia_ctc_workspace_bytes(B, T, S)
n_al = L.ia_ctc_align_workspace_bytes(B, T, S)
ws_loss = torch.empty(n_loss, dtype=torch.uint8, device="cuda")
ws_al = torch.empty(n_al, dtype=torch.uint8, device="cuda")
nll = torch.empty(B, device="cuda")
path = torch.empty(B, T, dtype=torch.int32, device="cuda")
spans = torch.empty(B, S, 2, dtype=torch.int32, device="cuda")
score = torch.empty(B, device="cuda")


def loss():
    _lib.check(L.ia_ctc_forward_logits(_lib.ptr(logits), ld, _lib.ptr(lse), _lib.ptr(tg), _lib.ptr(il), _lib.ptr(tl), B, T, V, S, V - 1, 1,
                                       _lib.ptr(nll), _lib.ptr(ws_loss), n_loss, _lib.stream_ptr()), "loss")


def align():
    _lib.check(L.ia_ctc_align(_lib.ptr(logits), ld, _lib.ptr(lse), _lib.ptr(tg), _lib.ptr(il), _lib.ptr(tl), B, T, V, S, V - 1,
                              _lib.ptr(path), _lib.ptr(spans), _lib.ptr(score), _lib.ptr(ws_al), n_al, _lib.stream_ptr()), "align")


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / reps   # us per call


for _ in range(50):
    loss(); align()
torch.cuda.synchronize()
res = {"loss_us": [], "align_us": []}
for _ in range(7):
    res["loss_us"].append(round(timed(loss, 2000), 2))
    res["align_us"].append(round(timed(align, 2000), 2))
res["shape"] = [B, T, V, S]
res["score_vs_nll"] = [float(score[0]), float(-nll[0])]
res["loss_us_median"] = sorted(res["loss_us"])[3]
res["align_us_median"] = sorted(res["align_us"])[3]
print(json.dumps(res))
