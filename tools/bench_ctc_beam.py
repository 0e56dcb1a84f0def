"""DESIGN.md section 6, "CTC prefix beam search": ia_ctc_beam_search at the benchmark's density (32 utterances, T = 375, V = 257,
row stride 264, W = 4 and 16) with device events, 20 launches after 5 warm-up launches; beside it, in the same process and on
the same batch, decoding.greedy_ctc_decode and the float64 host routine decoding.beam_ctc_decode_host (wall clock, one run
each: both end on the host).  One JSON line."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from indic_cl_asr_amd import _lib, decoding  # noqa: E402

L = _lib.lib()
B, T, V, ld = 32, 375, 257, 264
g = torch.Generator().manual_seed(0)
buf = torch.randn(B * T, ld, generator=g) * 4
buf[:, V - 1] += 4
logits = buf.cuda().view(B, T, ld)[..., :V]
lens = torch.full((B,), T, dtype=torch.long).cuda()
lse = torch.empty(B, T, device="cuda")
_lib.check(L.ia_ctc_row_lse(_lib.ptr(logits), ld, B * T, V, _lib.ptr(lse), _lib.stream_ptr()), "lse")
res = {"shape": [B, T, V], "ld": ld}

for W in (4, 16):
    n = L.ia_ctc_beam_workspace_bytes(B, T, V, W)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    tok = torch.empty(B, W, T, dtype=torch.int32, device="cuda")
    ln = torch.empty(B, W, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, W, device="cuda")

    def search():
        _lib.check(L.ia_ctc_beam_search(_lib.ptr(logits), _lib.ptr(lse), _lib.ptr(lens), B, T, ld, V, V - 1, W, float("-inf"),
                                        _lib.ptr(tok), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(ws), n, _lib.stream_ptr()), "beam")

    for _ in range(5):
        search()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        search()
    b.record()
    b.synchronize()
    res[f"beam_w{W}_us"] = round(a.elapsed_time(b) * 1000.0 / 20, 1)
    res[f"beam_w{W}_workspace_bytes"] = int(n)
    t0 = time.perf_counter()
    dev = decoding.beam_ctc_decode(logits, lens, beam_size=W, lse=lse)
    res[f"beam_w{W}_python_entry_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    host = decoding.beam_ctc_decode_host(logits.cpu(), lens.cpu(), beam_size=W, lse=lse.cpu())
    res[f"host_w{W}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res[f"w{W}_best_equal_to_host"] = sum(d.y_sequence == h.y_sequence for d, h in zip(dev, host))

lp = logits - lse.unsqueeze(-1)
for _ in range(5):
    decoding.greedy_ctc_decode(lp, lens)
torch.cuda.synchronize()
t0 = time.perf_counter()
for _ in range(20):
    decoding.greedy_ctc_decode(lp, lens)
res["greedy_ms"] = round((time.perf_counter() - t0) * 1e3 / 20, 3)
print(json.dumps(res))
