"""DESIGN.md, "CTC forced alignment of long transcripts": ia_ctc_align_long against the host routine align.ctc_forced_align_host
at the sizes of long recordings: B = 1, the head's V = 257 logits in [T, 264] rows + ia_ctc_row_lse, (T, S) = (7500, 2000),
(22500, 6000) and (45000, min(12000, limit)) -- 5, 15 and 30 minutes of audio at 25 frames and 4 tokens per second.

The kernel: device events, 5 launches after 2 warm-up launches (workspace allocated outside the timing).  The host routine: wall
clock of one call on the DEVICE tensors, so its device-to-host copy of the logits is included, as when it is the fall-back.
`--host-align-py FILE` times the ctc_forced_align_host of another revision's align.py (the parent commit's, say) instead of this
tree's.  One JSON line per shape."""
import argparse
import importlib.util
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from indic_cl_asr_amd import _lib, align  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--host-align-py", default=None)
ap.add_argument("--skip-host", action="store_true")
args = ap.parse_args()

host_mod = align
if args.host_align_py:
    spec = importlib.util.spec_from_file_location("indic_cl_asr_amd._bench_host_align", args.host_align_py)
    host_mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(host_mod)

L = _lib.lib()
limit = align.max_targets_long()
V, LD = 257, 264
for T, S in ((7500, 2000), (22500, 6000), (45000, min(12000, limit))):
    g = torch.Generator().manual_seed(T)
    x = (torch.randn(T, LD, generator=g) * 3).cuda().view(1, T, LD)[..., :V]
    lse = align.row_lse(x)
    tg = torch.randint(0, V - 1, (1, S), generator=g).cuda()
    il, tl = torch.tensor([T]).cuda(), torch.tensor([S]).cuda()
    n = int(L.ia_ctc_align_long_workspace_bytes(1, T, S))
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    packed = torch.empty(T + 2 * S + 1, dtype=torch.int32, device="cuda")
    path, spans, score = align._carve(packed, 1, T, S)

    def launch():
        _lib.check(L.ia_ctc_align_long(_lib.ptr(x), LD, _lib.ptr(lse), _lib.ptr(tg), _lib.ptr(il), _lib.ptr(tl), 1, T, V, S, V - 1,
                                       _lib.ptr(path), _lib.ptr(spans), _lib.ptr(score), _lib.ptr(ws), n, _lib.stream_ptr()),
                   "ia_ctc_align_long")

    for _ in range(2):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        launch()
    b.record()
    b.synchronize()
    res = {"T": T, "S": S, "kernel_ms": round(a.elapsed_time(b) / 5, 3), "kernel_us_per_frame": round(a.elapsed_time(b) / 5 * 1000 / T, 3),
           "workspace_bytes": n, "score": float(score[0])}
    if not args.skip_host:
        t0 = time.perf_counter()
        h_path, h_spans, h_score = host_mod.ctc_forced_align_host(x, il, tg, tl, V - 1, lse=lse)
        res["host_s"] = round(time.perf_counter() - t0, 2)
        res["host_over_kernel"] = round(res["host_s"] * 1000 / res["kernel_ms"], 1)
        res["equal"] = bool(torch.equal(h_path, path.cpu()) and torch.equal(h_spans, spans.cpu()) and torch.equal(h_score, score.cpu()))
        del h_path, h_spans, h_score
    print(json.dumps(res), flush=True)
