"""ia_adamw_step_segmented_rwalk against ia_adamw_step_segmented_si, and ia_rwalk_consolidate against ia_si_consolidate, on the
flat buffers of BASELINE configs[1]'s trainable set (Conformer-medium, freeze_layer(m, 12)).  The C entries are called directly
(the three launches of a step: liveness, walker, advance), between two device events, `--calls` calls per window; the legs
alternate inside every one of `--rounds` rounds, so that drift of the machine reaches all of them alike.  Per leg: the median
time of one call over the rounds, the spread (max - min over the rounds, relative to the median), and the achieved bytes/s from
the bytes the algorithm needs per element (plain 30, SI 38, EWC++ 38, RWalk 46, with a fold 62, the penalty + 8; the
liveness pass of a step that is not all-live reads the gradient once more, in the SI leg as in the others, and is not counted).
Developer tool; one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls * 1e3          # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=10)
    args = ap.parse_args()
    from indic_cl_asr_amd import _lib, cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config("medium", compute_dtype="bf16")).cuda()
    freeze_layer(m, 12)
    flat = cl.FlatParams(m)
    opt = cl.FusedAdamW(flat, lr=1e-4)
    L, p, stream = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    flat.grad.copy_(torch.randn(flat.numel, device="cuda") * 1e-2)
    elements = sum(e[2] for e in flat.entries)
    nchunks, nseg = flat.chunk_table.shape[0], len(flat.entries)
    buf = {k: torch.zeros_like(flat.theta) for k in ("fisher", "w", "anchor", "score", "acc", "omega")}
    buf["omega"].uniform_(0.0, 1.0)
    star = flat.theta.clone()
    one_lr, one_wd = (ctypes.c_float * 1)(1e-4), (ctypes.c_float * 1)(1e-2)

    def head(all_live):
        return (p(flat.theta), p(flat.grad), p(opt.exp_avg), p(opt.exp_avg_sq), p(flat.chunk_table), nchunks, p(opt.seg_active),
                p(opt.seg_step), nseg, int(all_live))

    def si(pen):
        return lambda: _lib.check(L.ia_adamw_step_segmented_si(
            *head(pen), 1e-4, 0.9, 0.999, 1e-8, 1e-2, 1.0, p(opt.shadow), None, 0, None, p(buf["w"]),
            p(buf["omega"]) if pen else None, p(star) if pen else None, 1.0, stream), "ia_adamw_step_segmented_si")

    def rwalk(scores, fold, pen):
        s = (lambda k: p(buf[k])) if scores else (lambda k: None)
        return lambda: _lib.check(L.ia_adamw_step_segmented_rwalk(
            *head(pen), 0.9, 0.999, 1e-8, 1.0, p(opt.shadow), None, 1, one_lr, one_wd, None, 0, None, p(buf["fisher"]), s("w"),
            s("anchor"), s("score"), p(buf["omega"]) if pen else None, p(star) if pen else None, 1.0, 0.9, 1e-3, int(fold), stream),
            "ia_adamw_step_segmented_rwalk")

    ws = torch.empty(L.ia_rwalk_workspace_bytes(nchunks), dtype=torch.uint8, device="cuda")
    maxima = torch.zeros(2, device="cuda")

    def rw_consolidate(scores):
        s = (lambda k: p(buf[k])) if scores else (lambda k: None)
        return lambda: _lib.check(L.ia_rwalk_consolidate(
            p(flat.theta), p(star), p(buf["fisher"]), s("w"), s("anchor"), s("score"), s("acc"), p(buf["omega"]), p(maxima), 1e-3, 1,
            0, flat.numel, p(flat.chunk_table), nchunks, p(ws), ws.numel(), stream), "ia_rwalk_consolidate")

    def si_consolidate():
        _lib.check(L.ia_si_consolidate(p(flat.theta), p(star), p(buf["w"]), p(buf["omega"]), 1e-3, flat.numel, stream),
                   "ia_si_consolidate")

    # leg -> (call, bytes per element, elements the bytes are counted over)
    legs = {"si": (si(False), 38, elements), "si_penalty": (si(True), 46, elements),
            "rwalk": (rwalk(True, False, False), 46, elements), "rwalk_fold": (rwalk(True, True, False), 62, elements),
            "rwalk_penalty": (rwalk(True, False, True), 54, elements), "ewcpp": (rwalk(False, False, False), 38, elements),
            "si_consolidate": (si_consolidate, 28, flat.numel),
            "rwalk_consolidate": (rw_consolidate(True), 64, flat.numel), "ewcpp_consolidate": (rw_consolidate(False), 20, flat.numel)}
    for fn, _, _ in legs.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(args.rounds):
        for k, (fn, _, _) in legs.items():
            times[k].append(window(fn, args.calls))
    out = {"numel": flat.numel, "elements": elements, "chunks": int(nchunks), "calls": args.calls, "rounds": args.rounds}
    for k, (_, nbytes, n) in legs.items():
        med = statistics.median(times[k])
        out[k] = {"us": round(med, 2), "spread": round((max(times[k]) - min(times[k])) / med, 4), "bytes_per_element": nbytes,
                  "TB_per_s": round(nbytes * n / med * 1e-6, 3)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
