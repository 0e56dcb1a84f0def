"""Key-tiled attention under its three spans at one shape: forward and backward time of full attention, local attention [w, w] and
limited contexts (regular / chunked_limited [L, R]), the C entry points called directly on preallocated buffers so that the window
times launches, not allocations.  The spans are timed round-robin, --reps times, and each line gives the median and the
min .. max of the repetitions' means: the spread to hold a difference against.

    python tools/bench_attn_context.py --shape 8 3001 8 64 --span full local:64 regular:64:64 chunked:70:13

--lib PATH times another build of the library (one that predates the context entry points can still time `full` and `local:w`),
which is how two commits are compared: one process per library, alternated by the caller.  Developer tool."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VP, I, F, U = C.c_void_p, C.c_int, C.c_float, C.c_uint


def _load(path):
    L = C.CDLL(path)
    ops, outs = [VP] * 5, [VP, VP, I, VP, VP, VP, VP, VP, VP]
    for kind, extra in (("flash", []), ("local", [I]), ("context", [I, I, I])):
        if not hasattr(L, f"ia_relpos_attention_{kind}_lse"):
            continue
        f = getattr(L, f"ia_relpos_attention_{kind}_lse"); f.restype = I
        f.argtypes = ops + [I, I, I, I] + extra + [F, U, VP, VP, VP]
        f = getattr(L, f"ia_relpos_attention_{kind}_bwd"); f.restype = I
        f.argtypes = ops + [VP, VP, VP, I, I, I, I] + extra + [F, U] + outs
        f = getattr(L, f"ia_relpos_attention_{kind}_bwd_dims"); f.restype = I
        f.argtypes = [I] + extra + [C.POINTER(I), C.POINTER(I)]
        f = getattr(L, f"ia_relpos_attention_{kind}_bwd_ws_elems"); f.restype = C.c_int64
        f.argtypes = [I, I, I, I] + extra
    return L


def _span(text):
    """'full' | 'local:W' | 'regular:L:R' | 'chunked:L:R' -> (entry-point infix, extra C arguments)"""
    parts = text.split(":")
    if parts[0] == "full":
        return "flash", ()
    if parts[0] == "local":
        return "local", (int(parts[1]),)
    return "context", ({"regular": 0, "chunked": 1}[parts[0]], int(parts[1]), int(parts[2]))


def _time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=os.path.join(ROOT, "indic_cl_asr_amd", "libindicasr_hip.so"))
    ap.add_argument("--shape", type=int, nargs=4, metavar=("B", "T", "H", "DK"), default=(8, 751, 8, 64))
    ap.add_argument("--span", nargs="+", default=["full", "local:64", "regular:64:64"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tag", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attn_context: needs the GPU (no timing without one)")
    L = _load(args.lib)
    B, T, H, dk = args.shape
    d = H * dk
    g = torch.Generator().manual_seed(0)
    bf = dict(dtype=torch.bfloat16, device="cuda")
    qkv = (torch.randn(B * T, 3 * d, generator=g) * 0.8).bfloat16().cuda()
    pl = (torch.randn(2 * T - 1, d, generator=g) * 0.8).bfloat16().cuda()
    bu, bv = (torch.randn(H, dk, generator=g) * 0.3).cuda(), (torch.randn(H, dk, generator=g) * 0.3).cuda()
    dctx = (torch.randn(B * T, d, generator=g) * 0.5).bfloat16().cuda()
    lens = torch.full((B,), T, dtype=torch.int64).cuda()
    P = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    runs = {}
    for text in args.span:
        kind, extra = _span(text)
        if not hasattr(L, f"ia_relpos_attention_{kind}_lse"):
            sys.exit(f"{args.lib} has no ia_relpos_attention_{kind}_lse")
        table = pl
        if kind == "local":
            w = min(extra[0], T - 1)
            table, extra = pl[T - 1 - w:T + w].contiguous(), (w,)
        rs, p0 = I(), I()
        assert getattr(L, f"ia_relpos_attention_{kind}_bwd_dims")(T, *extra, C.byref(rs), C.byref(p0)) == 0, text
        ctx, lse = torch.empty(B * T, d, **bf), torch.empty(B * H, T, device="cuda")
        dqkv, dpl = torch.empty(B * T, 3 * d, **bf), torch.empty_like(table)
        dBand, QvHM = torch.empty(H * B * T * rs.value, **bf), torch.empty(H * B * T * 64, **bf)
        ws = torch.empty(getattr(L, f"ia_relpos_attention_{kind}_bwd_ws_elems")(B, T, H, dk, *extra), device="cuda")
        dub = torch.empty(2, H, dk, device="cuda")

        def fwd(kind=kind, extra=extra, table=table, ctx=ctx, lse=lse):
            rc = getattr(L, f"ia_relpos_attention_{kind}_lse")(P(qkv), P(table), P(bu), P(bv), P(lens), B, T, H, dk, *extra, 0.0, 0, P(ctx),
                                                               P(lse), st)
            assert rc == 0, (kind, rc)

        def bwd(kind=kind, extra=extra, table=table, ctx=ctx, lse=lse, dqkv=dqkv, dpl=dpl, dBand=dBand, QvHM=QvHM, ws=ws, dub=dub):
            rc = getattr(L, f"ia_relpos_attention_{kind}_bwd")(P(qkv), P(table), P(bu), P(bv), P(lens), P(ctx), P(dctx), P(lse), B, T, H, dk,
                                                               *extra, 0.0, 0, P(dqkv), P(dpl), table.shape[0], P(dub[0]), P(dub[1]),
                                                               P(dBand), P(QvHM), P(ws), st)
            assert rc == 0, (kind, rc)

        runs[text] = (fwd, bwd)
        for _ in range(3):   # warm-up: code objects, LDS limits, the GEMM's choices
            fwd(); bwd()
    torch.cuda.synchronize()
    times = {text: ([], []) for text in runs}
    for _ in range(args.reps):
        for text, (fwd, bwd) in runs.items():
            times[text][0].append(_time(fwd, args.iters))
            times[text][1].append(_time(bwd, max(5, args.iters // 2)))
    for text, (tf, tb) in times.items():
        row = dict(tag=args.tag, shape=[B, T, H, dk], span=text,
                   fwd_us=dict(median=round(statistics.median(tf), 1), min=round(min(tf), 1), max=round(max(tf), 1)),
                   bwd_us=dict(median=round(statistics.median(tb), 1), min=round(min(tb), 1), max=round(max(tb), 1)))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
