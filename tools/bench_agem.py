"""Averaged GEM's cost in the optimizer step, on the flat buffers of BASELINE configs[1]'s trainable set (Conformer-medium,
freeze_layer(m, 12), about 40 M elements): FusedAdamW._apply plain, clipped, projected and projected + clipped, the last two
with an opposing reference (every step projects), and the three reduction passes on their own (ia_grad_norm, ia_agem_dots,
ia_grad_norm_projected) with their achieved bandwidth over the bytes the algorithm needs (4 / 8 / 8 B per element).

HIP events around `n` back-to-back calls after a warm-up; the variants alternate over `--rounds` rounds and the median and the
spread over the rounds are reported.  Developer tool; reads nothing outside the tree; one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, warmup, n):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3       # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_agem.py needs the GPU: a CPU run cannot give a time")
    from indic_cl_asr_amd import _lib, cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config("medium", compute_dtype="bf16")).cuda()
    freeze_layer(m, 12)
    flat = cl.FlatParams(m)
    elems = sum(e[2] for e in flat.entries)                          # what the chunk table covers (the gaps are not read)
    grad = torch.randn(flat.numel, device="cuda") * 1e-2
    ref = torch.randn(flat.numel, device="cuda") * 1e-2 - 0.5 * grad # opposing: g.r ~ -0.5 |g|^2

    def optimizer(project, **kw):
        agem = cl.AveragedGEM(flat) if project else None
        opt = cl.FusedAdamW(flat, lr=1e-4, projection=agem, **kw)
        if project:
            flat.grad.copy_(ref)
            agem.store_reference(opt)
        return opt, agem

    legs = {"plain": optimizer(False), "clipped": optimizer(False, max_grad_norm=1.0), "projected": optimizer(True),
            "projected_clipped": optimizer(True, max_grad_norm=1.0)}
    flat.grad.copy_(grad)

    # the reduction passes on their own, through the C entry points the step calls
    L = _lib.lib()
    nchunks, nseg = flat.chunk_table.shape[0], len(flat.entries)
    opt_c, agem_c = legs["projected_clipped"]
    opt_c._apply(1.0)                                                # allocates the norm buffers, leaves violated = 1
    assert agem_c.stats()["projected"] == 1
    ws = agem_c.workspace(nchunks)
    norm_args = (_lib.ptr(flat.grad), _lib.ptr(flat.chunk_table), nchunks, _lib.ptr(flat.seg_chunk_begin), nseg, 1.0, 1.0)
    norm_out = (_lib.ptr(opt_c._seg_norm), _lib.ptr(opt_c._norm_state), _lib.ptr(opt_c._norm_ws), opt_c._norm_ws.numel())

    def clip_pass():
        _lib.check(L.ia_grad_norm(*norm_args, None, *norm_out, _lib.stream_ptr()), "ia_grad_norm")

    def dots_pass():
        _lib.check(L.ia_agem_dots(_lib.ptr(flat.grad), _lib.ptr(agem_c.ref.flat), _lib.ptr(flat.chunk_table), nchunks, nseg, 1.0,
                                  None, _lib.ptr(agem_c.proj_state), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "ia_agem_dots")

    def proj_norm_pass():
        _lib.check(L.ia_grad_norm_projected(*norm_args, None, *norm_out, _lib.ptr(agem_c.ref.flat), _lib.ptr(agem_c.proj_state),
                                            _lib.stream_ptr()), "ia_grad_norm_projected")

    calls = {k: (lambda o=o: o._apply(1.0)) for k, (o, _) in legs.items()}
    calls.update(clip_pass=clip_pass, dots_pass=dots_pass, projected_norm_pass=proj_norm_pass)
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for k, fn in calls.items():
            times[k].append(timeit(fn, args.warmup, args.n))
    assert all(a.stats()["projected"] == 1 for _, a in legs.values() if a is not None)
    out = {"numel": flat.numel, "elements": elems, "segments": nseg, "chunks": int(nchunks), "rounds": args.rounds, "n": args.n}
    for k, v in times.items():
        out[k + "_us"] = round(statistics.median(v), 2)
        out[k + "_us_minmax"] = [round(min(v), 2), round(max(v), 2)]
    for k, bytes_per_elem in (("clip_pass", 4), ("dots_pass", 8), ("projected_norm_pass", 8)):
        out[k + "_GBps"] = round(elems * bytes_per_elem / (out[k + "_us"] * 1e-6) / 1e9, 1)
    plain, proj = out["plain_us"], out["projected_us"]
    out["projected_minus_plain_over_plain"] = round((proj - plain) / plain, 3)
    out["expected_ratio"] = round(12 / 30, 3)
    out["projected_clipped_minus_clipped_us"] = round(out["projected_clipped_us"] - out["clipped_us"], 2)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
