"""OGD's cost in the optimizer step, on the flat buffers of BASELINE configs[1]'s trainable set (Conformer-medium,
freeze_layer(m, 12)), for M = 1, 16, 64 and 256 stored directions: ia_ogd_dots on its own (both launches; (M + 1) * 4 B per
element), ia_ogd_project in place ((M + 2) * 4 B per element) and FusedAdamW._apply with the OGD projection (dots, projection, the
plain AdamW launches: 30 B per element more), and, in the same run, ia_gem_dots at K = 16 (the same bytes as M = 16), the plain
step and ia_peak_stream_copy, against which every rate is set.

The rows are random with norm about one: neither kernel knows whether they are orthonormal, and filling them directly spares
M inserts of about 16 M B per element each.  Every tensor is in scope.  HIP events around `n` back-to-back calls after a
warm-up; the legs alternate over `--rounds` rounds and the median and the spread over the rounds are reported.  The two
conditions of the design ("Orthogonal Gradient Descent") are evaluated and printed, not enforced.  Developer tool; reads
nothing outside the tree; one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_agem import timeit  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--directions", type=int, nargs="+", default=[1, 16, 64, 256])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ogd.py needs the GPU: a CPU run cannot give a time")
    from indic_cl_asr_amd import _lib, cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config("medium", compute_dtype="bf16")).cuda()
    freeze_layer(m, 12)
    flat = cl.FlatParams(m)
    elems = sum(e[2] for e in flat.entries)                          # what the chunk table covers (the gaps are not read)
    grad = torch.randn(flat.numel, device="cuda") * 1e-2
    L, ptr, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    nchunks, nseg = flat.chunk_table.shape[0], len(flat.entries)
    top = max(args.directions)
    ogd = cl.OGD(flat, top)
    for k in range(top):                                             # row by row: no temporary of the basis' size
        ogd.basis[k].normal_().mul_(flat.numel ** -0.5)
    opt = cl.FusedAdamW(flat, lr=1e-4, projection=ogd)
    plain = cl.FusedAdamW(flat, lr=1e-4)
    x = grad.clone()
    calls = {"plain_step": lambda: plain._apply(1.0)}

    def set_rows(k):
        ogd._rows = k

    for k in args.directions:
        calls[f"ogd_dots_m{k}"] = lambda k=k: ogd._dots(flat.grad, ogd.basis, k, None, ogd.dots64, ogd.dots32)
        calls[f"ogd_project_m{k}"] = lambda k=k: ogd._project(x, k, ogd.dots32, None, x)
        calls[f"ogd_step_m{k}"] = lambda k=k: (set_rows(k), opt._apply(1.0))
    gem = cl.GEM(flat, max_tasks=16)
    for t in range(16):
        flat.grad.copy_(ogd.basis[t, :flat.numel])
        gem.store_reference(t)
    gws = gem.workspace(nchunks)
    calls["gem_dots_k16"] = lambda: _lib.check(
        L.ia_gem_dots(ptr(flat.grad), ptr(gem.refs), gem.stride, 16, ptr(flat.chunk_table), nchunks, nseg, 1.0, None, -1,
                      ptr(gem.sums), ptr(gws), gws.numel(), s), "ia_gem_dots")
    copy_n = 1 << 30
    src, dst = torch.empty(copy_n, dtype=torch.uint8, device="cuda"), torch.empty(copy_n, dtype=torch.uint8, device="cuda")
    calls["copy"] = lambda: _lib.check(L.ia_peak_stream_copy(ptr(src), ptr(dst), copy_n, s), "ia_peak_stream_copy")
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            flat.grad.copy_(grad)
            x.copy_(grad)
            times[name].append(timeit(fn, args.warmup, args.n))
    assert bool(torch.isfinite(flat.grad).all()) and bool(torch.isfinite(x).all())
    out = {"numel": flat.numel, "elements": elems, "segments": nseg, "chunks": int(nchunks), "rounds": args.rounds, "n": args.n}
    med = {name: statistics.median(v) for name, v in times.items()}
    copy_rate = 2 * copy_n / (med["copy"] * 1e-6)
    out["copy_GBps"] = round(copy_rate / 1e9, 1)
    bytes_per_elem = {"gem_dots_k16": 17 * 4, "plain_step": 30}
    for k in args.directions:
        bytes_per_elem[f"ogd_dots_m{k}"] = (k + 1) * 4
        bytes_per_elem[f"ogd_project_m{k}"] = (k + 2) * 4
        bytes_per_elem[f"ogd_step_m{k}"] = (2 * k + 3) * 4 + 30
    for name, b in bytes_per_elem.items():
        rate = elems * b / (med[name] * 1e-6)
        out[name + "_us"] = round(med[name], 2)
        out[name + "_us_minmax"] = [round(min(times[name]), 2), round(max(times[name]), 2)]
        out[name + "_GBps"] = round(rate / 1e9, 1)
        out[name + "_of_copy"] = round(rate / copy_rate, 3)
    if {16, 64, 256} <= set(args.directions):
        out["dots_m16_over_gem_dots_k16"] = round(med["ogd_dots_m16"] / med["gem_dots_k16"], 4)                # condition: <= 1.05
        per_row_16 = med["ogd_dots_m16"] / 16
        per_row_tail = (med["ogd_dots_m256"] - med["ogd_dots_m64"]) / 192
        out["dots_us_per_row_m16"] = round(per_row_16, 3)
        out["dots_us_per_row_m64_to_m256"] = round(per_row_tail, 3)
        out["dots_per_row_ratio"] = round(per_row_tail / per_row_16, 4)                                         # condition: <= 1.1
        proj_16 = med["ogd_project_m16"] / 16
        out["project_per_row_ratio"] = round((med["ogd_project_m256"] - med["ogd_project_m64"]) / 192 / proj_16, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
