"""The one-pass merge kernels of csrc/merge.hip at the flat size of the `medium` preset with every tensor trainable, K task
vectors of randn * 0.01: ia_merge_linear and ia_merge_ties (density 1: cutoffs of zero, the pass alone) as the yardsticks,
ia_merge_fisher (importances randn^2 * 1e-3, floor 1e-6), ia_merge_linear_dare and ia_merge_ties_dare (density 0.5, rescaled).

Algorithmic bytes per element inside a tensor, with the bf16 shadow written: 4K + 10 for the linear and the TIES pass, plain or
DARE (K rows and base read, theta and its image written); 8K + 10 for Fisher (the importances are a second set of rows).

HIP events around `n` back-to-back launches after a warm-up; the legs alternate over `--rounds` rounds, the median and the spread
over the rounds are reported, and each rate is set against ia_peak_stream_copy measured in the same process.  Developer tool;
reads nothing outside the tree; one JSON line."""
import argparse
import ctypes
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
    ap.add_argument("--n", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tasks", type=int, default=5)
    ap.add_argument("--preset", default="medium")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_merge.py needs the GPU: a CPU run cannot give a time")
    from indic_cl_asr_amd import _lib, cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config(args.preset, compute_dtype="bf16")).cuda()
    flat = cl.FlatParams(m)
    K, n = args.tasks, flat.numel
    elems = sum(e[2] for e in flat.entries)                          # what the chunk table covers (the gaps are not read)
    L, ptr, s = _lib.lib(), _lib.ptr, _lib.stream_ptr()
    nchunks, nseg = flat.chunk_table.shape[0], len(flat.entries)
    base = flat.theta.clone()
    theta = torch.empty_like(base)
    shadow = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    rows = torch.randn(K, n, device="cuda") * 0.01
    imps = torch.randn(K, n, device="cuda") ** 2 * 1e-3
    coef = (ctypes.c_float * K)(*([1.0] * K))
    cutoffs = torch.zeros(K, nseg, dtype=torch.int32, device="cuda")
    scopes = torch.arange(nseg, dtype=torch.int32, device="cuda")
    counts = torch.zeros(nseg, 3, dtype=torch.int32, device="cuda")
    threshold, keep_prob = cl.density_to_keep(0.5)
    common = (ptr(theta), ptr(base), ptr(rows))
    table = (ptr(flat.chunk_table), nchunks)
    calls = {
        "linear": lambda: L.ia_merge_linear(*common, n, K, coef, 1.0, *table, ptr(shadow), s),
        "ties": lambda: L.ia_merge_ties(*common, n, K, ptr(cutoffs), ptr(scopes), nseg, 1.0, *table, nseg, ptr(shadow), ptr(counts), s),
        "fisher": lambda: L.ia_merge_fisher(*common, ptr(imps), n, K, coef, 1e-6, 1.0, *table, nseg, ptr(shadow), ptr(counts), s),
        "linear_dare": lambda: L.ia_merge_linear_dare(*common, n, K, coef, 1.0, *table, ptr(shadow), 0, threshold, keep_prob, s),
        "ties_dare": lambda: L.ia_merge_ties_dare(*common, n, K, 1.0, *table, nseg, ptr(shadow), ptr(counts), 0, threshold,
                                                  keep_prob, s),
    }
    for name, fn in calls.items():
        _lib.check(fn(), "ia_merge_" + name)
    copy_n = 1 << 30
    src, dst = torch.empty(copy_n, dtype=torch.uint8, device="cuda"), torch.empty(copy_n, dtype=torch.uint8, device="cuda")
    calls["copy"] = lambda: L.ia_peak_stream_copy(ptr(src), ptr(dst), copy_n, s)
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(timeit(fn, args.warmup, args.n))
    out = {"preset": args.preset, "tasks": K, "numel": n, "elements": elems, "segments": nseg, "chunks": int(nchunks),
           "rounds": args.rounds, "n": args.n}
    copy_rate = 2 * copy_n / (statistics.median(times["copy"]) * 1e-6)
    out["copy_GBps"] = round(copy_rate / 1e9, 1)
    bytes_per_elem = {"linear": 4 * K + 10, "ties": 4 * K + 10, "fisher": 8 * K + 10, "linear_dare": 4 * K + 10,
                      "ties_dare": 4 * K + 10}
    for name, b in bytes_per_elem.items():
        us = statistics.median(times[name])
        rate = elems * b / (us * 1e-6)
        out[name + "_us"] = round(us, 2)
        out[name + "_us_minmax"] = [round(min(times[name]), 2), round(max(times[name]), 2)]
        out[name + "_GB"] = round(elems * b / 1e9, 3)
        out[name + "_GBps"] = round(rate / 1e9, 1)
        out[name + "_of_copy"] = round(rate / copy_rate, 3)
        out[name + "_ps_per_byte"] = round(us * 1e6 / (elems * b), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
