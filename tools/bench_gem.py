"""GEM's cost in the optimizer step, on the flat buffers of BASELINE configs[1]'s trainable set (Conformer-medium,
freeze_layer(m, 12)), for K = 1, 4 and 11 stored references: ia_gem_dots on its own (with its finishing launch; (K + 1) * 4 B per
element), FusedAdamW._apply with the GEM projection (dots, program, projected AdamW; every reference opposes the gradient and
memory_strength = 0.5 keeps every v_k > 0, so the step reads all K rows: (7 + K) * 4 + 2 B per element), and, as the comparison,
the A-GEM step and the plain step as they were before GEM existed.

HIP events around `n` back-to-back calls after a warm-up; the legs alternate over `--rounds` rounds and the median and the
spread over the rounds are reported, with the fraction of the HBM copy peak (6.29 TB/s measured for a float4 copy on this part)
each byte count then amounts to.  Developer tool; reads nothing outside the tree; one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench_agem import timeit  # noqa: E402

COPY_PEAK = 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--tasks", type=int, nargs="+", default=[1, 4, 11])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_gem.py needs the GPU: a CPU run cannot give a time")
    from indic_cl_asr_amd import _lib, cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config("medium", compute_dtype="bf16")).cuda()
    freeze_layer(m, 12)
    flat = cl.FlatParams(m)
    elems = sum(e[2] for e in flat.entries)                          # what the chunk table covers (the gaps are not read)
    grad = torch.randn(flat.numel, device="cuda") * 1e-2
    L = _lib.lib()
    nchunks, nseg = flat.chunk_table.shape[0], len(flat.entries)

    def opposing():
        return torch.randn(flat.numel, device="cuda") * 1e-2 - 0.5 * grad

    plain = cl.FusedAdamW(flat, lr=1e-4)
    agem = cl.AveragedGEM(flat)
    agem_opt = cl.FusedAdamW(flat, lr=1e-4, projection=agem)
    flat.grad.copy_(opposing())
    agem.store_reference(agem_opt)
    calls = {"plain": lambda: plain._apply(1.0), "agem": lambda: agem_opt._apply(1.0)}
    gems = {}
    for k in args.tasks:
        gem = cl.GEM(flat, max_tasks=k)
        opt = cl.FusedAdamW(flat, lr=1e-4, projection=gem)
        for t in range(k):
            flat.grad.copy_(opposing())
            gem.store_reference(t, opt)
        ws = gem.workspace(nchunks)
        gems[k] = gem

        def dots(gem=gem, ws=ws, k=k):
            _lib.check(L.ia_gem_dots(_lib.ptr(flat.grad), _lib.ptr(gem.refs), gem.stride, k, _lib.ptr(flat.chunk_table), nchunks,
                                     nseg, 1.0, None, -1, _lib.ptr(gem.sums), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()),
                       "ia_gem_dots")

        calls[f"gem_dots_k{k}"] = dots
        calls[f"gem_step_k{k}"] = lambda opt=opt: opt._apply(1.0)
    flat.grad.copy_(grad)

    def agem_dots():
        ws = agem.workspace(nchunks)
        _lib.check(L.ia_agem_dots(_lib.ptr(flat.grad), _lib.ptr(agem.ref.flat), _lib.ptr(flat.chunk_table), nchunks, nseg, 1.0, None,
                                  _lib.ptr(agem.proj_state), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()), "ia_agem_dots")

    calls["agem_dots"] = agem_dots
    times = {k: [] for k in calls}
    for _ in range(args.rounds):
        for name, fn in calls.items():
            times[name].append(timeit(fn, args.warmup, args.n))
    assert agem.stats()["projected"] == 1
    out = {"numel": flat.numel, "elements": elems, "segments": nseg, "chunks": int(nchunks), "rounds": args.rounds, "n": args.n}
    for k, gem in gems.items():
        st = gem.stats()
        assert st["projected"] == 1 and st["unsolved_steps"] == 0 and all(v > 0 for v in st["v"]), st
        out[f"qp_iterations_k{k}"] = st["qp_iterations"]
    for name, v in times.items():
        out[name + "_us"] = round(statistics.median(v), 2)
        out[name + "_us_minmax"] = [round(min(v), 2), round(max(v), 2)]
    bytes_per_elem = {"agem_dots": 8}
    for k in args.tasks:
        bytes_per_elem[f"gem_dots_k{k}"] = (k + 1) * 4
        bytes_per_elem[f"gem_step_k{k}"] = (k + 1) * 4 + (7 + k) * 4 + 2      # the dots pass and the AdamW launch of one step
    for name, b in bytes_per_elem.items():
        rate = elems * b / (out[name + "_us"] * 1e-6)
        out[name + "_GBps"] = round(rate / 1e9, 1)
        out[name + "_of_copy_peak"] = round(rate / COPY_PEAK, 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
