"""DESIGN.md, "Transducer beam search": ia_rnnt_beam_alsd_bf16w at the benchmark's density (32 utterances, T = 375, Hp = Hj = 640,
V = 257, bf16 weights, W = 4, 8 and 16, alsd_max_target_len = 1.0) with device events, 20 launches after 5 warm-up launches;
beside it, on the same operands, the greedy kernel (ia_greedy_rnnt_decode_bf16w_ex, same timing) and the float64 host routine
decoding.beam_rnnt_alsd_host by wall clock (W = 4, the first `--host-utterances` utterances only: it is the slow path).  One
JSON line."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from indic_cl_asr_amd import _lib, decoding  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--host-utterances", type=int, default=1)
ap.add_argument("--frames", type=int, default=375)
args = ap.parse_args()

L = _lib.lib()
B, T, Hp, Hj, V = 32, args.frames, 640, 640, 257
g = torch.Generator().manual_seed(0)
case = dict(f_all=torch.randn(B, T, Hj, generator=g), EW=torch.randn(V + 1, 4 * Hp, generator=g) * 0.5,
            Whh=(torch.randn(4 * Hp, Hp, generator=g) / Hp ** 0.5).bfloat16(), Wp=(torch.randn(Hj, Hp, generator=g) / Hp ** 0.5).bfloat16(),
            bp=torch.randn(Hj, generator=g) * 0.1, Wh=(torch.randn(V, Hj, generator=g) / Hj ** 0.5).bfloat16(),
            bh=torch.randn(V, generator=g) * 0.1, lens=torch.full((B,), T, dtype=torch.long))
case["bh"][-1] += 4.0
dev = {k: v.cuda().contiguous() for k, v in case.items()}
res = {"shape": [B, T, Hp, Hj, V]}


def timed(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / 20


for W in (4, 8, 16):
    ms = timed(lambda: decoding.beam_rnnt_alsd_device(dev, W, 1.0, True))
    out = decoding.alsd_unpack(decoding.beam_rnnt_alsd_device(dev, W, 1.0, True))
    res[f"alsd_w{W}_ms"] = round(ms, 2)
    res[f"alsd_w{W}_us_per_step_bound"] = round(ms * 1000.0 / (2 * T), 1)          # at most len + u_max = 2 T steps
    res[f"alsd_w{W}_workspace_bytes"] = int(L.ia_rnnt_beam_workspace_bytes(B, T, Hp, Hj, V, W, T))
    res[f"alsd_w{W}_mean_tokens"] = round(sum(len(r["hyps"][0][0]) for r in out) / B, 1)
    res[f"alsd_w{W}_finished_utterances"] = sum(r["n_finished"] > 0 for r in out)
    if W == 4 and args.host_utterances > 0:
        n = min(B, args.host_utterances)
        sub = {k: (v[:n] if k in ("f_all", "lens") else v) for k, v in case.items()}
        t0 = time.perf_counter()
        host = decoding.beam_rnnt_alsd_host(sub, W)
        res["host_w4_s_per_utterance"] = round((time.perf_counter() - t0) / n, 2)
        res["host_w4_best_equal_to_device"] = sum(h["hyps"][0][0] == d["hyps"][0][0] for h, d in zip(host, out))

cap = T * 10
tokens = torch.empty(B, cap, dtype=torch.int32, device="cuda")
counts = torch.zeros(B, dtype=torch.int32, device="cuda")
ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
nw = int(L.ia_greedy_decode_cluster(B, Hp, Hj))
scratch = torch.empty(max(1, int(L.ia_greedy_decode_scratch_bytes(B, Hp, Hj))), dtype=torch.uint8, device="cuda")


def greedy():
    _lib.check(L.ia_greedy_rnnt_decode_bf16w_ex(_lib.ptr(dev["f_all"]), _lib.ptr(dev["lens"]), _lib.ptr(dev["EW"]), _lib.ptr(dev["Whh"]),
                                                _lib.ptr(dev["Wp"]), _lib.ptr(dev["bp"]), _lib.ptr(dev["Wh"]), _lib.ptr(dev["bh"]), B, T, Hp,
                                                Hj, V, V - 1, V - 1, V, 10, _lib.ptr(tokens), cap, _lib.ptr(counts), _lib.ptr(ovf), nw,
                                                _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr()), "greedy")


res["greedy_ms"] = round(timed(greedy), 2)
res["greedy_mean_tokens"] = round(float(counts.float().mean()), 1)
print(json.dumps(res))
