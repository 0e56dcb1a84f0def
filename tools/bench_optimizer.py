"""FusedAdamW._apply on the flat buffers of BASELINE configs[1]'s trainable set (Conformer-medium, freeze_layer(m, 12)):
plain, with max_grad_norm=1.0 (live-segment detection on / every segment live), and with a Synaptic Intelligence path integral
attached (first task: w only; later tasks: omega and theta* read as well, every segment live), and `grouped`: the plain step
with layerwise_lr_groups + no-decay parameter groups (ia_adamw_step_segmented_grouped), and `masked`: Piggyback on its default
kinds without clipping (ia_adamw_step_segmented_masked: matrices masked, heads free, the rest frozen), and `packed`: PackNet on the
same kinds (ia_adamw_step_segmented_packed with every packed weight free and trained; `prune_us`: one ia_pack_prune at fraction
0.5, each call from a zeroed owner map and the same weights, between its own two events; `packed_retrain_us`: the step after the
pruning, when half of the packed weights move), and `lora`: LoRA on its default kinds at rank 16 without clipping (ia_lora_grad, the
plain step on the free tensors, the AdamW rule on the factor buffer, ia_lora_apply; B is given seeded values so that both factor
gradients are real work).  Per leg: `<leg>_us` device time of one
_apply between two events, `<leg>_host_us` host wall-clock of one step() call with no synchronisation inside the timed loop
(what the training loop's thread pays: Python, ctypes and the launches).  Developer tool; one JSON line.

`--legs plain` uses nothing newer than the segmented AdamW itself, so the same file times an older checkout; every other leg
touches its own method only when it is asked for."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, warmup=5, n=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def host_timeit(fn, warmup=5, n=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / n * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="plain,clip,clip_all_live,si_first_task,si_penalty,grouped,masked,packed,lora")
    args = ap.parse_args()
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config("medium", compute_dtype="bf16")).cuda()
    freeze_layer(m, 12)
    flat = cl.FlatParams(m)
    grad = torch.randn(flat.numel, device="cuda") * 1e-2
    out = {"numel": flat.numel, "segments": len(flat.entries), "chunks": int(flat.chunk_table.shape[0])}
    for leg in args.legs.split(","):
        kw, live = {"plain": ({}, False), "clip": ({"max_grad_norm": 1.0}, False),
                    "clip_all_live": ({"max_grad_norm": 1.0}, True), "si_first_task": ({}, False),
                    "si_penalty": ({}, True), "grouped": ({}, False), "masked": ({}, False), "packed": ({}, False),
                    "lora": ({}, False)}[leg]
        if leg == "grouped":
            kw["param_groups"] = cl.layerwise_lr_groups(flat, 1e-4, 0.9)
        if leg.startswith("si_"):
            kw["path_integral"] = si = cl.SynapticIntelligence(flat)
            if leg == "si_penalty":                  # a consolidated task: the step reads omega and theta* and adds the penalty
                si.omega.flat.uniform_(0.0, 1.0)
                si.tasks_consolidated = 1
        if leg == "masked":
            kw["masks"] = cl.Piggyback(flat)
        if leg == "packed":
            kw["masks"] = pn = cl.PackNet(flat, prune=0.5)
        if leg == "lora":
            kw["masks"] = lora = cl.LoRA(flat, rank=16)
        opt = cl.FusedAdamW(flat, lr=1e-4, **kw)
        flat.grad.copy_(grad)
        if leg == "packed":
            pn.begin_language("bench", opt)
        if leg == "lora":
            lora.begin_language("bench", opt)
            for fac in lora.factor_views().values():                       # B != 0, so gA is not a sum of zeros
                fac["lora_B"].normal_(0.0, 1e-2)
            out["lora_adapted_elements"] = sum(a[2] * a[3] for a in lora.adapted)
            out["lora_factor_elements"] = sum(16 * (a[2] + a[3]) for a in lora.adapted)
            out["lora_tiles"] = int(lora.tile_table.shape[0])
            out["lora_workspace_bytes"] = lora.workspace_bytes
        if leg == "grouped":
            out["groups"] = len(opt.param_groups)
        out[leg + "_us"] = round(timeit(lambda: opt._apply(1.0, live)), 2)
        flat.all_grads_live = live
        out[leg + "_host_us"] = round(host_timeit(opt.step), 2)
        flat.all_grads_live = False
        if leg == "packed":
            theta0, total = flat.theta.clone(), 0.0
            for i in range(8):                       # the first three calls are warm-up
                pn.owner.zero_()
                flat.theta.copy_(theta0)
                pn.phase = "train"
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                pn.prune(opt)
                b.record()
                torch.cuda.synchronize()
                total += a.elapsed_time(b) * 1e3 if i >= 3 else 0.0
            out["prune_us"] = round(total / 5, 2)
            out["packed_elements"] = sum(e[2] for e in pn._packed_entries())
            out["packed_free_after_prune"] = round(pn.free_fraction(), 4)
            out["packed_retrain_us"] = round(timeit(lambda: opt._apply(1.0, live)), 2)
        del opt
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
