"""Bit-identity anchor of the segmented optimizer step: SHA-256 digests of every buffer a step writes, recorded in
tests/golden/optimizer_step_digests.json and compared after each step.

Every variant of the step (plain, clipped, skipped, SI, A-GEM, GEM, Piggyback, parameter groups) runs ONE chunk walker and ONE
update rule (csrc/cl_flat.hip), so the tests that compare a variant with "the plain step on the same gradient" compare the shared
arithmetic with itself.  This file pins that arithmetic to recorded values instead: a change of one rounding anywhere in the walker,
the rule, the norms, the dots or the counters changes a digest.

Toy(big=False) and the three seeded gradients of tests/test_optimizer_clip_gpu.py: sizes 1, 3, 4, 63, 64, 65, 4095, 4096, 4097,
2 * 4096 + 5, a 65 x 63 matrix and an idle tensor -- the smallest shapes that reach the sub-float4 tail, the alignment gaps, the
chunk boundary, the 2-D shadow view and the dead-tensor path; three steps per case.  Two more cases take one step on
Toy(big=True) (2049 chunks plus one element: a workgroup crosses tensors) under the A-GEM and the GEM step.

The digests of the inputs (initial weights, gradients, references, scores) are recorded too and checked first: when they differ,
torch's generators or the toy changed, not the kernels, and the failure says so.  A missing file or key fails; nothing skips.

The single-group C entry points (ia_adamw_step_segmented_clipped, _si, _projected: scalar lr / weight_decay, no seg_group) are
exported but FusedAdamW goes through ia_adamw_step_segmented_grouped; test_single_group_entry_points steps through them directly
and holds them to the digests recorded for the same cases.

The toy is imported from the sibling module as the other optimizer tests do (tests/ on sys.path: pytest's default rootdir
insertion, or running this file as a script).

`python tests/test_optimizer_digests_gpu.py` prints the JSON to record (IA_LIB_PATH selects the library that computes it)."""
import functools
import hashlib
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:       # when run as a script
    sys.path.insert(0, ROOT)

from test_optimizer_clip_gpu import Toy, make_grad  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "optimizer_step_digests.json")
MASKED, FROZEN = ["mat", "v1", "v5", "v7", "v9"], ["v0", "v4"]
GROUP1 = dict(params=["v5", "v6", "v7", "v8", "v9", "idle"], lr=1e-4, weight_decay=0.0)
GEM_KW = dict(max_tasks=3, memory_strength=0.1, eps=1e-3)


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def inputs(big):
    """CPU tensors, seeded and never modified: the initial weights, the gradients (three, or one for the big toy), the noise the
    A-GEM and GEM references are made of, and Piggyback scores within 2e-3 of the threshold so that bits go both ways."""
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big))
    e, n = list(flat.entries), flat.numel
    x = {"theta": flat.theta.detach().clone(), "g0": make_grad(e, n, 101)}
    if not big:
        x["g1"], x["g2"] = make_grad(e, n, 102, scale=1e-5), make_grad(e, n, 103)
        u = torch.rand(n, generator=torch.Generator().manual_seed(7)) * 2.0 - 1.0
        x["scores"] = torch.tensor(5e-3, dtype=torch.float32) + u * 2e-3
    x["noise_agem"] = make_grad(e, n, 104)
    for k in range(2 if big else 3):
        x[f"noise_gem{k}"] = make_grad(e, n, 200 + k)
    return x


def input_digests(big):
    return {k: sha(v) for k, v in inputs(big).items()}


def grads_of(big):
    x = inputs(big)
    return [x["g0"]] if big else [x["g0"], x["g1"], x["g2"]]


def optimizer(big, **kw):
    """(flat, optimizer, {name: constructor of an attached method}) on a fresh copy of the toy."""
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    method = {k: kw.pop(k)(flat) for k in ("path_integral", "projection", "masks") if k in kw}
    return flat, cl.FusedAdamW(flat, lr=1e-3, **method, **kw), method


def snapshot(opt, extra):
    """Digest of everything a step writes: the common buffers and the variant's own."""
    bufs = {"theta": opt.flat.theta, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "seg_step": opt.seg_step,
            "shadow": opt.shadow, "norm_state": opt._norm_state, "seg_norm": opt._seg_norm, "counters": opt._counters}
    bufs.update(extra)
    torch.cuda.synchronize()
    return {k: ("none" if v is None else sha(v)) for k, v in bufs.items()}


def direct_apply(opt, scale, all_live=False, hyper=None):
    """FusedAdamW._apply's launches for one parameter group, with the step going through the single-group C entry point of its
    variant: scalar lr and weight_decay, no seg_group.  norm_state / counters are passed when the norm is measured, omega and
    theta_star once a task has been consolidated."""
    from indic_cl_asr_amd import _lib
    L, ptr, stream, f = _lib.lib(), _lib.ptr, _lib.stream_ptr(), opt.flat
    g = opt.param_groups[0]
    assert len(opt.param_groups) == 1
    opt.step_count += 1
    max_norm, skip = g.get("max_grad_norm"), bool(g.get("skip_nonfinite", False))
    si, agem = opt.path_integral, opt.projection
    measured = max_norm is not None or skip or opt.track_grad_norm
    penalised = si is not None and si.tasks_consolidated > 0
    all_live = bool(all_live) or penalised
    scale, nchunks, nseg = float(scale), f.chunk_table.shape[0], len(f.entries)
    if measured and opt._seg_norm is None:
        opt._seg_norm = torch.zeros(nseg, dtype=torch.float32, device="cuda")
        opt._norm_ws = torch.empty(L.ia_grad_norm_workspace_bytes(nchunks), dtype=torch.uint8, device="cuda")
    live = None if all_live else ptr(opt.seg_active)
    norm = (ptr(f.grad), ptr(f.chunk_table), nchunks, ptr(f.seg_chunk_begin), nseg, scale, 0.0 if max_norm is None else float(max_norm),
            live, ptr(opt._seg_norm), ptr(opt._norm_state), ptr(opt._norm_ws), opt._norm_ws.numel()) if measured else None
    head = (ptr(f.theta), ptr(f.grad), ptr(opt.exp_avg), ptr(opt.exp_avg_sq), ptr(f.chunk_table), nchunks, ptr(opt.seg_active),
            ptr(opt.seg_step), nseg, int(all_live), float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]),
            float(g["weight_decay"]), scale, ptr(opt.shadow))
    clip = (ptr(opt._norm_state) if measured else None, int(skip), ptr(opt._counters) if measured else None)
    if agem is not None:
        assert agem.has_reference
        ws = agem.workspace(nchunks)
        _lib.check(L.ia_agem_dots(ptr(f.grad), ptr(agem.ref.flat), ptr(f.chunk_table), nchunks, nseg, scale, live,
                                  ptr(agem.proj_state), ptr(ws), ws.numel(), stream), "ia_agem_dots")
        if measured:
            _lib.check(L.ia_grad_norm_projected(*norm, ptr(agem.ref.flat), ptr(agem.proj_state), stream), "ia_grad_norm_projected")
        _lib.check(L.ia_adamw_step_segmented_projected(*head, *clip, ptr(agem.ref.flat), ptr(agem.proj_state),
                                                       ptr(agem.proj_counters), stream), "ia_adamw_step_segmented_projected")
    else:
        if measured:
            _lib.check(L.ia_grad_norm(*norm, stream), "ia_grad_norm")
        if si is not None:
            _lib.check(L.ia_adamw_step_segmented_si(*head, *clip, ptr(si.w.flat), ptr(si.omega.flat) if penalised else None,
                                                    ptr(si.theta_star.flat) if penalised else None, float(si.si_c), stream),
                       "ia_adamw_step_segmented_si")
        else:
            assert measured
            _lib.check(L.ia_adamw_step_segmented_clipped(*head, *clip, stream), "ia_adamw_step_segmented_clipped")
    opt._after_update()


def run(big, before_step=None, extra=lambda method: {}, grads=None, direct=False, **kw):
    """One digest dict per step.  before_step prepares a step (references, scores); extra(method) names the variant's buffers;
    direct: the optimizer's launches go through direct_apply."""
    flat, opt, method = optimizer(big, **kw)
    if direct:
        opt._apply = functools.partial(direct_apply, opt)
    out = []
    for i, g in enumerate(grads_of(big) if grads is None else grads):
        g = g.cuda()
        if before_step is not None:
            before_step(i, g, flat, opt, method)
        flat.grad.copy_(g)
        opt.step()
        out.append(snapshot(opt, extra(method)))
    return out


def si_buffers(method):
    si = method["path_integral"]
    return {"w": si.w.flat, "omega": si.omega.flat}


def case_plain(big=False, **kw):
    return run(big, **kw)


def case_skip_nan(**kw):
    gs = [g.clone() for g in grads_of(False)]
    gs[1][4097] = float("nan")                                          # the second step is skipped, the third is not
    return run(False, grads=gs, skip_nonfinite=True, **kw)


def case_si(consolidated, **kw):
    from indic_cl_asr_amd import cl

    def prepare(i, g, flat, opt, method):
        if consolidated and i == 0:                                     # one step of a first task, then its end
            flat.grad.copy_(g)
            opt.step()
            method["path_integral"].consolidate()

    return run(False, before_step=prepare, extra=si_buffers, path_integral=lambda f: cl.SynapticIntelligence(f, si_c=0.5, xi=1e-3),
               **kw)


def case_agem(big, sign, **kw):
    from indic_cl_asr_amd import cl
    noise = inputs(big)["noise_agem"].cuda()

    def prepare(i, g, flat, opt, method):                               # the memory batch's gradient becomes the reference
        flat.grad.copy_(noise + 0.5 * sign * g)
        method["projection"].store_reference(opt)

    def own(method):
        return {"proj_state": method["projection"].proj_state, "proj_counters": method["projection"].proj_counters}

    return run(big, before_step=prepare, extra=own, projection=cl.AveragedGEM, **kw)


def case_gem(big, signs, **kw):
    from indic_cl_asr_amd import cl
    noise = [inputs(big)[f"noise_gem{k}"].cuda() for k in range(len(signs))]

    def prepare(i, g, flat, opt, method):                               # one memory batch per earlier task
        for k, s in enumerate(signs):
            flat.grad.copy_(noise[k] + 0.5 * s * g)
            method["projection"].store_reference(f"task{k}", opt)

    def own(method):
        return {"gem_state": method["projection"].state, "gem_counters": method["projection"].counters}

    return run(big, before_step=prepare, extra=own, projection=lambda f: cl.GEM(f, **GEM_KW), **kw)


def case_piggyback():
    from indic_cl_asr_amd import cl
    scores = inputs(False)["scores"].cuda()

    def prepare(i, g, flat, opt, method):
        if i == 0:
            pb = method["masks"]
            inside = torch.zeros(flat.numel, dtype=torch.bool, device="cuda")
            for name, off, k, _ in flat.entries:
                if name in MASKED:
                    inside[off:off + k] = True
            pb.scores.flat.copy_(torch.where(inside, scores, torch.zeros_like(scores)))

    def own(method):
        return {"scores": method["masks"].scores.flat, "bits": method["masks"]._pack()}

    return run(False, before_step=prepare, extra=own, masks=lambda f: cl.Piggyback(f, masked=MASKED, frozen=FROZEN),
               max_grad_norm=1.0)


CASES = {
    "plain": lambda: case_plain(),
    "clipped": lambda: case_plain(max_grad_norm=1.0),
    "skip_nan": case_skip_nan,
    "si_first_task": lambda: case_si(False),
    "si_consolidated_clipped": lambda: case_si(True, max_grad_norm=1.0),
    "agem_violating_clipped": lambda: case_agem(False, -1.0, max_grad_norm=1.0),
    "agem_agreeing": lambda: case_agem(False, +1.0),
    "gem_k3_mixed_clipped": lambda: case_gem(False, (-1.0, +1.0, -1.0), max_grad_norm=1.0),
    "piggyback_clipped": case_piggyback,
    "two_groups_plain": lambda: case_plain(param_groups=[GROUP1]),
    "two_groups_si": lambda: case_si(False, param_groups=[GROUP1]),
    "big_agem_clipped": lambda: case_agem(True, -1.0, max_grad_norm=1.0),
    "big_gem_clipped": lambda: case_gem(True, (-1.0, +1.0), max_grad_norm=1.0),
}


def is_big(case):
    return case.startswith("big_")


@functools.lru_cache(maxsize=None)
def golden():
    assert os.path.exists(GOLDEN), f"{GOLDEN} is missing: record it with `python tests/test_optimizer_digests_gpu.py`"
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("big", [False, True])
def test_inputs_are_the_recorded_ones(big):
    key = "inputs_big" if big else "inputs_small"
    assert key in golden(), f"{key} is not recorded"
    assert input_digests(big) == golden()[key], "the INPUTS differ from the recorded ones (the toy or torch's generators), not the kernels"


@pytest.mark.parametrize("case", list(CASES))
def test_step_digests(case):
    key = "inputs_big" if is_big(case) else "inputs_small"
    assert key in golden() and case in golden().get("cases", {}), f"{case} is not recorded"
    assert input_digests(is_big(case)) == golden()[key], \
        "the INPUTS differ from the recorded ones (the toy or torch's generators), not the kernels"
    got, want = CASES[case](), golden()["cases"][case]
    assert len(got) == len(want), (case, len(got), len(want))
    for step, (g, w) in enumerate(zip(got, want)):
        differing = sorted(k for k in set(g) | set(w) if g.get(k) != w.get(k))
        assert not differing, f"{case}, step {step}: {differing} differ from the recorded digests"


# case -> how to run it through the single-group entry point of its variant
DIRECT = {
    "clipped": lambda: case_plain(max_grad_norm=1.0, direct=True),                           # _clipped
    "skip_nan": lambda: case_skip_nan(direct=True),                                          # _clipped, a skipped step
    "si_first_task": lambda: case_si(False, direct=True),                                    # _si: no omega, no norm_state
    "si_consolidated_clipped": lambda: case_si(True, max_grad_norm=1.0, direct=True),        # _si: omega, theta_star, norm_state
    "agem_violating_clipped": lambda: case_agem(False, -1.0, max_grad_norm=1.0, direct=True),    # _projected with norm_state
    "agem_agreeing": lambda: case_agem(False, +1.0, direct=True),                            # _projected without
}


@pytest.mark.parametrize("case", list(DIRECT))
def test_single_group_entry_points(case):
    assert case in golden().get("cases", {}), f"{case} is not recorded"
    assert input_digests(False) == golden()["inputs_small"], \
        "the INPUTS differ from the recorded ones (the toy or torch's generators), not the kernels"
    got, want = DIRECT[case](), golden()["cases"][case]
    assert len(got) == len(want), (case, len(got), len(want))
    for step, (g, w) in enumerate(zip(got, want)):
        differing = sorted(k for k in set(g) | set(w) if g.get(k) != w.get(k))
        assert not differing, f"{case} through its single-group entry point, step {step}: {differing} differ from the recorded digests"


if __name__ == "__main__":
    record = {"inputs_small": input_digests(False), "inputs_big": input_digests(True),
              "cases": {name: fn() for name, fn in CASES.items()}}
    print(json.dumps(record, indent=1, sort_keys=True))
