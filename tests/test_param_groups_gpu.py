"""FusedAdamW parameter groups on the device (ia_adamw_step_segmented_grouped): per-tensor lr / weight_decay looked up per
chunk inside the three step kernels, on the toy module of tests/test_optimizer_clip_gpu.py.

The main check is bit equality per group: the grouped optimizer G next to one un-grouped optimizer U_k per group, built with
group k's lr / weight_decay and fed the same gradients -- on the elements of group k's tensors G and U_k must agree in every
bit of every buffer (the update is elementwise; norm, clip coefficient, dot and alpha are global and depend on the gradient
alone).  A float64 closed form of the first step guards against both being wrong together.

Groups:   G0 = v0..v4 (lr 1e-3, wd 1e-2; the constructor's)   G1 = v5..v9 + idle (1e-4, 0)   G2 = mat [+ big] (3e-3, 0.2)"""
import ctypes
import math

import pytest
import torch

from test_optimizer_clip_gpu import Toy, make_grad, state

pytestmark = pytest.mark.gpu

HYPER = [(1e-3, 1e-2), (1e-4, 0.0), (3e-3, 0.2)]
G1 = ["v5", "v6", "v7", "v8", "v9", "idle"]


def specs(big):
    return [dict(params=G1, lr=HYPER[1][0], weight_decay=HYPER[1][1]),
            dict(match="^(mat|big)$" if big else "^mat$", lr=HYPER[2][0], weight_decay=HYPER[2][1])]


def group_of(name):
    return 1 if name in G1 else (2 if name in ("mat", "big") else 0)


def build(big, grouped, k=0, method=None, **kw):
    """One optimizer on its own copy of the toy: grouped, or un-grouped with group k's values."""
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    extra = {}
    if method == "si":
        extra["path_integral"] = cl.SynapticIntelligence(flat, si_c=0.5)
    elif method == "agem":
        extra["projection"] = cl.AveragedGEM(flat)
    if grouped:
        opt = cl.FusedAdamW(flat, lr=HYPER[0][0], weight_decay=HYPER[0][1], param_groups=specs(big), **extra, **kw)
    else:
        opt = cl.FusedAdamW(flat, lr=HYPER[k][0], weight_decay=HYPER[k][1], **extra, **kw)
    return flat, opt


@pytest.fixture(scope="module")
def small_grads():
    """Three gradients for Toy(big=False), shared and never modified, with a reference that opposes each of them."""
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=False))
    e, n = list(flat.entries), flat.numel
    gs = [make_grad(e, n, 901).cuda(), make_grad(e, n, 902).cuda(), make_grad(e, n, 903).cuda()]
    return e, gs, -(gs[0] + gs[1] + gs[2])


@pytest.fixture(scope="module")
def big_grads():
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=True))
    e, n = list(flat.entries), flat.numel
    return e, [make_grad(e, n, 911).cuda(), make_grad(e, n, 912, scale=1e-5).cuda(), make_grad(e, n, 913).cuda()]


def same_stats(a, b):
    return a.keys() == b.keys() and all(a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]) for k in a)


def buffers(opt):
    out = {k: v for k, v in state(opt).items() if k != "seg_step"}
    if opt.path_integral is not None:
        out["si.w"] = opt.path_integral.w.flat
    return out


def compare_per_group(entries, G, Us, what):
    bg, bu = buffers(G), [buffers(U) for U in Us]
    steps_g, steps_u = G.seg_step.tolist(), [U.seg_step.tolist() for U in Us]
    for seg, (name, off, k, _) in enumerate(entries):
        gi = group_of(name)
        for key in bg:
            assert torch.equal(bg[key][off:off + k], bu[gi][key][off:off + k]), (what, name, key)
        assert steps_g[seg] == steps_u[gi][seg], (what, name, "seg_step")
    for U in Us:
        assert same_stats(G.stats(), U.stats()), (what, G.stats(), U.stats())
        if G.projection is not None:
            assert same_stats(G.projection.stats(), U.projection.stats()), (what, G.projection.stats(), U.projection.stats())


def run_variant(entries, gs, big, method=None, ref=None, consolidate=False, **kw):
    flat_g, G = build(big, True, method=method, **kw)
    pairs = [build(big, False, k, method=method, **kw) for k in range(3)]
    Us = [u for _, u in pairs]
    everyone = [(flat_g, G)] + pairs
    assert all(torch.equal(flat_g.theta, f.theta) for f, _ in pairs)
    idle_seg = [e[0] for e in entries].index("idle")
    _, idle_off, idle_k, _ = entries[idle_seg]
    idle0 = {key: v[idle_off:idle_off + idle_k].clone() for key, v in buffers(G).items()}
    rounds = 2 if consolidate else 1
    for r in range(rounds):
        for step, g in enumerate(gs):
            for f, o in everyone:
                if ref is not None:
                    f.grad.copy_(ref)
                    o.projection.store_reference(o)
                f.grad.copy_(g)
                o.step()
            compare_per_group(entries, G, Us, f"round {r} step {step}")
            if ref is not None:
                assert G.projection.stats()["projected"] == 1, G.projection.stats()
        if r == 0:       # no penalty so far: `idle` received nothing and kept its bits, whatever its neighbours' groups
            for key, v in buffers(G).items():
                assert torch.equal(v[idle_off:idle_off + idle_k], idle0[key]), key
            assert G.seg_step.tolist()[idle_seg] == 0
            assert all(s == len(gs) for i, s in enumerate(G.seg_step.tolist()) if i != idle_seg)
        if consolidate and r == 0:
            for _, o in everyone:
                o.path_integral.consolidate()
    if consolidate:      # the penalised steps made every tensor live
        assert all(s == 2 * len(gs) for i, s in enumerate(G.seg_step.tolist()) if i != idle_seg)
        assert G.seg_step.tolist()[idle_seg] == len(gs)
    # the groups really differ: group 2's weights in G are not what the group-0 optimizer made of them
    _, off, k, _ = entries[[e[0] for e in entries].index("mat")]
    assert not torch.equal(G.flat.theta[off:off + k], Us[0].flat.theta[off:off + k])
    return G


@pytest.mark.parametrize("variant", ["plain", "clipped", "si", "si_consolidated", "agem"])
def test_each_group_matches_the_ungrouped_kernel_bit_for_bit(small_grads, variant):
    entries, gs, ref = small_grads
    if variant == "plain":
        run_variant(entries, gs, False)
    elif variant == "clipped":
        G = run_variant(entries, gs, False, max_grad_norm=1.0, skip_nonfinite=True)
        assert G.stats()["clipped_steps"] == 3 and G.stats()["skipped_steps"] == 0
    elif variant == "si":
        G = run_variant(entries, gs, False, method="si")
        assert G.path_integral.w.flat.ne(0).any()
    elif variant == "si_consolidated":
        G = run_variant(entries, gs, False, method="si", consolidate=True)
        assert G.path_integral.tasks_consolidated == 1 and G.path_integral.omega.flat.gt(0).any()
    else:
        G = run_variant(entries, gs, False, method="agem", ref=ref)
        assert G.projection.stats()["projected_steps"] == 3


@pytest.mark.parametrize("variant", ["plain", "clipped"])
def test_more_chunks_than_workgroups(big_grads, variant):
    """2049 + chunks on 2048 workgroups: every workgroup serves a chunk of an early tensor (G0 / G1) and then one of `big`
    (G2) -- a lookup hoisted out of the chunk loop would give `big` the wrong values."""
    entries, gs = big_grads
    kw = dict(max_grad_norm=1.0, skip_nonfinite=True) if variant == "clipped" else {}
    run_variant(entries, gs, True, **kw)


def closed_form_check(entries, theta0, grad, theta1, hyper_of, eps=1e-8):
    """theta1 = theta0 * (1 - lr * wd) - lr * g / (|g| + eps) in float64 from the fp32-rounded lr, wd, eps (with those the first
    step's bias corrections cancel exactly).  Bound per element 16 * 2^-24 * (|theta0| + lr): the update term passes through at
    most 11 fp32 roundings relative to a magnitude <= lr (the moments, the square root, the two bias factors, eps, the quotient,
    the product, the cast of step_size), the decay factor and product add 3 relative to |theta0|, the final difference 1.
    Returns the worst ratio to the bound over the tensors `hyper_of` knows (name -> (lr, wd), None for a tensor to skip)."""
    f32 = lambda x: torch.tensor(x, dtype=torch.float32).double().item()
    worst = 0.0
    for name, off, k, _ in entries:
        hp = hyper_of(name)
        if hp is None:
            continue
        lr, wd, e = f32(hp[0]), f32(hp[1]), f32(eps)
        t0, g, t1 = (x[off:off + k].double() for x in (theta0, grad, theta1))
        want = t0 * (1.0 - lr * wd) - lr * g / (g.abs() + e)
        bound = 16 * 2.0 ** -24 * (t0.abs() + lr)
        ratio = ((t1 - want).abs() / bound).max().item()
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, ratio)
    return worst


def test_first_step_matches_the_closed_form_in_float64(small_grads):
    entries, gs, _ = small_grads
    flat, G = build(False, True)
    theta0 = flat.theta.clone()
    flat.grad.copy_(gs[0])
    G.step()
    worst = closed_form_check(entries, theta0, gs[0], flat.theta, lambda n: None if n == "idle" else HYPER[group_of(n)])
    print("closed form: worst ratio to the bound", worst)
    # the closed form separates the groups: with group 0's values group 2's tensor misses the bound by far
    with pytest.raises(AssertionError):
        closed_form_check(entries, theta0, gs[0], flat.theta, lambda n: HYPER[0] if n == "mat" else None)


def test_one_group_is_the_old_path(small_grads):
    from indic_cl_asr_amd import _lib, cl
    entries, gs, _ = small_grads
    kw = dict(lr=2e-3, weight_decay=0.05, max_grad_norm=1.0)
    flats = [cl.FlatParams(Toy(big=False).cuda()) for _ in range(3)]
    opts = [cl.FusedAdamW(flats[0], **kw),
            cl.FusedAdamW(flats[1], param_groups=[], **kw),
            cl.FusedAdamW(flats[2], param_groups=[dict(match=".", lr=2e-3, weight_decay=0.05)], **kw)]
    assert [len(o.param_groups) for o in opts] == [1, 1, 2] and opts[2].param_groups[0]["params"] == []
    for g in gs:
        for f, o in zip(flats, opts):
            f.grad.copy_(g)
            o.step()
        for o in opts[1:]:
            for key, v in state(opts[0]).items():
                assert torch.equal(v, state(o)[key]), key
            assert same_stats(opts[0].stats(), o.stats())
    assert opts[0].stats()["clipped_steps"] == 3
    # the C entry points directly: ngroups = 1 and a NULL seg_group against ia_adamw_step_segmented
    L = _lib.lib()
    fa, fb = cl.FlatParams(Toy(big=False).cuda()), cl.FlatParams(Toy(big=False).cuda())
    bufs = []
    for f in (fa, fb):
        bufs.append(dict(m=torch.zeros_like(f.theta), v=torch.zeros_like(f.theta), shadow=f.theta.to(torch.bfloat16),
                         active=torch.zeros(len(entries), dtype=torch.int32, device="cuda"),
                         step=torch.zeros(len(entries), dtype=torch.int32, device="cuda")))
    nchunks, nseg = fa.chunk_table.shape[0], len(entries)
    lr, wd = (ctypes.c_float * 1)(2e-3), (ctypes.c_float * 1)(0.05)
    for g in gs[:2]:
        fa.grad.copy_(g); fb.grad.copy_(g)
        a, b = bufs
        head = lambda f, x: (_lib.ptr(f.theta), _lib.ptr(f.grad), _lib.ptr(x["m"]), _lib.ptr(x["v"]), _lib.ptr(f.chunk_table),
                             nchunks, _lib.ptr(x["active"]), _lib.ptr(x["step"]), nseg, 0)
        _lib.check(L.ia_adamw_step_segmented(*head(fa, a), 2e-3, 0.9, 0.999, 1e-8, 0.05, 1.0, _lib.ptr(a["shadow"]),
                                             _lib.stream_ptr()), "ia_adamw_step_segmented")
        _lib.check(L.ia_adamw_step_segmented_grouped(*head(fb, b), 0.9, 0.999, 1e-8, 1.0, _lib.ptr(b["shadow"]), None, 1, lr, wd,
                                                     None, 0, None, None, None, None, 0.0, None, None, None, _lib.stream_ptr()),
                   "ia_adamw_step_segmented_grouped")
        assert torch.equal(fa.theta, fb.theta)
        for key in a:
            assert torch.equal(a[key], b[key]), key
    assert a["step"].tolist().count(2) == nseg - 1 and not torch.equal(fa.theta, cl.FlatParams(Toy(big=False).cuda()).theta)


def test_scheduler_moves_each_group_and_global_settings_hold(small_grads):
    entries, gs, _ = small_grads
    lambdas = [lambda e: 1.0 / (1 + e), lambda e: 0.5 ** e, lambda e: 1.0 + 0.5 * e]
    fa, A = build(False, True, max_grad_norm=1.0, skip_nonfinite=True)
    fb, B = build(False, True, max_grad_norm=1.0, skip_nonfinite=True)
    sched = torch.optim.lr_scheduler.LambdaLR(A, lambdas)
    seq = [gs[0], gs[1], gs[2], gs[0]]
    for epoch, g in enumerate(seq):
        for k, grp in enumerate(B.param_groups):
            grp["lr"] = HYPER[k][0] * lambdas[k](epoch)
        assert [grp["lr"] for grp in A.param_groups] == [grp["lr"] for grp in B.param_groups]
        fa.grad.copy_(g); fb.grad.copy_(g)
        A.step(); B.step()
        sched.step()
        for key, v in state(A).items():
            assert torch.equal(v, state(B)[key]), (epoch, key)
    # the schedule was felt: a third optimizer at constant rates ends elsewhere
    fc, C = build(False, True, max_grad_norm=1.0, skip_nonfinite=True)
    for g in seq:
        fc.grad.copy_(g)
        C.step()
    assert not torch.equal(fc.theta, fa.theta)
    # betas are one per optimizer: refused before anything is launched
    before = {key: v.clone() for key, v in state(A).items()}
    A.param_groups[1]["betas"] = (0.8, 0.999)
    fa.grad.copy_(gs[2])
    with pytest.raises(ValueError, match=r"param_groups\[1\]\['betas'\]"):
        A.step()
    for key, v in state(A).items():
        assert torch.equal(v, before[key]), key
    assert A.step_count == 4 and int(A.seg_active.abs().sum()) == 0
    A.param_groups[1]["betas"] = A.param_groups[0]["betas"]
    # a non-finite gradient with skip_nonfinite: no group's state moves, one skipped step
    off = [e for e in entries if e[0] == "v9"][0][1]
    fa.grad.copy_(gs[2])
    fa.grad[off + 4100] = float("inf")            # data in a gradient buffer: nothing here faults the device
    A.step()
    for key, v in state(A).items():
        assert torch.equal(v, before[key]), key
    st = A.stats()
    assert st["skipped_steps"] == 1 and math.isinf(st["grad_norm"]) and int(A.seg_active.abs().sum()) == 0


def test_through_the_model_with_layerwise_groups():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    from test_si_gpu import _batch
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny')).cuda().train()
    freeze_layer(m, 0)
    flat = cl.FlatParams(m)
    opt = cl.FusedAdamW(flat, lr=1e-3, param_groups=cl.layerwise_lr_groups(m, 1e-3, 0.5))
    hyper = {n: (g["lr"], g["weight_decay"]) for g in opt.param_groups for n in g["names"]}
    assert len(hyper) == len(flat.names) and {lr for lr, _ in hyper.values()} == {1e-3, 0.5e-3}
    assert {wd for _, wd in hyper.values()} == {0.0, 1e-2}
    batch, langs = _batch(['hi'] * 4, seed=1)
    entries = list(flat.entries)
    for step in range(2):
        opt.zero_grad()
        loss, _ = m.training_step(batch, langs, compute_wer=False)
        loss.backward()
        if step == 0:
            theta0, grad = flat.theta.clone(), flat.grad.clone()
            opt.step()
            live = {name for name, off, k, _ in entries if grad[off:off + k].ne(0).any()}
            assert len(live) > len(entries) // 2
            worst = closed_form_check(entries, theta0, grad, flat.theta, lambda n: hyper[n] if n in live else None)
            print("through the model: worst ratio to the bound", worst, "live tensors", len(live), "of", len(entries))
            heads = [e for e in entries if ".ta." in e[0]]
            assert heads and not any(e[0] in live for e in heads)
            for name, off, k, _ in heads:                        # no gradient: no decay, no movement
                assert torch.equal(flat.theta[off:off + k], theta0[off:off + k]), name
        else:
            opt.step()
    assert torch.equal(opt.shadow[:flat.numel].float(), flat.theta.bfloat16().float())
    assert math.isfinite(float(loss.detach()))
