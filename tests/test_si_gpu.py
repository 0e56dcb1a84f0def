"""Synaptic Intelligence inside the fused optimizer step (ia_adamw_step_segmented_si, ia_si_consolidate) on the toy module of
tests/test_optimizer_clip_gpu.py, whose tensor sizes reach every path of the flat kernels (a tail shorter than a float4, the
alignment gaps, the 4096 chunk boundary, the 2-D shadow view, the idle tensor and -- `big=True`, first test only -- more than
2048 chunks), and once through the model.

The definitions (include/indicasr.h), per element of a live tensor, each product / difference / sum rounded to fp32 on its own:
    ge = g * grad_scale;  G = ge * coef + (2 * si_c * omega) * (theta - theta_star);  theta' = AdamW(theta, G)
    w  = w - ge * (theta' - theta)
so the checks are bit for bit: the weights and moments against the plain optimizer fed G built with one torch op per rounding,
w against the same rule in torch ops.  Only consolidate() has a tolerance: omega += max(0, w / ((theta - theta_star)^2 + xi))
against float64 within 1e-6 relative -- the added term sits under at most 7 fp32 roundings (the difference, its square, the
sum with xi, xi's own fp32 image, the quotient; none cancels except theta - theta_star, whose inputs are exact fp32:
7 * 2^-24 = 4.2e-7) plus one rounding for the sum."""
import pytest
import torch

from test_optimizer_clip_gpu import Toy, assert_same, make_grad, norms64, state

pytestmark = pytest.mark.gpu

XI = 1e-3


def build(big=False, si=True, si_kw=None, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    s = cl.SynapticIntelligence(flat, xi=XI, **(si_kw or {})) if si else None
    return flat, s, cl.FusedAdamW(flat, lr=1e-3, path_integral=s, **kw)


def make_grads(big):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big))
    e, n = list(flat.entries), flat.numel
    return e, [make_grad(e, n, 101).cuda(), make_grad(e, n, 102, scale=1e-5).cuda(), make_grad(e, n, 103).cuda()]


@pytest.fixture(scope="module")
def grads():
    """Toy(big=False): two gradients at norm ~ 4.7e2 and one far below the clip threshold of 1, on the device (never modified)."""
    return make_grads(big=False)


def dead_mask(entries, numel):
    """True in the alignment gaps and inside `idle` (the tensor that never receives a gradient)."""
    dead = torch.ones(numel, dtype=torch.bool, device="cuda")
    for name, off, k, _ in entries:
        if name != "idle":
            dead[off:off + k] = False
    return dead


def w_rule(w_prev, ge, theta_after, theta_before):
    """w - ge * (theta' - theta), one fp32 torch op per rounding."""
    moved = theta_after - theta_before
    prod = ge * moved
    return w_prev - prod


def first_task(entries, gs, big=False, **kw):
    """Steps A (with the path integral) and a plain twin B through `gs`, checking both after every step."""
    fa, si, A = build(big=big, **kw)
    fb, _, B = build(big=big, si=False)
    dead = dead_mask(entries, fa.numel)
    for step, g in enumerate(gs):
        before, w_prev = fa.theta.clone(), si.w.flat.clone()
        fa.grad.copy_(g); fb.grad.copy_(g)
        A.step(); B.step()
        assert_same(A, B, f"step {step}")
        assert torch.equal(si.w.flat, w_rule(w_prev, g * 1.0, fa.theta, before)), step
        assert not si.w.flat[dead].any()
        assert si.w.flat[~dead].ne(0).any()
    assert not si.omega.flat.any() and si.tasks_consolidated == 0
    return fa, si, A, fb, B


def test_first_task_is_the_plain_step_and_w_follows_the_rule_bit_for_bit():
    entries, gs = make_grads(big=True)
    fa, si, A, _, _ = first_task(entries, gs, big=True)
    idle = [i for i, e in enumerate(entries) if e[0] == "idle"][0]
    steps = A.seg_step.tolist()
    assert steps[idle] == 0 and all(s == 3 for i, s in enumerate(steps) if i != idle)
    assert float(si.w.flat.sum()) > 0                     # moving against the gradient: the path integral grows


def test_with_clipping_w_integrates_the_unclipped_task_gradient(grads):
    entries, gs = grads
    fa, si, A = build(max_grad_norm=1.0)
    fb, _, B = build(si=False)
    dead = dead_mask(entries, fa.numel)
    for step, g in enumerate(gs):
        before, w_prev = fa.theta.clone(), si.w.flat.clone()
        fa.grad.copy_(g)
        A.step()
        st = A.stats()
        coef = torch.tensor(st["clip_coef"], dtype=torch.float32, device="cuda")
        fb.grad.copy_(g * coef)           # fp32 product on the device, as tests/test_optimizer_clip_gpu.py feeds its twin
        B.step()
        assert_same(A, B, f"step {step}")
        assert torch.equal(si.w.flat, w_rule(w_prev, g * 1.0, fa.theta, before)), step
        assert not si.w.flat[dead].any()
        if step == 0:                     # without `big` the norm is 3 * sqrt(24.7e3 live elements) ~ 4.7e2: coef ~ 2.1e-3
            _, total64 = norms64(entries, g.cpu())
            assert total64 > 100.0 and abs(st["clip_coef"] - 1.0 / (total64 + 1e-6)) <= 2e-6 * st["clip_coef"]
            assert not torch.equal(si.w.flat, w_rule(w_prev, (g * 1.0) * coef, fa.theta, before))
        if step == 1:
            assert st["clip_coef"] == 1.0
    assert A.stats()["clipped_steps"] == 2


def test_nonfinite_step_leaves_w_untouched(grads):
    entries, (g0, _, g2) = grads
    fa, sa, A = build(skip_nonfinite=True)
    fb, sb, B = build(skip_nonfinite=True)            # the twin that never sees the bad step
    for f, o in ((fa, A), (fb, B)):
        f.grad.copy_(g0)
        o.step()
    before = {k: v.clone() for k, v in state(A).items()}
    w_before = sa.w.flat.clone()
    off = [e for e in entries if e[0] == "v9"][0][1]
    fa.grad.copy_(g2)
    fa.grad[off + 4100] = float("inf")                # data in a gradient buffer: nothing here faults the device
    A.step()
    for k, v in state(A).items():
        assert torch.equal(v, before[k]), k
    assert torch.equal(sa.w.flat, w_before)
    assert int(A.seg_active.abs().sum()) == 0 and A.stats()["skipped_steps"] == 1
    for f, o in ((fa, A), (fb, B)):
        f.grad.copy_(g2)
        o.step()
    assert_same(A, B, "after the skipped step")
    assert torch.equal(sa.w.flat, sb.w.flat) and not torch.equal(sa.w.flat, w_before)
    assert B.stats()["skipped_steps"] == 0


def consolidated(entries, gs, **kw):
    """First task on Toy(big=False), then consolidate(), checked against float64; returns both optimizers."""
    fa, si, A, fb, B = first_task(entries, gs, **kw)
    dead = dead_mask(entries, fa.numel)
    theta, star, w = fa.theta.double().cpu(), si.theta_star.flat.double().cpu(), si.w.flat.double().cpu()
    want = (w / ((theta - star) ** 2 + XI)).clamp_min(0.0)
    si.consolidate()
    got = si.omega.flat.double().cpu()
    err = ((got - want).abs() / want.abs().clamp_min(1e-300)).max().item()
    print("omega vs float64: worst rel", err, "positive entries", int((want > 0).sum()), "dropped", int((w < 0).sum()))
    assert bool(((got - want).abs() <= 1e-6 * want.abs()).all())
    assert bool((si.omega.flat >= 0).all()) and not si.omega.flat[dead].any() and si.omega.flat[~dead].gt(0).any()
    assert not si.w.flat.any()
    assert torch.equal(si.theta_star.flat, fa.theta)
    assert si.tasks_consolidated == 1
    return fa, si, A, fb, B


def test_consolidate_matches_float64_and_is_idempotent_without_steps(grads):
    entries, gs = grads
    fa, si, A, _, _ = consolidated(entries, gs)
    omega, theta = si.omega.flat.clone(), fa.theta.clone()
    si.consolidate()
    assert torch.equal(si.omega.flat, omega) and torch.equal(si.theta_star.flat, theta) and torch.equal(fa.theta, theta)
    assert not si.w.flat.any() and si.tasks_consolidated == 2
    from indic_cl_asr_amd import cl
    with pytest.raises(ValueError):
        cl.SynapticIntelligence(fa, xi=0.0)


def test_second_task_fused_penalty_bit_for_bit(grads):
    entries, gs = grads
    fa, si, A, fb, B = consolidated(entries, gs, si_kw=dict(si_c=0.5))
    assert_same(A, B, "start of the second task")
    c2 = torch.tensor(2.0 * 0.5, dtype=torch.float32, device="cuda")
    idle = [e for e in entries if e[0] == "idle"][0]
    idle_before = fa.theta[idle[1]:idle[1] + idle[2]].clone()
    for step, g in enumerate(gs[:2]):
        before, w_prev = fa.theta.clone(), si.w.flat.clone()
        fa.grad.copy_(g)
        A.step()
        cw = c2 * si.omega.flat                       # one fp32 torch op per rounding of the definition
        d = fb.theta - si.theta_star.flat
        pen = cw * d
        fb.grad.copy_(g * 1.0 + pen)
        fb.all_grads_live = True                      # what autograd on loss + surrogate gives: every tensor has a gradient
        B.step()
        assert_same(A, B, f"penalised step {step}")
        assert torch.equal(si.w.flat, w_rule(w_prev, g * 1.0, fa.theta, before)), step     # the task gradient only
    assert not torch.equal(fa.theta[idle[1]:idle[1] + idle[2]], idle_before)                # weight decay, zero gradient
    steps = A.seg_step.tolist()
    assert all(s == (2 if e[0] == "idle" else 5) for s, e in zip(steps, entries))
    want = float((si.omega.flat.double().cpu() * (fa.theta.double().cpu() - si.theta_star.flat.double().cpu()) ** 2).sum())
    got = float(si.penalty_value())
    print("penalty_value", got, "float64", want, "rel", abs(got - want) / want)
    assert want > 0 and abs(got - want) <= 1e-4 * want


def _batch(langs, seed, B=4, L=16000, U=6):
    g = torch.Generator().manual_seed(seed)
    sl = torch.tensor([L] + [int(L * (0.55 + 0.45 * torch.rand(1, generator=g))) for _ in range(B - 1)])
    sig = torch.randn(B, L, generator=g) * 0.1
    for i in range(B):
        sig[i, sl[i]:] = 0
    tl = torch.tensor([U] + [int(torch.randint(1, U + 1, (1,), generator=g)) for _ in range(B - 1)])
    tr = torch.randint(0, 16, (B, U), generator=g)
    return tuple(t.cuda() for t in (sig, sl, tr, tl)), langs


def test_through_the_model_two_tasks():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny')).cuda().train()
    freeze_layer(m, 0)
    flat = cl.FlatParams(m)
    si = cl.SynapticIntelligence(flat, xi=XI)
    opt = cl.FusedAdamW(flat, lr=1e-3, path_integral=si)
    w = torch.zeros_like(flat.theta)

    def task(batch, langs, steps=2):
        nonlocal w
        for _ in range(steps):
            opt.zero_grad()
            loss, monitor = m.training_step(batch, langs, compute_wer=False)
            loss.backward()
            g, before = flat.grad.clone(), flat.theta.clone()
            opt.step()
            w = w_rule(w, g * 1.0, flat.theta, before)
            assert torch.equal(si.w.flat, w)
            monitor['si_penalty'] = float(si.penalty_value())
        return monitor

    mon = task(*_batch(['hi'] * 4, seed=1))
    assert mon['si_penalty'] == 0.0 and mon['train_loss'] == mon['train_loss']
    assert si.w.flat.ne(0).any()
    si.consolidate()
    w = torch.zeros_like(w)
    for name, view in si.omega.items():
        if ".ta." in name:
            assert not view.any(), name
    assert any(view.gt(0).any() for name, view in si.omega.items() if ".hi." in name)
    assert any(".ta." in n for n in si.omega) and bool((si.omega.flat >= 0).all())
    mon = task(*_batch(['ta'] * 4, seed=2))
    assert mon['si_penalty'] > 0.0 and 'train_loss' in mon
    assert all(s >= 2 for s in opt.seg_step.tolist())     # with the penalty every tensor is live, the `hi` heads included
