"""Riemannian Walk inside the fused optimizer step (ia_adamw_step_segmented_rwalk, ia_rwalk_consolidate) on the toy module of
tests/test_optimizer_clip_gpu.py, whose tensor sizes reach every path of the flat kernels (a tail shorter than a float4, the
alignment gaps, the 4096 chunk boundary, the idle tensor and -- `big=True`, first test only -- more than 2048 chunks), and once
through the model.

The definitions (include/indicasr.h), per element of a live tensor, each product / difference / sum rounded to fp32 on its own:
    ge = g * grad_scale;  G = ge * coef + (2 * rw_lambda * importance) * (theta - theta_star);  theta' = AdamW(theta, G)
    F' = F + alpha * (ge*ge - F);  w' = w - ge * (theta' - theta)
    fold:  score += max(0, w') / ((0.5*F') * (theta' - anchor)^2 + eps);  w = 0;  anchor = theta'
so weights, moments, F and w are checked bit for bit: against the plain optimizer fed G built with one torch op per rounding, and
against the same rules in torch ops.  The two quantities with a division are held to float64 from the same stored fp32 inputs,
within bounds counted from roundings:
    one fold's score   6 roundings (d, d*d, u, den, the quotient, the sum; 0.5*F is exact, eps enters as its fp32 image), no term
                       cancels (all are >= 0): 6 * 2^-24 = 3.6e-7, asserted <= 4e-7 relative
    importance         4 roundings (two quotients, the sum inside the mean, the final sum; * 0.5 is exact): 4 * 2^-24 = 2.4e-7,
                       asserted <= 3e-7 relative
A float64 quotient of two fp32 numbers rounded once more to fp32 IS the correctly rounded fp32 quotient (53 >= 2 * 24 + 2
bits), so the normalisation is also checked exactly."""
import pytest
import torch

from test_optimizer_clip_gpu import Toy, assert_same, make_grad, state
from test_si_gpu import _batch, dead_mask, w_rule

pytestmark = pytest.mark.gpu

ALPHA, EPS = 0.9, 1e-3
SCORE_TOL, OMEGA_TOL = 4e-7, 3e-7
ALL = ("fisher", "importance", "theta_star", "w", "anchor", "score", "score_acc")


def build(big=False, rw=True, rw_kw=None, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    kw.setdefault("lr", 1e-3)
    r = cl.RWalk(flat, **dict(dict(alpha=ALPHA, eps=EPS), **(rw_kw or {}))) if rw else None
    return flat, r, cl.FusedAdamW(flat, path_integral=r, **kw)


def make_grads(big):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big))
    e, n = list(flat.entries), flat.numel
    return e, [make_grad(e, n, 201).cuda(), make_grad(e, n, 202, scale=1e-5).cuda(), make_grad(e, n, 203).cuda()]


@pytest.fixture(scope="module")
def grads():
    """Toy(big=False): two gradients at norm ~ 4.7e2 and one far below the clip threshold of 1, on the device (never modified)."""
    return make_grads(big=False)


def f32(x):
    return torch.tensor(x, dtype=torch.float32, device="cuda")


def fisher_rule(F, ge, alpha=ALPHA):
    """F + alpha * (ge*ge - F), one fp32 torch op per rounding."""
    sq = ge * ge
    df = sq - F
    t = f32(alpha) * df
    return F + t


def fold64(score_prev, w, theta, anchor, F, eps=EPS):
    """score + max(0, w) / (0.5 * F * (theta - anchor)^2 + eps) in float64 from fp32 inputs (eps as its fp32 image)."""
    d = theta.double() - anchor.double()
    den = 0.5 * F.double() * d * d + f32(eps).double()
    return score_prev.double() + w.double().clamp_min(0.0) / den


def worst_rel(got, want64):
    """max |got - want| / want over the entries where want != 0; where want == 0, got must be 0 exactly."""
    got = got.double()
    assert bool((got[want64 == 0] == 0).all())
    nz = want64 != 0
    return float(((got[nz] - want64[nz]).abs() / want64[nz].abs()).max())


def quotient(x, mx):
    """The correctly rounded fp32 x / mx (0 where mx == 0)."""
    if float(mx) == 0.0:
        return torch.zeros_like(x)
    return (x.double() / mx.double()).float()


def buffers(rw):
    return {k: getattr(rw, k).flat for k in ALL if getattr(rw, k) is not None}


def assert_same_buffers(a, b, what):
    ba, bb = buffers(a), buffers(b)
    assert ba.keys() == bb.keys()
    for k in ba:
        assert torch.equal(ba[k], bb[k]), (what, k)


def step_pair(fa, rw, A, fb, B, g, dead, what, fold, coef=None):
    """One step of A (with RWalk) and of the plain twin B (fed g [* coef]); checks weights, F, w, anchor and the fold flag, and
    returns (score before, w' of the rule, anchor before) for the score checks."""
    before, F_prev, w_prev = fa.theta.clone(), rw.fisher.flat.clone(), rw.w.flat.clone()
    anchor_prev, score_prev = rw.anchor.flat.clone(), rw.score.flat.clone()
    fa.grad.copy_(g)
    A.step()
    if coef is None:
        fb.grad.copy_(g)
    else:
        fb.grad.copy_(g * coef(A))
    B.step()
    assert_same(A, B, what)
    ge = g * 1.0
    assert torch.equal(rw.fisher.flat, fisher_rule(F_prev, ge)), what
    w_new = w_rule(w_prev, ge, fa.theta, before)
    for k in ("fisher", "w", "score"):
        assert not getattr(rw, k).flat[dead].any(), (what, k)
    assert torch.equal(rw.anchor.flat[dead], anchor_prev[dead]), what
    if fold:
        assert not rw.w.flat.any() and torch.equal(rw.anchor.flat, fa.theta), what
        assert w_new[~dead].ne(0).any()
    else:
        assert torch.equal(rw.w.flat, w_new) and rw.w.flat[~dead].ne(0).any(), what
        assert torch.equal(rw.anchor.flat, anchor_prev) and torch.equal(rw.score.flat, score_prev), what
    return score_prev, w_new, anchor_prev


def check_fold(fa, rw, score_prev, w_new, anchor_prev, what):
    want = fold64(score_prev, w_new, fa.theta, anchor_prev, rw.fisher.flat)
    err = worst_rel(rw.score.flat, want)
    print(what, "score vs float64: worst rel", err, "positive", int((want > 0).sum()), "dropped", int((w_new < 0).sum()))
    assert err <= SCORE_TOL, (what, err)
    assert bool((rw.score.flat >= 0).all())


def test_first_language_is_the_plain_step_and_fisher_and_w_follow_their_rules_bit_for_bit():
    entries, gs = make_grads(big=True)
    fa, rw, A = build(big=True, rw_kw=dict(interval=3))
    fb, _, B = build(big=True, rw=False)
    dead = dead_mask(entries, fa.numel)
    for step, g in enumerate(gs):
        sp, wn, ap = step_pair(fa, rw, A, fb, B, g, dead, f"step {step}", fold=step == 2)
    check_fold(fa, rw, sp, wn, ap, "big, fold at call 3")
    idle = [i for i, e in enumerate(entries) if e[0] == "idle"][0]
    steps = A.seg_step.tolist()
    assert steps[idle] == 0 and all(s == 3 for i, s in enumerate(steps) if i != idle)
    assert not rw.importance.flat.any() and rw.tasks_consolidated == 0 and rw.calls == 3
    assert rw.fisher.flat[~dead].gt(0).all() and rw.score.flat.gt(0).any()


@pytest.mark.parametrize("interval,folds", [(1, {1, 2, 3, 4, 5, 6}), (3, {3, 6})])
def test_folds_happen_on_every_interval_th_applied_call(grads, interval, folds):
    entries, gs = grads
    fa, rw, A = build(rw_kw=dict(interval=interval))
    fb, _, B = build(rw=False)
    dead = dead_mask(entries, fa.numel)
    for call in range(1, 7):
        sp, wn, ap = step_pair(fa, rw, A, fb, B, gs[(call - 1) % 3], dead, f"interval {interval} call {call}", fold=call in folds)
        if call in folds:                                 # the first fold adds to 0, the later ones to a stored score
            check_fold(fa, rw, sp, wn, ap, f"interval {interval} call {call}")
    assert rw.calls == 6


def test_with_clipping_fisher_and_w_follow_the_unclipped_task_gradient(grads):
    entries, gs = grads
    fa, rw, A = build(max_grad_norm=1.0, rw_kw=dict(interval=50))
    fb, _, B = build(rw=False)
    dead = dead_mask(entries, fa.numel)
    for step, g in enumerate(gs):
        before, F_prev, w_prev = fa.theta.clone(), rw.fisher.flat.clone(), rw.w.flat.clone()
        step_pair(fa, rw, A, fb, B, g, dead, f"clipped step {step}", fold=False,
                  coef=lambda opt: f32(opt.stats()["clip_coef"]))
        coef = A.stats()["clip_coef"]
        if step == 0:                                     # norm 3 * sqrt(24.7e3 live elements) ~ 4.7e2: coef ~ 2.1e-3
            assert coef < 0.01
            clipped = (g * 1.0) * f32(coef)
            assert not torch.equal(rw.fisher.flat, fisher_rule(F_prev, clipped))
            assert not torch.equal(rw.w.flat, w_rule(w_prev, clipped, fa.theta, before))
        if step == 1:
            assert coef == 1.0
    assert A.stats()["clipped_steps"] == 2


def test_nonfinite_step_leaves_every_buffer_untouched_and_drops_the_fold_that_was_due(grads):
    entries, (g0, _, g2) = grads
    fa, ra, A = build(skip_nonfinite=True, rw_kw=dict(interval=2))      # calls: g0, bad (fold due, skipped), g2, g0 (fold)
    fb, rb, B = build(skip_nonfinite=True, rw_kw=dict(interval=3))      # the twin that never sees the bad step: g0, g2, g0 (fold)
    for f, o in ((fa, A), (fb, B)):
        f.grad.copy_(g0)
        o.step()
    before = {k: v.clone() for k, v in state(A).items()}
    rw_before = {k: v.clone() for k, v in buffers(ra).items()}
    off = [e for e in entries if e[0] == "v9"][0][1]
    fa.grad.copy_(g2)
    fa.grad[off + 4100] = float("inf")                # data in a gradient buffer: nothing here faults the device
    A.step()
    for k, v in state(A).items():
        assert torch.equal(v, before[k]), k
    for k, v in buffers(ra).items():
        assert torch.equal(v, rw_before[k]), k
    assert ra.w.flat.ne(0).any() and not ra.score.flat.any() and ra.calls == 2          # the path is still pending
    assert int(A.seg_active.abs().sum()) == 0 and A.stats()["skipped_steps"] == 1
    for g in (g2, g0):
        for f, o in ((fa, A), (fb, B)):
            f.grad.copy_(g)
            o.step()
    assert_same(A, B, "after the skipped step")
    assert_same_buffers(ra, rb, "after the skipped step")
    assert ra.score.flat.gt(0).any() and not ra.w.flat.any()
    assert B.stats()["skipped_steps"] == 0


def run_language(fa, rw, A, fb, B, gs, dead):
    for step, g in enumerate(gs):
        fold = rw.scores and (rw.calls + 1) % rw.interval == 0
        if rw.scores:
            step_pair(fa, rw, A, fb, B, g, dead, f"step {step}", fold=fold)
        else:
            F_prev = rw.fisher.flat.clone()
            fa.grad.copy_(g); fb.grad.copy_(g)
            A.step(); B.step()
            assert_same(A, B, f"step {step}")
            assert torch.equal(rw.fisher.flat, fisher_rule(F_prev, g * 1.0))


def omega64(F, score, acc_prev, first, normalize=True):
    F, score = F.double(), score.double()
    mf, ms = F.max(), score.max()
    a = F / mf if normalize and mf > 0 else (F if not normalize else torch.zeros_like(F))
    b = score / ms if normalize and ms > 0 else (score if not normalize else torch.zeros_like(score))
    acc = b if first else 0.5 * (acc_prev.double() + b)
    return a + acc


def test_consolidate_matches_float64_and_the_exact_restatement_over_two_languages(grads):
    """interval=1: every step folds, so w == 0 at the end of a language, the last fold adds +0 and the score that consolidate()
    normalises is the stored one."""
    entries, gs = grads
    fa, rw, A = build(rw_kw=dict(interval=1, rw_lambda=0.5))
    fb, _, B = build(rw=False)
    dead = dead_mask(entries, fa.numel)
    run_language(fa, rw, A, fb, B, gs, dead)
    F, score = rw.fisher.flat.clone(), rw.score.flat.clone()
    rw.consolidate()
    assert torch.equal(rw.last_maxima, torch.stack([F.max(), score.max()])) and bool((rw.last_maxima > 0).all())
    err = worst_rel(rw.importance.flat, omega64(F, score, None, True))
    print("importance, first language, vs float64: worst rel", err)
    assert err <= OMEGA_TOL
    b1 = quotient(score, score.max())
    assert torch.equal(rw.score_acc.flat, b1)
    assert torch.equal(rw.importance.flat, quotient(F, F.max()) + b1)
    assert not rw.importance.flat[dead].any() and float(rw.importance.flat.max()) <= 2.0
    assert not rw.score.flat.any() and not rw.w.flat.any()
    assert torch.equal(rw.theta_star.flat, fa.theta) and torch.equal(rw.anchor.flat, fa.theta)
    assert torch.equal(rw.fisher.flat, F) and rw.tasks_consolidated == 1          # F keeps averaging through the next language
    assert_same(A, B, "consolidate() moves no weight")

    # second language: the penalised step against the plain twin fed G, one torch op per rounding
    c2 = f32(2.0 * 0.5)
    idle = [e for e in entries if e[0] == "idle"][0]
    idle_before = fa.theta[idle[1]:idle[1] + idle[2]].clone()
    for step, g in enumerate(gs[:2]):
        before, F_prev, anchor_prev, score_prev = (fa.theta.clone(), rw.fisher.flat.clone(), rw.anchor.flat.clone(),
                                                   rw.score.flat.clone())
        fa.grad.copy_(g)
        A.step()
        cw = c2 * rw.importance.flat
        d = fb.theta - rw.theta_star.flat
        pen = cw * d
        fb.grad.copy_(g * 1.0 + pen)
        fb.all_grads_live = True                      # what autograd on loss + penalty gives: every tensor has a gradient
        B.step()
        assert_same(A, B, f"penalised step {step}")
        ge = g * 1.0
        assert torch.equal(rw.fisher.flat, fisher_rule(F_prev, ge)), step           # the task gradient only
        w_new = w_rule(torch.zeros_like(ge), ge, fa.theta, before)
        assert not rw.w.flat.any() and torch.equal(rw.anchor.flat, fa.theta)
        assert worst_rel(rw.score.flat, fold64(score_prev, w_new, fa.theta, anchor_prev, rw.fisher.flat)) <= SCORE_TOL
    assert not torch.equal(fa.theta[idle[1]:idle[1] + idle[2]], idle_before)        # weight decay, zero gradient
    assert all(s == (2 if e[0] == "idle" else 5) for s, e in zip(A.seg_step.tolist(), entries))
    want = float((rw.importance.flat.double().cpu() * (fa.theta.double().cpu() - rw.theta_star.flat.double().cpu()) ** 2).sum())
    got = float(rw.penalty_value())
    assert want > 0 and abs(got - want) <= 1e-4 * want

    F2, score2, acc1 = rw.fisher.flat.clone(), rw.score.flat.clone(), rw.score_acc.flat.clone()
    rw.consolidate()
    assert torch.equal(rw.last_maxima, torch.stack([F2.max(), score2.max()]))
    err = worst_rel(rw.importance.flat, omega64(F2, score2, acc1, False))
    print("importance, second language, vs float64: worst rel", err)
    assert err <= OMEGA_TOL
    acc2 = (acc1 + quotient(score2, score2.max())) * 0.5
    assert torch.equal(rw.score_acc.flat, acc2)
    assert torch.equal(rw.importance.flat, quotient(F2, F2.max()) + acc2)
    assert rw.tasks_consolidated == 2 and torch.equal(rw.theta_star.flat, fa.theta)


def test_the_fold_inside_consolidate_is_the_fold_inside_the_step(grads):
    """Three steps, then consolidate(): with interval=3 the third step folds and consolidate() adds +0; with interval=50 nothing
    folds until consolidate() does, from the same w, theta, anchor and F."""
    entries, gs = grads
    fa, ra, A = build(rw_kw=dict(interval=3))
    fb, rb, B = build(rw_kw=dict(interval=50))
    for g in gs:
        for f, o in ((fa, A), (fb, B)):
            f.grad.copy_(g)
            o.step()
    assert ra.score.flat.gt(0).any() and not rb.score.flat.any() and rb.w.flat.ne(0).any()
    ra.consolidate(); rb.consolidate()
    assert_same_buffers(ra, rb, "after consolidate()")
    assert torch.equal(ra.last_maxima, rb.last_maxima) and float(ra.last_maxima[1]) > 0
    assert ra.importance.flat.gt(0).any()


def test_zero_maxima_give_a_zero_importance(grads):
    entries, _ = grads
    fa, rw, A = build(rw_kw=dict(interval=1))
    theta = fa.theta.clone()
    fa.grad.zero_()
    A.step()                                          # no tensor received a gradient: nothing is live
    assert torch.equal(fa.theta, theta) and not rw.fisher.flat.any() and not rw.score.flat.any()
    rw.consolidate()
    assert not rw.last_maxima.any()
    assert not rw.importance.flat.any() and not rw.score_acc.flat.any()           # 0 where the maximum is 0, not 0 / 0
    assert rw.tasks_consolidated == 1


def test_without_normalisation_the_importance_is_fisher_plus_score(grads):
    entries, gs = grads
    fa, rw, A = build(rw_kw=dict(interval=1, normalize=False))
    fb, _, B = build(rw=False)
    run_language(fa, rw, A, fb, B, gs, dead_mask(entries, fa.numel))
    F, score = rw.fisher.flat.clone(), rw.score.flat.clone()
    rw.consolidate()
    assert torch.equal(rw.last_maxima, torch.stack([F.max(), score.max()]))
    assert torch.equal(rw.score_acc.flat, score) and torch.equal(rw.importance.flat, F + score)
    assert worst_rel(rw.importance.flat, omega64(F, score, None, True, normalize=False)) <= OMEGA_TOL


def test_ewcpp_alone_importance_is_the_normalised_fisher(grads):
    entries, gs = grads
    fa, rw, A = build(rw_kw=dict(scores=False))
    fb, _, B = build(rw=False)
    dead = dead_mask(entries, fa.numel)
    run_language(fa, rw, A, fb, B, gs, dead)
    F = rw.fisher.flat.clone()
    rw.consolidate()
    assert torch.equal(rw.last_maxima, torch.stack([F.max(), torch.zeros_like(F[0])]))
    assert torch.equal(rw.importance.flat, quotient(F, F.max())) and float(rw.importance.flat.max()) == 1.0
    assert not rw.importance.flat[dead].any() and torch.equal(rw.theta_star.flat, fa.theta) and torch.equal(rw.fisher.flat, F)
    c2 = f32(2.0)                                     # rw_lambda = 1; the second step's penalty is not zero
    for step, g in enumerate(gs[:2]):
        F_prev = rw.fisher.flat.clone()
        fa.grad.copy_(g)
        A.step()
        cw = c2 * rw.importance.flat
        d = fb.theta - rw.theta_star.flat
        pen = cw * d
        fb.grad.copy_(g * 1.0 + pen)
        fb.all_grads_live = True
        B.step()
        assert_same(A, B, f"penalised EWC++ step {step}")
        assert torch.equal(rw.fisher.flat, fisher_rule(F_prev, g * 1.0))
    assert pen.ne(0).any()


def test_parameter_groups_move_every_tensor_as_its_own_groups_rule(grads):
    from indic_cl_asr_amd import cl
    entries, gs = grads
    hyper, g1 = [(1e-3, 1e-2), (1e-4, 0.0)], ["v5", "v6", "v7", "v8", "v9", "idle"]

    def one(grouped, k=0):
        flat = cl.FlatParams(Toy(big=False).cuda())
        rw = cl.RWalk(flat, alpha=ALPHA, eps=EPS, interval=2, normalize=False)    # a global maximum would couple the groups
        kw = dict(param_groups=[dict(params=g1, lr=hyper[1][0], weight_decay=hyper[1][1])]) if grouped else {}
        opt = cl.FusedAdamW(flat, lr=hyper[k][0], weight_decay=hyper[k][1], path_integral=rw, **kw)
        for step, g in enumerate(gs + gs[:1]):        # folds at calls 2 and 4; consolidated after call 3: call 4 is penalised
            if step == 3:
                rw.consolidate()
            flat.grad.copy_(g)
            opt.step()
        return dict(state(opt), **buffers(rw)), opt.seg_step.tolist()

    (G, steps_g), singles = one(True), [one(False, 0), one(False, 1)]
    for seg, (name, off, k, _) in enumerate(entries):
        U, steps_u = singles[1 if name in g1 else 0]
        for key in G:
            if key != "seg_step":
                assert torch.equal(G[key][off:off + k], U[key][off:off + k]), (name, key)
        assert steps_g[seg] == steps_u[seg], name
    assert not torch.equal(singles[0][0]["theta"], singles[1][0]["theta"])


def test_resume_reproduces_five_uninterrupted_steps(grads):
    from indic_cl_asr_amd import cl
    entries, gs = grads
    seq = [gs[0], gs[1], gs[2], gs[0], gs[2]]
    fu, ru, U = build(rw_kw=dict(interval=2))
    for g in seq:
        fu.grad.copy_(g)
        U.step()
    fa, ra, A = build(rw_kw=dict(interval=2))
    for g in seq[:3]:
        fa.grad.copy_(g)
        A.step()
    assert ra.w.flat.ne(0).any() and ra.calls == 3                  # saved between two folds: the pending path travels
    sd_opt, sd_rw, theta = A.state_dict(), ra.state_dict(), fa.theta.cpu().clone()
    assert all(not v.is_cuda for v in sd_rw.values() if torch.is_tensor(v))
    f2 = cl.FlatParams(Toy(big=False).cuda())
    f2.theta.copy_(theta)
    r2 = cl.RWalk(f2, alpha=0.5, eps=1.0, interval=7)               # hyper-parameters come from the saved state
    R = cl.FusedAdamW(f2, lr=5.0, path_integral=r2)
    R.load_state_dict(sd_opt)
    r2.load_state_dict(sd_rw)
    assert (r2.alpha, r2.eps, r2.interval, r2.calls) == (ALPHA, EPS, 2, 3)
    for g in seq[3:]:
        f2.grad.copy_(g)
        R.step()
    for k in ("theta", "exp_avg", "exp_avg_sq", "seg_step"):
        assert torch.equal(state(R)[k], state(U)[k]), k
    assert_same_buffers(r2, ru, "resumed")
    assert r2.calls == ru.calls == 5 and ru.score.flat.gt(0).any()


def test_through_the_model_two_steps_then_a_penalised_one():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny')).cuda().train()
    freeze_layer(m, 0)
    flat = cl.FlatParams(m)
    rw = cl.RWalk(flat, alpha=ALPHA, eps=EPS, interval=2)
    opt = cl.FusedAdamW(flat, lr=1e-3, path_integral=rw)
    batch, langs = _batch(['hi'] * 4, seed=1)
    for step in range(2):
        opt.zero_grad()
        loss, monitor = m.training_step(batch, langs, compute_wer=False)
        loss.backward()
        g, before, F_prev, w_prev = flat.grad.clone(), flat.theta.clone(), rw.fisher.flat.clone(), rw.w.flat.clone()
        opt.step()
        assert torch.equal(rw.fisher.flat, fisher_rule(F_prev, g * 1.0))
        if step == 0:
            assert torch.equal(rw.w.flat, w_rule(w_prev, g * 1.0, flat.theta, before)) and rw.w.flat.ne(0).any()
    assert monitor['train_loss'] == monitor['train_loss'] and not rw.w.flat.any() and rw.score.flat.gt(0).any()
    assert float(rw.penalty_value()) == 0.0
    rw.consolidate()
    for name, view in rw.importance.items():
        if ".ta." in name:
            assert not view.any(), name
    assert any(view.gt(0).any() for name, view in rw.importance.items() if ".hi." in name)
    assert any(".ta." in n for n in rw.importance) and bool((rw.importance.flat >= 0).all())
    assert float(rw.importance.flat.max()) <= 2.0 and bool((rw.last_maxima > 0).all())
    batch, langs = _batch(['ta'] * 4, seed=2)
    opt.zero_grad()
    loss, monitor = m.training_step(batch, langs, compute_wer=False)
    loss.backward()
    opt.step()
    assert float(rw.penalty_value()) > 0.0 and 'train_loss' in monitor
    assert all(s >= 1 for s in opt.seg_step.tolist())     # with the penalty every tensor is live, the `hi` heads included
