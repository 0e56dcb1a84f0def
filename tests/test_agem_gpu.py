"""Averaged GEM inside the fused optimizer step (ia_agem_dots, ia_grad_norm_projected, ia_adamw_step_segmented_projected) on the
toy module of tests/test_optimizer_clip_gpu.py, whose tensor sizes reach every path of the flat kernels (a tail shorter than a
float4, the alignment gaps, the 4096 chunk boundary, the 2-D shadow view, the idle tensor and -- `big=True`, first test only --
more than 2048 chunks), and once through the model.

The definitions (include/indicasr.h), per element of a live tensor, each product and difference rounded to fp32 on its own:
    ge = g * grad_scale;  gp = violated ? ge - alpha * r : ge;  G = gp * coef (when clipping);  theta' = AdamW(theta, G)
so the step is checked bit for bit against the plain optimizer fed G built with one torch op per rounding from the reported
alpha.  Only the reductions have tolerances, against float64 on the CPU:
  ref_sq   2e-6 relative: the sum-of-squares bound derived in tests/test_optimizer_clip_gpu.py (18 roundings of 2^-24).
  dot      |dot - dot64| <= 2e-6 * sum |g_i r_i|: the same 18 roundings, against the sum of magnitudes because the terms cancel.
  alpha    5e-6 relative of dot64 / ref_sq64.
  norm     2e-6 relative of the float64 norm of the projected gradient (the fp32 G the step consumed).
The references are g = make_grad(101) and r = make_grad(104) -/+ 0.5 g: their float64 dots are about -/+ 0.5 |g|^2, which the
tests assert to be at least a thousand times the dot's error bound, so the sign of the decision is never in doubt.
Orthogonality: G = g - alpha * r has G.r = 0 exactly; alpha carries a relative error of at most 5e-6, which leaves
|G.r| <= 5e-6 * |dot| <= 5e-6 |g||r|, and |G| >= |g| / 2 here (|alpha r| is below |g| / 2: asserted), so |G.r| <= 1e-5 |G||r|.
Observed on an MI355X: dot at 0.010 (big: 0.016) of its bound, ref_sq 4.4e-8, alpha 3.9e-8, norm 3.5e-8, |G.r| / (|G||r|) 3e-8."""
import copy

import pytest
import torch

from test_optimizer_clip_gpu import Toy, assert_same, make_grad, norms64, state

pytestmark = pytest.mark.gpu

TOL = 2e-6
KEYS = {"dot", "ref_sq", "alpha", "projected", "projected_steps"}


def build(big=False, agem=True, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    a = cl.AveragedGEM(flat) if agem else None
    return flat, a, cl.FusedAdamW(flat, lr=1e-3, projection=a, **kw)


def make_inputs(big, g_seed=101, r_seed=104):
    """entries, g, the opposing and the agreeing reference as fp32 device tensors."""
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big))
    e, n = list(flat.entries), flat.numel
    g, noise = make_grad(e, n, g_seed), make_grad(e, n, r_seed)
    return e, g.cuda(), (noise - 0.5 * g).cuda(), (noise + 0.5 * g).cuda()


@pytest.fixture(scope="module")
def inputs():
    """Toy(big=False): (entries, g, opposing r, agreeing r), never modified."""
    return make_inputs(big=False)


def step_with(flat, agem, opt, g, r, **kw):
    """What the training loop does: the memory batch's gradient becomes the reference, then the task gradient is stepped."""
    if r is not None:
        flat.grad.copy_(r)
        agem.store_reference(opt)
        assert not flat.grad.any() and agem.has_reference
    flat.grad.copy_(g)
    opt.step(**kw)


def f32(x):
    return torch.tensor(x, dtype=torch.float32, device="cuda")


def projected(g, r, alpha, scale=1.0):
    """g * scale - alpha * r with one fp32 torch op per rounding."""
    ge = g * f32(scale)
    ar = f32(alpha) * r
    return ge - ar


def rel(a, b):
    return abs(a - b) / abs(b)


def check_dots(st, g, r, scale):
    g64, r64 = g.double().cpu(), r.double().cpu()
    dot64, mag64, rr64 = scale * float(g64 @ r64), scale * float(g64.abs() @ r64.abs()), float(r64 @ r64)
    print("dot", st["dot"], "float64", dot64, "err / bound", abs(st["dot"] - dot64) / (TOL * mag64))
    print("ref_sq", st["ref_sq"], "float64", rr64, "rel", rel(st["ref_sq"], rr64))
    print("alpha", st["alpha"], "float64", dot64 / rr64, "rel", rel(st["alpha"], dot64 / rr64))
    assert dot64 < 0 and abs(dot64) > 1000 * TOL * mag64            # the margin of the decision
    assert rel(st["ref_sq"], rr64) <= TOL
    assert abs(st["dot"] - dot64) <= TOL * mag64
    assert rel(st["alpha"], dot64 / rr64) <= 5e-6
    assert st["projected"] == 1 and st["projected_steps"] == 1 and set(st) == KEYS


def test_dots_match_float64_and_reproduce():
    entries, g, opp, _ = make_inputs(big=False)
    fa, aa, A = build()
    fb, ab, B = build()
    step_with(fa, aa, A, g, opp)
    step_with(fb, ab, B, g, opp)
    check_dots(aa.stats(), g, opp, 1.0)
    assert torch.equal(aa.proj_state.view(torch.int32), ab.proj_state.view(torch.int32))
    assert_same(A, B, "two optimizers, same inputs")
    del fa, aa, A, fb, ab, B
    entries, g, opp, _ = make_inputs(big=True)                      # > 2048 chunks: the grid-stride loops run twice
    fa, aa, A = build(big=True)
    fb, ab, B = build(big=True)
    step_with(fa, aa, A, g, opp, grad_scale=0.5)
    step_with(fb, ab, B, g, opp, grad_scale=0.5)
    check_dots(aa.stats(), g, opp, 0.5)
    assert torch.equal(aa.proj_state.view(torch.int32), ab.proj_state.view(torch.int32))
    assert_same(A, B, "two optimizers, same inputs, big")


def test_projection_is_applied_bit_for_bit():
    fa, agem, A = build()
    fb, _, B = build(agem=False)
    for step, (g_seed, r_seed) in enumerate(((101, 104), (103, 105), (107, 106))):
        entries, g, opp, _ = make_inputs(False, g_seed, r_seed)
        step_with(fa, agem, A, g, opp)
        st = agem.stats()
        assert st["projected"] == 1 and st["alpha"] < 0 and float(f32(st["alpha"])) == st["alpha"]
        G = projected(g, opp, st["alpha"])
        fb.grad.copy_(G)
        B.step()
        assert_same(A, B, f"step {step}")
        G64, r64, g64 = g.double().cpu() - st["alpha"] * opp.double().cpu(), opp.double().cpu(), g.double().cpu()
        cos = abs(float(G64 @ r64)) / (float(G64.norm()) * float(r64.norm()))
        print("step", step, "alpha", st["alpha"], "|G.r| / (|G||r|)", cos)
        assert abs(st["alpha"]) * float(r64.norm()) < 0.5 * float(g64.norm())
        assert cos <= 1e-5
    assert agem.stats()["projected_steps"] == 3
    idle = [i for i, e in enumerate(entries) if e[0] == "idle"][0]
    steps = A.seg_step.tolist()
    assert steps[idle] == 0 and all(s == 3 for i, s in enumerate(steps) if i != idle)


def test_agreeing_reference_is_the_plain_step(inputs):
    entries, g, _, agree = inputs
    fa, agem, A = build()
    fb, _, B = build(agem=False)
    assert not agem.has_reference
    for what, r in (("no reference", None), ("agreeing reference", agree), ("cleared", None)):
        if what == "cleared":
            agem.clear()
            assert not agem.has_reference
        step_with(fa, agem, A, g, r)
        fb.grad.copy_(g)
        B.step()
        assert_same(A, B, what)
        st = agem.stats()
        assert st["projected"] == 0 and st["alpha"] == 0.0 and st["projected_steps"] == 0 and set(st) == KEYS
        if what == "agreeing reference":
            g64, r64 = g.double().cpu(), agree.double().cpu()
            assert st["dot"] > 0 and abs(st["dot"] - float(g64 @ r64)) <= TOL * float(g64.abs() @ r64.abs())


def test_projection_then_clipping(inputs):
    entries, g, opp, agree = inputs
    fa, agem, A = build(max_grad_norm=1.0)
    fb, _, B = build(agem=False)
    step_with(fa, agem, A, g, opp)
    st, ps = A.stats(), agem.stats()
    assert ps["projected"] == 1 and ps["projected_steps"] == 1 and st["clipped_steps"] == 1
    G = projected(g, opp, ps["alpha"], 1.0)
    _, want = norms64(entries, G.cpu())
    _, plain = norms64(entries, g.cpu())
    print("grad_norm", st["grad_norm"], "float64 of the projected gradient", want, "rel", rel(st["grad_norm"], want),
          "float64 of g", plain)
    assert rel(st["grad_norm"], want) <= TOL
    assert rel(st["grad_norm"], plain) > TOL
    assert rel(st["clip_coef"], 1.0 / (want + 1e-6)) <= TOL
    per = A.grad_norms()
    assert per["idle"] == 0.0
    coef = f32(st["clip_coef"])
    assert float(coef) == st["clip_coef"]
    fb.grad.copy_(G * coef)
    B.step()
    assert_same(A, B, "projected, then clipped")
    # the agreeing reference: a clipped optimizer without projection, the measured norm included
    fc, agem_c, C = build(max_grad_norm=1.0)
    fd, _, D = build(agem=False, max_grad_norm=1.0)
    step_with(fc, agem_c, C, g, agree)
    fd.grad.copy_(g)
    D.step()
    assert_same(C, D, "agreeing reference, clipped")
    assert torch.equal(C.last_grad_norm.clone().view(torch.int32), D.last_grad_norm.clone().view(torch.int32))
    assert torch.equal(C._seg_norm.view(torch.int32), D._seg_norm.view(torch.int32))
    assert C.stats() == D.stats() and C.stats()["clipped_steps"] == 1
    assert agem_c.stats()["projected_steps"] == 0


def test_liveness_and_degenerate_references(inputs):
    entries, g, opp, _ = inputs
    _, off, k, _ = [e for e in entries if e[0] == "idle"][0]
    idle_seg = [i for i, e in enumerate(entries) if e[0] == "idle"][0]
    # r is non-zero inside `idle`, where the task gradient is zero: the tensor stays untouched, r.r still counts it
    r = opp.clone()
    r[off:off + k] = torch.randn(k, generator=torch.Generator().manual_seed(9)).cuda() * 30.0
    fa, agem, A = build()
    fb, _, B = build(agem=False)
    idle_before = fa.theta[off:off + k].clone()
    step_with(fa, agem, A, g, r)
    st = agem.stats()
    rr64, rr64_live = float(r.double().cpu() @ r.double().cpu()), float(opp.double().cpu() @ opp.double().cpu())
    assert st["projected"] == 1 and rel(st["ref_sq"], rr64) <= TOL and rel(st["ref_sq"], rr64_live) > 100 * TOL
    G = projected(g, r, st["alpha"])
    assert G[off:off + k].any()
    G[off:off + k] = 0                                              # the twin's `.grad is None`
    fb.grad.copy_(G)
    B.step()
    assert_same(A, B, "r inside idle")
    assert torch.equal(fa.theta[off:off + k], idle_before) and int(A.seg_step[idle_seg]) == 0
    assert not A.exp_avg[off:off + k].any() and not A.exp_avg_sq[off:off + k].any()
    # r == 0 everywhere: no projection, no NaN, the plain step
    fa, agem, A = build()
    fb, _, B = build(agem=False)
    step_with(fa, agem, A, g, torch.zeros_like(g))
    fb.grad.copy_(g)
    B.step()
    assert_same(A, B, "zero reference")
    st = agem.stats()
    assert st == {"dot": 0.0, "ref_sq": 0.0, "alpha": 0.0, "projected": 0, "projected_steps": 0}
    assert all(bool(torch.isfinite(v.float()).all()) for v in state(A).values())


def test_nonfinite_step_is_skipped_and_not_counted():
    _, g0, r0, _ = make_inputs(False, 101, 104)
    entries, g2, r2, _ = make_inputs(False, 103, 105)
    fa, aa, A = build(skip_nonfinite=True)
    fb, ab, B = build(skip_nonfinite=True)                          # the twin that never sees the bad step
    for f, a, o in ((fa, aa, A), (fb, ab, B)):
        step_with(f, a, o, g0, r0)
    before = {k: v.clone() for k, v in state(A).items()}
    off = [e for e in entries if e[0] == "v9"][0][1]
    bad = g2.clone()
    bad[off + 4100] = float("inf")                                  # data in a gradient buffer: nothing here faults the device
    step_with(fa, aa, A, bad, r2)
    for k, v in state(A).items():
        assert torch.equal(v, before[k]), k
    assert int(A.seg_active.abs().sum()) == 0
    st = aa.stats()
    assert A.stats()["skipped_steps"] == 1 and st["projected_steps"] == 1 and st["projected"] == 0 and st["alpha"] == 0.0
    for f, a, o in ((fa, aa, A), (fb, ab, B)):
        step_with(f, a, o, g2, r2)
    assert_same(A, B, "after the skipped step")
    assert aa.stats()["projected_steps"] == ab.stats()["projected_steps"] == 2
    assert A.stats()["skipped_steps"] == 1 and B.stats()["skipped_steps"] == 0


def test_errors():
    from indic_cl_asr_amd import _lib, cl
    flat = cl.FlatParams(Toy(big=False).cuda())
    other = cl.FlatParams(Toy(big=False).cuda())
    with pytest.raises(ValueError):
        cl.FusedAdamW(flat, projection=cl.AveragedGEM(flat), path_integral=cl.SynapticIntelligence(flat))
    with pytest.raises(ValueError):
        cl.FusedAdamW(flat, projection=cl.AveragedGEM(other))
    L = _lib.lib()
    assert L.ia_agem_workspace_bytes(7) == 7 * 2 * 4
    # argument validation happens before any device work: null pointers -> IA_INVALID_VALUE (-1)
    assert L.ia_agem_dots(None, None, None, 1, 1, 1.0, None, None, None, 0, None) == -1
    assert L.ia_grad_norm_projected(None, None, 1, None, 1, 1.0, 0.0, None, None, None, None, 0, None, None, None) == -1
    assert L.ia_adamw_step_segmented_projected(None, None, None, None, None, 1, None, None, 1, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-2,
                                               1.0, None, None, 0, None, None, None, None, None) == -1
    # a short workspace is refused as the neighbouring entry points refuse it
    agem = cl.AveragedGEM(flat)
    n = flat.chunk_table.shape[0]
    ws = agem.workspace(n)
    assert L.ia_agem_dots(_lib.ptr(flat.grad), _lib.ptr(agem.ref.flat), _lib.ptr(flat.chunk_table), n, len(flat.entries), 1.0, None,
                          _lib.ptr(agem.proj_state), _lib.ptr(ws), ws.numel() - 1, _lib.stream_ptr()) == -2


def _batch(langs, seed, B=4, L=16000, U=6):
    g = torch.Generator().manual_seed(seed)
    sl = torch.tensor([L] + [int(L * (0.55 + 0.45 * torch.rand(1, generator=g))) for _ in range(B - 1)])
    sig = torch.randn(B, L, generator=g) * 0.1
    for i in range(B):
        sig[i, sl[i]:] = 0
    tl = torch.tensor([U] + [int(torch.randint(1, U + 1, (1,), generator=g)) for _ in range(B - 1)])
    tr = torch.randint(0, 16, (B, U), generator=g)
    return tuple(t.cuda() for t in (sig, sl, tr, tl)), langs


def test_through_the_model_with_an_episodic_memory():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny')).cuda().train()
    freeze_layer(m, 0)
    twin = copy.deepcopy(m)                                         # only its weights are used: it is fed gradients
    flat, flat_b = cl.FlatParams(m), cl.FlatParams(twin)
    assert flat.entries == flat_b.entries and torch.equal(flat.theta, flat_b.theta)
    agem = cl.AveragedGEM(flat)
    opt = cl.FusedAdamW(flat, lr=1e-3, projection=agem)
    B = cl.FusedAdamW(flat_b, lr=1e-3)
    memory = cl.EpisodicMemory(per_language=4, seed=0)

    hi, hi_langs = _batch(['hi'] * 4, seed=1)
    for _ in range(2):                                              # task `hi`: nothing to project on yet
        opt.zero_grad()
        loss, _ = m.training_step(hi, hi_langs, compute_wer=False)
        loss.backward()
        flat_b.grad.copy_(flat.grad)
        opt.step(); B.step()
        assert_same(opt, B, "task hi")
    assert agem.stats()["projected_steps"] == 0
    memory.add(hi, hi_langs)
    assert len(memory) == 4 and memory.languages() == ['hi']

    ta, ta_langs = _batch(['ta'] * 4, seed=2)
    for step in range(2):                                           # task `ta`
        opt.zero_grad()
        mb, ml = memory.sample(4, "cuda")
        assert ml == ['hi'] * 4
        loss, _ = m.training_step(mb, ml, compute_wer=False)
        loss.backward()
        mem_grad = flat.grad.clone()
        assert mem_grad.any()
        agem.store_reference(opt)
        assert torch.equal(agem.ref.flat, mem_grad) and not flat.grad.any()
        loss, _ = m.training_step(ta, ta_langs, compute_wer=False)
        loss.backward()
        g, before = flat.grad.clone(), flat.theta.clone()
        r = mem_grad
        if step == 1 and float(g.double() @ r.double()) > 0:        # whatever the data gave, the last step has to project
            agem.ref.flat.neg_()
            r = -mem_grad
        opt.step()
        st = agem.stats()
        assert set(st) == KEYS
        print("step", step, st)
        assert st["projected"] == int(st["dot"] < 0) and (step == 0 or st["projected"] == 1)
        G = projected(g, r, st["alpha"]) if st["projected"] else g * 1.0
        hi_heads = 0
        for name, off, k, _ in flat.entries:                        # `.grad is None` where the task gave no gradient
            if not g[off:off + k].any():
                G[off:off + k] = 0
                assert torch.equal(flat.theta[off:off + k], before[off:off + k]), name
            if ".hi." in name:                                      # the memory's language: r is non-zero there, g is not
                hi_heads += int(bool(mem_grad[off:off + k].any()))
                assert not g[off:off + k].any(), name
                assert torch.equal(flat.theta[off:off + k], before[off:off + k]), name
        assert hi_heads > 0
        flat_b.grad.copy_(G)
        B.step()
        assert_same(opt, B, f"task ta, step {step}")
    assert agem.stats()["projected_steps"] >= 1
