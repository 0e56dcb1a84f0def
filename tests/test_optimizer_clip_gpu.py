"""FusedAdamW's on-device gradient clipping, non-finite skip and resumable state (ia_grad_norm,
ia_adamw_step_segmented_clipped) on a toy module whose tensor sizes hit every path of the flat kernels: a tail shorter than
a float4, the 64-float alignment gaps, a chunk boundary (4096), the bf16 shadow views of a 2-D tensor, and a tensor of more
than 2048 chunks so that the grid-stride loop of the 2048-workgroup launches runs twice.

References are float64 on the CPU: the norms from the definition, the clipped first moment from 0.1 * g * coef.  The clip
itself is checked bit for bit against the unclipped optimizer fed the same gradient multiplied by the reported coefficient
(Adam's step is nearly invariant to the gradient's scale, so the weights alone would not show a missing clip).

Norm bound 2e-6 relative: every term of a sum of squares is positive, a chunk's fp32 sum sits under at most 17 roundings
(4 inside x*x + y*y + z*z + w*w, 4 for a thread's four float4, 6 for the wave sum, 3 for the four waves; the squares add one
more on each term) before the fp64 finish -- 18 * 2^-24 = 1.1e-6 on the sum, half of that on the root, plus the final
fp32 rounding of the root and of the scale product (2 * 6e-8): below 1e-6, inside the stated 2e-6."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 5]
BIG = 2049 * 4096 + 1
TOL = 2e-6


class Toy(torch.nn.Module):
    def __init__(self, big=True):
        super().__init__()
        g = torch.Generator().manual_seed(11)
        for i, n in enumerate(SIZES):
            setattr(self, f"v{i}", torch.nn.Parameter(torch.randn(n, generator=g)))
        self.mat = torch.nn.Parameter(torch.randn(65, 63, generator=g))
        self.idle = torch.nn.Parameter(torch.randn(130, generator=g))      # never receives a gradient
        if big:
            self.big = torch.nn.Parameter(torch.randn(BIG, generator=g))


def make_grad(entries, numel, seed, scale=3.0):
    """Flat CPU gradient: seeded randn * scale inside every tensor but `idle`, zero in the alignment gaps."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(numel)
    for name, off, k, _ in entries:
        if name != "idle":
            flat[off:off + k] = torch.randn(k, generator=g) * scale
    return flat


def norms64(entries, flat_cpu):
    per = {name: flat_cpu[off:off + k].double().norm().item() for name, off, k, _ in entries}
    return per, sum(v * v for v in per.values()) ** 0.5


def build(**kw):
    from indic_cl_asr_amd import cl
    m = Toy().cuda()
    flat = cl.FlatParams(m)
    return m, flat, cl.FusedAdamW(flat, lr=1e-3, **kw)


def state(opt):
    return {"theta": opt.flat.theta, "exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq, "seg_step": opt.seg_step,
            "shadow": opt.shadow}


def assert_same(a, b, what):
    sa, sb = state(a), state(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), (what, k)


@pytest.fixture(scope="module")
def grads():
    """Three gradients shared by the tests (never modified): two at norm ~ 8.7e3 and one far below the threshold of 1."""
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy())
    e, n = list(flat.entries), flat.numel
    return e, [make_grad(e, n, 101), make_grad(e, n, 102, scale=1e-5), make_grad(e, n, 103)]


def rel(a, b):
    return abs(a - b) / abs(b)


def test_norm_and_coefficient_match_float64(grads):
    entries, (g, _, _) = grads
    per64, total64 = norms64(entries, g)
    m, flat, opt = build(max_grad_norm=1.0)
    flat.grad.copy_(g)
    opt.step()
    st = opt.stats()
    per = opt.grad_norms()
    print("grad_norm", st["grad_norm"], "float64", total64, "rel", rel(st["grad_norm"], total64))
    print("clip_coef", st["clip_coef"], "float64", 1.0 / (total64 + 1e-6), "rel", rel(st["clip_coef"], 1.0 / (total64 + 1e-6)))
    worst = max((rel(per[n], per64[n]), n) for n in per64 if n != "idle")
    print("worst per-tensor rel", worst)
    assert rel(st["grad_norm"], total64) <= TOL
    assert float(opt.last_grad_norm) == st["grad_norm"]
    assert rel(st["clip_coef"], 1.0 / (total64 + 1e-6)) <= TOL
    assert set(per) == set(per64)
    for n in per64:
        if n == "idle":
            assert per[n] == 0.0
        else:
            assert rel(per[n], per64[n]) <= TOL, (n, per[n], per64[n])
    assert st["clipped_steps"] == 1 and st["skipped_steps"] == 0


def test_clip_is_applied_bit_for_bit(grads):
    entries, gs = grads
    _, fa, A = build(max_grad_norm=1.0)
    _, fb, B = build()
    assert torch.equal(fa.theta, fb.theta)
    for step, g in enumerate(gs):
        gd = g.cuda()
        fa.grad.copy_(gd)
        A.step()
        st = A.stats()
        coef = torch.tensor(st["clip_coef"], dtype=torch.float32, device="cuda")
        assert float(coef) == st["clip_coef"]
        fb.grad.copy_(gd * coef)          # fp32 product on the device: torch's g.mul_(coef)
        B.step()
        assert_same(A, B, f"step {step}")
        if step == 0:
            _, total64 = norms64(entries, g)
            want = 0.1 * g.double() * (1.0 / (total64 + 1e-6))
            got = A.exp_avg.double().cpu()
            err = ((got - want).abs() / want.abs().clamp_min(1e-300)).max().item()
            print("exp_avg vs 0.1*g64*coef64: worst rel", err)
            assert torch.allclose(got, want, rtol=1e-6, atol=0.0)
        if step == 1:                     # norm ~ 0.03 < 1: not clipped
            assert st["clip_coef"] == 1.0 and st["clipped_steps"] == 1
    assert A.stats()["clipped_steps"] == 2
    idle = [i for i, e in enumerate(entries) if e[0] == "idle"][0]
    steps = A.seg_step.tolist()
    assert steps[idle] == 0 and all(s == 3 for i, s in enumerate(steps) if i != idle)


def test_norm_is_deterministic(grads):
    _, (g, _, _) = grads
    _, f1, o1 = build(track_grad_norm=True)
    _, f2, o2 = build(track_grad_norm=True)
    f1.grad.copy_(g); f2.grad.copy_(g)
    o1.step(); o2.step()
    a, b = o1.last_grad_norm.clone(), o2.last_grad_norm.clone()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(o1._seg_norm.view(torch.int32), o2._seg_norm.view(torch.int32))
    assert o1.stats()["clip_coef"] == 1.0 and o1.stats()["clipped_steps"] == 0      # measure only


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_nonfinite_gradient_skips_the_step(grads, bad):
    entries, (g0, _, g2) = grads
    _, fa, A = build(max_grad_norm=1.0, skip_nonfinite=True)
    _, fb, B = build(max_grad_norm=1.0, skip_nonfinite=True)      # the twin that never sees the bad step
    for f, o in ((fa, A), (fb, B)):
        f.grad.copy_(g0)
        o.step()
    before = {k: v.clone() for k, v in state(A).items()}
    off = [e for e in entries if e[0] == "v9"][0][1]
    fa.grad.copy_(g2)
    fa.grad[off + 4100] = bad             # data in a gradient buffer: nothing here faults the device
    A.step()
    for k, v in state(A).items():
        assert torch.equal(v, before[k]), k
    assert int(A.seg_active.abs().sum()) == 0
    st = A.stats()
    assert st["skipped_steps"] == 1 and st["clipped_steps"] == 1
    assert not (st["grad_norm"] - st["grad_norm"] == 0.0)          # inf or NaN is what was measured
    for f, o in ((fa, A), (fb, B)):
        f.grad.copy_(g2)
        o.step()
    assert_same(A, B, "after the skipped step")
    assert A.stats()["skipped_steps"] == 1 and B.stats()["skipped_steps"] == 0
    assert A.stats()["clipped_steps"] == B.stats()["clipped_steps"] == 2


def test_defaults_are_the_plain_step(grads):
    entries, (g0, _, g2) = grads
    m, fa, A = build()
    _, fb, B = build(track_grad_norm=True)                          # measures, multiplies by coef == 1
    ref = [torch.nn.Parameter(p.detach().double().cpu().clone()) for p in fa.params]
    ref_opt = torch.optim.AdamW(ref, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    st = A.stats()
    assert st["clipped_steps"] == 0 and st["skipped_steps"] == 0 and st["clip_coef"] == 1.0
    assert st["grad_norm"] != st["grad_norm"]                       # NaN: nothing measured
    for g in (g0, g2):
        fa.grad.copy_(g); fb.grad.copy_(g)
        A.step(); B.step()
        for (name, off, k, shape), p in zip(entries, ref):
            p.grad = None if name == "idle" else g[off:off + k].double().view(shape)
        ref_opt.step()
    assert_same(A, B, "default vs measure-only")
    st = A.stats()
    assert st["clipped_steps"] == 0 and st["skipped_steps"] == 0 and st["grad_norm"] != st["grad_norm"]
    # torch.optim.AdamW in float64: per step the fp32 kernel rounds the decay factor 1 - lr * wd, the decayed weight and the
    # updated weight (2 steps: 6 roundings of at most 2^-24 |theta|); the update itself (lr = 1e-3 times a quotient of
    # magnitude <= 1 with a relative fp32 error of ~1e-6) adds ~1e-9 per step
    for (name, off, k, shape), p in zip(entries, ref):
        got = fa.theta[off:off + k].double().cpu().view(shape)
        atol = 6 * 2.0 ** -24 * float(p.detach().abs().max()) + 1e-8
        assert torch.allclose(got, p.detach(), rtol=0.0, atol=atol), name


def test_state_dict_resumes_bit_for_bit(grads):
    from indic_cl_asr_amd import cl
    entries, gs = grads
    seq = [gs[0], gs[1], gs[2], gs[0]]
    _, fu, U = build(max_grad_norm=1.0, skip_nonfinite=True)        # 4 uninterrupted steps
    for g in seq:
        fu.grad.copy_(g)
        U.step()
    _, fa, A = build(max_grad_norm=1.0, skip_nonfinite=True)
    for g in seq[:2]:
        fa.grad.copy_(g)
        A.step()
    sd = A.state_dict()
    assert all(not v.is_cuda for v in sd.values() if torch.is_tensor(v))
    theta = fa.theta.cpu().clone()
    m2 = Toy().cuda()
    f2 = cl.FlatParams(m2)
    f2.theta.copy_(theta)
    R = cl.FusedAdamW(f2, lr=5.0)                                   # hyper-parameters come from the saved state
    R.load_state_dict(sd)
    assert R.param_groups[0]["lr"] == 1e-3 and R.param_groups[0]["max_grad_norm"] == 1.0
    for g in seq[2:]:
        f2.grad.copy_(g)
        R.step()
    for k in ("theta", "exp_avg", "exp_avg_sq", "seg_step"):
        assert torch.equal(state(R)[k], state(U)[k]), k
    su, sr = U.stats(), R.stats()
    assert (sr["clipped_steps"], sr["skipped_steps"]) == (su["clipped_steps"], su["skipped_steps"]) == (3, 0)
    assert R.step_count == U.step_count == 4
