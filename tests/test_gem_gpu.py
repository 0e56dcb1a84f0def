"""GEM inside the fused optimizer step (ia_gem_dots, ia_gem_solve, ia_grad_norm_gem, ia_adamw_step_segmented_gem) on the toy
module of tests/test_optimizer_clip_gpu.py, whose tensor sizes reach every path of the flat kernels (a tail shorter than a float4,
the alignment gaps, the 4096 chunk boundary, the 2-D shadow view, the idle tensor and -- `big=True`, first test only -- more than
2048 chunks), and once through the model.

The definition (include/indicasr.h): d_k = s <g, r_k>, P = R R' + eps I, v = argmin 1/2 v'Pv + d'v subject to v >= gamma when
some d_k < 0, and per element of a live tensor, each product and sum rounded to fp32 on its own,
    acc = g * s;  for k ascending with v_k != 0: acc = acc + v_k * r_k;  G = acc * coef (when clipping);  theta' = AdamW(theta, G)
so the step is checked bit for bit against the plain optimizer fed G built with one torch op per rounding from the reported v.

Inputs.  g = make_grad(seed) and r_k = make_grad(seed_k) -/+ 0.5 g: an opposing row has d_k ~ -0.5 |g|^2, an agreeing one
+0.5 |g|^2, the Gram matrix is ~ |g|^2 (1.25 I + 0.25 (ss' - I)) for the sign vector s.  In these units the free minimiser of an
opposing row is 0.5 / (1 + 0.25 K) <= 0.4, below the default memory_strength of 0.5, where every v_k would sit at the bound; the
tests therefore run at GAMMA = 0.1, which leaves the opposing rows free (v_k > gamma, the issue's "active") and the agreeing
ones at the bound (v_k == gamma): `reference` asserts in float64 that both kinds occur (K >= 2), that some d_k is negative by a
thousand times the dot's error bound, and cond(P) <= 1e6.  gamma and eps are the fp32 values the kernel receives.

Tolerances, all against float64 on the CPU:
  dots, Gram  |d_k - d64_k| <= 2e-6 s sum_i |g_i r_ki|, Gram entries against sum_i |r_ji r_ki|: the bound of this reduction shape
              derived in tests/test_optimizer_clip_gpu.py (18 roundings of 2^-24), against the sum of magnitudes.
  solver      max |v - v64| <= 2^-22 max |v64|, v64 from the values the device reported for d and the Gram matrix (tests/
              test_gem_host.py's enumerator for K <= 5; for K = 16 the two free coordinates are known by construction, the 2 x 2
              system is solved in float64 and its KKT conditions asserted).  The device solves in fp64 at cond <= 1e6 (~1e-9)
              and rounds once to fp32 (6e-8): the bound leaves 4x over the rounding.
  KKT         v >= gamma exactly; lambda = Pv + d >= -tol and |(v_k - gamma) lambda_k| <= tol with
              tol = 2^-22 max_k sum_j |P_kj| |v_j|: what rounding v to fp32 moves lambda by, with the same 4x.
  norm        2e-6 relative of the float64 norm of the fp32 G the step consumed.
  feasibility <G64, r_k> >= -eps v_k - 2e-6 (s sum |g_i r_ki| + sum_j v_j sum_i |r_ji r_ki|).
Observed on an MI355X: dots at 0.0059 of their bound (big: 0.0005), Gram entries at 0.0073 (big: 0.0012); max |v - v64| / max |v64|
1.6e-8 (K = 1), 2.1e-8 (K = 3), 2.0e-8 (K = 5), 2.8e-8 (K = 16) against 2.4e-7, in 1, 2, 3 and 2 solver iterations; the smallest
multiplier -0.0022 against a tol of 0.026 to 0.064; norm 2.3e-8; feasibility at 0.0021 of its bound; with K = 1, gamma = eps = 0
v equals A-GEM's -alpha bit for bit and the weights are equal."""
import copy

import pytest
import torch

from test_gem_host import enumerate_qp, kkt_residuals
from test_optimizer_clip_gpu import Toy, assert_same, make_grad, norms64, state

pytestmark = pytest.mark.gpu

TOL = 2e-6
VTOL = 2.0 ** -22
KEYS = {"dots", "v", "projected", "active", "qp_iterations", "projected_steps", "unsolved_steps"}


def f32(x):
    return torch.tensor(x, dtype=torch.float32, device="cuda")


GAMMA = float(torch.tensor(0.1, dtype=torch.float32))
EPS = float(torch.tensor(1e-3, dtype=torch.float32))


def build(big=False, gem=True, max_tasks=11, gamma=GAMMA, eps=EPS, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    p = cl.GEM(flat, max_tasks=max_tasks, memory_strength=gamma, eps=eps) if gem else None
    return flat, p, cl.FusedAdamW(flat, lr=1e-3, projection=p, **kw)


_LAYOUT = {}


def layout(big):
    if big not in _LAYOUT:
        from indic_cl_asr_amd import cl
        flat = cl.FlatParams(Toy(big=big))
        _LAYOUT[big] = (list(flat.entries), flat.numel)
    return _LAYOUT[big]


def make_inputs(big, signs, g_seed=101, r_seed=200):
    """g and one reference per entry of `signs` (-1: opposes g, +1: agrees with it) as fp32 device tensors."""
    e, n = layout(big)
    g = make_grad(e, n, g_seed)
    refs = [(make_grad(e, n, r_seed + k) + 0.5 * s * g).cuda() for k, s in enumerate(signs)]
    return g.cuda(), refs


def step_with(flat, gem, opt, g, refs, **kw):
    """What the training loop does: one memory batch per earlier task becomes that task's reference, then the task step."""
    for k, r in enumerate(refs):
        flat.grad.copy_(r)
        gem.store_reference(f"task{k}", opt)
        assert not flat.grad.any() and gem.has_reference
    flat.grad.copy_(g)
    opt.step(**kw)


def reference(g, refs, scale, gamma=GAMMA, eps=EPS, free=None, mixed=True):
    """float64 on the CPU from the inputs themselves: d, sum |g r_k|, Gram, sum |r_j r_k|, P, v; asserts what the tests need."""
    g64 = g.double().cpu()
    R = torch.stack([r.double().cpu() for r in refs])
    d = scale * (R @ g64)
    dmag = scale * (R.abs() @ g64.abs())
    gram, gmag = R @ R.T, R.abs() @ R.abs().T
    P = gram + eps * torch.eye(len(refs), dtype=torch.float64)
    assert float(torch.linalg.cond(P)) <= 1e6
    assert bool((d < -1000 * TOL * dmag).any())                     # the margin of the decision
    v, fr = solve64(P, d, gamma, free)
    if mixed and len(refs) > 1:
        assert bool(fr.any()) and not bool(fr.all()), fr            # v_k > gamma and v_k == gamma both occur
    return dict(g=g64, R=R, d=d, dmag=dmag, gram=gram, gmag=gmag, P=P, v=v, free=fr)


def solve64(P, d, gamma, free=None):
    """The exact solution: by enumeration, or from a known free set whose KKT conditions are asserted."""
    if free is None:
        return enumerate_qp(P, d, gamma)
    free = torch.tensor(free)
    v = torch.full((d.numel(),), float(gamma), dtype=torch.float64)
    v[free] = torch.linalg.solve(P[free][:, free], -(d[free] + P[free][:, ~free] @ v[~free]))
    lam = P @ v + d
    assert bool((v[free] > gamma).all()) and bool((lam[~free] > 0).all())
    assert float(lam[free].abs().max()) <= 1e-12 * float((P.abs() @ v.abs()).max())
    return v, free


def reported(gem, eps=EPS):
    """(stats, d, P) as float64 from what the device holds: the inputs of ia_gem_solve."""
    st = gem.stats()
    assert set(st) == KEYS
    d = torch.tensor(st["dots"], dtype=torch.float64)
    P = gem.gram_matrix().double() + eps * torch.eye(d.numel(), dtype=torch.float64)
    return st, d, P


def gem_grad(g, refs, v, scale=1.0):
    """g * scale + sum_k v_k * r_k with one fp32 torch op per rounding, k ascending, rows with v_k == 0 left out."""
    acc = g * f32(scale)
    for vk, r in zip(v, refs):
        if vk != 0.0:
            acc = acc + f32(vk) * r
    return acc


def rel(a, b):
    return abs(a - b) / abs(b)


def check_dots(gem, ref):
    st, d, P = reported(gem)
    gram = gem.gram_matrix().double()
    derr = ((d - ref["d"]).abs() / (TOL * ref["dmag"])).max().item()
    gerr = ((gram - ref["gram"]).abs() / (TOL * ref["gmag"])).max().item()
    print("dots", st["dots"], "float64", ref["d"].tolist(), "worst err / bound", derr)
    print("gram worst err / bound", gerr, "symmetric", bool(torch.equal(gram, gram.T)))
    assert derr <= 1.0 and gerr <= 1.0 and torch.equal(gram, gram.T)
    assert st["projected"] == 1 and st["projected_steps"] == 1 and st["unsolved_steps"] == 0


def test_dots_and_gram_match_float64_and_reproduce():
    signs = (-1, +1, -1)
    for big, scale in ((False, 1.0), (True, 0.5)):                  # big: > 2048 chunks, the grid-stride loops run twice
        g, refs = make_inputs(big, signs)
        fa, pa, A = build(big=big, max_tasks=3)
        fb, pb, B = build(big=big, max_tasks=3)
        kw = {} if scale == 1.0 else {"grad_scale": scale}
        step_with(fa, pa, A, g, refs, **kw)
        step_with(fb, pb, B, g, refs, **kw)
        check_dots(pa, reference(g, refs, scale))
        assert torch.equal(pa._buf, pb._buf)
        assert_same(A, B, f"two optimizers, same inputs, big={big}")
        del fa, pa, A, fb, pb, B, g, refs


@pytest.mark.parametrize("K", [1, 3, 5, 16])
def test_solver_matches_the_exact_solution(K):
    if K == 16:                                                     # exactly two opposing rows: two free coordinates
        signs, free = [+1] * 16, [False] * 16
        for k in (3, 12):
            signs[k], free[k] = -1, True
    else:
        signs, free = [(-1, +1, -1, -1, +1)[k] for k in range(K)], None
    g, refs = make_inputs(False, signs)
    flat, gem, opt = build(max_tasks=16)
    step_with(flat, gem, opt, g, refs)
    reference(g, refs, 1.0, free=free)                              # the inputs do what the test needs
    st, d, P = reported(gem)
    v64, fr = solve64(P, d, GAMMA, free)                            # from the device's own d and Gram: no reduction error
    v = torch.tensor(st["v"], dtype=torch.float64)
    err = float((v - v64).abs().max()) / float(v64.abs().max())
    tol = VTOL * float((P.abs() @ v.abs()).max())
    lo, lam_min, comp = kkt_residuals(P, d, v, GAMMA)
    print(f"K={K} v", st["v"], "max|v - v64| / max|v64|", err, "bound", VTOL, "min lambda", lam_min, "comp", comp, "tol", tol,
          "iterations", st["qp_iterations"], "active", st["active"])
    assert err <= VTOL
    assert lo >= 0.0 and lam_min >= -tol and comp <= tol
    assert st["projected"] == 1 and st["unsolved_steps"] == 0 and len(st["v"]) == len(st["dots"]) == K
    assert st["active"] == int(fr.sum()) == int((v > GAMMA).sum()) and 1 <= st["qp_iterations"] <= 4 * K
    assert all(float(f32(x)) == x for x in st["v"])                 # v is fp32, rounded once


def test_step_is_applied_bit_for_bit():
    signs = (-1, +1, -1)
    fa, gem, A = build()
    fb, _, B = build(gem=False)
    for step, (g_seed, r_seed) in enumerate(((101, 200), (103, 300), (107, 400))):
        g, refs = make_inputs(False, signs, g_seed, r_seed)
        reference(g, refs, 1.0)
        step_with(fa, gem, A, g, refs)
        st = gem.stats()
        assert st["projected"] == 1 and all(x >= GAMMA for x in st["v"]) and max(st["v"]) > GAMMA
        fb.grad.copy_(gem_grad(g, refs, st["v"]))
        B.step()
        assert_same(A, B, f"step {step}")
    assert gem.stats()["projected_steps"] == 3 and gem.tasks() == ["task0", "task1", "task2"]
    entries, _ = layout(False)
    idle = [i for i, e in enumerate(entries) if e[0] == "idle"][0]
    steps = A.seg_step.tolist()
    assert steps[idle] == 0 and all(s == 3 for i, s in enumerate(steps) if i != idle)


def test_projection_then_clipping():
    entries, _ = layout(False)
    g, refs = make_inputs(False, (-1, +1, -1))
    reference(g, refs, 1.0)
    fa, gem, A = build(max_grad_norm=1.0)
    fb, _, B = build(gem=False)
    step_with(fa, gem, A, g, refs)
    st, ps = A.stats(), gem.stats()
    assert ps["projected"] == 1 and ps["projected_steps"] == 1 and st["clipped_steps"] == 1
    G = gem_grad(g, refs, ps["v"])
    _, want = norms64(entries, G.cpu())
    _, plain = norms64(entries, g.cpu())
    print("grad_norm", st["grad_norm"], "float64 of the projected gradient", want, "rel", rel(st["grad_norm"], want),
          "float64 of g", plain)
    assert rel(st["grad_norm"], want) <= TOL and rel(st["grad_norm"], plain) > TOL
    assert rel(st["clip_coef"], 1.0 / (want + 1e-6)) <= TOL
    assert A.grad_norms()["idle"] == 0.0
    coef = f32(st["clip_coef"])
    assert float(coef) == st["clip_coef"]
    fb.grad.copy_(G * coef)
    B.step()
    assert_same(A, B, "projected, then clipped")
    idle = [i for i, e in enumerate(entries) if e[0] == "idle"][0]
    assert int(A.seg_step[idle]) == 0


def test_two_parameter_groups():
    entries, _ = layout(False)
    g, refs = make_inputs(False, (-1, +1, -1))
    reference(g, refs, 1.0)
    groups = [dict(params=["v8", "mat"], lr=3e-4, weight_decay=0.0)]
    fa, gem, A = build(param_groups=groups)
    fb, _, B = build(gem=False, param_groups=groups)
    fc, _, C = build(gem=False)
    step_with(fa, gem, A, g, refs)
    G = gem_grad(g, refs, gem.stats()["v"])
    fb.grad.copy_(G); fc.grad.copy_(G)
    B.step(); C.step()
    assert_same(A, B, "two groups")
    assert not torch.equal(fa.theta, fc.theta)                      # the second group's values reached the kernel
    idle = [i for i, e in enumerate(entries) if e[0] == "idle"][0]
    assert int(A.seg_step[idle]) == 0


def test_projected_gradient_is_feasible_in_float64():
    g, refs = make_inputs(False, (-1, +1, -1, -1, +1))
    ref = reference(g, refs, 1.0)
    flat, gem, opt = build()
    step_with(flat, gem, opt, g, refs)
    st = gem.stats()
    v = torch.tensor(st["v"], dtype=torch.float64)
    G64 = ref["g"] + v @ ref["R"]
    lhs = ref["R"] @ G64
    slack = EPS * v + TOL * (ref["dmag"] + ref["gmag"] @ v)
    print("<G, r_k>", lhs.tolist(), "allowed below zero", slack.tolist(), "worst (lhs + eps v) / bound",
          float((-(lhs + EPS * v) / (TOL * (ref["dmag"] + ref["gmag"] @ v))).max()))
    assert st["projected"] == 1 and bool((lhs >= -slack).all())
    assert bool((ref["R"] @ ref["g"] < 0).any())                    # the unprojected gradient is not feasible


def test_agreeing_references_are_the_plain_step():
    g, agree = make_inputs(False, (+1, +1, +1))
    R, g64 = torch.stack([r.double().cpu() for r in agree]), g.double().cpu()
    assert bool((R @ g64 > 1000 * TOL * (R.abs() @ g64.abs())).all())
    fa, gem, A = build()
    fb, _, B = build(gem=False)
    assert not gem.has_reference and gem.tasks() == []
    for what, refs in (("no reference", []), ("agreeing references", agree), ("cleared", [])):
        if what == "cleared":
            gem.clear()
            assert not gem.has_reference
        step_with(fa, gem, A, g, refs)
        fb.grad.copy_(g)
        B.step()
        assert_same(A, B, what)
        st = gem.stats()
        assert st["projected"] == 0 and st["projected_steps"] == 0 and st["unsolved_steps"] == 0 and set(st) == KEYS
        assert st["active"] == 0 and not any(st["v"])
        if what == "agreeing references":
            assert len(st["dots"]) == 3 and all(x > 0 for x in st["dots"])
    # clipped: the measured norm is ia_grad_norm's bit for bit
    fc, gem_c, C = build(max_grad_norm=1.0)
    fd, _, D = build(gem=False, max_grad_norm=1.0)
    step_with(fc, gem_c, C, g, agree)
    fd.grad.copy_(g)
    D.step()
    assert_same(C, D, "agreeing references, clipped")
    assert torch.equal(C.last_grad_norm.clone().view(torch.int32), D.last_grad_norm.clone().view(torch.int32))
    assert torch.equal(C._seg_norm.view(torch.int32), D._seg_norm.view(torch.int32))
    assert C.stats() == D.stats() and C.stats()["clipped_steps"] == 1 and gem_c.stats()["projected_steps"] == 0


def test_one_task_without_margin_is_agem():
    from indic_cl_asr_amd import cl
    g, (r,) = make_inputs(False, (-1,))
    fa, gem, A = build(gamma=0.0, eps=0.0)
    fb = cl.FlatParams(Toy(big=False).cuda())
    agem = cl.AveragedGEM(fb)
    B = cl.FusedAdamW(fb, lr=1e-3, projection=agem)
    step_with(fa, gem, A, g, [r])
    fb.grad.copy_(r)
    agem.store_reference(B)
    fb.grad.copy_(g)
    B.step()
    sg, sa = gem.stats(), agem.stats()
    v, alpha = f32(sg["v"][0]), f32(-sa["alpha"])
    ulp = float(torch.nextafter(alpha, f32(float("inf"))) - alpha)
    print("v", sg["v"][0], "-alpha", -sa["alpha"], "difference in ulp", float(v - alpha) / ulp)
    assert sg["projected"] == sa["projected"] == 1 and sg["active"] == 1
    assert abs(float(v - alpha)) <= ulp
    # One ulp of the coefficient moves G by at most dG = ulp |r_i| plus the two roundings of G itself, a relative change
    # delta = dG / |G|.  In the first step m / (sqrt(v) / sqrt(1 - beta2) + eps) has magnitude <= 0.1 and moves by at most 2 delta
    # (m by delta, the root by delta) plus its own roundings (under 8 * 2^-24); times step_size = lr / (1 - beta1) = 1e-2 that is
    # 1e-3 (2 delta + 8 * 2^-24) on the update, and the final fma rounds each weight once: 2^-23 |theta| between the two.
    G = gem_grad(g, [r], sg["v"]).abs()
    dG = ulp * r.abs() + 2.0 ** -23 * G
    live = G > 0
    bound = torch.zeros_like(G)
    bound[live] = 1e-3 * (2 * dG[live] / G[live] + 8 * 2.0 ** -24) + 2.0 ** -23 * fa.theta[live].abs()
    diff = (fa.theta - fb.theta).abs()
    print("max weight difference", float(diff.max()), "of its bound", float((diff[live] / bound[live]).max()))
    assert bool((diff <= bound).all())


def test_refusals():
    from indic_cl_asr_amd import _lib, cl
    g, refs = make_inputs(False, (-1, +1, -1))
    # a non-finite reference never projects: the plain step, counted
    fa, gem, A = build()
    fb, _, B = build(gem=False)
    bad = refs[1].clone()
    entries, _ = layout(False)
    off = [e for e in entries if e[0] == "v9"][0][1]
    bad[off + 4100] = float("inf")                                  # data in a reference buffer: nothing here faults the device
    step_with(fa, gem, A, g, [refs[0], bad, refs[2]])
    fb.grad.copy_(g)
    B.step()
    assert_same(A, B, "non-finite reference")
    st = gem.stats()
    assert st["projected"] == 0 and st["projected_steps"] == 0 and st["unsolved_steps"] == 1 and not any(st["v"])
    # a 17th task, bad arguments, path_integral, a foreign FlatParams
    flat = cl.FlatParams(Toy(big=False).cuda())
    other = cl.FlatParams(Toy(big=False).cuda())
    small = cl.GEM(flat, max_tasks=2)
    for k in range(2):
        small.store_reference(k)
    small.store_reference(0)                                        # an existing task keeps its row
    assert small.tasks() == [0, 1]
    with pytest.raises(ValueError, match="max_tasks"):
        small.store_reference("one more")
    full = cl.GEM(flat, max_tasks=16)
    for k in range(16):
        full.store_reference(("lang", k))
    with pytest.raises(ValueError, match="max_tasks"):
        full.store_reference(("lang", 16))
    del full
    for kw in (dict(max_tasks=0), dict(max_tasks=17), dict(memory_strength=-0.1), dict(eps=-1e-3)):
        with pytest.raises(ValueError):
            cl.GEM(flat, **kw)
    with pytest.raises(ValueError):
        cl.FusedAdamW(flat, projection=cl.GEM(flat, max_tasks=1), path_integral=cl.SynapticIntelligence(flat))
    with pytest.raises(ValueError):
        cl.FusedAdamW(flat, projection=cl.GEM(other, max_tasks=1))
    L = _lib.lib()
    assert L.ia_gem_workspace_bytes(7, 3) == 7 * 3 * 4 and L.ia_gem_workspace_bytes(7, 17) == 0
    # argument validation happens before any device work: null pointers -> IA_INVALID_VALUE (-1)
    assert L.ia_gem_dots(None, None, 4, 1, None, 1, 1, 1.0, None, -1, None, None, 0, None) == -1
    assert L.ia_gem_solve(None, None, 1, 0.5, 1e-3, None) == -1
    assert L.ia_grad_norm_gem(None, None, 1, None, 1, 1.0, 0.0, None, None, None, None, 0, None, 4, 1, None, None) == -1
    assert L.ia_adamw_step_segmented_gem(None, None, None, None, None, 1, None, None, 1, 0, 0.9, 0.999, 1e-8, 1.0, None, None, 1,
                                         None, None, None, 0, None, None, 4, 1, None, None, None) == -1
    n = flat.chunk_table.shape[0]
    ws = small.workspace(n)
    args = (_lib.ptr(flat.grad), _lib.ptr(small.refs), small.stride, 2, _lib.ptr(flat.chunk_table), n, len(flat.entries), 1.0, None)
    assert L.ia_gem_dots(*args, -1, _lib.ptr(small.sums), _lib.ptr(ws), 2 * n * 4 - 1, _lib.stream_ptr()) == -2
    assert L.ia_gem_dots(*args, 2, _lib.ptr(small.sums), _lib.ptr(ws), ws.numel(), _lib.stream_ptr()) == -1    # gram_row >= ntasks
    assert L.ia_gem_solve(_lib.ptr(small.sums), _lib.ptr(small.state), 17, 0.5, 1e-3, _lib.stream_ptr()) == -1


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
    m = EncDecHybridRNNTCTCModel(model_config('tiny', languages=['hi', 'ta', 'bn'])).cuda().train()
    freeze_layer(m, 0)
    twin = copy.deepcopy(m)                                         # only its weights are used: it is fed gradients
    flat, flat_b = cl.FlatParams(m), cl.FlatParams(twin)
    assert flat.entries == flat_b.entries and torch.equal(flat.theta, flat_b.theta)
    gem = cl.GEM(flat, max_tasks=2, memory_strength=GAMMA)
    opt = cl.FusedAdamW(flat, lr=1e-3, projection=gem)
    B = cl.FusedAdamW(flat_b, lr=1e-3)
    memory = cl.EpisodicMemory(per_language=4, seed=0)
    for lang, seed in (("hi", 1), ("ta", 2)):
        batch, ids = _batch([lang] * 4, seed=seed)
        memory.add(batch, ids)
    assert len(memory) == 8 and memory.languages() == ["hi", "ta"]

    opt.zero_grad()
    mem_grads = []
    for lang in memory.languages():                                 # one memory batch and one reference per earlier language
        mb, ml = memory.sample(4, "cuda", language=lang)
        assert ml == [lang] * 4
        loss, _ = m.training_step(mb, ml, compute_wer=False)
        loss.backward()
        mem_grads.append(flat.grad.clone())
        assert mem_grads[-1].any()
        gem.store_reference(lang, opt)
        assert not flat.grad.any()
    assert gem.tasks() == ["hi", "ta"] and torch.equal(gem.refs[0, :flat.numel], mem_grads[0])
    assert torch.equal(gem.refs[1, :flat.numel], mem_grads[1])
    task, task_langs = _batch(["bn"] * 4, seed=3)
    loss, _ = m.training_step(task, task_langs, compute_wer=False)
    loss.backward()
    g, before = flat.grad.clone(), flat.theta.clone()
    if float(g.double() @ mem_grads[1].double()) > 0:               # whatever the data gave, this step has to project
        gem.refs[1].neg_()
        mem_grads[1] = -mem_grads[1]
        flat.grad.copy_(mem_grads[1])                               # stored again: the Gram row follows the row
        gem.store_reference("ta", opt)
        flat.grad.copy_(g)
    opt.step()
    st = gem.stats()
    print(st)
    assert set(st) == KEYS and len(st["v"]) == len(st["dots"]) == 2
    assert st["projected"] == 1 and st["projected_steps"] == 1 and st["unsolved_steps"] == 0
    assert all(x >= GAMMA for x in st["v"]) and 0 <= st["active"] <= 2 and st["qp_iterations"] >= 0
    assert not torch.equal(flat.theta, before)
    G = gem_grad(g, mem_grads, st["v"])
    for name, off, k, _ in flat.entries:                            # `.grad is None` where the task gave no gradient
        if not g[off:off + k].any():
            G[off:off + k] = 0
            assert torch.equal(flat.theta[off:off + k], before[off:off + k]), name
    flat_b.grad.copy_(G)
    B.step()
    assert_same(opt, B, "task step")                                # weights, moments, counters and the fresh bf16 images
