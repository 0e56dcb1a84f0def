"""Orthogonal Gradient Descent inside the fused optimizer step (ia_ogd_dots, ia_ogd_project, cl.OGD) on the toy module of
tests/test_optimizer_clip_gpu.py, whose tensor sizes reach every path of the flat kernels (a tail shorter than a float4, the
alignment gaps, the 4096 chunk boundary, the idle tensor and -- `big=True`, one case -- more than 2048 chunks), and once through
the model.  Row counts 1, 15, 16, 17 and 33: one tile of the dots kernel, the tile boundary, and beyond GEM's cap of 16; they also
cover every remainder of the four-row groups both kernels issue their loads in.  The scope leaves out v3 (63 elements: float4
body and a 3-element tail) and v8 (4097 elements: two chunks), so out-of-scope chunks of both shapes occur.

The definition (include/indicasr.h): c_k = <x, v_k> over the scope, fp32 partial sums per chunk finished in fp64 and rounded once
to fp32, and per element of a live tensor in scope, each product and difference rounded to fp32 on its own,
    acc = x;  for k ascending: acc = acc - c_k * v_k;  dst = acc * alpha
so projection and step are checked bit for bit against one torch op per rounding built from the coefficients the device reports.

Tolerances, all against float64 on the CPU:
  dots        |c_k - c64_k| <= 2e-6 sum_i |g_i v_ki|: the per-row reduction shape is ia_agem_dots's (a thread's four float4, the DPP
              wave sum, the four wave sums: 18 roundings of 2^-24, the bound derived in tests/test_optimizer_clip_gpu.py), against
              the sum of magnitudes; <g, g> to 2e-6 relative (the same shape, every term positive).
  basis       max |<v_i, v_j> - delta_ij| <= 2 (2e-6 + (M + 2) 2^-24) after M = 33 inserts: by Cauchy-Schwarz the dots' bound is
              relative to |x| |v|, one rounding is added per subtracted row plus the normalisation, doubled for the pair.
  insert      a dependent candidate has a float64 residual ratio below tol / 100, the independent ones above 100 tol, both
              asserted in the reference, so no decision sits near the threshold.
  model       |<G, v_k>| <= 2e-6 sum_i |g_i v_ki| for the projected gradient G: the dots' bound.
Observed on an MI355X (printed with pytest -s): dots at 0.0014 of their bound for M = 15 .. 33 (M = 1: 0.0002; big, M = 3: 0.00003),
<g, g> at 0.0074 of its bound (big: 0.00007); max |<v_i, v_j> - delta_ij| after 33 inserts at 0.011 of its bound (9.1e-8); the
dependent candidate's float64 residual ratio 2.6e-8 against tol / 100 = 1e-5; through the model
the worst |<G, v_k>| at 0.0034 of its bound and removed_fraction = 0.123."""
import copy

import pytest
import torch

from test_ogd import STAT_KEYS, gram_schmidt64, residual64, scope_mask
from test_optimizer_clip_gpu import Toy, assert_same, make_grad, norms64

pytestmark = pytest.mark.gpu

TOL = 2e-6
OUT = ("v3", "v8")
ROWS = [1, 15, 16, 17, 33]
SEED0 = 500                                                       # candidate k of a basis is make_grad(seed SEED0 + k)


def f32(x):
    return torch.tensor(x, dtype=torch.float32, device="cuda")


def bits(t):
    return t.contiguous().view(torch.int32)


_LAYOUT = {}


def layout(big=False):
    if big not in _LAYOUT:
        from indic_cl_asr_amd import cl
        flat = cl.FlatParams(Toy(big=big))
        _LAYOUT[big] = (list(flat.entries), flat.numel)
    return _LAYOUT[big]


def scope_of(big=False):
    return [e[0] for e in layout(big)[0] if e[0] not in OUT]


def build(big=False, ogd=True, max_directions=1, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    p = cl.OGD(flat, max_directions, scope=scope_of(big)) if ogd else None
    return flat, p, cl.FusedAdamW(flat, lr=1e-3, projection=p, **kw)


_BASIS = {}


def basis_state(M, big=False):
    """The state_dict of an OGD after M inserts of seeded gradients, built once per (M, big) and never modified."""
    if (M, big) not in _BASIS:
        e, n = layout(big)
        flat, ogd, opt = build(big=big, max_directions=M)
        for k in range(M):
            flat.grad.copy_(make_grad(e, n, SEED0 + k))
            assert ogd.add_direction(opt) and not flat.grad.any()
        assert ogd.directions == M and ogd.has_reference
        st = ogd.stats()
        assert set(st) == STAT_KEYS and st["directions"] == M and st["dependent"] == st["nonfinite"] == 0
        _BASIS[(M, big)] = ogd.state_dict()
    return _BASIS[(M, big)]


def with_basis(M, big=False, room=0, **kw):
    flat, ogd, opt = build(big=big, max_directions=M + room, **kw)
    ogd.load_state_dict(basis_state(M, big))
    return flat, ogd, opt


def rows_of(ogd):
    return [ogd.basis[k, :ogd.flat.numel] for k in range(ogd.directions)]


def restate(x, rows, coef, entries, scope, live=None, alpha=1.0, dst=None):
    """The definition with one fp32 torch op per rounding.  `live`: names of the live tensors (None: all).  dst None: in place
    (everything that is not projected keeps x's bits); otherwise what is not projected keeps dst's bits, except the elements of
    out-of-scope tensors, which become zero."""
    acc = x.clone()
    for ck, v in zip(coef, rows):
        prod = f32(ck) * v
        acc = acc - prod
    acc = acc * f32(alpha)
    out = x.clone() if dst is None else dst.clone()
    for name, off, k, _ in entries:
        if name in scope:
            if live is None or name in live:
                out[off:off + k] = acc[off:off + k]
        elif dst is not None:
            out[off:off + k] = 0.0
    return out


def live_names(entries, g):
    return {name for name, off, k, _ in entries if bool(g[off:off + k].any())}


def note(key, value):
    """The figures the header records (pytest -s)."""
    print("observed", key, value)


@pytest.mark.parametrize("M,big", [(m, False) for m in ROWS] + [(3, True)])
def test_dots_match_float64_and_reproduce(M, big):
    e, n = layout(big)
    g = make_grad(e, n, 101)
    fa, oa, A = with_basis(M, big)
    fb, ob, B = with_basis(M, big)
    for f, o in ((fa, A), (fb, B)):
        f.grad.copy_(g)
        o.step()
    assert torch.equal(bits(oa.dots64), bits(ob.dots64)) and torch.equal(bits(oa.dots32), bits(ob.dots32))
    assert_same(A, B, "two optimizers, same inputs")
    mask = scope_mask(e, n, set(oa.scope_names))
    V = oa.basis[:M, :n].double().cpu()
    g64 = g.double() * mask
    c64, mag = V @ g64, V.abs() @ g64.abs()
    c = oa.dots64[:M].cpu()
    frac = float(((c - c64).abs() / (TOL * mag)).max())
    sq, sq64 = float(oa.dots64[M]), float(g64 @ g64)
    note(f"dots M={M} big={big}: worst err / bound", frac)
    note(f"<g, g> M={M} big={big}: rel err / bound", abs(sq - sq64) / (TOL * sq64))
    assert frac <= 1.0
    assert abs(sq - sq64) <= TOL * sq64
    assert torch.equal(oa.dots32[:M].cpu(), c.float())               # rounded once
    assert torch.equal(oa.coefficients(), c.float())
    st = oa.stats()
    removed64 = float((c64 * c64).sum()) / sq64
    slack = float((2 * c64.abs() * TOL * mag).sum()) / sq64 + 2 * TOL * removed64
    assert set(st) == STAT_KEYS and st["directions"] == M
    assert abs(st["removed_fraction"] - removed64) <= slack and 0.0 < st["removed_fraction"] < 1.0
    del fa, oa, A, fb, ob, B


@pytest.mark.parametrize("M", ROWS)
def test_projection_is_bit_for_bit(M):
    from indic_cl_asr_amd import _lib
    e, n = layout(False)
    flat, ogd, opt = with_basis(M)
    scope = set(ogd.scope_names)
    gen = torch.Generator().manual_seed(7 + M)
    x = torch.randn(n, generator=gen).cuda()                         # non-zero everywhere: gaps, idle, out-of-scope tensors
    coef = torch.randn(M, generator=gen).cuda()
    ogd.basis[0, :n] = torch.randn(n, generator=gen).cuda()          # a row with data everywhere: the kernel decides what it reads
    rows = rows_of(ogd)
    names = [name for name, *_ in e]
    dead = ("idle", "v6", "v0")
    flags = torch.tensor([int(name not in dead) for name in names], dtype=torch.int32, device="cuda")
    live = {name for name in names if name not in dead}
    for alpha in (1.0, 0.37):
        y = x.clone()
        ogd._project(y, M, coef, _lib.ptr(flags), y, alpha)          # in place, with flags: the step
        want = restate(x, rows, coef.tolist(), e, scope, live, alpha)
        assert torch.equal(bits(y), bits(want)), ("in place", alpha)
        assert not torch.equal(bits(y), bits(x))
    for name, off, k, _ in e:                                        # idle, out of scope: x's bits (the gaps: checked above)
        if name in dead or name in OUT:
            assert torch.equal(bits(want[off:off + k]), bits(x[off:off + k])), name
    dst0 = torch.full((ogd.stride,), 7.0, device="cuda")
    dst = dst0.clone()
    ogd._project(x, M, coef, None, dst, 0.37)                        # into another buffer, no flags: the insert
    want = restate(x, rows, coef.tolist(), e, scope, None, 0.37, dst=dst0[:n])
    assert torch.equal(bits(dst[:n]), bits(want)) and torch.equal(dst[n:], dst0[n:])
    for name, off, k, _ in e:
        if name in OUT:
            assert not dst[off:off + k].any(), name
    covered = torch.zeros(n, dtype=torch.bool)
    for name, off, k, _ in e:
        covered[off:off + k] = True
    assert bool((dst[:n].cpu()[~covered] == 7.0).all()) and int((~covered).sum()) > 0     # the alignment gaps


VARIANTS = {
    "plain": ({}, {}),
    "clipped": (dict(max_grad_norm=1.0), {}),
    "two_groups": (dict(param_groups=[dict(params=["v8", "mat"], lr=3e-4, weight_decay=0.0)]), {}),
    "grad_scale": ({}, dict(grad_scale=0.5)),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_step_is_the_plain_step_on_the_restated_gradient(variant):
    kw, step_kw = VARIANTS[variant]
    e, n = layout(False)
    fa, ogd, A = with_basis(17, **kw)
    fb, _, B = build(ogd=False, **kw)
    scope, rows = set(ogd.scope_names), rows_of(ogd)
    for step, seed in enumerate((101, 103)):
        g = make_grad(e, n, seed).cuda()
        fa.grad.copy_(g)
        A.step(**step_kw)
        G = restate(g, rows, ogd.coefficients().tolist(), e, scope, live_names(e, g))
        assert torch.equal(bits(fa.grad), bits(G)) and not torch.equal(bits(G), bits(g))
        fb.grad.copy_(G)
        B.step(**step_kw)
        assert_same(A, B, f"{variant}, step {step}")
        if variant == "clipped":                                    # project, then clip: the norm is the consumed gradient's
            st = A.stats()
            _, want = norms64(e, G.cpu())
            _, plain = norms64(e, g.cpu())
            assert st == B.stats() and st["clipped_steps"] == step + 1
            assert abs(st["grad_norm"] - want) <= TOL * want and abs(st["grad_norm"] - plain) > TOL * plain
    idle = [i for i, entry in enumerate(e) if entry[0] == "idle"][0]
    steps = A.seg_step.tolist()
    assert steps[idle] == 0 and all(s == 2 for i, s in enumerate(steps) if i != idle)
    if variant == "two_groups":
        fc, _, C = build(ogd=False)
        fc.grad.copy_(G)
        C.step()
        C.step()
        assert not torch.equal(fa.theta, fc.theta)                  # the second group's values reached the kernel


def test_empty_basis_is_the_plain_step():
    e, n = layout(False)
    g = make_grad(e, n, 101).cuda()
    fa, ogd, A = build(max_directions=2, max_grad_norm=1.0)
    fb, _, B = build(ogd=False, max_grad_norm=1.0)
    for what in ("empty", "one direction, then cleared"):
        if what != "empty":
            fa.grad.copy_(make_grad(e, n, SEED0))
            assert ogd.add_direction(A) and ogd.has_reference
            ogd.clear()
        assert not ogd.has_reference and ogd.directions == 0
        fa.grad.copy_(g)
        fb.grad.copy_(g)
        A.step()
        B.step()
        assert torch.equal(bits(fa.grad), bits(g))
        assert_same(A, B, what)
        assert A.stats() == B.stats()


def test_live_tensor_whose_projected_gradient_is_zero_still_steps():
    e, n = layout(False)
    idx = [i for i, entry in enumerate(e) if entry[0] == "v0"][0]
    off = e[idx][1]
    assert e[idx][2] == 1
    lr, wd = 1e-3, 1e-2
    flat, ogd, opt = build(max_directions=2, weight_decay=wd)
    d = torch.zeros(n)
    d[off] = 3.0
    flat.grad.copy_(d)
    assert ogd.add_direction(opt)
    row = ogd.basis[0]
    assert float(row[off]) == 1.0 and int(row.count_nonzero()) == 1  # normalised to exactly 1
    g = make_grad(e, n, 101)
    g[off] = 2.0
    G = g.clone()
    G[off] = 0.0
    theta0 = flat.theta.clone()
    flat.grad.copy_(g)
    opt.step()
    assert ogd.coefficients().tolist() == [2.0]
    assert torch.equal(bits(flat.grad), bits(G.cuda()))             # exactly zero there, everything else untouched
    assert int(opt.seg_step[idx]) == 1 and float(opt.exp_avg[off]) == 0.0 and float(opt.exp_avg_sq[off]) == 0.0
    t0, t1 = float(theta0[off]), float(flat.theta[off])
    want = t0 * (1.0 - lr * wd)
    assert t1 != t0 and abs(t1 - want) <= 2.0 ** -23 * abs(want)    # decay and the product: one fp32 rounding each
    # a plain optimizer fed G takes v0 for dead: it differs there and nowhere else
    fb, _, B = build(ogd=False, weight_decay=wd)
    fb.grad.copy_(G.cuda())
    B.step()
    assert int(B.seg_step[idx]) == 0 and float(fb.theta[off]) == t0
    differ = (bits(flat.theta) != bits(fb.theta)).nonzero().flatten().tolist()
    assert differ == [off]


def test_inserts_are_orthonormal_and_bad_candidates_are_dropped():
    M = 33
    e, n = layout(False)
    flat, ogd, opt = with_basis(M, room=1)
    mask = scope_mask(e, n, set(ogd.scope_names))
    V = ogd.basis[:M, :n].double().cpu()
    err = float((V @ V.T - torch.eye(M, dtype=torch.float64)).abs().max())
    bound = 2 * (2e-6 + (M + 2) * 2.0 ** -24)
    note("basis: max |<v_i, v_j> - delta_ij| / bound", err / bound)
    assert err <= bound
    assert not bool((V * (1.0 - mask)).any()) and not bool(ogd.basis[:M, n:].any())
    # the reference: every candidate was far from dependent, the combination is far from independent
    cands = [make_grad(e, n, SEED0 + k) for k in range(M + 1)]
    _, kept, ratios = gram_schmidt64(cands, mask, ogd.tol)
    assert all(kept) and min(ratios) > 100 * ogd.tol
    comb = f32(2.0) * ogd.basis[3, :n] + f32(-0.5) * ogd.basis[7, :n]       # an fp32 combination of stored rows
    c64 = comb.double().cpu()
    ratio = float(residual64(list(V), c64).norm() / c64.norm())
    note("dependent candidate: float64 residual ratio", ratio)
    assert ratio < ogd.tol / 100
    flat.grad.copy_(comb)
    assert ogd.add_direction(opt) is False and not flat.grad.any()
    assert ogd.directions == M and ogd.stats()["dependent"] == 1
    bad = cands[M].clone()
    off = [entry for entry in e if entry[0] == "v9"][0][1]
    bad[off + 4100] = float("nan")                                  # data in a gradient buffer: nothing here faults the device
    flat.grad.copy_(bad)
    assert ogd.add_direction(opt) is False and not flat.grad.any()
    st = ogd.stats()
    assert ogd.directions == M and st["nonfinite"] == 1 and st["dependent"] == 1 and st["directions"] == M
    assert torch.equal(ogd.basis[:M, :n].double().cpu(), V)         # the stored rows were not touched
    flat.grad.copy_(cands[M])                                       # the row the dropped candidates used is written afresh
    assert ogd.add_direction(opt) is True and ogd.directions == M + 1
    W = ogd.basis[:M + 1, :n].double().cpu()
    assert float((W @ W.T - torch.eye(M + 1, dtype=torch.float64)).abs().max()) <= 2 * (2e-6 + (M + 3) * 2.0 ** -24)
    flat.grad.copy_(make_grad(e, n, SEED0 + M + 1))
    with pytest.raises(ValueError, match="max_directions"):
        ogd.add_direction(opt)


def test_state_round_trip_gives_identical_step_bits(tmp_path):
    from indic_cl_asr_amd import checkpoint, cl
    e, n = layout(False)
    fa, oa, A = with_basis(17)
    path = str(tmp_path / "ogd.pt")
    checkpoint.save_projection(oa, path)
    fb, ob, B = build(max_directions=20)
    assert checkpoint.load_projection(ob, path) is ob and ob.directions == 17
    assert torch.equal(bits(ob.basis[:17]), bits(oa.basis[:17]))
    g = make_grad(e, n, 101).cuda()
    for f, o in ((fa, A), (fb, B)):
        f.grad.copy_(g)
        o.step()
    assert_same(A, B, "after load_projection")
    assert torch.equal(bits(oa.dots64[:18]), bits(ob.dots64[:18]))
    other = cl.OGD(cl.FlatParams(torch.nn.Linear(3, 2).cuda()), 20)
    with pytest.raises(ValueError, match="different set of trainable tensors"):
        checkpoint.load_projection(other, path)
    narrower = cl.OGD(cl.FlatParams(Toy(big=False).cuda()), 20, scope=["mat"])
    with pytest.raises(ValueError, match="different scope"):
        checkpoint.load_projection(narrower, path)


def test_through_the_model():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    from test_gem_gpu import _batch
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny', languages=['hi', 'ta', 'bn'])).cuda().train()
    freeze_layer(m, 0)
    twin = copy.deepcopy(m)                                         # only its weights are used: it is fed gradients
    flat, flat_b = cl.FlatParams(m), cl.FlatParams(twin)
    scope = [name for name in flat.names if not cl._HEAD_RE.search(name)]      # the per-language heads stay out
    assert 0 < len(scope) < len(flat.names)
    ogd = cl.OGD(flat, 4, scope=scope)
    opt = cl.FusedAdamW(flat, lr=1e-3, projection=ogd)
    B = cl.FusedAdamW(flat_b, lr=1e-3)
    for lang, seed in (("hi", 1), ("ta", 2)):                       # the end of a language: its gradients become directions
        opt.zero_grad()
        batch, ids = _batch([lang] * 4, seed=seed)
        loss, _ = m.training_step(batch, ids, compute_wer=False)
        loss.backward()
        assert flat.grad.any() and ogd.add_direction(opt) and not flat.grad.any()
    assert ogd.directions == 2
    task, task_langs = _batch(["bn"] * 4, seed=3)
    loss, _ = m.training_step(task, task_langs, compute_wer=False)
    loss.backward()
    g, before = flat.grad.clone(), flat.theta.clone()
    opt.step()
    st = ogd.stats()
    print(st)
    assert set(st) == STAT_KEYS and st["directions"] == 2 and 0.0 < st["removed_fraction"] < 1.0
    assert not torch.equal(flat.theta, before)
    entries, n = list(flat.entries), flat.numel
    mask = scope_mask(entries, n, set(scope))
    V, G64, g64 = ogd.basis[:2, :n].double().cpu(), flat.grad.double().cpu(), g.double().cpu() * mask
    left, bound = (V @ G64).abs(), TOL * (V.abs() @ g64.abs())
    note("model: worst |<G, v_k>| / bound", float((left / bound).max()))
    note("model: removed_fraction", st["removed_fraction"])
    assert bool((left <= bound).all()) and bool(((V @ g64).abs() > bound).all())      # g itself was not orthogonal
    G = restate(g, rows_of(ogd), ogd.coefficients().tolist(), entries, set(scope), live_names(entries, g))
    assert torch.equal(bits(flat.grad), bits(G))
    for name, off, k, _ in entries:                                 # `.grad is None` where the task gave no gradient
        if not g[off:off + k].any():
            assert torch.equal(flat.theta[off:off + k], before[off:off + k]), name
    flat_b.grad.copy_(G)
    B.step()
    assert_same(opt, B, "task step")                                # weights, moments, counters and the fresh bf16 images
