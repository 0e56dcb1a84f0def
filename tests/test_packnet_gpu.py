"""PackNet inside the fused optimizer step (ia_adamw_step_segmented_packed, ia_grad_norm_packed), its pruning (ia_pack_prune) and
ia_pack_apply on the toy module of tests/test_optimizer_clip_gpu.py, and once through the model.

packed = v0, v1, v5, v7, v9, mat (1, 3, 65, 4096, 2 * 4096 + 5 and 65 x 63 elements: r == 0, a tail shorter than a float4, the
alignment gaps, an exact chunk, several chunks, the 2-D shadow view), frozen = v4, free = the rest; `idle` never receives a gradient.

The definition (include/indicasr.h): an element of a live packed tensor whose owner is train_owner takes exactly the plain rule,
every other one keeps the bit patterns of its weight and moments; the pruning is an exact selection.  So every check is bit for
bit against torch on the same data -- a plain optimizer fed the same gradient, kthvalue followed by <= -- except the measured
norm, which is held to the bound tests/test_optimizer_clip_gpu.py derives for ia_grad_norm."""
import math

import pytest
import torch

from test_optimizer_clip_gpu import TOL, Toy, make_grad, rel
from test_piggyback_gpu import bits_equal, where

pytestmark = pytest.mark.gpu

PACKED = ["v0", "v1", "v5", "v7", "v9", "mat"]
FROZEN = ["v4"]
FREE = {"v2", "v3", "v6", "v8", "idle"}


def build(big=False, packed=PACKED, prune=0.5, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    pn = cl.PackNet(flat, packed=packed, frozen=FROZEN, prune=prune)
    return flat, pn, cl.FusedAdamW(flat, lr=1e-3, masks=pn, **kw)


def plain(big=False, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    return flat, cl.FusedAdamW(flat, lr=1e-3, **kw)


def kind_masks(flat, pn):
    kinds = pn.kinds()
    return {k: where(flat.entries, flat.numel, {n for n, kk in kinds.items() if kk == k}) for k in ("free", "packed", "frozen")}


def write_owner(pn, P, seed, values=3):
    """owner = seeded draws from 0 .. values - 1 inside the packed tensors (interleaved inside every float4), 0 elsewhere."""
    g = torch.Generator().manual_seed(seed)
    o = torch.randint(0, values, (pn.flat.numel,), generator=g, dtype=torch.uint8).cuda()
    pn.owner.copy_(torch.where(P, o, torch.zeros_like(o)))


def randomize_state(opt, seed):
    """Moments as a run would have left them (exp_avg_sq >= 0), zero in the alignment gaps."""
    g = torch.Generator().manual_seed(seed)
    inside = where(opt.flat.entries, opt.flat.numel, set(opt.flat.names))
    zero = torch.zeros((), device="cuda")
    opt.exp_avg.copy_(torch.where(inside, torch.randn(opt.flat.numel, generator=g).cuda() * 0.1, zero))
    opt.exp_avg_sq.copy_(torch.where(inside, torch.rand(opt.flat.numel, generator=g).cuda() * 0.1, zero))


@pytest.fixture(scope="module")
def grads():
    """Toy(big=False): three gradients on the device (never modified); the second far below the clip threshold of 1."""
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=False))
    e, n = list(flat.entries), flat.numel
    return e, [make_grad(e, n, 101).cuda(), make_grad(e, n, 102, scale=1e-5).cuda(), make_grad(e, n, 103).cuda()]


def test_kinds_of_the_toy():
    flat, pn, _ = build()
    kinds = pn.kinds()
    assert [n for n, k in kinds.items() if k == "packed"] == sorted(PACKED, key=flat.names.index)
    assert {n for n, k in kinds.items() if k == "frozen"} == set(FROZEN)
    assert {n for n, k in kinds.items() if k == "free"} == FREE


# ---- 1. the first language trains everything that is free
@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_first_language_takes_the_plain_step_bit_for_bit(grads, max_norm):
    entries, gs = grads
    fa, pn, A = build(max_grad_norm=max_norm)
    fb, B = plain()
    K = kind_masks(fa, pn)
    idle = where(entries, fa.numel, {"idle"})
    moving = (K["packed"] | K["free"]) & ~idle
    still = K["frozen"] | idle
    before = fa.theta.clone()
    pn.begin_language("a", A)
    assert pn.train_owner == 0 and bits_equal(fa.theta, before)                # the first language keeps theta
    for step, g in enumerate(gs):
        fa.grad.copy_(g)
        A.step()
        ge = g * 1.0
        if max_norm is not None:
            st = A.stats()
            coef = torch.tensor(st["clip_coef"], dtype=torch.float32, device="cuda")
            assert float(coef) == st["clip_coef"] and (st["clip_coef"] < 1.0) == (step != 1)
            ge = ge * coef
        fb.grad.copy_(ge)
        B.step()
        for name, a, b in (("theta", fa.theta, fb.theta), ("exp_avg", A.exp_avg, B.exp_avg),
                           ("exp_avg_sq", A.exp_avg_sq, B.exp_avg_sq), ("shadow", A.shadow, B.shadow)):
            assert bits_equal(a[moving], b[moving]), (step, name)
        assert bits_equal(fa.theta[still], before[still]), step
        assert not A.exp_avg[still].any() and not A.exp_avg_sq[still].any(), step
        assert bits_equal(A.shadow, fa.theta.to(torch.bfloat16)), step
    assert not torch.equal(fa.theta[K["packed"]], before[K["packed"]])         # they did move
    steps = dict(zip(fa.names, A.seg_step.tolist()))
    assert all(steps[n] == (0 if n in FROZEN or n == "idle" else 3) for n in fa.names), steps
    if max_norm is not None:
        assert A.stats()["clipped_steps"] == 2


# ---- 2. a mixed owner map
def mixed_run(entries, g, train_owner, clip=False):
    """A (PackNet, owners 0 / 1 / 2 interleaved, -0.0f planted where nothing may move) beside a plain optimizer that starts from
    the same weights and moments and is fed the same gradient.  Returns everything the checks need."""
    fa, pn, A = build(max_grad_norm=1.0 if clip else None)
    fb, B = plain()
    K = kind_masks(fa, pn)
    P = K["packed"]
    write_owner(pn, P, seed=31)
    randomize_state(A, seed=32)
    mine = P & (pn.owner.to(torch.int32) == train_owner)
    other = P & ~mine
    plant = other & (torch.rand(fa.numel, generator=torch.Generator().manual_seed(33)).cuda() < 0.25)
    assert int(plant.sum()) > 100
    with torch.no_grad():
        for t in (fa.theta, A.exp_avg, A.exp_avg_sq):
            t[plant] = -0.0
    fb.theta.copy_(fa.theta); B.exp_avg.copy_(A.exp_avg); B.exp_avg_sq.copy_(A.exp_avg_sq)
    start = {"theta": fa.theta.clone(), "exp_avg": A.exp_avg.clone(), "exp_avg_sq": A.exp_avg_sq.clone()}
    pn.train_owner = train_owner
    fa.grad.copy_(g)
    A.step()
    return fa, pn, A, fb, B, K, mine, other, plant, start


def test_mixed_owner_map_moves_only_the_trained_owner(grads):
    entries, (g, _, _) = grads
    fa, pn, A, fb, B, K, mine, other, plant, start = mixed_run(entries, g, train_owner=2)
    fb.grad.copy_(g)
    B.step()
    now = {"theta": fa.theta, "exp_avg": A.exp_avg, "exp_avg_sq": A.exp_avg_sq}
    ref = {"theta": fb.theta, "exp_avg": B.exp_avg, "exp_avg_sq": B.exp_avg_sq}
    for owner in (0, 1, 2):                                                    # every float4 mixes them
        assert int((pn.owner[K["packed"]] == owner).sum()) > 1000
    for name in now:
        assert bits_equal(now[name][mine], ref[name][mine]), name             # owner 2: the plain rule
        assert not torch.equal(now[name][mine], start[name][mine]), name
        assert bits_equal(now[name][other], start[name][other]), name         # everybody else: the starting bit pattern
        assert bits_equal(now[name][K["free"]], ref[name][K["free"]]), name
        assert bits_equal(now[name][K["frozen"]], start[name][K["frozen"]]), name
    minus_zero = torch.tensor(-0.0).view(torch.int32).item()
    assert bool((fa.theta[plant].view(torch.int32) == minus_zero).all())
    assert bool((A.exp_avg[plant].view(torch.int32) == minus_zero).all())
    assert bits_equal(A.shadow, fa.theta.to(torch.bfloat16))                   # -0.0f included
    assert bool((A.shadow[plant].view(torch.int16) == torch.tensor(-0.0, dtype=torch.bfloat16).view(torch.int16).item()).all())
    steps = dict(zip(fa.names, A.seg_step.tolist()))
    assert all(steps[n] == (0 if n in FROZEN or n == "idle" else 1) for n in fa.names), steps


def test_train_owner_minus_one_moves_no_packed_element(grads):
    entries, (g, _, _) = grads
    fa, pn, A, fb, B, K, mine, other, plant, start = mixed_run(entries, g, train_owner=-1)
    assert int(mine.sum()) == 0
    P = K["packed"]
    assert bits_equal(fa.theta[P], start["theta"][P]) and bits_equal(A.exp_avg[P], start["exp_avg"][P])
    assert bits_equal(A.exp_avg_sq[P], start["exp_avg_sq"][P])
    assert not torch.equal(fa.theta[K["free"]], start["theta"][K["free"]])     # the free tensors still train
    assert bits_equal(A.shadow, fa.theta.to(torch.bfloat16))
    fresh_flat, fresh, opt = build()                                           # and so does a PackNet nobody has opened
    assert fresh.train_owner == -1
    before = fresh_flat.theta.clone()
    fresh_flat.grad.copy_(g)
    opt.step()
    P = kind_masks(fresh_flat, fresh)["packed"]
    assert bits_equal(fresh_flat.theta[P], before[P])


# ---- 3. the clip norm is that of the consumed gradient
def test_clip_norm_is_that_of_the_consumed_gradient(grads):
    entries, (g, _, _) = grads
    fa, pn, A, fb, B, K, mine, other, plant, start = mixed_run(entries, g, train_owner=2, clip=True)
    consumed = torch.where(mine | K["free"], g, torch.zeros_like(g)).double().cpu()
    want = consumed.norm().item()
    raw = g.double().cpu().norm().item()
    st = A.stats()
    print("grad_norm", st["grad_norm"], "float64 consumed", want, "rel", rel(st["grad_norm"], want), "raw", raw)
    assert rel(st["grad_norm"], want) <= TOL
    assert rel(raw, want) > 0.1                                                # the raw norm would have failed
    assert rel(st["clip_coef"], 1.0 / (want + 1e-6)) <= TOL and st["clipped_steps"] == 1
    per = A.grad_norms()
    for name, o, k, _ in entries:
        w = consumed[o:o + k].norm().item()
        assert per[name] == 0.0 if w == 0.0 else rel(per[name], w) <= TOL, (name, per[name], w)
    assert per["v4"] == 0.0 and per["idle"] == 0.0
    coef = torch.tensor(st["clip_coef"], dtype=torch.float32, device="cuda")
    fb.grad.copy_((g * 1.0) * coef)
    B.step()
    assert bits_equal(fa.theta[mine | K["free"]], fb.theta[mine | K["free"]])  # ... and the coefficient is applied


# ---- 4. / 5. the pruning against torch
def prune_reference(entries, names, theta, owner, fraction, task):
    """Per packed tensor: kthvalue of |theta| over the free elements at floor(fraction * n), then <=.  In place on CPU copies;
    returns the counts {name: (released, newly owned)} and the cutoffs.  `fraction` is the float the C entry receives."""
    f32 = float(torch.tensor(fraction, dtype=torch.float32))
    counts, cutoffs = {}, {}
    for name, o, k, _ in entries:
        if name not in names:
            continue
        t, ow = theta[o:o + k], owner[o:o + k]
        F = ow == 0
        n = int(F.sum())
        r = math.floor(f32 * n)
        release = torch.zeros_like(F)
        if r > 0:
            cutoffs[name] = torch.kthvalue(t[F].abs(), r).values
            release = F & (t.abs() <= cutoffs[name])
        t[release] = 0.0
        ow[F & ~release] = task
        counts[name] = (int(release.sum()), n - int(release.sum()))
    return counts, cutoffs


def check_prune(fa, pn, A, names, fraction, task, P):
    """Run pn.prune against prune_reference from the state as it is; every output is compared bit for bit."""
    entries = list(fa.entries)
    theta, owner = fa.theta.cpu().clone(), pn.owner.cpu().clone()
    randomize_state(A, seed=40 + task)
    m0, v0 = A.exp_avg.clone(), A.exp_avg_sq.clone()
    A.seg_step.fill_(7)
    counts, cutoffs = prune_reference(entries, names, theta, owner, fraction, task)
    pn.prune(A, fraction=fraction)
    assert torch.equal(pn.owner.cpu(), owner)
    assert bits_equal(fa.theta.cpu(), theta)
    assert bits_equal(A.exp_avg[P], torch.zeros_like(m0[P])) and bits_equal(A.exp_avg_sq[P], torch.zeros_like(v0[P]))
    assert bits_equal(A.exp_avg[~P], m0[~P]) and bits_equal(A.exp_avg_sq[~P], v0[~P])
    assert bits_equal(A.shadow, fa.theta.to(torch.bfloat16))
    got = pn.seg_counts.tolist()
    for k, (name, _, _, _) in enumerate(entries):
        assert tuple(got[k]) == counts.get(name, (0, 0)), (name, got[k])
    assert A.seg_step.tolist() == [0 if n in names else 7 for n in fa.names]
    assert pn.phase == "retrain" and pn.train_owner == task
    return counts, cutoffs


def plant_ties(fa, name, fraction):
    """Duplicates of the tensor's cutoff magnitude with both signs, on both sides of its first chunk boundary."""
    _, o, k, _ = [e for e in fa.entries if e[0] == name][0]
    t = fa.theta[o:o + k]
    x = torch.kthvalue(t.abs().cpu(), math.floor(fraction * k)).values.cuda()
    with torch.no_grad():
        for j, i in enumerate(range(4092, 4100)):
            t[i] = x if j % 2 else -x
    return x


@pytest.mark.parametrize("fraction", [0.5, 0.0, 0.999])
def test_prune_against_torch(fraction):
    fa, pn, A = build()
    P = kind_masks(fa, pn)["packed"]
    x = plant_ties(fa, "v9", 0.5)
    pn.begin_language("a", A)
    counts, cutoffs = check_prune(fa, pn, A, PACKED, fraction, 1, P)
    sizes = {e[0]: e[2] for e in fa.entries}
    assert counts["v0"] == (0, 1)                                              # r == 0: nothing released
    if fraction == 0.0:
        assert all(counts[n] == (0, sizes[n]) for n in PACKED)                 # nothing released, everything owned
        assert bool((pn.owner[P] == 1).all())
    if fraction == 0.5:
        assert cutoffs["v9"] == x.cpu()                                        # the planted ties sit AT the cutoff ...
        _, o, k, _ = [e for e in fa.entries if e[0] == "v9"][0]
        assert not fa.theta[o + 4092:o + 4100].any() and not pn.owner[o + 4092:o + 4100].any()      # ... and all go, both signs
        assert counts["v9"][0] > math.floor(0.5 * k)                           # more than r were released
        assert counts["v1"] == (1, 2) and counts["v7"] == (2048, 2048)
    if fraction == 0.999:
        assert counts["v7"] == (4091, 5) and counts["v1"] == (2, 1)


def test_second_prune_counts_free_elements_only():
    fa, pn, A = build()
    P = kind_masks(fa, pn)["packed"]
    pn.begin_language("a", A)
    check_prune(fa, pn, A, PACKED, 0.5, 1, P)
    pn.finish_language()
    pn.begin_language("b", A)
    assert pn.tasks == {"a": 1, "b": 2} and pn.train_owner == 0
    free = P & (pn.owner == 0)
    assert not fa.theta[free].any()                                            # what a released
    g = torch.Generator().manual_seed(50)
    with torch.no_grad():                                                      # b's training, in short; and owned weights far
        fa.theta[free] = torch.randn(int(free.sum()), generator=g).cuda()      # below every free magnitude
        owned = P & (pn.owner == 1)
        fa.theta[owned] = fa.theta[owned] * 1e-12
    owned_before = fa.theta[owned].clone()
    counts, _ = check_prune(fa, pn, A, PACKED, 0.5, 2, P)
    assert bits_equal(fa.theta[owned], owned_before) and bool((pn.owner[owned] == 1).all())
    assert counts["v7"] == (1024, 1024) and counts["v0"] == (0, 0)             # n counts the free elements only
    assert counts["v1"] == (0, 1)                                              # one free element: r == 0
    assert sorted(pn.owner[P].unique().tolist()) == [0, 1, 2]


def test_prune_with_more_than_2048_chunks():
    names = PACKED + ["big"]
    fa, pn, A = build(big=True, packed=names)
    assert fa.chunk_table.shape[0] > 2048
    P = kind_masks(fa, pn)["packed"]
    pn.begin_language("a", A)
    counts, _ = check_prune(fa, pn, A, names, 0.5, 1, P)
    big = [e for e in fa.entries if e[0] == "big"][0][2]
    assert counts["big"][0] >= big // 2 and sum(counts["big"]) == big            # r, and whatever ties the cutoff has
    with torch.no_grad():
        fa.theta[P] = 7.0
    pn.finish_language()                                                       # base <- theta
    with torch.no_grad():
        fa.theta[P] = -3.0
        A.shadow[P] = -3.0
    pn.activate("a")                                                           # ia_pack_apply over the same table
    want = torch.where(P, torch.where(pn.owner == 1, pn.base.flat, torch.zeros_like(fa.theta)), fa.theta)
    assert bits_equal(fa.theta, want) and bits_equal(A.shadow, want.to(torch.bfloat16))


# ---- 6. zero forgetting
def test_zero_forgetting_over_two_languages():
    from indic_cl_asr_amd import cl
    fa, pn, A = build()
    K = kind_masks(fa, pn)
    P = K["packed"]
    entries = list(fa.entries)
    seeds = iter(range(200, 300))

    def step():
        A.zero_grad()
        fa.grad.copy_(make_grad(entries, fa.numel, next(seeds)).cuda())
        A.step()

    pn.begin_language("a", A)
    step(); step()
    pn.prune(A)
    released_a = P & (pn.owner == 0)
    step(); step()
    assert not fa.theta[released_a].any()
    pn.finish_language()
    at_a = (fa.theta.clone(), A.shadow.clone())
    usage = pn.usage()
    assert all(abs(u["owned"]["a"] + u["free"] - 1.0) < 1e-12 for u in usage.values())

    pn.begin_language("b", A)
    assert bits_equal(fa.theta, at_a[0])                                       # owner >= 1 ? base : 0 is what a left
    assert not A.exp_avg[~K["frozen"]].any() and int(A.seg_step.sum()) == 0
    owned_a = P & (pn.owner == 1)
    keep = fa.theta[owned_a].clone()
    for _ in range(2):
        step()
        assert bits_equal(fa.theta[owned_a], keep)
    assert bool(fa.theta[released_a].ne(0).any())                              # b trains what a released
    pn.prune(A)
    released_b = P & (pn.owner == 0)
    assert 0 < int(released_b.sum()) < int(released_a.sum())
    assert bits_equal(fa.theta[owned_a], keep)
    for _ in range(2):
        step()
        assert bits_equal(fa.theta[owned_a], keep)
        assert bits_equal(fa.theta[released_b], torch.zeros_like(fa.theta[released_b]))
    assert not torch.equal(fa.theta[K["free"]], at_a[0][K["free"]])            # the heads moved on
    pn.finish_language()
    at_b = (fa.theta.clone(), A.shadow.clone())

    pn.activate("a")
    assert bits_equal(fa.theta, at_a[0]) and bits_equal(A.shadow, at_a[1]) and pn.current == "a"
    pn.activate("b")
    assert bits_equal(fa.theta, at_b[0]) and bits_equal(A.shadow, at_b[1]) and pn.current == "b"
    A.zero_grad()
    fa.grad.copy_(make_grad(entries, fa.numel, 299).cuda())
    A.step()                                                                   # no language open: no packed weight moves
    assert bits_equal(fa.theta[P], at_b[0][P])
    assert pn.languages() == ["a", "b"] and 0.0 < pn.free_fraction() < 0.5


# ---- 8. the report
def test_usage_matches_a_bincount_of_the_owner_map():
    fa, pn, A = build()
    P = kind_masks(fa, pn)["packed"]
    write_owner(pn, P, seed=61, values=3)
    pn.tasks = {"a": 1, "b": 2}
    usage = pn.usage()
    assert list(usage) == sorted(PACKED, key=fa.names.index)
    total_free = 0
    for name, o, k, _ in fa.entries:
        if name not in PACKED:
            continue
        count = torch.bincount(pn.owner[o:o + k].long(), minlength=3).tolist()
        u = usage[name]
        assert list(u["owned"]) == ["a", "b"]
        assert u["free"] == count[0] / k and u["owned"]["a"] == count[1] / k and u["owned"]["b"] == count[2] / k
        assert abs(u["free"] + sum(u["owned"].values()) - 1.0) < 1e-12
        total_free += count[0]
    assert pn.free_fraction() == total_free / int(P.sum())


# ---- 7. through the model once
def test_through_the_model_two_languages():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    from test_si_gpu import _batch
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny')).cuda().train()
    freeze_layer(m, 0)
    flat = cl.FlatParams(m)
    pn = cl.PackNet(flat, prune=0.5)
    opt = cl.FusedAdamW(flat, lr=1e-3, masks=pn)

    def train(batch, langs, steps):
        m.train()
        for _ in range(steps):
            opt.zero_grad()
            loss, _ = m.training_step(batch, langs, compute_wer=False)
            loss.backward()
            opt.step()

    def evaluate(batch, langs):
        m.eval()
        with torch.no_grad():
            loss, _ = m.training_step(batch, langs, compute_wer=False)
        return float(loss)

    hi, ta = _batch(['hi'] * 4, seed=1), _batch(['ta'] * 4, seed=2)
    pn.begin_language('hi', opt)
    train(*hi, steps=2)
    pn.prune(opt)
    train(*hi, steps=1)
    pn.finish_language()
    snap_theta = flat.theta.clone()
    snap_buffers = {n: b.clone() for n, b in m.named_buffers()}
    hi_1, hi_2 = evaluate(*hi), evaluate(*hi)
    free_after_hi = pn.free_fraction()
    assert 0.0 < free_after_hi < 1.0

    pn.begin_language('ta', opt)
    train(*ta, steps=2)
    pn.prune(opt)
    train(*ta, steps=1)
    pn.finish_language()
    assert any(not torch.equal(b, snap_buffers[n]) for n, b in m.named_buffers())      # BatchNorm statistics moved in train mode
    assert not torch.equal(flat.theta, snap_theta)
    assert 0.0 < pn.free_fraction() < free_after_hi
    ta_own = evaluate(*ta)

    pn.activate('hi')
    assert bits_equal(flat.theta, snap_theta)
    assert bits_equal(opt.shadow, snap_theta.to(torch.bfloat16))
    for n, b in m.named_buffers():
        assert torch.equal(b, snap_buffers[n]), n
    hi_3 = evaluate(*hi)
    print("hi loss before", hi_1, hi_2, "after ta and activate('hi')", hi_3)
    if hi_1 == hi_2:
        assert hi_3 == hi_1
    else:                                                                     # run-to-run differences of the forward itself
        assert min(abs(hi_3 - hi_1), abs(hi_3 - hi_2)) <= abs(hi_1 - hi_2)
    pn.activate('ta')
    ta_again = evaluate(*ta)
    print("ta loss at finish", ta_own, "after activate('ta')", ta_again)
    assert ta_again == ta_again and pn.languages() == ['hi', 'ta'] and pn.current == 'ta'
