"""Piggyback masks inside the fused optimizer step (ia_adamw_step_segmented_masked, ia_mask_pack, ia_mask_apply) on the toy module
of tests/test_optimizer_clip_gpu.py, and once through the model.

masked = mat, v1, v5, v7, v9 (65 x 63, 3, 65, 4096 and 2 * 4096 + 5 elements: the 2-D shadow view, a tail shorter than a float4, the
alignment gaps, the chunk boundary, a tensor of several chunks), frozen = v0, v4, free = the rest; `idle` never receives a gradient.

The definition (include/indicasr.h), per element of a live masked tensor, every product rounded to fp32 on its own:
    ge = g * grad_scale [* coef];  gs = ge * base;  score, m, v = AdamW(score, gs; weight decay 0);  theta = score >= thr ? base : +0
so every check is bit for bit: the scores and moments against a plain optimizer without weight decay whose weights ARE the scores
and whose gradient is gs built with one torch op per rounding; theta and the bf16 image against torch.where on those scores; a
free tensor against the plain optimizer fed the same gradient."""
import numpy as np
import pytest
import torch

from test_optimizer_clip_gpu import Toy, assert_same, make_grad

pytestmark = pytest.mark.gpu

MASKED = ["mat", "v1", "v5", "v7", "v9"]
FROZEN = ["v0", "v4"]
THR, INIT = 5e-3, 1e-2


def build(big=False, masked=MASKED, pb_kw=None, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    pb = cl.Piggyback(flat, masked=masked, frozen=FROZEN, **(pb_kw or {}))
    return flat, pb, cl.FusedAdamW(flat, lr=1e-3, masks=pb, **kw)


def plain(big=False, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=big).cuda())
    return flat, cl.FusedAdamW(flat, lr=1e-3, **kw)


def where(entries, numel, names):
    """Boolean flat mask on the device: True inside the named tensors."""
    m = torch.zeros(numel, dtype=torch.bool, device="cuda")
    for name, off, k, _ in entries:
        if name in names:
            m[off:off + k] = True
    return m


def kind_masks(flat, pb):
    e, n = flat.entries, flat.numel
    kinds = pb.kinds()
    return {k: where(e, n, {name for name, kk in kinds.items() if kk == k}) for k in ("free", "masked", "frozen")}


def seg_ids(flat, names):
    return [i for i, e in enumerate(flat.entries) if e[0] in names]


def bits_equal(a, b):
    """Same bit patterns (torch.equal alone would let -0.0 pass for +0.0)."""
    view = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and torch.equal(a.view(view), b.view(view))


def masked_weights(pb):
    """(theta, bf16 image) the scores define, as flat tensors: base where score >= threshold, +0 elsewhere."""
    thr = torch.tensor(pb.threshold, dtype=torch.float32, device="cuda")
    want = torch.where(pb.scores.flat >= thr, pb.base.flat, torch.zeros_like(pb.base.flat))
    return want, want.to(torch.bfloat16)


def write_scores(pb, M, seed, spread=2e-3):
    """scores = thr + U(-spread, spread) inside the masked tensors (0 elsewhere), seeded."""
    g = torch.Generator().manual_seed(seed)
    u = (torch.rand(pb.flat.numel, generator=g) * 2.0 - 1.0) * spread
    s = (torch.tensor(pb.threshold, dtype=torch.float32) + u).cuda()
    pb.scores.flat.copy_(torch.where(M, s, torch.zeros_like(s)))


@pytest.fixture(scope="module")
def grads():
    """Toy(big=False): three gradients on the device (never modified); the second far below the clip threshold of 1."""
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy(big=False))
    e, n = list(flat.entries), flat.numel
    return e, [make_grad(e, n, 101).cuda(), make_grad(e, n, 102, scale=1e-5).cuda(), make_grad(e, n, 103).cuda()]


def test_kinds_of_the_toy():
    flat, pb, _ = build()
    kinds = pb.kinds()
    assert [n for n, k in kinds.items() if k == "masked"] == sorted(MASKED, key=flat.names.index)
    assert {n for n, k in kinds.items() if k == "frozen"} == set(FROZEN)
    assert {n for n, k in kinds.items() if k == "free"} == {"v2", "v3", "v6", "v8", "idle"}


@pytest.mark.parametrize("max_norm", [None, 1.0])
def test_free_tensors_take_the_plain_step_bit_for_bit(grads, max_norm):
    entries, gs = grads
    fa, pb, A = build(max_grad_norm=max_norm)
    fb, B = plain(max_grad_norm=max_norm)
    F = kind_masks(fa, pb)["free"]
    free_ids = seg_ids(fa, {n for n, k in pb.kinds().items() if k == "free"})
    for step, g in enumerate(gs):
        fa.grad.copy_(g); fb.grad.copy_(g)
        A.step(); B.step()
        for name, a, b in (("theta", fa.theta, fb.theta), ("exp_avg", A.exp_avg, B.exp_avg),
                           ("exp_avg_sq", A.exp_avg_sq, B.exp_avg_sq), ("shadow", A.shadow, B.shadow)):
            assert torch.equal(a[F], b[F]), (step, name)
        assert torch.equal(A.seg_step[free_ids], B.seg_step[free_ids]), step
    assert not torch.equal(fa.theta[F], pb.base.flat[F])                     # they did move
    if max_norm is not None:
        sa, sb = A.stats(), B.stats()
        assert sa == sb and sa["clipped_steps"] == 2                          # the norm is measured exactly as without masks
    steps = dict(zip(fa.names, A.seg_step.tolist()))
    assert all(steps[n] == (0 if n in FROZEN or n == "idle" else 3) for n in fa.names), steps


def masked_rule_run(entries, g, steps, clip, scores_seed=None):
    """A (masks) beside the twin T: a plain optimizer without weight decay whose theta is the scores, fed gs.  Checks the rule
    after every step; returns (A's FlatParams, pb, A, the masked-element mask, on-bits before the first step)."""
    fa, pb, A = build(max_grad_norm=1.0 if clip else None)
    ft, T = plain(weight_decay=0.0)
    M = kind_masks(fa, pb)["masked"]
    base = pb.base.flat
    if scores_seed is not None:
        write_scores(pb, M, scores_seed)
    ft.theta.copy_(pb.scores.flat)
    on_before = pb.scores.flat >= torch.tensor(THR, dtype=torch.float32, device="cuda")
    for step in range(steps):
        fa.grad.copy_(g)
        A.step()
        ge = g * 1.0
        if clip:
            st = A.stats()
            coef = torch.tensor(st["clip_coef"], dtype=torch.float32, device="cuda")
            assert float(coef) == st["clip_coef"] and st["clip_coef"] < 1.0
            ge = ge * coef
        ft.grad.copy_(ge * base)
        T.step()
        assert torch.equal(pb.scores.flat[M], ft.theta[M]), step
        assert torch.equal(A.exp_avg[M], T.exp_avg[M]) and torch.equal(A.exp_avg_sq[M], T.exp_avg_sq[M]), step
        want, want16 = masked_weights(pb)
        assert bits_equal(fa.theta[M], want[M]), step
        assert bits_equal(A.shadow[M], want16[M]), step
    return fa, pb, A, M, on_before


@pytest.mark.parametrize("clip", [False, True])
def test_masked_rule_bit_for_bit(grads, clip):
    entries, (g, _, _) = grads
    fa, pb, A, M, on_before = masked_rule_run(entries, g, 8, clip)
    assert bool(on_before[M].all())                                           # init >= threshold: every bit starts on
    off = float((pb.scores.flat[M] < THR).float().mean())
    print("fraction of masked elements off after step 8:", off, "clip", clip)
    assert 0.2 <= off <= 0.8                                                  # the weights really are masked
    on = pb.sparsity()
    assert set(on) == set(MASKED)
    for name, o, k, _ in fa.entries:
        if name in MASKED:
            assert on[name] == float((pb.scores.flat[o:o + k] >= THR).sum()) / k, name
    Z = kind_masks(fa, pb)["frozen"]
    assert bits_equal(fa.theta[Z], pb.base.flat[Z])
    assert A.param_groups[0]["weight_decay"] == 1e-2                          # ... which the scores ignored: the twin has none


def test_bits_switch_both_ways_in_one_step(grads):
    entries, (g, _, _) = grads
    fa, pb, A, M, on_before = masked_rule_run(entries, g, 1, clip=False, scores_seed=7)
    on_after = pb.scores.flat >= THR
    went_off = int((on_before & ~on_after & M).sum())
    came_on = int((~on_before & on_after & M).sum())
    print("on -> off", went_off, "off -> on", came_on, "of", int(M.sum()))
    assert went_off > 0 and came_on > 0
    back = ~on_before & on_after & M
    assert bits_equal(fa.theta[back], pb.base.flat[back])
    assert not fa.theta[on_before & ~on_after & M].any()


def test_frozen_and_idle_tensors(grads):
    entries, (g0, _, g2) = grads
    fa, pb, A = build()
    K = kind_masks(fa, pb)
    idle = where(entries, fa.numel, {"idle"})
    gaps = ~where(entries, fa.numel, set(fa.names))
    assert g0[K["frozen"]].ne(0).all()                                        # autograd did give them a gradient
    with torch.no_grad():                                                     # the bf16 image made at construction is stale now
        fa.theta[K["frozen"] | idle] += 0.5
    before = fa.theta.clone()
    assert not torch.equal(A.shadow[K["frozen"] | idle], before.to(torch.bfloat16)[K["frozen"] | idle])
    for g in (g0, g2):
        fa.grad.copy_(g)
        A.step()
    Z = K["frozen"]
    assert torch.equal(fa.theta[Z], before[Z]) and not A.exp_avg[Z].any() and not A.exp_avg_sq[Z].any()
    steps = dict(zip(fa.names, A.seg_step.tolist()))
    assert all(steps[n] == 0 for n in FROZEN + ["idle"]) and all(steps[n] == 2 for n in MASKED)
    assert torch.equal(fa.theta[idle], before[idle])
    assert bits_equal(A.shadow[Z | idle], fa.theta.to(torch.bfloat16)[Z | idle])
    assert not pb.scores.flat[~K["masked"]].any()                             # scores live inside masked tensors only
    assert not pb.scores.flat[gaps].any() and not fa.theta[gaps].any()
    pb.save_language("x")
    bits = pb.records["x"]["bits"].cpu().numpy().view(np.uint8)
    unpacked = torch.from_numpy(np.unpackbits(bits, bitorder="little").astype(bool)).cuda()
    assert not unpacked[gaps].any() and not unpacked[~K["masked"]].any() and unpacked[K["masked"]].any()


def test_nonfinite_gradient_skips_the_step(grads):
    entries, (g0, _, g2) = grads
    fa, pb, A = build(skip_nonfinite=True)
    fa.grad.copy_(g0)
    A.step()
    keep = {"scores": pb.scores.flat, "theta": fa.theta, "exp_avg": A.exp_avg, "exp_avg_sq": A.exp_avg_sq,
            "seg_step": A.seg_step, "shadow": A.shadow}
    before = {k: v.clone() for k, v in keep.items()}
    off = [e for e in entries if e[0] == "v9"][0][1]
    fa.grad.copy_(g2)
    fa.grad[off + 4100] = float("nan")                                       # data in a gradient buffer: nothing here faults the device
    A.step()
    for k, v in keep.items():
        assert torch.equal(v, before[k]), k
    assert int(A.seg_active.abs().sum()) == 0 and A.stats()["skipped_steps"] == 1
    fa.grad.copy_(g2)
    A.step()
    assert not torch.equal(pb.scores.flat, before["scores"]) and A.stats()["skipped_steps"] == 1


def packed_reference(pb, M):
    on = (pb.scores.flat >= THR) & M
    return torch.from_numpy(np.packbits(on.cpu().numpy(), bitorder="little").view(np.int64).copy()).cuda(), on


def test_pack_and_apply(grads):
    from indic_cl_asr_amd import _lib
    entries, _ = grads
    fa, pb, A = build()
    K = kind_masks(fa, pb)
    M = K["masked"]
    inside = where(entries, fa.numel, set(fa.names))                          # no kernel writes the alignment gaps
    gen = torch.Generator().manual_seed(3)
    expect = {}
    for lang, seed in (("a", 21), ("b", 22)):
        write_scores(pb, M, seed)
        with torch.no_grad():
            fa.theta[K["free"]] = torch.randn(int(K["free"].sum()), generator=gen).cuda()
        want_bits, on = packed_reference(pb, M)
        # the entry itself, with the per-tensor counts
        bits = torch.full((fa.numel // 64,), -1, dtype=torch.int64, device="cuda")
        kept = torch.full((len(entries),), 99, dtype=torch.int32, device="cuda")
        st = _lib.lib().ia_mask_pack(_lib.ptr(pb.scores.flat), _lib.ptr(fa.chunk_table), fa.chunk_table.shape[0],
                                     _lib.ptr(pb.seg_kind), len(entries), THR, _lib.ptr(bits), bits.numel(), _lib.ptr(kept),
                                     _lib.stream_ptr())
        assert st == 0
        assert torch.equal(bits, want_bits)
        assert kept.tolist() == [int(on[o:o + k].sum()) for _, o, k, _ in entries]
        assert 0 < int(on.sum()) < int(M.sum())
        pb.save_language(lang)
        assert torch.equal(pb.records[lang]["bits"], want_bits) and pb.current == lang
        theta = torch.where(M, masked_weights(pb)[0], fa.theta)
        expect[lang] = (theta.clone(), fa.theta[K["free"]].clone())
    assert not torch.equal(pb.records["a"]["bits"], pb.records["b"]["bits"]) and pb.languages() == ["a", "b"]
    for lang in ("a", "b", "a", "b", "a"):
        with torch.no_grad():                                                 # noise over everything apply has to rewrite
            fa.theta[M | K["free"]] = torch.randn(int((M | K["free"]).sum()), generator=gen).cuda()
            A.shadow.copy_(torch.where(inside, torch.randn(fa.numel, generator=gen).cuda(), torch.zeros((), device="cuda")))
        pb.activate(lang)
        want, free = expect[lang]
        assert bits_equal(fa.theta[M], want[M]), lang
        assert torch.equal(fa.theta[K["free"]], free), lang                   # from the snapshot
        assert bits_equal(fa.theta, want), lang
        assert bits_equal(A.shadow, fa.theta.to(torch.bfloat16)), lang        # every tensor: free, frozen and idle too
        assert pb.current == lang
    with pytest.raises(ValueError, match="unknown language"):
        pb.activate("c")
    with pytest.raises(RuntimeError, match="begin_language"):
        pb.save_language()                                                    # the scores are b's, theta shows a
    pb.begin_language("c", A)
    assert bool((pb.scores.flat[M] == INIT).all()) and bits_equal(fa.theta[M], pb.base.flat[M]) and pb.current == "c"
    assert bits_equal(A.shadow, fa.theta.to(torch.bfloat16))
    pb.save_language()
    assert pb.languages() == ["a", "b", "c"] and int(pb.records["c"]["bits"].ne(0).sum()) > 0


def test_more_than_2048_chunks():
    from indic_cl_asr_amd import cl
    masked = MASKED + ["big"]
    fa, pb, A = build(big=True, masked=masked)
    ft, T = plain(big=True, weight_decay=0.0)
    assert fa.chunk_table.shape[0] > 2048
    M = kind_masks(fa, pb)["masked"]
    write_scores(pb, M, 9)
    ft.theta.copy_(pb.scores.flat)
    on_before = pb.scores.flat >= THR
    g = make_grad(list(fa.entries), fa.numel, 101).cuda()
    fa.grad.copy_(g)
    A.step()
    ft.grad.copy_((g * 1.0) * pb.base.flat)
    T.step()
    assert torch.equal(pb.scores.flat[M], ft.theta[M])
    assert torch.equal(A.exp_avg[M], T.exp_avg[M]) and torch.equal(A.exp_avg_sq[M], T.exp_avg_sq[M])
    want, want16 = masked_weights(pb)
    assert bits_equal(fa.theta[M], want[M]) and bits_equal(A.shadow[M], want16[M])
    on_after = pb.scores.flat >= THR
    assert int((on_before & ~on_after & M).sum()) > 0 and int((~on_before & on_after & M).sum()) > 0
    pb.save_language("x")
    want_bits, on = packed_reference(pb, M)
    assert torch.equal(pb.records["x"]["bits"], want_bits)
    theta = fa.theta.clone()
    with torch.no_grad():
        fa.theta[M] = 7.0
        A.shadow[M] = 7.0
    pb.activate("x")
    assert bits_equal(fa.theta, theta) and bits_equal(A.shadow, theta.to(torch.bfloat16))
    big = [e for e in fa.entries if e[0] == "big"][0]
    assert pb.sparsity()["big"] == float(on[big[1]:big[1] + big[2]].sum()) / big[2]


def test_through_the_model_two_languages():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    from test_si_gpu import _batch
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny')).cuda().train()
    freeze_layer(m, 0)
    flat = cl.FlatParams(m)

    def train(opt, batch, langs, steps):
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
    train(cl.FusedAdamW(flat, lr=1e-3), *hi, steps=2)                          # the backbone's own language, plainly
    pb = cl.Piggyback(flat, init=6e-3)
    opt = cl.FusedAdamW(flat, lr=1e-3, masks=pb)
    pb.save_language('hi')
    assert all(v == 1.0 for v in pb.sparsity().values())                      # the backbone's language: every bit on
    snap_theta = flat.theta.clone()
    snap_buffers = {n: b.clone() for n, b in m.named_buffers()}
    base = pb.base.flat.clone()
    hi_1, hi_2 = evaluate(*hi), evaluate(*hi)
    ta_all_on = evaluate(*ta)

    pb.begin_language('ta', opt)
    train(opt, *ta, steps=3)
    pb.save_language('ta')
    on = pb.sparsity()
    off = 1.0 - sum(on[n] * flat.params[flat.names.index(n)].numel() for n in on) / \
        sum(flat.params[flat.names.index(n)].numel() for n in on)
    print("fraction of masked weights off after three steps on ta:", off)
    # Adam's first steps move a score by about lr = 1e-3 each, against the sign of its gradient: from 6e-3 the scores whose gradient
    # kept its sign are below 5e-3 after two steps -- about half of those that received one (unused embedding rows receive none)
    assert 0.05 < off < 0.95
    assert torch.equal(pb.base.flat, base)                                    # the backbone never moves
    kinds = pb.kinds()
    for n, k in kinds.items():
        if k == "frozen":
            assert torch.equal(flat.params_dict()[n], pb.base[n]), n
    assert any(not torch.equal(b, snap_buffers[n]) for n, b in m.named_buffers())      # BatchNorm statistics moved in train mode

    pb.activate('hi')
    assert bits_equal(flat.theta, snap_theta)
    assert bits_equal(opt.shadow, snap_theta.to(torch.bfloat16))
    for n, k in kinds.items():
        if k == "free":
            assert torch.equal(flat.params_dict()[n], pb.records['hi']["free"][n]), n
    for n, b in m.named_buffers():
        assert torch.equal(b, snap_buffers[n]), n
    hi_3 = evaluate(*hi)
    print("hi loss before", hi_1, hi_2, "after activate('hi')", hi_3)
    if hi_1 == hi_2:
        assert hi_3 == hi_1
    else:                                                                     # run-to-run differences of the forward itself
        assert min(abs(hi_3 - hi_1), abs(hi_3 - hi_2)) <= abs(hi_1 - hi_2)

    pb.activate('ta')
    ta_masked = evaluate(*ta)
    print("ta loss with every bit on", ta_all_on, "with ta's masks and heads", ta_masked)
    assert ta_masked == ta_masked and ta_masked != ta_all_on
    assert pb.languages() == ['hi', 'ta'] and pb.current == 'ta'
