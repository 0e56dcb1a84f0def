"""LoRA inside the fused optimizer step (ia_lora_grad, the shared AdamW rule on the factor buffer, ia_lora_apply) on a toy module of
its own, and once through the model.

adapted: w65x63 (odd both ways), w130x257 (33 410 elements: several chunks, rows that are not 16-byte aligned, two column tiles
and three row tiles), w8x4096 (one row per chunk, sixteen column tiles), w1030x8 (seventeen row tiles to add up for gA), conv
[24, 16, 3] viewed as 24 x 48, idle 70 x 66 (never receives a gradient).  free: the vectors v0..v3 (3, 65, 4096, 2 * 4096 + 5
elements).  frozen: z0, z1.  Ranks 1, 5 and 8 on all of them and rank 64 on w130x257 alone; three steps (the second with a tiny
gradient, the third with grad_scale = 0.75), with and without max_grad_norm = 1.

What is held to what (include/indicasr.h has the definitions):
  factor gradients    fp64 from the same fp32 G and the pre-step factors, within the forward-error bound of a sum of K terms in
                      any order: (K + 2) * 2^-24 * s * sum |terms|
  factor update       bit for bit against a plain FusedAdamW whose parameters ARE the factors, fed the kernel's factor_grad
  weights             base + s * B @ A in fp64 within (r + 2) * 2^-24 * (|base| + s * sum_j |B_ij| |A_jc|); the bf16 image bit for bit
  free tensors        bit for bit against a plain FusedAdamW fed the same gradient
  end to end          torch.optim.AdamW on [A, B] in fp64 and in fp32: the kernel path's error against fp64 is at most 4 x torch
                      fp32's plus 2^-24 * max |ref| (the two fp32 paths add in different orders).  Measured on the MI355X over
                      every case of this file: see the docstring of test_end_to_end_against_torch."""
import functools

import pytest
import torch

from test_optimizer_clip_gpu import make_grad

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SHAPES = {"w65x63": (65, 63), "w130x257": (130, 257), "w8x4096": (8, 4096), "w1030x8": (1030, 8), "conv": (24, 16, 3),
          "idle": (70, 66)}
VECTORS = {"v0": 3, "v1": 65, "v2": 4096, "v3": 2 * 4096 + 5}
ADAPTED = list(SHAPES)
FROZEN = ["z0", "z1"]
GROUP1 = dict(params=["w130x257", "w1030x8", "v1"], lr=3e-3, weight_decay=0.1)      # splits the adapted and the free tensors
CASES = [(1, False), (1, True), (5, False), (5, True), (8, False), (8, True), (64, False), (64, True)]
SCALES = (3.0, 1e-7, 0.5)             # the second gradient is far below the clip threshold
GRAD_SCALES = (None, None, 0.75)


class Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(23)
        for n, shape in SHAPES.items():
            setattr(self, n, torch.nn.Parameter(torch.randn(*shape, generator=g)))
        for n, k in VECTORS.items():
            setattr(self, n, torch.nn.Parameter(torch.randn(k, generator=g)))
        self.z0 = torch.nn.Parameter(torch.randn(130, generator=g))
        self.z1 = torch.nn.Parameter(torch.randn(7, generator=g))
        self.register_buffer("stat", torch.zeros(5))


def adapted_of(rank):
    return ["w130x257"] if rank == 64 else ADAPTED


def build(rank, clip=False, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy().cuda())
    lora = cl.LoRA(flat, rank=rank, alpha=16.0, adapted=adapted_of(rank), frozen=FROZEN, seed=1)
    opt = cl.FusedAdamW(flat, lr=1e-3, weight_decay=1e-2, masks=lora, param_groups=[GROUP1],
                        max_grad_norm=1.0 if clip else None, **kw)
    return flat, lora, opt


def plain(clip=False, **kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Toy().cuda())
    return flat, cl.FusedAdamW(flat, lr=1e-3, weight_decay=1e-2, param_groups=[GROUP1], max_grad_norm=1.0 if clip else None, **kw)


def bits_equal(a, b):
    """Same bit patterns (torch.equal alone would let -0.0 pass for +0.0)."""
    view = {4: torch.int32, 2: torch.int16}[a.element_size()]
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(view), b.view(view))


def where(flat, names):
    m = torch.zeros(flat.numel, dtype=torch.bool, device="cuda")
    for name, off, k, _ in flat.entries:
        if name in names:
            m[off:off + k] = True
    return m


def seed_b(lora, seed=77, spread=0.05):
    """B = seeded non-zero values (begin_language leaves B = 0, which makes gA all zeros), then the weights follow."""
    g = torch.Generator().manual_seed(seed)
    for name, fac in lora.factor_views().items():
        fac["lora_B"].copy_(torch.randn(fac["lora_B"].shape, generator=g) * spread)
    lora._apply_factors(lora.factors)


def gradients(flat):
    return [make_grad(list(flat.entries), flat.numel, 300 + i, scale=s).cuda() for i, s in enumerate(SCALES)]


def snapshot(flat, lora, opt):
    return {"theta": flat.theta.clone(), "shadow": opt.shadow.clone(), "factors": lora.factors.clone(),
            "factor_grad": lora.factor_grad.clone(), "fm": lora.factor_exp_avg.clone(), "fv": lora.factor_exp_avg_sq.clone(),
            "factor_step": lora.factor_step.clone(), "m": opt.exp_avg.clone(), "v": opt.exp_avg_sq.clone(),
            "seg_step": opt.seg_step.clone(), "coef": opt._norm_state[1].clone()}


def _run(rank, clip, seeded):
    """Three steps; -> (flat, lora, opt, the gradients, [state before step 0, after step 0, after step 1, after step 2])."""
    flat, lora, opt = build(rank, clip)
    lora.begin_language("a", opt)
    if seeded:
        seed_b(lora)
    gs = gradients(flat)
    states = [snapshot(flat, lora, opt)]
    for g, scale in zip(gs, GRAD_SCALES):
        opt.zero_grad()
        flat.grad.copy_(g)
        opt.step(grad_scale=scale)
        states.append(snapshot(flat, lora, opt))
    return flat, lora, opt, gs, states


run = functools.lru_cache(maxsize=None)(_run)      # computed once per case and shared; nothing in it is modified afterwards


def consumed(g, scale, coef, clip):
    """The fp32 G the step consumes: grad * grad_scale [* coef], one torch op per rounding."""
    G = g * torch.tensor(1.0 if scale is None else scale, dtype=torch.float32, device="cuda")
    return G * coef if clip else G


def test_kinds_and_begin_language():
    flat, lora, opt = build(8)
    kinds = lora.kinds()
    assert [n for n, k in kinds.items() if k == "adapted"] == ADAPTED
    assert {n for n, k in kinds.items() if k == "frozen"} == set(FROZEN)
    assert {n for n, k in kinds.items() if k == "free"} == set(VECTORS)
    theta0 = flat.theta.clone()
    lora.begin_language("a", opt)
    assert bits_equal(flat.theta, theta0) and bits_equal(opt.shadow, theta0.to(torch.bfloat16))     # B = 0: theta = base + s * 0
    again = build(8)[1]
    again.begin_language("a")
    other = build(8)[1]
    other.begin_language("b")
    assert bits_equal(again.factors, lora.factors) and not torch.equal(other.factors, lora.factors)   # seeded by the language
    for name, fac in lora.factor_views().items():
        n = fac["lora_A"].shape[1]
        assert not fac["lora_B"].any() and float(fac["lora_A"].abs().max()) <= n ** -0.5, name
        if fac["lora_A"].numel() >= 256:
            assert float(fac["lora_A"].abs().max()) > 0.9 * n ** -0.5 and abs(float(fac["lora_A"].mean())) < 0.2 * n ** -0.5, name
    gaps = torch.ones(lora.factor_numel, dtype=torch.bool, device="cuda")
    for fac in lora.factor_views(gaps).values():
        fac["lora_A"].fill_(False); fac["lora_B"].fill_(False)
    assert not lora.factors[gaps].any()
    only = build(64)[1].kinds()
    assert [n for n, k in only.items() if k == "adapted"] == ["w130x257"] and only["w65x63"] == "free"


@pytest.mark.parametrize("rank,clip", CASES)
def test_factor_gradients_against_fp64(rank, clip):
    flat, lora, opt, gs, states = run(rank, clip, True)
    s = float(lora.scale)
    worst = 0.0
    for step, g in enumerate(gs):
        G = consumed(g, GRAD_SCALES[step], states[step + 1]["coef"], clip)
        if clip:
            assert (float(states[step + 1]["coef"]) < 1.0) == (step != 1)           # clipped, not clipped, clipped
        pre = lora.factor_views(states[step]["factors"])
        got = lora.factor_views(states[step + 1]["factor_grad"])
        for name, k, m, n, b_off, a_off in lora.adapted:
            o = flat.entries[k][1]
            G64 = G[o:o + m * n].view(m, n).double()
            A64, B64 = pre[name]["lora_A"].double(), pre[name]["lora_B"].double()
            for key, ref, terms, K in (("lora_B", s * (G64 @ A64.t()), s * (G64.abs() @ A64.abs().t()), n),
                                       ("lora_A", s * (B64.t() @ G64), s * (B64.abs().t() @ G64.abs()), m)):
                err = (got[name][key].double() - ref).abs()
                bound = (K + 2) * U * terms
                ratio = float((err / bound.clamp_min(1e-300)).max())
                worst = max(worst, ratio)
                assert bool((err <= bound).all()), (step, name, key, ratio)
                if name == "idle":
                    assert not got[name][key].any()
                else:
                    assert got[name][key].abs().max() > 0, (step, name, key)
    print(f"rank {rank} clip {clip}: largest |error| / bound of a factor gradient = {worst:.3f}")


class Factors(torch.nn.Module):
    """The factors of every adapted tensor that receives a gradient as a module's parameters, B before A, in layout order."""

    def __init__(self, lora, factors):
        super().__init__()
        views = lora.factor_views(factors)
        for t, (name, *_rest) in enumerate(lora.adapted):
            if name != "idle":
                setattr(self, f"t{t}_B", torch.nn.Parameter(views[name]["lora_B"].clone()))
                setattr(self, f"t{t}_A", torch.nn.Parameter(views[name]["lora_A"].clone()))


@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("rank,clip", CASES)
def test_factor_update_bit_for_bit(rank, clip, seeded):
    from indic_cl_asr_amd import cl
    flat, lora, opt, gs, states = run(rank, clip, seeded)
    ref_flat = cl.FlatParams(Factors(lora, states[0]["factors"]).cuda())
    live = [a for a in lora.adapted if a[0] != "idle"]
    assert [e[1] for e in ref_flat.entries] == [off for a in live for off in (a[4], a[5])]       # the same layout, idle at its end
    in_group1 = [f"t{t}_{x}" for t, a in enumerate(lora.adapted) if a[0] in GROUP1["params"] for x in "BA"]
    ref = cl.FusedAdamW(ref_flat, lr=1e-3, weight_decay=1e-2, bf16_shadow=False,
                        param_groups=[dict(params=in_group1, lr=GROUP1["lr"], weight_decay=GROUP1["weight_decay"])])
    N, nf = ref_flat.numel, 2 * len(live)
    for step in range(3):
        now = states[step + 1]
        if not seeded and step == 0:                             # B = 0: gA is all zeros and A must still take the step
            for name, fac in lora.factor_views(now["factor_grad"]).items():
                assert not fac["lora_A"].any() and (name == "idle" or fac["lora_B"].any()), name
        ref.zero_grad()
        ref_flat.grad.copy_(now["factor_grad"][:N])
        ref_flat.all_grads_live = True                           # liveness is the parent's: every factor here is live
        ref.step()
        assert bits_equal(now["factors"][:N], ref_flat.theta), step
        assert bits_equal(now["fm"][:N], ref.exp_avg) and bits_equal(now["fv"][:N], ref.exp_avg_sq), step
        assert torch.equal(now["factor_step"][:nf], ref.seg_step) and now["factor_step"][:nf].tolist() == [step + 1] * nf, step
        # idle: no gradient, so factors, moments and counters stay
        assert bits_equal(now["factors"][N:], states[0]["factors"][N:]) and not now["fm"][N:].any() and not now["fv"][N:].any()
        assert not now["factor_step"][nf:].any()
    if rank != 64:
        assert lora.factor_numel > N                             # idle's factors do lie behind the others
    assert not bits_equal(states[3]["factors"][:N], states[0]["factors"][:N])


@pytest.mark.parametrize("rank,clip", CASES)
def test_materialised_weights_free_and_frozen_tensors(rank, clip):
    flat, lora, opt, gs, states = run(rank, clip, True)
    fb, P = plain(clip)
    s, r = float(lora.scale), lora.rank
    kinds = lora.kinds()
    F = where(flat, {n for n, k in kinds.items() if k == "free"})
    Z = where(flat, set(FROZEN) | ({"idle"} if rank != 64 else set()))
    AD = where(flat, {n for n, k in kinds.items() if k == "adapted"})
    free_ids = [i for i, n in enumerate(flat.names) if kinds[n] == "free"]
    other_ids = [i for i, n in enumerate(flat.names) if kinds[n] != "free"]
    worst = 0.0
    for step in range(4):
        now = states[step]
        if step:
            fb.grad.copy_(gs[step - 1])
            P.step(grad_scale=GRAD_SCALES[step - 1])
            for key, mine, theirs in (("theta", now["theta"], fb.theta), ("exp_avg", now["m"], P.exp_avg),
                                      ("exp_avg_sq", now["v"], P.exp_avg_sq), ("shadow", now["shadow"], P.shadow)):
                assert bits_equal(mine[F], theirs[F]), (step, key)
            assert torch.equal(now["seg_step"][free_ids], P.seg_step[free_ids]) and now["seg_step"][free_ids].tolist() == \
                [0 if flat.names[i] == "idle" else step for i in free_ids]      # at rank 64 idle is free, and still gets no gradient
            if clip:
                assert bits_equal(now["coef"], P._norm_state[1])             # the norm is the task gradient's over all tensors
        views = lora.factor_views(now["factors"])
        for name, k, m, n, b_off, a_off in lora.adapted:
            o = flat.entries[k][1]
            B64, A64 = views[name]["lora_B"].double(), views[name]["lora_A"].double()
            base = lora.base.flat[o:o + m * n].view(m, n).double()
            err = (now["theta"][o:o + m * n].view(m, n).double() - (base + s * (B64 @ A64))).abs()
            bound = (r + 2) * U * (base.abs() + s * (B64.abs() @ A64.abs()))
            worst = max(worst, float((err / bound).max()))
            assert bool((err <= bound).all()), (step, name, float((err / bound).max()))
        assert bits_equal(now["shadow"], now["theta"].to(torch.bfloat16)), step                 # the whole buffer
        # frozen tensors and idle keep their weights; nothing but a free tensor has its full-size moments or counter written
        assert bits_equal(now["theta"][Z], states[0]["theta"][Z]), step
        assert not now["m"][~F].any() and not now["v"][~F].any() and not now["seg_step"][other_ids].any(), step
    assert not bits_equal(states[3]["theta"][AD], states[0]["theta"][AD]) and not bits_equal(states[3]["theta"][F], states[0]["theta"][F])
    print(f"rank {rank} clip {clip}: largest |error| / bound of a materialised weight = {worst:.3f}")


@pytest.mark.parametrize("rank,clip", CASES)
def test_end_to_end_against_torch(rank, clip):
    """torch.optim.AdamW on [A, B] with the loss sum_t <G_t, W0 + s * B @ A>, in fp64 and in fp32 on the device, against the kernel
    path after three steps, per factor: err(kernel) <= 4 * err(torch fp32) + 2^-24 * max |ref|.

    Measured on the MI355X: the largest error / allowance over all cases and factors is 0.84, A of w130x257 at rank 64 with
    clipping (kernel 2.3e-6, torch fp32 6.9e-7: a ratio of 3.4, so the factor 4 is not wide there); every other case stays
    below 0.4."""
    flat, lora, opt, gs, states = run(rank, clip, True)
    s = float(lora.scale)
    Gs = [consumed(g, GRAD_SCALES[i], states[i + 1]["coef"], clip) for i, g in enumerate(gs)]
    start = lora.factor_views(states[0]["factors"])
    final = lora.factor_views(states[3]["factors"])
    results = {}
    for dtype in (torch.float64, torch.float32):
        params, groups = {}, {0: [], 1: []}
        for name, k, m, n, b_off, a_off in lora.adapted:
            if name == "idle":
                continue
            A = start[name]["lora_A"].to(dtype).clone().requires_grad_(True)
            B = start[name]["lora_B"].to(dtype).clone().requires_grad_(True)
            params[name] = (A, B)
            groups[1 if name in GROUP1["params"] else 0] += [A, B]
        spec = [dict(params=groups[0], lr=1e-3, weight_decay=1e-2),
                dict(params=groups[1], lr=GROUP1["lr"], weight_decay=GROUP1["weight_decay"])]
        spec = [g for g in spec if g["params"]]
        topt = torch.optim.AdamW(spec, betas=(0.9, 0.999), eps=1e-8)
        for G in Gs:
            topt.zero_grad()
            loss = 0
            for name, k, m, n, b_off, a_off in lora.adapted:
                if name in params:
                    A, B = params[name]
                    o = flat.entries[k][1]
                    W0 = lora.base.flat[o:o + m * n].view(m, n).to(dtype)
                    loss = loss + (G[o:o + m * n].view(m, n).to(dtype) * (W0 + s * (B @ A))).sum()
            loss.backward()
            topt.step()
        results[dtype] = params
    worst = 0.0
    for name, (A64, B64) in results[torch.float64].items():
        A32, B32 = results[torch.float32][name]
        for key, ref, t32 in (("lora_A", A64, A32), ("lora_B", B64, B32)):
            ref = ref.detach()
            e_kernel = float((final[name][key].double() - ref).abs().max())
            e_torch = float((t32.detach().double() - ref).abs().max())
            allowed = 4.0 * e_torch + U * float(ref.abs().max())
            worst = max(worst, e_kernel / allowed)
            print(f"rank {rank} clip {clip} {name}.{key}: kernel {e_kernel:.3e} torch fp32 {e_torch:.3e} "
                  f"ratio to the allowance {e_kernel / allowed:.3f}")
            assert e_kernel <= allowed, (name, key, e_kernel, e_torch)
    print(f"rank {rank} clip {clip}: largest error / allowance = {worst:.3f}")


@pytest.mark.parametrize("rank,clip", [(5, True), (64, False)])
def test_zero_forgetting_and_determinism(rank, clip):
    first = run(rank, clip, True)
    again = _run(rank, clip, True)
    for a, b in zip(first[4], again[4]):
        assert all(bits_equal(a[k], b[k]) for k in a), "the same three steps gave other bits"

    flat, lora, opt = build(rank, clip)
    kinds = lora.kinds()
    AD = where(flat, {n for n, k in kinds.items() if k == "adapted"})
    F = where(flat, {n for n, k in kinds.items() if k == "free"})
    gs = gradients(flat)
    base = lora.base.flat.clone()

    def train(seed_shift):
        for i, g in enumerate(gs):
            opt.zero_grad()
            flat.grad.copy_(g.roll(seed_shift) if seed_shift else g)
            flat.grad.mul_(where(flat, set(flat.names) - {"idle"}))           # rolled values stay out of idle and the gaps
            opt.step()
            flat.model.stat.add_(1.0 + seed_shift)                            # a module buffer that moves while training

    lora.begin_language("a", opt)
    train(0)
    lora.save_language()
    snap = {"theta": flat.theta.clone(), "shadow": opt.shadow.clone(), "stat": flat.model.stat.clone()}
    assert not bits_equal(snap["theta"][AD], base[AD])
    lora.begin_language("b", opt)
    assert bits_equal(flat.theta[AD], base[AD])                               # B = 0 again: the backbone itself
    assert bits_equal(flat.theta[F], snap["theta"][F])                        # free tensors continue from where they are
    assert not lora.factor_exp_avg.any() and not lora.factor_step.any() and not opt.exp_avg[F].any() and not opt.seg_step.any()
    train(3)
    lora.save_language()
    b_theta = flat.theta.clone()
    assert not bits_equal(b_theta[AD], snap["theta"][AD]) and not bits_equal(b_theta[F], snap["theta"][F])
    lora.activate("a")
    assert bits_equal(flat.theta, snap["theta"]) and bits_equal(opt.shadow, snap["shadow"])
    assert bits_equal(flat.model.stat, snap["stat"])
    assert bits_equal(lora.base.flat, base)                                   # the backbone never moves
    assert lora.languages() == ["a", "b"] and lora.current == "a"
    with pytest.raises(RuntimeError, match="belong to another language"):
        lora.save_language()                                                  # the live factors are b's
    lora.activate("b")
    assert bits_equal(flat.theta, b_theta)
    # delta and export describe the same weights
    delta = lora.delta("a")
    ex = lora.export("a")
    for name, k, m, n, b_off, a_off in lora.adapted:
        want = float(lora.scale) * (ex[name]["lora_B"].double() @ ex[name]["lora_A"].double())
        got = delta[name].view(m, n).double()
        assert bool(((got - want).abs() <= (rank + 2) * U * float(lora.scale) *
                     (ex[name]["lora_B"].double().abs() @ ex[name]["lora_A"].double().abs())).all()), name
    assert not delta.flat[~AD].any()


@pytest.mark.parametrize("where_nan", ["w130x257", "v2"])
def test_nonfinite_gradient_skips_the_step(where_nan):
    flat, lora, opt = build(5, skip_nonfinite=True)
    lora.begin_language("a", opt)
    seed_b(lora)
    gs = gradients(flat)
    flat.grad.copy_(gs[0])
    opt.step()
    before = snapshot(flat, lora, opt)
    opt.zero_grad()
    flat.grad.copy_(gs[2])
    flat.grads_dict()[where_nan].view(-1)[17] = float("nan")
    opt.step()
    after = snapshot(flat, lora, opt)
    for key in before:
        if key not in ("coef", "factor_grad"):
            assert bits_equal(before[key], after[key]), key
    assert opt.stats()["skipped_steps"] == 1 and not lora.factor_active.any() and not opt.seg_active.any()
    opt.zero_grad()
    flat.grad.copy_(gs[2])
    opt.step()                                                   # and the next finite step moves everything again
    moved = snapshot(flat, lora, opt)
    assert opt.stats()["skipped_steps"] == 1
    assert not bits_equal(moved["factors"], before["factors"]) and not bits_equal(moved["theta"], before["theta"])
    live = 2 * (len(lora.adapted) - 1)
    assert moved["factor_step"].tolist() == [2] * live + [0, 0]


def test_once_through_the_model():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    from test_si_gpu import _batch
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny')).cuda().train()
    freeze_layer(m, 0)
    flat = cl.FlatParams(m)
    lora = cl.LoRA(flat)                                          # default kinds, rank 8
    opt = cl.FusedAdamW(flat, lr=1e-3, masks=lora)
    kinds = lora.kinds()
    assert set(kinds.values()) == {"free", "adapted", "frozen"}

    def evaluate(batch, langs):
        m.eval()
        with torch.no_grad():
            loss, _ = m.training_step(batch, langs, compute_wer=False)
        return float(loss)

    hi = _batch(['hi'] * 4, seed=1)
    lora.begin_language('hi', opt)
    base = lora.base.flat.clone()
    m.train()
    for _ in range(2):
        opt.zero_grad()
        loss, _ = m.training_step(*hi, compute_wer=False)
        loss.backward()
        opt.step()
        assert bool(torch.isfinite(loss))
    cl.flush_pending_updates()
    for n, k in kinds.items():
        moved = not torch.equal(flat.params_dict()[n], lora.base[n])
        if k == "frozen":
            assert not moved, n
        elif k == "adapted":
            assert moved, n
    assert any(not torch.equal(flat.params_dict()[n], lora.base[n]) for n, k in kinds.items() if k == "free")
    assert bits_equal(opt.shadow, flat.theta.to(torch.bfloat16))
    lora.save_language()
    recorded = evaluate(*hi)
    snap = flat.theta.clone()
    lora.begin_language('ta', opt)
    assert evaluate(*hi) != recorded                              # the backbone alone is another network
    lora.activate('hi')
    assert bits_equal(flat.theta, snap) and bits_equal(lora.base.flat, base)
    after = evaluate(*hi)
    print("hi loss recorded", recorded, "after save_language, begin_language('ta'), activate('hi')", after)
    assert after == recorded and recorded == recorded
