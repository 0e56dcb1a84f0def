"""ia_merge_fisher, ia_merge_linear_dare, ia_merge_ties_dare and the three methods of cl.TaskVectors.merge that run on them, on
the device, bit for bit against the CPU references of tests/test_merge_fisher_dare.py (`ref_fisher`; `dare_keep` and
`ref_dare_rows` in front of `ref_linear` and of `ref_ties` with all-zero cutoffs).  No tolerance anywhere.

The layout is the Toy of tests/test_optimizer_clip_gpu.py without its large tensor, as in tests/test_merge_gpu.py: 1, 3, 4, 63,
64, 65, 4095, 4096, 4097, 2 * 4096 + 5, 65 x 63 and 130 elements.  Targets start from a sentinel inside the tensors and +0 in the
alignment gaps, which must stay +0."""
import ctypes

import pytest
import torch

from test_merge import f32, ref_linear, ref_ties
from test_merge_fisher_dare import dare_keep, ref_dare_rows, ref_fisher
from test_merge_gpu import MAGNITUDES, SENTINEL, Dev, bits, quantised_rows, random_rows, same_bits
from test_optimizer_clip_gpu import Toy

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return Dev()


def gaps_untouched(dev, theta, shadow):
    return not bits(theta)[~dev.inside].any() and not bits(shadow)[~dev.inside].any()


# ------------------------------------------------------------------------------------------ ia_merge_fisher
def fisher_call(dev, vec, imp, coef, floor, scale, theta, shadow, counts):
    K = vec.shape[0]
    assert vec.shape == imp.shape and vec.stride(0) == imp.stride(0)
    return dev.L.ia_merge_fisher(dev.ptr(theta), dev.ptr(dev.base_d), dev.ptr(vec), dev.ptr(imp), vec.stride(0), K,
                                 (ctypes.c_float * K)(*coef), floor, scale, dev.ptr(dev.table), dev.nchunks, dev.nseg,
                                 dev.ptr(shadow), dev.ptr(counts), dev.lib.stream_ptr())


def importance_rows(dev, K, seed):
    """randn^2 * 1e-3 (the size of a squared gradient), and inside the largest tensor and the matrix: exact zeros in every row
    (den == 0 at floor 0), entries below 1e-6 in every row, importances of 1e-30 whose products with a tau of 1e-10 are
    subnormal, one NaN and one negative entry."""
    g = torch.Generator().manual_seed(seed)
    rows = torch.where(dev.inside, torch.randn(K, dev.numel, generator=g) ** 2 * 1e-3, torch.zeros(K, dev.numel))
    where = {}
    for name in ("v9", "mat"):
        o = dev.offset(name)
        rows[:, o:o + 6] = 0.0
        rows[:, o + 6:o + 12] = 1e-7
        rows[:, o + 12:o + 18] = 1e-30
        rows[K - 1, o + 20] = float("nan")
        rows[0, o + 21] = -0.5
        where[name] = o
    return rows, where


@pytest.mark.parametrize("floor", [1e-6, 0.0])
@pytest.mark.parametrize("K", [1, 2, 5, 32])
def test_fisher_bit_for_bit(dev, K, floor):
    from indic_cl_asr_amd import cl
    assert cl.MERGE_MAX_TASKS == 32
    taus = random_rows(dev, K, 130 + K)
    imp, where = importance_rows(dev, K, 140 + K)
    for o in where.values():
        taus[:, o + 12:o + 18] = 1e-10
    coef = [1.0, 0.5, 2.0, 1.0 / 3, 1.5][:K] if K <= 5 else [0.25 + 0.125 * (k % 7) for k in range(K)]
    scale = 0.7
    want, want16, want_counts = ref_fisher(dev.base, taus, imp, coef, floor, scale, dev.entries)
    # the data are what they are meant to be
    o = where["v9"]
    sub = (f32(coef[0]) * imp[0, o + 12]) * taus[0, o + 12]
    if floor == 0.0:
        assert 0.0 < float(sub) < 2.0 ** -126                                           # a subnormal product
        lone = 4 if K == 1 else 0                          # the NaN and the negative entry have no other row beside them
        assert same_bits(want[o:o + 6], dev.base[o:o + 6]) and int(want_counts[:, 1].sum()) == 12 + lone
        assert int(want_counts[:, 0].sum()) == 12 + lone                                # only these are not above 0
    else:
        assert int(want_counts[:, 1].sum()) == 0 and int(want_counts[:, 0].sum()) >= 36  # zeros, 1e-7, 1e-30 (and small randn^2)
    assert torch.isfinite(want[dev.inside]).all()                                       # the NaN importance became the floor
    # rows read by stride from wider buffers, with other rows around them
    wide_t, wide_f = torch.full((K + 2, dev.numel + 64), 3.0), torch.full((K + 2, dev.numel + 64), 5.0)
    wide_t[1:K + 1, :dev.numel], wide_f[1:K + 1, :dev.numel] = taus, imp
    vec, fis = wide_t.cuda()[1:K + 1], wide_f.cuda()[1:K + 1]
    theta, shadow = dev.targets()
    counts = torch.full((dev.nseg, 2), 99, dtype=torch.int32, device="cuda")            # zeroed by the launch
    assert fisher_call(dev, vec, fis, coef, floor, scale, theta, shadow, counts) == 0
    print(K, floor, "counts", counts.sum(0).tolist(), "of", int(dev.inside.sum()))
    assert same_bits(theta, want) and same_bits(shadow, want16)
    assert torch.equal(counts.cpu(), want_counts)
    assert gaps_untouched(dev, theta, shadow) and not (theta.cpu()[dev.inside] == SENTINEL).all()
    # without a shadow only theta is written; a second launch adds nothing to the counts
    theta2, shadow2 = dev.targets()
    assert fisher_call(dev, vec, fis, coef, floor, scale, theta2, None, counts) == 0
    assert same_bits(theta2, want) and same_bits(shadow2, dev.targets()[1]) and torch.equal(counts.cpu(), want_counts)


def test_fisher_equal_importances_are_the_weighted_mean_of_the_kernels(dev):
    """Importances that are the same power of two in every row cancel exactly: theta equals ia_merge_linear's with coef / sum."""
    taus = random_rows(dev, 2, 150).cuda()
    imp = torch.full((2, dev.numel), 2.0 ** -10).cuda()
    theta, shadow = dev.targets()
    counts = torch.zeros(dev.nseg, 2, dtype=torch.int32, device="cuda")
    assert fisher_call(dev, taus, imp, [1.0, 3.0], 0.0, 1.0, theta, shadow, counts) == 0
    theta2, shadow2 = dev.targets()
    assert dev.linear(taus, [0.25, 0.75], 1.0, theta2, shadow2) == 0
    assert same_bits(theta, theta2) and same_bits(shadow, shadow2) and not counts.any()


# ------------------------------------------------------------------------------------------ DARE
def linear_dare_call(dev, vec, coef, scale, theta, shadow, seed, threshold, keep_prob):
    K = vec.shape[0]
    return dev.L.ia_merge_linear_dare(dev.ptr(theta), dev.ptr(dev.base_d), dev.ptr(vec), vec.stride(0), K,
                                      (ctypes.c_float * K)(*coef), scale, dev.ptr(dev.table), dev.nchunks, dev.ptr(shadow),
                                      seed, threshold, keep_prob, dev.lib.stream_ptr())


def ties_dare_call(dev, vec, scale, theta, shadow, counts, seed, threshold, keep_prob):
    return dev.L.ia_merge_ties_dare(dev.ptr(theta), dev.ptr(dev.base_d), dev.ptr(vec), vec.stride(0), vec.shape[0], scale,
                                    dev.ptr(dev.table), dev.nchunks, dev.nseg, dev.ptr(shadow), dev.ptr(counts), seed, threshold,
                                    keep_prob, dev.lib.stream_ptr())


@pytest.fixture(scope="module")
def dare_rows(dev):
    """{(kind, K): rows on the CPU}, shared and never modified."""
    out = {}
    for K in (1, 2, 5):
        out["quantised", K] = quantised_rows(dev, K, 160 + K)
        out["random", K] = random_rows(dev, K, 170 + K)
    return out


COEF = {1: [0.7], 2: [1.0, -0.5], 5: [1.0, 0.0, -2.5, 0.3, 1.0 / 3]}
ZERO_CUT = {}


def zero_cutoffs(K, numel):
    if (K, numel) not in ZERO_CUT:
        ZERO_CUT[K, numel] = torch.zeros(K, numel, dtype=torch.int32)
    return ZERO_CUT[K, numel]


@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("density", [1.0, 0.5, 0.1])
@pytest.mark.parametrize("K", [1, 2, 5])
@pytest.mark.parametrize("kind", ["quantised", "random"])
def test_dare_linear_and_ties_bit_for_bit(dev, dare_rows, kind, K, density, rescale):
    from indic_cl_asr_amd import cl
    rows = dare_rows[kind, K]
    seed, scale = 1000 + K, 0.8
    threshold, keep_prob = cl.density_to_keep(density, rescale)
    keep = dare_keep(seed, K, dev.numel, threshold)
    kept = int(keep[:, dev.inside].sum())
    total = K * int(dev.inside.sum())
    print(kind, K, density, rescale, "kept", kept, "of", total)
    assert kept == total if density == 1.0 else 0 < kept < total
    t = ref_dare_rows(rows, keep, keep_prob)
    vec = rows.cuda()
    # ---- linear
    want, want16 = ref_linear(dev.base, t, COEF[K], scale)
    theta, shadow = dev.targets()
    assert linear_dare_call(dev, vec, COEF[K], scale, theta, shadow, seed, threshold, keep_prob) == 0
    assert same_bits(theta, want) and same_bits(shadow, want16) and gaps_untouched(dev, theta, shadow)
    theta2, shadow2 = dev.targets()
    assert linear_dare_call(dev, vec, COEF[K], scale, theta2, None, seed, threshold, keep_prob) == 0
    assert same_bits(theta2, want) and same_bits(shadow2, dev.targets()[1])
    # ---- TIES' election on the kept entries
    want, want16, want_counts = ref_ties(dev.base, t, zero_cutoffs(K, dev.numel), scale, dev.entries)
    theta, shadow = dev.targets()
    counts = torch.full((dev.nseg, 3), 99, dtype=torch.int32, device="cuda")
    assert ties_dare_call(dev, vec, scale, theta, shadow, counts, seed, threshold, keep_prob) == 0
    assert same_bits(theta, want) and same_bits(shadow, want16) and gaps_untouched(dev, theta, shadow)
    assert torch.equal(counts.cpu(), want_counts)
    # the same seed gives the same bits, another seed other ones
    again, again16 = dev.targets()
    assert ties_dare_call(dev, vec, scale, again, again16, counts, seed, threshold, keep_prob) == 0
    assert same_bits(again, theta) and same_bits(again16, shadow) and torch.equal(counts.cpu(), want_counts)
    if density == 1.0:
        # nothing is dropped and x / 1 = x, also x / float32(1): the plain entries' output
        plain, plain16 = dev.targets()
        assert dev.linear(vec, COEF[K], scale, plain, plain16) == 0
        assert same_bits(theta2, plain) and same_bits(shadow, want16)
        theta3, shadow3 = dev.targets()
        assert linear_dare_call(dev, vec, COEF[K], scale, theta3, shadow3, seed, threshold, keep_prob) == 0
        assert same_bits(shadow3, plain16)
        zero = torch.zeros(K, dev.nseg, dtype=torch.int32, device="cuda")
        plain_counts = torch.zeros(dev.nseg, 3, dtype=torch.int32, device="cuda")
        assert dev.ties(vec, zero, "tensor", scale, plain, plain16, plain_counts) == 0
        assert same_bits(theta, plain) and same_bits(shadow, plain16) and torch.equal(counts, plain_counts)
    else:
        other, other16 = dev.targets()
        assert ties_dare_call(dev, vec, scale, other, other16, counts, seed + 1, threshold, keep_prob) == 0
        assert not same_bits(other, theta)
        assert linear_dare_call(dev, vec, COEF[K], scale, other, other16, seed + 1, threshold, keep_prob) == 0
        assert not same_bits(other, theta2)


def test_dare_reads_rows_by_stride_and_numbers_them_from_zero(dev, dare_rows):
    """Rows 1 and 2 of a wider buffer: the mask's task index is the position in the merge, not the row of the buffer."""
    from indic_cl_asr_amd import cl
    rows = dare_rows["random", 2]
    wide = torch.full((4, dev.numel + 64), 3.0)
    wide[1:3, :dev.numel] = rows
    threshold, keep_prob = cl.density_to_keep(0.5)
    t = ref_dare_rows(rows, dare_keep(5, 2, dev.numel, threshold), keep_prob)
    want, want16 = ref_linear(dev.base, t, [2.0, -1.0], 0.5)
    theta, shadow = dev.targets()
    assert linear_dare_call(dev, wide.cuda()[1:3], [2.0, -1.0], 0.5, theta, shadow, 5, threshold, keep_prob) == 0
    assert same_bits(theta, want) and same_bits(shadow, want16)


def test_invalid_arguments_leave_theta_untouched(dev):
    rows = random_rows(dev, 2, 181).cuda()
    imp = torch.ones(2, dev.numel).cuda()
    theta, shadow = dev.targets()
    before, before16 = theta.clone(), shadow.clone()
    L, ptr, s = dev.L, dev.ptr, dev.lib.stream_ptr()
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    coef = (ctypes.c_float * 2)(1.0, 1.0)
    counts = torch.zeros(dev.nseg, 3, dtype=torch.int32, device="cuda")
    inf, nan = float("inf"), float("nan")
    good = [ptr(theta), ptr(dev.base_d), ptr(rows), ptr(imp), dev.numel, 2, coef, 1e-6, 1.0, ptr(dev.table), dev.nchunks, dev.nseg,
            ptr(shadow), ptr(counts), s]
    for at, value in ((3, None), (13, None), (5, 0), (5, 33), (7, -1.0), (7, nan), (7, inf), (8, nan), (11, 0), (4, dev.numel + 2),
                      (3, off(imp, 4)), (12, off(shadow, 2))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_fisher(*args) == -1, ("fisher", at, value)
    good = [ptr(theta), ptr(dev.base_d), ptr(rows), dev.numel, 2, coef, 1.0, ptr(dev.table), dev.nchunks, ptr(shadow), 0, 1 << 31,
            0.5, s]
    for at, value in ((2, None), (4, 33), (6, inf), (12, 0.0), (12, 2.0), (12, nan), (2, off(rows, 4))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_linear_dare(*args) == -1, ("linear_dare", at, value)
    good = [ptr(theta), ptr(dev.base_d), ptr(rows), dev.numel, 2, 1.0, ptr(dev.table), dev.nchunks, dev.nseg, ptr(shadow),
            ptr(counts), 0, 1 << 31, 0.5, s]
    for at, value in ((10, None), (4, 0), (5, nan), (8, 0), (13, 0.0), (13, nan), (0, off(theta, 8))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_ties_dare(*args) == -1, ("ties_dare", at, value)
    torch.cuda.synchronize()
    assert same_bits(theta, before) and same_bits(shadow, before16) and not counts.any()


# ------------------------------------------------------------------------------------------ cl.TaskVectors on the toy
def toy_with_buffers():
    m = Toy(big=False)
    m.register_buffer("stat", torch.zeros(4))
    m.register_buffer("seen", torch.zeros((), dtype=torch.int64))
    return m.cuda()


def test_merge_through_the_class():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.ops import fast
    m = toy_with_buffers()
    flat = cl.FlatParams(m)
    opt = cl.FusedAdamW(flat, lr=1e-3)
    tv = cl.TaskVectors(flat, max_tasks=4)
    tv.set_base(opt)
    n, entries = flat.numel, list(flat.entries)
    inside = torch.zeros(n, dtype=torch.bool)
    for _, off, k, _ in entries:
        inside[off:off + k] = True
    stats_kept = {}
    for seed, lang in enumerate(("hi", "ta", "bn"), start=1):
        g = torch.Generator().manual_seed(190 + seed)
        step = torch.where(inside, MAGNITUDES[torch.randint(0, 6, (n,), generator=g)] *
                           torch.where(torch.rand(n, generator=g) < 0.5, f32(-0.01), f32(0.01)), torch.zeros(n))
        flat.theta.add_(step.cuda())
        m.stat.copy_(torch.randn(4, generator=g))
        m.seen.fill_(10 * seed)
        stats_kept[lang] = m.stat.clone()
        # the language's own Fisher through the real calls: two batches of squared gradients weighted by the loss
        fish = flat.zeros()
        for b in range(2):
            grad = torch.where(inside, torch.randn(n, generator=g) * 0.03, torch.zeros(n))
            grad[entries[-1][1]:entries[-1][1] + entries[-1][2]] = 0.0                   # `idle` never receives a gradient
            flat.grad.copy_(grad)
            cl.fisher_accumulate(flat, fish, torch.tensor([1.5 + b, 0.5], device="cuda"))
        fish = cl.fisher_finish(None, fish, 2, 1.0)
        flat.grad.zero_()
        tv.store(lang, opt, importance=fish)
        assert same_bits(tv.importance(lang).flat, fish.flat) and (fish.flat > 0).any()
        tv.restore_base(opt)
    base = tv.base.flat.cpu()
    taus, imps = tv.vectors[:3, :n].cpu(), tv.importances[:3, :n].cpu()
    idle = entries[-1][0]
    assert idle == "idle" and not tv.importance("hi")[idle].any()

    def dirty():
        opt.exp_avg.fill_(0.5); opt.exp_avg_sq.fill_(0.25); opt.seg_step.fill_(3)
        return fast.WEIGHT_EPOCH

    def after(epoch, names):
        assert not opt.exp_avg.any() and not opt.exp_avg_sq.any() and not opt.seg_step.any() and fast.WEIGHT_EPOCH > epoch
        mean = stats_kept[names[0]].clone()
        for lang in names[1:]:
            mean = mean + stats_kept[lang]
        assert torch.equal(m.stat, mean / len(names)) and int(m.seen) == 10 * (("hi", "ta", "bn").index(names[-1]) + 1)
        assert same_bits(tv.base.flat, base)

    # ---- fisher: every language in row order, then a subset in another order with weights and floor 0
    for names, idx, weights, floor, scale in ((["hi", "ta", "bn"], [0, 1, 2], None, 1e-6, 1.0),
                                              (["bn", "hi"], [2, 0], {"hi": 0.5, "bn": 2.0}, 0.0, 0.9)):
        epoch = dirty()
        stats = tv.merge("fisher", names, weights=weights, fisher_floor=floor, scale=scale)
        coef = [1.0] * len(names) if weights is None else [weights[x] for x in names]
        want, want16, counts = ref_fisher(base, taus[idx], imps[idx], coef, floor, scale, entries)
        assert same_bits(flat.theta, want) and same_bits(opt.shadow, want16)
        assert stats["method"] == "fisher" and stats["languages"] == names and stats["coefficients"] == coef
        assert (stats["scale"], stats["fisher_floor"]) == (scale, floor)
        assert stats["floored"] == int(counts[:, 0].sum()) and stats["unweighted"] == int(counts[:, 1].sum())
        assert stats["tensors"]["mat"] == {"floored": int(counts[-2, 0]), "unweighted": int(counts[-2, 1])}
        assert stats["tensors"][idle]["floored"] == 130 and stats["tensors"][idle]["unweighted"] == (130 if floor == 0.0 else 0)
        assert tv.last_merge is stats
        after(epoch, names)
    # ---- dare_linear and dare_ties
    for names, idx, density, rescale, seed in ((None, [0, 1, 2], 0.5, True, 0), (["bn", "ta"], [2, 1], 0.1, False, 2 ** 32 - 1)):
        threshold, keep_prob = cl.density_to_keep(density, rescale)
        t = ref_dare_rows(taus[idx], dare_keep(seed, len(idx), n, threshold), keep_prob)
        listed = names or ["hi", "ta", "bn"]
        coef = [1.0, -0.5, 2.0][:len(idx)]
        epoch = dirty()
        stats = tv.merge("dare_linear", names, density=density, rescale=rescale, seed=seed, weights=coef, scale=0.4)
        want, want16 = ref_linear(base, t, coef, 0.4)
        assert same_bits(flat.theta, want) and same_bits(opt.shadow, want16)
        assert stats == {"method": "dare_linear", "languages": listed, "coefficients": coef, "scale": 0.4, "seed": seed,
                         "density": density, "rescale": rescale}
        after(epoch, listed)
        epoch = dirty()
        stats = tv.merge("dare_ties", names, density=density, rescale=rescale, seed=seed, scale=0.9)
        want, want16, counts = ref_ties(base, t, zero_cutoffs(len(idx), n), 0.9, entries)
        assert same_bits(flat.theta, want) and same_bits(opt.shadow, want16)
        assert stats["surviving"] == int(counts[:, 0].sum()) > 0 and stats["conflicts"] == int(counts[:, 1].sum())
        assert stats["cancelled"] == int(counts[:, 2].sum()) - (sum(e[2] for e in entries) - int(counts[:, 0].sum()))
        assert stats["tensors"]["mat"]["conflicts"] == int(counts[-2, 1])
        assert (stats["seed"], stats["density"], stats["rescale"], stats["languages"]) == (seed, density, rescale, listed)
        assert "trim" not in stats
        after(epoch, listed)
    # a merge without an optimizer writes no shadow and still moves the weight epoch
    tv.restore_base()
    tv._optimizer = None
    epoch, image = fast.WEIGHT_EPOCH, opt.shadow.clone()
    tv.merge("fisher", fisher_floor=1e-6)
    assert fast.WEIGHT_EPOCH > epoch and same_bits(opt.shadow, image)
    assert same_bits(flat.theta, ref_fisher(base, taus, imps, [1.0] * 3, 1e-6, 1.0, entries)[0])
