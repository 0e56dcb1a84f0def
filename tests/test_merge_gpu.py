"""ia_merge_linear, ia_merge_trim, ia_merge_ties and cl.TaskVectors on the device, bit for bit against the torch fp32
restatement of tests/test_merge.py (sequential adds in task order, kthvalue and >=, /, .bfloat16()) computed on the CPU from
the same data.  No tolerance anywhere: every operation of the kernels is rounded on its own.

The module is the Toy of tests/test_optimizer_clip_gpu.py without its large tensor: 1, 3, 4, 63, 64, 65, 4095, 4096, 4097,
2 * 4096 + 5, 65 x 63 and 130 elements -- a tensor whose trim rank is 0, tails shorter than a float4, alignment gaps, an exact
chunk, several chunks and a 2-D shadow view."""
import ctypes

import pytest
import torch

from test_merge import cutoffs_per_element, f32, patterns, ref_cutoffs, ref_linear, ref_ties, scope_groups
from test_optimizer_clip_gpu import Toy

pytestmark = pytest.mark.gpu

SENTINEL = 7.0


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


class Dev:
    """The toy's flat layout on the device, a seeded base and the operands of direct calls into the library."""

    def __init__(self):
        from indic_cl_asr_amd import _lib, cl
        self.flat = cl.FlatParams(Toy(big=False).cuda())
        f = self.flat
        self.L, self.ptr, self.lib = _lib.lib(), _lib.ptr, _lib
        self.entries, self.numel, self.nseg = list(f.entries), f.numel, len(f.entries)
        self.table, self.nchunks = f.chunk_table, f.chunk_table.shape[0]
        self.inside = torch.zeros(self.numel, dtype=torch.bool)
        for _, off, n, _ in self.entries:
            self.inside[off:off + n] = True
        g = torch.Generator().manual_seed(21)
        self.base = torch.where(self.inside, torch.randn(self.numel, generator=g), torch.zeros(self.numel))
        self.base_d = self.base.cuda()
        self.scopes = {"tensor": torch.arange(self.nseg, dtype=torch.int32).cuda(),
                       "model": torch.zeros(self.nseg, dtype=torch.int32).cuda()}

    def offset(self, name):
        return next(off for n, off, _, _ in self.entries if n == name)

    def targets(self):
        """theta and its bf16 image before a launch: a sentinel inside the tensors, +0 in the alignment gaps."""
        theta = torch.where(self.inside, torch.full((self.numel,), SENTINEL), torch.zeros(self.numel))
        return theta.cuda(), theta.bfloat16().cuda()

    def nscope(self, scope):
        return self.nseg if scope == "tensor" else 1

    def linear(self, vec, coef, scale, theta, shadow):
        K = vec.shape[0]
        return self.L.ia_merge_linear(self.ptr(theta), self.ptr(self.base_d), self.ptr(vec), vec.shape[1], K,
                                      (ctypes.c_float * K)(*coef), scale, self.ptr(self.table), self.nchunks, self.ptr(shadow),
                                      self.lib.stream_ptr())

    def trim(self, vec, scope, trim):
        K, ns = vec.shape[0], self.nscope(scope)
        ws = torch.empty(self.L.ia_merge_trim_workspace_bytes(K, ns), dtype=torch.uint8, device="cuda")
        cut = torch.full((K, ns), -1, dtype=torch.int32, device="cuda")
        st = self.L.ia_merge_trim(self.ptr(vec), vec.shape[1], K, self.ptr(self.table), self.nchunks, self.ptr(self.scopes[scope]),
                                  ns, trim, self.ptr(cut), self.ptr(ws), ws.numel(), self.lib.stream_ptr())
        return st, cut

    def ties(self, vec, cut, scope, scale, theta, shadow, counts):
        return self.L.ia_merge_ties(self.ptr(theta), self.ptr(self.base_d), self.ptr(vec), vec.shape[1], vec.shape[0],
                                    self.ptr(cut), self.ptr(self.scopes[scope]), self.nscope(scope), scale, self.ptr(self.table),
                                    self.nchunks, self.nseg, self.ptr(shadow), self.ptr(counts), self.lib.stream_ptr())


@pytest.fixture(scope="module")
def dev():
    return Dev()


def random_rows(dev, K, seed, scale=0.05):
    g = torch.Generator().manual_seed(seed)
    return torch.where(dev.inside, torch.randn(K, dev.numel, generator=g) * scale, torch.zeros(K, dev.numel))


MAGNITUDES = torch.tensor([0.0, 0.25, 0.5, 1.0, 2.0, 3.0])


def quantised_rows(dev, K, seed, nonfinite=False):
    """Task vectors of six magnitudes with random signs (-0.0 among them): a sixth of every tensor ties at whatever the
    cutoff is.  nonfinite: the last row also holds one inf and one NaN, in the largest tensor and in the matrix."""
    g = torch.Generator().manual_seed(seed)
    mag = MAGNITUDES[torch.randint(0, len(MAGNITUDES), (K, dev.numel), generator=g)]
    sign = torch.where(torch.rand(K, dev.numel, generator=g) < 0.5, -torch.ones(1), torch.ones(1))
    rows = torch.where(dev.inside, mag * sign, torch.zeros(K, dev.numel))
    assert (bits(rows) == -2 ** 31).any() and (bits(rows) == 0)[:, dev.inside].any()         # both zeros occur inside tensors
    if nonfinite:
        for name, at in (("v9", 17), ("mat", 4001)):
            rows[K - 1, dev.offset(name) + at] = float("inf")
            rows[K - 1, dev.offset(name) + at + 1] = float("nan")
    return rows


# ------------------------------------------------------------------------------------------ ia_merge_linear
@pytest.mark.parametrize("K, coef, scale", [
    (1, [0.7], 0.37), (2, [1.0, -0.5], 0.37), (5, [1.0, 0.0, -2.5, 0.3, 1.0 / 3], -1.25),
    (1, [1.0], 1.0), (2, [0.5, 0.5], 1.0), (5, [0.2] * 5, 1.0)])
def test_linear_and_average_bit_for_bit(dev, K, coef, scale):
    taus = random_rows(dev, K, 30 + K)
    want, want16 = ref_linear(dev.base, taus, coef, scale)
    theta, shadow = dev.targets()
    assert dev.linear(taus.cuda(), coef, scale, theta, shadow) == 0
    assert same_bits(theta, want) and same_bits(shadow, want16)
    assert not bits(theta)[~dev.inside].any() and not bits(shadow)[~dev.inside].any()        # the gaps stay +0
    assert not (theta.cpu()[dev.inside] == SENTINEL).all()
    # without a shadow only theta is written
    theta2, shadow2 = dev.targets()
    assert dev.linear(taus.cuda(), coef, scale, theta2, None) == 0
    assert same_bits(theta2, want) and same_bits(shadow2, dev.targets()[1])


def test_linear_reads_rows_by_stride(dev):
    """Rows of a buffer wider than the flat length, as TaskVectors hands them over when languages were dropped or skipped."""
    taus = random_rows(dev, 3, 44)
    wide = torch.zeros(3, dev.numel + 64)
    wide[:, :dev.numel] = taus
    want, want16 = ref_linear(dev.base, taus[1:], [2.0, -1.0], 0.5)
    theta, shadow = dev.targets()
    assert dev.linear(wide.cuda()[1:], [2.0, -1.0], 0.5, theta, shadow) == 0
    assert same_bits(theta, want) and same_bits(shadow, want16)


# ------------------------------------------------------------------------------------------ ia_merge_trim
def tiny_density(dev, scope):
    """Half an element of the largest scope segment: r = floor(n - 0.5) = n - 1 there, only the largest magnitude stays."""
    return 0.5 / max(sum(n for _, _, n, _ in group) for group in scope_groups(dev.entries, scope))


@pytest.fixture(scope="module")
def trim_rows(dev):
    return quantised_rows(dev, 3, 51, nonfinite=True)


@pytest.mark.parametrize("scope", ["tensor", "model"])
@pytest.mark.parametrize("density", [1.0, 0.5, 0.2, "tiny"])
def test_trim_cutoffs_equal_kthvalue(dev, trim_rows, scope, density):
    from indic_cl_asr_amd import cl
    trim = cl.density_to_trim(tiny_density(dev, scope) if density == "tiny" else density)
    want = ref_cutoffs(trim_rows, dev.entries, trim, scope)
    assert torch.equal(want, ref_cutoffs(trim_rows, dev.entries, trim, scope, by_pattern=True))
    st, cut = dev.trim(trim_rows.cuda(), scope, trim)
    assert st == 0
    print(scope, density, "cutoffs", cut.cpu().tolist())
    assert torch.equal(cut.cpu(), want)
    v9 = [e[0] for e in dev.entries].index("v9")
    if density == 1.0:
        assert not cut.any()                                         # r == 0 everywhere: everything stays
    elif scope == "tensor":
        assert int(want[0, 0]) == 0                                  # the one-element tensor: r == 0 at every density
        # the magnitudes are few, so many elements tie at the cutoff (and all of them stay)
        off, n = dev.offset("v9"), 2 * 4096 + 5
        assert int((patterns(trim_rows[0, off:off + n]) == int(want[0, v9])).sum()) > 100
        if density == "tiny":                                        # r = n - 1: the last row's cutoff is its infinity, the NaN above it
            assert int(want[2, v9]) == int(f32(float("inf")).view(torch.int32))


def test_trim_is_deterministic(dev, trim_rows):
    rows = trim_rows.cuda()
    first = dev.trim(rows, "tensor", 0.5)[1].cpu()
    for _ in range(3):
        assert torch.equal(dev.trim(rows, "tensor", 0.5)[1].cpu(), first)


# ------------------------------------------------------------------------------------------ ia_merge_ties
def constructed(dev, rows):
    """Hand-made elements at the head of the largest tensor and of the matrix; -> {case: flat positions}."""
    K = rows.shape[0]
    where = {}
    for name in ("v9", "mat"):
        o = dev.offset(name)
        rows[:, o + 0] = 3.0                                         # full agreement
        rows[:K - 1, o + 1] = -3.0                                   # the sign with more entries ...
        rows[K - 1, o + 1] = 3.0 * (K - 1) + 1.0                     # ... loses to the one with more mass
        rows[:, o + 2] = torch.tensor([1e-3 * (-1) ** k for k in range(K)])      # every entry below the cutoff
        rows[:, o + 3] = 0.0
        rows[0, o + 3], rows[1, o + 3] = 2.0, -2.0                   # exact cancellation
        rows[:, o + 4] = -0.0                                        # -0.0 entries
        for case, at in (("agree", 0), ("conflict", 1), ("trimmed", 2), ("cancel", 3), ("negzero", 4)):
            where.setdefault(case, []).append(o + at)
    return where


@pytest.mark.parametrize("K, scope, density, nonfinite", [
    (2, "tensor", 0.5, False), (3, "tensor", 0.2, False), (3, "model", 0.5, True), (5, "tensor", 0.5, False),
    (5, "model", 0.2, False), (2, "model", 1.0, False)])
def test_ties_bit_for_bit(dev, K, scope, density, nonfinite):
    from indic_cl_asr_amd import cl
    rows = quantised_rows(dev, K, 60 + K, nonfinite)
    where = constructed(dev, rows)
    trim, scale = cl.density_to_trim(density), 0.8
    cutoffs = ref_cutoffs(rows, dev.entries, trim, scope)
    cut_elem = cutoffs_per_element(cutoffs, dev.entries, scope, dev.numel)
    want, want16, want_counts = ref_ties(dev.base, rows, cut_elem, scale, dev.entries)
    # the constructed elements are what they are meant to be under these cutoffs
    pat = lambda x: int(f32(x).view(torch.int32))
    if density < 1.0:
        assert (cut_elem[:, where["trimmed"]] > pat(1e-3)).all() and (cut_elem[:, where["agree"]] <= pat(3.0)).all()
        assert same_bits(want[where["trimmed"]], dev.base[where["trimmed"]])
    assert torch.equal(want[where["agree"]], dev.base[where["agree"]] + f32(3.0) * f32(scale))
    assert torch.equal(want[where["conflict"]], dev.base[where["conflict"]] + f32(3.0 * (K - 1) + 1.0) * f32(scale))
    assert same_bits(want[where["cancel"]], dev.base[where["cancel"]])
    assert same_bits(want[where["negzero"]], dev.base[where["negzero"]])
    vec = rows.cuda()
    st, cut = dev.trim(vec, scope, trim)
    assert st == 0 and torch.equal(cut.cpu(), cutoffs)
    theta, shadow = dev.targets()
    counts = torch.full((dev.nseg, 3), 99, dtype=torch.int32, device="cuda")          # zeroed by the launch
    assert dev.ties(vec, cut, scope, scale, theta, shadow, counts) == 0
    print(K, scope, density, "counts", counts.sum(0).tolist(), "of", int(dev.inside.sum()))
    assert same_bits(theta, want) and same_bits(shadow, want16)
    assert torch.equal(counts.cpu(), want_counts)
    assert not bits(theta)[~dev.inside].any() and not bits(shadow)[~dev.inside].any()
    assert int(want_counts[:, 1].sum()) > 100 and int(want_counts[:, 2].sum()) > 100   # conflicts and zero masses do occur
    # a second launch on the same operands adds nothing to the counts and changes no bit
    assert dev.ties(vec, cut, scope, scale, theta, shadow, counts) == 0
    assert same_bits(theta, want) and torch.equal(counts.cpu(), want_counts)


# ------------------------------------------------------------------------------------------ IA_INVALID_VALUE
def test_invalid_arguments_leave_theta_untouched(dev):
    rows = random_rows(dev, 2, 71).cuda()
    theta, shadow = dev.targets()
    before, before16 = theta.clone(), shadow.clone()
    L, ptr, s = dev.L, dev.ptr, dev.lib.stream_ptr()
    off = lambda t, k: ctypes.c_void_p(t.data_ptr() + k)
    coef = (ctypes.c_float * 2)(1.0, 1.0)
    cut = torch.zeros(2, dev.nseg, dtype=torch.int32, device="cuda")
    counts = torch.zeros(dev.nseg, 3, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.ia_merge_trim_workspace_bytes(2, dev.nseg), dtype=torch.uint8, device="cuda")
    sc = dev.scopes["tensor"]
    inf, nan = float("inf"), float("nan")
    good = [ptr(theta), ptr(dev.base_d), ptr(rows), dev.numel, 2, coef, 1.0, ptr(dev.table), dev.nchunks, ptr(shadow), s]
    for at, value in ((0, None), (1, None), (2, None), (5, None), (7, None), (4, 0), (4, 33), (6, inf), (6, nan), (8, 0), (3, 0),
                      (3, dev.numel + 2), (0, off(theta, 4)), (1, off(dev.base_d, 4)), (2, off(rows, 4)), (7, off(dev.table, 4)),
                      (9, off(shadow, 2))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_linear(*args) == -1, ("linear", at, value)
    good = [ptr(rows), dev.numel, 2, ptr(dev.table), dev.nchunks, ptr(sc), dev.nseg, 0.5, ptr(cut), ptr(ws), ws.numel(), s]
    for at, value in ((0, None), (3, None), (5, None), (8, None), (9, None), (2, 0), (2, 33), (4, 0), (6, 0), (7, 1.0), (7, -0.5),
                      (7, nan), (1, dev.numel + 1), (0, off(rows, 8)), (9, off(ws, 8))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_trim(*args) == -1, ("trim", at, value)
    good = [ptr(theta), ptr(dev.base_d), ptr(rows), dev.numel, 2, ptr(cut), ptr(sc), dev.nseg, 1.0, ptr(dev.table), dev.nchunks,
            dev.nseg, ptr(shadow), ptr(counts), s]
    for at, value in ((0, None), (1, None), (2, None), (5, None), (6, None), (9, None), (13, None), (4, 0), (4, 33), (7, 0),
                      (8, inf), (8, nan), (10, 0), (11, 0), (3, dev.numel + 3), (0, off(theta, 8)), (2, off(rows, 4)),
                      (12, off(shadow, 4))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_ties(*args) == -1, ("ties", at, value)
    torch.cuda.synchronize()
    assert same_bits(theta, before) and same_bits(shadow, before16) and not cut.any() and not counts.any()


# ------------------------------------------------------------------------------------------ cl.TaskVectors on the toy
def toy_vectors():
    from indic_cl_asr_amd import cl
    m = Toy(big=False).cuda()
    flat = cl.FlatParams(m)
    opt = cl.FusedAdamW(flat, lr=1e-3)
    tv = cl.TaskVectors(flat, max_tasks=4)
    tv.set_base(opt)
    inside = torch.zeros(flat.numel, dtype=torch.bool)
    for _, off, n, _ in flat.entries:
        inside[off:off + n] = True
    thetas = {}
    for seed, lang in enumerate(("hi", "ta", "bn"), start=1):
        g = torch.Generator().manual_seed(80 + seed)
        step = torch.where(inside, MAGNITUDES[torch.randint(0, 6, (flat.numel,), generator=g)] *
                           torch.where(torch.rand(flat.numel, generator=g) < 0.5, f32(-0.01), f32(0.01)), torch.zeros(flat.numel))
        flat.theta.add_(step.cuda())
        tv.store(lang, opt)
        thetas[lang] = flat.theta.clone()
        tv.restore_base(opt)
    return flat, opt, tv, thetas


def test_store_restore_and_merge_through_the_class():
    from indic_cl_asr_amd import cl
    flat, opt, tv, thetas = toy_vectors()
    base = tv.base.flat.clone()
    n = flat.numel
    assert same_bits(flat.theta, base) and same_bits(opt.shadow, base.bfloat16())         # restore_base: the bit patterns
    for row, lang in enumerate(("hi", "ta", "bn")):
        assert same_bits(tv.vectors[row, :n], thetas[lang] - base)                        # store: theta - base
    opt.exp_avg.fill_(0.5); opt.exp_avg_sq.fill_(0.25); opt.seg_step.fill_(3)
    taus, base_c = tv.vectors[:3, :n].cpu(), base.cpu()
    entries = list(flat.entries)
    # every language, in row order: the rows are read in place
    stats = tv.merge("task_arithmetic", scale=0.4, weights=[1.0, -0.5, 2.0])
    want, want16 = ref_linear(base_c, taus, [1.0, -0.5, 2.0], 0.4)
    assert same_bits(flat.theta, want) and same_bits(opt.shadow, want16)
    assert stats == {"method": "task_arithmetic", "languages": ["hi", "ta", "bn"], "coefficients": [1.0, -0.5, 2.0], "scale": 0.4}
    assert not opt.exp_avg.any() and not opt.exp_avg_sq.any() and not opt.seg_step.any()
    assert same_bits(tv.base.flat, base)                                                  # the base is only read
    # a subset in another order: gathered rows, the order of `languages` is the task order
    tv.merge("average", ["bn", "hi"])
    want, want16 = ref_linear(base_c, taus[[2, 0]], [0.5, 0.5], 1.0)
    assert same_bits(flat.theta, want) and same_bits(opt.shadow, want16)
    tv.merge("task_arithmetic", ["ta", "bn"], weights={"bn": 0.25, "ta": 3.0})
    want, want16 = ref_linear(base_c, taus[1:3], [3.0, 0.25], 1.0)
    assert same_bits(flat.theta, want) and same_bits(opt.shadow, want16)
    for scope, density, names, idx in (("tensor", 0.5, None, [0, 1, 2]), ("model", 0.2, ["bn", "ta", "hi"], [2, 1, 0])):
        stats = tv.merge("ties", names, density=density, scope=scope, scale=0.9)
        trim = cl.density_to_trim(density)
        cutoffs = ref_cutoffs(taus[idx], entries, trim, scope)
        want, want16, counts = ref_ties(base_c, taus[idx], cutoffs_per_element(cutoffs, entries, scope, n), 0.9, entries)
        assert same_bits(flat.theta, want) and same_bits(opt.shadow, want16)
        assert torch.equal(tv.cutoffs(3, scope).cpu(), cutoffs)
        assert stats["surviving"] == int(counts[:, 0].sum()) and stats["conflicts"] == int(counts[:, 1].sum())
        assert stats["cancelled"] == int(counts[:, 2].sum()) - (sum(e[2] for e in entries) - int(counts[:, 0].sum()))
        assert stats["tensors"]["mat"]["conflicts"] == int(counts[[e[0] for e in entries].index("mat"), 1]) > 0
        assert (stats["trim"], stats["scope"], stats["density"]) == (trim, scope, density)
    # back to the base, bit for bit, and from there a step runs
    tv.restore_base()
    assert same_bits(flat.theta, base) and same_bits(opt.shadow, base.bfloat16())
    # a merge without an optimizer writes no shadow and still moves the weight epoch
    from indic_cl_asr_amd.ops import fast
    tv._optimizer = None
    epoch, image = fast.WEIGHT_EPOCH, opt.shadow.clone()
    tv.merge("average")
    assert fast.WEIGHT_EPOCH > epoch and same_bits(opt.shadow, image)
    assert same_bits(flat.theta, ref_linear(base_c, taus, [1.0 / 3] * 3, 1.0)[0])


# ------------------------------------------------------------------------------------------ once through the model
def test_through_the_model_merged_forward_equals_a_fresh_model():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    from test_si_gpu import _batch

    def fresh():
        torch.manual_seed(0)
        return EncDecHybridRNNTCTCModel(model_config('tiny')).cuda().eval()

    def forward(model):
        with torch.no_grad():
            out, lens = model.forward(input_signal=sig, input_signal_length=sig_len)
        return out.clone(), lens.clone()

    (sig, sig_len, _, _), _ = _batch(['hi'] * 2, seed=5, B=2, L=8000)
    m = fresh()
    flat = cl.FlatParams(m)
    opt = cl.FusedAdamW(flat, lr=1e-3)
    tv = cl.TaskVectors(flat)
    tv.set_base(opt)
    start = {k: v.detach().clone() for k, v in m.state_dict().items()}
    y_base, _ = forward(m)                                           # fills every cache of weight images at the base
    float_buffers = [n for n, b in m.named_buffers() if b.is_floating_point()]
    int_buffers = [n for n, b in m.named_buffers() if not b.is_floating_point()]
    assert float_buffers and int_buffers
    kept = {}
    for seed, lang in ((1, "hi"), (2, "ta")):
        g = torch.Generator().manual_seed(90 + seed)
        with torch.no_grad():
            for p in flat.params:
                p.add_((torch.randn(p.shape, generator=g) * 2e-2).cuda())
            for n, b in m.named_buffers():                           # the BatchNorm statistics, as training would move them
                if "running_" in n:
                    b.mul_((1.0 + 0.2 * torch.rand(b.shape, generator=g)).cuda())
                elif n.endswith("num_batches_tracked"):
                    b.fill_(10 * seed)
        tv.store(lang, opt)
        kept[lang] = {n: b.detach().clone() for n, b in m.named_buffers()}
        tv.restore_base(opt)
    assert same_bits(forward(m)[0], y_base)                          # restore_base: weights, images and buffers are back
    n = flat.numel
    taus, base = tv.vectors[:2, :n].cpu(), tv.base.flat.cpu()
    entries = list(flat.entries)
    other = fresh()
    opt.exp_avg.fill_(0.5); opt.seg_step.fill_(3)
    for method in ("ties", "task_arithmetic"):
        if method == "ties":
            tv.merge("ties", density=0.2, scale=0.9, optimizer=opt)
            cutoffs = ref_cutoffs(taus, entries, cl.density_to_trim(0.2), "tensor")
            want, want16, _ = ref_ties(base, taus, cutoffs_per_element(cutoffs, entries, "tensor", n), 0.9, entries)
        else:
            tv.merge("task_arithmetic", scale=0.6, weights=[1.0, 0.5], optimizer=opt)
            want, want16 = ref_linear(base, taus, [1.0, 0.5], 0.6)
        assert same_bits(flat.theta, want) and same_bits(opt.shadow, want16)
        y, y_len = forward(m)
        # a fresh model given the torch-computed weights and the mean buffers
        other.load_state_dict(start)
        params = dict(other.named_parameters())
        with torch.no_grad():
            for name, off, k, shape in entries:
                params[name].copy_(want[off:off + k].view(shape).cuda())
            for name, b in other.named_buffers():
                if name in float_buffers:
                    b.copy_((kept["hi"][name] + kept["ta"][name]) / 2)
                else:
                    b.copy_(kept["ta"][name])
        for name, b in m.named_buffers():
            assert torch.equal(b, dict(other.named_buffers())[name]), name
        z, z_len = forward(other)
        assert torch.equal(y_len, z_len) and same_bits(y, z), method
        assert not same_bits(y, y_base)
    # the attached optimizer: fresh moments and step counters (PackNet's convention), and a step equal to that of a new
    # optimizer on a model that was given the merged weights
    assert not opt.exp_avg.any() and not opt.exp_avg_sq.any() and not opt.seg_step.any()
    g = torch.Generator().manual_seed(99)
    inside = torch.zeros(n, dtype=torch.bool)
    for _, off, k, _ in entries:
        inside[off:off + k] = True
    grad = torch.where(inside, torch.randn(n, generator=g) * 1e-2, torch.zeros(n)).cuda()
    flat2 = cl.FlatParams(other)
    opt2 = cl.FusedAdamW(flat2, lr=1e-3)
    assert list(flat2.entries) == entries and same_bits(flat2.theta, flat.theta)
    for f, o in ((flat, opt), (flat2, opt2)):
        f.grad.copy_(grad)
        o.step()
    torch.cuda.synchronize()
    assert same_bits(flat.theta, flat2.theta) and same_bits(opt.shadow, opt2.shadow) and same_bits(opt.exp_avg, opt2.exp_avg)
    assert not same_bits(flat.theta, want) and torch.isfinite(flat.theta).all()
    assert same_bits(forward(m)[0], forward(other)[0])
