"""cl.TaskVectors on the CPU (host logic only: no kernel is launched; ia_merge_linear, ia_merge_trim and ia_merge_ties run in
tests/test_merge_gpu.py): row bookkeeping, argument checks of the class and of the C entries, the density -> trim conversion,
buffer averaging, the state dict and its refusal of a foreign tensor table.

The second half is the pure-torch restatement of the three merge rules, one torch op per rounding, in task order:
`ref_linear`, `ref_cutoffs`, `ref_ties`.  The GPU tests import them as their reference (and nothing else computes one); here
they are held to small cases worked out by hand."""
import ctypes
import math

import pytest
import torch

ABS = 0x7FFFFFFF


# ------------------------------------------------------------------------------------------ the reference (torch fp32)
def f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def patterns(t):
    """The 31-bit pattern of |t| as int32: the order the trimming is defined in."""
    return t.contiguous().view(torch.int32) & ABS


def ref_linear(base, taus, coef, scale):
    """theta = base + scale * (coef_0 tau_0 + coef_1 tau_1 + ...), every product and sum one fp32 torch op, in task order.
    base [n], taus [K, n] -> (theta fp32, its bf16 image)."""
    s = taus[0] * f32(coef[0]).to(taus.device)
    for k in range(1, taus.shape[0]):
        s = s + taus[k] * f32(coef[k]).to(taus.device)
    theta = base + s * f32(scale).to(taus.device)
    return theta, theta.bfloat16()


def scope_groups(entries, scope):
    """The scope segments as lists of table entries: one per tensor, or one for the whole model."""
    return [[e] for e in entries] if scope == "tensor" else [list(entries)]


def trim_rank(trim, n):
    """r = floor((double)(float)trim * n)"""
    return math.floor(float(ctypes.c_float(trim).value) * n)


def ref_cutoffs(taus, entries, trim, scope, by_pattern=False):
    """int32 [K, scope segments]: the bit pattern of the r-th smallest |tau| of every (task, scope segment), 0 where r == 0.
    torch.kthvalue on abs(), as the authors' topk_values_mask does; by_pattern selects on the integer patterns instead (the
    definition, which also orders NaNs)."""
    groups = scope_groups(entries, scope)
    out = torch.zeros(taus.shape[0], len(groups), dtype=torch.int32, device=taus.device)
    for k in range(taus.shape[0]):
        for s, group in enumerate(groups):
            vals = torch.cat([taus[k, off:off + n] for _, off, n, _ in group])
            r = trim_rank(trim, vals.numel())
            if r > 0:
                if by_pattern:
                    out[k, s] = patterns(vals).kthvalue(r).values
                else:
                    out[k, s] = vals.abs().kthvalue(r).values.view(torch.int32)
    return out


def cutoffs_per_element(cutoffs, entries, scope, numel):
    """[K, numel] int32: every element's cutoff (0 in the alignment gaps)."""
    per = torch.zeros(cutoffs.shape[0], numel, dtype=torch.int32, device=cutoffs.device)
    for s, group in enumerate(scope_groups(entries, scope)):
        for _, off, n, _ in group:
            per[:, off:off + n] = cutoffs[:, s:s + 1]
    return per


def ref_ties(base, taus, cut_elem, scale, entries):
    """TIES after the trimming, per element: t_k = tau_k where |tau_k| >= cutoff (pattern order) else +0; mass = t_0 + t_1 + ...;
    the entries with the sign of the mass are added in task order and divided by their number; theta = base + scale * that.
    -> (theta, bf16 image, int32 [tensors, 3]: elements with an entry != 0, with entries of both signs, with zero mass)."""
    K = taus.shape[0]
    t = torch.where(patterns(taus) >= cut_elem.to(taus.device), taus, torch.zeros_like(taus))
    mass = t[0].clone()
    for k in range(1, K):
        mass = mass + t[k]
    pos, neg = mass > 0, mass < 0
    acc, cnt = torch.zeros_like(mass), torch.zeros_like(mass)
    for k in range(K):
        sel = (pos & (t[k] > 0)) | (neg & (t[k] < 0))
        acc = acc + torch.where(sel, t[k], torch.zeros_like(mass))
        cnt = cnt + sel.to(torch.float32)
    m = torch.where(cnt > 0, acc / cnt.clamp(min=1.0), torch.zeros_like(mass))
    theta = base + m * f32(scale).to(taus.device)
    any_entry, both, zero = (t != 0).any(0), (t > 0).any(0) & (t < 0).any(0), mass == 0
    flags = torch.stack([any_entry, both, zero]).to(torch.int32)
    counts = torch.stack([flags[:, off:off + n].sum(1) for _, off, n, _ in entries]).to(torch.int32).cpu()
    return theta, theta.bfloat16(), counts


# ------------------------------------------------------------------------------------------ the reference, by hand
def test_reference_linear_by_hand():
    base = torch.tensor([1.0, -2.0, 0.5, 0.0])
    taus = torch.tensor([[1.0, 2.0, -1.0, 0.0], [3.0, -2.0, 0.25, 0.0], [0.5, 0.5, 0.5, 0.0]])
    theta, image = ref_linear(base, taus, [1.0, -1.0, 0.0], 0.5)
    assert theta.tolist() == [0.0, 0.0, 0.5 + 0.5 * -1.25, 0.0]
    assert image.dtype == torch.bfloat16 and torch.equal(image, theta.bfloat16())
    avg, _ = ref_linear(base, taus[:2], [0.5, 0.5], 1.0)
    assert avg.tolist() == [3.0, -2.0, 0.5 - 0.375, 0.0]
    # every rounding on its own: (0.1f * 3) + (0.1f * 7) is not 0.1f * 10
    one = torch.ones(1)
    got, _ = ref_linear(torch.zeros(1), torch.stack([3 * one, 7 * one]), [0.1, 0.1], 1.0)
    assert got.item() == (f32(0.1) * 3 + f32(0.1) * 7).item()


def test_reference_cutoffs_by_hand_and_in_both_orders():
    entries = [("a", 0, 5, (5,)), ("b", 64, 4, (4,))]
    taus = torch.zeros(2, 128)
    taus[0, :5] = torch.tensor([0.5, -3.0, 2.0, -0.5, 1.0])
    taus[0, 64:68] = torch.tensor([-4.0, 0.25, 0.25, -0.0])
    taus[1, :5] = torch.tensor([float("nan"), float("inf"), -1.0, 1.0, 0.0])
    taus[1, 64:68] = torch.tensor([1.0, 1.0, 1.0, 1.0])
    pat = lambda x: int(f32(x).view(torch.int32))
    # trim 0.5: r = floor(2.5) = 2 of 5 and 2 of 4, per tensor
    c = ref_cutoffs(taus, entries, 0.5, "tensor")
    assert c.tolist() == [[pat(0.5), pat(0.25)], [pat(1.0), pat(1.0)]]
    # the whole vector: r = floor(4.5) = 4 of 9; gaps are not counted
    c = ref_cutoffs(taus, entries, 0.5, "model")
    assert c.tolist() == [[pat(0.5)], [pat(1.0)]]
    # r = floor(0.19 * 5) = 0: nothing is trimmed, the cutoff is 0
    assert ref_cutoffs(taus, entries, 0.19, "tensor").tolist() == [[0, 0], [0, 0]]
    # kthvalue on the floats and on the patterns agree, with inf and one NaN on top
    for trim in (0.0, 0.2, 0.5, 0.8, 0.9):
        for scope in ("tensor", "model"):
            assert torch.equal(ref_cutoffs(taus, entries, trim, scope), ref_cutoffs(taus, entries, trim, scope, by_pattern=True))
    assert ref_cutoffs(taus, entries, 0.8, "tensor")[1, 0].item() == pat(float("inf"))       # r = 4 of 5: NaN is the largest
    per = cutoffs_per_element(ref_cutoffs(taus, entries, 0.5, "tensor"), entries, "tensor", 128)
    assert per[0, :5].tolist() == [pat(0.5)] * 5 and per[0, 5:64].tolist() == [0] * 59 and per[1, 64:68].tolist() == [pat(1.0)] * 4


def test_reference_ties_by_hand():
    entries = [("a", 0, 8, (8,))]
    n = 64
    #                 agree   conflict (two small minority vs one large)   all trimmed   cancel   -0 entries   one survivor
    rows = [[2.0,     -1.0,                                                 0.1,          3.0,     -0.0,        0.1,   0.0, 0.0],
            [4.0,     -1.5,                                                 -0.1,         -3.0,    -0.0,        5.0,   0.0, 0.0],
            [6.0,     9.0,                                                  0.1,          0.0,     0.0,         -0.1,  0.0, 0.0]]
    taus = torch.zeros(3, n)
    taus[:, :8] = torch.tensor(rows)
    base = torch.full((n,), 10.0)
    cut = torch.zeros(3, n, dtype=torch.int32)
    cut[:, :8] = int(f32(0.5).view(torch.int32))
    theta, image, counts = ref_ties(base, taus, cut, 2.0, entries)
    #   agree: mean 4;  conflict: mass 6.5 > 0, only the 9 carries the sign;  trimmed: base;  cancel: base;  zeros: base;  5 alone
    assert theta[:8].tolist() == [18.0, 28.0, 10.0, 10.0, 10.0, 20.0, 10.0, 10.0]
    assert torch.equal(image, theta.bfloat16())
    assert counts.tolist() == [[4, 2, 5]]            # entries: 0, 1, 3, 5;  both signs: 1, 3;  zero mass: 2, 3, 4, 6, 7
    # a minority that is larger in number loses to the larger mass, and the mean is over the winners only
    taus2 = torch.zeros(3, n)
    taus2[:, 0] = torch.tensor([-1.0, -1.5, 9.0])
    taus2[:, 1] = torch.tensor([1.0, 2.0, -2.5])
    theta2, _, counts2 = ref_ties(torch.zeros(n), taus2, torch.zeros(3, n, dtype=torch.int32), 1.0, entries)
    assert theta2[:2].tolist() == [9.0, 1.5] and counts2.tolist() == [[2, 2, 6]]


# ------------------------------------------------------------------------------------------ host logic of cl.TaskVectors
class Net(torch.nn.Module):
    """Odd sizes (alignment gaps, a tail shorter than a float4) and BatchNorm buffers: two floating-point, one integer."""

    def __init__(self, seed=3):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.a = torch.nn.Parameter(torch.randn(3, generator=g))
        self.w = torch.nn.Parameter(torch.randn(5, 13, generator=g))
        self.b = torch.nn.Parameter(torch.randn(70, generator=g))
        self.bn = torch.nn.BatchNorm1d(4)


def _tv(**kw):
    from indic_cl_asr_amd import cl
    flat = cl.FlatParams(Net())
    return flat, cl.TaskVectors(flat, **kw)


def _finetune(flat, seed):
    """What fine-tuning leaves: other weights inside the tensors (the gaps stay +0) and other buffers."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in flat.params:
            p.add_(torch.randn(p.shape, generator=g) * 0.1)
        bn = flat.model.bn
        bn.running_mean.copy_(torch.randn(4, generator=g))
        bn.running_var.copy_(torch.rand(4, generator=g) + 0.5)
        bn.num_batches_tracked.fill_(seed)


def test_rows_store_overwrite_drop_order():
    flat, tv = _tv(max_tasks=3)
    assert tv.languages() == [] and tv.stats()["has_base"] is False
    with pytest.raises(RuntimeError, match="no base has been set"):
        tv.store("hi")
    tv.set_base()
    base = flat.theta.clone()
    assert torch.equal(tv.base.flat, base) and tv.base.flat.data_ptr() != flat.theta.data_ptr()
    thetas = {}
    for seed, lang in enumerate(("hi", "ta", "bn"), start=1):
        _finetune(flat, seed)
        tv.store(lang)
        thetas[lang] = flat.theta.clone()
        tv.restore_base()
        assert torch.equal(flat.theta.view(torch.int32), base.view(torch.int32))
        assert int(flat.model.bn.num_batches_tracked) == 0
    assert tv.languages() == ["hi", "ta", "bn"] and tv.stride == flat.numel and tv.vectors.shape == (3, tv.stride)
    for lang in tv.languages():
        assert torch.equal(tv.vectors[tv._rows[lang], :flat.numel], thetas[lang] - base)
        assert torch.equal(tv.task_vector(lang)["w"], (thetas[lang] - base)[64:64 + 65].view(5, 13))
    gaps = torch.ones(flat.numel, dtype=torch.bool)
    for _, off, n, _ in flat.entries:
        gaps[off:off + n] = False
    assert not tv.vectors[:, :flat.numel][:, gaps].view(torch.int32).any()             # +0 in the alignment gaps
    with pytest.raises(ValueError, match="max_tasks = 3 languages are stored already; 'mr' would be one more"):
        tv.store("mr")
    # storing a language again overwrites its row and keeps the order
    _finetune(flat, 7)
    tv.store("ta")
    assert tv.languages() == ["hi", "ta", "bn"] and torch.equal(tv.vectors[1, :flat.numel], flat.theta - base)
    assert int(tv.buffers["ta"]["bn.num_batches_tracked"]) == 7
    tv.restore_base()
    # dropping moves the later rows up
    bn_row = tv.vectors[2].clone()
    tv.drop("ta")
    assert tv.languages() == ["hi", "bn"] and tv._rows == {"hi": 0, "bn": 1} and set(tv.buffers) == {"hi", "bn"}
    assert torch.equal(tv.vectors[1], bn_row) and not tv.vectors[2].any()
    with pytest.raises(ValueError, match="unknown language 'ta'"):
        tv.drop("ta")
    tv.store("mr")
    assert tv.languages() == ["hi", "bn", "mr"]
    st = tv.stats()
    assert (st["rows_in_use"], st["rows_allocated"], st["max_tasks"], st["bytes_vectors"]) == (3, 3, 3, 4 * 3 * tv.stride)
    # a new base drops the vectors: they are differences from the old one
    tv.set_base()
    assert tv.languages() == [] and tv.buffers == {}


def test_rows_are_allocated_on_demand():
    flat, tv = _tv()
    assert tv.max_tasks == 32 and tv.vectors is None
    tv.set_base()
    sizes = []
    for k in range(5):
        tv.store(f"l{k}")
        sizes.append(tv.vectors.shape[0])
    assert sizes == [1, 2, 4, 4, 8]
    from indic_cl_asr_amd import cl
    for bad in (0, 33):
        with pytest.raises(ValueError, match=r"max_tasks must be in 1\.\.32"):
            cl.TaskVectors(flat, max_tasks=bad)


def test_merge_argument_checks_launch_nothing():
    flat, tv = _tv()
    with pytest.raises(RuntimeError, match="no base has been set"):
        tv.merge("average")
    tv.set_base()
    for lang in ("hi", "ta"):
        _finetune(flat, 1)
        tv.store(lang)
    before = flat.theta.clone()
    bad = [(dict(method="dare"), "unknown method 'dare'"),
           (dict(method="ties", scope="layer"), "unknown scope 'layer'"),
           (dict(method="average", languages=[]), "no language to merge"),
           (dict(method="average", languages=["hi", "mr"]), "unknown language 'mr'"),
           (dict(method="average", languages=["hi", "hi"]), "listed twice"),
           (dict(method="task_arithmetic", scale=float("inf")), "scale must be finite"),
           (dict(method="task_arithmetic", scale=float("nan")), "scale must be finite"),
           (dict(method="task_arithmetic", weights=[1.0]), "1 weights for 2 languages"),
           (dict(method="task_arithmetic", weights=[1.0, float("nan")]), "weights must be finite"),
           (dict(method="average", weights=[0.5, 0.5]), "weights belong to 'task_arithmetic'"),
           (dict(method="ties", weights=[0.5, 0.5]), "weights belong to 'task_arithmetic'"),
           (dict(method="average", scale=0.5), "its scale is 1"),
           (dict(method="ties", density=0.0), r"outside \(0, 1\]"),
           (dict(method="ties", density=1.5), r"outside \(0, 1\]"),
           (dict(method="ties", density=float("nan")), r"outside \(0, 1\]"),
           (dict(method="ties", density=1e-9), "too small")]
    for kw, message in bad:
        with pytest.raises(ValueError, match=message):
            tv.merge(**kw)
    # the arithmetic is the HIP kernels': no eager fallback on a host model
    with pytest.raises(RuntimeError, match="runs on the HIP kernels"):
        tv.merge("average")
    assert torch.equal(flat.theta, before)
    names, coef, scale, trim = tv._checked_merge("average", None, 1.0, None, 0.2, "tensor")
    assert (names, coef, scale, trim) == (["hi", "ta"], [0.5, 0.5], 1.0, None)
    names, coef, _, trim = tv._checked_merge("task_arithmetic", ["ta", "hi"], 0.3, {"hi": 2.0, "ta": -1.0}, 0.2, "tensor")
    assert (names, coef, trim) == (["ta", "hi"], [-1.0, 2.0], None)
    assert tv._checked_merge("ties", None, 1.0, None, 0.2, "model")[3] == ctypes.c_float(0.8).value


def test_density_becomes_trim_in_double_then_float():
    from indic_cl_asr_amd import cl
    assert cl.density_to_trim(1.0) == 0.0 and cl.density_to_trim(0.5) == 0.5
    for density in (0.2, 0.1, 1.0 / 3, 1.0 / 4161, 1e-6):
        trim = cl.density_to_trim(density)
        assert trim == ctypes.c_float(1.0 - density).value and 0.0 <= trim < 1.0
    # the rank is floor((double)trim * n) on that float: float32(0.8) = 0.800000011920929 lies above 0.8
    assert trim_rank(cl.density_to_trim(0.2), 10) == 8 and trim_rank(cl.density_to_trim(0.2), 5) == 4
    assert trim_rank(cl.density_to_trim(0.5), 4161) == 2080 and trim_rank(cl.density_to_trim(1.0), 4161) == 0
    assert all(trim_rank(cl.density_to_trim(1.0 / n), n) in (n - 2, n - 1) for n in (3, 65, 4096, 4161, 8197))
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match=r"outside \(0, 1\]"):
            cl.density_to_trim(bad)
    with pytest.raises(ValueError, match="rounds to 1 in fp32"):
        cl.density_to_trim(2.0 ** -26)


def test_buffers_float_mean_integer_from_the_last():
    flat, tv = _tv()
    tv.set_base()
    for seed, lang in enumerate(("hi", "ta", "bn"), start=1):
        _finetune(flat, seed)
        tv.store(lang)
        tv.restore_base()
    b = tv.buffers
    merged = tv.merged_buffers(["bn", "hi", "ta"])
    for key in ("bn.running_mean", "bn.running_var"):
        assert torch.equal(merged[key], (b["bn"][key] + b["hi"][key] + b["ta"][key]) / 3)
    assert merged["bn.num_batches_tracked"].dtype == torch.int64 and int(merged["bn.num_batches_tracked"]) == 2     # ta's
    two = tv.merged_buffers(["ta", "bn"])
    assert torch.equal(two["bn.running_mean"], (b["ta"]["bn.running_mean"] + b["bn"]["bn.running_mean"]) / 2)
    assert int(two["bn.num_batches_tracked"]) == 3
    one = tv.merged_buffers(["hi"])
    assert all(torch.equal(one[k], b["hi"][k]) for k in one) and one["bn.running_var"].data_ptr() != b["hi"]["bn.running_var"].data_ptr()


def test_state_dict_round_trips_through_save_masks_and_refuses_a_foreign_table(tmp_path):
    from indic_cl_asr_amd import checkpoint, cl
    flat, tv = _tv(max_tasks=4)
    tv.set_base()
    for seed, lang in enumerate(("hi", "ta", "bn"), start=1):
        _finetune(flat, seed)
        tv.store(lang)
        tv.restore_base()
    sd = tv.state_dict()
    assert set(sd) == {"entries", "max_tasks", "base", "base_buffers", "task_languages", "vectors", "buffers"}
    assert sd["task_languages"] == ["hi", "ta", "bn"] and sd["vectors"].shape == (3, flat.numel)
    path = str(tmp_path / "vectors.pt")
    checkpoint.save_masks(tv, path)
    flat2, tv2 = _tv(max_tasks=4)
    tv2.set_base()
    tv2.store("xx")
    assert checkpoint.load_masks(tv2, path) is tv2
    assert tv2.languages() == ["hi", "ta", "bn"] and tv2._rows == tv._rows
    assert torch.equal(tv2.base.flat, tv.base.flat) and torch.equal(tv2.vectors[:3], tv.vectors[:3])
    assert "xx" not in tv2.buffers and not tv2.vectors[3:].any()
    for lang in tv.languages():
        assert all(torch.equal(tv2.buffers[lang][k], tv.buffers[lang][k]) for k in tv.buffers[lang])
    assert all(torch.equal(tv2.base_buffers[k], tv.base_buffers[k]) for k in tv.base_buffers)
    # a loader without a base of its own, and with too few rows
    flat3, tv3 = _tv(max_tasks=2)
    with pytest.raises(ValueError, match="3 task vectors were saved, max_tasks here is 2"):
        checkpoint.load_masks(tv3, path)
    flat3, tv3 = _tv()
    checkpoint.load_masks(tv3, path)
    assert torch.equal(tv3.base.flat, tv.base.flat) and tv3.languages() == ["hi", "ta", "bn"]
    # another set of trainable tensors
    other = cl.FlatParams(torch.nn.Linear(3, 2))
    with pytest.raises(ValueError, match="'masks' was saved for a different set of trainable tensors"):
        checkpoint.load_masks(cl.TaskVectors(other), path)
    # another kind of state behind the same table
    with pytest.raises(ValueError, match="does not hold task vectors"):
        tv3.load_state_dict({"entries": list(flat3.entries), "owner": None}, source="x")
    with pytest.raises(ValueError, match="does not hold a PackNet owner map"):
        cl.PackNet(flat3).load_state_dict(sd, source="x")


# ------------------------------------------------------------------------------------------ argument checks of the C entries
def _host_args():
    """Aligned host buffers standing in for device pointers: every call below is refused before any device work."""
    buf = (ctypes.c_float * 1024)()
    at = ctypes.addressof(buf)
    at += -at % 16
    p = lambda k=0: ctypes.c_void_p(at + k)
    return buf, p


def test_c_entries_refuse_bad_arguments_before_any_device_work():
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    buf, p = _host_args()
    coef = (ctypes.c_float * 32)(*([1.0] * 32))
    inf, nan = float("inf"), float("nan")
    # ia_merge_linear(theta, base, vectors, stride, ntasks, coef, scale, chunk_table, nchunks, shadow, stream)
    good = [p(0), p(256), p(512), 64, 2, coef, 1.0, p(1024), 1, None, None]
    for at, value in ((0, None), (1, None), (2, None), (5, None), (7, None), (4, 0), (4, 33), (4, -1), (6, inf), (6, -inf),
                      (6, nan), (8, 0), (3, 0), (3, 6), (0, p(4)), (1, p(8)), (2, p(4)), (7, p(4)), (9, p(2))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_linear(*args) == -1, (at, value)
    # ia_merge_trim(vectors, stride, ntasks, chunk_table, nchunks, seg_of_scope, nscope, trim, cutoffs, workspace, bytes, stream)
    assert L.ia_merge_trim_workspace_bytes(2, 3) == 2 * 3 * (16 + 256 * 4)
    assert L.ia_merge_trim_workspace_bytes(0, 3) == L.ia_merge_trim_workspace_bytes(33, 3) == L.ia_merge_trim_workspace_bytes(2, 0) == 0
    good = [p(0), 64, 2, p(1024), 1, p(2048), 1, 0.5, p(2304), p(2560), 1 << 20, None]
    for at, value in ((0, None), (3, None), (5, None), (8, None), (9, None), (2, 0), (2, 33), (4, 0), (6, 0), (7, 1.0), (7, -0.1),
                      (7, nan), (7, inf), (1, 0), (1, 2), (0, p(4)), (3, p(8)), (5, p(2)), (8, p(2)), (9, p(8))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_trim(*args) == -1, (at, value)
    args = list(good)
    args[10] = L.ia_merge_trim_workspace_bytes(2, 1) - 1
    assert L.ia_merge_trim(*args) == -2                                  # IA_WORKSPACE_TOO_SMALL, also before any device work
    # ia_merge_ties(theta, base, vectors, stride, ntasks, cutoffs, seg_of_scope, nscope, scale, chunk_table, nchunks, nseg,
    #               shadow, seg_counts, stream)
    good = [p(0), p(256), p(512), 64, 2, p(2304), p(2048), 1, 1.0, p(1024), 1, 1, None, p(2560), None]
    for at, value in ((0, None), (1, None), (2, None), (5, None), (6, None), (9, None), (13, None), (4, 0), (4, 33), (7, 0),
                      (8, inf), (8, nan), (10, 0), (11, 0), (3, -4), (3, 5), (0, p(8)), (1, p(4)), (2, p(8)), (5, p(2)),
                      (6, p(2)), (9, p(4)), (12, p(4)), (13, p(2))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_ties(*args) == -1, (at, value)
    assert not any(buf)
