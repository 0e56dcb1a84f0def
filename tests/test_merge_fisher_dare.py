"""Fisher merging and DARE of cl.TaskVectors on the CPU (no kernel is launched; ia_merge_fisher, ia_merge_linear_dare and
ia_merge_ties_dare run in tests/test_merge_fisher_dare_gpu.py).

The first part is the reference the GPU tests compare with, bit for bit: `ref_fisher` (one torch fp32 op per rounding, in task
order), `dare_keep` (an integer numpy replica of the kernels' hash) and `ref_dare_rows`, whose result goes through the
`ref_linear` and `ref_ties` of tests/test_merge.py.  `ref_fisher` is held to cases worked out by hand, the hash to the
statistics a Bernoulli mask would have: a keep count X of n independent draws with probability p has mean n p and standard
deviation sqrt(n p (1 - p)); 5 sigma is exceeded by chance once in 1.7 million.  These are conditions on the hash.

The second part is host logic: the density -> threshold conversion, the importance bookkeeping, the state dict, every new
ValueError and the argument checks of the three C entries."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_merge import Net, _finetune, _host_args, _tv, f32, ref_linear, ref_ties

M32 = 0xFFFFFFFF


# ------------------------------------------------------------------------------------------ the reference (torch fp32, numpy ints)
def ref_fisher(base, taus, fishers, coef, floor, scale, entries):
    """g_k = F_k > floor ? F_k : floor; a_k = coef_k g_k; num = a_0 tau_0 + a_1 tau_1 + ...; den = a_0 + a_1 + ...;
    theta = base + scale * (den > 0 ? num / den : +0).  -> (theta, bf16 image, int32 [tensors, 2]: elements where no F_k
    exceeded the floor, elements with den == 0)."""
    fl = f32(floor)
    num = den = None
    floored = torch.ones(taus.shape[1], dtype=torch.bool)
    for k in range(taus.shape[0]):
        above = fishers[k] > fl
        a = torch.where(above, fishers[k], fl) * f32(coef[k])
        p = a * taus[k]
        num = p if k == 0 else num + p
        den = a if k == 0 else den + a
        floored &= ~above
    positive = den > 0
    m = torch.where(positive, num / torch.where(positive, den, torch.ones_like(den)), torch.zeros_like(num))
    theta = base + m * f32(scale)
    flags = torch.stack([floored, den == 0]).to(torch.int32)
    counts = torch.stack([flags[:, off:off + n].sum(1) for _, off, n, _ in entries]).to(torch.int32)
    return theta, theta.bfloat16(), counts


def hash32(x):
    """ia_dm_hash32 of csrc/dropout_mask.h on a uint64 array holding 32-bit values."""
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x85EBCA6B)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(13))
    x = (x * np.uint64(0xC2B2AE35)) & np.uint64(M32)
    return x ^ (x >> np.uint64(16))


def dare_hash(seed, K, numel):
    """uint64 [K, numel]: h = H(i * 0x9E3779B1 + H(H(seed) ^ (k + 1))) in 32-bit arithmetic."""
    i = np.arange(numel, dtype=np.uint64)
    hseed = hash32(np.array([seed], dtype=np.uint64))
    rows = []
    for k in range(K):
        key = hash32(hseed ^ np.uint64(k + 1))
        rows.append(hash32((i * np.uint64(0x9E3779B1) + key) & np.uint64(M32)))
    return np.stack(rows)


def dare_keep(seed, K, numel, threshold):
    """bool [K, numel]: entry i of the k-th listed language is kept iff its hash is below the threshold."""
    return torch.from_numpy(dare_hash(seed, K, numel) < np.uint64(threshold))


def ref_dare_rows(taus, keep, keep_prob):
    """t = keep ? tau / keep_prob : +0, the quotient one fp32 torch op."""
    return torch.where(keep, taus / f32(keep_prob), torch.zeros_like(taus))


# ------------------------------------------------------------------------------------------ ref_fisher, by hand
ONE = [("a", 0, 4, (4,))]


def _fisher(taus, fishers, coef, floor, scale=1.0, base=10.0):
    n = 64
    t, f = torch.zeros(len(taus), n), torch.zeros(len(taus), n)
    t[:, :4], f[:, :4] = torch.tensor(taus), torch.tensor(fishers)
    theta, image, counts = ref_fisher(torch.full((n,), base), t, f, coef, floor, scale, ONE)
    assert torch.equal(image, theta.bfloat16())
    return theta[:4].tolist(), counts.tolist()


def test_reference_fisher_by_hand():
    nan = float("nan")
    # equal Fishers: the weighted mean (1 * 2 + 3 * 6) / 4 = 5, whatever the Fisher is; scale 2
    theta, counts = _fisher([[2.0] * 4, [6.0] * 4], [[0.5, 0.25, 8.0, 1.0]] * 2, [1.0, 3.0], 0.0, scale=2.0)
    assert theta == [20.0] * 4 and counts == [[0, 0]]
    # one dominant Fisher (the others exactly zero, floor 0) returns that language's tau
    theta, counts = _fisher([[1.0, 2.0, 3.0, 4.0], [-5.0] * 4, [7.0] * 4], [[0.0] * 4, [0.5, 1.0, 2.0, 0.125], [0.0] * 4],
                            [1.0, 1.0, 1.0], 0.0)
    assert theta == [5.0] * 4 and counts == [[0, 0]]
    # all-zero Fisher with floor 0: den == 0, the base, counted as unweighted (and as floored: nothing exceeded the floor)
    theta, counts = _fisher([[1.0] * 4, [3.0] * 4], [[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0]], [1.0, 1.0], 0.0)
    assert theta == [10.0, 10.0, 12.0, 10.0] and counts == [[3, 3]]
    # the same with a floor: a plain mean, floored but weighted
    theta, counts = _fisher([[1.0] * 4, [3.0] * 4], [[0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 1.0, 0.0]], [1.0, 1.0], 0.5)
    assert theta == [12.0] * 4 and counts == [[3, 0]]
    # a NaN or a negative Fisher is the floor: columns 0 and 1 weigh 0.25 : 0.25, column 2 is 0.25 : 0.75, column 3 is above
    theta, counts = _fisher([[4.0] * 4, [8.0] * 4], [[nan, -1.0, nan, 0.5], [-2.0, nan, 0.75, 0.5]], [1.0, 1.0], 0.25)
    assert theta == [16.0, 16.0, 17.0, 16.0] and counts == [[2, 0]]
    # an importance equal to the floor is "at or below" it
    _, counts = _fisher([[4.0] * 4, [8.0] * 4], [[0.25] * 4, [0.25, 0.25, 0.25, 0.5]], [1.0, 1.0], 0.25)
    assert counts == [[3, 0]]
    # every rounding on its own: (0.1f * 3) + (0.1f * 7) over 0.1f + 0.1f
    theta, _ = _fisher([[3.0] * 4, [7.0] * 4], [[0.1] * 4] * 2, [1.0, 1.0], 0.0, base=0.0)
    assert theta[0] == ((f32(0.1) * 3 + f32(0.1) * 7) / (f32(0.1) + f32(0.1))).item()


def test_reference_dare_rows_by_hand():
    taus = torch.tensor([[1.0, -0.0, 3.0, float("nan")], [0.3, 0.3, -0.3, 0.3]])
    keep = torch.tensor([[True, True, False, False], [True, False, True, False]])
    got = ref_dare_rows(taus, keep, 0.5)
    assert got[0].tolist() == [2.0, -0.0, 0.0, 0.0] and math.copysign(1.0, got[0, 1].item()) == -1.0
    assert got[1].tolist() == [(f32(0.3) / f32(0.5)).item(), 0.0, (f32(-0.3) / f32(0.5)).item(), 0.0]
    assert torch.equal(ref_dare_rows(taus[1:], keep[1:], 1.0), torch.where(keep[1:], taus[1:], torch.zeros(1, 4)))
    # the quotient, not a product with the reciprocal: 1 / 0.1f is not 10
    x = torch.tensor([[5.0, 7.0, 11.0, 13.0]])
    assert torch.equal(ref_dare_rows(x, torch.ones(1, 4, dtype=torch.bool), 0.1), x / f32(0.1))


# ------------------------------------------------------------------------------------------ the mask's statistics
def toy_numel():
    """The flat length of Toy(big=False) of tests/test_optimizer_clip_gpu.py: every tensor starts on a multiple of 64."""
    sizes = [1, 3, 4, 63, 64, 65, 4095, 4096, 4097, 2 * 4096 + 5, 65 * 63, 130]
    return sum((n + 63) // 64 * 64 for n in sizes)


def within(count, n, p):
    return abs(count - n * p) <= 5.0 * math.sqrt(n * p * (1.0 - p))


def test_hash_replica_values():
    """Three values of the finaliser worked out from its definition, so that the replica cannot drift with the kernel's."""
    assert int(hash32(np.array([0], dtype=np.uint64))[0]) == 0
    x = 1
    x ^= x >> 16; x = x * 0x85EBCA6B & M32; x ^= x >> 13; x = x * 0xC2B2AE35 & M32; x ^= x >> 16
    assert int(hash32(np.array([1], dtype=np.uint64))[0]) == x
    h = dare_hash(0, 2, 3)
    key1 = int(hash32(np.array([2], dtype=np.uint64))[0])                  # H(H(0) ^ 2), H(0) = 0
    assert int(h[1, 2]) == int(hash32(np.array([(2 * 0x9E3779B1 + key1) & M32], dtype=np.uint64))[0])
    assert h.max() <= M32 and dare_keep(0, 2, 3, 0).sum() == 0


@pytest.mark.parametrize("density", [0.5, 0.1, 0.01])
def test_keep_rate(density):
    from indic_cl_asr_amd import cl
    n = toy_numel()
    threshold, _ = cl.density_to_keep(density)
    for seed in (0, 1, 12345, M32):
        keep = dare_keep(seed, 5, n, threshold)
        for k in range(5):
            assert within(int(keep[k].sum()), n, density), (seed, k, int(keep[k].sum()), n * density)
        assert within(int(keep.sum()), 5 * n, density)


def test_keep_is_independent_across_rows_seeds_and_neighbours():
    from indic_cl_asr_amd import cl
    n = toy_numel()
    threshold, _ = cl.density_to_keep(0.5)
    for seed, other in ((0, 1), (1, 2), (12345, 12346), (7, 1 << 31)):
        a, b = dare_keep(seed, 5, n, threshold), dare_keep(other, 5, n, threshold)
        for k in range(4):
            assert within(int((a[k] & a[k + 1]).sum()), n, 0.25), ("rows", seed, k)            # two rows of one seed
        assert within(int((a[0] & a[4]).sum()), n, 0.25)
        for k in range(5):
            assert within(int((a[k] & b[k]).sum()), n, 0.25), ("seeds", seed, other, k)        # one row of two seeds
            assert within(int((a[k, :-1] & a[k, 1:]).sum()), n - 1, 0.25), ("neighbours", seed, k)


# ------------------------------------------------------------------------------------------ host logic
def test_density_becomes_a_32_bit_threshold():
    from indic_cl_asr_amd import cl
    assert cl.density_to_keep(1.0) == (M32, 1.0)                               # 2^32 does not fit: the largest threshold
    assert cl.density_to_keep(0.5) == (1 << 31, 0.5)
    assert cl.density_to_keep(2.0 ** -32) == (1, 2.0 ** -32)
    assert cl.density_to_keep(0.1) == (math.floor(0.1 * 2.0 ** 32), ctypes.c_float(0.1).value)
    assert cl.density_to_keep(0.99)[0] == math.floor(0.99 * 2.0 ** 32) < M32
    assert cl.density_to_keep(0.1, rescale=False) == (math.floor(0.1 * 2.0 ** 32), 1.0)
    for bad in (0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match=r"outside \(0, 1\]"):
            cl.density_to_keep(bad)
    with pytest.raises(ValueError, match="too small"):
        cl.density_to_keep(2.0 ** -33)
    assert cl.MERGE_METHODS == ("task_arithmetic", "average", "ties", "fisher", "dare_linear", "dare_ties")


def _importance(flat, seed, gaps=0.0):
    """A FlatDict of the layout with seeded values inside the tensors and `gaps` between them."""
    g = torch.Generator().manual_seed(seed)
    d = flat.zeros()
    d.flat.fill_(gaps)
    for name in d:
        d[name].copy_(torch.rand(d[name].shape, generator=g))
    return d


def _stored(max_tasks=4):
    flat, tv = _tv(max_tasks=max_tasks)
    tv.set_base()
    for seed, lang in enumerate(("hi", "ta", "bn"), start=1):
        _finetune(flat, seed)
        tv.store(lang)
        tv.restore_base()
    return flat, tv


def test_importance_rows_follow_store_drop_and_set_base():
    flat, tv = _stored()
    n = flat.numel
    assert tv.importances is None and tv.stats()["importance_languages"] == [] and tv.stats()["bytes_importances"] == 0
    with pytest.raises(ValueError, match="no importance is stored for 'hi'"):
        tv.importance("hi")
    imp = {lang: _importance(flat, 10 + k, gaps=float("nan")) for k, lang in enumerate(("hi", "ta", "bn", "mr"))}
    tv.set_importance("ta", imp["ta"])
    assert tv.importances.shape == tv.vectors.shape == (4, tv.stride) and tv.importances.data_ptr() != imp["ta"].flat.data_ptr()
    assert tv.stats()["importance_languages"] == ["ta"] and tv.stats()["bytes_importances"] == 4 * 4 * tv.stride
    inside = torch.zeros(n, dtype=torch.bool)
    for _, off, k, _ in flat.entries:
        inside[off:off + k] = True
    assert torch.equal(tv.importances[1, :n][inside], imp["ta"].flat[inside])
    assert not tv.importances[1, :n][~inside].view(torch.int32).any()               # +0 in the gaps, whatever the source held
    assert not tv.importances[0].any() and not tv.importances[2:].any()
    assert torch.equal(tv.importance("ta")["w"], imp["ta"]["w"]) and tv.importance("ta")["w"].shape == (5, 13)
    # store(..., importance=) on a new and on a stored language; the latter keeps its row
    _finetune(flat, 9)
    tv.store("bn", importance=imp["bn"])
    tv.store("mr", importance=imp["mr"])
    tv.restore_base()
    assert tv.languages() == ["hi", "ta", "bn", "mr"] and tv.stats()["importance_languages"] == ["ta", "bn", "mr"]
    assert torch.equal(tv.importance("mr")["b"], imp["mr"]["b"])
    # storing again without an importance keeps the one there is
    tv.store("ta")
    assert torch.equal(tv.importance("ta")["a"], imp["ta"]["a"])
    # drop moves the importance rows with the vectors
    tv.drop("ta")
    assert tv.languages() == ["hi", "bn", "mr"] and tv.stats()["importance_languages"] == ["bn", "mr"]
    assert torch.equal(tv.importance("bn")["w"], imp["bn"]["w"]) and torch.equal(tv.importance("mr")["w"], imp["mr"]["w"])
    assert not tv.importances[0].any() and not tv.importances[3].any()
    tv.drop("hi")
    assert torch.equal(tv.importances[0, :n][inside], imp["bn"].flat[inside]) and not tv.importances[2:].any()
    # refusals change nothing
    with pytest.raises(ValueError, match="unknown language 'xx'"):
        tv.set_importance("xx", imp["hi"])
    with pytest.raises(ValueError, match="must be a FlatDict of this layout"):
        tv.set_importance("bn", {"w": torch.zeros(5, 13)})
    from indic_cl_asr_amd import cl
    with pytest.raises(ValueError, match="must be a FlatDict of this layout"):
        tv.set_importance("bn", cl.FlatParams(torch.nn.Linear(3, 2)).zeros())
    with pytest.raises(ValueError, match="must be a FlatDict of this layout"):
        tv.store("zz", importance=torch.zeros(n))
    assert tv.languages() == ["bn", "mr"]
    # a new base drops them with the vectors
    tv.set_base()
    assert tv.stats()["importance_languages"] == [] and not tv.importances.any()
    tv.store("hi")
    with pytest.raises(ValueError, match="no importance is stored for 'hi'"):
        tv.importance("hi")


def test_importances_grow_with_the_vectors():
    flat, tv = _tv()
    tv.set_base()
    kept = {}
    for k in range(5):
        kept[f"l{k}"] = _importance(flat, 20 + k)
        tv.store(f"l{k}", importance=kept[f"l{k}"] if k != 2 else None)
        assert tv.importances.shape == tv.vectors.shape
    assert tv.vectors.shape[0] == 8 and tv.stats()["importance_languages"] == ["l0", "l1", "l3", "l4"]
    for lang in ("l0", "l1", "l3", "l4"):
        assert torch.equal(tv.importance(lang)["w"], kept[lang]["w"])
    assert not tv.importances[2].any() and not tv.importances[5:].any()


def test_state_dict_with_and_without_importances(tmp_path):
    from indic_cl_asr_amd import checkpoint
    flat, tv = _stored()
    plain = tv.state_dict()
    assert set(plain) == {"entries", "max_tasks", "base", "base_buffers", "task_languages", "vectors", "buffers"}
    imp = {lang: _importance(flat, 30 + k) for k, lang in enumerate(("hi", "bn"))}
    tv.set_importance("bn", imp["bn"])
    tv.set_importance("hi", imp["hi"])
    sd = tv.state_dict()
    assert set(sd) == set(plain) | {"importances", "importance_languages"}
    assert sd["importance_languages"] == ["hi", "bn"] and sd["importances"].shape == (2, flat.numel)       # row order
    assert torch.equal(sd["importances"][1], imp["bn"].flat) and not sd["importances"].is_cuda
    path = str(tmp_path / "vectors.pt")
    checkpoint.save_masks(tv, path)
    flat2, tv2 = _tv(max_tasks=4)
    assert checkpoint.load_masks(tv2, path) is tv2
    assert tv2.languages() == ["hi", "ta", "bn"] and tv2.stats()["importance_languages"] == ["hi", "bn"]
    assert torch.equal(tv2.importances[:3], tv.importances[:3]) and torch.equal(tv2.vectors[:3], tv.vectors[:3])
    assert torch.equal(tv2.importance("bn")["w"], imp["bn"]["w"]) and not tv2.importances[1].any()
    with pytest.raises(ValueError, match="no importance is stored for 'ta'"):
        tv2.importance("ta")
    # a state without the keys clears the importances of the loader
    tv2.load_state_dict(plain)
    assert tv2.stats()["importance_languages"] == [] and not tv2.importances.any() and tv2.languages() == ["hi", "ta", "bn"]
    # importances that do not belong to the saved vectors
    broken = dict(sd, importance_languages=["hi", "mr"])
    with pytest.raises(ValueError, match="importances do not match"):
        tv2.load_state_dict(broken, source="x")
    broken = dict(sd, importances=sd["importances"][:1])
    with pytest.raises(ValueError, match="importances do not match"):
        tv2.load_state_dict(broken, source="x")


def test_new_merge_argument_checks_launch_nothing():
    flat, tv = _stored()
    for k, lang in enumerate(("hi", "ta")):
        tv.set_importance(lang, _importance(flat, 40 + k))
    before = flat.theta.clone()
    inf, nan = float("inf"), float("nan")
    two = ["hi", "ta"]
    bad = [(dict(method="fisher"), "none is stored for 'bn'"),
           (dict(method="fisher", languages=["bn", "hi"]), "none is stored for 'bn'"),
           (dict(method="fisher", languages=two, weights=[1.0, 0.0]), "weights of 'fisher' must be > 0"),
           (dict(method="fisher", languages=two, weights=[1.0, -2.0]), "weights of 'fisher' must be > 0"),
           (dict(method="fisher", languages=two, weights=[1.0, inf]), "weights must be finite"),
           (dict(method="fisher", languages=two, weights=[1.0]), "1 weights for 2 languages"),
           (dict(method="fisher", languages=two, fisher_floor=-1e-9), "fisher_floor must be finite and >= 0"),
           (dict(method="fisher", languages=two, fisher_floor=inf), "fisher_floor must be finite and >= 0"),
           (dict(method="fisher", languages=two, fisher_floor=nan), "fisher_floor must be finite and >= 0"),
           (dict(method="fisher", languages=two, scale=nan), "scale must be finite"),
           (dict(method="fisher", languages=["hi", "mr"]), "unknown language 'mr'"),
           (dict(method="dare_linear", density=0.0), r"outside \(0, 1\]"),
           (dict(method="dare_linear", density=1.5), r"outside \(0, 1\]"),
           (dict(method="dare_ties", density=nan), r"outside \(0, 1\]"),
           (dict(method="dare_ties", density=1e-12), "too small"),
           (dict(method="dare_linear", seed=-1), r"seed must be an int in \[0, 2\^32\)"),
           (dict(method="dare_linear", seed=2 ** 32), r"seed must be an int in \[0, 2\^32\)"),
           (dict(method="dare_ties", seed=1.5), r"seed must be an int in \[0, 2\^32\)"),
           (dict(method="dare_ties", seed=True), r"seed must be an int in \[0, 2\^32\)"),
           (dict(method="dare_ties", weights=[1.0, 1.0, 1.0]), "weights belong to 'task_arithmetic'"),
           (dict(method="dare_linear", weights=[1.0, nan, 1.0]), "weights must be finite"),
           (dict(method="dare_linear", scale=inf), "scale must be finite"),
           (dict(method="dare_ties", languages=["hi", "hi"]), "listed twice"),
           (dict(method="dare"), "unknown method 'dare'")]
    for kw, message in bad:
        with pytest.raises(ValueError, match=message):
            tv.merge(**kw)
    # valid arguments reach the kernels, and there is no eager fallback on a host model
    for kw in (dict(method="fisher", languages=two), dict(method="fisher", languages=two, weights={"hi": 2.0, "ta": 0.5}, fisher_floor=0),
               dict(method="dare_linear", density=0.5, seed=M32, weights=[1.0, -1.0, 0.0]), dict(method="dare_ties", density=1.0, rescale=False)):
        with pytest.raises(RuntimeError, match="runs on the HIP kernels"):
            tv.merge(**kw)
    assert torch.equal(flat.theta, before) and tv.last_merge is None
    # the tuple of _checked_merge keeps its shape for the new methods
    assert tv._checked_merge("fisher", two, 0.5, None, 0.2, "tensor") == (two, [1.0, 1.0], 0.5, None)
    assert tv._checked_merge("dare_linear", None, 1.0, [1.0, 2.0, 3.0], 0.2, "tensor") == (["hi", "ta", "bn"], [1.0, 2.0, 3.0], 1.0, None)
    assert tv._checked_merge("dare_ties", two, 1.0, None, 1e-12, "model")[3] is None
    rule = tv._checked_rule("dare_ties", two, [1.0, 1.0], 0.25, 1e-6, 7, False)
    assert rule == {"keep_threshold": 1 << 30, "keep_prob": 1.0, "seed": 7, "density": 0.25, "rescale": False}
    assert tv._checked_rule("fisher", two, [1.0, 1.0], 0.2, 0, 0, True) == {"fisher_floor": 0.0}
    assert tv._checked_rule("ties", two, [1.0, 1.0], 0.2, -1.0, -1, True) == {}


# ------------------------------------------------------------------------------------------ argument checks of the C entries
def test_new_c_entries_refuse_bad_arguments_before_any_device_work():
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    buf, p = _host_args()
    coef = (ctypes.c_float * 32)(*([1.0] * 32))
    inf, nan = float("inf"), float("nan")
    # ia_merge_fisher(theta, base, vectors, importances, stride, ntasks, coef, floor, scale, chunk_table, nchunks, nseg, shadow,
    #                 seg_counts, stream)
    good = [p(0), p(256), p(512), p(1536), 64, 2, coef, 1e-6, 1.0, p(1024), 1, 1, None, p(2560), None]
    for at, value in ((0, None), (1, None), (2, None), (3, None), (6, None), (9, None), (13, None), (5, 0), (5, 33), (5, -1),
                      (7, -1e-9), (7, inf), (7, -inf), (7, nan), (8, inf), (8, nan), (10, 0), (11, 0), (4, 0), (4, 6), (4, -4),
                      (0, p(4)), (1, p(8)), (2, p(4)), (3, p(4)), (3, p(8)), (9, p(4)), (12, p(4)), (13, p(2))):
        args = list(good)
        args[at] = value
        assert L.ia_merge_fisher(*args) == -1, (at, value)
    # ia_merge_linear_dare(theta, base, vectors, stride, ntasks, coef, scale, chunk_table, nchunks, shadow, seed, threshold,
    #                      keep_prob, stream)
    good = [p(0), p(256), p(512), 64, 2, coef, 1.0, p(1024), 1, None, 0, 1 << 31, 0.5, None]
    for at, value in ((0, None), (1, None), (2, None), (5, None), (7, None), (4, 0), (4, 33), (6, inf), (6, nan), (8, 0), (3, 0),
                      (3, 6), (0, p(4)), (1, p(8)), (2, p(4)), (7, p(4)), (9, p(2)), (12, 0.0), (12, -0.5), (12, 1.5), (12, nan),
                      (12, inf)):
        args = list(good)
        args[at] = value
        assert L.ia_merge_linear_dare(*args) == -1, (at, value)
    # ia_merge_ties_dare(theta, base, vectors, stride, ntasks, scale, chunk_table, nchunks, nseg, shadow, seg_counts, seed,
    #                    threshold, keep_prob, stream)
    good = [p(0), p(256), p(512), 64, 2, 1.0, p(1024), 1, 1, None, p(2560), 0, 1 << 31, 0.5, None]
    for at, value in ((0, None), (1, None), (2, None), (6, None), (10, None), (4, 0), (4, 33), (5, inf), (5, nan), (7, 0), (8, 0),
                      (3, -4), (3, 5), (0, p(8)), (1, p(4)), (2, p(8)), (6, p(4)), (9, p(4)), (10, p(2)), (13, 0.0), (13, 1.0001),
                      (13, nan)):
        args = list(good)
        args[at] = value
        assert L.ia_merge_ties_dare(*args) == -1, (at, value)
    assert not any(buf)
