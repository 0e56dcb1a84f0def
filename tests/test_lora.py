"""cl.LoRA on the CPU (host logic only: no kernel is launched; ia_lora_grad, the factor update and ia_lora_apply run in
tests/test_lora_gpu.py): default kinds and their overrides, the rank and size refusals, the factor layout, what FusedAdamW
refuses, the state dict, layout refusal, export shapes, argument checks of the C entries."""
import pytest
import torch


def _model(freeze_till=0):
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny'))
    freeze_layer(m, freeze_till)
    return cl.FlatParams(m)


def _lora(freeze_till=0, **kw):
    from indic_cl_asr_amd import cl
    flat = _model(freeze_till)
    return flat, cl.LoRA(flat, **kw)


def _view(shape, numel):
    return shape[0], numel // shape[0]


def _fill(lora):
    """What training and save_language() leave behind, written by hand: the kernels need the device."""
    g = torch.Generator().manual_seed(5)
    flat = lora.flat
    lora.base.flat.copy_(torch.randn(flat.numel, generator=g))
    for buf in (lora.factors, lora.factor_exp_avg, lora.factor_exp_avg_sq):
        buf.copy_(torch.randn(lora.factor_numel, generator=g))
    lora.factor_step.copy_(torch.arange(lora.factor_step.numel(), dtype=torch.int32))
    free = [n for n, k in lora.kinds().items() if k == "free"]
    for lang in ("hi", "ta"):
        lora.records[lang] = {
            "factors": torch.randn(lora.factor_numel, generator=g),
            "free": {n: torch.randn(flat.params[flat.names.index(n)].shape, generator=g) for n in free},
            "buffers": {n: torch.randn(b.shape, generator=g).to(b.dtype) for n, b in flat.model.named_buffers()}}
    lora.current = lora._factors_lang = "ta"


def test_default_kinds_and_factor_layout():
    flat, lora = _lora(rank=4, alpha=8.0)
    kinds = lora.kinds()
    assert list(kinds) == flat.names and set(kinds.values()) == {"free", "adapted", "frozen"}
    pb_kinds = __import__("indic_cl_asr_amd.cl", fromlist=["cl"]).Piggyback(flat).kinds()
    small = []
    for (n, off, numel, shape), p in zip(flat.entries, flat.params):
        m, k = _view(shape, numel)
        if pb_kinds[n] == "free":
            assert kinds[n] == "free", n                         # the heads: Piggyback's default
        elif p.dim() >= 2 and min(m, k) >= 8:
            assert kinds[n] == "adapted", n
        else:
            assert kinds[n] == "frozen", n
            small += [n] if p.dim() >= 2 else []
    assert any(n.endswith("pos_bias_u") for n in small)          # [4, 8] is too small for rank 4: frozen, not free
    at16 = __import__("indic_cl_asr_amd.cl", fromlist=["cl"]).LoRA(flat, rank=16).kinds()
    dw = next(n for n in flat.names if ".depthwise_conv.weight" in n)
    assert kinds[dw] == "adapted" and at16[dw] == "frozen"       # [d, 1, 31] is viewed as [d, 31]: too small from rank 16 on
    assert lora.seg_kind.tolist() == [("free", "adapted", "frozen").index(kinds[n]) for n in flat.names]
    assert lora.step_kind.tolist() == [0 if kinds[n] == "free" else 2 for n in flat.names]
    assert (lora.rank, lora.alpha, lora.scale, lora.current, lora.languages()) == (4, 8.0, 2.0, None, [])
    assert torch.equal(lora.base.flat, flat.theta) and lora.base.flat.data_ptr() != flat.theta.data_ptr()
    # the factor buffer: per adapted tensor B [m, r] then A [r, n], each on a 64-float boundary, in the order of the flat layout
    expect = 0
    assert [a[0] for a in lora.adapted] == [n for n in flat.names if kinds[n] == "adapted"]
    for name, k, m, n, b_off, a_off in lora.adapted:
        assert (m, n) == _view(flat.entries[k][3], flat.entries[k][2]) and flat.names[k] == name
        assert b_off == expect and b_off % 64 == 0 and a_off % 64 == 0 and a_off >= b_off + m * 4
        expect = a_off + (4 * n + 63) // 64 * 64
    assert lora.factor_numel == expect
    for buf in (lora.factors, lora.factor_grad, lora.factor_exp_avg, lora.factor_exp_avg_sq):
        assert buf.shape == (expect,) and buf.dtype == torch.float32 and not buf.any()
    # its chunk table: chunks never straddle factors, cover every factor element once and nothing else
    covered = torch.zeros(expect, dtype=torch.int32)
    for off, cnt, fac, t in lora.factor_table.tolist():
        assert 0 < cnt <= 4096 and off % 4 == 0 and fac // 2 == t
        name, k, m, n, b_off, a_off = lora.adapted[t]
        start, size = (a_off, 4 * n) if fac & 1 else (b_off, m * 4)
        assert start <= off and off + cnt <= start + size
        covered[off:off + cnt] += 1
    assert int(covered.sum()) == sum(4 * (m + n) for _, _, m, n, _, _ in lora.adapted) and int(covered.max()) == 1
    assert lora.seg_tensor.tolist() == [[a[1] for a in lora.adapted].index(k) if kinds[n] == "adapted" else -1
                                        for k, n in enumerate(flat.names)]
    size = lora.bytes_per_language()
    assert size["factors"] == 4 * 4 * sum(m + n for _, _, m, n, _, _ in lora.adapted) <= size["factors_padded"] == 4 * expect
    assert size["total"] == size["factors_padded"] + size["free"] + size["buffers"]
    assert size["free"] == 4 * sum(p.numel() for n, p in zip(flat.names, flat.params) if kinds[n] == "free")
    full = 4 * sum(m * n for _, _, m, n, _, _ in lora.adapted)
    assert size["factors"] < full


def test_tiles_cover_every_adapted_tensor_once_and_the_workspace_is_disjoint():
    from indic_cl_asr_amd import _lib
    flat, lora = _lora(rank=4)
    L = _lib.lib()
    R, C = L.ia_lora_tile_rows(), L.ia_lora_tile_cols()
    seen = set()
    for t, rt, ct, _ in lora.tile_table.tolist():
        name, k, m, n, b_off, a_off = lora.adapted[t]
        assert 0 <= rt * R < m and 0 <= ct * C < n and (t, rt, ct) not in seen
        seen.add((t, rt, ct))
    assert len(seen) == sum(((m + R - 1) // R) * ((n + C - 1) // C) for _, _, m, n, _, _ in lora.adapted)
    end = 0
    for row, (name, k, m, n, b_off, a_off) in zip(lora.tensor_table.tolist(), lora.adapted):
        g_off, dm, dn, db, da, ws_b, ws_a, seg = row
        assert (g_off, dm, dn, db, da, seg) == (flat.entries[k][1], m, n, b_off, a_off, k)
        assert ws_b == end and ws_a == ws_b + ((n + C - 1) // C) * m * 4
        end = ws_b + L.ia_lora_workspace_bytes(m, n, 4) // 4
        assert ws_a + ((m + R - 1) // R) * 4 * n <= end
    assert lora.workspace_bytes == 4 * end


def test_overrides_and_refusals():
    from indic_cl_asr_amd import cl
    flat = _model()
    weight = "encoder.layers.1.feed_forward1.linear1.weight"
    bias = "encoder.layers.1.feed_forward1.linear1.bias"
    default = cl.LoRA(flat, rank=4).kinds()
    assert default[weight] == "adapted" and default[bias] == "frozen"
    by_list = cl.LoRA(flat, rank=4, adapted=[weight]).kinds()
    others = [n for n in flat.names if n != weight]
    assert by_list[weight] == "adapted" and all(by_list[n] != "adapted" for n in others)     # adapted= replaces the default set
    assert all(by_list[n] == default[n] for n in others if default[n] == "free")
    by_re = cl.LoRA(flat, rank=4, frozen=r"feed_forward1\.linear1\.").kinds()
    assert by_re[weight] == by_re[bias] == "frozen"
    assert by_re["encoder.layers.1.feed_forward1.linear2.weight"] == "adapted"
    assert by_re["encoder.layers.1.feed_forward1.linear2.bias"] == "free"                   # frozen= replaces the default set too
    with pytest.raises(ValueError, match="claimed by adapted= and by frozen="):
        cl.LoRA(flat, rank=4, adapted=[weight], frozen=r"linear1")
    with pytest.raises(ValueError, match="not a trainable tensor"):
        cl.LoRA(flat, adapted=["no.such.tensor"])
    for rank in (0, 65, -1):
        with pytest.raises(ValueError, match=f"rank {rank} is outside 1..64"):
            cl.LoRA(flat, rank=rank)
    m, n = _view(flat.entries[flat.names.index(weight)][3], flat.entries[flat.names.index(weight)][2])
    exact = cl.LoRA(flat, rank=min(m, n, 64), adapted=[weight])                            # min(m, n) == rank is allowed when asked for
    assert exact.kinds()[weight] == "adapted"
    dw = next(n for n in flat.names if ".depthwise_conv.weight" in n)                     # [d, 1, k]: n = k
    k = flat.entries[flat.names.index(dw)][2] // flat.entries[flat.names.index(dw)][3][0]
    with pytest.raises(ValueError, match=dw.replace(".", r"\.") + ".*too small for rank"):
        cl.LoRA(flat, rank=k + 1, adapted=[dw])
    with pytest.raises(ValueError, match="too small for rank"):
        cl.LoRA(flat, rank=4, adapted=[bias])                                               # a vector is [m, 1]
    # a rank the default set cannot serve at all
    if all(min(_view(e[3], e[2])) < 128 for e in flat.entries):
        with pytest.raises(ValueError, match="no trainable tensor is adapted"):
            cl.LoRA(flat, rank=64)


def test_seeds_depend_on_seed_language_and_tensor():
    flat, lora = _lora(rank=4, seed=3)
    other = __import__("indic_cl_asr_amd.cl", fromlist=["cl"]).LoRA(flat, rank=4, seed=4)
    seeds = {lora._seed_of("hi", 0), lora._seed_of("hi", 1), lora._seed_of("ta", 0), other._seed_of("hi", 0)}
    assert len(seeds) == 4 and all(0 <= s < 2 ** 63 for s in seeds)
    assert lora._seed_of("hi", 7) == lora._seed_of("hi", 7)


def test_fused_adamw_refusals_and_unchanged_state_keys():
    from indic_cl_asr_amd import cl
    flat, lora = _lora(rank=4)
    plain = cl.FusedAdamW(flat, lr=3e-4)
    opt = cl.FusedAdamW(flat, lr=3e-4, masks=lora)
    assert opt.masks is lora and lora._optimizer() is opt
    assert set(opt.state_dict()) == set(plain.state_dict())
    assert set(opt.param_groups[0]) == set(plain.param_groups[0])
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=lora, path_integral=cl.SynapticIntelligence(flat))
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=lora, projection=cl.AveragedGEM(flat))
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=lora, projection=cl.GEM(flat, max_tasks=2))
    with pytest.raises(ValueError, match="another FlatParams"):
        cl.FusedAdamW(_model(), masks=lora)
    with pytest.raises(ValueError, match="another FlatParams"):
        lora.begin_language("hi", cl.FusedAdamW(_model()))


def test_state_dict_round_trips_through_torch_save_in_place(tmp_path):
    from indic_cl_asr_amd import checkpoint
    flat, lora = _lora(rank=4, alpha=6.0, seed=9, frozen=r"\.bias$")
    _fill(lora)
    sd = lora.state_dict()
    assert set(sd) == {"entries", "kinds", "rank", "alpha", "seed", "base", "factors", "factor_exp_avg", "factor_exp_avg_sq",
                       "factor_step", "current", "factors_language", "languages"}
    assert sd["entries"] == list(flat.entries) and sd["kinds"] == list(lora.kinds().values())
    assert set(sd["languages"]) == {"hi", "ta"} and all(not sd[k].is_cuda for k in ("base", "factors", "factor_step"))
    path = str(tmp_path / "masks.pt")
    checkpoint.save_masks(lora, path)
    flat2, lora2 = _lora(rank=4, frozen=r"\.bias$")
    theta = flat2.theta.clone()
    held = lambda x: [t.data_ptr() for t in (x.base.flat, x.factors, x.factor_exp_avg, x.factor_exp_avg_sq, x.factor_step,
                                             x.seg_kind, x.tensor_table)]
    ptrs = held(lora2)
    assert checkpoint.load_masks(lora2, path) is lora2
    assert ptrs == held(lora2)                                   # an optimizer and the tables hold them
    for key in ("factors", "factor_exp_avg", "factor_exp_avg_sq", "factor_step"):
        assert torch.equal(getattr(lora2, key), getattr(lora, key)), key
    assert torch.equal(lora2.base.flat, lora.base.flat) and lora2.kinds() == lora.kinds()
    assert (lora2.alpha, lora2.scale, lora2.seed, lora2.current, lora2.languages()) == (6.0, 1.5, 9, "ta", ["hi", "ta"])
    for lang in ("hi", "ta"):
        a, b = lora.records[lang], lora2.records[lang]
        assert torch.equal(a["factors"], b["factors"])
        for part in ("free", "buffers"):
            assert set(a[part]) == set(b[part]) and all(torch.equal(a[part][n], b[part][n]) for n in a[part])
    assert torch.equal(flat2.theta, theta)                       # the weights are not LoRA state
    sd["factors"].zero_()                                        # the saved tensors are copies, not views
    assert lora.factors.abs().sum() > 0


def test_other_layouts_are_refused(tmp_path):
    from indic_cl_asr_amd import checkpoint, cl
    flat, lora = _lora(rank=4)
    _fill(lora)
    _, other = _lora(freeze_till=1, rank=4)
    with pytest.raises(ValueError, match="'masks' was saved for a different set of trainable tensors"):
        other.load_state_dict(lora.state_dict())
    path = str(tmp_path / "masks.pt")
    checkpoint.save_masks(lora, path)
    with pytest.raises(ValueError, match="was saved for a different set of trainable tensors"):
        checkpoint.load_masks(other, path)
    with pytest.raises(ValueError, match="another factor layout"):
        checkpoint.load_masks(cl.LoRA(flat, rank=5), path)                                   # another rank
    with pytest.raises(ValueError, match="another factor layout"):
        checkpoint.load_masks(cl.LoRA(flat, rank=4, frozen=r"linear1\.weight$"), path)       # other kinds
    pb = cl.Piggyback(flat)
    with pytest.raises(ValueError, match="does not hold LoRA factors"):
        lora.load_state_dict(pb.state_dict())


def test_export_shapes_and_unknown_languages():
    flat, lora = _lora(rank=4, alpha=8.0)
    _fill(lora)
    out = lora.export("hi")
    assert out["r"] == 4 and out["alpha"] == 8.0
    names = [a[0] for a in lora.adapted]
    assert set(out) == set(names) | {"r", "alpha"}
    views = lora.factor_views(lora.records["hi"]["factors"])
    for name, k, m, n, b_off, a_off in lora.adapted:
        assert out[name]["lora_A"].shape == (4, n) and out[name]["lora_B"].shape == (m, 4)
        assert torch.equal(out[name]["lora_A"], views[name]["lora_A"]) and torch.equal(out[name]["lora_B"], views[name]["lora_B"])
        assert out[name]["lora_A"].data_ptr() != views[name]["lora_A"].data_ptr()           # copies
        assert m * n == flat.entries[k][2]
    live = lora.export()
    assert torch.equal(live[names[0]]["lora_B"], lora.factor_views()[names[0]]["lora_B"])
    for call in (lora.activate, lora.export, lora.delta):
        with pytest.raises(ValueError, match="unknown language 'bn'"):
            call("bn")
    _, fresh = _lora(rank=4)
    with pytest.raises(ValueError, match="no language is current"):
        fresh.save_language()


def test_entry_points_refuse_bad_arguments_and_workspace_bytes_is_monotone():
    """Argument checks come before any device work: -1 (IA_INVALID_VALUE) with no GPU in the machine."""
    from indic_cl_asr_amd import _lib
    L, ptr = _lib.lib(), _lib.ptr
    assert L.ia_lora_grad(None, None, None, None, 1, None, 1, None, 1, 8, 2.0, 1.0, None, 0, 0, None, None, 0, 0, None) == -1
    assert L.ia_lora_apply(None, None, None, None, 1, None, None, 1, 1, 8, 2.0, None, None, 0, None) == -1
    assert L.ia_adamw_step_segmented_kinds(None, None, None, None, None, 1, None, None, 1, 0, 0.9, 0.999, 1e-8, 1.0, None, None,
                                           1, None, None, None, 0, None, None, 0, None) == -1
    host = torch.zeros(64)                                       # never dereferenced: counts, rank and alignment are checked first
    table = torch.zeros(4, dtype=torch.int32)
    desc = torch.zeros(8, dtype=torch.int64)
    flags = torch.zeros(2, dtype=torch.int32)
    grad = lambda rank, nt=1, tiles=1, chunks=1, g=host: L.ia_lora_grad(
        ptr(g), ptr(host), ptr(host), ptr(desc), nt, ptr(table), tiles, ptr(table), chunks, rank, 2.0, 1.0, None, 0, 0, ptr(flags),
        ptr(host), 256, 256, None)
    apply_ = lambda rank, nt=1, chunks=1, nseg=1, p=host: L.ia_lora_apply(
        ptr(p), ptr(host), ptr(host), ptr(desc), nt, ptr(flags), ptr(table), chunks, nseg, rank, 2.0, None, None, 0, None)
    for rank in (0, 65, -3):
        assert grad(rank) == -1 and apply_(rank) == -1
    assert grad(8, nt=0) == -1 and grad(8, tiles=0) == -1 and grad(8, chunks=0) == -1
    assert apply_(8, nt=0) == -1 and apply_(8, chunks=0) == -1 and apply_(8, nseg=0) == -1
    assert grad(8, g=host[1:]) == -1 and apply_(8, p=host[1:]) == -1                        # 4-byte aligned only
    assert L.ia_lora_grad(ptr(host), ptr(host), ptr(host), ptr(desc), 1, ptr(table), 1, ptr(table), 1, 8, 2.0, 1.0, None, 0, 0,
                          ptr(flags), ptr(host), 128, 256, None) == -2                       # IA_WORKSPACE_TOO_SMALL
    R, C = L.ia_lora_tile_rows(), L.ia_lora_tile_cols()
    assert R > 0 and C > 0
    ws = L.ia_lora_workspace_bytes
    assert ws(0, 8, 4) == ws(8, 0, 4) == ws(8, 8, 0) == ws(8, 8, 65) == 0
    last = 0
    for m, n, r in ((1, 1, 1), (8, 8, 1), (65, 63, 5), (65, 63, 8), (130, 257, 8), (130, 257, 64), (1030, 257, 64), (1030, 4096, 64)):
        now = ws(m, n, r)
        assert now > 0 and now % 256 == 0 and now >= last
        assert now >= 4 * r * (((n + C - 1) // C) * m + ((m + R - 1) // R) * n)
        last = now
