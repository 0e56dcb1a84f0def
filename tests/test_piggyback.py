"""cl.Piggyback on the CPU (host logic only: no kernel is launched; the masked step, pack and apply run in
tests/test_piggyback_gpu.py): default kinds and their overrides, the state dict, layout refusal, what FusedAdamW refuses,
argument checks of the three C entries."""
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


def _pb(freeze_till=0, **kw):
    from indic_cl_asr_amd import cl
    flat = _model(freeze_till)
    return flat, cl.Piggyback(flat, **kw)


def _fill(pb):
    """What save_language() records, written by hand: the pack kernel needs the device."""
    g = torch.Generator().manual_seed(5)
    flat = pb.flat
    pb.scores.flat.copy_(torch.rand(flat.numel, generator=g) * 1e-2)
    pb.base.flat.copy_(torch.randn(flat.numel, generator=g))
    free = [n for n, k in pb.kinds().items() if k == "free"]
    for lang in ("hi", "ta"):
        pb.records[lang] = {
            "bits": torch.randint(-2 ** 62, 2 ** 62, (flat.numel // 64,), generator=g, dtype=torch.int64),
            "free": {n: torch.randn(flat.params[flat.names.index(n)].shape, generator=g) for n in free},
            "buffers": {n: torch.randn(b.shape, generator=g).to(b.dtype) for n, b in flat.model.named_buffers()}}
    pb.current = "ta"


def test_default_kinds():
    flat, pb = _pb()
    kinds = pb.kinds()
    assert list(kinds) == flat.names and set(kinds.values()) == {"free", "masked", "frozen"}
    heads = [n for n in flat.names if ".hi." in n or ".ta." in n]
    assert len(heads) == 4 and all(n.startswith("joint.joint_net.") for n in heads)
    for n, p in zip(flat.names, flat.params):
        if n in heads or n in ("ctc_decoder.decoder_layers.0.weight", "ctc_decoder.decoder_layers.0.bias"):
            assert kinds[n] == "free", n
        elif p.dim() >= 2:
            assert kinds[n] == "masked", n
        else:
            assert kinds[n] == "frozen", n
    assert pb.threshold == 5e-3 and pb.init == 1e-2 and pb.current is None and pb.languages() == []
    assert torch.equal(pb.base.flat, flat.theta) and pb.base.flat.data_ptr() != flat.theta.data_ptr()
    for n, view in pb.scores.items():
        assert bool((view == (1e-2 if kinds[n] == "masked" else 0.0)).all()), n
    gaps = torch.ones(flat.numel, dtype=torch.bool)
    for _, off, k, _ in flat.entries:
        gaps[off:off + k] = False
    assert not pb.scores.flat[gaps].any()
    assert pb.seg_kind.tolist() == [("free", "masked", "frozen").index(kinds[n]) for n in flat.names]
    size = pb.bytes_per_language()
    assert size["mask"] == flat.numel // 8 and size["total"] == size["mask"] + size["free"] + size["buffers"]
    assert size["free"] == 4 * sum(p.numel() for n, p in zip(flat.names, flat.params) if kinds[n] == "free")


def test_overrides_by_list_and_by_regular_expression():
    from indic_cl_asr_amd import cl
    flat = _model()
    bias = "encoder.layers.1.feed_forward1.linear1.bias"
    weight = "encoder.layers.1.feed_forward1.linear1.weight"
    default = cl.Piggyback(flat).kinds()
    assert default[bias] == "frozen" and default[weight] == "masked"
    by_list = cl.Piggyback(flat, masked=[weight, bias]).kinds()
    assert by_list[weight] == by_list[bias] == "masked"
    others = [n for n in flat.names if n not in (weight, bias)]
    assert all(by_list[n] != "masked" for n in others)                  # masked= replaces the default set
    assert all(by_list[n] == default[n] for n in others if default[n] != "masked")
    assert all(by_list[n] == "free" for n in others if default[n] == "masked")
    by_re = cl.Piggyback(flat, frozen=r"feed_forward1\.linear1\.").kinds()
    assert by_re[weight] == by_re[bias] == "frozen"                      # an explicit claim wins over the other default set
    assert by_re["encoder.layers.1.feed_forward1.linear2.weight"] == "masked"
    assert by_re["encoder.layers.1.feed_forward1.linear2.bias"] == "free"    # frozen= replaces the default set too
    both = cl.Piggyback(flat, masked=r"\.weight$", frozen=r"\.bias$").kinds()
    assert all(k == ("masked" if n.endswith(".weight") else "frozen" if n.endswith(".bias") else "free")
               for n, k in both.items())
    with pytest.raises(ValueError, match="claimed by masked= and by frozen="):
        cl.Piggyback(flat, masked=[weight], frozen=r"linear1")
    with pytest.raises(ValueError, match="not a trainable tensor"):
        cl.Piggyback(flat, masked=["no.such.tensor"])
    with pytest.raises(ValueError, match="matches no trainable tensor"):
        cl.Piggyback(flat, frozen=r"no_such_tensor")
    with pytest.raises(ValueError, match="init"):
        cl.Piggyback(flat, threshold=5e-3, init=1e-3)


def test_state_dict_round_trips_through_torch_save_in_place(tmp_path):
    from indic_cl_asr_amd import checkpoint
    flat, pb = _pb(threshold=2e-3, init=4e-3, frozen=r"\.bias$")
    _fill(pb)
    sd = pb.state_dict()
    assert set(sd) == {"entries", "kinds", "threshold", "init", "base", "scores", "current", "scores_language", "languages"}
    assert sd["entries"] == list(flat.entries) and sd["kinds"] == list(pb.kinds().values())
    assert set(sd["languages"]) == {"hi", "ta"}
    assert all(not t.is_cuda for t in (sd["base"], sd["scores"]))
    path = str(tmp_path / "masks.pt")
    checkpoint.save_masks(pb, path)
    flat2, pb2 = _pb()
    theta = flat2.theta.clone()
    ptrs = [t.data_ptr() for t in (pb2.base.flat, pb2.scores.flat, pb2.seg_kind)]
    assert checkpoint.load_masks(pb2, path) is pb2
    assert ptrs == [t.data_ptr() for t in (pb2.base.flat, pb2.scores.flat, pb2.seg_kind)]     # an optimizer holds them
    assert torch.equal(pb2.base.flat, pb.base.flat) and torch.equal(pb2.scores.flat, pb.scores.flat)
    assert torch.equal(pb2.seg_kind, pb.seg_kind) and pb2.kinds() == pb.kinds()
    assert (pb2.threshold, pb2.init, pb2.current, pb2.languages()) == (2e-3, 4e-3, "ta", ["hi", "ta"])
    for lang in ("hi", "ta"):
        a, b = pb.records[lang], pb2.records[lang]
        assert torch.equal(a["bits"], b["bits"]) and b["bits"].dtype == torch.int64
        for part in ("free", "buffers"):
            assert set(a[part]) == set(b[part]) and all(torch.equal(a[part][n], b[part][n]) for n in a[part])
    assert torch.equal(flat2.theta, theta)                       # the weights are not mask state
    sd["base"].zero_()                                           # the saved tensors are copies, not views
    assert pb.base.flat.abs().sum() > 0


def test_other_trainable_set_is_refused(tmp_path):
    from indic_cl_asr_amd import checkpoint
    _, pb = _pb(freeze_till=0)
    _fill(pb)
    _, other = _pb(freeze_till=1)
    with pytest.raises(ValueError, match="'masks' was saved for a different set of trainable tensors"):
        other.load_state_dict(pb.state_dict())
    path = str(tmp_path / "masks.pt")
    checkpoint.save_masks(pb, path)
    with pytest.raises(ValueError, match="was saved for a different set of trainable tensors"):
        checkpoint.load_masks(other, path)


def test_fused_adamw_refusals_and_unchanged_state_keys():
    from indic_cl_asr_amd import cl
    flat, pb = _pb()
    plain = cl.FusedAdamW(flat, lr=3e-4)
    assert plain.masks is None
    opt = cl.FusedAdamW(flat, lr=3e-4, masks=pb)
    assert opt.masks is pb
    assert set(opt.state_dict()) == set(plain.state_dict())
    assert set(opt.param_groups[0]) == set(plain.param_groups[0])
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=pb, path_integral=cl.SynapticIntelligence(flat))
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=pb, projection=cl.AveragedGEM(flat))
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=pb, projection=cl.GEM(flat, max_tasks=2))
    other = _model()
    with pytest.raises(ValueError, match="another FlatParams"):
        cl.FusedAdamW(other, masks=pb)


def test_unknown_language_raises():
    _, pb = _pb()
    with pytest.raises(ValueError, match="unknown language 'hi'"):
        pb.activate("hi")
    _fill(pb)
    with pytest.raises(ValueError, match="unknown language 'bn'"):
        pb.activate("bn")
    _, fresh = _pb()
    with pytest.raises(ValueError, match="no language is current"):
        fresh.save_language()


def test_entry_points_refuse_null_pointers():
    """Argument checks come before any device work: -1 (IA_INVALID_VALUE) with no GPU in the machine."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    assert L.ia_adamw_step_segmented_masked(None, None, None, None, None, 1, None, None, 1, 0, 0.9, 0.999, 1e-8, 1.0, None, None,
                                            1, None, None, None, 0, None, None, None, None, 5e-3, None) == -1
    assert L.ia_mask_pack(None, None, 1, None, 1, 5e-3, None, 1, None, None) == -1
    assert L.ia_mask_apply(None, None, None, 1, None, 1, None, 1, None, None) == -1
    host = torch.zeros(64)                                       # never dereferenced: the counts are checked first
    bits = torch.zeros(1, dtype=torch.int64)
    kind = torch.zeros(1, dtype=torch.int32)
    table = torch.zeros(4, dtype=torch.int32)
    assert L.ia_mask_pack(_lib.ptr(host), _lib.ptr(table), 1, _lib.ptr(kind), 1, 5e-3, _lib.ptr(bits), 0, None, None) == -1
    assert L.ia_mask_apply(_lib.ptr(host), _lib.ptr(host), _lib.ptr(bits), 1, _lib.ptr(table), 0, _lib.ptr(kind), 1, None,
                           None) == -1
