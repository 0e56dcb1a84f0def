"""cl.PackNet on the CPU (host logic only: no kernel is launched; the packed step, the pruning and apply run in
tests/test_packnet_gpu.py): default kinds and their overrides, the state dict, layout refusal, what FusedAdamW refuses, the phase
errors of the per-language loop, argument checks of the C entries."""
import pytest
import torch

from test_piggyback import _model


def _pn(freeze_till=0, **kw):
    from indic_cl_asr_amd import cl
    flat = _model(freeze_till)
    return flat, cl.PackNet(flat, **kw)


def _fill(pn):
    """What two finished languages and an open third leave, written by hand: pruning needs the device."""
    g = torch.Generator().manual_seed(5)
    flat = pn.flat
    pn.owner.copy_(torch.randint(0, 4, (flat.numel,), generator=g, dtype=torch.uint8))
    pn.base.flat.copy_(torch.randn(flat.numel, generator=g))
    free = [n for n, k in pn.kinds().items() if k == "free"]
    for task, lang in enumerate(("hi", "ta"), start=1):
        pn.tasks[lang] = task
        pn.records[lang] = {
            "task": task,
            "free": {n: torch.randn(flat.params[flat.names.index(n)].shape, generator=g) for n in free},
            "buffers": {n: torch.randn(b.shape, generator=g).to(b.dtype) for n, b in flat.model.named_buffers()}}
    pn.tasks["bn"] = 3
    pn.current, pn.phase, pn.train_owner = "bn", "retrain", 3


def test_default_kinds_equal_piggybacks():
    from indic_cl_asr_amd import cl
    flat, pn = _pn()
    kinds = pn.kinds()
    pb = cl.Piggyback(flat).kinds()
    assert list(kinds) == flat.names and set(kinds.values()) == {"free", "packed", "frozen"}
    assert {n: ("masked" if k == "packed" else k) for n, k in kinds.items()} == pb
    assert pn.seg_kind.tolist() == [("free", "packed", "frozen").index(kinds[n]) for n in flat.names]
    assert pn.seg_kind.tolist() == cl.Piggyback(flat).seg_kind.tolist()                  # the same numbering
    assert pn.owner.dtype == torch.uint8 and pn.owner.numel() == flat.numel and not pn.owner.any()
    assert torch.equal(pn.base.flat, flat.theta) and pn.base.flat.data_ptr() != flat.theta.data_ptr()
    assert (pn.prune_fraction, pn.current, pn.phase, pn.train_owner, pn.languages()) == (0.5, None, None, -1, [])
    size = pn.bytes_per_language()
    assert size["free"] == 4 * sum(p.numel() for n, p in zip(flat.names, flat.params) if kinds[n] == "free")
    assert size["total"] == size["free"] + size["buffers"]
    assert size["shared_owner_map"] == flat.numel and size["shared_base"] == 4 * flat.numel


def test_overrides_by_list_and_by_regular_expression():
    from indic_cl_asr_amd import cl
    flat = _model()
    bias = "encoder.layers.1.feed_forward1.linear1.bias"
    weight = "encoder.layers.1.feed_forward1.linear1.weight"
    default = cl.PackNet(flat).kinds()
    assert default[bias] == "frozen" and default[weight] == "packed"
    by_list = cl.PackNet(flat, packed=[weight, bias]).kinds()
    assert by_list[weight] == by_list[bias] == "packed"
    others = [n for n in flat.names if n not in (weight, bias)]
    assert all(by_list[n] != "packed" for n in others)                  # packed= replaces the default set
    assert all(by_list[n] == default[n] for n in others if default[n] != "packed")
    assert all(by_list[n] == "free" for n in others if default[n] == "packed")
    by_re = cl.PackNet(flat, frozen=r"feed_forward1\.linear1\.").kinds()
    assert by_re[weight] == by_re[bias] == "frozen"
    assert by_re["encoder.layers.1.feed_forward1.linear2.weight"] == "packed"
    assert by_re["encoder.layers.1.feed_forward1.linear2.bias"] == "free"
    for kw in (dict(packed=r"\.weight$", frozen=r"\.bias$"), dict(packed=[weight], frozen=[bias]), dict(frozen=r"linear1")):
        as_pb = cl.Piggyback(flat, **{("masked" if k == "packed" else k): v for k, v in kw.items()}).kinds()
        assert {n: ("masked" if k == "packed" else k) for n, k in cl.PackNet(flat, **kw).kinds().items()} == as_pb
    with pytest.raises(ValueError, match="PackNet: .* is claimed by packed= and by frozen="):
        cl.PackNet(flat, packed=[weight], frozen=r"linear1")
    with pytest.raises(ValueError, match="PackNet: packed=: 'no.such.tensor' is not a trainable tensor"):
        cl.PackNet(flat, packed=["no.such.tensor"])
    with pytest.raises(ValueError, match="PackNet: frozen= 'no_such_tensor' matches no trainable tensor"):
        cl.PackNet(flat, frozen=r"no_such_tensor")
    with pytest.raises(ValueError, match="Piggyback: masked=: 'no.such.tensor' is not a trainable tensor"):
        cl.Piggyback(flat, masked=["no.such.tensor"])                   # Piggyback's strings are as they were
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
            cl.PackNet(flat, prune=bad)


def test_state_dict_round_trips_through_torch_save_in_place(tmp_path):
    from indic_cl_asr_amd import checkpoint
    flat, pn = _pn(prune=0.75, frozen=r"\.bias$")
    _fill(pn)
    sd = pn.state_dict()
    assert set(sd) == {"entries", "kinds", "prune", "owner", "base", "current", "phase", "tasks", "languages"}
    assert sd["entries"] == list(flat.entries) and sd["kinds"] == list(pn.kinds().values())
    assert set(sd["languages"]) == {"hi", "ta"} and sd["tasks"] == {"hi": 1, "ta": 2, "bn": 3}
    assert all(not t.is_cuda for t in (sd["base"], sd["owner"])) and sd["owner"].dtype == torch.uint8
    path = str(tmp_path / "masks.pt")
    checkpoint.save_masks(pn, path)
    flat2, pn2 = _pn()
    theta = flat2.theta.clone()
    ptrs = [t.data_ptr() for t in (pn2.base.flat, pn2.owner, pn2.seg_kind)]
    assert checkpoint.load_masks(pn2, path) is pn2
    assert ptrs == [t.data_ptr() for t in (pn2.base.flat, pn2.owner, pn2.seg_kind)]      # an optimizer holds them
    assert torch.equal(pn2.base.flat, pn.base.flat) and torch.equal(pn2.owner, pn.owner)
    assert torch.equal(pn2.seg_kind, pn.seg_kind) and pn2.kinds() == pn.kinds()
    assert (pn2.prune_fraction, pn2.current, pn2.phase, pn2.train_owner) == (0.75, "bn", "retrain", 3)
    assert pn2.languages() == ["hi", "ta"] and pn2.tasks == {"hi": 1, "ta": 2, "bn": 3}
    for lang in ("hi", "ta"):
        a, b = pn.records[lang], pn2.records[lang]
        assert a["task"] == b["task"]
        for part in ("free", "buffers"):
            assert set(a[part]) == set(b[part]) and all(torch.equal(a[part][n], b[part][n]) for n in a[part])
    assert torch.equal(flat2.theta, theta)                       # the weights are not PackNet state
    sd["base"].zero_()                                           # the saved tensors are copies, not views
    assert pn.base.flat.abs().sum() > 0
    for phase, owner in (("train", 0), ("finished", -1), (None, -1)):
        sd2 = pn.state_dict()
        sd2["phase"] = phase
        pn2.load_state_dict(sd2)
        assert pn2.train_owner == owner


def test_other_trainable_set_is_refused(tmp_path):
    from indic_cl_asr_amd import checkpoint, cl
    _, pn = _pn(freeze_till=0)
    _fill(pn)
    _, other = _pn(freeze_till=1)
    with pytest.raises(ValueError, match="'masks' was saved for a different set of trainable tensors"):
        other.load_state_dict(pn.state_dict())
    path = str(tmp_path / "masks.pt")
    checkpoint.save_masks(pn, path)
    with pytest.raises(ValueError, match="was saved for a different set of trainable tensors"):
        checkpoint.load_masks(other, path)
    with pytest.raises(ValueError, match="owner map"):
        pn.load_state_dict(cl.Piggyback(pn.flat).state_dict())


def test_fused_adamw_refusals_and_unchanged_state_keys():
    from indic_cl_asr_amd import cl
    flat, pn = _pn()
    plain = cl.FusedAdamW(flat, lr=3e-4)
    opt = cl.FusedAdamW(flat, lr=3e-4, masks=pn)
    assert opt.masks is pn and pn._optimizer() is opt
    assert set(opt.state_dict()) == set(plain.state_dict())
    assert set(opt.param_groups[0]) == set(plain.param_groups[0])
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=pn, path_integral=cl.SynapticIntelligence(flat))
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=pn, projection=cl.AveragedGEM(flat))
    with pytest.raises(ValueError, match="masks cannot be combined"):
        cl.FusedAdamW(flat, masks=pn, projection=cl.GEM(flat, max_tasks=2))
    other = _model()
    with pytest.raises(ValueError, match="another FlatParams"):
        cl.FusedAdamW(other, masks=pn)
    with pytest.raises(ValueError, match="another FlatParams"):
        pn.begin_language("hi", cl.FusedAdamW(other, lr=3e-4))


def test_phase_errors():
    from indic_cl_asr_amd import cl
    flat, pn = _pn()
    opt = cl.FusedAdamW(flat, lr=3e-4, masks=pn)
    with pytest.raises(RuntimeError, match="begin_language"):
        pn.prune(opt)                                            # before begin_language
    with pytest.raises(RuntimeError, match="no language is open"):
        pn.finish_language()
    with pytest.raises(ValueError, match="unknown language 'hi'"):
        pn.activate("hi")
    theta = flat.theta.clone()
    pn.begin_language("hi", opt)                                 # the first language keeps theta: nothing is launched
    assert torch.equal(flat.theta, theta)
    assert (pn.current, pn.phase, pn.train_owner, pn.tasks) == ("hi", "train", 0, {"hi": 1})
    with pytest.raises(RuntimeError, match="'hi' is still open"):
        pn.begin_language("ta", opt)
    with pytest.raises(RuntimeError, match="has not been pruned"):
        pn.finish_language()
    for bad in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
            pn.prune(opt, fraction=bad)
    pn.phase, pn.train_owner = "retrain", 1                      # what prune() leaves (the kernel needs the device)
    with pytest.raises(RuntimeError, match="pruned already"):
        pn.prune(opt)                                            # twice in one language
    with pytest.raises(RuntimeError, match="still open"):
        pn.begin_language("ta", opt)
    pn.owner.fill_(1)
    pn.finish_language()
    assert (pn.phase, pn.train_owner, pn.languages()) == ("finished", -1, ["hi"])
    assert set(pn.records["hi"]) == {"task", "free", "buffers"} and pn.records["hi"]["task"] == 1
    with pytest.raises(RuntimeError, match="prune: no language is open"):
        pn.prune(opt)
    with pytest.raises(ValueError, match="trained already"):
        pn.begin_language("hi", opt)
    with pytest.raises(RuntimeError, match="no packed tensor has a free weight left"):
        pn.begin_language("ta", opt)                             # every packed weight is owned
    _, lone = _pn()
    lone.phase, lone.current, lone.tasks = "train", "hi", {"hi": 1}
    with pytest.raises(RuntimeError, match="no optimizer is attached"):
        lone.prune()


def test_a_256th_language_is_refused():
    _, pn = _pn()
    rec = {"free": {}, "buffers": {}}
    for t in range(1, 256):
        pn.tasks[f"l{t}"] = t
        pn.records[f"l{t}"] = dict(rec, task=t)
    pn.phase = "finished"
    with pytest.raises(ValueError, match="255 languages"):
        pn.begin_language("one too many")


def test_entry_points_refuse_bad_arguments():
    """Argument checks come before any device work: -1 (IA_INVALID_VALUE) with no GPU in the machine."""
    from indic_cl_asr_amd import _lib
    L, p = _lib.lib(), _lib.ptr
    assert L.ia_adamw_step_segmented_packed(None, None, None, None, None, 1, None, None, 1, 0, 0.9, 0.999, 1e-8, 1.0, None, None,
                                            1, None, None, None, 0, None, None, None, 0, None) == -1
    assert L.ia_grad_norm_packed(None, None, 1, None, 1, 1.0, 0.0, None, None, None, None, 0, None, None, 0, None) == -1
    assert L.ia_pack_prune(None, None, None, None, None, 1, None, 1, 0.5, 1, None, None, None, 0, None) == -1
    assert L.ia_pack_apply(None, None, None, None, 1, None, 1, 1, 255, None, None) == -1
    assert L.ia_pack_prune_workspace_bytes(0) == 0 and L.ia_pack_prune_workspace_bytes(3) == 3 * (16 + 256 * 4)
    host = torch.zeros(64)                                       # never dereferenced: the values are checked first
    owner = torch.zeros(64, dtype=torch.uint8)
    kind = torch.ones(1, dtype=torch.int32)
    counts = torch.zeros(2, dtype=torch.int32)
    table = torch.tensor([0, 64, 0, 0], dtype=torch.int32)
    ws = torch.zeros(L.ia_pack_prune_workspace_bytes(1), dtype=torch.uint8)

    def prune(fraction=0.5, task=1, theta=host, own=owner, nbytes=ws.numel()):
        return L.ia_pack_prune(p(theta), p(host), p(host), p(own), p(table), 1, p(kind), 1, fraction, task, None, p(counts), p(ws),
                               nbytes, None)

    for task in (0, -1, 256):
        assert prune(task=task) == -1, task
    for fraction in (1.0, -0.25, 1.5, float("nan"), float("inf")):
        assert prune(fraction=fraction) == -1, fraction
    assert prune(theta=host[1:]) == -1 and prune(own=owner[1:]) == -1         # misaligned
    assert prune(nbytes=ws.numel() - 1) == -2                                  # IA_WORKSPACE_TOO_SMALL, still before any launch
    assert L.ia_pack_apply(p(host), p(host), p(owner), p(table), 0, p(kind), 1, 1, 255, None, None) == -1
    assert L.ia_pack_apply(p(host), p(host), p(owner[1:]), p(table), 1, p(kind), 1, 1, 255, None, None) == -1
