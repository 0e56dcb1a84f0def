"""FusedAdamW.state_dict / load_state_dict and checkpoint.save_optimizer / load_optimizer on the CPU (host logic only: no
kernel is launched; the resumed steps themselves run in tests/test_optimizer_clip_gpu.py)."""
import pytest
import torch


def _optimizer(freeze_till=0, **kw):
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny'))
    freeze_layer(m, freeze_till)
    flat = cl.FlatParams(m)
    return flat, cl.FusedAdamW(flat, **kw)


def _fill(opt):
    g = torch.Generator().manual_seed(3)
    opt.exp_avg.copy_(torch.randn(opt.flat.numel, generator=g))
    opt.exp_avg_sq.copy_(torch.rand(opt.flat.numel, generator=g))
    opt.seg_step.copy_(torch.randint(0, 50, (len(opt.flat.entries),), generator=g, dtype=torch.int32))
    opt.step_count = 57
    opt._counters.copy_(torch.tensor([5, 2], dtype=torch.int32))


def _assert_equal_state(a, b):
    assert torch.equal(a.exp_avg, b.exp_avg) and torch.equal(a.exp_avg_sq, b.exp_avg_sq)
    assert torch.equal(a.seg_step, b.seg_step) and a.step_count == b.step_count
    ga = {k: v for k, v in a.param_groups[0].items() if k != "params"}
    gb = {k: v for k, v in b.param_groups[0].items() if k != "params"}
    assert ga == gb
    sa, sb = a.stats(), b.stats()
    assert (sa["clipped_steps"], sa["skipped_steps"]) == (sb["clipped_steps"], sb["skipped_steps"]) == (5, 2)


def test_state_dict_round_trips_through_torch_save(tmp_path):
    flat, opt = _optimizer(lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05, max_grad_norm=2.5, skip_nonfinite=True)
    _fill(opt)
    sd = opt.state_dict()
    assert set(sd) == {"entries", "exp_avg", "exp_avg_sq", "seg_step", "step_count", "param_group", "clipped_steps",
                       "skipped_steps"}
    assert "params" not in sd["param_group"] and sd["entries"] == list(flat.entries)
    assert sd["param_group"] == dict(lr=3e-4, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.05, max_grad_norm=2.5,
                                     skip_nonfinite=True)
    path = tmp_path / "opt.pt"
    torch.save(sd, path)
    flat2, opt2 = _optimizer()
    theta = flat2.theta.clone()
    opt2.load_state_dict(torch.load(path, map_location="cpu"))
    _assert_equal_state(opt, opt2)
    assert torch.equal(flat2.theta, theta)                       # weights are not optimizer state
    sd["exp_avg"].zero_()                                        # the saved tensors are copies, not views
    assert opt.exp_avg.abs().sum() > 0


def test_defaults_report_nothing_measured():
    _, opt = _optimizer()
    st = opt.stats()
    assert st["grad_norm"] != st["grad_norm"] and st["clip_coef"] == 1.0
    assert st["clipped_steps"] == 0 and st["skipped_steps"] == 0
    g = opt.param_groups[0]
    assert g["max_grad_norm"] is None and g["skip_nonfinite"] is False
    with pytest.raises(RuntimeError):
        opt.grad_norms()


def test_other_trainable_set_is_refused(tmp_path):
    _, opt = _optimizer(freeze_till=0)
    _fill(opt)
    _, other = _optimizer(freeze_till=1)
    with pytest.raises(ValueError, match="different set of trainable tensors"):
        other.load_state_dict(opt.state_dict())
    from indic_cl_asr_amd import checkpoint
    path = str(tmp_path / "opt.pt")
    checkpoint.save_optimizer(opt, path)
    with pytest.raises(ValueError, match="different set of trainable tensors"):
        checkpoint.load_optimizer(other, path)


def test_checkpoint_wrappers_agree_with_state_dict(tmp_path):
    from indic_cl_asr_amd import checkpoint
    _, opt = _optimizer(lr=3e-4, max_grad_norm=2.5)
    _fill(opt)
    path = str(tmp_path / "opt.pt")
    checkpoint.save_optimizer(opt, path)
    _, opt2 = _optimizer()
    assert checkpoint.load_optimizer(opt2, path) is opt2
    _assert_equal_state(opt, opt2)
    a, b = opt.state_dict(), opt2.state_dict()
    assert a["entries"] == b["entries"] and a["param_group"] == b["param_group"]
