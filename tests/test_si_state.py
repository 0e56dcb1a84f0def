"""cl.SynapticIntelligence on the CPU (host logic only: no kernel is launched; the step, the consolidation and the penalty
themselves run in tests/test_si_gpu.py): state dict, CL-state files, layout refusal, argument checks of the two C entries."""
import pytest
import torch


def _si(freeze_till=0, **kw):
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny'))
    freeze_layer(m, freeze_till)
    flat = cl.FlatParams(m)
    return flat, cl.SynapticIntelligence(flat, **kw)


def _fill(si):
    g = torch.Generator().manual_seed(5)
    si.w.flat.copy_(torch.randn(si.flat.numel, generator=g))
    si.omega.flat.copy_(torch.rand(si.flat.numel, generator=g))
    si.theta_star.flat.copy_(torch.randn(si.flat.numel, generator=g))
    si.tasks_consolidated = 3


def _assert_equal_state(a, b):
    for x, y in ((a.w, b.w), (a.omega, b.omega), (a.theta_star, b.theta_star)):
        assert torch.equal(x.flat, y.flat)


def test_initial_state():
    flat, si = _si()
    assert si.tasks_consolidated == 0 and si.si_c == 1.0 and si.xi == 1e-3
    assert torch.equal(si.theta_star.flat, flat.theta) and si.theta_star.flat.data_ptr() != flat.theta.data_ptr()
    assert not si.w.flat.any() and not si.omega.flat.any()
    assert set(si.w) == set(flat.names)                          # FlatDicts: name -> view


def test_state_dict_round_trips_through_torch_save(tmp_path):
    flat, si = _si(si_c=0.25, xi=1e-2)
    _fill(si)
    sd = si.state_dict()
    assert set(sd) == {"entries", "w", "omega", "theta_star", "si_c", "xi", "tasks_consolidated"}
    assert sd["entries"] == list(flat.entries)
    assert all(not v.is_cuda for v in sd.values() if torch.is_tensor(v))
    path = tmp_path / "si.pt"
    torch.save(sd, path)
    flat2, si2 = _si()
    theta = flat2.theta.clone()
    ptrs = [d.flat.data_ptr() for d in (si2.w, si2.omega, si2.theta_star)]
    si2.load_state_dict(torch.load(path, map_location="cpu"))
    _assert_equal_state(si, si2)
    assert (si2.si_c, si2.xi, si2.tasks_consolidated) == (0.25, 1e-2, 3)
    assert ptrs == [d.flat.data_ptr() for d in (si2.w, si2.omega, si2.theta_star)]    # loaded in place: an optimizer holds them
    assert torch.equal(flat2.theta, theta)                       # weights are not SI state
    sd["omega"].zero_()                                          # the saved tensors are copies, not views
    assert si.omega.flat.abs().sum() > 0


def test_cl_state_file_round_trips_flat_dicts(tmp_path):
    from indic_cl_asr_amd import checkpoint
    flat, si = _si()
    _fill(si)
    assert set(si.flat_dicts()) == {"si_w", "si_omega", "si_theta_star"}
    path = str(tmp_path / "cl_state.pt")
    checkpoint.save_cl_state(path, **si.flat_dicts())
    flat2, si2 = _si()
    si2.load_flat_dicts(checkpoint.load_cl_state(path, flat2))
    _assert_equal_state(si, si2)
    assert si2.tasks_consolidated == 1                           # the file has no task count: a non-zero omega attaches the penalty
    si2.load_flat_dicts(checkpoint.load_cl_state(path, flat2), tasks_consolidated=3)
    assert si2.tasks_consolidated == 3


def test_other_trainable_set_is_refused(tmp_path):
    from indic_cl_asr_amd import checkpoint
    _, si = _si(freeze_till=0)
    _fill(si)
    flat_other, other = _si(freeze_till=1)
    with pytest.raises(ValueError, match="'si' was saved for a different set of trainable tensors"):
        other.load_state_dict(si.state_dict())
    path = str(tmp_path / "cl_state.pt")
    checkpoint.save_cl_state(path, **si.flat_dicts())
    with pytest.raises(ValueError, match="was saved for a different set of trainable tensors"):
        checkpoint.load_cl_state(path, flat_other)


@pytest.mark.parametrize("xi", [0.0, -1e-3, float("nan")])
def test_xi_must_be_positive(xi):
    with pytest.raises(ValueError, match="xi"):
        _si(xi=xi)


def test_config_keys_are_read_with_defaults():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import AttrDict
    flat, _ = _si()
    si = cl.SynapticIntelligence.from_config(flat, AttrDict(cl_config=AttrDict(e_lambda=5.0)))
    assert (si.si_c, si.xi) == (1.0, 1e-3)
    si = cl.SynapticIntelligence.from_config(flat, AttrDict(cl_config=AttrDict(si_c=0.5, si_xi=0.1)))
    assert (si.si_c, si.xi) == (0.5, 0.1)


def test_optimizer_state_keys_are_unchanged_with_a_path_integral():
    from indic_cl_asr_amd import cl
    flat, si = _si()
    plain = cl.FusedAdamW(flat, lr=3e-4)
    opt = cl.FusedAdamW(flat, lr=3e-4, path_integral=si)
    assert opt.path_integral is si
    sd = opt.state_dict()
    assert set(sd) == set(plain.state_dict()) == {"entries", "exp_avg", "exp_avg_sq", "seg_step", "step_count", "param_group",
                                                  "clipped_steps", "skipped_steps"}
    assert set(opt.param_groups[0]) == set(plain.param_groups[0])
    assert sd["param_group"] == plain.state_dict()["param_group"]
    other_flat, _ = _si()
    with pytest.raises(ValueError, match="another FlatParams"):
        cl.FusedAdamW(other_flat, path_integral=si)


def test_entry_points_refuse_null_pointers():
    """Argument checks come before any device work: -1 (IA_INVALID_VALUE) with no GPU in the machine."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    assert L.ia_adamw_step_segmented_si(None, None, None, None, None, 1, None, None, 1, 0, 1e-3, 0.9, 0.999, 1e-8, 1e-2, 1.0,
                                        None, None, 0, None, None, None, None, 1.0, None) == -1
    assert L.ia_si_consolidate(None, None, None, None, 1e-3, 64, None) == -1
    host = torch.zeros(64)                                       # never dereferenced: xi is checked first
    for xi in (0.0, -1.0):
        assert L.ia_si_consolidate(_lib.ptr(host), _lib.ptr(host), _lib.ptr(host), _lib.ptr(host), xi, 64, None) == -1
