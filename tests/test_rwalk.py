"""cl.RWalk on the CPU (host logic only: no kernel is launched; the step and the consolidation themselves run in
tests/test_rwalk_gpu.py): initial state, argument refusals, state dict, CL-state files, layout refusal, the three buffers of
EWC++ alone, and the argument checks of the two C entries."""
import pytest
import torch

ALL = ("fisher", "importance", "theta_star", "w", "anchor", "score", "score_acc")
EWCPP = ALL[:3]


def _rw(freeze_till=0, **kw):
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny'))
    freeze_layer(m, freeze_till)
    flat = cl.FlatParams(m)
    return flat, cl.RWalk(flat, **kw)


def _fill(rw):
    g = torch.Generator().manual_seed(5)
    for k in (ALL if rw.scores else EWCPP):
        getattr(rw, k).flat.copy_(torch.rand(rw.flat.numel, generator=g))
    rw.tasks_consolidated, rw.calls = 3, 7


def _assert_equal_state(a, b):
    for k in (ALL if a.scores else EWCPP):
        assert torch.equal(getattr(a, k).flat, getattr(b, k).flat), k


def test_initial_state():
    flat, rw = _rw()
    assert (rw.rw_lambda, rw.alpha, rw.interval, rw.eps, rw.scores, rw.normalize) == (1.0, 0.9, 50, 1e-3, True, True)
    assert rw.tasks_consolidated == 0 and rw.calls == 0
    for k in ("theta_star", "anchor"):
        d = getattr(rw, k)
        assert torch.equal(d.flat, flat.theta) and d.flat.data_ptr() != flat.theta.data_ptr()
    for k in ("fisher", "importance", "w", "score", "score_acc"):
        assert not getattr(rw, k).flat.any(), k
    assert len({getattr(rw, k).flat.data_ptr() for k in ALL}) == 7
    assert set(rw.importance) == set(rw.fisher) == set(flat.names)           # FlatDicts: name -> view
    assert rw.last_maxima.shape == (2,) and rw.last_maxima.dtype == torch.float32 and not rw.last_maxima.any()


def test_ewcpp_alone_allocates_three_buffers():
    flat, rw = _rw(scores=False)
    assert rw.w is None and rw.anchor is None and rw.score is None and rw.score_acc is None
    assert set(rw.flat_dicts()) == {"rw_fisher", "rw_importance", "rw_theta_star"}
    assert set(rw.state_dict()) == {"entries", "rw_lambda", "alpha", "interval", "eps", "scores", "normalize", "calls",
                                    "tasks_consolidated", "fisher", "importance", "theta_star"}
    assert [rw._next_fold() for _ in range(3)] == [0, 0, 0] and rw.calls == 3      # nothing to fold without scores


def test_fold_is_requested_on_every_interval_th_applied_update():
    _, rw = _rw(interval=3)
    assert [rw._next_fold() for _ in range(7)] == [0, 0, 1, 0, 0, 1, 0] and rw.calls == 7
    _, rw = _rw(interval=1)
    assert [rw._next_fold() for _ in range(3)] == [1, 1, 1]


@pytest.mark.parametrize("kw", [dict(alpha=0.0), dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=float("nan")),
                                dict(eps=0.0), dict(eps=-1e-3), dict(eps=float("nan")), dict(interval=0), dict(interval=-2),
                                dict(interval=2.5)])
def test_arguments_are_refused(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        _rw(**kw)


def test_alpha_one_is_allowed():
    _, rw = _rw(alpha=1.0)
    assert rw.alpha == 1.0


def test_state_dict_round_trips_through_torch_save(tmp_path):
    flat, rw = _rw(rw_lambda=0.25, alpha=0.5, interval=4, eps=1e-2, normalize=False)
    _fill(rw)
    sd = rw.state_dict()
    assert set(sd) == {"entries", "rw_lambda", "alpha", "interval", "eps", "scores", "normalize", "calls",
                       "tasks_consolidated"} | set(ALL)
    assert sd["entries"] == list(flat.entries)
    assert all(not v.is_cuda for v in sd.values() if torch.is_tensor(v))
    path = tmp_path / "rw.pt"
    torch.save(sd, path)
    flat2, rw2 = _rw()
    theta = flat2.theta.clone()
    ptrs = [getattr(rw2, k).flat.data_ptr() for k in ALL]
    rw2.load_state_dict(torch.load(path, map_location="cpu"))
    _assert_equal_state(rw, rw2)
    assert (rw2.rw_lambda, rw2.alpha, rw2.interval, rw2.eps, rw2.normalize) == (0.25, 0.5, 4, 1e-2, False)
    assert (rw2.calls, rw2.tasks_consolidated) == (7, 3)
    assert ptrs == [getattr(rw2, k).flat.data_ptr() for k in ALL]            # loaded in place: an optimizer holds them
    assert torch.equal(flat2.theta, theta)                                   # weights are not RWalk state
    sd["fisher"].zero_()                                                     # the saved tensors are copies, not views
    assert rw.fisher.flat.abs().sum() > 0


def test_cl_state_file_round_trips_flat_dicts(tmp_path):
    from indic_cl_asr_amd import checkpoint
    flat, rw = _rw()
    _fill(rw)
    assert set(rw.flat_dicts()) == {"rw_" + k for k in ALL}
    path = str(tmp_path / "cl_state.pt")
    checkpoint.save_cl_state(path, **rw.flat_dicts())
    flat2, rw2 = _rw()
    rw2.load_flat_dicts(checkpoint.load_cl_state(path, flat2))
    _assert_equal_state(rw, rw2)
    assert rw2.tasks_consolidated == 1 and rw2.calls == 0      # the file has no counts: a non-zero importance attaches the penalty
    rw2.load_flat_dicts(checkpoint.load_cl_state(path, flat2), tasks_consolidated=3, calls=7)
    assert (rw2.tasks_consolidated, rw2.calls) == (3, 7)
    flat3, ewcpp = _rw(scores=False)                           # EWC++ alone reads its three buffers from the same file
    ewcpp.load_flat_dicts(checkpoint.load_cl_state(path, flat3))
    assert torch.equal(ewcpp.fisher.flat, rw.fisher.flat)


def test_other_trainable_set_and_other_buffer_set_are_refused(tmp_path):
    from indic_cl_asr_amd import checkpoint
    _, rw = _rw(freeze_till=0)
    _fill(rw)
    flat_other, other = _rw(freeze_till=1)
    with pytest.raises(ValueError, match="'rwalk' was saved for a different set of trainable tensors"):
        other.load_state_dict(rw.state_dict())
    path = str(tmp_path / "cl_state.pt")
    checkpoint.save_cl_state(path, **rw.flat_dicts())
    with pytest.raises(ValueError, match="was saved for a different set of trainable tensors"):
        checkpoint.load_cl_state(path, flat_other)
    flat2, ewcpp = _rw(scores=False)
    with pytest.raises(ValueError, match="scores"):
        ewcpp.load_state_dict(rw.state_dict())
    path2 = str(tmp_path / "ewcpp.pt")
    checkpoint.save_cl_state(path2, **ewcpp.flat_dicts())
    flat3, full = _rw()
    with pytest.raises(ValueError, match="rw_w"):
        full.load_flat_dicts(checkpoint.load_cl_state(path2, flat3))
    bad = rw.state_dict()
    bad["alpha"] = 0.0
    with pytest.raises(ValueError, match="alpha"):
        _rw()[1].load_state_dict(bad)


def test_config_keys_are_read_with_defaults():
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import AttrDict
    flat, _ = _rw()
    rw = cl.RWalk.from_config(flat, AttrDict(cl_config=AttrDict(e_lambda=5.0)))
    assert (rw.rw_lambda, rw.alpha, rw.interval, rw.eps) == (1.0, 0.9, 50, 1e-3)
    rw = cl.RWalk.from_config(flat, AttrDict(cl_config=AttrDict(rwalk_lambda=0.5, rwalk_alpha=0.75, rwalk_interval=10,
                                                                rwalk_eps=0.1)), scores=False)
    assert (rw.rw_lambda, rw.alpha, rw.interval, rw.eps, rw.scores) == (0.5, 0.75, 10, 0.1, False)


def test_optimizer_accepts_it_as_a_path_integral_and_keeps_the_refusals():
    from indic_cl_asr_amd import cl
    flat, rw = _rw()
    plain = cl.FusedAdamW(flat, lr=3e-4)
    opt = cl.FusedAdamW(flat, lr=3e-4, path_integral=rw)
    assert opt.path_integral is rw
    assert set(opt.state_dict()) == set(plain.state_dict())                  # the RWalk buffers are not optimizer state
    other_flat, _ = _rw()
    with pytest.raises(ValueError, match="another FlatParams"):
        cl.FusedAdamW(other_flat, path_integral=rw)
    with pytest.raises(ValueError, match="path_integral"):
        cl.FusedAdamW(flat, path_integral=rw, projection=cl.AveragedGEM(flat))
    with pytest.raises(ValueError, match="path_integral"):
        cl.FusedAdamW(flat, path_integral=rw, masks=cl.Piggyback(flat))


def _step_args(host, table, *, fisher, w, anchor, score, importance, star, alpha=0.9, eps=1e-3, fold=0, counters=None,
               norm_state=None):
    """The operands of ia_adamw_step_segmented_rwalk over one host buffer (never dereferenced: every call here is refused)."""
    from indic_cl_asr_amd import _lib
    import ctypes
    p = _lib.ptr
    one = (ctypes.c_float * 1)(1e-3)
    return (p(host), p(host), p(host), p(host), p(table), 1, p(table), p(table), 1, 0, 0.9, 0.999, 1e-8, 1.0, None, None, 1, one,
            one, norm_state, 0, counters, fisher, w, anchor, score, importance, star, 1.0, alpha, eps, fold, None)


def test_step_entry_refuses_null_and_incomplete_operands():
    """Argument checks come before any device work: -1 (IA_INVALID_VALUE) with no GPU in the machine."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    host, table = torch.zeros(64), torch.zeros(4, dtype=torch.int32)
    h = _lib.ptr(host)
    full = dict(fisher=h, w=h, anchor=h, score=h, importance=h, star=h)
    none = {k: None for k in full}
    assert L.ia_adamw_step_segmented_rwalk(*[None] * 5, 1, None, None, 1, 0, 0.9, 0.999, 1e-8, 1.0, None, None, 1, None, None,
                                           None, 0, None, *[None] * 6, 1.0, 0.9, 1e-3, 0, None) == -1
    bad = [dict(none),                                             # no Fisher
           dict(full, fisher=None),
           dict(full, w=None), dict(full, anchor=None), dict(full, score=None),        # scores: all three or none
           dict(none, fisher=h, w=h),
           dict(full, importance=None), dict(full, star=None),                         # penalty: both or neither
           dict(none, fisher=h, fold=1),                                               # a fold needs the scores
           dict(full, alpha=0.0), dict(full, alpha=1.5), dict(full, alpha=float("nan")),
           dict(full, eps=0.0), dict(full, eps=-1.0),
           dict(full, counters=_lib.ptr(table)),                                       # counters without norm_state
           dict(full, norm_state=h)]
    for kw in bad:
        assert L.ia_adamw_step_segmented_rwalk(*_step_args(host, table, **kw)) == -1, kw
    off = torch.zeros(68)[1:]                                      # 4 bytes off a 16-byte boundary
    if off.data_ptr() % 16:
        assert L.ia_adamw_step_segmented_rwalk(*_step_args(host, table, **dict(full, fisher=_lib.ptr(off)))) == -1


def test_consolidate_entry_refuses_null_and_incomplete_operands():
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    assert L.ia_rwalk_workspace_bytes(0) == 0 and L.ia_rwalk_workspace_bytes(5) == 40
    host, table = torch.zeros(64), torch.zeros(4, dtype=torch.int32)
    h, t = _lib.ptr(host), _lib.ptr(table)

    def call(theta=h, star=h, fisher=h, w=h, anchor=h, score=h, acc=h, importance=h, maxima=h, eps=1e-3, n=64, tab=t, nchunks=1,
             ws=h, ws_bytes=8):
        return L.ia_rwalk_consolidate(theta, star, fisher, w, anchor, score, acc, importance, maxima, eps, 1, 1, n, tab, nchunks,
                                      ws, ws_bytes, None)

    assert L.ia_rwalk_consolidate(*[None] * 9, 1e-3, 1, 1, 64, None, 1, None, 0, None) == -1
    for kw in (dict(theta=None), dict(star=None), dict(fisher=None), dict(importance=None), dict(maxima=None), dict(tab=None),
               dict(ws=None), dict(w=None), dict(anchor=None), dict(score=None), dict(acc=None),      # the four scores: all or none
               dict(w=None, anchor=None, score=None), dict(eps=0.0), dict(eps=-1.0), dict(n=0), dict(nchunks=0)):
        assert call(**kw) == -1, kw
    assert call(ws_bytes=4) == -2                                  # IA_WORKSPACE_TOO_SMALL, still before any device work
