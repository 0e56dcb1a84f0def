"""FusedAdamW parameter groups on the CPU (host logic only: no kernel is launched; the grouped steps themselves run in
tests/test_param_groups_gpu.py): resolution of `param_groups=`, its errors, the two helpers, the torch.optim.Optimizer
surface (schedulers attach), the state with several groups, and the argument validation of
ia_adamw_step_segmented_grouped, which happens before any device work."""
import re

import pytest
import torch

# the schedulers here are stepped without an optimizer step in between: no kernel is launched in this file
pytestmark = pytest.mark.filterwarnings("ignore:Detected call of `lr_scheduler.step\\(\\)` before")


def _tiny(freeze_till=0):
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny'))
    freeze_layer(m, freeze_till)
    return m, cl.FlatParams(m)


def _toy():
    from indic_cl_asr_amd import cl
    from test_optimizer_clip_gpu import Toy
    m = Toy(big=False)
    return m, cl.FlatParams(m)


def _check_resolution(flat, opt, want):
    """`want`: one list of names per group, group 0 first."""
    param = dict(zip(flat.names, flat.params))
    assert len(opt.param_groups) == len(want)
    for g, names in zip(opt.param_groups, want):
        assert g["names"] == names
        assert len(g["params"]) == len(names) and all(p is param[n] for p, n in zip(g["params"], names))
        assert {"params", "names", "lr", "weight_decay", "betas", "eps"} <= set(g)
    assert sorted(n for names in want for n in names) == sorted(e[0] for e in flat.entries)
    index = {n: k for k, names in enumerate(want) for n in names}
    assert opt.seg_group.dtype == torch.int32
    assert opt.seg_group.tolist() == [index[e[0]] for e in flat.entries]


def test_names_parameters_and_match_resolve_on_the_toy():
    from indic_cl_asr_amd import cl
    m, flat = _toy()
    groups = [dict(params=["v5", m.v6, "v7", m.v8, "v9", "idle"], lr=1e-4, weight_decay=0.0, name="slow"),
              dict(match=r"^mat$", lr=3e-3, weight_decay=0.2)]
    opt = cl.FusedAdamW(flat, lr=1e-3, weight_decay=1e-2, param_groups=groups)
    _check_resolution(flat, opt, [[f"v{i}" for i in range(5)], ["v5", "v6", "v7", "v8", "v9", "idle"], ["mat"]])
    g0, g1, g2 = opt.param_groups
    assert (g0["lr"], g0["weight_decay"]) == (1e-3, 1e-2) and (g1["lr"], g1["weight_decay"]) == (1e-4, 0.0)
    assert (g2["lr"], g2["weight_decay"]) == (3e-3, 0.2) and g1["name"] == "slow" and "name" not in g2
    assert "max_grad_norm" in g0 and "skip_nonfinite" in g0 and "max_grad_norm" not in g1 and "skip_nonfinite" not in g2
    assert g1["betas"] == g0["betas"] == (0.9, 0.999) and g2["eps"] == g0["eps"] == 1e-8


def test_resolution_on_the_tiny_model():
    from indic_cl_asr_amd import cl
    m, flat = _tiny()
    heads = [n for n in flat.names if n.startswith("joint.")]
    pos = [n for n in flat.names if re.search(r"pos_bias_[uv]$", n)]
    assert heads and pos
    by_name = dict(m.named_parameters())
    opt = cl.FusedAdamW(flat, param_groups=[dict(params=[by_name[n] for n in heads], lr=5e-3),
                                            dict(match=r"pos_bias_[uv]$", weight_decay=0.0)])
    rest = [n for n in flat.names if n not in heads and n not in pos]
    _check_resolution(flat, opt, [rest, heads, pos])
    assert opt.param_groups[1]["lr"] == 5e-3 and opt.param_groups[1]["weight_decay"] == 1e-2     # weight decay inherited
    assert opt.param_groups[2]["lr"] == 1e-3 and opt.param_groups[2]["weight_decay"] == 0.0       # lr inherited


def test_without_the_keyword_the_list_is_unchanged():
    from indic_cl_asr_amd import cl
    _, flat = _toy()
    opt = cl.FusedAdamW(flat, lr=2e-3)
    assert len(opt.param_groups) == 1
    assert list(opt.param_groups[0]) == ["lr", "betas", "eps", "weight_decay", "max_grad_norm", "skip_nonfinite", "params"]
    assert opt.param_groups[0]["params"] == flat.params and opt.seg_group.tolist() == [0] * len(flat.entries)
    empty = cl.FusedAdamW(flat, lr=2e-3, param_groups=[])
    assert len(empty.param_groups) == 1 and empty.param_groups[0]["names"] == flat.names


def test_every_error_names_the_offender():
    from indic_cl_asr_amd import cl
    m, flat = _toy()
    with pytest.raises(ValueError, match=r"'v3' is claimed by group 1 \('a'\) and by group 2 \('b'\)"):
        cl.FusedAdamW(flat, param_groups=[dict(params=["v3"], name="a"), dict(match=r"^v[23]$", name="b")])
    with pytest.raises(ValueError, match=r"group 1: 'v99' is not a trainable tensor"):
        cl.FusedAdamW(flat, param_groups=[dict(params=["v0", "v99"])])
    stranger = torch.nn.Parameter(torch.zeros(7, 3))
    with pytest.raises(ValueError, match=r"shape \(7, 3\) is not a trainable tensor"):
        cl.FusedAdamW(flat, param_groups=[dict(params=[stranger])])
    with pytest.raises(ValueError, match=r"match 'encoder\\\.' matches no trainable tensor"):
        cl.FusedAdamW(flat, param_groups=[dict(match=r"encoder\.")])
    with pytest.raises(ValueError, match=r"unknown key 'betas'"):
        cl.FusedAdamW(flat, param_groups=[dict(params=["v0"], betas=(0.8, 0.9))])
    with pytest.raises(ValueError, match=r"group 1 needs either 'params' or 'match'"):
        cl.FusedAdamW(flat, param_groups=[dict(lr=1e-4)])
    with pytest.raises(ValueError, match=r"64 groups \+ group 0 exceed the limit of 64"):
        cl.FusedAdamW(flat, param_groups=[dict(params=[])] * 64)
    cl.FusedAdamW(flat, param_groups=[dict(params=[])] * 63)                    # 64 in all: allowed
    # a frozen tensor is not a trainable tensor of the layout
    m2, flat2 = _tiny(freeze_till=0)
    frozen = [n for n, p in m2.named_parameters() if not p.requires_grad][0]
    with pytest.raises(ValueError, match=re.escape(f"'{frozen}' is not a trainable tensor")):
        cl.FusedAdamW(flat2, param_groups=[dict(params=[frozen])])


def test_layerwise_lr_groups_follow_the_formula():
    from indic_cl_asr_amd import cl
    m, flat = _tiny(freeze_till=0)
    L = len(m.encoder.layers)
    groups = cl.layerwise_lr_groups(m, 1e-3, 0.5)
    assert groups == cl.layerwise_lr_groups(flat, 1e-3, 0.5)                    # a model or its FlatParams
    claimed = [n for g in groups for n in g["params"]]
    assert sorted(claimed) == sorted(flat.names) and len(set(claimed)) == len(claimed)          # a partition
    param = dict(zip(flat.names, flat.params))
    for g in groups:
        assert g["params"], "a depth without a trainable tensor is left out"
        for n in g["params"]:
            if n.startswith(("decoder.", "joint.", "ctc_decoder.")):
                want = 1e-3
            elif n.startswith("encoder.layers."):
                want = 1e-3 * 0.5 ** (L - int(n.split(".")[2]))
            else:
                assert n.startswith("encoder.pre_encode.")
                want = 1e-3 * 0.5 ** (L + 1)
            assert g["lr"] == want, (n, g["lr"], want)
            bare = param[n].ndim <= 1 or n.endswith(("pos_bias_u", "pos_bias_v"))
            assert (g.get("weight_decay") == 0.0) == bare and ("weight_decay" in g) == bare, n
    # layer 0 and pre_encode are frozen: their depths do not appear, layer 1 of 2 sits one step below the heads
    assert sorted({g["lr"] for g in groups}) == [0.5e-3, 1e-3] and len(groups) == 4
    opt = cl.FusedAdamW(flat, lr=7.0, param_groups=groups)
    assert opt.param_groups[0]["params"] == [] and len(opt.param_groups) == 5
    one_per_depth = cl.layerwise_lr_groups(m, 1e-3, 0.5, no_decay_1d=False)
    assert len(one_per_depth) == 2 and all("weight_decay" not in g for g in one_per_depth)
    # with everything trainable pre_encode appears at the deepest rate
    m3, flat3 = _tiny(freeze_till=-1)
    for p in m3.parameters():
        p.requires_grad = True
    flat3 = cl.FlatParams(m3)
    deep = [g for g in cl.layerwise_lr_groups(flat3, 1e-3, 0.5) if any(n.startswith("encoder.pre_encode.") for n in g["params"])]
    assert deep and all(g["lr"] == 1e-3 * 0.5 ** (L + 1) for g in deep)


def test_no_decay_groups_claim_vectors_and_position_biases():
    from indic_cl_asr_amd import cl
    m, flat = _tiny(freeze_till=0)
    (g,) = cl.no_decay_groups(m)
    want = [n for n, p in zip(flat.names, flat.params) if p.ndim <= 1 or n.endswith("pos_bias_u") or n.endswith("pos_bias_v")]
    assert g["params"] == want and g["weight_decay"] == 0.0 and "lr" not in g
    assert any(n.endswith("pos_bias_u") and dict(zip(flat.names, flat.params))[n].ndim == 2 for n in want)
    (h,) = cl.no_decay_groups(flat, no_decay=lambda name, p: name.startswith("joint."))
    assert h["params"] == [n for n in flat.names if n.startswith("joint.")]
    opt = cl.FusedAdamW(flat, weight_decay=0.05, param_groups=cl.no_decay_groups(m))
    assert opt.param_groups[0]["weight_decay"] == 0.05 and opt.param_groups[1]["weight_decay"] == 0.0
    assert all(p.ndim >= 2 for p in opt.param_groups[0]["params"])


def test_torch_optimizer_surface_and_schedulers():
    from indic_cl_asr_amd import cl
    _, flat = _toy()
    opt = cl.FusedAdamW(flat, lr=1e-3, param_groups=[dict(params=["v5"], lr=1e-4), dict(match="^mat$", lr=3e-3)])
    assert isinstance(opt, torch.optim.Optimizer)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 1.0 / (1 + e), lambda e: 2.0 ** e, lambda e: 1.0 - 0.25 * e])
    base = [1e-3, 1e-4, 3e-3]
    for epoch in range(1, 4):
        sched.step()
        want = [base[0] * (1.0 / (1 + epoch)), base[1] * 2.0 ** epoch, base[2] * (1.0 - 0.25 * epoch)]
        assert [g["lr"] for g in opt.param_groups] == want
    assert all(g["initial_lr"] == b for g, b in zip(opt.param_groups, base))
    with pytest.raises(NotImplementedError, match="fixed at construction"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(3))]))
    assert len(opt.param_groups) == 3
    plain = cl.FusedAdamW(flat, lr=1e-3)                                       # a scheduler attaches to the one-group form too
    torch.optim.lr_scheduler.LambdaLR(plain, lambda e: 0.5).step()
    assert plain.param_groups[0]["lr"] == 0.5e-3
    opt.param_groups[2]["betas"] = (0.85, 0.999)
    with pytest.raises(ValueError, match=r"param_groups\[2\]\['betas'\]"):
        opt._group_hyper()


def _three_groups(flat, **kw):
    from indic_cl_asr_amd import cl
    return cl.FusedAdamW(flat, lr=1e-3, weight_decay=1e-2, param_groups=[
        dict(params=["v5", "v6", "v7", "v8", "v9", "idle"], lr=1e-4, weight_decay=0.0),
        dict(match="^mat$", lr=3e-3, weight_decay=0.2)], **kw)


def test_state_with_one_group_keeps_its_keys():
    from indic_cl_asr_amd import cl
    _, flat = _toy()
    keys = {"entries", "exp_avg", "exp_avg_sq", "seg_step", "step_count", "param_group", "clipped_steps", "skipped_steps"}
    assert set(cl.FusedAdamW(flat).state_dict()) == keys
    sd = cl.FusedAdamW(flat, param_groups=[]).state_dict()
    assert set(sd) == keys and set(sd["param_group"]) == {"lr", "betas", "eps", "weight_decay", "max_grad_norm", "skip_nonfinite"}


def test_three_group_state_survives_torch_save(tmp_path):
    _, flat = _toy()
    opt = _three_groups(flat, max_grad_norm=2.0)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 0.5 ** e, lambda e: 1.0 + e, lambda e: 1.0 / (1 + e)])
    sched.step(); sched.step()
    g = torch.Generator().manual_seed(5)
    opt.exp_avg.copy_(torch.randn(flat.numel, generator=g))
    opt.seg_step.fill_(2)
    sd = opt.state_dict()
    assert [pg["names"] for pg in sd["param_groups"]] == [pg["names"] for pg in opt.param_groups]
    assert all("params" not in pg and "initial_lr" in pg for pg in sd["param_groups"])
    assert sd["param_group"]["max_grad_norm"] == 2.0 and "names" not in sd["param_group"]
    path = tmp_path / "opt.pt"
    torch.save(sd, path)
    _, flat2 = _toy()
    fresh = _three_groups(flat2)
    fresh.load_state_dict(torch.load(path, map_location="cpu"))
    for a, b in zip(opt.param_groups, fresh.param_groups):
        assert {k: v for k, v in a.items() if k != "params"} == {k: v for k, v in b.items() if k != "params"}
    assert [pg["lr"] for pg in fresh.param_groups] == [1e-3 * 0.25, 1e-4 * 3.0, 3e-3 / 3]
    assert [pg["initial_lr"] for pg in fresh.param_groups] == [1e-3, 1e-4, 3e-3]
    assert fresh.param_groups[0]["max_grad_norm"] == 2.0
    assert torch.equal(fresh.exp_avg, opt.exp_avg) and torch.equal(fresh.seg_step, opt.seg_step)
    assert all(p is q for p, q in zip(fresh.param_groups[2]["params"], [flat2.params[flat2.names.index("mat")]]))


def test_another_partition_is_refused(tmp_path):
    from indic_cl_asr_amd import checkpoint, cl
    _, flat = _toy()
    sd = _three_groups(flat).state_dict()
    _, flat2 = _toy()
    other = cl.FusedAdamW(flat2, param_groups=[dict(params=["v5", "v6", "v7", "v8", "v9"], lr=1e-4, weight_decay=0.0),
                                               dict(params=["mat", "idle"], lr=3e-3, weight_decay=0.2)])
    with pytest.raises(ValueError, match="different partition into parameter groups"):
        other.load_state_dict(sd)
    with pytest.raises(ValueError, match="different partition into parameter groups"):
        cl.FusedAdamW(flat2).load_state_dict(sd)                                # one group here, three saved
    with pytest.raises(ValueError, match="different partition into parameter groups"):
        _three_groups(flat2).load_state_dict(cl.FusedAdamW(flat).state_dict())  # three here, one saved
    path = str(tmp_path / "opt.pt")
    checkpoint.save_optimizer(_three_groups(flat), path)
    assert len(checkpoint.load_optimizer(_three_groups(flat2), path).param_groups) == 3


def test_grouped_entry_point_refuses_invalid_arguments():
    """IA_INVALID_VALUE (-1) before any device work: the library loads and the calls return without a GPU.  The pointers are
    16-byte aligned host addresses that a refused call never dereferences."""
    import ctypes
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    buf = torch.zeros(64, dtype=torch.float32)
    P = ctypes.c_void_p(buf.data_ptr())
    assert buf.data_ptr() % 16 == 0
    lr = (ctypes.c_float * 64)(*([1e-3] * 64))
    wd = (ctypes.c_float * 64)(*([1e-2] * 64))

    def call(theta=P, grad=P, m=P, v=P, table=P, nchunks=1, active=P, step=P, nseg=1, seg_group=P, ngroups=2, glr=lr, gwd=wd,
             norm=None, counters=None, path_w=None, omega=None, star=None, ref=None, proj=None, proj_counters=None):
        return L.ia_adamw_step_segmented_grouped(theta, grad, m, v, table, nchunks, active, step, nseg, 0, 0.9, 0.999, 1e-8, 1.0,
                                                 None, seg_group, ngroups, glr, gwd, norm, 0, counters, path_w, omega, star, 1.0,
                                                 ref, proj, proj_counters, None)

    for name in ("theta", "grad", "m", "v", "table", "active", "step", "glr", "gwd"):
        assert call(**{name: None}) == -1, name
    assert call(nchunks=0) == -1 and call(nseg=0) == -1
    assert call(ngroups=0) == -1 and call(ngroups=65) == -1 and call(ngroups=-3) == -1
    assert call(seg_group=None, ngroups=2) == -1
    assert call(counters=P) == -1                                   # counters without norm_state
    assert call(norm=P) == -1                                       # ... and the reverse
    assert call(path_w=P, ref=P, proj=P, proj_counters=P) == -1     # SI and projection operands together
    assert call(omega=P, star=P, ref=P, proj=P, proj_counters=P) == -1
    assert call(omega=P, star=P) == -1                              # a penalty without the path integral
    assert call(path_w=P, omega=P) == -1                            # omega without theta_star
    assert call(ref=P) == -1 and call(ref=P, proj=P) == -1          # an incomplete projection triple
    off4 = ctypes.c_void_p(buf.data_ptr() + 4)                      # the alignment conditions of the four
    for name in ("theta", "grad", "m", "v", "table"):
        assert call(**{name: off4}) == -1, name
    assert call(path_w=off4) == -1 and call(ref=off4, proj=P, proj_counters=P) == -1
