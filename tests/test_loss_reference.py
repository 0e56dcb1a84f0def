"""Pins oracle/loss_ref.py -- the fp64 restatement the CTC and transducer kernels are held to in test_loss_reference_gpu.py --
against independent statements of the same losses (CPU only): ATen's double CTC with its autograd gradient at every width
boundary of the kernels' dispatch, a brute-force sum over every alignment, two closed forms, the pure-Python transducer of
oracle/rnnt_oracle.py, the recorded answers under tests/golden/ and the fp32 C oracle for FastEmit and the clamp."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_cases as LC
from conftest import GOLDEN
from oracle import loss_ref
from oracle import rnnt_oracle as orc


def test_case_tables_reach_every_instantiation_and_boundary():
    assert {s for s, _, _ in LC.CTC_TABLE} == {0, 1, 31, 32, 63, 64, 127, 128, 255}
    assert {v for _, v, _ in LC.CTC_TABLE} == {2, 17, 65, 257} and max(v for _, v, _ in LC.CTC_TABLE_LOGITS) > 512
    for lo, hi in ((0, 31), (32, 63), (64, 127), (128, 255)):                  # each K of ctc_alpha_beta: both scales
        assert {sc for s, _, sc in LC.CTC_TABLE if lo <= s <= hi} == {1.5, 30.0}
    names = LC.ctc_batch(32, 17, 1.5)["names"]
    assert {"full", "t1_empty", "t1_one", "t2", "t3", "t5", "empty_long", "minimal", "infeasible", "unique", "len0_empty"} <= set(names)
    assert {u for u, _, _ in LC.RNNT_TABLE} >= {1, 2, 63, 64, 127, 128, 255, 256, 511, 512, 1023}
    assert {t for _, t, _ in LC.RNNT_TABLE} == {1, 2, 3, 7, 9, 17}
    assert {v for _, _, v in LC.RNNT_TABLE} == {1, 2, 3, 4, 5, 63, 64, 65, 128, 129, 192, 256, 320, 384, 448, 512, 513}
    assert {(v + 63) // 64 for _, _, v in LC.RNNT_TABLE} >= set(range(1, 10))   # NV = 1 .. 8 and the generic path
    for lo, hi in ((1, 63), (64, 127), (128, 255), (256, 511), (512, 1023)):   # each K of rnnt_alpha_beta: odd and even V
        assert {v % 2 for u, _, v in LC.RNNT_TABLE if lo <= u <= hi} == {0, 1}
    for u, t, v in LC.RNNT_TABLE:
        assert (v <= 5 and t <= 9) if u > 9 else True
        assert v > 1 or u == 1
        assert 4 * t * u * v * 4 <= 4 << 20                                    # the largest tensor stays a few MB
    c = LC.rnnt_batch(64, 7, 2)
    assert c["flen"][0] == 7 and c["flen"][1] == 1 and c["glen"][2] == 0 and c["glen"][3] == 63


def _aten_ctc(c, zero_infinity=True):
    lp = torch.tensor(c["x"], dtype=torch.double).requires_grad_(True)
    nll = F.ctc_loss(lp.transpose(0, 1), torch.tensor(c["targets"]), torch.tensor(c["il"]), torch.tensor(c["tl"]),
                     blank=c["blank"], reduction="none", zero_infinity=zero_infinity)
    return lp, nll


@pytest.mark.parametrize("S,V,scale", LC.CTC_TABLE)
def test_ctc_ref_matches_aten_double(S, V, scale):
    c = LC.ctc_case(S, V, scale, "lp")
    r = c["r64"]
    names = c["names"]
    expect_inf = {"infeasible", "len0_one"}
    assert [n in expect_inf for n in names] == (~r["feasible"]).tolist()
    _, raw = _aten_ctc(c, zero_infinity=False)
    assert np.array_equal(np.isinf(raw.detach().numpy()), ~r["feasible"])
    lp, nll = _aten_ctc(c)
    (nll * torch.tensor(c["w"], dtype=torch.double)).sum().backward()
    want = np.where(r["feasible"], r["nll"], 0.0)
    assert np.allclose(nll.detach().numpy(), want, rtol=1e-12, atol=1e-10)
    got = r["grad_lp"] * c["w"].astype(np.float64)[:, None, None]
    # two fp64 evaluations of alpha + beta + nll - lp at |nll| up to a few thousand: 1e-9 is ~1e4 double ulps of that sum
    assert np.abs(lp.grad.numpy() - got).max() <= 1e-9
    live = (np.arange(c["T"])[None, :] < c["il"][:, None]) & r["feasible"][:, None]
    assert np.abs(r["occupancy"].sum(-1)[live] - 1.0).max() <= 1e-9        # => sum_v (softmax - occupancy) = 0
    assert not r["grad_lp"][~live].any() and not r["occupancy"][~live].any()


def test_ctc_ref_logits_form_is_log_softmax_then_ctc():
    c = LC.ctc_case(63, 17, 1.5, "logits")
    r = c["r64"]
    x = torch.tensor(c["logits"], dtype=torch.double).requires_grad_(True)
    nll = F.ctc_loss(x.log_softmax(-1).transpose(0, 1), torch.tensor(c["targets"]), torch.tensor(c["il"]), torch.tensor(c["tl"]),
                     blank=c["blank"], reduction="none", zero_infinity=True)
    nll.sum().backward()
    assert np.allclose(nll.detach().numpy(), np.where(r["feasible"], r["nll"], 0.0), rtol=1e-12, atol=1e-10)
    assert np.abs(x.grad.numpy() - r["grad_logits"]).max() <= 1e-9
    live = (np.arange(c["T"])[None, :] < c["il"][:, None]) & r["feasible"][:, None]
    assert np.abs(r["grad_logits"].sum(-1)).max() <= 1e-9                   # the logits gradient sums to 0 over the classes
    assert np.allclose(r["lse"][live], torch.logsumexp(x.detach(), -1).numpy()[live], rtol=1e-14)


def test_ctc_ref_never_reads_the_padding_columns():
    c = LC.ctc_case(32, 17, 1.5, "logits")
    pad = np.full((c["B"], c["T"], c["V"] + 24), np.nan, np.float32)
    pad[:, :, :c["V"]] = c["logits"]
    r = loss_ref.ctc_ref(pad, c["targets"], c["il"], c["tl"], c["blank"], logits=True, valid_cols=c["V"])
    assert np.array_equal(r["nll"], c["r64"]["nll"]) and np.array_equal(r["grad_logits"], c["r64"]["grad_logits"])
    assert r["grad_logits"].shape[-1] == c["V"]


@pytest.mark.parametrize("T,V,target", [(1, 2, [0]), (2, 2, [0, 0]), (3, 2, [0, 0]), (3, 3, [0, 1]), (4, 3, [1, 1]), (5, 3, [0, 1]),
                                        (5, 3, [1, 1]), (4, 3, [2]), (5, 3, []), (5, 2, [0, 0])])
def test_ctc_ref_matches_brute_force_enumeration(T, V, target):
    rng = np.random.default_rng(T * 10 + V)
    for blank in range(V):
        tg = [v if v != blank else (blank + 1) % V for v in target]
        if V == 2:
            tg = [1 - blank] * len(target)
        lp = np.log(rng.dirichlet(np.ones(V), size=T))
        if T >= 4:
            lp[2, tg[0] if tg else blank] = -np.inf            # a forbidden emission
        want = loss_ref.ctc_brute_force(lp, tg, blank)
        r = loss_ref.ctc_ref(lp[None], np.asarray(tg, np.int64).reshape(1, -1), [T], [len(tg)], blank, logits=False)
        if np.isinf(want):
            assert np.isinf(r["nll"][0]) and not r["feasible"][0] and not r["grad_lp"].any()
        else:
            assert abs(r["nll"][0] - want) <= 1e-12 * max(1.0, abs(want))


def test_ctc_ref_closed_forms():
    rng = np.random.default_rng(4)
    T, V, blank = 40, 6, 2
    lp = np.log(rng.dirichlet(np.ones(V), size=T))[None]
    r = loss_ref.ctc_ref(lp, np.zeros((1, 0), np.int64), [T], [0], blank, logits=False)
    assert abs(r["nll"][0] + lp[0, :, blank].sum()) <= 1e-12 * abs(r["nll"][0])          # the all-blank transcript
    for S in (1, 2, 31, 255):
        T = 2 * S - 1                                                                  # S copies of one label: one path
        lp = np.log(rng.dirichlet(np.ones(V), size=T))[None]
        tg = np.full((1, S), 4, np.int64)
        r = loss_ref.ctc_ref(lp, tg, [T], [S], blank, logits=False)
        path = -(lp[0, 0::2, 4].sum() + lp[0, 1::2, blank].sum())
        assert abs(r["nll"][0] - path) <= 1e-12 * path
        occ = np.zeros((T, V)); occ[0::2, 4] = 1.0; occ[1::2, blank] = 1.0
        assert np.abs(r["occupancy"][0] - occ).max() <= 1e-9
        if S > 1:
            short = loss_ref.ctc_ref(lp[:, :T - 1], tg, [T - 1], [S], blank, logits=False)
            assert np.isinf(short["nll"][0]) and not short["grad_lp"].any()


def test_ctc_ref_edge_lengths_and_fp32_replay():
    rng = np.random.default_rng(6)
    lp = np.log(rng.dirichlet(np.ones(5), size=(4, 3))).astype(np.float32)
    tg = np.asarray([[0, 0], [1, 2], [3, 3], [0, 1]])
    r = loss_ref.ctc_ref(lp, tg, [0, 0, 1, 1], [0, 1, 0, 1], 4, logits=False)
    assert r["nll"][0] == 0.0 and np.isinf(r["nll"][1])
    assert r["nll"][2] == -np.float64(lp[2, 0, 4]) and r["nll"][3] == -np.float64(lp[3, 0, 0])
    c = LC.ctc_case(64, 17, 30.0, "lp")
    assert c["r32"]["nll"].dtype == np.float32 and c["r32"]["alpha"].dtype == np.float32 and c["r32"]["grad_lp"].dtype == np.float32
    # the replay really runs in fp32 and stays fp32-small: |nll| reaches 4e3 at logit scale 30, where one fp32 ulp is 2.4e-4
    assert 0.0 < c["e_nll"] < 1e-2 and 0.0 < c["e_grad"] < 1e-2


# ------------------------------------------------------------------------------------------------------------- RNNT
@pytest.mark.parametrize("U1,T,V", [(1, 1, 1), (1, 4, 3), (2, 2, 2), (5, 6, 7), (9, 3, 65), (64, 3, 4)])
def test_rnnt_ref_matches_pure_python(U1, T, V):
    c = LC.rnnt_case(U1, T, V, 0.0, 0.0)
    costs, grads = orc.rnnt_loss_numpy(c["logits"], c["labels"], c["flen"], c["glen"], c["blank"])
    r = c["r64"]
    assert np.allclose(r["costs"], costs, rtol=1e-12, atol=1e-12)
    for b in range(c["B"]):
        Tb, Ub = int(c["flen"][b]), int(c["glen"][b]) + 1
        assert np.abs(r["grads"][b, :Tb, :Ub] - grads[b, :Tb, :Ub]).max() <= 1e-12
        out = np.ones((T, U1), bool); out[:Tb, :Ub] = False
        assert not r["grads"][b][out].any() and not r["alphas"][b][out].any() and not r["betas"][b][out].any()
        assert np.abs(r["grads"][b, :Tb, :Ub].sum(-1)).max() <= 1e-12      # sums to 0 over the vocabulary in every live cell
        assert abs(r["betas"][b, 0, 0] - r["ll"][b]) <= 1e-10 * max(1.0, abs(r["ll"][b]))


KA = json.load(open(os.path.join(GOLDEN, "rnnt_known_answers.json")))


def test_rnnt_ref_known_answers():
    k = KA["test_case_small"]
    acts = np.array(k["acts"], np.float32)
    r = loss_ref.rnnt_ref(acts, np.array(k["labels"]), [acts.shape[1]], [2], 0)
    assert np.allclose(r["costs"].sum(), k["expected_cost"], atol=1e-6, rtol=1e-6)
    assert np.allclose(r["grads"], np.array(k["expected_grads"]), atol=1e-6, rtol=1e-5)
    k = KA["test_case_big_tensor"]
    acts = np.array(k["acts"], np.float32)
    B, T, U1, V = acts.shape
    r = loss_ref.rnnt_ref(acts, np.array(k["labels"]), [T] * B, [U1 - 1] * B, 0)
    assert np.allclose(r["costs"], k["expected_costs"], atol=1e-5)
    assert np.allclose(r["grads"], np.array(k["expected_grads"]), atol=1e-6, rtol=1e-3)
    k = KA["test_case_small_clamp"]
    acts = np.array(k["acts"], np.float32)
    r = loss_ref.rnnt_ref(acts, np.array(k["labels"]), [acts.shape[1]], [2], 0, clamp=k["GRAD_CLAMP"])
    assert np.allclose(r["costs"].sum(), k["expected_cost"], atol=1e-6, rtol=1e-5)
    assert np.allclose(r["grads"], np.array(k["expected_grads"]), atol=1e-6, rtol=1e-5)


def _npz():
    z = np.load(os.path.join(GOLDEN, "rnnt_numpy_cases.npz"))
    return z, sorted({k.split("/")[0] for k in z.files})


@pytest.mark.parametrize("name", _npz()[1])
def test_rnnt_ref_recorded_cases(name):
    z, _ = _npz()
    g = lambda k: z[f"{name}/{k}"]
    fe = float(g("fastemit"))
    r = loss_ref.rnnt_ref(g("acts"), g("labels"), g("flen"), g("glen"), int(g("blank")), fe)
    # the recorded arrays are fp32 results of the reference's own implementation
    assert np.allclose(r["costs"], g("costs"), atol=2e-5, rtol=1e-5)
    assert np.allclose(r["alphas"], g("alphas"), atol=2e-5, rtol=1e-5)
    assert np.allclose(r["betas"], g("betas"), atol=2e-5, rtol=1e-5)
    if fe == 0.0:   # with FastEmit the fused logits gradient carries a term the recorded autograd path does not
        assert np.allclose(r["grads"], g("grads_logits"), atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("fastemit,clamp", [(0.01, 0.0), (0.0, 0.05), (0.25, 0.0), (0.1, 0.02)])
@pytest.mark.parametrize("U1,T,V", [(2, 2, 3), (5, 6, 7), (9, 3, 65), (63, 3, 4)])
def test_rnnt_ref_fastemit_and_clamp_match_the_c_oracle(U1, T, V, fastemit, clamp):
    c = LC.rnnt_batch(U1, T, V)
    a = (c["logits"], c["labels"], c["flen"], c["glen"], c["blank"], fastemit, clamp)
    r = loss_ref.rnnt_ref(*a)
    o = orc.rnnt_loss(*a)
    sc = max(1.0, np.abs(r["costs"]).max())
    # the C oracle is fp32 throughout: a few hundred ulps of the lattice magnitude after U1 + T dependent log-add-exps
    assert np.abs(o["costs"] - r["costs"]).max() <= 3e-5 * sc
    assert np.abs(o["alphas"] - r["alphas"]).max() <= 3e-5 * sc and np.abs(o["betas"] - r["betas"]).max() <= 3e-5 * sc
    assert np.abs(o["grads"] - r["grads"]).max() <= 3e-5 * sc
    if clamp > 0.0:
        assert np.abs(r["grads"]).max() <= clamp and (np.abs(r["grads"]) == clamp).any()      # the clamp bites
    else:
        plain = loss_ref.rnnt_ref(*a[:5])
        assert np.allclose(r["costs"], (1.0 + fastemit) * plain["costs"], rtol=1e-12)
        assert np.abs(r["grads"] - plain["grads"]).max() > 1e-4                               # FastEmit bites
        for b in range(c["B"]):
            Tb, Ub = int(c["flen"][b]), int(c["glen"][b]) + 1
            # FastEmit scales the label branch by (1 + lambda) in the subtracted term and by lambda in the softmax term: the sum
            # over the vocabulary stays 0 in every live cell
            assert np.abs(r["grads"][b, :Tb, :Ub].sum(-1)).max() <= 1e-12


def test_rnnt_ref_fp32_replay_and_speed_of_the_long_cases():
    c = LC.rnnt_case(1023, 9, 3, 0.0, 0.0)
    assert c["r32"]["alphas"].dtype == np.float32 and c["r32"]["grads"].dtype == np.float32
    assert 0.0 < c["e_costs"] < 1e-1 and 0.0 < c["e_grads"] < 1e-2
    c = LC.ctc_long_case("lp")
    # 3000 dependent fp32 roundings at |alpha| up to 8e3 (ulp 4.9e-4): a random walk of about sqrt(3000) half-ulps, 1.3e-2
    assert c["r64"]["feasible"].all() and 0.0 < c["e_grad"] < 1e-1
