"""oracle/decode_ref.py (the fp64 replay of greedy transducer decoding and its acceptable sets, the reference of
tests/test_decode_reference_gpu.py) pinned on the CPU: it equals the independent per-utterance oracle and the fp32 torch loop of
tests/test_greedy_decode_gpu.py where no tolerance is in play, the conditions that keep an acceptable set from hiding a failure
hold for every case the GPU file uses (same generators, same seeds), a hand-made near-tie branches into exactly its two
continuations, and a perturbation of twice a step's tolerance (past the runner-up's deficit) moves the main path out of the old set."""
import pytest
import torch

from oracle import decode_ref as R
from oracle import step_ref as S

import test_decode_reference_gpu as G
from test_greedy_decode_gpu import _bf16_case, _bf16_decode_torch


@pytest.mark.parametrize("max_symbols", [1, 3, 10])
def test_exact_reference_equals_the_per_utterance_oracle(max_symbols):
    from test_decoding import _models
    o, _ = _models()
    g = torch.Generator().manual_seed(3)
    enc = torch.randn(4, 32, 23, generator=g)
    lens = torch.tensor([23, 17, 9, 1])
    total = 0
    for lang in ('hi', 'ta'):
        case = R.case_from_model(o, enc, lens, lang)
        assert not case["bf16"] and case["f_all"].dtype == torch.float64
        got = [r["hyp"] for r in R.decode_reference(case, max_symbols, None)]
        assert got == S.greedy_rnnt_decode_ref(o, enc, lens, lang, max_symbols=max_symbols)
        total += sum(len(h) for h in got)
        # the tolerant replays follow the same main path and, on these margins, accept nothing else
        for mode in ("gemv", "mfma"):
            res = R.decode_reference(case, max_symbols, mode)
            assert [r["hyp"] for r in res] == got or mode == "mfma"
            assert all(tuple(r["hyp"]) in r["accept"] for r in res)
    assert total > 0


def test_exact_reference_restarts_from_the_blank_row_after_a_first_blank():
    """_bf16_decode_torch's semantics on a case whose first evaluation is blank and whose EW[blank] is non-zero."""
    case = _bf16_case(5, 37, 64, 96, 33, seed=537, blank_bias=2.0)
    assert float(case["EW"][32].abs().max()) > 0
    for ms in (1, 3):
        for mode, act_bf16 in ((None, False), ("gemv", False), ("mfma", True)):
            res = R.decode_reference(case, ms, mode)
            assert [r["hyp"] for r in res] == _bf16_decode_torch(case, ms, act_bf16=act_bf16), (ms, mode)
            assert sum(r["counts"]["first_blank"] for r in res) >= 1
    # feeding the SOS row instead changes the hypotheses: the restart is visible in this case
    sos = dict(case); sos["EW"] = case["EW"].clone(); sos["EW"][32] = case["EW"][33]
    assert [r["hyp"] for r in R.decode_reference(sos, 3, None)] != [r["hyp"] for r in R.decode_reference(case, 3, None)]


def test_lengths_are_clamped_and_a_cap_truncates():
    name = "lens"
    B, T, Hp, Hj, V, ms = G.CASES[name][:6]
    res = R.decode_reference(G.make_case(name), ms, "gemv")
    assert res[1]["hyp"] == [] and res[2]["hyp"] == [] and res[1]["steps"] == [] and res[2]["steps"] == []
    assert max(s["frame"] for s in res[3]["steps"]) == T - 1
    full = R.decode_reference(G.make_case("small"), 3, "mfma")
    n = max(len(r["hyp"]) for r in full)
    capped = R.decode_reference(G.make_case("small"), 3, "mfma", cap=n - 1)
    for a, b in zip(full, capped):
        assert b["hyp"] == a["hyp"][:n - 1] and b["counts"]["overflow"] == (len(a["hyp"]) > n - 1)


@pytest.mark.parametrize("name", list(G.CASES))
def test_conditions_hold_for_every_case_of_the_gpu_file(name):
    """The allowance is not vacuous: (almost) no step has a second candidate, every acceptable set is a single sequence, and blanks,
    labels, first blanks, in-tile emissions and frames at the cap all occur."""
    B, T, Hp, Hj, V, ms, bias, lens, kind = G.CASES[name]
    case = G.make_case(name)
    for mode in ("mfma", "gemv"):
        res = R.decode_reference(case, ms, mode)
        s = G.check_case_conditions(res, kind)
        print(name, mode, s)
        assert s["set_max"] == 1 and s["multi"] == 0          # as chosen: the kernels are held to the fp64 hypothesis itself
        if kind != "extreme" and name != "one-frame":
            assert s["margin_min"] > 1e-4 and s["tol_median"] < 1e-5
    if name in G.ROUNDING_VISIBLE:
        assert [r["hyp"] for r in R.decode_reference(case, ms, "mfma")] != [r["hyp"] for r in R.decode_reference(case, ms, "gemv")]
    if name in G.TIES:                             # the blank-tied construction's reference: never blank
        never = dict(case); never["bh"] = case["bh"].clone(); never["bh"][V - 1] = -50.0
        never["Wh"] = case["Wh"].clone(); never["Wh"][V - 1] = case["Wh"][0]
        for mode in ("mfma", "gemv"):
            res = R.decode_reference(never, ms, mode)
            R.check_conditions(res, balanced=False)
            assert all(len(r["hyp"]) == ms * int(l) for r, l in zip(res, case["lens"]))


def test_the_old_allowance_tests_cases_have_single_sequence_sets():
    """tests/test_greedy_decode_gpu.py::test_bf16_decode_mfma_head_and_clusters now asserts membership on its own four cases."""
    for B, T, Hp, Hj, V, bias, ms in [(11, 45, 640, 640, 257, 3.0, 10), (5, 37, 64, 96, 33, 0.8, 3), (3, 20, 128, 64, 17, 50.0, 10),
                                      (4, 18, 64, 64, 40, -50.0, 2)]:
        case = _bf16_case(B, T, Hp, Hj, V, seed=B * 100 + T, blank_bias=bias)
        for mode in ("mfma", "gemv"):
            s = R.check_conditions(R.decode_reference(case, ms, mode), balanced=False)
            assert s["set_max"] == 1, (B, mode, s)


@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_conditions_hold_for_the_model_level_cases(compute_dtype):
    m = G.make_model(compute_dtype)
    enc, lens = G.model_inputs()
    case = R.case_from_model(m, enc, lens, 'hi')
    assert case["bf16"] == (compute_dtype == "bf16")
    if case["bf16"]:
        assert case["Wh"].dtype == torch.bfloat16 and case["Whh"].dtype == torch.bfloat16 and case["Wp"].dtype == torch.bfloat16
    # the operands as greedy_rnnt_decode_device lays them out: labels, the blank / padding row, the zero-input SOS row
    lstm = m.decoder.prediction["dec_rnn"].lstm
    emb = m.decoder.prediction["embed"].weight
    b = (lstm.bias_ih_l0 + lstm.bias_hh_l0).double()
    assert torch.allclose(case["EW"][17], b, atol=0, rtol=0)
    assert torch.allclose(case["EW"][16], lstm.weight_ih_l0.double() @ emb[m.decoder.blank_idx].double() + b, atol=1e-12)
    assert float((case["EW"][16] - case["EW"][17]).abs().max()) > 0.1
    assert float((case["f_all32"].double() - case["f_all"]).abs().max()) > 0          # e_pre sees the set-up GEMMs' fp32 error
    res = R.decode_reference(case, G.MODEL_MS, G.model_rounding(case))
    s = G.check_case_conditions(res, "balanced")
    print(compute_dtype, s)
    assert s["set_max"] == 1
    enc4, lens4 = G.model_inputs(B=4, seed=6)
    for i, lang in enumerate(['hi', 'ta', 'ta', 'hi']):
        c = R.case_from_model(m, enc4[i:i + 1], lens4[i:i + 1], lang)
        r = R.decode_reference(c, G.MODEL_MS, G.model_rounding(c))
        assert len(r[0]["accept"]) == 1 and r[0]["counts"]["multi"] == 0


def _two_label_case(delta):
    """One utterance, two frames, labels 0 and 1 + blank, one symbol per frame.  Only label 0's head row reads anything: the first
    activation, which f pins (W_pred's first row and bias are zero) at 1 in frame 0 and at 2 in frame 1 -- both bf16 values, every
    product exact in fp32.  z_0 = x_t - 1 + delta, z_1 = 0, blank at -5: label 0 leads by `delta` in frame 0 and by 1 in frame 1."""
    g = torch.Generator().manual_seed(11)
    Hp, Hj, V, T = 8, 8, 3, 2
    f_all = torch.zeros(1, T, Hj); f_all[0, 0, 0] = 1.0; f_all[0, 1, 0] = 2.0
    Wp = torch.randn(Hj, Hp, generator=g).bfloat16(); Wp[0] = 0
    bp = torch.randn(Hj, generator=g) * 0.1; bp[0] = 0
    Wh = torch.zeros(V, Hj).bfloat16(); Wh[0, 0] = 1.0
    bh = torch.tensor([-1.0, 0.0, -5.0], dtype=torch.float64); bh[0] += delta
    return dict(f_all=f_all, EW=torch.randn(V + 1, 4 * Hp, generator=g), Whh=(torch.randn(4 * Hp, Hp, generator=g) * 0.3).bfloat16(),
                Wp=Wp, bp=bp, Wh=Wh, bh=bh.float(), lens=torch.tensor([T]))


@pytest.mark.parametrize("mode", ["gemv", "mfma"])
def test_a_margin_below_tol_branches_into_exactly_the_two_continuations(mode):
    wide = R.decode_reference(_two_label_case(1e-3), 1, mode)[0]
    assert wide["accept"] == {(0, 0)} and wide["counts"]["multi"] == 0
    tol = wide["steps"][0]["tol"]
    assert R.FLOOR * 5 <= tol < 2 * R.FLOOR * 5                               # the head is exact here: the relative floor alone
    near = R.decode_reference(_two_label_case(tol / 2), 1, mode)[0]
    assert near["steps"][0]["margin"] < near["steps"][0]["tol"] and near["steps"][1]["margin"] > 0.9
    assert [s["candidates"] for s in near["steps"]] == [[0, 1], [0]]
    assert near["hyp"] == [0, 0] and near["accept"] == {(0, 0), (1, 0)}       # the two continuations, and they differ
    assert near["counts"]["multi"] == 1
    exact = R.decode_reference(_two_label_case(tol / 2), 1, None)[0]          # no tolerance, no branch
    assert exact["accept"] == {(0, 0)}
    # an exact tie is a pair of candidates as well, whichever index comes first
    tie = R.decode_reference(_two_label_case(0.0), 1, mode)[0]
    assert tie["hyp"] == [0, 0] and tie["accept"] == {(0, 0), (1, 0)}


@pytest.mark.parametrize("mode", ["gemv", "mfma"])
def test_a_perturbation_of_twice_tol_leaves_the_acceptable_set(mode):
    """To the runner-up of an utterance's first decision, add what it lacks plus twice the step's tol -- and a hundredth more, because
    a lead of exactly the two labels' tolerances together still leaves the old label a candidate (the rule's >=): the main path
    changes and the old hypothesis is no longer acceptable.  The same amount short of the lead, nothing changes."""
    name = "small"
    ms = G.CASES[name][5]
    case = G.make_case(name)
    res = R.decode_reference(case, ms, mode)
    moved = 0
    for b in range(len(res)):
        step = res[b]["steps"][0]
        one = {k: (v[b:b + 1] if k in ("f_all", "lens") else v) for k, v in case.items()}
        assert R.decode_reference(one, ms, mode)[0]["hyp"] == res[b]["hyp"]
        for sign, same in ((+1, False), (-1, True)):
            pert = dict(one); pert["bh"] = case["bh"].double().clone()
            pert["bh"][step["second"]] += step["margin"] + sign * 2.01 * step["tol"]
            got = R.decode_reference(pert, ms, mode)[0]
            assert (got["steps"][0]["choice"] == step["choice"]) == same, (b, sign, step)
            if not same:
                assert got["steps"][0]["choice"] == step["second"]
                assert got["hyp"] != res[b]["hyp"] and tuple(res[b]["hyp"]) not in got["accept"], (b, step)
                moved += 1
    assert moved == len(res)
