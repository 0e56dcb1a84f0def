"""Transducer beam search (alignment-length synchronous decoding) on the host: decoding.beam_rnnt_alsd_host against the lists
NeMo's own routine returned (tests/golden/rnnt_alsd_cases.npz, written by tests/golden/make_rnnt_alsd_golden.py), its edge
cases, the strategy's surface on the model, and the conditions of the GPU cases on the reference alone."""
import ctypes
import math
import os
import types

import numpy as np
import pytest
import torch

import rnnt_beam_cases as C
from indic_cl_asr_amd import decoding as D


# ---------------------------------------------------------------------------------------------------- the reference's lists
@pytest.fixture(scope="module")
def golden(golden_dir):
    z = np.load(os.path.join(golden_dir, "rnnt_alsd_cases.npz"))
    cases = []
    for c in range(int(z["n_cases"])):
        case = {k: torch.from_numpy(z[f"c{c}_{k}"]) for k in ("f_all", "EW", "Whh", "Wp", "bp", "Wh", "bh", "lens")}
        want = []
        for u in range(case["f_all"].shape[0]):
            ln = z[f"c{c}_u{u}_len"].tolist()
            off = np.concatenate([[0], np.cumsum(ln)]).tolist()
            tok, ts, sc = z[f"c{c}_u{u}_tok"].tolist(), z[f"c{c}_u{u}_ts"].tolist(), z[f"c{c}_u{u}_score"].tolist()
            want.append([(tok[a:b], s, ts[a:b]) for a, b, s in zip(off, off[1:], sc)])
        cases.append((case, int(z[f"c{c}_W"]), want))
    return cases


def test_host_routine_reproduces_the_reference_lists(golden):
    recomb, longer, empty, fin_recomb = 0, 0, 0, 0
    for case, W, want in golden:
        got = D.beam_rnnt_alsd_host(case, W)
        for g, w in zip(got, want):
            assert len(g["hyps"]) == len(w)
            assert [h[0] for h in g["hyps"]] == [h[0] for h in w] and [h[2] for h in g["hyps"]] == [h[2] for h in w]
            assert all(abs(a[1] - b[1]) <= 1e-9 for a, b in zip(g["hyps"], w))
            recomb += g["recombinations"]; fin_recomb += g["finished_recombined"]
            longer += g["n_finished"] > W; empty += g["n_finished"] == 0
    assert recomb >= 10 and longer >= 1 and empty >= 1 and fin_recomb >= 1      # what the fixture was chosen to hold


def test_a_finished_score_carries_the_recombination_of_its_own_step(golden):
    """The last case of the fixture: a blank candidate enters the finished list and, in the same step's walk over the new beam,
    receives a duplicate's score.  The reference's list shows the merged score; without the merge the score differs."""
    case, W, want = golden[-1]
    got = D.beam_rnnt_alsd_host(case, W)[0]
    assert got["finished_recombined"] >= 1 and got["n_finished"] == len(want[0])
    assert all(abs(a[1] - b[1]) <= 1e-9 for a, b in zip(got["hyps"], want[0]))


# ---------------------------------------------------------------------------------------------------- edge cases
def _small(lens, seed=5, bias=3.0, T=10, V=9):
    from test_greedy_decode_gpu import _bf16_case
    c = _bf16_case(len(lens), T, 16, 16, V, seed, bias, torch.tensor(lens))
    return {k: (v.float() if v.dtype == torch.bfloat16 else v) for k, v in c.items()}


def test_lengths_are_clamped_and_short_utterances_end_at_once():
    c = _small([10, 0, -3, 25, 1])
    out = D.beam_rnnt_alsd_host(c, 3)
    assert out[1]["hyps"] == [([], 0.0, [])] and out[2]["hyps"] == [([], 0.0, [])] and out[1]["n_finished"] == 0
    assert out[3]["hyps"] == D.beam_rnnt_alsd_host(dict(c, lens=torch.tensor([10] * 5)), 3)[3]["hyps"]
    one = out[4]                                      # len 1, u_max 1: two steps
    assert one["steps"] <= 2 and all(len(h[0]) <= 1 and all(s in (0, 1) for s in h[2]) for h in one["hyps"])
    assert one["n_finished"] >= 1 and [] in [h[0] for h in one["hyps"]]


def test_u_max_from_a_float_and_from_an_int():
    assert D.alsd_u_max(1.0, 7) == 7 and D.alsd_u_max(0.5, 7) == 3 and D.alsd_u_max(3, 7) == 3 and D.alsd_u_max(0, 7) == 0
    assert D.alsd_u_max(0.0, 7) == 0
    c = _small([10, 8])
    for a, cap in ((0.5, lambda n: n // 2), (3, lambda n: 3), (0, lambda n: 0), (1.0, lambda n: n)):
        for r, n in zip(D.beam_rnnt_alsd_host(c, 3, a), (10, 8)):
            assert r["steps"] <= n + cap(n)
            assert all(len(h[0]) <= cap(n) for h in r["hyps"]) or r["n_finished"] == 0
            assert all(len(h[0]) <= n + cap(n) and all(s < n + cap(n) for s in h[2]) for h in r["hyps"])
    zero = D.beam_rnnt_alsd_host(c, 3, 0)
    assert all(r["steps"] == n for r, n in zip(zero, (10, 8)))


def test_width_one_and_score_norm_off():
    c = _small([10, 7], bias=6.0)
    assert all(r["n_finished"] > 4 for r in D.beam_rnnt_alsd_host(c, 4))
    for r in D.beam_rnnt_alsd_host(_small([10, 7], bias=8.0), 1):
        assert r["recombinations"] == 0 and r["n_finished"] >= 1
        assert all(len(h[0]) == len(h[2]) for h in r["hyps"])
    on, off = D.beam_rnnt_alsd_host(c, 4), D.beam_rnnt_alsd_host(c, 4, score_norm=False)
    for a, b in zip(on, off):
        assert sorted(h[1] for h in a["hyps"]) == sorted(h[1] for h in b["hyps"])          # the same list, ranked differently
        assert [h[1] for h in b["hyps"]] == sorted((h[1] for h in b["hyps"]), reverse=True)
        key = [h[1] / (len(h[0]) + 1) for h in a["hyps"]]
        assert key == sorted(key, reverse=True)
    assert any([h[0] for h in a["hyps"]] != [h[0] for h in b["hyps"]] for a, b in zip(on, off))
    assert [len(r["hyps"]) for r in D.beam_rnnt_alsd_host(c, 4, n_best=2)] == [2, 2]
    with pytest.raises(ValueError, match="cannot be less than 1"):
        D.beam_rnnt_alsd_host(c, 0)


def test_an_exact_tie_between_label_rows_goes_to_the_smaller_id():
    """Rows 3 and 6 of the head are copies of row 1 and the three dominate (as the `tie8` cases of the CTC search): every row's
    best labels are an exact three-way tie, of which the rule admits the smaller ids."""
    c = _small([10], bias=-50.0)                      # never blank: every step extends
    for k in (3, 6):
        c["Wh"][k] = c["Wh"][1]
    c["bh"][1] = c["bh"][3] = c["bh"][6] = 8.0
    for rounding in (None, "gemv"):
        one = D.beam_rnnt_alsd_host(c, 1, 0, rounding=rounding)[0]
        assert one["hyps"][0][0] == [1] * 10 and one["n_finished"] == 0
        two = D.beam_rnnt_alsd_host(c, 2, 0, rounding=rounding)[0]
        assert len(two["hyps"]) == 2 and all(set(h[0]) <= {1, 3} and len(h[0]) == 10 for h in two["hyps"])
        assert two["hyps"][0][0][0] == 1 or two["hyps"][1][0][0] == 1
        assert two["decided"] or rounding is None or all(kind != "labels" for _, kind in two["undecided"])


# ---------------------------------------------------------------------------------------------------- the GPU cases' conditions
@pytest.mark.parametrize("weights", ["bf16", "fp32"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_gpu_cases_meet_their_conditions_on_the_reference(name, weights):
    ref = C.reference(name, weights)
    f = C.check_conditions(name, ref)
    print(name, weights, f)
    B, T, W, a = C.CASES[name][0], C.CASES[name][1], C.CASES[name][5], C.CASES[name][9]
    lens = C.operands(name)["lens"].clamp(0, T).tolist()
    if name == "all_blank":
        assert all(r["hyps"][0][0] == [] for r in ref)
    if name == "never_blank":
        assert all(r["n_finished"] == 0 and all(len(h[0]) == n + D.alsd_u_max(a, n) for h in r["hyps"]) for r, n in zip(ref, lens))
    exact = D.beam_rnnt_alsd_host(C.case_for(name, "fp32"), W, a) if name in ("w4", "clamped") else None
    if exact is not None:                             # the rounding modes change scores by no more than their slack
        gemv = C.reference(name, "fp32")
        for e, g in zip(exact, gemv):
            if g["decided"]:
                assert [h[0] for h in e["hyps"]] == [h[0] for h in g["hyps"]]
                assert all(abs(x[1] - y[1]) <= 1e-12 for x, y in zip(e["hyps"], g["hyps"]))


# ---------------------------------------------------------------------------------------------------- the model's surface
@pytest.fixture(scope="module")
def model():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(3)
    return EncDecHybridRNNTCTCModel(model_config("tiny"))


def test_change_decoding_strategy_accepts_alsd(model):
    m = model
    try:
        m.change_decoding_strategy({"strategy": "alsd", "beam": {"beam_size": 4}})
        assert m.cur_decoder == "rnnt" and m.decoding_strategy["rnnt"] == dict(
            strategy="alsd", max_symbols=10, beam_size=4, return_best_hypothesis=True, score_norm=True, alsd_max_target_len=1.0)
        m.change_decoding_strategy({"strategy": "alsd", "beam": {"return_best_hypothesis": False, "score_norm": False,
                                                               "alsd_max_target_len": 2}}, decoder_type="rnnt")
        assert m.decoding_strategy["rnnt"] == dict(strategy="alsd", max_symbols=10, beam_size=4, return_best_hypothesis=False,
                                                   score_norm=False, alsd_max_target_len=2)
        m.change_decoding_strategy()                                                       # None: the configuration set before
        assert m.decoding_strategy["rnnt"]["beam_size"] == 4 and m.decoding_strategy["rnnt"]["alsd_max_target_len"] == 2
        cfg = types.SimpleNamespace(strategy="alsd", beam=types.SimpleNamespace(beam_size=1, softmax_temperature=1.0))
        m.change_decoding_strategy(cfg)
        assert m.decoding_strategy["rnnt"]["beam_size"] == 1
        m.change_decoding_strategy({"strategy": "greedy", "greedy": {"max_symbols": 5}})
        assert m.decoding_strategy["rnnt"] == dict(strategy="greedy", max_symbols=5)
        with pytest.raises(NotImplementedError, match="beam_size"):                        # greedy in between: nothing is remembered
            m.change_decoding_strategy({"strategy": "alsd"})
    finally:
        m.decoding_strategy = {}
        m.cur_decoder = "rnnt"


def test_change_decoding_strategy_refuses_what_alsd_does_not_do(model):
    m = model
    m.change_decoding_strategy({"strategy": "alsd", "beam": {"beam_size": 3}})
    before = (m.cur_decoder, {k: dict(v) for k, v in m.decoding_strategy.items()})
    alsd = lambda top=None, **kw: dict({"strategy": "alsd", "beam": dict({"beam_size": 2}, **kw)}, **(top or {}))
    try:
        for st in ("beam", "tsd", "maes"):
            with pytest.raises(NotImplementedError, match=st):
                m.change_decoding_strategy({"strategy": st, "beam": {"beam_size": 2}})
        for key in ("preserve_alignments", "compute_timestamps", "ngram_lm_model", "language_model"):
            with pytest.raises(NotImplementedError, match=key):
                m.change_decoding_strategy(alsd(**{key: True}))
        for key in ("preserve_alignments", "compute_timestamps"):
            with pytest.raises(NotImplementedError, match=key):
                m.change_decoding_strategy(alsd(top={key: True}))
        with pytest.raises(NotImplementedError, match="softmax_temperature"):
            m.change_decoding_strategy(alsd(softmax_temperature=0.5))
        with pytest.raises(ValueError, match="cannot be less than 1"):
            m.change_decoding_strategy(alsd(beam_size=0))
        with pytest.raises(ValueError, match="alsd_max_target_len"):
            m.change_decoding_strategy(alsd(alsd_max_target_len=-1.0))
        with pytest.raises(ValueError, match="Decoding strategy must be one of"):
            m.change_decoding_strategy({"strategy": "viterbi"})
        assert (m.cur_decoder, m.decoding_strategy) == before                              # a refusal changes nothing
        m.decoding_strategy = {}
        with pytest.raises(NotImplementedError, match="alsd"):                             # NeMo's config has no default beam_size
            m.change_decoding_strategy({"strategy": "alsd"})
        with pytest.raises(NotImplementedError, match="beam_size"):
            m.change_decoding_strategy({"strategy": "alsd", "beam": {"score_norm": False}})
        assert m.decoding_strategy == {}
    finally:
        m.decoding_strategy = {}
        m.cur_decoder = "rnnt"


def test_transcribe_on_the_host_follows_the_strategy(model):
    """transcribe's side of the strategy on CPU tensors (the float64 host routine): greedy before and after, hypotheses in
    between; `forward` is stood in for by seeded encoder outputs, as tests/test_ctc_beam.py does."""
    from oracle import decode_ref as R
    m = model.eval()
    g = torch.Generator().manual_seed(4)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (9000, 6000)]
    enc = torch.randn(2, m.cfg.d_model, 14, generator=g) * 4
    lens = torch.tensor([14, 9])
    monkey = pytest.MonkeyPatch()
    monkey.setattr(m, "forward", lambda input_signal=None, input_signal_length=None, **kw: (enc, lens), raising=False)
    try:
        greedy = m.transcribe(audio, language_id="hi", batch_size=2, return_hypotheses=True)
        assert all(isinstance(s, str) for s in greedy[0])
        m.change_decoding_strategy({"strategy": "alsd", "beam": {"beam_size": 3, "return_best_hypothesis": False}})
        best, nbest = m.transcribe(audio, language_id="hi", batch_size=2, return_hypotheses=True)
        strings = m.transcribe(audio, language_id="hi", batch_size=2)
        case = R.case_from_model(m, enc, lens, "hi")
        case = dict(case, f_all=case["f_all32"].double(), EW=case["EW32"].double())        # the operands the model multiplies with
        want = D.beam_rnnt_alsd_host(case, 3, n_best=3)
        for b in range(2):
            hs = nbest[b].n_best_hypotheses
            assert isinstance(nbest[b], D.NBestHypotheses) and nbest[b].n_finished == want[b]["n_finished"] and best[b] is hs[0]
            assert [(h.y_sequence, h.timestep) for h in hs] == [(w[0], w[2]) for w in want[b]["hyps"]]
            assert all(math.isclose(h.score, w[1], rel_tol=1e-5, abs_tol=1e-5) for h, w in zip(hs, want[b]["hyps"]))
            assert all(h.text == " ".join(str(i) for i in h.y_sequence) for h in hs)
        assert strings[0] == [h.text for h in best] and strings[1] == strings[0]
        m.change_decoding_strategy({"strategy": "alsd", "beam": {"return_best_hypothesis": True}})
        one, every = m.transcribe(audio, language_id="hi", batch_size=2, return_hypotheses=True)
        assert all(isinstance(h, D.Hypothesis) for h in one) and every == one
        assert [h.y_sequence for h in one] == [h.y_sequence for h in best]
        m.change_decoding_strategy({"strategy": "greedy_batch"})
        assert m.transcribe(audio, language_id="hi", batch_size=2, return_hypotheses=True) == greedy
    finally:
        monkey.undo()
        m.decoding_strategy = {}
        m.cur_decoder = "rnnt"


# ---------------------------------------------------------------------------------------------------- the C entries
def check_entry_point_refusals():
    """Every call below is refused before any device work: the pointers are never dereferenced."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    assert L.ia_rnnt_beam_max_width() == 16
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(15)]
    B, T, Hp, Hj, V, W = 2, 10, 64, 64, 17, 4
    need = L.ia_rnnt_beam_workspace_bytes(B, T, Hp, Hj, V, W, T)
    assert need > 0 and need % 256 == 0 and need >= B * 33 * (2 * Hp + Hj) * 4
    assert L.ia_rnnt_beam_workspace_bytes(B, T, Hp, Hj, V, 17, T) == 0 and L.ia_rnnt_beam_workspace_bytes(0, T, Hp, Hj, V, W, T) == 0
    assert L.ia_rnnt_beam_workspace_bytes(B, T, Hp, Hj, V, 0, T) == 0 and L.ia_rnnt_beam_workspace_bytes(B, T, Hp, Hj, V, W, -1) == 0
    assert L.ia_rnnt_beam_workspace_bytes(32, 375, 640, 640, 257, 16, 375) > 0

    def call(fn=L.ia_rnnt_beam_alsd_bf16w, ptrs=None, Hp=Hp, Hj=Hj, V=V, W=W, K=W, nbytes=need):
        q = p if ptrs is None else ptrs
        return fn(*q[:9], B, T, Hp, Hj, V, W, K, T, 1, *q[9:15], nbytes, None)

    for fn in (L.ia_rnnt_beam_alsd_bf16w, L.ia_rnnt_beam_alsd):
        for i in range(15):
            q = list(p); q[i] = None
            assert call(fn, q) == -1, i                                                  # IA_INVALID_VALUE: null pointers
        for i in (0, 3, 4, 5, 7):
            q = list(p); q[i] = ctypes.c_void_p(4096 * (i + 1) + 4)
            assert call(fn, q) == -1, i                                                  # 16-byte operands
        q = list(p); q[14] = ctypes.c_void_p(4096 * 15 + 128)
        assert call(fn, q) == -1                                                         # the workspace: 256 bytes
        assert call(fn, W=0) == -1 and call(fn, K=0) == -1 and call(fn, V=1) == -1
        assert call(fn, W=17, K=16) == -4 and call(fn, K=17) == -4                       # IA_UNSUPPORTED
        assert call(fn, Hp=50) == -4 and call(fn, Hj=62) == -4
        assert call(fn, V=40000) == -4                                                   # the logits no longer fit the LDS
        assert call(fn, nbytes=need - 1) == -2 and call(fn, nbytes=0) == -2              # IA_WORKSPACE_TOO_SMALL
        assert call(fn, W=17, K=16, nbytes=0) == -4 and call(fn, W=0, Hp=50) == -1       # the order of the checks
    assert call(L.ia_rnnt_beam_alsd_bf16w, Hp=48) == -4 and call(L.ia_rnnt_beam_alsd_bf16w, Hj=40) == -4   # bf16: multiples of 32


def test_entry_points_refuse_bad_arguments_before_device_work():
    check_entry_point_refusals()
