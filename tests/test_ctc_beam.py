"""CTC prefix beam search, host side: the float64 host routine of indic_cl_asr_amd/decoding.py against known answers, against
the exact CTC likelihood where the beam holds every prefix, against the numpy restatement tests/ctc_beam_ref.py (E); the
parsing and refusals of model.change_decoding_strategy; the C entries' argument checks.  No device."""
import ctypes
import math
import types
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctc_beam_ref as R
from indic_cl_asr_amd import decoding as D

INF = float("inf")


def _logp(rows):
    return torch.tensor(rows, dtype=torch.float64).log()


# ---------------------------------------------------------------------------------------------------- known answers
def test_two_frames_where_the_sum_over_alignments_beats_the_best_path():
    """[a: 0.4, blank: 0.6] twice: the best path is blank blank (0.36), the labelling `a` owns a-, -a and aa (0.64)."""
    lp = _logp([[[0.4, 0.6], [0.4, 0.6]]])
    lens = torch.tensor([2])
    assert D.greedy_ctc_decode(lp, lens) == [[]]
    best = D.beam_ctc_decode(lp, lens, beam_size=2)[0]
    assert isinstance(best, D.Hypothesis) and best.y_sequence == [0] and best.score == pytest.approx(math.log(0.64), abs=1e-12)
    nbest = D.beam_ctc_decode(lp, lens, beam_size=2, return_best_hypothesis=False)[0]
    assert isinstance(nbest, D.NBestHypotheses)
    assert [h.y_sequence for h in nbest.n_best_hypotheses] == [[0], []]
    assert nbest.n_best_hypotheses[1].score == pytest.approx(math.log(0.36), abs=1e-12)
    # beam_size 1 keeps `a` after the first frame only if it leads there: it does not (0.4 < 0.6), so the answer is greedy's
    assert D.beam_ctc_decode(lp, lens, beam_size=1)[0].y_sequence == []


def test_a_repeated_label_needs_a_blank_between():
    """`a a` over frames a, blank, a is their product; without the blank frame no alignment collapses to it."""
    rows = [[0.7, 0.2, 0.1], [0.1, 0.1, 0.8], [0.6, 0.3, 0.1]]
    lp = _logp([rows])
    hyps = {tuple(y): s for y, s in D.beam_ctc_search_host(lp, torch.tensor([3]), beam_size=32)[0]}
    assert hyps[(0, 0)] == pytest.approx(math.log(0.7 * 0.8 * 0.6), abs=1e-12)
    assert hyps[(0, 0, 0)] == -INF                                       # would need five frames
    two = {tuple(y): s for y, s in D.beam_ctc_search_host(lp, torch.tensor([2]), beam_size=32)[0]}
    assert two[(0, 0)] == -INF and two[(0,)] == pytest.approx(math.log(0.7 * 0.1 + 0.7 * 0.8 + 0.1 * 0.1), abs=1e-12)
    assert D.beam_ctc_search_host(lp, torch.tensor([0]), beam_size=4)[0] == [([], 0.0)]


# ---------------------------------------------------------------------------------------------------- exhaustive
def test_a_beam_that_holds_every_prefix_returns_the_ctc_likelihoods():
    """V = 3, T = 4, W = 32: nothing is ever pruned, so the 31 prefixes over two labels all arrive and each score is the
    exact log-likelihood of its labelling (-F.ctc_loss in float64; -inf for a labelling four frames cannot spell)."""
    g = torch.Generator().manual_seed(5)
    lp = (torch.randn(2, 4, 3, generator=g, dtype=torch.float64) * 2).log_softmax(-1)
    out = D.beam_ctc_search_host(lp, torch.tensor([4, 4]), beam_size=32)
    for b in range(2):
        assert len(out[b]) == 31 and len({tuple(y) for y, _ in out[b]}) == 31
        assert [s for _, s in out[b]] == sorted((s for _, s in out[b]), reverse=True)
        for y, s in out[b]:
            tg = torch.tensor([y], dtype=torch.long).reshape(1, len(y))
            nll = F.ctc_loss(lp[b].unsqueeze(1), tg, torch.tensor([4]), torch.tensor([len(y)]), blank=2, reduction="none")
            want = -float(nll)
            assert (s == want) if want == -INF else abs(s - want) <= 1e-9, (y, s, want)
            assert s == pytest.approx(R.ctc_log_likelihood(lp[b].numpy(), y, 2), abs=1e-9) or s == want == -INF


# ---------------------------------------------------------------------------------------------------- against E
@pytest.mark.parametrize("V,W,logits", [(5, 1, True), (5, 3, False), (17, 4, True), (17, 16, False), (33, 8, True), (40, 32, False)])
def test_host_routine_equals_the_restatement(V, W, logits):
    g = torch.Generator().manual_seed(V * 100 + W)
    B, T = 4, 24
    x = torch.randn(B, T, V, generator=g) * 3
    x[..., V - 1] += 3
    lse = torch.logsumexp(x, -1) if logits else None
    if not logits:
        x = x.log_softmax(-1)
    lens = torch.tensor([T, 0, 1, T - 5])
    got = D.beam_ctc_search_host(x, lens, beam_size=W, lse=lse)
    for b in range(B):
        n = int(lens[b])
        e, gap = R.E(x[b, :n].numpy(), W, lse=None if lse is None else lse[b, :n].numpy())
        assert len(got[b]) == len(e)
        assert max(abs(a[1] - c[1]) for a, c in zip(e, got[b])) <= 1e-9
        if gap > 1e-9:
            assert [y for y, _ in got[b]] == [y for y, _ in e]
    assert got[1] == [([], 0.0)]


REENTRY = [[0.0097, 0.2233, 0.767], [0.8155, 0.0194, 0.165], [0.3883, 0.466, 0.1456], [0.8932, 0.0194, 0.0874],
           [0.4466, 0.4369, 0.1165], [0.2427, 0.6019, 0.1553]]


def test_a_prefix_that_left_the_beam_and_came_back_merges_with_its_child():
    """W = 3 over labels a, b: `a b` is in the beam after frame 2, gone after frame 3 while its child `a b a` stays, and back
    after frame 4 as the extension of `a`.  In frame 5 the extension `a b` + a denotes the member `a b a`: one candidate.  An
    implementation that knows prefixes by (parent slot, token) keeps two copies of `a b a` and returns `a` as third
    hypothesis instead."""
    lp = _logp([REENTRY])
    trace = []
    e, gap = R.E(lp[0].numpy(), 3, trace=trace)
    assert (0, 1) in trace[2] and (0, 1) not in trace[3] and (0, 1) in trace[4]          # the case is what it claims to be
    assert all((0, 1, 0) in trace[t] for t in (3, 4, 5)) and gap > 1e-3
    got = D.beam_ctc_search_host(lp, torch.tensor([6]), beam_size=3)[0]
    assert [y for y, _ in got] == [y for y, _ in e] == [[0, 1], [0, 1, 0, 1], [0, 1, 0]]
    assert max(abs(a[1] - c[1]) for a, c in zip(e, got)) <= 1e-12
    assert got[2][1] == pytest.approx(R.ctc_log_likelihood(lp[0].numpy(), [0, 1, 0], 2), abs=0.2)
    assert got[2][1] <= R.ctc_log_likelihood(lp[0].numpy(), [0, 1, 0], 2) + 1e-12


def test_token_min_logp_prunes_extensions_only():
    g = torch.Generator().manual_seed(9)
    x = (torch.randn(3, 16, 9, generator=g) * 2).log_softmax(-1)
    lens = torch.tensor([16, 9, 16])
    floor = math.log(0.08)
    got = D.beam_ctc_search_host(x, lens, beam_size=4, token_min_logp=floor)
    off = D.beam_ctc_search_host(x, lens, beam_size=4)
    assert D.beam_ctc_search_host(x, lens, beam_size=4, token_min_logp=-INF) == off
    for b in range(3):
        e, _ = R.E(x[b, :int(lens[b])].numpy(), 4, token_min_logp=floor)
        assert [y for y, _ in got[b]] == [y for y, _ in e]
        assert max(abs(a[1] - c[1]) for a, c in zip(e, got[b])) <= 1e-9
    assert any(g_ != o for g_, o in zip(got, off))
    # a floor above every token: only stays remain, the one hypothesis is the empty one with the blank path's probability
    lone = D.beam_ctc_search_host(x, lens, beam_size=4, token_min_logp=1.0)
    for b in range(3):
        n = int(lens[b])
        assert len(lone[b]) == 1 and lone[b][0][0] == []
        assert lone[b][0][1] == pytest.approx(float(x[b, :n, 8].double().sum()), abs=1e-9)


def test_decode_wrapper_checks_its_arguments():
    x = torch.zeros(1, 3, 4).log_softmax(-1)
    with pytest.raises(ValueError, match="cannot be less than 1"):
        D.beam_ctc_decode(x, torch.tensor([3]), beam_size=0)
    with pytest.raises(ValueError, match="blank"):
        D.beam_ctc_decode(x, torch.tensor([3]), blank=4)
    with pytest.raises(ValueError, match="B,T,V"):
        D.beam_ctc_decode(x[0], torch.tensor([3]))
    h = D.beam_ctc_decode(x, torch.tensor([9]), beam_size=2, blank=0)[0]               # a length beyond T is clamped
    assert h.text is None and h.score <= 0 and all(1 <= c <= 3 for c in h.y_sequence)


# ---------------------------------------------------------------------------------------------------- change_decoding_strategy
@pytest.fixture(scope="module")
def model():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(3)
    return EncDecHybridRNNTCTCModel(model_config("tiny"))


def test_change_decoding_strategy_parses_mappings_and_objects(model):
    m = model
    assert m.cur_decoder == "rnnt" and m.decoding_strategy == {}
    m.change_decoding_strategy(decoder_type="ctc")
    assert m.cur_decoder == "ctc" and m.decoding_strategy["ctc"] == {"strategy": "greedy"}
    m.change_decoding_strategy({"strategy": "beam", "beam": {"beam_size": 8, "return_best_hypothesis": False, "search_type": "nemo",
                                                           "beam_alpha": 0.5, "beam_beta": 1.5, "kenlm_path": None,
                                                           "token_min_logp": -5.0}}, decoder_type="ctc", lang_id="hi")
    assert m.decoding_strategy["ctc"] == dict(strategy="beam", beam_size=8, search_type="nemo", return_best_hypothesis=False,
                                              beam_alpha=0.5, beam_beta=1.5, token_min_logp=-5.0)
    m.change_decoding_strategy(decoder_type="ctc")                                     # None: the configuration set before
    assert m.decoding_strategy["ctc"]["beam_size"] == 8
    cfg = types.SimpleNamespace(strategy="beam", beam=types.SimpleNamespace(beam_size=2))
    m.change_decoding_strategy(cfg, "ctc")
    assert m.decoding_strategy["ctc"]["beam_size"] == 2 and m.decoding_strategy["ctc"]["search_type"] == "nemo"
    m.change_decoding_strategy({"strategy": "beam"}, "ctc")
    m.change_decoding_strategy({"strategy": "greedy"}, "ctc")
    assert m.decoding_strategy["ctc"] == {"strategy": "greedy"}
    m.change_decoding_strategy({"strategy": "beam"}, "ctc")                            # defaults after greedy
    assert m.decoding_strategy["ctc"] == dict(strategy="beam", beam_size=4, search_type="default", return_best_hypothesis=True,
                                              beam_alpha=1.0, beam_beta=0.0, token_min_logp=None)
    m.change_decoding_strategy({"strategy": "greedy", "greedy": {"max_symbols": 5}}, decoder_type="rnnt")
    assert m.cur_decoder == "rnnt" and m.decoding_strategy["rnnt"] == dict(strategy="greedy", max_symbols=5)
    m.change_decoding_strategy()                                                       # decoder_type None: the transducer
    assert m.cur_decoder == "rnnt" and m.decoding_strategy["rnnt"]["max_symbols"] == 5
    m.change_decoding_strategy({"strategy": "greedy_batch"})
    assert m.decoding_strategy["rnnt"]["strategy"] == "greedy_batch" and m.decoding_strategy["ctc"]["strategy"] == "beam"
    m.decoding_strategy = {}


def test_change_decoding_strategy_refusals(model):
    m = model
    before = (m.cur_decoder, dict(m.decoding_strategy))
    beam = lambda **kw: {"strategy": "beam", "beam": kw}
    with pytest.raises(NotImplementedError, match="kenlm_path"):
        m.change_decoding_strategy(beam(kenlm_path="lm.bin"), "ctc")
    for st in ("pyctcdecode", "flashlight"):
        with pytest.raises(NotImplementedError, match=st):
            m.change_decoding_strategy(beam(search_type=st), "ctc")
        with pytest.raises(NotImplementedError, match=st):
            m.change_decoding_strategy({"strategy": st}, "ctc")
    with pytest.raises(NotImplementedError, match="not supported"):
        m.change_decoding_strategy(beam(search_type="other"), "ctc")
    for cfg in ({"strategy": "beam", "compute_timestamps": True}, {"strategy": "beam", "preserve_alignments": True},
                beam(compute_timestamps=True), beam(preserve_alignments=True)):
        with pytest.raises(ValueError, match="Currently this flag is not supported for beam search algorithms"):
            m.change_decoding_strategy(cfg, "ctc")
    with pytest.raises(ValueError, match="Decoding strategy must be one of"):
        m.change_decoding_strategy({"strategy": "viterbi"}, "ctc")
    with pytest.raises(ValueError, match="cannot be less than 1"):
        m.change_decoding_strategy(beam(beam_size=0), "ctc")
    for st in ("beam", "tsd", "alsd", "maes"):
        with pytest.raises(NotImplementedError, match=st):
            m.change_decoding_strategy({"strategy": st}, "rnnt")
    with pytest.raises(ValueError, match="Decoding strategy must be one of"):
        m.change_decoding_strategy({"strategy": "viterbi"})
    with pytest.raises(ValueError, match="decoder_type=lm is not supported"):
        m.change_decoding_strategy(None, "lm")
    assert (m.cur_decoder, m.decoding_strategy) == before                              # a refusal changes nothing


def test_transcribe_on_the_host_follows_the_strategy(model):
    """transcribe's side of the strategy on CPU tensors (the float64 host routine): greedy before and after, hypotheses in
    between.  The front end and the encoder have no host path, so `forward` is stood in for by seeded encoder outputs; the
    CTC head, the search and everything transcribe does with their results are the model's own."""
    m = model.eval()
    g = torch.Generator().manual_seed(4)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (9000, 6000)]
    enc = torch.randn(2, m.cfg.d_model, 14, generator=g) * 4
    monkey = pytest.MonkeyPatch()
    monkey.setattr(m, "forward", lambda input_signal=None, input_signal_length=None, **kw: (enc, torch.tensor([14, 9])),
                   raising=False)
    try:
        _transcribe_follows_the_strategy(m, audio)
    finally:
        monkey.undo()
        m.decoding_strategy = {}
        m.cur_decoder = "rnnt"


def _transcribe_follows_the_strategy(m, audio):
    m.change_decoding_strategy({"strategy": "greedy"}, "ctc")
    greedy = m.transcribe(audio, language_id="hi", batch_size=2, return_hypotheses=True)
    assert all(isinstance(s, str) for s in greedy[0])                                  # as before this strategy existed
    m.change_decoding_strategy({"strategy": "beam", "beam": {"beam_size": 3, "return_best_hypothesis": False}}, "ctc")
    keep = m._beam_keep = []
    try:
        best, nbest = m.transcribe(audio, language_id="hi", batch_size=2, return_hypotheses=True)
        strings = m.transcribe(audio, language_id="hi", batch_size=2)
    finally:
        m._beam_keep = None
    assert len(best) == len(nbest) == 2 and all(isinstance(h, D.Hypothesis) for h in best)
    assert all(isinstance(nb, D.NBestHypotheses) and 1 <= len(nb.n_best_hypotheses) <= 3 for nb in nbest)
    x, lse, lens = keep[0]
    want = D.beam_ctc_search_host(x, lens, beam_size=3, blank=m.cfg.vocab_per_lang, lse=lse)
    for b in range(2):
        hs = nbest[b].n_best_hypotheses
        assert [(h.y_sequence, h.score) for h in hs] == want[b] and best[b] is hs[0]
        assert all(h.text == " ".join(str(i) for i in h.y_sequence) for h in hs)
        assert [h.score for h in hs] == sorted((h.score for h in hs), reverse=True)
    assert strings[0] == [h.text for h in best] and strings[1] == strings[0]
    m.change_decoding_strategy({"strategy": "beam", "beam": {"beam_size": 3}}, "ctc")  # return_best_hypothesis stays False
    m.change_decoding_strategy({"strategy": "beam", "beam": {"return_best_hypothesis": True}}, "ctc")
    one, every = m.transcribe(audio, language_id="hi", batch_size=2, return_hypotheses=True)
    assert [h.y_sequence for h in one] == [h.y_sequence for h in best] and every == one
    m.change_decoding_strategy({"strategy": "greedy"}, "ctc")
    assert m.transcribe(audio, language_id="hi", batch_size=2, return_hypotheses=True) == greedy
    m.change_decoding_strategy(decoder_type="rnnt")
    m.decoding_strategy = {}


# ---------------------------------------------------------------------------------------------------- the C entries
def test_entry_points_refuse_bad_arguments_before_device_work():
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    assert L.ia_ctc_beam_max_width() == 32
    x, z, n, tok, ln, sc, ws = (ctypes.c_void_p(4096 * (i + 1)) for i in range(7))     # never dereferenced: every call is refused
    B, T, V, W = 2, 10, 17, 4
    need = L.ia_ctc_beam_workspace_bytes(B, T, V, W)
    assert need > 0 and need % 256 == 0 and need >= B * 8 * (1 + W * T)
    assert L.ia_ctc_beam_workspace_bytes(B, T, V, 33) == 0 and L.ia_ctc_beam_workspace_bytes(B, T, 1025, W) == 0
    assert L.ia_ctc_beam_workspace_bytes(0, T, V, W) == 0 and L.ia_ctc_beam_workspace_bytes(B, 0, V, W) == 0
    assert L.ia_ctc_beam_workspace_bytes(B, T, V, 0) == 0
    assert L.ia_ctc_beam_workspace_bytes(B, T, 1024, 32) > 0

    def call(x=x, z=z, n=n, B=B, T=T, ld=V, V=V, blank=V - 1, W=W, floor=-INF, tok=tok, ln=ln, sc=sc, ws=ws, nbytes=need):
        return L.ia_ctc_beam_search(x, z, n, B, T, ld, V, blank, W, floor, tok, ln, sc, ws, nbytes, None)

    bad = ctypes.c_void_p(4096 + 2)
    for kw in (dict(x=None), dict(n=None), dict(tok=None), dict(ln=None), dict(sc=None), dict(ws=None),
               dict(x=bad), dict(z=bad), dict(n=ctypes.c_void_p(4096 + 4)), dict(tok=bad), dict(ln=bad), dict(sc=bad),
               dict(ws=ctypes.c_void_p(4096 + 128)), dict(B=0), dict(T=0), dict(V=0), dict(ld=V - 1), dict(blank=V), dict(blank=-1),
               dict(W=0), dict(floor=float("nan"))):
        assert call(**kw) == -1, kw                                                     # IA_INVALID_VALUE
    assert call(W=33) == -4 and call(V=1025, ld=1025, blank=3) == -4                    # IA_UNSUPPORTED
    assert call(nbytes=need - 1) == -2 and call(nbytes=0) == -2                         # IA_WORKSPACE_TOO_SMALL
    assert call(W=33, nbytes=0) == -4 and call(blank=V, W=33) == -1                     # the order of the checks
