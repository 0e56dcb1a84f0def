"""csrc/rnnt_beam.hip (transducer beam search, alignment-length synchronous decoding, one launch per batch) against the float64
host routine decoding.beam_rnnt_alsd_host with the kernel's rounding points (tests/rnnt_beam_cases.py; the host routine itself
is pinned to the reference's lists by tests/test_rnnt_beam.py).

Tolerance, from reference quantities only: the host routine carries every sequence's state in fp64 and in fp32 and takes each
evaluation's logit tolerance from oracle.decode_ref._evaluate (C = 4, FLOOR = 2^-20, the bf16 flip term in "mfma" mode); a
candidate's slack is its parent's plus twice the step's largest logit tolerance, a recombined score takes the larger of the two.
A step is decided when the beam-th and (beam+1)-th candidates, a winning row's beam-th and (beam+1)-th labels, two duplicates
in the beam and neighbours of the final ranking are further apart than their slacks' sum; for a decided utterance the kernel
must return the reference's lists, order, alignment steps and finished count, each score within its slack + 2^-20 max(1, |E|).

Figures measured on the MI355X box (bf16 / fp32 weights: undecided utterances; recombinations; utterances with a finished list;
largest slack; largest |K - E| of the kernel; largest |K - E| / bound):
  w4          0/0 of 8; 38;  8; 7.5e-4 / 1.8e-4; 3.1e-6 / 2.8e-6; 0.016 / 0.016
  full_tile   1/1 of 8; 303; 8; 3.4e-3 / 4.1e-4; 1.4e-6 / 1.8e-6; 0.011 / 0.010
  w2          0/0 of 8; 1;   6; 4.9e-4 / 2.2e-4; 6.3e-6 / 3.7e-6; 0.025 / 0.056
  production  0/0 of 8; 36;  8; 7.3e-3 / 2.3e-4; 3.8e-6 / 3.2e-6; 0.027 / 0.039
  w1          0/0 of 8; 0;   6; 4.6e-3 / 1.2e-4; 1.3e-6 / 2.0e-6; 0.012 / 0.018
  clamped     0/0 of 4; 8;   2; 1.5e-3 / 3.0e-4; 4.7e-6 / 5.4e-6; 0.015 / 0.017
  all_blank   0/0 of 4; 4;   4; 2.4e-3 / 2.5e-3; 2.4e-6 / 3.6e-6; 0.004 / 0.003
  never_blank 0/0 of 8; 0;   0; 1.4e-3 / 1.3e-3; 3.2e-6 / 4.1e-6; 0.002 / 0.003
The smallest decisive gap of a decided utterance exceeds its slacks' sum by construction (that is what `decided` says).  A beam
of one member (w1) cannot hold a duplicate, so the recombination condition does not apply to it."""
import pytest
import torch

import rnnt_beam_cases as C

pytestmark = pytest.mark.gpu


def _device_case(name, weights):
    return {k: v.cuda() for k, v in C.case_for(name, weights).items()}


def _run(name, weights, n_best=None):
    from indic_cl_asr_amd import decoding as D
    W, a = C.CASES[name][5], C.CASES[name][9]
    raw = D.beam_rnnt_alsd_device(_device_case(name, weights), W, a, True, n_best)
    assert raw is not None, "the kernel refused a shape it must take"
    torch.cuda.synchronize()
    return raw


@pytest.mark.parametrize("weights", ["bf16", "fp32"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_kernel_returns_the_reference_lists(name, weights):
    from indic_cl_asr_amd import decoding as D
    ref = C.reference(name, weights)
    print(name, weights, C.check_conditions(name, ref))
    raw = _run(name, weights)
    got = D.alsd_unpack(raw)
    W = C.CASES[name][5]
    C.assert_matches(name, ref, got, W)
    if name == "never_blank":
        T, a = C.CASES[name][1], C.CASES[name][9]
        lens = C.operands(name)["lens"].clamp(0, T).tolist()
        for b, g in enumerate(got):
            assert g["n_finished"] == 0 and all(len(h[0]) == lens[b] + D.alsd_u_max(a, lens[b]) for h in g["hyps"])
    if name == "clamped":
        assert got[1]["hyps"] == [([], 0.0, [])] and got[2]["hyps"] == [([], 0.0, [])]      # lengths 0 and -3


@pytest.mark.parametrize("name,weights", [("full_tile", "bf16"), ("w4", "fp32"), ("never_blank", "bf16")])
def test_two_launches_are_bit_identical_and_sentinels_intact(name, weights):
    one, two = _run(name, weights), _run(name, weights)
    for x, y in zip(one, two):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    tokens, steps, lengths, scores, nfin = (t.cpu() for t in one)
    B, K, L = tokens.shape
    V = C.CASES[name][4]
    for b in range(B):
        for r in range(K):
            n = int(lengths[b, r])
            if n < 0:
                assert float(scores[b, r]) == float("-inf")
                n = 0
            assert bool((tokens[b, r, n:] == -1).all()) and bool((steps[b, r, n:] == -1).all())
            assert bool(((tokens[b, r, :n] >= 0) & (tokens[b, r, :n] < V - 1)).all())
            st = steps[b, r, :n].tolist()
            assert st == sorted(set(st))                                                # alignment steps increase strictly


def test_n_best_takes_the_first_of_the_ranking():
    from indic_cl_asr_amd import decoding as D
    full, two = D.alsd_unpack(_run("w4", "bf16")), D.alsd_unpack(_run("w4", "bf16", n_best=2))
    for f, t in zip(full, two):
        assert t["hyps"] == f["hyps"][:2] and t["n_finished"] == f["n_finished"]


@pytest.mark.parametrize("weights", ["bf16", "fp32"])
def test_exact_ties_between_label_rows_go_to_the_smaller_id(weights):
    """Copies of a head row give bit-equal logits on the device as on the host: the tie is broken by the rule, not by noise."""
    from indic_cl_asr_amd import decoding as D
    c = C.case_for("w4", weights)
    c = dict(c, Wh=c["Wh"].clone(), bh=c["bh"].clone())
    for dst, src in ((9, 2), (5, 2), (12, 7)):
        c["Wh"][dst] = c["Wh"][src]
        c["bh"][dst] = c["bh"][src]
    ref = D.beam_rnnt_alsd_host(c, 4, 3, True, C.ROUNDING[weights])
    raw = D.beam_rnnt_alsd_device({k: v.cuda() for k, v in c.items()}, 4, 3, True)
    torch.cuda.synchronize()
    C.assert_matches("tie", ref, D.alsd_unpack(raw), 4)
    assert sum(r["decided"] for r in ref) >= 6, [r["undecided"] for r in ref]


def test_refusals_occur_without_launching():
    from test_rnnt_beam import check_entry_point_refusals
    check_entry_point_refusals()
    torch.cuda.synchronize()                                                            # nothing was launched, nothing faulted


# --------------------------------------------------------------------------------------------------------- model level
@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_transcribe_under_alsd_equals_the_host_routine(compute_dtype):
    from indic_cl_asr_amd import decoding as D
    from oracle import decode_ref as R
    from test_decode_reference_gpu import make_model, model_rounding
    m = make_model(compute_dtype).cuda()
    g = torch.Generator().manual_seed(8)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (16000, 11000, 8000)]
    greedy = m.transcribe(audio, language_id="hi", batch_size=3, return_hypotheses=True)
    m.change_decoding_strategy({"strategy": "alsd", "beam": {"beam_size": 4, "return_best_hypothesis": False}})
    keep = m._beam_keep = []
    try:
        best, nbest = m.transcribe(audio, language_id="hi", batch_size=3, return_hypotheses=True)
        strings = m.transcribe(audio, language_id="hi", batch_size=3)
    finally:
        m._beam_keep = None
    enc, lens = keep[0]
    case = R.case_from_model(m, enc, lens, "hi")
    ref = D.beam_rnnt_alsd_host(case, 4, 1.0, True, model_rounding(case))
    print(compute_dtype, [r["decided"] for r in ref], [r["n_finished"] for r in ref])
    got = [dict(hyps=[(h.y_sequence, h.score, h.timestep) for h in nb.n_best_hypotheses], n_finished=nb.n_finished) for nb in nbest]
    C.assert_matches("model", ref, got, 4)
    assert sum(r["decided"] for r in ref) >= 1
    assert all(isinstance(nb, D.NBestHypotheses) and best[b] is nb.n_best_hypotheses[0] for b, nb in enumerate(nbest))
    assert all(h.text == " ".join(str(i) for i in h.y_sequence) for nb in nbest for h in nb.n_best_hypotheses)
    assert strings[0] == [h.text for h in best]
    m.change_decoding_strategy({"strategy": "greedy_batch"})
    assert m.transcribe(audio, language_id="hi", batch_size=3, return_hypotheses=True) == greedy
