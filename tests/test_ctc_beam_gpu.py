"""CTC prefix beam search on the MI355X (csrc/ctc_beam.hip) through its C ABI and through the model, against the float64
restatement E of tests/ctc_beam_ref.py.

The kernel sums in fp32 in its own order, so a decision that rests on a score difference below the fp32 error may fall either
way.  margin = 16 x the largest |F32 - E| hypothesis-score difference on the case's own inputs (F32 = the same restatement
in float32; no code under test is involved; the factor leaves room for another summation order).  An utterance whose smallest
decisive gap in E exceeds the margin is DECIDED: tokens, order and lengths must equal E's exactly, and each score must satisfy
|K - E| <= 4 |F32 - E| + 2^-20 max(1, |E|).  At most one third of a case's utterances may be undecided.

Measured (MI355X, the seeds below, raw logits + lse / log-probs; ratio = max |K - E| / bound over decided hypotheses):
    T   V   W   margin             undecided of 8   ratio
    48  17  1   4.7e-5 / 1.1e-4    0 / 0            0.037 / 0.032
    48  17  4   1.3e-4 / 9.4e-5    0 / 0            0.040 / 0.033
    48  17  16  2.0e-4 / 8.1e-5    1 / 0            0.040 / 0.047
    24  17  32  4.7e-5 / 3.2e-5    0 / 0            0.076 / 0.081
    48  257 4   1.4e-4 / 1.0e-4    0 / 0            0.043 / 0.045
    48  257 16  1.5e-4 / 1.2e-4    1 / 1            0.045 / 0.042
    33  257 32  7.5e-5 / 7.7e-5    0 / 0            0.043 / 0.043
  T = 300, V = 257, W = 8: margin 1.3e-3, smallest gaps 3.5e-5 and 1.0e-4 (undecided, as expected), best labelling E's in both
  utterances, max (K - exact log-likelihood) = -1.4e-3.  End to end: six utterances, gaps 1.9e-3 .. 2.7e-2 against margins
  of 3.5e-5 and 8.3e-5: all decided.  Every case prints its figures before it asserts (pytest -s); DESIGN.md has the table."""
import numpy as np
import pytest
import torch

import ctc_beam_ref as R

pytestmark = pytest.mark.gpu

INF = float("inf")
GUARD = 64


def _call(x, lens, V, W, lse=None, blank=None, floor=-INF, ws_bytes=None):
    """ia_ctc_beam_search on host tensors x [B,T,ld]; outputs live between sentinel-filled guards of one buffer.
    Returns (status, tokens [B,W,T], lengths [B,W], scores [B,W], the whole buffer as bytes)."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    B, T, ld = x.shape
    blank = V - 1 if blank is None else blank
    xd, ild = x.cuda().contiguous(), lens.cuda()
    lsed = lse.cuda().contiguous() if lse is not None else None
    n = L.ia_ctc_beam_workspace_bytes(B, T, V, W) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device="cuda")
    n_tok, n_w = B * W * T, B * W
    buf = torch.full((4 * GUARD + n_tok + 2 * n_w,), -7, dtype=torch.int32, device="cuda")
    o_tok, o_len, o_sc = GUARD, 2 * GUARD + n_tok, 3 * GUARD + n_tok + n_w
    tok, ln, sc = buf[o_tok:o_tok + n_tok], buf[o_len:o_len + n_w], buf[o_sc:o_sc + n_w]
    st = L.ia_ctc_beam_search(_lib.ptr(xd), _lib.ptr(lsed), _lib.ptr(ild), B, T, ld, V, blank, W, floor, _lib.ptr(tok), _lib.ptr(ln),
                              _lib.ptr(sc), _lib.ptr(ws), n, _lib.stream_ptr())
    torch.cuda.synchronize()
    host = buf.cpu()
    guards = torch.cat([host[:o_tok], host[o_tok + n_tok:o_len], host[o_len + n_w:o_sc], host[o_sc + n_w:]])
    assert bool((guards == -7).all()), "bytes outside the documented outputs were written"
    return (st, host[o_tok:o_tok + n_tok].view(B, W, T).numpy(), host[o_len:o_len + n_w].view(B, W).numpy(),
            host[o_sc:o_sc + n_w].view(torch.float32).view(B, W).numpy(), host.numpy().tobytes())


def _hyps(tok, ln, sc, b):
    """Hypotheses of utterance b from the packed result, checking the padding on the way."""
    W, T = tok.shape[1], tok.shape[2]
    out = []
    for r in range(W):
        n = int(ln[b, r])
        if n < 0:
            assert n == -1 and sc[b, r] == -INF and np.all(tok[b, r] == -1)
            assert all(int(ln[b, q]) == -1 for q in range(r, W))                    # unfilled slots come last
            continue
        assert n <= T and np.all(tok[b, r, n:] == -1) and np.all(tok[b, r, :n] >= 0)
        out.append((tok[b, r, :n].tolist(), float(sc[b, r])))
    return out


def _inputs(T, V, s, B, seed, ld):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, T, ld, generator=g) * s
    x[..., V - 1] += s
    lens = torch.tensor([T, 0, 1, T, T - 3, T - 10, T, (T + 1) // 2][:B])
    return x, lens


def _check_case(x, lens, V, W, logits_mode, label, blank=None, floor=None):
    """Decisions and scores of one batch against E under the margin rule; returns the figures and the packed result."""
    B, T, ld = x.shape
    blank = V - 1 if blank is None else blank
    if logits_mode:
        xin, lse = x, torch.logsumexp(x[..., :V], -1)
    else:
        xin, lse = torch.zeros_like(x), None
        xin[..., :V] = x[..., :V].log_softmax(-1)
        xin[..., V:] = 7.0                                                            # the padding columns are never read
    cut = [min(max(int(n), 0), T) for n in lens]                                      # the kernel clamps the lengths
    xs = [xin[b, :cut[b], :V].numpy() for b in range(B)]
    lses = None if lse is None else [lse[b, :cut[b]].numpy() for b in range(B)]
    es, fs, worst = R.margin_of(xs, W, blank, lses, floor)
    margin = 16 * worst
    st, tok, ln, sc, _ = _call(xin, lens, V, W, lse=lse, blank=blank, floor=-INF if floor is None else floor)
    assert st == 0
    undecided, ratio = 0, 0.0
    for b in range(B):
        (e, gap), (f, _) = es[b], fs[b]
        k = _hyps(tok, ln, sc, b)
        if not gap > margin:
            undecided += 1
            continue
        assert [y for y, _ in k] == [y for y, _ in e], (label, b, gap, margin)
        for r, ((y, se), (_, sk)) in enumerate(zip(e, k)):
            f_err = abs(f[r][1] - se) if r < len(f) and f[r][0] == y else worst
            bound = 4 * f_err + 2.0 ** -20 * max(1.0, abs(se))
            ratio = max(ratio, abs(sk - se) / bound)
            assert abs(sk - se) <= bound, (label, b, r, sk, se, bound)
    print(f"{label}: max|F32-E|={worst:.3e} margin={margin:.3e} undecided={undecided}/{B} max|K-E|/bound={ratio:.3f}")
    assert 3 * undecided <= B, (label, undecided, B)
    return tok, ln, sc


CASES = [(48, 17, 1), (48, 17, 4), (48, 17, 16), (24, 17, 32), (48, 257, 4), (48, 257, 16), (33, 257, 32)]


@pytest.mark.parametrize("logits_mode", [True, False])
@pytest.mark.parametrize("T,V,W", CASES)
def test_decisions_and_scores_against_the_restatement(T, V, W, logits_mode):
    """Logits s N(0,1) with +s on the blank column (s = 3 at V = 17, 4 at V = 257), lengths 0, 1, T and others in one batch,
    ld > V, raw logits + lse and log-probs.  Measured: DESIGN.md."""
    x, lens = _inputs(T, V, 3.0 if V == 17 else 4.0, 8, 1000 * W + V + T, V + 7)
    _check_case(x, lens, V, W, logits_mode, f"T={T} V={V} W={W} {'logits+lse' if logits_mode else 'log-probs'}")


def test_a_realistic_shape_holds_the_tie_tolerant_properties():
    """T = 300, V = 257, W = 8: near-ties are certain over that many frames, so: no hypothesis scores above its labelling's
    exact CTC log-likelihood (the beam only ever loses alignments) by more than the margin; the best labelling is E's, or
    its exact log-likelihood reaches E's best score up to the margin; two launches agree bit for bit."""
    T, V, W, ld = 300, 257, 8, 264
    x, _ = _inputs(T, V, 4.0, 2, 77, ld)
    lens = torch.tensor([T, 257])
    lse = torch.logsumexp(x[..., :V], -1)
    xs = [x[b, :int(lens[b]), :V].numpy() for b in range(2)]
    lses = [lse[b, :int(lens[b])].numpy() for b in range(2)]
    es, fs, worst = R.margin_of(xs, W, V - 1, lses)
    margin = 16 * worst
    st, tok, ln, sc, raw = _call(x, lens, V, W, lse=lse)
    assert st == 0
    for b in range(2):
        k = _hyps(tok, ln, sc, b)
        assert len(k) == W and len({tuple(y) for y, _ in k}) == W
        assert [s for _, s in k] == sorted((s for _, s in k), reverse=True)
        lp = xs[b].astype(np.float64) - lses[b].astype(np.float64)[:, None]
        exact = [R.ctc_log_likelihood(lp, y, V - 1) for y, _ in k]
        over = max(s - ll for (_, s), ll in zip(k, exact))
        (e, gap), same = es[b], k[0][0] == es[b][0][0][0]
        print(f"b={b}: margin={margin:.3e} gap={gap:.3e} max(K - exact)={over:.3e} best is E's: {same} "
              f"K best={k[0][1]:.6f} E best={e[0][1]:.6f} exact(K best)={exact[0]:.6f}")
        assert over <= margin
        assert same or exact[0] >= e[0][1] - margin
    again = _call(x, lens, V, W, lse=lse)
    assert again[0] == 0 and again[4] == raw


def test_beam_of_one_and_the_padding():
    """W = 1: one slot per utterance.  Frames beyond a hypothesis hold -1; an utterance without frames is the empty
    hypothesis with score 0; lengths beyond T are clamped; nothing outside the three outputs is written (_call's guards)."""
    T, V = 40, 17
    x, _ = _inputs(T, V, 3.0, 4, 5, V + 3)
    lens = torch.tensor([T, 0, T + 50, -3])
    tok, ln, sc = _check_case(x, lens, V, 1, True, "W=1, lengths T, 0, T+50, -3")
    assert tok.shape == (4, 1, T) and all(len(_hyps(tok, ln, sc, b)) == 1 for b in range(4))
    assert ln[1, 0] == 0 and sc[1, 0] == 0.0 and ln[3, 0] == 0 and sc[3, 0] == 0.0 and ln[2, 0] <= T
    # a beam wider than the candidates there are: the slots the beam never filled say so
    tok, ln, sc = _check_case(x[:, :1].contiguous(), torch.tensor([1, 1, 0, 1]), V, 32, True, "W=32 over one frame")
    for b in (0, 1, 3):
        assert len(_hyps(tok, ln, sc, b)) == V and np.all(ln[b, V:] == -1) and np.all(sc[b, V:] == -INF)
    assert len(_hyps(tok, ln, sc, 2)) == 1


def test_token_min_logp_and_a_blank_that_is_not_last():
    """Extensions below the floor are not made (about two thirds of the tokens of a frame here); class 0 is the blank."""
    T, V, W = 30, 17, 4
    x, lens = _inputs(T, V, 3.0, 6, 21, V)
    tok, ln, sc = _check_case(x, lens, V, W, False, "token_min_logp=log 0.05, blank=0", blank=0, floor=float(np.log(0.05)))
    free = _check_case(x, lens, V, W, False, "no floor, blank=0", blank=0)
    assert any(_hyps(tok, ln, sc, b) != _hyps(*free, b) for b in range(6))


def test_a_prefix_that_left_the_beam_and_came_back_merges_with_its_child():
    """The constructed case of tests/test_ctc_beam.py (`a b` leaves, its child `a b a` stays, `a b` returns) on the kernel:
    its trie must find the old node of `a b` again, or `a b a` is in the beam twice."""
    from test_ctc_beam import REENTRY
    lp = torch.tensor([REENTRY], dtype=torch.float64).log().float()
    e, gap = R.E(lp[0].numpy(), 3)
    st, tok, ln, sc, _ = _call(lp, torch.tensor([6]), 3, 3)
    k = _hyps(tok, ln, sc, 0)
    assert st == 0 and gap > 1e-3 and [y for y, _ in k] == [y for y, _ in e] == [[0, 1], [0, 1, 0, 1], [0, 1, 0]]
    assert max(abs(a[1] - c[1]) for a, c in zip(e, k)) <= 2.0 ** -20 * 8       # six frames of fp32 sums of magnitude < 4


def test_python_entry_dispatch_and_limits():
    from indic_cl_asr_amd import decoding as D
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(2, 12, 9, generator=g) * 3).log_softmax(-1)
    lens = torch.tensor([12, 7])
    dev = D.beam_ctc_decode(x.cuda(), lens.cuda(), beam_size=3, return_best_hypothesis=False)
    host = D.beam_ctc_decode_host(x, lens, beam_size=3, return_best_hypothesis=False)
    for a, b in zip(dev, host):
        assert [h.y_sequence for h in a.n_best_hypotheses] == [h.y_sequence for h in b.n_best_hypotheses]
        assert np.allclose([h.score for h in a.n_best_hypotheses], [h.score for h in b.n_best_hypotheses], atol=1e-4)
    D._warned_beam_limit = False
    with pytest.warns(UserWarning, match="32"):
        wide = D.beam_ctc_decode(x.cuda(), lens.cuda(), beam_size=33)
    assert [h.y_sequence for h in wide] == [h.y_sequence for h in D.beam_ctc_decode_host(x, lens, beam_size=33)]


@pytest.fixture(scope="module")
def tiny():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(17)
    return EncDecHybridRNNTCTCModel(model_config("tiny")).cuda().eval()


def test_transcribe_returns_the_n_best_of_the_head_logits(tiny):
    """change_decoding_strategy(ctc, beam) + transcribe(return_hypotheses=True): the N-best equals beam_ctc_decode_host on the
    very logits and lse the kernel read, on decided utterances under the margin rule and cap above; back on greedy the
    transcripts are those from before."""
    from indic_cl_asr_amd import decoding as D
    m = tiny
    lang = m.cfg.languages[0]
    g = torch.Generator().manual_seed(6)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (16000, 9000, 12000, 5000, 14000, 8000)]
    m.change_decoding_strategy(decoder_type="ctc", decoding_cfg={"strategy": "greedy"})
    before = m.transcribe(audio, language_id=lang, batch_size=3, return_hypotheses=True)
    m.change_decoding_strategy(decoder_type="ctc", decoding_cfg={"strategy": "beam", "beam": {"beam_size": 4, "return_best_hypothesis": False}})
    keep = m._beam_keep = []
    try:
        best, nbest = m.transcribe(audio, language_id=lang, batch_size=3, return_hypotheses=True)
    finally:
        m._beam_keep = None
    assert len(best) == len(nbest) == 6 and len(keep) == 2
    V = m.cfg.vocab_per_lang + 1
    k, undecided = 0, 0
    for x, lse, enc_len in keep:
        assert x.is_cuda and lse is not None and x.shape[-1] == V
        xc, lc, nc = x.float().cpu(), lse.cpu(), enc_len.cpu()
        host = D.beam_ctc_decode_host(xc, nc, beam_size=4, blank=V - 1, lse=lc, return_best_hypothesis=False)
        xs = [xc[b, :int(nc[b])].numpy() for b in range(xc.shape[0])]
        lses = [lc[b, :int(nc[b])].numpy() for b in range(xc.shape[0])]
        es, fs, worst = R.margin_of(xs, 4, V - 1, lses)
        margin = 16 * worst
        for b in range(xc.shape[0]):
            got, want = nbest[k].n_best_hypotheses, host[b].n_best_hypotheses
            assert best[k] is got[0] and all(isinstance(h.text, str) for h in got)
            gap = es[b][1]
            print(f"utterance {k}: gap={gap:.3e} margin={margin:.3e}")
            if gap > margin:
                assert [h.y_sequence for h in got] == [h.y_sequence for h in want]
                for r, (a, w) in enumerate(zip(got, want)):
                    f_err = abs(fs[b][0][r][1] - es[b][0][r][1]) if fs[b][0][r][0] == es[b][0][r][0] else worst
                    assert abs(a.score - w.score) <= 4 * f_err + 2.0 ** -20 * max(1.0, abs(w.score))
            else:
                undecided += 1
            k += 1
    assert 3 * undecided <= 6
    m.change_decoding_strategy(decoder_type="ctc", decoding_cfg={"strategy": "greedy"})
    assert m.transcribe(audio, language_id=lang, batch_size=3, return_hypotheses=True) == before
    m.change_decoding_strategy(decoder_type="rnnt")
    m.decoding_strategy = {}
