"""CTC prefix beam search with n-gram LM shallow fusion on the MI355X (csrc/ctc_beam_lm.hip) through its C ABI and through the
model, against the float64 restatement E of tests/ngram_lm_ref.py.

The margin rule of tests/test_ctc_beam_gpu.py, restated with E and F32 the LM restatement: margin = 16 x the case's largest
|F32 - E| hypothesis-score difference; an utterance whose smallest decisive gap in E exceeds the margin is DECIDED: tokens, order
and lengths must equal E's, and each score must satisfy |K - E| <= 4 |F32 - E| + 2^-20 max(1, |E|).  At most 2 of a case's 8
utterances may be undecided (tests/test_ctc_beam_lm.py holds that condition on the CPU, with E and F32 alone).  The LM of a case
goes the whole way: dict -> ARPA text -> ngram_lm.NGramLM -> device image.  Every case prints its figures before it asserts
(pytest -s); DESIGN.md has the table."""
import ctypes
import math

import numpy as np
import pytest
import torch

import ngram_lm_ref as R
from test_ctc_beam_lm import ALPHA, BETA, GPU_CASES, gpu_case, load
from test_ctc_beam_gpu import GUARD, _call, _hyps

pytestmark = pytest.mark.gpu

INF = float("inf")


def _call_lm(x, lens, V, W, lm, alpha=ALPHA, beta=BETA, lse=None, blank=None, floor=-INF, ws_bytes=None, image=None, null=(),
             shift=()):
    """ia_ctc_beam_search_lm on host tensors x [B,T,ld]; outputs between sentinel-filled guards of one buffer, as _call of
    tests/test_ctc_beam_gpu.py.  `image`: an ia_ngram_lm to pass instead of lm's; `null` / `shift`: names among x, lens, tok, ln,
    sc, ws, lm to pass as NULL / two bytes off."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    B, T, ld = x.shape
    blank = V - 1 if blank is None else blank
    xd, ild = x.cuda().contiguous(), lens.cuda()
    lsed = lse.cuda().contiguous() if lse is not None else None
    n = L.ia_ctc_beam_lm_workspace_bytes(B, T, V, W) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device="cuda")
    n_tok, n_w = B * W * T, B * W
    buf = torch.full((4 * GUARD + n_tok + 2 * n_w,), -7, dtype=torch.int32, device="cuda")
    o_tok, o_len, o_sc = GUARD, 2 * GUARD + n_tok, 3 * GUARD + n_tok + n_w
    tok, ln, sc = buf[o_tok:o_tok + n_tok], buf[o_len:o_len + n_w], buf[o_sc:o_sc + n_w]
    img = lm.to("cuda")[1] if image is None else image
    ptrs = dict(x=_lib.ptr(xd), lens=_lib.ptr(ild), tok=_lib.ptr(tok), ln=_lib.ptr(ln), sc=_lib.ptr(sc), ws=_lib.ptr(ws))
    for k in null:
        if k != "lm":
            ptrs[k] = None
    for k in shift:
        ptrs[k] = ctypes.c_void_p(ptrs[k].value + 2)
    st = L.ia_ctc_beam_search_lm(ptrs["x"], _lib.ptr(lsed), ptrs["lens"], B, T, ld, V, blank, W, floor,
                                 None if "lm" in null else ctypes.byref(img), alpha, beta, ptrs["tok"], ptrs["ln"], ptrs["sc"],
                                 ptrs["ws"], n, _lib.stream_ptr())
    torch.cuda.synchronize()
    host = buf.cpu()
    guards = torch.cat([host[:o_tok], host[o_tok + n_tok:o_len], host[o_len + n_w:o_sc], host[o_sc + n_w:]])
    assert bool((guards == -7).all()), "bytes outside the documented outputs were written"
    return (st, host[o_tok:o_tok + n_tok].view(B, W, T).numpy(), host[o_len:o_len + n_w].view(B, W).numpy(),
            host[o_sc:o_sc + n_w].view(torch.float32).view(B, W).numpy(), host.numpy().tobytes())


def _judge(label, es, fs, worst, tok, ln, sc, cap=2):
    """The margin rule over one batch; prints the figures, then asserts the cap."""
    margin, B = 16 * worst, len(es)
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
    assert undecided <= cap, (label, undecided, B)


@pytest.mark.parametrize("logits_mode", [True, False])
@pytest.mark.parametrize("T,V,W,N", list(GPU_CASES))
def test_decisions_and_scores_against_the_restatement(tmp_path, T, V, W, N, logits_mode):
    """The construction of tests/test_ctc_beam_gpu.py (lengths T, 0, 1, T, T-3, T-10, T, (T+1)//2, row stride V + 7, raw logits
    + lse and log-probs) with a random model of order N: log10 p in [-3, -0.1], back-off in [-1, 0], arc density 0.3 at V = 17
    and 0.02 above, alpha = 0.7, beta = 0.5.  (6, 1024, 32, 2) sits at both limits of the kernel."""
    xin, lse, lens, src, es, fs, worst = gpu_case(T, V, W, N, logits_mode)
    lm = load(tmp_path, src, N, V - 1)
    st, tok, ln, sc, _ = _call_lm(xin, lens, V, W, lm, lse=lse)
    assert st == 0
    _judge(f"T={T} V={V} W={W} N={N} {'logits+lse' if logits_mode else 'log-probs'}", es, fs, worst, tok, ln, sc)


def test_two_launches_agree_and_zero_weights_are_the_search_without_a_model(tmp_path):
    """Bit for bit over the whole output buffer, guards included: a second launch; and alpha = beta = 0 against
    ia_ctc_beam_search on the same inputs (plain and with a floor; V = 17 and V = 257)."""
    for (T, V, W, N), floor in (((48, 257, 16, 2), -INF), ((48, 17, 16, 3), -INF), ((33, 257, 32, 3), math.log(0.01))):
        xin, lse, lens, src, *_ = gpu_case(T, V, W, N, True)
        lm = load(tmp_path, src, N, V - 1, name=f"v{V}n{N}.arpa")
        one = _call_lm(xin, lens, V, W, lm, lse=lse, floor=floor)
        two = _call_lm(xin, lens, V, W, lm, lse=lse, floor=floor)
        assert one[0] == two[0] == 0 and one[4] == two[4]
        zero = _call_lm(xin, lens, V, W, lm, alpha=0.0, beta=0.0, lse=lse, floor=floor)
        free = _call(xin, lens, V, W, lse=lse, floor=floor)
        assert zero[0] == free[0] == 0 and zero[4] == free[4]
        assert one[4] != free[4]


def test_an_unpruned_search_scores_ctc_plus_alpha_lm_plus_beta_length(tmp_path):
    """V = 3, T = 4, W = 32: all 31 prefixes arrive and each finite score is ln P_CTC(l) + alpha ln P_LM(l) + beta |l| up to the
    fp32 bound of the margin rule (4 x the largest |F32 - E| of these inputs + 2^-20 max(1, |score|))."""
    g = torch.Generator().manual_seed(5)
    lp = (torch.randn(2, 4, 3, generator=g, dtype=torch.float64) * 2).log_softmax(-1).float()
    src = R.random_lm(2, 3, 0.6, 11)
    lm = load(tmp_path, src, 3, 2)
    xs = [lp[b].numpy() for b in range(2)]
    _, _, worst = R.margin_of(xs, 32, src, 3, ALPHA, BETA, 2)
    st, tok, ln, sc, _ = _call_lm(lp, torch.tensor([4, 4]), 3, 32, lm)
    assert st == 0
    for b in range(2):
        k = _hyps(tok, ln, sc, b)
        assert len(k) == 31 and len({tuple(y) for y, _ in k}) == 31
        for y, s in k:
            want = R.ctc_log_likelihood(xs[b], y, 2) + ALPHA * R.lm_sequence(src, 3, y) + BETA * len(y)
            assert (s == want) if want == -INF else abs(s - want) <= 4 * worst + 2.0 ** -20 * max(1.0, abs(want)), (y, s, want)


def test_a_prefix_that_left_the_beam_and_came_back_merges_with_its_child(tmp_path):
    """The construction of tests/test_ctc_beam.py with a model attached (alpha = 0.1: `a b` still leaves after frame 3 and
    returns after frame 4 while `a b a` stays -- asserted on E's trace): the trie finds the old node of `a b` again and the
    returning member gets a state and a row of its own."""
    from test_ctc_beam import REENTRY
    lp = torch.tensor([REENTRY], dtype=torch.float64).log().float()
    src = R.random_lm(2, 3, 0.6, 1)
    lm = load(tmp_path, src, 3, 2)
    trace = []
    e, gap = R.E(lp[0].numpy(), 3, src, 3, 0.1, 0.0, trace=trace)
    assert (0, 1) in trace[2] and (0, 1) not in trace[3] and (0, 1) in trace[4] and all((0, 1, 0) in trace[t] for t in (3, 4, 5))
    st, tok, ln, sc, _ = _call_lm(lp, torch.tensor([6]), 3, 3, lm, alpha=0.1, beta=0.0)
    k = _hyps(tok, ln, sc, 0)
    assert st == 0 and gap > 1e-3 and [y for y, _ in k] == [y for y, _ in e] and [0, 1, 0] in [y for y, _ in k]
    assert max(abs(a[1] - c[1]) for a, c in zip(e, k)) <= 2.0 ** -20 * 16     # six frames of fp32 sums of magnitude < 8


def test_token_min_logp_and_a_blank_that_is_not_last(tmp_path):
    """Class 0 is the blank, so the LM's tokens are the classes 1 .. V - 1 (token 0 is never asked for); the floor looks at
    the acoustic log-prob alone."""
    from test_ctc_beam_gpu import _inputs
    T, V, W, N = 30, 17, 4, 3
    x, lens = _inputs(T, V, 3.0, 6, 21, V)
    xin = x.log_softmax(-1)
    src = R.random_lm(V, N, 0.3, 5)
    lm = load(tmp_path, src, N, V)
    xs = [xin[b, :int(lens[b])].numpy() for b in range(6)]
    out = {}
    for floor in (float(np.log(0.05)), None):
        es, fs, worst = R.margin_of(xs, W, src, N, ALPHA, BETA, 0, None, floor)
        st, tok, ln, sc, _ = _call_lm(xin, lens, V, W, lm, blank=0, floor=-INF if floor is None else floor)
        assert st == 0
        _judge(f"blank=0 floor={floor}", es, fs, worst, tok, ln, sc)
        out[floor] = [_hyps(tok, ln, sc, b) for b in range(6)]
    assert out[None] != out[float(np.log(0.05))]


def test_every_refusal_leaves_the_outputs_untouched(tmp_path):
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    T, V, W = 12, 17, 4
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(2, T, V, generator=g) * 3).log_softmax(-1)
    lens = torch.tensor([T, 7])
    lm = load(tmp_path, R.random_lm(V - 1, 3, 0.3, 2), 3, V - 1)
    uni = load(tmp_path, R.random_lm(V - 1, 1, 0.3, 2), 1, V - 1, name="uni.arpa")
    good = lm.to("cuda")[1]
    untouched = lambda raw: np.all(np.frombuffer(raw, np.int32) == -7)

    def changed(**kw):
        img = _lib.NGramLM.from_buffer_copy(good)
        for k, v in kw.items():
            setattr(img, k, v)
        return img

    assert L.ia_ctc_beam_lm_max_order() == 8 and L.ia_ctc_beam_lm_workspace_bytes(2, T, V, W) > L.ia_ctc_beam_workspace_bytes(2, T, V, W)
    assert L.ia_ctc_beam_lm_workspace_bytes(2, T, V, 33) == 0 and L.ia_ctc_beam_lm_workspace_bytes(2, T, 1025, W) == 0
    assert _call_lm(x, lens, V, W, lm)[0] == 0 and _call_lm(x, lens, V, W, uni)[0] == 0
    invalid = [dict(null=(k,)) for k in ("x", "lens", "tok", "ln", "sc", "ws", "lm")] + [dict(shift=(k,)) for k in ("x", "tok", "ws")]
    invalid += [dict(alpha=float("nan")), dict(beta=float("nan")), dict(floor=float("nan")), dict(blank=V)]
    invalid += [dict(image=changed(**kw)) for kw in (dict(order=0), dict(n_states=0), dict(n_arcs=-1), dict(n_tokens=0),
                                                     dict(start=lm.n_states), dict(start=-1), dict(order=1), dict(states=None),
                                                     dict(arcs=None), dict(uni_next=None), dict(backoff=good.backoff + 2),
                                                     dict(unk_logp=float("nan")))]
    for kw in invalid:
        st, *_, raw = _call_lm(x, lens, V, W, lm, **kw)
        assert st == -1 and untouched(raw), kw                                        # IA_INVALID_VALUE
    for kw in (dict(image=changed(order=9)),):
        st, *_, raw = _call_lm(x, lens, V, W, lm, **kw)
        assert st == -4 and untouched(raw), kw                                        # IA_UNSUPPORTED
    st, *_, raw = _call_lm(x, lens, V, 33, lm, ws_bytes=1 << 20)
    assert st == -4 and untouched(raw)
    wide = torch.zeros(2, T, 1025)
    st, *_, raw = _call_lm(wide, lens, 1025, W, lm, ws_bytes=1 << 20)
    assert st == -4 and untouched(raw)
    st, *_, raw = _call_lm(x, lens, V, W, lm, ws_bytes=L.ia_ctc_beam_lm_workspace_bytes(2, T, V, W) - 1)
    assert st == -2 and untouched(raw)                                                # IA_WORKSPACE_TOO_SMALL


def test_python_entry_dispatch(tmp_path):
    from indic_cl_asr_amd import decoding as D
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(2, 12, 9, generator=g) * 3).log_softmax(-1)
    lens = torch.tensor([12, 7])
    lm = load(tmp_path, R.random_lm(8, 3, 0.4, 2), 3, 8)
    kw = dict(beam_size=3, return_best_hypothesis=False, lm=lm, beam_alpha=ALPHA, beam_beta=BETA)
    dev = D.beam_ctc_decode(x.cuda(), lens.cuda(), **kw)
    host = D.beam_ctc_decode_host(x, lens, **kw)
    for a, b in zip(dev, host):
        assert [h.y_sequence for h in a.n_best_hypotheses] == [h.y_sequence for h in b.n_best_hypotheses]
        assert np.allclose([h.score for h in a.n_best_hypotheses], [h.score for h in b.n_best_hypotheses], atol=1e-4)
    D._warned_beam_limit = False
    with pytest.warns(UserWarning, match="32"):
        wide = D.beam_ctc_decode(x.cuda(), lens.cuda(), **dict(kw, beam_size=33))
    assert [[h.y_sequence for h in nb.n_best_hypotheses] for nb in wide] == \
        [[h.y_sequence for h in nb.n_best_hypotheses] for nb in D.beam_ctc_decode_host(x, lens, **dict(kw, beam_size=33))]


@pytest.fixture(scope="module")
def tiny():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(17)
    return EncDecHybridRNNTCTCModel(model_config("tiny")).cuda().eval()


def test_transcribe_fuses_the_model_of_the_language(tiny, tmp_path):
    """change_decoding_strategy(ctc, beam, kenlm_path=<ARPA file>) + transcribe(return_hypotheses=True): the N-best equals
    beam_ctc_decode_host with the same model on the very logits and lse the kernel read (decided utterances, margin rule, at
    most one third undecided as in tests/test_ctc_beam_gpu.py), and differs from the N-best without a model."""
    from indic_cl_asr_amd import decoding as D
    m = tiny
    lang = m.cfg.languages[0]
    Vt = m.cfg.vocab_per_lang
    src = R.random_lm(Vt, 3, 0.05, 3)
    path = tmp_path / "tiny.arpa"
    R.write_arpa(path, src, 3)
    g = torch.Generator().manual_seed(6)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (16000, 9000, 12000, 5000, 14000, 8000)]
    beam = {"beam_size": 4, "return_best_hypothesis": False}
    try:
        m.change_decoding_strategy(decoder_type="ctc", decoding_cfg={"strategy": "beam", "beam": beam})
        _, free = m.transcribe(audio, language_id=lang, batch_size=3, return_hypotheses=True)
        m.change_decoding_strategy(decoder_type="ctc", decoding_cfg={"strategy": "beam", "beam": dict(
            beam, kenlm_path={lang: str(path)}, beam_alpha=ALPHA, beam_beta=BETA)})
        keep = m._beam_keep = []
        try:
            best, nbest = m.transcribe(audio, language_id=lang, batch_size=3, return_hypotheses=True)
        finally:
            m._beam_keep = None
        lm = m.decoding_strategy["ctc"]["lms"][lang]
        assert len(best) == len(nbest) == 6 and len(keep) == 2
        V = Vt + 1
        k, undecided = 0, 0
        for x, lse, enc_len in keep:
            xc, lc, nc = x.float().cpu(), lse.cpu(), enc_len.cpu()
            host = D.beam_ctc_decode_host(xc, nc, beam_size=4, blank=V - 1, lse=lc, return_best_hypothesis=False, lm=lm,
                                          beam_alpha=ALPHA, beam_beta=BETA)
            xs = [xc[b, :int(nc[b])].numpy() for b in range(xc.shape[0])]
            lses = [lc[b, :int(nc[b])].numpy() for b in range(xc.shape[0])]
            es, fs, worst = R.margin_of(xs, 4, src, 3, ALPHA, BETA, V - 1, lses)
            margin = 16 * worst
            for b in range(xc.shape[0]):
                got, want = nbest[k].n_best_hypotheses, host[b].n_best_hypotheses
                assert best[k] is got[0] and all(isinstance(h.text, str) for h in got)
                gap = es[b][1]
                print(f"utterance {k}: gap={gap:.3e} margin={margin:.3e}")
                if gap > margin:
                    assert [h.y_sequence for h in got] == [h.y_sequence for h in want] == [y for y, _ in es[b][0]]
                    for r, (a, w) in enumerate(zip(got, want)):
                        f_err = abs(fs[b][0][r][1] - es[b][0][r][1]) if fs[b][0][r][0] == es[b][0][r][0] else worst
                        assert abs(a.score - w.score) <= 4 * f_err + 2.0 ** -20 * max(1.0, abs(w.score))
                else:
                    undecided += 1
                k += 1
        assert 3 * undecided <= 6
        assert any([h.y_sequence for h in a.n_best_hypotheses] != [h.y_sequence for h in b.n_best_hypotheses]
                   for a, b in zip(nbest, free))
    finally:
        m.change_decoding_strategy(decoder_type="rnnt")
        m.decoding_strategy = {}
