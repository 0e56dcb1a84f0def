"""CTC prefix beam search with n-gram LM shallow fusion, host side: the ARPA reader and its flat image, the float64 host routine
of indic_cl_asr_amd/decoding.py against the numpy restatement tests/ngram_lm_ref.py (E), the identity an unpruned search obeys,
the kenlm_path surface of model.change_decoding_strategy, and the condition under which the GPU cases of
tests/test_ctc_beam_lm_gpu.py mean something (the cap check).  No device."""
import functools
import math
import types

import numpy as np
import pytest
import torch

import ngram_lm_ref as R
from indic_cl_asr_amd import decoding as D
from indic_cl_asr_amd.ngram_lm import NGramLM

INF = float("inf")
ALPHA, BETA = 0.7, 0.5


def load(tmp_path, lm, order, n_tokens, name="lm.arpa", **kw):
    path = tmp_path / name
    R.write_arpa(path, lm, order, **kw)
    return NGramLM.from_arpa(str(path), n_tokens)


# ---------------------------------------------------------------------------------------------------- the reader
SMALL = {("<unk>",): (-2.5, 0.0), ("<s>",): (-99.0, -0.3), (0,): (-0.7, -0.2), (1,): (-0.9, -0.4), (2,): (-1.1, -0.5), (4,): (-1.3, 0.0),
         ("<s>", 0): (-0.4, -0.1), (0, 1): (-0.5, -0.6), (1, 0): (-0.8, 0.0), (2, 1): (-0.3, -0.25), (1, 2): (-0.6, -0.15),
         ("<s>", 0, 1): (-0.2, 0.0), (0, 1, 0): (-0.35, 0.0), (1, 2, 1): (-0.45, 0.0), (2, 1, 4): (-0.15, 0.0)}
SMALL_EXTRA = [(1, "-1.0\t</s>"), (1, "-1.2\tab\t-0.1"), (2, "-0.5\t" + chr(100) + " </s>"), (2, "-0.6\t" + chr(101) + " <s>\t-0.1"),
               (3, "-0.7\t" + chr(100) + " " + chr(101) + " </s>"), (2, "-0.9\t" + chr(100) + " " + chr(100 + 7) + "\t-0.1")]


def test_arpa_round_trip_scores_as_the_dict_formula(tmp_path):
    """Order 3 over the tokens 0 .. 4: token 3 has no unigram (-> <unk>, empty history after it); the context (2, 1) has
    trigrams while its suffix (1,) holds none of them; `ab` and chr(107) are unmapped words, and </s> n-grams and a <s> in
    second position are in the file: dropped and counted.  Every (history up to three tokens, token) scores as the formula."""
    lm = load(tmp_path, SMALL, 3, 5, extra=SMALL_EXTRA)
    assert lm.order == 3 and lm.dropped == len(SMALL_EXTRA) and len(lm.ngrams) == len(SMALL) - 1
    assert lm.nbytes == sum(a.nbytes for a in lm.arrays.values()) > 0
    hists = [()] + [(a,) for a in range(5)] + [(a, b) for a in range(5) for b in range(5)] + [(2, 1, 4), (0, 1, 0), (3, 3, 3)]
    for h in hists:
        for c in range(6):                                                  # 5: beyond the tokens, scored as <unk>
            assert lm.score(h, c) == pytest.approx(float(R.lm_score(SMALL, 3, h, c)), abs=1e-12), (h, c)
    want = float(R.natural(-0.1)) + float(R.natural(-0.2)) + float(R.natural(-2.5))       # bo(<s> 0) + bo(0) + log p(<unk>)
    assert lm.score((0,), 3) == pytest.approx(want, abs=1e-12) and lm.score((0, 3), 1) == pytest.approx(float(R.natural(-0.9)), abs=1e-12)
    assert lm.score((), 0) == pytest.approx(float(R.natural(-0.4)), abs=1e-12)                               # the bigram <s> 0


def test_the_flat_image_walks_to_the_same_scores(tmp_path):
    """The image the kernel reads, walked in numpy the way the kernel builds a row (unigram fill, then the arcs of each chain
    state, shortest first), gives lm.score for every state reached by up to four tokens."""
    for order, n_tok, dens, seed in ((3, 6, 0.4, 1), (5, 5, 0.5, 2), (1, 6, 0.5, 3), (2, 9, 0.3, 4)):
        src = R.random_lm(n_tok, order, dens, seed, skip_unigrams=(2,))
        lm = load(tmp_path, src, order, n_tok, name=f"m{order}.arpa")
        a = lm.arrays
        assert a["states"].shape == (lm.n_states, 3) and a["states"][0].tolist() == [0, 0, 0]
        g = np.random.default_rng(seed)
        for _ in range(60):
            y = [int(v) for v in g.integers(0, n_tok, int(g.integers(0, 5)))]
            s = lm.start
            for c in y:                                                     # the successor as the kernel takes it: from the row
                s = _row(lm, s)[1][c]
            vals, _ = _row(lm, s)
            assert lm.row(y, n_tok + 2).tolist() == [lm.score(y, c) for c in range(n_tok + 2)]      # what the host search adds
            for c in range(n_tok):
                assert vals[c] == pytest.approx(lm.score(y, c), abs=1e-5), (order, y, c)


def _row(lm, s):
    a = lm.arrays
    chain, acc, accs = [], 0.0, []
    while s > 0:
        chain.append(s); accs.append(acc)
        acc += float(a["backoff"][s]); s = int(a["states"][s, 0])
    vals, nxt = acc + a["uni_logp"].astype(np.float64), a["uni_next"].copy()
    for s, ac in zip(chain[::-1], accs[::-1]):
        for k in range(a["states"][s, 1], a["states"][s, 2]):
            vals[a["arcs"][k, 0]] = ac + float(a["arc_logp"][k]); nxt[a["arcs"][k, 0]] = a["arcs"][k, 1]
    return vals, nxt


GOOD = "\\data\\\nngram 1=3\nngram 2=1\n\n\\1-grams:\n-1.0\t<unk>\n-99\t<s>\t-0.5\n-0.5\td\t-0.3\n\n\\2-grams:\n-0.2\t<s> d\n\n\\end\\\n"


@pytest.mark.parametrize("change,line,why", [
    (lambda s: s.replace("ngram 2=1", "ngram 2=2"), 13, "announces 2 2-grams"),
    (lambda s: s.replace("ngram 2=1", "ngram 3=1"), 3, "order 3 after order 1"),
    (lambda s: s.replace("ngram 1=3", "ngram 1=x"), 2, "ngram n=count"),
    (lambda s: s.replace("-0.5\td\t-0.3", "-0.5\td\t-0.3\t7"), 8, "fields"),
    (lambda s: s.replace("-0.5\td\t-0.3", "zero\td\t-0.3"), 8, "not a number"),
    (lambda s: s.replace("-0.5\td\t-0.3", "-inf\td\t-0.3"), 8, "finite"),
    (lambda s: s.replace("\\2-grams:", "\\3-grams:"), 10, "out of order"),
    (lambda s: s.replace("\\2-grams:", "\\two:"), 10, "unknown section"),
    (lambda s: s.replace("\\end\\\n", ""), 11, "no .end"),
    (lambda s: s + "more\n", 14, "after .end"),
    (lambda s: s.replace("-0.2\t<s> d\n", "-0.2\t<s> d\n-0.3\t<s> d\n").replace("ngram 2=1", "ngram 2=2"), 12, "twice"),
    (lambda s: s.replace("\\data\\\n", "\\data\\\n\\data\\\n"), 2, "second"),
])
def test_a_malformed_file_names_its_line(tmp_path, change, line, why):
    p = tmp_path / "bad.arpa"
    p.write_text(change(GOOD), encoding="utf-8")
    with pytest.raises(ValueError, match=f"line {line}: .*{why}"):
        NGramLM.from_arpa(str(p), 8)


def test_files_that_are_refused_whole(tmp_path):
    p = tmp_path / "x.arpa"
    p.write_text(GOOD, encoding="utf-8")
    lm = NGramLM.from_arpa(str(p), 8)
    assert lm.order == 2 and lm.dropped == 0 and lm.score((), 0) == pytest.approx(-0.2 * math.log(10), abs=1e-6)
    assert NGramLM.from_arpa(str(p), 8, vocabulary=["x", "d"]).score((), 1) == pytest.approx(-0.2 * math.log(10), abs=1e-6)
    p.write_text(GOOD.replace("-1.0\t<unk>\n", "").replace("ngram 1=3", "ngram 1=2"), encoding="utf-8")
    with pytest.raises(ValueError, match="<unk>"):
        NGramLM.from_arpa(str(p), 8)
    p.write_text(GOOD.replace("-99\t<s>\t-0.5\n", "").replace("ngram 1=3", "ngram 1=2"), encoding="utf-8")
    with pytest.raises(ValueError, match="prefix"):
        NGramLM.from_arpa(str(p), 8)
    for blob in (b"mmap lm http://kheafield.com/code format version 5\n\x00\x1c\x00\x00\xff\xfe", b"\xff\xfe\x00binary", b"ngram 1=1\n"):
        p.write_bytes(blob)
        with pytest.raises(NotImplementedError, match="kenlm_path.*ARPA only"):
            NGramLM.from_arpa(str(p), 8)


# ---------------------------------------------------------------------------------------------------- the host routine
def _check_host(got, x, lens, W, src, order, lse=None, floor=None, blank=None, alpha=ALPHA, beta=BETA):
    for b in range(x.shape[0]):
        n = int(lens[b])
        e, gap = R.E(x[b, :n].numpy(), W, src, order, alpha, beta, blank=blank, lse=None if lse is None else lse[b, :n].numpy(),
                     token_min_logp=floor)
        assert len(got[b]) == len(e)
        assert max((abs(a[1] - c[1]) for a, c in zip(e, got[b]) if a[1] > -INF or c[1] > -INF), default=0.0) <= 1e-9
        if gap > 1e-9:
            assert [y for y, _ in got[b]] == [y for y, _ in e]


@pytest.mark.parametrize("floor", [None, math.log(0.05)])
@pytest.mark.parametrize("V,W,N,logits", [(5, 1, 2, True), (5, 3, 3, False), (17, 4, 3, True), (17, 16, 5, False), (33, 8, 1, True),
                                          (40, 32, 2, False)])
def test_host_routine_equals_the_restatement(tmp_path, V, W, N, logits, floor):
    g = torch.Generator().manual_seed(V * 100 + W)
    B, T = 4, 24
    x = torch.randn(B, T, V, generator=g) * 3
    x[..., V - 1] += 3
    lse = torch.logsumexp(x, -1) if logits else None
    if not logits:
        x = x.log_softmax(-1)
    lens = torch.tensor([T, 0, 1, T - 5])
    src = R.random_lm(V - 1, N, 0.3, V + N, skip_unigrams=(1,))
    lm = load(tmp_path, src, N, V - 1)
    got = D.beam_ctc_search_host(x, lens, beam_size=W, lse=lse, token_min_logp=floor, lm=lm, beam_alpha=ALPHA, beam_beta=BETA)
    _check_host(got, x, lens, W, src, N, lse, floor)
    assert got[1] == [([], 0.0)]
    if V == 17 and floor is None:
        assert got != D.beam_ctc_search_host(x, lens, beam_size=W, lse=lse)


def test_an_unpruned_search_scores_ctc_plus_alpha_lm_plus_beta_length(tmp_path):
    """V = 3, T = 4, W = 32: no prefix is ever pruned and the LM term depends on (l, c) alone, so every finite hypothesis
    scores ln P_CTC(l) + alpha ln P_LM(l) + beta |l|."""
    g = torch.Generator().manual_seed(5)
    lp = (torch.randn(2, 4, 3, generator=g, dtype=torch.float64) * 2).log_softmax(-1)
    src = R.random_lm(2, 3, 0.6, 11)
    lm = load(tmp_path, src, 3, 2)
    out = D.beam_ctc_search_host(lp, torch.tensor([4, 4]), beam_size=32, lm=lm, beam_alpha=ALPHA, beam_beta=BETA)
    for b in range(2):
        assert len(out[b]) == 31
        for y, s in out[b]:
            want = R.ctc_log_likelihood(lp[b].numpy(), y, 2) + ALPHA * R.lm_sequence(src, 3, y) + BETA * len(y)
            assert (s == want) if want == -INF else abs(s - want) <= 1e-9, (y, s, want)


def test_zero_weights_are_the_search_without_a_model(tmp_path):
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(3, 20, 9, generator=g) * 3).log_softmax(-1)
    lens = torch.tensor([20, 11, 20])
    lm = load(tmp_path, R.random_lm(8, 3, 0.4, 2), 3, 8)
    for kw in ({}, {"token_min_logp": math.log(0.05)}):
        assert D.beam_ctc_search_host(x, lens, beam_size=5, lm=lm, beam_alpha=0.0, beam_beta=0.0, **kw) == \
            D.beam_ctc_search_host(x, lens, beam_size=5, **kw)
    a = D.beam_ctc_decode(x, lens, beam_size=5, lm=lm, beam_alpha=0.0, beam_beta=0.0, return_best_hypothesis=False)
    assert a == D.beam_ctc_decode(x, lens, beam_size=5, return_best_hypothesis=False)


def test_the_model_flips_the_winner_of_two_frames(tmp_path):
    """Two frames [a 0.5, b 0.4, blank 0.1] twice: without a model `a` (0.35) beats `b` (0.24), `a b` (0.20) and `b a` (0.20).
    The model: P(a | <s>) = 0.5, P(b | a) = 0.9, every other token 0.01.  With alpha = 1, beta = 0, `a` (0.35 * 0.5) still
    leads and `a b` (0.2 * 0.5 * 0.9) is second; a bonus of beta = 1.5 per token then puts `a b` first.  The empty prefix
    keeps ln 0.01: stays carry no LM term.  (The file holds log10 values to four decimals: hence 5e-4.)"""
    lp = torch.tensor([[[0.5, 0.4, 0.1], [0.5, 0.4, 0.1]]], dtype=torch.float64).log()
    l10 = math.log10
    src = {("<unk>",): (-4.0, 0.0), ("<s>",): (-99.0, 0.0), (0,): (l10(0.01), 0.0), (1,): (l10(0.01), 0.0),
           ("<s>", 0): (l10(0.5), 0.0), (0, 1): (l10(0.9), 0.0)}
    lm = load(tmp_path, src, 2, 2)
    free = D.beam_ctc_search_host(lp, torch.tensor([2]), beam_size=8)[0]
    assert free[0][0] == [0] and free[0][1] == pytest.approx(math.log(0.35), abs=1e-12)
    one = D.beam_ctc_search_host(lp, torch.tensor([2]), beam_size=8, lm=lm, beam_alpha=1.0, beam_beta=0.0)[0]
    assert one[0][0] == [0] and one[0][1] == pytest.approx(math.log(0.35 * 0.5), abs=5e-4)
    assert one[1][0] == [0, 1] and one[1][1] == pytest.approx(math.log(0.2 * 0.5 * 0.9), abs=5e-4)
    two = D.beam_ctc_search_host(lp, torch.tensor([2]), beam_size=8, lm=lm, beam_alpha=1.0, beam_beta=1.5)[0]
    assert two[0][0] == [0, 1] and two[0][1] == pytest.approx(math.log(0.2 * 0.5 * 0.9) + 3.0, abs=5e-4)
    assert dict((tuple(y), s) for y, s in two)[()] == pytest.approx(math.log(0.01), abs=1e-12)             # stays carry no LM term


# ---------------------------------------------------------------------------------------------------- change_decoding_strategy
@pytest.fixture(scope="module")
def model():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(3)
    return EncDecHybridRNNTCTCModel(model_config("tiny"))


def _tiny_lm(m, tmp_path, name="tiny.arpa", seed=3):
    src = R.random_lm(m.cfg.vocab_per_lang, 3, 0.05, seed)
    path = tmp_path / name
    R.write_arpa(path, src, 3)
    return src, str(path)


def test_change_decoding_strategy_takes_an_arpa_path(model, tmp_path):
    m = model
    la, lb = m.cfg.languages[0], m.cfg.languages[1]
    src, path = _tiny_lm(m, tmp_path)
    beam = lambda **kw: {"strategy": "beam", "beam": kw}
    try:
        m.change_decoding_strategy(beam(kenlm_path=path, beam_alpha=0.6, beam_beta=1.25), "ctc")
        st = m.decoding_strategy["ctc"]
        assert st["kenlm_path"] == path and st["beam_alpha"] == 0.6 and st["beam_beta"] == 1.25
        lm = st["lms"][None]
        assert isinstance(lm, NGramLM) and lm.order == 3 and lm.num_tokens == m.cfg.vocab_per_lang
        m.change_decoding_strategy(beam(beam_size=2), "ctc")                          # the model set before stays, not read again
        assert m.decoding_strategy["ctc"]["lms"][None] is lm and m.decoding_strategy["ctc"]["beam_alpha"] == 0.6
        m.change_decoding_strategy(beam(kenlm_path=None), "ctc")                      # and leaves when told so
        assert "lms" not in m.decoding_strategy["ctc"]
        m.change_decoding_strategy({"strategy": "greedy"}, "ctc")
        cfg = types.SimpleNamespace(strategy="beam", beam=types.SimpleNamespace(kenlm_path={la: path}))      # NeMo's defaults
        m.change_decoding_strategy(cfg, "ctc")
        st = m.decoding_strategy["ctc"]
        assert list(st["lms"]) == [la] and st["beam_alpha"] == 1.0 and st["beam_beta"] == 0.0
        before = (m.cur_decoder, dict(m.decoding_strategy))
        with pytest.raises(NotImplementedError, match="kenlm_path.*binar.*ARPA"):
            m.change_decoding_strategy(beam(kenlm_path=str(tmp_path / "no_such_dir" / "lm.bin")), "ctc")
        with pytest.raises(NotImplementedError, match="kenlm_path"):
            m.change_decoding_strategy(beam(kenlm_path={la: path, lb: "other.binary"}), "ctc")
        with pytest.raises(FileNotFoundError, match="missing.arpa"):
            m.change_decoding_strategy(beam(kenlm_path=str(tmp_path / "missing.arpa")), "ctc")
        with pytest.raises(ValueError, match="xx"):
            m.change_decoding_strategy(beam(kenlm_path={"xx": path}), "ctc")
        for st_ in ("pyctcdecode", "flashlight"):
            with pytest.raises(NotImplementedError, match=st_):
                m.change_decoding_strategy(beam(search_type=st_, kenlm_path=path), "ctc")
        assert (m.cur_decoder, m.decoding_strategy) == before                         # a refusal changes nothing
    finally:
        m.decoding_strategy = {}
        m.cur_decoder = "rnnt"


def test_transcribe_on_the_host_follows_the_model(model, tmp_path):
    """As tests/test_ctc_beam.py does it: seeded encoder outputs stand in for `forward`; the head, the search with the
    language's model and what transcribe does with the results are the model's own."""
    m = model.eval()
    la, lb = m.cfg.languages[0], m.cfg.languages[1]
    src, path = _tiny_lm(m, tmp_path)
    g = torch.Generator().manual_seed(4)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (9000, 6000)]
    enc = torch.randn(2, m.cfg.d_model, 14, generator=g) * 4
    lens = torch.tensor([14, 9])
    monkey = pytest.MonkeyPatch()
    monkey.setattr(m, "forward", lambda input_signal=None, input_signal_length=None, **kw: (enc, lens), raising=False)
    beam = {"beam_size": 3, "return_best_hypothesis": False}
    try:
        m.change_decoding_strategy({"strategy": "beam", "beam": beam}, "ctc")
        _, free = m.transcribe(audio, language_id=la, batch_size=2, return_hypotheses=True)
        m.change_decoding_strategy({"strategy": "beam", "beam": dict(beam, kenlm_path={la: path}, beam_alpha=2.0, beam_beta=1.0)}, "ctc")
        keep = m._beam_keep = []                                                      # the head outputs the search read
        try:
            best, fused = m.transcribe(audio, language_id=la, batch_size=2, return_hypotheses=True)
        finally:
            m._beam_keep = None
        (lp, lse, _), = keep
        assert lse is None and not lp.is_cuda
        V = m.cfg.vocab_per_lang + 1
        want = D.beam_ctc_decode_host(lp, lens, beam_size=3, blank=V - 1, return_best_hypothesis=False,
                                      lm=m.decoding_strategy["ctc"]["lms"][la], beam_alpha=2.0, beam_beta=1.0)
        assert [[(h.y_sequence, h.score) for h in nb.n_best_hypotheses] for nb in fused] == \
            [[(h.y_sequence, h.score) for h in nb.n_best_hypotheses] for nb in want]
        assert all(isinstance(h.text, str) for nb in fused for h in nb.n_best_hypotheses) and best[0] is fused[0].n_best_hypotheses[0]
        _check_host([[(h.y_sequence, h.score) for h in nb.n_best_hypotheses] for nb in fused], lp.detach(), lens, 3, src, 3,
                    alpha=2.0, beta=1.0)
        assert [[h.y_sequence for h in nb.n_best_hypotheses] for nb in fused] != [[h.y_sequence for h in nb.n_best_hypotheses] for nb in free]
        with pytest.raises(ValueError, match=lb):                                     # the mapping has no model for that language
            m.transcribe(audio, language_id=lb, batch_size=2, return_hypotheses=True)
    finally:
        monkey.undo()
        m.decoding_strategy = {}
        m.cur_decoder = "rnnt"


# ---------------------------------------------------------------------------------------------------- the GPU cases, and their cap
# (T, V, W, N) -> the seed of its inputs (tests/test_ctc_beam_gpu.py's construction); chosen on the CPU, with E and F32 alone,
# so that at most 2 of the 8 utterances are undecided under the margin rule in both input modes.  The cap is a condition.
GPU_CASES = {(48, 17, 1, 3): 1, (48, 17, 4, 3): 1, (48, 17, 16, 3): 1, (24, 17, 32, 3): 1, (48, 17, 8, 5): 1, (48, 17, 4, 1): 1,
             (48, 257, 4, 3): 1, (48, 257, 16, 2): 2, (33, 257, 32, 3): 9, (6, 1024, 32, 2): 1}
LENGTHS = lambda T: [T, 0, 1, T, T - 3, T - 10, T, (T + 1) // 2]


@functools.lru_cache(maxsize=None)
def gpu_case(T, V, W, N, logits_mode, seed=None):
    """The inputs of one GPU case and what E and F32 say about them, computed once per session: (xin [8,T,V+7], lse or None,
    lens, the LM dict, E's results, F32's results, the largest |F32 - E|)."""
    seed = GPU_CASES[(T, V, W, N)] if seed is None else seed
    s, ld = (3.0 if V == 17 else 4.0), V + 7
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(8, T, ld, generator=g) * s
    x[..., V - 1] += s
    lens = torch.tensor(LENGTHS(T))
    if logits_mode:
        xin, lse = x, torch.logsumexp(x[..., :V], -1)
    else:
        xin, lse = torch.zeros_like(x), None
        xin[..., :V] = x[..., :V].log_softmax(-1)
        xin[..., V:] = 7.0                                                            # the padding columns are never read
    src = R.random_lm(V - 1, N, 0.3 if V == 17 else 0.02, 1000 * N + V)
    cut = [min(max(int(n), 0), T) for n in lens]
    xs = [xin[b, :cut[b], :V].numpy() for b in range(8)]
    lses = None if lse is None else [lse[b, :cut[b]].numpy() for b in range(8)]
    es, fs, worst = R.margin_of(xs, W, src, N, ALPHA, BETA, V - 1, lses)
    return xin, lse, lens, src, es, fs, worst


def undecided_of(es, worst):
    return sum(1 for e, gap in es if not gap > 16 * worst)


@pytest.mark.parametrize("logits_mode", [True, False])
@pytest.mark.parametrize("T,V,W,N", list(GPU_CASES))
def test_the_gpu_cases_leave_at_most_two_utterances_undecided(T, V, W, N, logits_mode):
    _, _, _, _, es, fs, worst = gpu_case(T, V, W, N, logits_mode)
    assert worst > 0 and undecided_of(es, worst) <= 2, (undecided_of(es, worst), worst)
