"""CTC forced alignment on the host: the project's host routine against the reference aligner's recorded alignments
(tests/golden/ctc_align_cases.npz, exact: the inputs lie on a grid where every fp32 addition is exact), the time / word /
CTM rules, and model.align on the CPU."""
import pytest
import torch

from ctc_align_fixture import assert_case, assert_valid_alignment, load_cases, make_batch

from indic_cl_asr_amd import align as A


@pytest.fixture(scope="module")
def golden():
    return load_cases()


@pytest.mark.parametrize("logits_mode", [False, True])
def test_host_routine_reproduces_every_fixture_case(golden, logits_mode):
    cases, _ = golden
    assert len(cases) == 39 and sum(c["path"] is None for c in cases) == 5
    for c in cases:
        x, lse, tg, il, tl = make_batch([c], logits_mode)
        path, spans, score = A.ctc_forced_align(x, il, tg, tl, c["blank"], lse=lse)
        assert path.dtype == torch.int32 and spans.dtype == torch.int32 and score.dtype == torch.float32
        assert_case(c, path[0].numpy(), spans[0].numpy(), float(score[0]))


def test_host_routine_ragged_batch(golden):
    """The batch of 4 with T_b < T: every utterance as if it were alone, nothing leaks from the padding (+7 there)."""
    cases, batch = golden
    group = [cases[i] for i in batch]
    x, lse, tg, il, tl = make_batch(group, True, T=max(c["lp"].shape[0] for c in group) + 3)
    path, spans, score = A.ctc_forced_align(x, il, tg, tl, group[0]["blank"], lse=lse)
    for b, c in enumerate(group):
        assert_case(c, path[b].numpy(), spans[b].numpy(), float(score[b]))


def test_times_words_and_ctm(tmp_path):
    # states:            0  1  1  2  3  5  5  5  6   (tokens 7, 8, 9 at states 1, 3, 5)
    path = torch.tensor([[0, 1, 1, 2, 3, 5, 5, 5, 6, -1]], dtype=torch.int32)
    spans = A.spans_of_path(path, 3)
    assert spans.tolist() == [[[1, 2], [4, 4], [5, 7]]]
    al, = A.build_alignments(path, spans, torch.tensor([-12.5]), [[7, 8, 9]], 0.04)
    assert al.feasible and al.score == -12.5 and al.frames == [0, 1, 1, 2, 3, 5, 5, 5, 6] and al.words == []
    assert [(t.id, t.text, t.first_frame, t.last_frame) for t in al.tokens] == [(7, "7", 1, 2), (8, "8", 4, 4), (9, "9", 5, 7)]
    assert [round(t.t_start, 6) for t in al.tokens] == [0.04, 0.16, 0.20]
    assert [round(t.t_end, 6) for t in al.tokens] == [0.12, 0.20, 0.32]
    A.write_ctm(str(tmp_path / "tok.ctm"), ["utt0"], [al], level="token")
    assert (tmp_path / "tok.ctm").read_text() == "utt0 1 0.04 0.08 7\nutt0 1 0.16 0.04 8\nutt0 1 0.20 0.12 9\n"
    A.write_ctm(str(tmp_path / "w.ctm"), ["utt0"], [al], level="word")
    assert (tmp_path / "w.ctm").read_text() == ""
    with pytest.raises(ValueError):
        A.write_ctm(str(tmp_path / "x.ctm"), ["utt0"], [al], level="segment")
    with pytest.raises(ValueError):
        A.write_ctm(str(tmp_path / "x.ctm"), ["utt0", "utt1"], [al])
    bad, = A.build_alignments(torch.full((1, 4), -1, dtype=torch.int32), torch.full((1, 2, 2), -1, dtype=torch.int32),
                              torch.tensor([float("-inf")]), [[1, 2]], 0.04)
    assert not bad.feasible and bad.tokens == [] and bad.frames == [] and bad.score == float("-inf")


def test_frame_duration_is_40_ms():
    from indic_cl_asr_amd.config import model_config
    assert A.frame_seconds(model_config("tiny")) == pytest.approx(0.04, abs=1e-12)


def test_word_grouping_with_sentencepiece(corpus, tmp_path):
    from indic_cl_asr_amd import data as D
    root, files, texts, durs = corpus
    tok = D.MultilingualTokenizer({"hi": str(root / "hi.model")}, vocab_per_lang=64)
    text = texts[1]                                       # "yah ek pariksha hai"
    ids = tok.text_to_ids(text, "hi")
    n = len(ids)
    path = torch.tensor([[s for i in range(n) for s in (2 * i + 1, 2 * i + 1, 2 * i + 2)]], dtype=torch.int32)   # 3 frames a token
    al, = A.build_alignments(path, A.spans_of_path(path, n), torch.tensor([-1.0]), [ids], 0.04, tok, "hi")
    assert [w.text for w in al.words] == text.split()
    assert [t.text for t in al.tokens] == [tok.sp["hi"].IdToPiece(i) for i in ids]
    starts = [i for i, t in enumerate(al.tokens) if t.text.startswith(A.WORD_START)]
    assert len(starts) == len(al.words)
    for w, first, nxt in zip(al.words, starts, starts[1:] + [n]):
        assert w.t_start == al.tokens[first].t_start and w.t_end == al.tokens[nxt - 1].t_end
    A.write_ctm(str(tmp_path / "w.ctm"), ["u1"], [al])
    lines = (tmp_path / "w.ctm").read_text().splitlines()
    assert [l.split()[-1] for l in lines] == text.split() and all(l.startswith("u1 1 ") for l in lines)
    assert lines[0] == "u1 1 %.2f %.2f %s" % (al.words[0].t_start, al.words[0].t_end - al.words[0].t_start, al.words[0].text)


def _tiny():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(5)
    return EncDecHybridRNNTCTCModel(model_config("tiny", compute_dtype="fp32"))


def test_model_align_argument_errors():
    m = _tiny()
    audio = [torch.zeros(8000)]
    with pytest.raises(ValueError):
        m.align(audio, language_id="hi")                                     # neither transcripts nor token_ids
    with pytest.raises(ValueError):
        m.align(audio, transcripts=["a"], token_ids=[[1]], language_id="hi")  # both
    with pytest.raises(ValueError):
        m.align(audio, token_ids=[[1]])                                      # no language
    with pytest.raises(ValueError):
        m.align(audio, token_ids=[[1], [2]], language_id="hi")               # one audio, two transcripts
    with pytest.raises(ValueError):
        A.ctc_forced_align(torch.zeros(1, 3, 5), torch.tensor([3]), torch.zeros(1, 1, dtype=torch.long), torch.tensor([1]), blank=5)


def _host_front_end(monkeypatch):
    """The log-mel front end is HIP only; on the host the test stands in for its two ops (any features will do: what is
    under test starts at the encoder's output)."""
    from indic_cl_asr_amd import features

    def log_mel(signal, window, fb, n_fft=512, hop=160, **kw):
        win = torch.nn.functional.pad(window, ((n_fft - window.numel()) // 2, (n_fft - window.numel() + 1) // 2))
        p = torch.stft(signal, n_fft, hop_length=hop, window=win, center=True, return_complex=True).abs() ** 2
        return torch.log(fb @ p + 2.0 ** -24)

    def normalize_mask(x, seq_len, spec_aug=None):
        keep = (torch.arange(x.shape[-1]).unsqueeze(0) < seq_len.unsqueeze(1)).unsqueeze(1)
        n = seq_len.view(-1, 1, 1).float()
        mean = (x * keep).sum(-1, keepdim=True) / n
        var = (((x - mean) * keep) ** 2).sum(-1, keepdim=True) / (n - 1).clamp(min=1)
        return ((x - mean) / (var.sqrt() + 1e-5)) * keep

    monkeypatch.setattr(features.ops, "log_mel", log_mel)
    monkeypatch.setattr(features.ops, "normalize_mask", normalize_mask)


def test_model_align_cpu_token_ids(monkeypatch):
    _host_front_end(monkeypatch)
    m = _tiny().train()
    f = m.preprocessor.featurizer
    f.dither, f.pad_to = 1e-5, 16
    g = torch.Generator().manual_seed(0)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (16000, 9000, 12000)]
    ids = [[3, 3, 7, 1], [], [15, 0, 2, 2, 2, 9]]
    keep = []
    out = m.align(audio, token_ids=ids, language_id="ta", batch_size=2, _keep=keep)
    assert m.training and f.dither == 1e-5 and f.pad_to == 16               # restored
    assert len(out) == 3 and len(keep) == 2 and all(a.feasible for a in out)
    blank = m.cfg.vocab_per_lang
    k = 0
    for x, lse, enc_len, tg, tg_len in keep:
        assert lse is None and x.shape[-1] == blank + 1                     # the head's own log-probs
        path, spans, score = A.ctc_forced_align_host(x, enc_len, tg, tg_len, blank)
        for b in range(x.shape[0]):
            a, y, n = out[k], ids[k], int(enc_len[b])
            assert a.frames == path[b, :n].tolist() and a.score == float(score[b])
            assert_valid_alignment(a.frames, y, blank)
            assert [t.id for t in a.tokens] == y and [t.text for t in a.tokens] == [str(i) for i in y] and a.words == []
            assert [[t.first_frame, t.last_frame] for t in a.tokens] == spans[b, :len(y)].tolist()
            for t in a.tokens:
                assert t.t_start == t.first_frame * 0.04 and t.t_end == (t.last_frame + 1) * 0.04
                assert all(a.frames[i] == 2 * a.tokens.index(t) + 1 for i in range(t.first_frame, t.last_frame + 1))
            # the path's score is the sum of the head's log-probs along it
            ext = [blank if s % 2 == 0 else y[s // 2] for s in range(2 * len(y) + 1)]
            resc = sum(float(x[b, t, ext[s]]) for t, s in enumerate(a.frames))
            assert a.score == pytest.approx(resc, rel=1e-5)
            k += 1
    assert out[1].frames == [0] * len(out[1].frames) and out[1].tokens == []   # empty transcript: every frame in state 0
