"""CTC forced alignment on the MI355X (csrc/ctc_align.hip): the kernel through its C ABI against the reference aligner's
recorded alignments (exact), unquantised inputs against an fp64 optimum (bounded), model.align against the host routine."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from ctc_align_fixture import assert_case, assert_valid_alignment, best_and_rescored_fp64, load_cases, make_batch, spans_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return load_cases()


def _call(x, ld, lse, tg, il, tl, V, blank, ws_bytes=None):
    """ia_ctc_align through ctypes on host tensors x [B,T,ld] ...: (status, path, spans, score) back on the host."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    B, T, S = x.shape[0], x.shape[1], tg.shape[1]
    xd, tgd, ild, tld = x.cuda().contiguous(), tg.cuda().contiguous(), il.cuda(), tl.cuda()
    lsed = lse.cuda().contiguous() if lse is not None else None
    n = L.ia_ctc_align_workspace_bytes(B, T, S) if ws_bytes is None else ws_bytes
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device="cuda")
    path = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    spans = torch.full((B, S, 2), -7, dtype=torch.int32, device="cuda")
    score = torch.full((B,), 123.0, dtype=torch.float32, device="cuda")
    st = L.ia_ctc_align(_lib.ptr(xd), ld, _lib.ptr(lsed), _lib.ptr(tgd), _lib.ptr(ild), _lib.ptr(tld), B, T, V, S, blank,
                        _lib.ptr(path), _lib.ptr(spans), _lib.ptr(score), _lib.ptr(ws), n, _lib.stream_ptr())
    torch.cuda.synchronize()
    return st, path.cpu().numpy(), spans.cpu().numpy(), score.cpu().numpy()


@pytest.mark.parametrize("logits_mode", [False, True])
def test_kernel_reproduces_every_fixture_case(golden, logits_mode):
    """(a) every utterance alone (so that each runs on the template its own S selects: K = 1, 2, 4, 8), V = 257 cases with
    the head's row stride 264; lse = NULL on log-probs, and logits with lse.  Exact: see the fixture script."""
    cases, _ = golden
    for c in cases:
        ld = 264 if c["V"] == 257 else c["V"]
        x, lse, tg, il, tl = make_batch([c], logits_mode, ld=ld)
        st, path, spans, score = _call(x, ld, lse, tg, il, tl, c["V"], c["blank"])
        assert st == 0, c["name"]
        assert_case(c, path[0], spans[0], float(score[0]))


@pytest.mark.parametrize("logits_mode", [False, True])
def test_kernel_ragged_batch(golden, logits_mode):
    """(a) the batch of 4: T_b < T, lengths that are no multiples of the prefetch depth, an empty transcript among them;
    S padded beyond every transcript."""
    cases, batch = golden
    group = [cases[i] for i in batch]
    T = max(c["lp"].shape[0] for c in group) + 3
    x, lse, tg, il, tl = make_batch(group, logits_mode, T=T, S=33)
    st, path, spans, score = _call(x, 33, lse, tg, il, tl, 33, 32)
    assert st == 0
    for b, c in enumerate(group):
        assert_case(c, path[b], spans[b], float(score[b]))
    # an infeasible utterance and one without frames among feasible ones: they alone come back -inf / -1
    il2 = il.clone(); il2[0] = 5; il2[2] = 0
    st, path2, spans2, score2 = _call(x, 33, lse, tg, il2, tl, 33, 32)
    assert st == 0
    for b in (0, 2):
        assert score2[b] == -np.inf and np.all(path2[b] == -1) and np.all(spans2[b] == -1)
    for b in (1, 3):
        assert_case(group[b], path2[b], spans2[b], float(score2[b]))


def test_abi_argument_checks(golden):
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    cases, _ = golden
    c = next(c for c in cases if c["name"] == "random_T5_S2")
    x, lse, tg, il, tl = make_batch([c], False)
    assert L.ia_ctc_align_max_targets() == 255
    assert L.ia_ctc_align_workspace_bytes(1, 5, 255) == 5 * 128 + 128 and L.ia_ctc_align_workspace_bytes(1, 5, 256) == 0
    assert L.ia_ctc_align_workspace_bytes(0, 5, 2) == 0
    tg256 = torch.zeros(1, 256, dtype=torch.long)
    assert _call(x, 33, None, tg256, il, tl, 33, 32, ws_bytes=4096)[0] == -4          # IA_UNSUPPORTED: S > 255
    assert _call(x, 33, None, tg, il, tl, 33, 33)[0] == -1                            # blank outside the classes
    assert _call(x, 32, None, tg, il, tl, 33, 32)[0] == -1                            # ld < V
    assert _call(x, 33, None, tg, il, tl, 33, 32, ws_bytes=128)[0] == -2              # IA_WORKSPACE_TOO_SMALL
    z = ctypes.c_void_p(None)
    xd = x.cuda()
    assert L.ia_ctc_align(z, 33, z, z, z, z, 1, 5, 33, 2, 32, z, z, z, z, 0, _lib.stream_ptr()) == -1
    assert L.ia_ctc_align(_lib.ptr(xd), 33, z, z, z, z, 1, 5, 33, 2, 32, z, z, z, z, 0, _lib.stream_ptr()) == -1


@pytest.mark.parametrize("B,T,V,S", [(4, 160, 257, 40), (2, 376, 257, 105)])
def test_unquantised_inputs_within_fp32_bound(B, T, V, S):
    """(b) randn * 3 logits in the head's [B*T, 264] layout, lse from ia_ctc_row_lse, ragged lengths.  The fp32 recurrence
    returns the maximum over alignments of each alignment's fp32 sum (rounding is monotone), and each such sum is within
    T_b 2^-24 |sum| of exact (T_b - 1 additions of same-sign terms), so the chosen path, rescored in fp64, is within
    2 T_b 2^-24 |rescored| of the fp64 optimum, and the reported score within T_b 2^-24 |rescored| of the rescored one."""
    from indic_cl_asr_amd import align as A
    g = torch.Generator().manual_seed(T + S)
    buf = torch.randn(B * T, 264, generator=g) * 3
    x = buf.cuda().view(B, T, 264)[..., :V]
    tg = torch.randint(0, V - 1, (B, S), generator=g)
    for i in range(2, S, 3):
        tg[:, i] = tg[:, i - 1]                                      # repeats: forbidden skips
    il = torch.tensor([T - 37 * b for b in range(B)])
    tl = torch.tensor([S - 7 * b for b in range(B)])
    lse = A.row_lse(x)
    assert torch.allclose(lse.cpu(), torch.logsumexp(buf.view(B, T, 264)[..., :V], -1), atol=1e-4)
    path, spans, score = (t.cpu().numpy() for t in A.ctc_forced_align(x, il.cuda(), tg.cuda(), tl.cuda(), V - 1, lse=lse))
    q32 = (buf.view(B, T, 264)[..., :V] - lse.cpu().unsqueeze(-1)).numpy()      # the fp32 value the kernel adds per frame
    for b in range(B):
        n, y = int(il[b]), tg[b, :int(tl[b])].numpy()
        assert np.all(path[b, n:] == -1)
        assert_valid_alignment(path[b, :n], y, V - 1)
        best64, rescored = best_and_rescored_fp64(q32[b, :n], y, V - 1, path[b, :n])
        gap, eps = best64 - rescored, n * 2.0 ** -24 * abs(rescored)
        print(f"b={b} T_b={n} S_b={len(y)}: best64={best64:.6f} rescored={rescored:.6f} gap={gap:.3e} "
              f"score={float(score[b]):.6f} |score-rescored|={abs(float(score[b]) - rescored):.3e} eps={eps:.3e}")
        assert -1e-9 <= gap <= 2 * eps           # (below zero only by the fp64 roundoff of two summation orders)
        assert abs(float(score[b]) - rescored) <= eps
        assert np.array_equal(spans[b, :len(y)], spans_of(path[b, :n], len(y))) and np.all(spans[b, len(y):] == -1)


def test_beyond_the_limit_runs_on_the_host_with_a_warning():
    from indic_cl_asr_amd import align as A
    g = torch.Generator().manual_seed(1)
    B, T, V, S = 1, 270, 17, 256
    x = torch.randn(B, T, V, generator=g).log_softmax(-1)
    tg = (torch.arange(S) % (V - 1)).view(1, S)                      # no repeats: feasible from T = 256
    il, tl = torch.tensor([T]), torch.tensor([S])
    A._warned_limit = False
    with pytest.warns(UserWarning, match="255"):
        got = A.ctc_forced_align(x.cuda(), il.cuda(), tg.cuda(), tl.cuda(), V - 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                               # one time only
        A.ctc_forced_align(x.cuda(), il.cuda(), tg.cuda(), tl.cuda(), V - 1)
    ref = A.ctc_forced_align_host(x, il, tg, tl, V - 1)
    assert all(a.is_cuda and torch.equal(a.cpu(), r) for a, r in zip(got, ref)) and float(ref[2]) > -np.inf


@pytest.fixture(scope="module")
def model3():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(11)
    return EncDecHybridRNNTCTCModel(model_config("medium", n_layers=3, languages=["hi", "ta"])).cuda()


def test_model_align_equals_host_routine_on_the_device_logits(model3):
    """(c) + (d).  The host routine is fed the very logits and lse the kernel read, copied back.  Both add the same fp32
    numbers in the same order (max of three, plus (logit - lse)) with the same tie-break, so the equality is EXACT -- the
    bound of (b) is not needed here."""
    from indic_cl_asr_amd import align as A
    m = model3.train()
    f = m.preprocessor.featurizer
    f.dither, f.pad_to = 1e-5, 16
    m.cur_decoder = "rnnt"                                            # the aligner uses the CTC head whatever this says
    g = torch.Generator().manual_seed(2)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (24000, 11000, 17000)]
    ids = [[5, 5, 200, 17, 3, 3, 3, 90], [], [255, 0, 31, 31, 8]]
    keep = []
    out = m.align(audio, token_ids=ids, language_id="ta", batch_size=2, _keep=keep)
    assert m.training and f.dither == 1e-5 and f.pad_to == 16 and m.cur_decoder == "rnnt"       # (d)
    assert len(out) == 3 and len(keep) == 2 and all(a.feasible for a in out)
    k = 0
    for x, lse, enc_len, tg, tg_len in keep:
        assert x.is_cuda and x.shape[-1] == 257 and x.stride(1) == 264 and lse is not None     # the head's padded rows, in place
        path, spans, score = A.ctc_forced_align_host(x.cpu(), enc_len.cpu(), tg.cpu(), tg_len.cpu(), 256, lse=lse.cpu())
        for b in range(x.shape[0]):
            a, y, n = out[k], ids[k], int(enc_len[b])
            assert a.frames == path[b, :n].tolist() and a.score == float(score[b])
            assert [[t.first_frame, t.last_frame] for t in a.tokens] == spans[b, :len(y)].tolist()
            assert [t.id for t in a.tokens] == y and a.words == []
            assert_valid_alignment(a.frames, y, 256)
            k += 1
    assert set(out[1].frames) == {0}
    # eval mode, dither off: a second call returns the same alignments
    again = m.align(audio, token_ids=ids, language_id="ta", batch_size=2)
    assert [a.frames for a in again] == [a.frames for a in out]


def test_model_align_transcripts_words_and_ctm(model3, corpus, tmp_path):
    from indic_cl_asr_amd import align as A
    from indic_cl_asr_amd import data as D
    root, files, texts, durs = corpus
    m = model3.eval()
    tok = D.MultilingualTokenizer({"hi": str(root / "hi.model")})
    old = m.tokenizer
    try:
        m.set_tokenizer(tok)
        out = m.align(files[:3], transcripts=texts[:3], language_id="hi", batch_size=2)
    finally:
        m.set_tokenizer(old)
    assert len(out) == 3
    for a, text, dur in zip(out, texts, durs):
        ids = tok.text_to_ids(text, "hi")
        assert a.feasible and [t.id for t in a.tokens] == ids and [w.text for w in a.words] == text.split()
        assert_valid_alignment(a.frames, ids, 256)
        assert all(x.t_end <= y.t_start for x, y in zip(a.tokens[:-1], a.tokens[1:]))
        assert a.tokens[-1].t_end <= len(a.frames) * 0.04 + 1e-9 and abs(len(a.frames) * 0.04 - dur) < 0.08
    A.write_ctm(str(tmp_path / "words.ctm"), ["u0", "u1", "u2"], out)
    lines = (tmp_path / "words.ctm").read_text().splitlines()
    assert [l.split()[-1] for l in lines] == " ".join(texts[:3]).split()
    assert [l.split()[0] for l in lines] == [u for u, t in zip(("u0", "u1", "u2"), texts) for _ in t.split()]
