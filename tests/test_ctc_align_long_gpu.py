"""CTC forced alignment of long transcripts on the MI355X (csrc/ctc_align_long.hip, one workgroup per utterance).  Every check
is an EXACT equality of path, spans and score: against the reference aligner's recorded alignments, against the one-wave
kernel, and against the host routine fed the same fp32 tensors (same additions in the same order, same tie-breaks)."""
import warnings

import numpy as np
import pytest
import torch

from ctc_align_fixture import assert_case, load_cases, make_batch
from ctc_align_long_fixture import load_long_cases, min_frames, repeating_targets

pytestmark = pytest.mark.gpu


def _call(entry, x, ld, lse, tg, il, tl, V, blank):
    """ia_ctc_align / ia_ctc_align_long through ctypes on host tensors x [B,T,ld] ...: (status, path, spans, score) on the host."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    B, T, S = x.shape[0], x.shape[1], tg.shape[1]
    xd, tgd, ild, tld = x.cuda().contiguous(), tg.cuda().contiguous(), il.cuda(), tl.cuda()
    lsed = lse.cuda().contiguous() if lse is not None else None
    n = getattr(L, entry + "_workspace_bytes")(B, T, S)
    ws = torch.empty(max(n, 256), dtype=torch.uint8, device="cuda")
    path = torch.full((B, T), -7, dtype=torch.int32, device="cuda")
    spans = torch.full((B, max(S, 1), 2), -7, dtype=torch.int32, device="cuda")[:, :S]
    score = torch.full((B,), 123.0, dtype=torch.float32, device="cuda")
    st = getattr(L, entry)(_lib.ptr(xd), ld, _lib.ptr(lsed), _lib.ptr(tgd), _lib.ptr(ild), _lib.ptr(tld), B, T, V, S, blank,
                           _lib.ptr(path), _lib.ptr(spans), _lib.ptr(score), _lib.ptr(ws), n, _lib.stream_ptr())
    torch.cuda.synchronize()
    return st, path.cpu().numpy(), spans.cpu().numpy(), score.cpu().numpy()


def _np(a):
    return a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _equal(got, ref):
    """path, spans and score, element for element (-inf equals -inf)."""
    return all(_np(a).shape == _np(r).shape and np.array_equal(_np(a), _np(r)) for a, r in zip(got, ref))


# ------------------------------------------------------------------------------------------------------------ 1. fixture
@pytest.mark.parametrize("logits_mode", [False, True])
def test_long_kernel_reproduces_every_long_fixture_case(logits_mode):
    """Every case alone: S = 256, 512, 600, 1023, 2047 and 4096 select (K, waves) = (4, 4), (4, 8), (4, 16) and (16, 16) -- not
    (8, 16), which the boundary test below holds against the host routine at S = 2048 and 4095; log-probs with lse = NULL, and
    logits with a synthetic lse.  Exact: see the fixture script."""
    for c in load_long_cases():
        x, lse, tg, il, tl = make_batch([c], logits_mode)
        st, path, spans, score = _call("ia_ctc_align_long", x, c["V"], lse, tg, il, tl, c["V"], c["blank"])
        assert st == 0, c["name"]
        assert_case(c, path[0], spans[0], float(score[0]))


# ------------------------------------------------------------------------------------------ 2. against the one-wave kernel
@pytest.mark.parametrize("logits_mode", [False, True])
def test_long_kernel_equals_the_one_wave_kernel_on_its_fixture(logits_mode):
    """Every case of ctc_align_cases.npz (S <= 255) alone, and its ragged batch: bit-identical path, spans and score from
    ia_ctc_align_long and ia_ctc_align."""
    cases, batch = load_cases()
    for c in cases:
        ld = 264 if c["V"] == 257 else c["V"]
        args = make_batch([c], logits_mode, ld=ld)
        one = _call("ia_ctc_align", args[0], ld, *args[1:], c["V"], c["blank"])
        wg = _call("ia_ctc_align_long", args[0], ld, *args[1:], c["V"], c["blank"])
        assert one[0] == 0 and wg[0] == 0, c["name"]
        assert all(np.array_equal(a, b) for a, b in zip(one[1:], wg[1:])), c["name"]
    group = [cases[i] for i in batch]
    T = max(c["lp"].shape[0] for c in group) + 3
    args = make_batch(group, logits_mode, T=T, S=33)
    one = _call("ia_ctc_align", args[0], 33, *args[1:], 33, 32)
    wg = _call("ia_ctc_align_long", args[0], 33, *args[1:], 33, 32)
    assert one[0] == 0 and wg[0] == 0
    assert all(np.array_equal(a, b) for a, b in zip(one[1:], wg[1:]))
    for b, c in enumerate(group):
        assert_case(c, wg[1][b], wg[2][b], float(wg[3][b]))


# ------------------------------------------------------------------------------------- 3. boundaries of the decomposition
def _head_layout_case(S, V, seed):
    """randn * 3 logits in the head's [B*T, 264] layout (V = 257) narrowed to V columns, lse from ia_ctc_row_lse, repeats at every
    third target, T = minimum feasible + 5: (x [1,T,V] device view, lse device, targets, lens)."""
    from indic_cl_asr_amd import align as A
    g = torch.Generator().manual_seed(seed)
    tg = repeating_targets(g, 1, S, V)
    T = max(min_frames(tg[0].numpy()), 1) + 5
    buf = torch.randn(T, 264, generator=g) * 3
    x = buf.cuda().view(1, T, 264)[..., :V]
    return x, A.row_lse(x), tg, torch.tensor([T]), torch.tensor([S])


@pytest.mark.parametrize("S", [0, 1, 31, 32, 33, 63, 64, 127, 128, 255, 256, 511, 512, 1023, 1024, 2047, 2048, 4095, 4096])
def test_long_kernel_equals_host_routine_at_the_boundaries(S):
    """Unquantised inputs, exact equality with ctc_forced_align_host on the same fp32 logits and lse.  The kernel's (K, waves)
    is (4, 1) up to S = 127, (4, 2) to 255, (4, 4) to 511, (4, 8) to 1023, (4, 16) to 2047, (8, 16) to 4095 and (16, 16) to 8191:
    both sides of each change are here (S = 127/128, 255/256, 511/512, 1023/1024, 2047/2048, 4095/4096), with sizes that end
    inside a wave (31 ... 64: 63 to 129 states) and inside a lane.  T = minimum feasible + 5 is no multiple of the prefetch
    depth (4) or of the backtrace window (16) in general, and the path has little slack: skips and forbidden skips everywhere."""
    from indic_cl_asr_amd import align as A
    x, lse, tg, il, tl = _head_layout_case(S, 257, 1000 + S)
    S_pad = max(S, 1)                                                 # the padded width the collate would give
    tgp = torch.zeros(1, S_pad, dtype=torch.long); tgp[:, :S] = tg
    got = A.ctc_forced_align_long(x, il.cuda(), tgp.cuda(), tl.cuda(), 256, lse=lse)
    ref = A.ctc_forced_align_host(x.cpu(), il, tgp, tl, 256, lse=lse.cpu())
    assert float(ref[2]) > -np.inf
    assert all(t.is_cuda for t in got) and _equal(got, ref), S


def test_long_kernel_with_targets_of_width_zero():
    """S = 0 itself (the boundary test pads its empty transcript to width 1): a [1, 0] target tensor and no spans buffer.  Every
    frame is in state 0 and the score is the host routine's for the same utterance at width 1."""
    from indic_cl_asr_amd import align as A
    x, lse, _, il, tl = _head_layout_case(0, 257, 1000)
    T = x.shape[1]
    buf = torch.zeros(1, T, 264); buf[..., :257] = x.cpu()
    st, path, spans, score = _call("ia_ctc_align_long", buf, 264, lse.cpu(), torch.zeros(1, 0, dtype=torch.long), il, tl, 257, 256)
    ref = A.ctc_forced_align_host(x.cpu(), il, torch.zeros(1, 1, dtype=torch.long), tl, 256, lse=lse.cpu())
    assert st == 0 and spans.shape == (1, 0, 2)
    assert np.array_equal(path, ref[0].numpy()) and np.all(path == 0)
    assert np.array_equal(score, ref[2].numpy()) and score[0] > -np.inf


def test_long_kernel_at_the_limit_of_k16():
    """S = 8191 (L = 16383 of the 16384 states of 1024 lanes x 16), V = 33, log-probs without lse."""
    from indic_cl_asr_amd import align as A
    assert A.max_targets_long() >= 8191
    g = torch.Generator().manual_seed(8191)
    S, V = 8191, 33
    tg = repeating_targets(g, 1, S, V)
    T = min_frames(tg[0].numpy()) + 5
    x = (torch.randn(1, T, V, generator=g) * 3).log_softmax(-1)
    il, tl = torch.tensor([T]), torch.tensor([S])
    got = A.ctc_forced_align_long(x.cuda(), il.cuda(), tg.cuda(), tl.cuda(), V - 1)
    ref = A.ctc_forced_align_host(x, il, tg, tl, V - 1)
    assert float(ref[2]) > -np.inf and _equal(got, ref)


# ------------------------------------------------------------------------------------------ 4. full width, ragged lengths
def test_full_width_infeasible_utterance():
    from indic_cl_asr_amd import align as A
    g = torch.Generator().manual_seed(4)
    S, T, V = A.max_targets_long(), 64, 33
    x = torch.randn(1, T, V, generator=g).log_softmax(-1)
    tg = torch.randint(0, V - 1, (1, S), generator=g)
    st, path, spans, score = _call("ia_ctc_align_long", x, V, None, tg, torch.tensor([T]), torch.tensor([S]), V, V - 1)
    assert st == 0                                                    # IA_OK
    assert score[0] == -np.inf and np.all(path == -1) and np.all(spans == -1)


def _ragged_batch(seed=7, S=300, V=33):
    g = torch.Generator().manual_seed(seed)
    tg = repeating_targets(g, 4, S, V)
    T = max(min_frames(tg[b].numpy()) for b in range(4)) + 11
    x = (torch.randn(4, T, V, generator=g) * 3).log_softmax(-1)
    il = torch.tensor([T, 0, -3, T + 9])                               # clamped to [0, T]
    tl = torch.tensor([S, 5, S + 4, 0])                                # clamped to [0, S]
    return x, tg, il, tl, T, S, V


def test_ragged_batch_clamps_and_empty_utterances_match_the_host():
    from indic_cl_asr_amd import align as A
    x, tg, il, tl, T, S, V = _ragged_batch()
    st, path, spans, score = _call("ia_ctc_align_long", x, V, None, tg, il, tl, V, V - 1)
    ref = A.ctc_forced_align_host(x, il, tg, tl, V - 1)
    assert st == 0 and _equal((path, spans, score), ref)
    assert score[0] > -np.inf and score[1] == -np.inf and score[2] == -np.inf and score[3] > -np.inf
    assert np.all(path[3] == 0) and np.all(spans[3] == -1)             # an empty transcript: every frame in state 0
    assert np.all(path[1] == -1) and np.all(path[2] == -1)


# ------------------------------------------------------------------------------------------ 5. two launches
def test_two_launches_are_bit_identical_and_padding_is_minus_one():
    g = torch.Generator().manual_seed(9)
    B, S, V = 3, 700, 33
    tg = repeating_targets(g, B, S, V)
    tl = torch.tensor([S, S - 123, 257])
    T = min_frames(tg[0].numpy()) + 70
    il = torch.tensor([T, T - 64, T - 300])
    x = (torch.randn(B, T, V, generator=g) * 3).log_softmax(-1)
    a = _call("ia_ctc_align_long", x, V, None, tg, il, tl, V, V - 1)
    b = _call("ia_ctc_align_long", x, V, None, tg, il, tl, V, V - 1)
    assert a[0] == 0 and b[0] == 0 and all(np.array_equal(p, q) for p, q in zip(a[1:], b[1:]))
    _, path, spans, score = a
    for i in range(B):
        n, m = int(il[i]), int(tl[i])
        assert score[i] > -np.inf
        assert np.all(path[i, n:] == -1) and np.all(path[i, :n] >= 0) and path[i, n - 1] in (2 * m - 1, 2 * m)
        assert np.all(spans[i, m:] == -1) and np.all(spans[i, :m] >= 0)


# ------------------------------------------------------------------------------------------ 6. model level
@pytest.fixture(scope="module")
def model3():
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(11)
    return EncDecHybridRNNTCTCModel(model_config("medium", n_layers=3, languages=["hi", "ta"])).cuda()


def _align_and_check(m, audio, ids, batch_size):
    """model.align raises no warning and returns, exactly, what the host routine computes from the logits and lse the kernel
    read."""
    from indic_cl_asr_amd import align as A
    keep = []
    A._warned_limit = A._warned_limit_long = False                      # the warnings are one-time: a fall-back must be heard here
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = m.align(audio, token_ids=ids, language_id="ta", batch_size=batch_size, _keep=keep)
    assert len(out) == len(audio)
    k = 0
    for x, lse, enc_len, tg, tg_len in keep:
        assert x.is_cuda and x.shape[-1] == 257 and x.stride(1) == 264 and lse is not None
        assert tg.shape[1] > A.max_targets()                            # the batch is beyond the one-wave kernel
        path, spans, score = A.ctc_forced_align_host(x.cpu(), enc_len.cpu(), tg.cpu(), tg_len.cpu(), 256, lse=lse.cpu())
        for b in range(x.shape[0]):
            a, y, n = out[k], ids[k], int(enc_len[b])
            assert a.feasible and a.frames == path[b, :n].tolist() and a.score == float(score[b])
            assert [[t.first_frame, t.last_frame] for t in a.tokens] == spans[b, :len(y)].tolist()
            assert [t.id for t in a.tokens] == y
            k += 1
    assert k == len(audio)
    return out


def test_model_align_long_transcripts_stay_on_the_device(model3):
    m = model3.train()
    f = m.preprocessor.featurizer
    f.dither, f.pad_to = 1e-5, 16
    g = torch.Generator().manual_seed(3)
    audio = [torch.randn(n, generator=g) * 0.1 for n in (30 * 16000, 12 * 16000)]
    ids = [torch.randint(0, 256, (n,), generator=g).tolist() for n in (300, 20)]
    _align_and_check(m, audio, ids, batch_size=2)
    assert m.training and f.dither == 1e-5 and f.pad_to == 16
    # the documented long-recording recipe end to end: local attention, one long clip, a transcript of 1200 tokens
    m.change_attention_model("rel_pos_local_attn", att_context_size=[64, 64])
    try:
        audio = [torch.randn(120 * 16000, generator=g) * 0.1]
        ids = [torch.randint(0, 256, (1200,), generator=g).tolist()]
        out = _align_and_check(m, audio, ids, batch_size=1)
        assert len(out[0].frames) >= 2999 and len(out[0].tokens) == 1200
        assert m.training and f.dither == 1e-5 and f.pad_to == 16
    finally:
        m.change_attention_model("rel_pos")


# ------------------------------------------------------------------------------------------ 7. beyond the limit
def test_beyond_the_long_limit_runs_on_the_host_with_a_warning():
    from indic_cl_asr_amd import align as A
    g = torch.Generator().manual_seed(1)
    limit = A.max_targets_long()
    B, T, V, S = 1, 8, 17, limit + 1
    x = torch.randn(B, T, V, generator=g).log_softmax(-1)
    tg = torch.randint(0, V - 1, (B, S), generator=g)
    il, tl = torch.tensor([T]), torch.tensor([S])
    A._warned_limit_long = False
    with pytest.warns(UserWarning, match=str(limit)):
        got = A.ctc_forced_align_long(x.cuda(), il.cuda(), tg.cuda(), tl.cuda(), V - 1)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                               # one time only
        A.ctc_forced_align_long(x.cuda(), il.cuda(), tg.cuda(), tl.cuda(), V - 1)
    ref = A.ctc_forced_align_host(x, il, tg, tl, V - 1)
    assert all(a.is_cuda for a in got) and _equal(got, ref) and float(ref[2]) == -np.inf
