"""CTC forced alignment: which frames each token of a known transcript occupies, the path's log-probability, CTM files.

The semantics are those of the forced aligner the reference's NeMo ships for this model family
(tools/nemo_forced_aligner: utils/viterbi_decoding.py:19-136 run on one utterance alone, the time rule of
utils/data_prep.py:588-672, the CTM lines of utils/make_ctm_files.py:82-119).  What differs in HOW: the Viterbi pass is one
launch of csrc/ctc_align.hip (one wave per utterance, backpointers and backtrace on the device; transcripts beyond its 255
tokens: one workgroup per utterance, csrc/ctc_align_long.hip) instead of T Python iterations of batched torch ops and a host
backtrace, and it reads the CTC head's raw logits + per-frame log-sum-exp.

  v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2) if s is odd and label(s) != label(s-2)) + q_t(label(s))

over the extended label sequence (L = 2 S_b + 1 states: blank at even positions, token i at state 2i+1), in fp32, with
torch.max's tie-break: the first maximum of [stay, s-1, s-2] wins; at the end state L-2 beats L-1; L = 1 ends in state 0.
"""
import warnings
from dataclasses import dataclass, field
from typing import List

import numpy as np
import torch

from . import _lib

SUBSAMPLING_FACTOR = 4          # the encoder's striding subsampling: one output frame per 4 feature frames
WORD_START = "▁"           # SentencePiece's word-start marker


@dataclass
class TokenSpan:
    id: int
    text: str
    t_start: float
    t_end: float
    first_frame: int
    last_frame: int


@dataclass
class WordSpan:
    text: str
    t_start: float
    t_end: float


@dataclass
class UtteranceAlignment:
    tokens: List[TokenSpan] = field(default_factory=list)
    words: List[WordSpan] = field(default_factory=list)
    score: float = float("-inf")          # log-prob of the best path
    frames: List[int] = field(default_factory=list)   # extended-label state of every frame (empty when infeasible)
    feasible: bool = False


# ---------------------------------------------------------------------------------------------------------- host routine
def ctc_forced_align_host(x, input_lens, targets, target_lens, blank, lse=None):
    """The alignment on the host, vectorised over the batch (one torch op per frame and candidate, as
    decoding.greedy_rnnt_decode_host is): same semantics, same arithmetic order and same tie-break as csrc/ctc_align.hip.
    x [B,T,V] f32 log-probs, or logits with lse [B,T]; returns (path [B,T] i32, spans [B,S,2] i32, score [B] f32)."""
    x = x.detach().float().cpu()
    B, T, V = x.shape
    targets = targets.detach().long().cpu().reshape(B, -1)
    S = targets.shape[1]
    Tb = input_lens.detach().long().cpu().reshape(B).clamp(0, T)
    Sb = target_lens.detach().long().cpu().reshape(B).clamp(0, S)
    Lmax = 2 * S + 1
    pos = torch.arange(Lmax)
    Lb = (2 * Sb + 1).unsqueeze(1)
    valid = pos.unsqueeze(0) < Lb                                        # [B,Lmax]
    ext = torch.full((B, Lmax), int(blank), dtype=torch.long)
    if S > 0:
        ext[:, 1::2] = targets.clamp(0, V - 1)
    ext = torch.where(valid, ext, torch.full_like(ext, int(blank)))
    skip = torch.zeros(B, Lmax, dtype=torch.bool)
    if Lmax >= 4:
        skip[:, 3::2] = ext[:, 3::2] != ext[:, 1:-2:2]
    skip &= valid
    z = None if lse is None else lse.detach().float().cpu().reshape(B, T)
    ninf = torch.tensor(float("-inf"))

    def q_at(t):
        q = x[:, t, :].gather(1, ext)
        return q if z is None else q - z[:, t:t + 1]

    v = torch.where((pos.unsqueeze(0) < 2) & valid, q_at(0), ninf) if T > 0 else ninf.expand(B, Lmax)
    bps = torch.zeros(B, max(T, 1), Lmax, dtype=torch.int8)
    for t in range(1, T):
        a1 = torch.cat([ninf.expand(B, 1), v[:, :-1]], 1) if Lmax > 1 else ninf.expand(B, Lmax)
        a2 = torch.cat([ninf.expand(B, 2), v[:, :-2]], 1) if Lmax > 2 else ninf.expand(B, Lmax)
        a2 = torch.where(skip, a2, ninf)
        m, bp = v, torch.zeros(B, Lmax, dtype=torch.int8)     # the first maximum wins: a later candidate needs strictly more
        take = a1 > m
        m, bp = torch.where(take, a1, m), torch.where(take, torch.ones_like(bp), bp)
        take = a2 > m
        m, bp = torch.where(take, a2, m), torch.where(take, torch.full_like(bp, 2), bp)
        new = torch.where(valid, m + q_at(t), ninf)
        live = (t < Tb).unsqueeze(1)                             # a shorter utterance keeps the values of its last frame
        v = torch.where(live, new, v)
        bps[:, t] = bp
    rows = torch.arange(B)
    last = v.gather(1, (2 * Sb).unsqueeze(1)).squeeze(1)                              # state L-1
    tok = v.gather(1, (2 * Sb - 1).clamp(min=0).unsqueeze(1)).squeeze(1)              # state L-2
    take_tok = (Sb > 0) & (tok >= last)
    score = torch.where(take_tok, tok, last)
    score = torch.where(Tb > 0, score, ninf)
    s = torch.where(take_tok, 2 * Sb - 1, 2 * Sb)
    feasible = score != float("-inf")
    path = torch.full((B, T), -1, dtype=torch.int64)
    for t in range(T - 1, 0, -1):
        live = feasible & (t < Tb)
        path[:, t] = torch.where(live, s, path[:, t])
        s = torch.where(live, s - bps[rows, t, s].long(), s)
    if T > 0:
        path[:, 0] = torch.where(feasible, s, path[:, 0])
    path = path.to(torch.int32)
    return path, spans_of_path(path, S), score.float()


def spans_of_path(path, S):
    """[B,S,2] i32: first and last frame of every odd (token) state of path [B,T]; -1 where the token does not occur."""
    p = path.cpu().numpy()
    out = np.full((p.shape[0], S, 2), -1, dtype=np.int32)
    for b in range(p.shape[0]):
        idx = np.nonzero((p[b] >= 0) & (p[b] & 1 == 1))[0]
        tok = p[b, idx] >> 1
        out[b, tok[::-1], 0] = idx[::-1]     # descending frames: the earliest is written last
        out[b, tok, 1] = idx
    return torch.from_numpy(out)


# ---------------------------------------------------------------------------------------------------------- device
_warned_limit = False


def max_targets():
    """Longest transcript (tokens) the kernel takes; beyond it ctc_forced_align runs the host routine."""
    return int(_lib.lib().ia_ctc_align_max_targets())


def row_lse(logits):
    """Per-frame log-sum-exp [B,T] f32 of device logits [B,T,V] (a view with 8-padded rows is read in place)."""
    x, ld = _rows_in_place(logits)
    B, T, V = x.shape
    lse = torch.empty(B, T, dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().ia_ctc_row_lse(_lib.ptr(x), ld, B * T, V, _lib.ptr(lse), _lib.stream_ptr()), "ia_ctc_row_lse")
    return lse


def _rows_in_place(x):
    """(tensor, row stride) such that frame (b,t) starts at element (b*T + t) * ld: the head's [M,264] logits narrowed to
    their valid columns pass as they are, anything else is made contiguous."""
    B, T, V = x.shape
    if x.dtype == torch.float32 and x.stride(2) == 1 and x.stride(1) >= V and x.stride(0) == T * x.stride(1):
        return x, x.stride(1)
    x = x.float().contiguous()
    return x, V


def _carve(packed, B, T, S):
    n_path, n_spans = B * T, B * S * 2
    return (packed[:n_path].view(B, T), packed[n_path:n_path + n_spans].view(B, S, 2),
            packed[n_path + n_spans:].view(torch.float32))


def _align_device(x, input_lens, targets, target_lens, blank, lse, entry="ia_ctc_align"):
    """One launch; (packed i32 [B*T + 2*B*S + B], path, spans, score) -- the three outputs are views of `packed`, so one copy
    brings them to the host."""
    L = _lib.lib()
    launch, ws_bytes = getattr(L, entry), getattr(L, entry + "_workspace_bytes")
    x, ld = _rows_in_place(x.detach())
    B, T, V = x.shape
    dev = x.device
    tg = targets.detach().to(dev).long().reshape(B, -1).contiguous()
    S = tg.shape[1]
    il = input_lens.detach().to(dev).long().contiguous()
    tl = target_lens.detach().to(dev).long().contiguous()
    z = None if lse is None else lse.detach().to(dev).float().contiguous()
    n = ws_bytes(B, T, S)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    packed = torch.empty(B * T + 2 * B * S + B, dtype=torch.int32, device=dev)
    path, spans, score = _carve(packed, B, T, S)
    with torch.cuda.device(dev):
        _lib.check(launch(_lib.ptr(x), ld, _lib.ptr(z), _lib.ptr(tg), _lib.ptr(il), _lib.ptr(tl), B, T, V, S, int(blank),
                          _lib.ptr(path), _lib.ptr(spans) if S > 0 else None, _lib.ptr(score), _lib.ptr(ws), n,
                          _lib.stream_ptr()), entry)
    return packed, path, spans, score


def _align_device_long(x, input_lens, targets, target_lens, blank, lse):
    """_align_device on csrc/ctc_align_long.hip (one workgroup per utterance): any S <= max_targets_long()."""
    return _align_device(x, input_lens, targets, target_lens, blank, lse, entry="ia_ctc_align_long")


def ctc_forced_align(logits_or_log_probs, input_lens, targets, target_lens, blank, lse=None):
    """Best CTC path of every utterance through its transcript.

    logits_or_log_probs [B,T,V] f32: log-probs, or raw logits when `lse` [B,T] (their per-frame log-sum-exp) is given.
    Returns (path [B,T] i32: state per frame, -1 for t >= input_lens[b];  spans [B,S,2] i32: first and last frame of each
    token, -1 beyond target_lens[b];  score [B] f32: log-prob of the path), on the input's device.  An utterance too short
    for its transcript has score -inf and -1 everywhere.  CUDA tensors run csrc/ctc_align.hip, CPU tensors the host routine."""
    global _warned_limit
    x = logits_or_log_probs
    if x.dim() != 3:
        raise ValueError(f"expected [B,T,V] log-probs or logits, got shape {tuple(x.shape)}")
    if not 0 <= int(blank) < x.shape[2]:
        raise ValueError(f"blank={blank} outside the {x.shape[2]} classes")
    if not x.is_cuda:
        return ctc_forced_align_host(x, input_lens, targets, target_lens, blank, lse)
    S = targets.reshape(x.shape[0], -1).shape[1]
    if S > max_targets():
        if not _warned_limit:
            warnings.warn(f"ctc_forced_align: transcripts padded to {S} tokens exceed the kernel's limit of {max_targets()} "
                          "(extended length 2S+1 <= 512); aligning on the host instead")
            _warned_limit = True
        out = ctc_forced_align_host(x, input_lens, targets, target_lens, blank, lse)
        return tuple(t.to(x.device) for t in out)
    return _align_device(x, input_lens, targets, target_lens, blank, lse)[1:]


_warned_limit_long = False


def max_targets_long():
    """Longest transcript (tokens) the workgroup kernel takes; beyond it ctc_forced_align_long runs the host routine."""
    return int(_lib.lib().ia_ctc_align_long_max_targets())


def ctc_forced_align_long(logits_or_log_probs, input_lens, targets, target_lens, blank, lse=None):
    """ctc_forced_align for long transcripts: same arguments, same return values, bit-equal results.  CUDA tensors run
    csrc/ctc_align_long.hip (one workgroup per utterance) for any S <= max_targets_long(), short transcripts included; beyond
    that the host routine, with a one-time warning.  CPU tensors run the host routine."""
    global _warned_limit_long
    x = logits_or_log_probs
    if x.dim() != 3:
        raise ValueError(f"expected [B,T,V] log-probs or logits, got shape {tuple(x.shape)}")
    if not 0 <= int(blank) < x.shape[2]:
        raise ValueError(f"blank={blank} outside the {x.shape[2]} classes")
    if not x.is_cuda:
        return ctc_forced_align_host(x, input_lens, targets, target_lens, blank, lse)
    S = targets.reshape(x.shape[0], -1).shape[1]
    if S > max_targets_long():
        if not _warned_limit_long:
            warnings.warn(f"ctc_forced_align_long: transcripts padded to {S} tokens exceed the workgroup kernel's limit of "
                          f"{max_targets_long()} (extended length 2S+1 <= 16384); aligning on the host instead")
            _warned_limit_long = True
        out = ctc_forced_align_host(x, input_lens, targets, target_lens, blank, lse)
        return tuple(t.to(x.device) for t in out)
    return _align_device_long(x, input_lens, targets, target_lens, blank, lse)[1:]


# ---------------------------------------------------------------------------------------------------------- results
def frame_seconds(cfg):
    """Duration of one encoder frame: the feature hop times the subsampling factor (0.04 s for the reference's settings)."""
    return cfg.n_window_stride / cfg.sample_rate * SUBSAMPLING_FACTOR


def _pieces(ids, tokenizer, language_id):
    sp = getattr(tokenizer, "sp", {}).get(language_id) if tokenizer is not None else None
    if sp is None:
        return None
    n = sp.GetPieceSize()
    return [sp.IdToPiece(int(i)) if 0 <= int(i) < n else None for i in ids]


def _group_words(tokens, pieces):
    """Words from SentencePiece pieces: a piece that begins with the word-start marker opens a word."""
    words, cur = [], None
    for tok, piece in zip(tokens, pieces):
        if piece is None:           # an id without a piece: part of no word
            continue
        if piece.startswith(WORD_START) or cur is None:
            cur = [piece.lstrip(WORD_START), tok.t_start, tok.t_end]
            words.append(cur)
        else:
            cur[0] += piece
            cur[2] = tok.t_end
    return [WordSpan(text=w[0], t_start=w[1], t_end=w[2]) for w in words if w[0]]


def build_alignments(path, spans, score, token_ids, frame_s, tokenizer=None, language_id=None):
    """Host tensors of ctc_forced_align + the transcripts' id lists -> one UtteranceAlignment per utterance.
    Times follow the aligner's rule: t_start = first_frame * frame_s, t_end = (last_frame + 1) * frame_s."""
    path, spans, score = path.cpu().numpy(), spans.cpu().numpy(), score.cpu().numpy()
    out = []
    for b, ids in enumerate(token_ids):
        sc = float(score[b])
        if sc == float("-inf"):
            out.append(UtteranceAlignment(score=sc, feasible=False))
            continue
        pieces = _pieces(ids, tokenizer, language_id)
        tokens = []
        for i, tid in enumerate(ids):
            f0, f1 = int(spans[b, i, 0]), int(spans[b, i, 1])
            text = pieces[i] if pieces is not None and pieces[i] is not None else str(int(tid))
            tokens.append(TokenSpan(id=int(tid), text=text, t_start=f0 * frame_s, t_end=(f1 + 1) * frame_s, first_frame=f0,
                                    last_frame=f1))
        words = _group_words(tokens, pieces) if pieces is not None else []
        frames = [int(s) for s in path[b] if s >= 0]
        out.append(UtteranceAlignment(tokens=tokens, words=words, score=sc, frames=frames, feasible=True))
    return out


def write_ctm(path, utt_ids, alignments, level="word"):
    """One line per word or token, `<utt_id> 1 <start> <duration> <text>` with two decimals (make_ctm_files.py:109-119;
    a space inside a text would split the field and is written as <space>)."""
    if level not in ("word", "token"):
        raise ValueError(f"level must be 'word' or 'token', got {level!r}")
    if len(utt_ids) != len(alignments):
        raise ValueError(f"{len(utt_ids)} utterance ids for {len(alignments)} alignments")
    with open(path, "w", encoding="utf-8") as f:
        for utt, al in zip(utt_ids, alignments):
            for it in (al.words if level == "word" else al.tokens):
                f.write("%s 1 %.2f %.2f %s\n" % (utt, it.t_start, it.t_end - it.t_start, it.text.replace(" ", "<space>")))


def pad_token_ids(token_ids):
    """Id lists -> (targets [B,S] i64 zero-padded with S >= 1, lengths [B] i64), the collate's layout."""
    S = max(1, max((len(t) for t in token_ids), default=0))
    tg = torch.zeros(len(token_ids), S, dtype=torch.long)
    for i, t in enumerate(token_ids):
        tg[i, :len(t)] = torch.as_tensor(list(t), dtype=torch.long)
    return tg, torch.tensor([len(t) for t in token_ids], dtype=torch.long)
