"""Greedy decoding and WER for the hybrid model.

* greedy_rnnt_decode  -- GreedyBatchedRNNTInfer._greedy_decode_blank_as_pad_loop_frames
  (A/parts/submodules/rnnt_greedy_decoding.py:711-909): frame-synchronous over the batch, at most `max_symbols`
  prediction-net + joint micro-steps per frame, sticky per-frame blank mask, hidden state rolled back for utterances that
  emitted blank.  All tensors stay on the device and the loop makes ONE host read per micro-step (`blank_mask.all()`, as the
  reference does); the encoder and prediction projections of the joint are hoisted out of the loop.  On the MI355X the
  same decode runs DEVICE-RESIDENT (csrc/greedy_decode.hip: one launch, one persistent workgroup per utterance, no host
  read per micro-step) -- greedy_rnnt_decode dispatches to it; the host-driven loop stays as greedy_rnnt_decode_host
  (CPU tensors, and the cross-check of the kernel in tests).
* greedy_ctc_decode   -- GreedyCTCInfer (ctc_greedy_decoding.py:145-229): argmax, collapse repeats, drop blanks.
* beam_ctc_decode     -- CTC prefix beam search (Hannun et al. 2014, arXiv:1408.2873), alone or with a token-level n-gram LM
  fused in (ngram_lm.NGramLM, read from ARPA text), what CTCBPEDecoding's `strategy: beam` stands for (NeMo delegates it to
  KenLM-backed ctc_decoders, pyctcdecode or flashlight; the algorithm is reproduced, not their bits): N-best Hypothesis objects
  with scores.  Device tensors run csrc/ctc_beam.hip / csrc/ctc_beam_lm.hip (one launch per batch), CPU tensors the float64
  host routine beam_ctc_decode_host of the same definition.
* beam_rnnt_decode    -- transducer beam search, NeMo's `strategy: alsd` (alignment-length synchronous decoding, Saon et al.
  2020; rnnt_beam_decoding.py:829-1068 as written): Hypothesis objects with scores and alignment steps.  Device tensors run
  csrc/rnnt_beam.hip (one launch per batch, one workgroup per utterance), CPU tensors the float64 host routine
  beam_rnnt_alsd_host of the same definition.
* word_error_rate / WER -- A/metrics/wer.py:293-360: sum of edit distances over sum of reference lengths.  Hypotheses
  and references are sequences of tokens here; pass `detokenize` (ids -> str) to score words as the reference does
  (its SentencePiece models are not part of the repository).
"""
import warnings
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence

import torch


def _edit_distance_py(a: Sequence, b: Sequence) -> int:
    if len(a) < len(b):
        a, b = b, a
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def _edit_distances(pairs) -> List[int]:
    """Levenshtein distances of (hypothesis, reference) pairs of unit sequences (tokens, words or characters): ONE call of
    the library's host routine (csrc/host_metrics.hip, the reference's `editdistance` C extension: wer.py:58-60) -- the
    pure-Python programme cost more per training step than the decode.  Units are numbered through a dictionary first."""
    pairs = [(list(a), list(b)) for a, b in pairs]
    if not pairs:
        return []
    if sum(len(a) * len(b) for a, b in pairs) < 256:      # tiny: not worth the call
        return [_edit_distance_py(a, b) for a, b in pairs]
    import ctypes
    import numpy as np
    from . import _lib
    L = _lib.lib()
    ids = {}
    fa, fb, oa, ob = [], [], [0], [0]
    for a, b in pairs:
        fa.extend(ids.setdefault(x, len(ids)) for x in a)
        fb.extend(ids.setdefault(x, len(ids)) for x in b)
        oa.append(len(fa)); ob.append(len(fb))
    A, Bv = np.asarray(fa, dtype=np.int32), np.asarray(fb, dtype=np.int32)
    OA, OB = np.asarray(oa, dtype=np.int64), np.asarray(ob, dtype=np.int64)
    out = np.zeros(len(pairs), dtype=np.int64)
    vp = lambda arr: ctypes.c_void_p(arr.ctypes.data)
    _lib.check(L.ia_edit_distance_batch(vp(A), vp(OA), vp(Bv), vp(OB), len(pairs), vp(out)), "ia_edit_distance_batch")
    return out.tolist()


def _edit_distance(a: Sequence, b: Sequence) -> int:
    """Levenshtein distance (editdistance.eval in the reference, wer.py:58-60)."""
    return _edit_distances([(a, b)])[0]


def word_error_rate(hypotheses: List[Sequence], references: List[Sequence], detokenize: Optional[Callable] = None):
    """(wer, total_edits, total_reference_units).  With `detokenize` both sides are turned into strings and split on
    whitespace (words); without it the units are the tokens themselves."""
    pairs = []
    for h, r in zip(hypotheses, references):
        if detokenize is not None:
            h, r = detokenize(list(h)).split(), detokenize(list(r)).split()
        pairs.append((list(h), list(r)))
    words = sum(len(r) for _, r in pairs)
    scores = sum(_edit_distances(pairs))
    wer = scores / words if words > 0 else float("inf")
    return wer, scores, words


class WER:
    """update()/compute()/reset() surface of A/metrics/wer.py for the step's monitor."""

    def __init__(self, detokenize: Optional[Callable] = None):
        self.detokenize = detokenize
        self.reset()

    def reset(self):
        self.scores, self.words = 0, 0

    def update(self, hypotheses, references):
        _, s, w = word_error_rate(hypotheses, references, self.detokenize)
        self.scores += s
        self.words += w

    def compute(self):
        wer = self.scores / self.words if self.words > 0 else float("inf")
        return wer, self.scores, self.words


class PendingHyps:
    """Hypotheses whose device work and device->host copies have been ENQUEUED (on the stream that was current at the call);
    `result()` waits for the copies' event and builds the token lists.  training_step(compute_wer=True) holds two of them
    (transducer + CTC) in the monitor, so the decode runs beside the rest of the step instead of in front of it."""

    def __init__(self, finish):
        self._finish, self._res = finish, None

    def result(self) -> List[List[int]]:
        if self._finish is not None:
            self._res = self._finish()
            self._finish = None
        return self._res


def _pinned_async(t):
    """Asynchronous device->host copy of `t` into pinned memory on the current stream."""
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t, non_blocking=True)
    return h


@torch.no_grad()
def greedy_rnnt_decode(model, encoded, encoded_len, language_ids, max_symbols: Optional[int] = 10) -> List[List[int]]:
    """encoded [B,d,T'] (encoder output), encoded_len [B] -> per-utterance language-local token ids.  A batch that mixes
    languages is decoded language by language (every utterance goes through its own language's head, rnnt.py:1632-1640;
    utterances decode independently of their neighbours)."""
    langs = list(language_ids)
    if len(set(langs)) > 1:
        out = [None] * len(langs)
        for lang in dict.fromkeys(langs):
            idx = [i for i, l in enumerate(langs) if l == lang]
            sel = torch.tensor(idx, device=encoded.device)
            sub = greedy_rnnt_decode(model, encoded.index_select(0, sel), encoded_len.to(encoded.device).index_select(0, sel),
                                     [lang] * len(idx), max_symbols)
            for i, h in zip(idx, sub):
                out[i] = h
        return out
    if encoded.is_cuda and device_decode_supported(model):
        return greedy_rnnt_decode_device(model, encoded, encoded_len, language_ids, max_symbols)
    return greedy_rnnt_decode_host(model, encoded, encoded_len, language_ids, max_symbols)


def device_decode_supported(model) -> bool:
    from . import _lib
    c = model.cfg
    return (c.pred_hidden % 4 == 0 and c.joint_hidden % 4 == 0
            and _lib.lib().ia_greedy_decode_lds_bytes(c.pred_hidden, c.joint_hidden, c.vocab_per_lang + 1) <= 160 * 1024
            and model.decoder.prediction["dec_rnn"].lstm.num_layers == 1)


@torch.no_grad()
def _rnnt_decode_operands(model, encoded, encoded_len, language_ids, defer: bool = False, who: str = "greedy_rnnt_decode"):
    """What the device-resident transducer decodes (csrc/greedy_decode.hip, csrc/rnnt_beam.hip) multiply with: f_all [B,T,Hj] =
    the joint's encoder projection of all frames, EW [V+1,4Hp] = W_ih embedding[row] + b_ih + b_hh over the language's labels,
    the blank / padding row and the zero SOS input (both on the HIP fp32 GEMM for device tensors), the clamped-later lengths,
    and W_hh / W_pred / the head with their biases -- as bf16 images for a model that computes in bf16 (`w16`).  CPU tensors
    get the same operands from torch (the host routines)."""
    from . import cl
    cl.flush_pending_updates()
    if len(set(language_ids)) != 1:
        raise NotImplementedError(f"{who}: one language per batch (as the CL scripts evaluate)")
    dec, joint = model.decoder, model.joint
    dev = encoded.device
    B, d, T = encoded.shape
    V = model.cfg.vocab_per_lang + 1
    blank = V - 1
    Hp, Hj = model.cfg.pred_hidden, model.cfg.joint_hidden
    head = joint.joint_net[-1][language_ids[0]]
    lstm = dec.prediction["dec_rnn"].lstm
    emb = dec.prediction["embed"].weight

    def gemm32(a, w):   # a [M,K] @ w[N,K]^T on csrc/gemm_f32.hip
        a, w = a.float().contiguous(), w.float().contiguous()
        if a.shape[1] % 16 != 0 or not a.is_cuda:
            return a @ w.t()
        from . import _lib
        out = torch.empty(a.shape[0], w.shape[0], dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().ia_gemm_f32(_lib.ptr(a), a.shape[1], _lib.ptr(w), w.shape[1], a.shape[0], w.shape[0], a.shape[1],
                                          _lib.ptr(out), w.shape[0], _lib.stream_ptr()), "ia_gemm_f32")
        return out

    f_all = (gemm32(encoded.transpose(1, 2).reshape(B * T, d), joint.enc.weight) + joint.enc.bias.float()).view(B, T, Hj).contiguous()
    rows = torch.cat([emb[:blank].float(), emb[dec.blank_idx:dec.blank_idx + 1].float(),
                      torch.zeros(1, Hp, dtype=torch.float32, device=dev)], 0)                      # [V + 1, Hp]
    EW = (gemm32(rows, lstm.weight_ih_l0) + (lstm.bias_ih_l0 + lstm.bias_hh_l0).float()).contiguous()
    out_len = encoded_len.to(dev).long().contiguous()
    # a model that trains in bf16 decodes on the bf16 images of W_hh / W_pred / the head (what its training step multiplies
    # with, kept current by the fused optimizer: ops/fast.bf16_shadow): half the bytes per emitted symbol of a loop bound by
    # the CU's L2 bandwidth; an fp32 model decodes in fp32
    w16 = model.cfg.compute_dtype == "bf16" and Hp % 8 == 0 and Hj % 8 == 0

    def snap(p, image16=False):   # contiguous image; with `defer` a private COPY: the optimizer may rewrite the weights meanwhile
        if image16:
            if not p.is_cuda:
                return p.detach().float().bfloat16().contiguous()
            from .ops import fast
            t = fast.bf16_shadow(p)
            return t.clone() if defer else t
        t = p.detach().float().contiguous()
        return t.clone() if (defer and t.data_ptr() == p.data_ptr()) else t

    return dict(B=B, T=T, Hp=Hp, Hj=Hj, V=V, blank=blank, w16=w16, f_all=f_all, EW=EW, out_len=out_len,
                Whh=snap(lstm.weight_hh_l0, w16), Wp=snap(joint.pred.weight, w16), bp=snap(joint.pred.bias),
                Wh=snap(head.weight, w16), bh=snap(head.bias))


@torch.no_grad()
def greedy_rnnt_decode_device(model, encoded, encoded_len, language_ids, max_symbols: Optional[int] = 10, defer: bool = False):
    """The same decode in ONE launch (csrc/greedy_decode.hip).  Setup on the HIP fp32 GEMM: the joint's encoder projection of
    all frames and the table EW = W_ih embedding[row] + b_ih + b_hh over the 257 rows the loop can feed the prediction
    network (the language's labels by their ids as decoding.greedy_rnnt_decode_host feeds them, the blank / padding row, the
    zero SOS input); one device->host copy of the token matrix at the end."""
    from . import _lib
    L = _lib.lib()
    op = _rnnt_decode_operands(model, encoded, encoded_len, language_ids, defer)
    dev = encoded.device
    B, T, Hp, Hj, V, blank, w16 = op["B"], op["T"], op["Hp"], op["Hj"], op["V"], op["blank"], op["w16"]
    f_all, EW, out_len = op["f_all"], op["EW"], op["out_len"]
    Whh, Wp, bp, Wh, bh = op["Whh"], op["Wp"], op["bp"], op["Wh"], op["bh"]
    ms = int(max_symbols) if max_symbols is not None else 1 << 30
    cap = T * (int(max_symbols) if max_symbols is not None else 8)
    tokens = torch.empty(B, cap, dtype=torch.int32, device=dev)
    counts = torch.zeros(B, dtype=torch.int32, device=dev)
    overflow = torch.zeros(1, dtype=torch.int32, device=dev)
    args = (_lib.ptr(f_all), _lib.ptr(out_len), _lib.ptr(EW), _lib.ptr(Whh), _lib.ptr(Wp), _lib.ptr(bp),
            _lib.ptr(Wh), _lib.ptr(bh), B, T, Hp, Hj, V, blank, blank, V, ms, _lib.ptr(tokens), cap,
            _lib.ptr(counts), _lib.ptr(overflow))
    scratch = None
    if w16:
        # head over 16 frames at once on the matrix cores, the per-symbol GEMVs split over a cluster of workgroups per utterance
        nw = int(L.ia_greedy_decode_cluster(B, Hp, Hj))
        scratch = torch.empty(int(L.ia_greedy_decode_scratch_bytes(B, Hp, Hj)), dtype=torch.uint8, device=dev) if nw > 1 else None
        st = L.ia_greedy_rnnt_decode_bf16w_ex(*args, nw, _lib.ptr(scratch) if scratch is not None else None,
                                              scratch.numel() if scratch is not None else 0, _lib.stream_ptr())
    else:
        st = L.ia_greedy_rnnt_decode(*args, _lib.stream_ptr())
    _lib.check(st, "ia_greedy_rnnt_decode")

    def check_flags(ovf):
        if ovf & 2:
            raise RuntimeError("greedy_rnnt_decode: a hand-off between the workgroups of an utterance timed out (csrc/greedy_decode.hip); "
                               "the hypotheses of this batch are not valid")
        if ovf & 1:
            raise RuntimeError("greedy_rnnt_decode: an utterance emitted more symbols than the output buffer holds "
                               f"({cap} per utterance); pass a finite max_symbols")
    if defer:
        h_tok, h_n, h_ovf = _pinned_async(tokens), _pinned_async(counts), _pinned_async(overflow)
        ev = torch.cuda.Event()
        ev.record()
        keep = [tokens, counts, overflow, f_all, EW, Whh, Wp, bp, Wh, bh, out_len, scratch]   # alive until the kernel has run

        def finish():
            ev.synchronize()
            keep.clear()
            check_flags(int(h_ovf[0]))
            n = h_n.tolist()
            return [h_tok[b, :n[b]].tolist() for b in range(B)]
        return PendingHyps(finish)
    host_tok, host_n, ovf = tokens.cpu(), counts.cpu().tolist(), int(overflow.item())
    check_flags(ovf)
    return [host_tok[b, :host_n[b]].tolist() for b in range(B)]


@torch.no_grad()
def greedy_rnnt_decode_host(model, encoded, encoded_len, language_ids, max_symbols: Optional[int] = 10) -> List[List[int]]:
    """Host-driven form (one host read per micro-step, as the reference)."""
    dec, joint = model.decoder, model.joint
    dev = encoded.device
    B = encoded.shape[0]
    V = model.cfg.vocab_per_lang + 1
    blank = V - 1
    if len(set(language_ids)) != 1:
        raise NotImplementedError("greedy_rnnt_decode: one language per batch (as the CL scripts evaluate)")
    head = joint.joint_net[-1][language_ids[0]]
    f_all = joint.project_encoder(encoded.transpose(1, 2).float())          # [B,T,H] hoisted out of the loop
    out_len = encoded_len.to(dev)
    T = int(out_len.max().item())
    last_label = torch.full((B, 1), blank, dtype=torch.long, device=dev)
    hidden = None
    tokens = torch.full((B, 0), -1, dtype=torch.long, device=dev)
    cols = []
    for t in range(T):
        f = f_all[:, t]                                                      # [B,H]
        blank_mask = t >= out_len
        symbols = 0
        while max_symbols is None or symbols < max_symbols:
            if hidden is None and t == 0 and symbols == 0:
                g, hidden_prime = dec.predict(None, None, add_sos=False, batch_size=B)      # SOS = zero embedding
            else:
                y = torch.where(last_label == blank, torch.full_like(last_label, dec.blank_idx), last_label)
                g, hidden_prime = dec.predict(y, hidden, add_sos=False, batch_size=B)
            logits = head(torch.relu(f + joint.project_prednet(g[:, 0].float())))            # [B,V]
            k = logits.float().argmax(-1)
            blank_mask = blank_mask | (k == blank)
            if bool(blank_mask.all()):
                break
            if hidden is not None:   # utterances that emitted blank keep their previous state
                keep = blank_mask.view(1, B, 1)
                hidden_prime = tuple(torch.where(keep, h_old, h_new) for h_old, h_new in zip(hidden, hidden_prime))
            else:
                keep = blank_mask.view(1, B, 1)
                hidden_prime = tuple(torch.where(keep, torch.zeros_like(h_new), h_new) for h_new in hidden_prime)
            k = torch.where(blank_mask, last_label[:, 0], k)
            cols.append(torch.where(blank_mask, torch.full_like(k, -1), k))
            last_label = k.view(B, 1)
            hidden = hidden_prime
            symbols += 1
    if cols:
        tokens = torch.stack(cols, 1)
    host = tokens.tolist()
    return [[v for v in row if v >= 0] for row in host]


@torch.no_grad()
def greedy_ctc_decode(log_probs, lengths, blank: Optional[int] = None, defer: bool = False):
    """log_probs [B,T,V] (language-restricted), lengths [B] -> collapsed token ids (repeats merged, blanks removed).
    defer (CUDA): PendingHyps -- argmax / collapse mask enqueued, one asynchronous copy, lists built on result()."""
    B, T, V = log_probs.shape
    blank = V - 1 if blank is None else blank
    k = log_probs.argmax(-1)                                                  # [B,T]
    valid = torch.arange(T, device=k.device)[None, :] < lengths.to(k.device)[:, None]
    prev = torch.cat([torch.full((B, 1), -1, dtype=k.dtype, device=k.device), k[:, :-1]], 1)
    keep = valid & (k != blank) & (k != prev)
    if defer and k.is_cuda:
        h = _pinned_async(torch.where(keep, k, torch.full_like(k, -1)).to(torch.int32))
        ev = torch.cuda.Event()
        ev.record()

        def finish():
            ev.synchronize()
            arr = h.numpy()
            return [row[row >= 0].tolist() for row in arr]
        return PendingHyps(finish)
    host_k, host_keep = k.tolist(), keep.tolist()
    return [[v for v, m in zip(r, mk) if m] for r, mk in zip(host_k, host_keep)]


# ---------------------------------------------------------------------------------------------------------- CTC prefix beam search
@dataclass
class Hypothesis:
    """The fields of NeMo's rnnt_utils.Hypothesis that the search fills: `score` = log-probability of the labelling (all its
    alignments), `y_sequence` = language-local token ids, `text` (filled by transcribe), `timestep` (the transducer beam
    search: the alignment step at which each label was emitted, as NeMo's ALSD fills it)."""
    score: float
    y_sequence: List[int]
    text: Optional[str] = None
    timestep: Optional[List[int]] = None


@dataclass
class NBestHypotheses:
    """rnnt_utils.NBestHypotheses: the beam by descending score.  `n_finished` (the transducer beam search): how many
    finished hypotheses the search ranked; the list holds the first beam_size of them."""
    n_best_hypotheses: Optional[List[Hypothesis]] = None
    n_finished: Optional[int] = None


_NEG_INF = float("-inf")
_warned_beam_limit = False


def beam_ctc_limits():
    """(largest beam width, largest class count) csrc/ctc_beam.hip takes; beyond them beam_ctc_decode runs the host routine."""
    from . import _lib
    return int(_lib.lib().ia_ctc_beam_max_width()), 1024


def beam_ctc_lm_max_order():
    """The largest LM order csrc/ctc_beam_lm.hip takes (its other limits are beam_ctc_limits())."""
    from . import _lib
    return int(_lib.lib().ia_ctc_beam_lm_max_order())


def beam_ctc_search_host(scores, lengths, beam_size=4, blank=None, lse=None, token_min_logp=None, lm=None, beam_alpha=1.0,
                         beam_beta=0.0):
    """CTC prefix beam search (Hannun et al. 2014, arXiv:1408.2873) in float64 on the host: the definition of
    include/indicasr.h, which csrc/ctc_beam.hip follows too.  scores [B,T,V] log-probs, or logits with lse [B,T].
    Returns per utterance a list of (token ids, score) by descending score, ties to the smaller candidate id.

    Prefix identity is the node of a trie of (parent node, token) pairs kept in a dictionary; one frame is a [n, V] matrix
    of candidate scores, the at most n extensions that denote a beam member folded into that member's stay.

    lm (an ngram_lm.NGramLM): shallow fusion -- every extension by c != blank carries beam_alpha lm.score(l, c) + beam_beta, also
    when it is folded into a member's stay; stays carry none; token_min_logp still looks at the acoustic log-prob alone."""
    import numpy as np
    x = scores.detach().double().cpu().numpy()
    B, T, V = x.shape
    blank = V - 1 if blank is None else int(blank)
    W = int(beam_size)
    if W < 1:
        raise ValueError("Beam search size cannot be less than 1!")
    if not 0 <= blank < V:
        raise ValueError(f"blank={blank} outside the {V} classes")
    if lse is not None:
        x = x - lse.detach().double().cpu().numpy().reshape(B, T, 1)
    lens = np.clip(lengths.detach().long().cpu().numpy().reshape(B), 0, T)
    floor = _NEG_INF if token_min_logp is None else float(token_min_logp)
    out = []
    with np.errstate(invalid="ignore"):
        for b in range(B):
            parent, token, child = [-1], [-1], {}              # the trie: node -> (parent, token), (parent, token) -> node
            tail = [()]                                        # with an LM: node -> its last order - 1 tokens, what h(l) needs
            node, pb, pnb = [0], np.array([0.0]), np.array([_NEG_INF])
            for t in range(int(lens[b])):
                lp = x[b, t]
                n = len(node)
                last = np.array([token[k] for k in node])
                p = np.logaddexp(pb, pnb)
                base = np.repeat(p[:, None], V, 1)
                rows = np.nonzero(last >= 0)[0]
                base[rows, last[rows]] = pb[rows]
                c_pnb = base + lp[None, :]
                if lm is not None:
                    c_pnb = c_pnb + np.stack([beam_alpha * lm.row(tail[k], V) + beam_beta for k in node])
                c_pnb[:, lp < floor] = np.nan                  # not a candidate
                c_pb = np.full((n, V), _NEG_INF)
                c_pb[:, blank] = p + lp[blank]
                c_pnb[:, blank] = _NEG_INF
                c_pnb[rows, blank] = pnb[rows] + lp[last[rows]]
                ids = np.arange(n * V).reshape(n, V)
                slot = {k: i for i, k in enumerate(node)}
                for j in rows:                                  # l_i + c is the beam member l_j: one candidate
                    i = slot.get(parent[node[j]])
                    c = last[j]
                    if i is not None and not np.isnan(c_pnb[i, c]):
                        c_pnb[j, blank] = np.logaddexp(c_pnb[j, blank], c_pnb[i, c])
                        ids[j, blank] = min(ids[j, blank], ids[i, c])
                        c_pnb[i, c] = np.nan
                total = np.logaddexp(c_pb, c_pnb).ravel()
                live = np.nonzero(~np.isnan(total))[0]
                order = live[np.lexsort((ids.ravel()[live], -total[live]))][:W]
                new_node, new_pb, new_pnb = [], [], []
                for k in order:
                    i, c = divmod(int(k), V)
                    if c == blank:
                        new_node.append(node[i])
                    else:
                        key = (node[i], c)
                        if key not in child:
                            child[key] = len(parent)
                            parent.append(node[i]); token.append(c)
                            if lm is not None:
                                tail.append((tail[node[i]] + (c,))[-(lm.order - 1):] if lm.order > 1 else ())
                        new_node.append(child[key])
                    new_pb.append(c_pb[i, c]); new_pnb.append(c_pnb[i, c])
                node, pb, pnb = new_node, np.array(new_pb), np.array(new_pnb)
            hyps = []
            for k, s in zip(node, np.logaddexp(pb, pnb)):
                y = []
                while k > 0:
                    y.append(int(token[k])); k = parent[k]
                hyps.append((y[::-1], float(s)))
            out.append(hyps)
    return out


def _beam_results(raw, return_best_hypothesis):
    res = []
    for hyps in raw:
        hs = [Hypothesis(score=s, y_sequence=list(y)) for y, s in hyps]
        res.append(hs[0] if return_best_hypothesis else NBestHypotheses(hs))
    return res


def beam_ctc_decode_host(scores, lengths, beam_size=4, blank=None, lse=None, token_min_logp=None, return_best_hypothesis=True,
                         lm=None, beam_alpha=1.0, beam_beta=0.0):
    """beam_ctc_decode on the host in float64 (CPU tensors; the cross-check of the kernel in tests)."""
    return _beam_results(beam_ctc_search_host(scores, lengths, beam_size, blank, lse, token_min_logp, lm, beam_alpha, beam_beta),
                         return_best_hypothesis)


def _beam_device(scores, lengths, W, blank, lse, floor, lm=None, alpha=1.0, beta=0.0):
    """One launch of csrc/ctc_beam.hip (with `lm`: csrc/ctc_beam_lm.hip); the packed result [B*W*T tokens | B*W lengths |
    B*W scores] as one i32 device tensor."""
    from . import _lib
    from .align import _rows_in_place
    L = _lib.lib()
    x, ld = _rows_in_place(scores.detach())
    B, T, V = x.shape
    dev = x.device
    il = lengths.detach().to(dev).long().contiguous()
    z = None if lse is None else lse.detach().to(dev).float().contiguous()
    n = (L.ia_ctc_beam_workspace_bytes if lm is None else L.ia_ctc_beam_lm_workspace_bytes)(B, T, V, W)
    ws = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
    packed = torch.empty(B * W * T + 2 * B * W, dtype=torch.int32, device=dev)
    tok, ln, sc = packed[:B * W * T], packed[B * W * T:B * W * T + B * W], packed[B * W * T + B * W:]
    with torch.cuda.device(dev):
        if lm is not None:
            import ctypes
            _, image = lm.to(dev)
            _lib.check(L.ia_ctc_beam_search_lm(_lib.ptr(x), _lib.ptr(z), _lib.ptr(il), B, T, ld, V, int(blank), W, floor,
                                               ctypes.byref(image), float(alpha), float(beta), _lib.ptr(tok), _lib.ptr(ln),
                                               _lib.ptr(sc), _lib.ptr(ws), n, _lib.stream_ptr()), "ia_ctc_beam_search_lm")
            return packed
        _lib.check(L.ia_ctc_beam_search(_lib.ptr(x), _lib.ptr(z), _lib.ptr(il), B, T, ld, V, int(blank), W, floor, _lib.ptr(tok),
                                        _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(ws), n, _lib.stream_ptr()), "ia_ctc_beam_search")
    return packed


@torch.no_grad()
def beam_ctc_decode(scores, lengths, beam_size=4, blank=None, lse=None, token_min_logp=None, return_best_hypothesis=True,
                    lm=None, beam_alpha=1.0, beam_beta=0.0):
    """CTC prefix beam search, with `lm` (an ngram_lm.NGramLM) fused into it: per utterance the best Hypothesis, or with
    return_best_hypothesis=False the NBestHypotheses (at most beam_size of them, by descending score).  With an LM every
    extension by a token c carries beam_alpha ln P_LM(c | history) + beam_beta and the scores are the fused totals; the classes
    are the LM's tokens.

    scores [B,T,V] f32: log-probs, or raw logits when `lse` [B,T] (their per-frame log-sum-exp) is given; lengths [B];
    blank defaults to V - 1; token_min_logp (None = off): extensions by a token whose log-prob in the frame is below it are not
    made.  Device tensors within the kernel's limits run csrc/ctc_beam.hip (one launch, one device-to-host copy of the packed
    result); CPU tensors, and shapes beyond the limits (with a warning), run the float64 host routine.  A Hypothesis score is
    the log-probability of the labelling as far as the beam kept its alignments, never more than its CTC log-likelihood."""
    global _warned_beam_limit
    if scores.dim() != 3:
        raise ValueError(f"expected [B,T,V] log-probs or logits, got shape {tuple(scores.shape)}")
    B, T, V = scores.shape
    blank = V - 1 if blank is None else int(blank)
    W = int(beam_size)
    if W < 1:
        raise ValueError("Beam search size cannot be less than 1!")
    if not 0 <= blank < V:
        raise ValueError(f"blank={blank} outside the {V} classes")
    if not scores.is_cuda or B == 0 or T == 0:
        return beam_ctc_decode_host(scores, lengths, W, blank, lse, token_min_logp, return_best_hypothesis, lm, beam_alpha, beam_beta)
    max_w, max_v = beam_ctc_limits()
    if lm is not None and lm.order > beam_ctc_lm_max_order():
        if not _warned_beam_limit:
            warnings.warn(f"beam_ctc_decode: an LM of order {lm.order} exceeds the kernel's limit (order <= "
                          f"{beam_ctc_lm_max_order()}); searching on the host instead")
            _warned_beam_limit = True
        return beam_ctc_decode_host(scores, lengths, W, blank, lse, token_min_logp, return_best_hypothesis, lm, beam_alpha, beam_beta)
    if W > max_w or V > max_v:
        if not _warned_beam_limit:
            warnings.warn(f"beam_ctc_decode: beam_size={W}, {V} classes exceed the kernel's limits (beam_size <= {max_w}, "
                          f"classes <= {max_v}); searching on the host instead")
            _warned_beam_limit = True
        return beam_ctc_decode_host(scores, lengths, W, blank, lse, token_min_logp, return_best_hypothesis, lm, beam_alpha, beam_beta)
    floor = _NEG_INF if token_min_logp is None else float(token_min_logp)
    host = _beam_device(scores, lengths, W, blank, lse, floor, lm, beam_alpha, beam_beta).cpu()
    tok = host[:B * W * T].view(B, W, T).numpy()
    ln = host[B * W * T:B * W * T + B * W].view(B, W).numpy()
    sc = host[B * W * T + B * W:].view(torch.float32).view(B, W).numpy()
    raw = [[(tok[b, r, :ln[b, r]].tolist(), float(sc[b, r])) for r in range(W) if ln[b, r] >= 0] for b in range(B)]
    return _beam_results(raw, return_best_hypothesis)


# ------------------------------------------------------------------------------------- transducer beam search (ALSD)
class _AlsdSide:
    """The decode operands in one precision (the dict of oracle.decode_ref.decode_reference: f_all [B,T,Hj], EW [V+1,4Hp], Whh,
    Wp, bp, Wh, bh; optional f_all32 / EW32 = the fp32 images of operands given in fp64)."""

    def __init__(self, case, dt):
        s = "32" if dt == torch.float32 else ""
        cpu = lambda t: t.detach().cpu().to(dt)
        self.f_all, self.EW = cpu(case.get("f_all" + s, case["f_all"])), cpu(case.get("EW" + s, case["EW"]))
        self.Whh, self.Wp, self.Wh = cpu(case["Whh"]), cpu(case["Wp"]), cpu(case["Wh"])
        self.bp, self.bh = cpu(case["bp"]), cpu(case["bh"])
        self.Hp = self.Whh.shape[1]
        self.zero = torch.zeros(self.Hp, dtype=dt)

    def cell(self, row, h, c):
        Hp = self.Hp
        g = self.Whh @ h + self.EW[row]
        i, f, gg, o = torch.sigmoid(g[:Hp]), torch.sigmoid(g[Hp:2 * Hp]), torch.tanh(g[2 * Hp:3 * Hp]), torch.sigmoid(g[3 * Hp:])
        cn = f * c + i * gg
        hn = o * torch.tanh(cn)
        return hn, cn, self.Wp @ hn + self.bp


class _AlsdHyp:
    __slots__ = ("seq", "score", "own", "ts", "slack", "parent")

    def __init__(self, seq, score, ts, slack, parent):
        self.seq, self.score, self.own, self.ts, self.slack, self.parent = seq, score, score, ts, slack, parent


class _AlsdEval:
    """What oracle.decode_ref._evaluate reads of a path: the frame and the pending (h, c, g) of both precisions."""
    __slots__ = ("t", "pend")


def alsd_u_max(alsd_max_target_len, length: int) -> int:
    """NeMo's u_max: int(a * len) for a float a, int(a) for an int."""
    a = alsd_max_target_len
    return max(0, int(a * length) if isinstance(a, float) else int(a))


def _alsd_utterance(S64, S32, b, length, W, u_max, score_norm, rounding, absW):
    import math
    V = S64.Wh.shape[0]
    blank = V - 1
    beam = min(W, V - 1)
    sides = (S64,) if rounding is None else (S64, S32)
    if rounding is not None:
        from oracle.decode_ref import _evaluate
    cache = {}

    def state(h):                                   # a pure function of the sequence: computed once per sequence
        st = cache.get(h.seq)
        if st is None:
            st = cache[h.seq] = tuple(S.cell(h.seq[-1], p[0], p[1]) for S, p in zip(sides, h.parent))
        return st

    Bm = [_AlsdHyp((blank,), 0.0, [], 0.0, tuple((S.zero, S.zero) for S in sides))]
    F, undecided, steps, recomb, fin_recomb = [], [], 0, 0, 0
    for i in range(length + u_max):
        live = [h for h in Bm if i - (len(h.seq) - 1) <= length - 1]
        if not live:
            break
        A, rows, fin_now = [], [], set()
        for h in live:
            t = i - (len(h.seq) - 1)
            st = state(h)
            if rounding is None:
                z = S64.Wh @ torch.relu(S64.f_all[b, t] + st[0][2]) + S64.bh
                step_tol = 0.0
            else:
                ev = _AlsdEval()
                ev.t, ev.pend = t, st
                z, tol, _, _ = _evaluate(S64, S32, b, ev, rounding, absW)
                step_tol = 2.0 * float(tol.max())
            lp = (z - torch.logsumexp(z, 0)).tolist()
            slack = h.slack + step_tol
            n = _AlsdHyp(h.seq, h.score + lp[blank], h.ts, slack, h.parent)
            A.append(n)
            if t == length - 1:
                F.append(n)                           # the same record: a recombination of this step shows in F
                fin_now.add(id(n))
            order = sorted(range(blank), key=lambda k: (-lp[k], k))      # equal values: the smaller id
            for k in order[:beam]:
                A.append(_AlsdHyp(h.seq + (k,), h.score + lp[k], h.ts + [i], slack, st))
            if blank > beam:
                rows.append((len(A) - 1, lp[order[beam - 1]] - lp[order[beam]], 2.0 * slack))
        order = sorted(range(len(A)), key=lambda j: -A[j].score)         # stable: ties keep A's order
        Bm = [A[j] for j in order[:beam]]
        if rounding is not None:
            if len(A) > beam:
                x, y = A[order[beam - 1]], A[order[beam]]
                if 0.0 != x.score - y.score <= x.slack + y.slack:      # an exact tie is decided by the stable order
                    undecided.append((i, "prune"))
            won = set(order[:beam])
            for last, gap, slack2 in rows:
                if last in won and 0.0 != gap <= slack2:               # an exact tie goes to the smaller id
                    undecided.append((i, "labels"))
        first = {}
        for h in Bm:
            f = first.get(h.seq)
            if f is None:
                first[h.seq] = h
                continue
            recomb += 1
            fin_recomb += id(f) in fin_now
            if rounding is not None and abs(f.own - h.own) <= f.slack + h.slack:
                undecided.append((i, "duplicates"))
            f.score = float(f.score + math.log1p(math.exp(h.score - f.score))) if f.score >= h.score else \
                float(h.score + math.log1p(math.exp(f.score - h.score)))
            f.slack = max(f.slack, h.slack)
        steps += 1
    if F:
        div = (lambda h: len(h.seq)) if score_norm else (lambda h: 1)
        out = sorted(F, key=lambda h: -(h.score / div(h)))               # stable
        key = lambda h: (h.score / div(h), h.slack / div(h))
    else:
        out = Bm
        key = lambda h: (h.own, h.slack)
    if rounding is not None:
        for x, y in zip(out, out[1:]):
            (kx, sx), (ky, sy) = key(x), key(y)
            if abs(kx - ky) <= sx + sy:
                undecided.append((-1, "ranking"))
    return dict(hyps=[(list(h.seq[1:]), float(h.score), list(h.ts)) for h in out], slack=[h.slack for h in out],
                n_finished=len(F), decided=not undecided, undecided=undecided, steps=steps, recombinations=recomb,
                finished_recombined=fin_recomb)


def beam_rnnt_alsd_host(case, beam_size=4, alsd_max_target_len=1.0, score_norm=True, rounding=None, n_best=None):
    """Alignment-length synchronous decoding (Saon et al. 2020) as NeMo's align_length_sync_decoding computes it
    (rnnt_beam_decoding.py:829-1068, its recombine_hypotheses -- which merges into the first occurrence and returns the
    unmerged list -- included), in float64 on the host: the definition of include/indicasr.h that csrc/rnnt_beam.hip follows.

    case: the decode operands (f_all [B,T,Hj], EW [V+1,4Hp] with rows labels / blank = padding row V-1 / SOS row V, Whh, Wp, bp,
    Wh, bh, lens [B]).  A hypothesis is a sequence (blank, y1..yu) whose state is the LSTM cell applied along it from the zero
    state; per step i every live member of the beam (t = i - u <= len - 1) contributes its blank candidate (also to the finished
    list when t = len - 1) and its min(beam_size, V-1) best labels; the beam is the first `beam` candidates by descending score
    (stable), and a member that repeats an earlier member's sequence adds its score to that one while staying in the beam.

    rounding None: exact.  "gemv" / "mfma": the kernel's rounding points (oracle.decode_ref._evaluate: nothing rounded / the
    head's operand rounded to bf16), with an fp32 twin of every sequence's state next to the fp64 one; each hypothesis then
    carries a slack (its parent's plus twice the step's largest logit tolerance; a recombined score the larger of the two)
    and the utterance a verdict `decided`: no pruning boundary, no row's beam-th label that won, no pair of duplicates and no
    pair of neighbours in the final ranking is closer than the slacks' sum.  (A difference of exactly 0 at the pruning boundary
    or between labels is decided: bit-equal fp64 values come from bit-equal operands -- copies of a head row -- which are
    bit-equal in every precision, and the stable order / smaller id then rules.  When nothing finished, the neighbours of the
    returned beam are compared by the scores the last pruning sorted them by.)

    Returns per utterance a dict: hyps = [(token ids, score, alignment steps)] in result order (the finished list by
    descending score / (u + 1) with score_norm, else by score; the beam as it stands when nothing finished; the first
    `n_best` of them if given), slack, n_finished, decided, undecided, steps, recombinations, finished_recombined (recombinations into
    a record that entered the finished list in the same step)."""
    assert rounding in ("mfma", "gemv", None)
    W = int(beam_size)
    if W < 1:
        raise ValueError("Beam search size cannot be less than 1!")
    S64 = _AlsdSide(case, torch.float64)
    S32 = None if rounding is None else _AlsdSide(case, torch.float32)
    absW = S64.Wh.abs() if rounding == "mfma" else None
    B, T, _ = S64.f_all.shape
    lens = case["lens"] if "lens" in case else case["out_len"]
    out = []
    for b in range(B):
        length = min(max(int(lens[b]), 0), T)
        r = _alsd_utterance(S64, S32, b, length, W, alsd_u_max(alsd_max_target_len, length), bool(score_norm), rounding, absW)
        if n_best is not None:
            r["hyps"], r["slack"] = r["hyps"][:n_best], r["slack"][:n_best]
        out.append(r)
    return out


def beam_rnnt_max_width():
    """The largest beam width csrc/rnnt_beam.hip takes; beyond it beam_rnnt_decode runs the host routine."""
    from . import _lib
    return int(_lib.lib().ia_rnnt_beam_max_width())


def beam_rnnt_alsd_device(op, beam_size, alsd_max_target_len=1.0, score_norm=True, n_best=None):
    """One launch of csrc/rnnt_beam.hip on device operands (f_all, EW, Whh, Wp, bp, Wh, bh, lens; the three weight matrices
    both bf16 or both fp32).  Returns None when the kernel refuses the shape as unsupported (before any device work), else the
    device tensors (tokens [B,K,L], steps [B,K,L], lengths [B,K], scores [B,K], n_finished [B]), K = min(n_best or beam_size,
    beam_size), L = T + the largest u_max."""
    from . import _lib
    L = _lib.lib()
    f_all = op["f_all"].float().contiguous()
    dev = f_all.device
    B, T, Hj = f_all.shape
    Whh, Wp, Wh = op["Whh"], op["Wp"], op["Wh"]
    w16 = Whh.dtype == torch.bfloat16
    if not w16:
        Whh, Wp, Wh = Whh.float(), Wp.float(), Wh.float()
    Whh, Wp, Wh = Whh.contiguous(), Wp.contiguous(), Wh.contiguous()
    EW, bp, bh = op["EW"].float().contiguous(), op["bp"].float().contiguous(), op["bh"].float().contiguous()
    Hp, V = Whh.shape[1], Wh.shape[0]
    W = int(beam_size)
    K = W if n_best is None else max(1, min(int(n_best), W))
    lens = (op["lens"] if "lens" in op else op["out_len"]).to(dev).long().contiguous()
    a = alsd_max_target_len
    clamped = lens.clamp(0, T)
    um = (clamped.double() * a).long() if isinstance(a, float) else torch.full_like(clamped, int(a))
    um = um.clamp(min=0).to(torch.int32).contiguous()
    max_umax = alsd_u_max(a, T)
    n = int(L.ia_rnnt_beam_workspace_bytes(B, T, Hp, Hj, V, W, max_umax))
    if n == 0:
        return None
    ws = torch.empty(n, dtype=torch.uint8, device=dev)
    ml = T + max_umax
    tokens = torch.empty(B, K, ml, dtype=torch.int32, device=dev)
    steps = torch.empty(B, K, ml, dtype=torch.int32, device=dev)
    lengths = torch.empty(B, K, dtype=torch.int32, device=dev)
    scores = torch.empty(B, K, dtype=torch.float32, device=dev)
    nfin = torch.empty(B, dtype=torch.int32, device=dev)
    fn = L.ia_rnnt_beam_alsd_bf16w if w16 else L.ia_rnnt_beam_alsd
    with torch.cuda.device(dev):
        st = fn(_lib.ptr(f_all), _lib.ptr(lens), _lib.ptr(um), _lib.ptr(EW), _lib.ptr(Whh), _lib.ptr(Wp), _lib.ptr(bp), _lib.ptr(Wh),
                _lib.ptr(bh), B, T, Hp, Hj, V, W, K, max_umax, int(bool(score_norm)), _lib.ptr(tokens), _lib.ptr(steps),
                _lib.ptr(lengths), _lib.ptr(scores), _lib.ptr(nfin), _lib.ptr(ws), n, _lib.stream_ptr())
    if st == -4:                                    # IA_UNSUPPORTED: refused before any device work
        return None
    _lib.check(st, "ia_rnnt_beam_alsd")
    return tokens, steps, lengths, scores, nfin


def alsd_unpack(raw):
    """The device result as the host routine's lists: per utterance dict(hyps=[(token ids, score, steps)], n_finished)."""
    tokens, steps, lengths, scores, nfin = (t.cpu() for t in raw)
    out = []
    for b in range(tokens.shape[0]):
        hyps = []
        for r in range(tokens.shape[1]):
            n = int(lengths[b, r])
            if n >= 0:
                hyps.append((tokens[b, r, :n].tolist(), float(scores[b, r]), steps[b, r, :n].tolist()))
        out.append(dict(hyps=hyps, n_finished=int(nfin[b])))
    return out


@torch.no_grad()
def beam_rnnt_decode(model, encoded, encoded_len, language_ids, beam_size=4, return_best_hypothesis=True, score_norm=True,
                     alsd_max_target_len=1.0):
    """Transducer beam search, `strategy: alsd` of NeMo's RNNTBPEDecoding: per utterance the best Hypothesis (score,
    y_sequence, timestep = the alignment step of each label), or with return_best_hypothesis=False the NBestHypotheses: the
    first beam_size of the ranked list (NeMo returns every finished hypothesis; `n_finished` says how many there were).
    The operands are those of greedy_rnnt_decode_device; device tensors run csrc/rnnt_beam.hip (one launch per language, one
    device-to-host copy), CPU tensors and shapes beyond the kernel's limits (with a warning) the float64 host routine
    beam_rnnt_alsd_host.  beam_size = 1 runs the same definition with one hypothesis (NeMo substitutes its greedy search)."""
    global _warned_beam_limit
    W = int(beam_size)
    if W < 1:
        raise ValueError("Beam search size cannot be less than 1!")
    langs = list(language_ids)
    if len(set(langs)) > 1:
        out = [None] * len(langs)
        for lang in dict.fromkeys(langs):
            idx = [i for i, l in enumerate(langs) if l == lang]
            sel = torch.tensor(idx, device=encoded.device)
            sub = beam_rnnt_decode(model, encoded.index_select(0, sel), encoded_len.to(encoded.device).index_select(0, sel),
                                   [lang] * len(idx), W, return_best_hypothesis, score_norm, alsd_max_target_len)
            for i, h in zip(idx, sub):
                out[i] = h
        return out
    op = _rnnt_decode_operands(model, encoded, encoded_len, langs, who="beam_rnnt_decode")
    op["lens"] = op["out_len"]
    res = None
    if encoded.is_cuda and op["B"] > 0 and op["T"] > 0:
        raw = beam_rnnt_alsd_device(op, W, alsd_max_target_len, score_norm) if W <= beam_rnnt_max_width() else None
        if raw is None and not _warned_beam_limit:
            warnings.warn(f"beam_rnnt_decode: beam_size={W}, pred_hidden={op['Hp']}, joint_hidden={op['Hj']}, {op['V']} classes "
                          f"exceed the kernel's limits (beam_size <= {beam_rnnt_max_width()}); searching on the host instead")
            _warned_beam_limit = True
        res = alsd_unpack(raw) if raw is not None else None
    if res is None:
        res = beam_rnnt_alsd_host(op, W, alsd_max_target_len, score_norm, None, W)
    out = []
    for r in res:
        hs = [Hypothesis(score=s, y_sequence=list(y), timestep=list(ts)) for y, s, ts in r["hyps"]]
        out.append(hs[0] if return_best_hypothesis else NBestHypotheses(hs, n_finished=r["n_finished"]))
    return out
