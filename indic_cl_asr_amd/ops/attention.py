"""Relative-position multi-head self-attention core (multi_head_attention.py:197-250 semantics).

scores[i,j] = ((q_i+u)·k_j + (q_i+v)·p[T-1-i+j]) / sqrt(dk): the reference's rel_shift pad/view trick
(:184-195) restated as index arithmetic on the [2T-1] relative-position axis; keys j >= len_b are excluded
(fill -10000 then zero after softmax, :108-111), and so are all keys for padded queries (their row is
uniform over the masked keys in the reference; it never reaches a loss because every consumer masks by length).
"""
import math

import torch


def _rel_shift_index(T, device):
    i = torch.arange(T, device=device).view(T, 1)
    j = torch.arange(T, device=device).view(1, T)
    return (T - 1 - i + j)  # [T,T] indices into the 2T-1 axis


def context_interval_mask(T, style, left, right, device=None):
    """[T, T] bool, True where query i and key j do NOT pair under a limited context (conformer_encoder.py:686-740 restated as
    intervals).  'regular' [L, R]: i - j <= L and j - i <= R.  'chunked_limited' [L, R], R >= 0: with C = R + 1 and n = L // C,
    0 <= i // C - j // C <= n; [L, -1]: i - j <= L only.  A negative side is unlimited."""
    if style not in ("regular", "chunked_limited"):
        raise ValueError(f"Invalid att_context_style: {style}")
    left, right = int(left), int(right)
    i = torch.arange(T, device=device).view(T, 1)
    j = torch.arange(T, device=device).view(1, T)
    if style == "regular" or right < 0:
        ok = torch.ones(T, T, dtype=torch.bool, device=device)
        if left >= 0:
            ok = ok & (i - j <= left)
        if right >= 0 and style == "regular":
            ok = ok & (j - i <= right)
        return ~ok
    C = right + 1
    dc = i // C - j // C
    ok = dc >= 0
    if left >= 0:
        ok = ok & (dc <= left // C)
    return ~ok


def rel_pos_attention(q, k, v, p, bias_u, bias_v, lens, dropout_p=0.0, training=False, keep_mask=None, window=None, context=None):
    """q,k,v: [B,h,T,dk]; p: [h,2T-1,dk]; bias_u/bias_v: [h,dk]; lens: [B] i64 -> context [B,h,T,dk].

    window = w > 0: local attention (RelPositionMultiHeadAttentionLongformer, multi_head_attention.py:253-470, symmetric window
    [w, w], no global tokens): p is [h, >= 2w+1, dk] with row r <-> relative position w - r, scores[i,j] takes p[w-i+j] and only
    the keys |i - j| <= w, j < len_b take part.  Differentiable like the full composition; window=None is unchanged.

    context = (style, L, R): a limited context under full rel-pos attention (the reference's att_context_size with
    att_context_style 'regular' or 'chunked_limited', a mask there): p and the position index are the full composition's, and
    only the pairs of context_interval_mask take part.  Not combined with window; context=None is unchanged."""
    if window is not None and window <= 0:
        raise ValueError("When using local attention, context size must be set > 0")
    if window is not None and context is not None:
        raise ValueError("rel_pos_attention: a limited context and a local window exclude each other")
    B, h, T, dk = q.shape
    scale = 1.0 / math.sqrt(dk)
    qu = q + bias_u.view(1, h, 1, dk).to(q.dtype)
    qv = q + bias_v.view(1, h, 1, dk).to(q.dtype)
    ac = torch.matmul(qu, k.transpose(-2, -1))                       # [B,h,T,T]
    valid = torch.arange(T, device=q.device)[None, :] < lens[:, None]            # [B,T]
    mask = ~(valid[:, :, None] & valid[:, None, :])                                # [B,T,T]
    if window is None:
        bd_full = torch.matmul(qv, p.unsqueeze(0).transpose(-2, -1))     # [B,h,T,2T-1]
        idx = _rel_shift_index(T, q.device)
        if context is not None:
            mask = mask | context_interval_mask(T, *context, device=q.device).unsqueeze(0)
    else:
        if p.shape[1] < 2 * window + 1:
            raise ValueError(f"rel_pos_attention: {p.shape[1]} position rows < 2 * {window} + 1")
        bd_full = torch.matmul(qv, p[:, :2 * window + 1].unsqueeze(0).transpose(-2, -1))     # [B,h,T,2w+1]
        rel = _rel_shift_index(T, q.device) - (T - 1)                    # j - i
        idx = (window + rel).clamp(0, 2 * window)                        # (clamped entries lie outside the band)
        mask = mask | (rel.abs() > window).unsqueeze(0)
    bd = torch.gather(bd_full, 3, idx.view(1, 1, T, T).expand(B, h, T, T))
    scores = ac + bd
    scores = (scores if scores.dtype == torch.float64 else scores.float()) * scale   # (fp64 callers: the reference checks)
    scores = scores.masked_fill(mask.unsqueeze(1), -10000.0)
    attn = torch.softmax(scores, dim=-1).masked_fill(mask.unsqueeze(1), 0.0)
    if keep_mask is not None:      # explicit dropout mask (0 or 1/(1-p)) [B,h,T,T]: the HIP kernel's, for its backward
        attn = attn * keep_mask.to(attn.dtype)
    elif training and dropout_p > 0.0:
        attn = torch.nn.functional.dropout(attn, dropout_p, True)
    return torch.matmul(attn.to(v.dtype), v)
