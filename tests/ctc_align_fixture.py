"""Shared by tests/test_ctc_align.py and tests/test_ctc_align_gpu.py: the golden cases of tests/golden/ctc_align_cases.npz
(written by tests/golden/make_ctc_align_golden.py from the reference's aligner), batches built from them, and the
properties of a CTC alignment that hold whatever the tie-break."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ctc_align_cases.npz")


def load_cases():
    """One dict per utterance: name, lp [T,V] f32 (log-probs), lse [T] f32 and logits = lp + lse (all exact on the
    fixture's grid), y [S] i64, V, blank, path [T] i64 or None (infeasible), score (f64, -inf when infeasible)."""
    z = np.load(GOLDEN)
    cases = []
    for i, name in enumerate(z["name"]):
        step = float(z["step"][i])
        lp = (-(z[f"g{i}"].astype(np.float64)) * step).astype(np.float32)
        lse = (z[f"z{i}"].astype(np.float64) * step).astype(np.float32)
        score = float(z["score"][i])
        cases.append(dict(name=str(name), lp=lp, lse=lse, logits=lp + lse[:, None], y=z[f"y{i}"].astype(np.int64), V=lp.shape[1],
                          blank=lp.shape[1] - 1, score=score,
                          path=None if score == -np.inf else z[f"path{i}"].astype(np.int64)))
    return cases, [int(i) for i in z["batch"]]


def spans_of(path, S):
    """[S,2]: first and last frame of token i (state 2i+1) in `path`; -1 where it does not occur."""
    out = np.full((S, 2), -1, dtype=np.int64)
    for t, s in enumerate(path):
        if s >= 0 and s & 1:
            if out[s >> 1, 0] < 0:
                out[s >> 1, 0] = t
            out[s >> 1, 1] = t
    return out


def make_batch(cases, logits_mode, T=None, S=None, ld=None):
    """Utterances (all of one V) -> padded tensors (x [B,T,ld], lse [B,T] or None, targets [B,S], input_lens, target_lens).
    Padding frames and columns hold +7 (a large score a kernel must never pick up), padding targets hold 0."""
    B, V = len(cases), cases[0]["V"]
    T = T or max(c["lp"].shape[0] for c in cases)
    S = S if S is not None else max(1, max(len(c["y"]) for c in cases))
    ld = ld or V
    x = torch.full((B, T, ld), 7.0)
    lse = torch.zeros(B, T)
    tg = torch.zeros(B, S, dtype=torch.long)
    for b, c in enumerate(cases):
        n = c["lp"].shape[0]
        x[b, :n, :V] = torch.from_numpy(c["logits"] if logits_mode else c["lp"])
        lse[b, :n] = torch.from_numpy(c["lse"])
        tg[b, :len(c["y"])] = torch.from_numpy(c["y"])
    il = torch.tensor([c["lp"].shape[0] for c in cases], dtype=torch.long)
    tl = torch.tensor([len(c["y"]) for c in cases], dtype=torch.long)
    return x, (lse if logits_mode else None), tg, il, tl


def assert_case(c, path, spans, score, T_b=None):
    """path [T] / spans [S,2] / score of one utterance against the reference's alignment: exact."""
    n = c["lp"].shape[0]
    path, spans = np.asarray(path, dtype=np.int64), np.asarray(spans, dtype=np.int64)
    assert np.all(path[n:] == -1), c["name"]
    assert np.all(spans[len(c["y"]):] == -1), c["name"]
    if c["path"] is None:
        assert score == -np.inf and np.all(path == -1) and np.all(spans == -1), c["name"]
        return
    assert np.array_equal(path[:n], c["path"]), f"{c['name']}: path differs from the reference's"
    assert np.array_equal(spans[:len(c["y"])], spans_of(c["path"], len(c["y"]))), c["name"]
    assert float(score) == c["score"], f"{c['name']}: score {float(score)!r} != {c['score']!r}"


def assert_valid_alignment(path, y, blank):
    """Starts in {0,1}; steps in {0,1,2}; a skip only onto a token that differs from the one two states back; ends in
    {L-2, L-1} (L = 1: state 0)."""
    path = [int(s) for s in path]
    L = 2 * len(y) + 1
    ext = [blank if s % 2 == 0 else int(y[s // 2]) for s in range(L)]
    assert len(path) >= 1 and path[0] in (0, 1) and path[0] < L
    for a, b in zip(path[:-1], path[1:]):
        assert 0 <= b - a <= 2 and b < L
        if b - a == 2:
            assert b % 2 == 1 and ext[b] != ext[a], "a skip between equal labels (or over a token)"
    assert path[-1] in ((0,) if L == 1 else (L - 2, L - 1))


def best_and_rescored_fp64(q, y, blank, path):
    """(fp64 optimum over all alignments, fp64 score of `path`) on the per-frame scores q [T,V] (any float dtype)."""
    q = np.asarray(q, dtype=np.float64)
    T, L = q.shape[0], 2 * len(y) + 1
    ext = np.full(L, blank, dtype=np.int64)
    ext[1::2] = y
    skip = np.zeros(L, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    v = np.full(L, -np.inf)
    v[:2] = q[0, ext[:2]]
    for t in range(1, T):
        a1 = np.concatenate([[-np.inf], v[:-1]])
        a2 = np.where(skip, np.concatenate([[-np.inf, -np.inf], v[:-2]])[:L], -np.inf)
        v = np.maximum(np.maximum(v, a1), a2) + q[t, ext]
    best = v[L - 1] if L == 1 else max(v[L - 1], v[L - 2])
    return float(best), float(np.sum(q[np.arange(T), ext[np.asarray(path, dtype=np.int64)]]))
