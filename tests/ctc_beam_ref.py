"""CTC prefix beam search restated in numpy for the tests (Hannun et al. 2014, arXiv:1408.2873, in log space), in float64 (E)
and in float32 (F32).  Shares no code with the package.  A prefix IS its tuple of labels here, so identity is exact by
construction; candidates live in an [n, V] matrix per frame (slot i, token c; a stay sits in the blank column).

Per utterance: lp = x - lse, blank = V - 1, the beam starts as the empty prefix with pb = 0, pnb = -inf.  Frame t, member l in
slot i with last label e and p = pb (+) pnb:
  stay    l gets pb' (+)= p + lp[blank], and if non-empty pnb' (+)= pnb + lp[e]
  extend  l + c (c != blank, lp[c] >= token_min_logp) gets pnb' (+)= (c == e ? pb : p) + lp[c]
Candidates that denote the same prefix are one candidate; the new beam is the W largest pb' (+) pnb', ties to the smaller id
i V + c (a merged candidate keeps its smallest id)."""
import numpy as np

NEG_INF = float("-inf")


def _gap(a, b):
    """a >= b, neighbours in an ordered list: what separates them (two -inf are ordered by their ids alone: never close)."""
    if not np.isfinite(a) or not np.isfinite(b):
        return float("inf")
    return float(a) - float(b)


def search(x, W, blank=None, lse=None, dtype=np.float64, token_min_logp=None, trace=None):
    """x [T,V] (the frames of ONE utterance, already cut to its length).  Returns (hypotheses, gap): hypotheses = list of
    (label list, score) in beam order; gap = the smallest score difference a decision rested on (W-th against (W+1)-th
    candidate of any frame, neighbours of the final list).  `trace`, a list, receives the beam (tuples) after every frame."""
    x = np.asarray(x, dtype=dtype)
    T, V = x.shape
    blank = V - 1 if blank is None else blank
    lp_all = x if lse is None else x - np.asarray(lse, dtype=dtype).reshape(T, 1)
    floor = NEG_INF if token_min_logp is None else token_min_logp
    beam, pb, pnb = [()], np.zeros(1, dtype), np.full(1, NEG_INF, dtype)
    gap = float("inf")
    with np.errstate(invalid="ignore"):
        for t in range(T):
            lp = lp_all[t]
            n = len(beam)
            p = np.logaddexp(pb, pnb)
            cpnb = p[:, None] + lp[None, :]
            cpb = np.full((n, V), NEG_INF, dtype)
            alive = np.ones((n, V), bool)
            alive[:, lp < floor] = False
            alive[:, blank] = True
            cpb[:, blank] = p + lp[blank]
            cpnb[:, blank] = NEG_INF
            for i, l in enumerate(beam):
                if l:
                    cpnb[i, l[-1]] = pb[i] + lp[l[-1]]
                    cpnb[i, blank] = pnb[i] + lp[l[-1]]
            ids = np.arange(n * V).reshape(n, V)
            where = {l: i for i, l in enumerate(beam)}
            for j, l in enumerate(beam):
                i = where.get(l[:-1]) if l else None
                if i is not None and alive[i, l[-1]]:
                    cpnb[j, blank] = np.logaddexp(cpnb[j, blank], cpnb[i, l[-1]])
                    ids[j, blank] = min(ids[j, blank], ids[i, l[-1]])
                    alive[i, l[-1]] = False
            tot = np.logaddexp(cpb, cpnb)
            assert tot.dtype == dtype
            flat = np.nonzero(alive.ravel())[0]
            order = flat[np.lexsort((ids.ravel()[flat], -tot.ravel()[flat]))]
            if len(order) > W:
                gap = min(gap, _gap(tot.ravel()[order[W - 1]], tot.ravel()[order[W]]))
            order = order[:W]
            new = []
            for k in order:
                i, c = divmod(int(k), V)
                new.append(beam[i] if c == blank else beam[i] + (c,))
            assert len(set(new)) == len(new)
            beam, pb, pnb = new, cpb.ravel()[order], cpnb.ravel()[order]
            if trace is not None:
                trace.append(list(beam))
    score = np.logaddexp(pb, pnb)
    for a, b in zip(score[:-1], score[1:]):
        gap = min(gap, _gap(a, b))
    return [(list(l), float(s)) for l, s in zip(beam, score)], gap


def E(x, W, blank=None, lse=None, token_min_logp=None, trace=None):
    return search(x, W, blank, lse, np.float64, token_min_logp, trace)


def F32(x, W, blank=None, lse=None, token_min_logp=None):
    return search(np.asarray(x, np.float32), W, blank, None if lse is None else np.asarray(lse, np.float32), np.float32,
                  None if token_min_logp is None else np.float32(token_min_logp))


def ctc_log_likelihood(lp, y, blank):
    """log p(y | x) summed over all alignments: the CTC forward recurrence in float64 on log-probs lp [T,V]."""
    lp = np.asarray(lp, np.float64)
    T = lp.shape[0]
    ext = [blank]
    for c in y:
        ext += [int(c), blank]
    L = len(ext)
    if T == 0:
        return 0.0 if not y else NEG_INF
    a = np.full(L, NEG_INF)
    a[0] = lp[0, ext[0]]
    if L > 1:
        a[1] = lp[0, ext[1]]
    skip = np.array([s >= 2 and ext[s] != blank and ext[s] != ext[s - 2] for s in range(L)])
    e = np.array(ext)
    for t in range(1, T):
        s1 = np.concatenate([[NEG_INF], a])[:L]
        s2 = np.where(skip, np.concatenate([[NEG_INF, NEG_INF], a])[:L], NEG_INF)
        a = np.logaddexp(np.logaddexp(a, s1), s2) + lp[t, e]
    return float(np.logaddexp(a[-1], a[-2]) if L > 1 else a[-1])


def margin_of(xs, W, blank=None, lses=None, token_min_logp=None):
    """For utterances xs (each [T_b,V] float32, lses their float32 lse or None): E's results, F32's results, and the largest
    |F32 - E| hypothesis-score difference over hypotheses that both lists hold at the same rank."""
    es, fs, worst = [], [], 0.0
    for k, x in enumerate(xs):
        lse = None if lses is None else lses[k]
        e, f = E(x, W, blank, lse, token_min_logp), F32(x, W, blank, lse, token_min_logp)
        es.append(e); fs.append(f)
        for (ye, se), (yf, sf) in zip(e[0], f[0]):
            if ye == yf and np.isfinite(se) and np.isfinite(sf):
                worst = max(worst, abs(se - sf))
    return es, fs, worst
