"""CTC prefix beam search with n-gram LM shallow fusion restated in numpy for the tests, in float64 (E) and float32 (F32).
Shares no code with the package.  The search is tests/ctc_beam_ref.py's with ONE rule changed:

  extend  l + c (c != blank, lp[c] >= token_min_logp) gets pnb' (+)= ((c == e ? pb : p) + lp[c]) + (alpha lm(l, c) + beta)

also when that extension is folded into a beam member's stay; stays get no LM term; the floor looks at lp[c] alone.

The LM is a plain dict {n-gram tuple: (log10 p, log10 back-off)}; a word is a token id, "<s>" (first position only), and the
unigram ("<unk>",) must be there.  lm(l, c) = ln P(c | h), h = the last N - 1 symbols of ("<s>", l_1 .. l_k):
  for k = |h| .. 0:  if h[-k:] + (c,) is in the dict: acc + log p of it;  else acc += back-off(h[-k:]) (0 if absent or k = 0)
  a token without a unigram: acc + log p(<unk>).
log10 values become natural logs in float64 and are rounded to float32 once (the definition); E adds them in float64, F32 in
float32."""
import math

import numpy as np

from ctc_beam_ref import NEG_INF, _gap, ctc_log_likelihood  # noqa: F401  (ctc_log_likelihood: for the tests)

LN10 = math.log(10.0)


def natural(v):
    return np.float32(v * LN10)


def lm_score(lm, order, prefix, c, dtype=np.float64):
    """ln P(c | h(prefix)) by the formula above, summed in `dtype`."""
    h = (("<s>",) + tuple(prefix))[-(order - 1):] if order > 1 else ()
    acc = dtype(0)
    known = (c,) in lm
    for k in range(len(h), -1, -1):
        ctx = h[len(h) - k:]
        if known and ctx + (c,) in lm:
            return acc + dtype(natural(lm[ctx + (c,)][0]))
        if k > 0 and ctx in lm:
            acc = acc + dtype(natural(lm[ctx][1]))
    return acc + dtype(natural(lm[("<unk>",)][0]))


def lm_sequence(lm, order, y):
    """ln P_LM(y) = the sum of lm(y[:k], y[k]) in float64 (no </s>)."""
    return float(sum(lm_score(lm, order, y[:k], y[k]) for k in range(len(y))))


class Rows:
    """lm(l, c) for all classes c < V at once, per history: the same formula, each context's n-grams applied as arrays (longest
    context first, a token keeps the first value it got)."""

    def __init__(self, lm, order, V, dtype):
        self.lm, self.order, self.V, self.dtype, self.cache = lm, order, V, dtype, {}
        kids = {}
        for g, (p, _) in lm.items():
            if g != ("<unk>",) and isinstance(g[-1], int) and g[-1] < V:
                kids.setdefault(g[:-1], []).append((g[-1], natural(p)))
        self.kids = {ctx: (np.array([t for t, _ in v]), np.array([p for _, p in v]).astype(dtype)) for ctx, v in kids.items()}
        self.unk = dtype(natural(lm[("<unk>",)][0]))

    def __call__(self, prefix):
        h = (("<s>",) + tuple(prefix))[-(self.order - 1):] if self.order > 1 else ()
        got = self.cache.get(h)
        if got is None:
            out, filled, acc = np.zeros(self.V, self.dtype), np.zeros(self.V, bool), self.dtype(0)
            for k in range(len(h), -1, -1):
                ctx = h[len(h) - k:]
                if ctx in self.kids:
                    toks, ps = self.kids[ctx]
                    new = ~filled[toks]
                    out[toks[new]] = acc + ps[new]
                    filled[toks[new]] = True
                if k > 0 and ctx in self.lm:
                    acc = acc + self.dtype(natural(self.lm[ctx][1]))
            out[~filled] = acc + self.unk
            assert out.dtype == self.dtype
            got = self.cache[h] = out
        return got


def search(x, W, lm, order, alpha, beta, blank=None, lse=None, dtype=np.float64, token_min_logp=None, rows=None,
           trace=None):
    """ctc_beam_ref.search with the LM term.  Returns (hypotheses, gap) as there; the scores are the fused totals."""
    x = np.asarray(x, dtype=dtype)
    T, V = x.shape
    blank = V - 1 if blank is None else blank
    lp_all = x if lse is None else x - np.asarray(lse, dtype=dtype).reshape(T, 1)
    floor = NEG_INF if token_min_logp is None else token_min_logp
    rows = Rows(lm, order, V, dtype) if rows is None else rows
    a, bt = dtype(alpha), dtype(beta)
    beam, pb, pnb = [()], np.zeros(1, dtype), np.full(1, NEG_INF, dtype)
    gap = float("inf")
    with np.errstate(invalid="ignore"):
        for t in range(T):
            lp = lp_all[t]
            n = len(beam)
            p = np.logaddexp(pb, pnb)
            fuse = np.stack([a * rows(l) + bt for l in beam])
            cpnb = (p[:, None] + lp[None, :]) + fuse
            cpb = np.full((n, V), NEG_INF, dtype)
            alive = np.ones((n, V), bool)
            alive[:, lp < floor] = False
            alive[:, blank] = True
            cpb[:, blank] = p + lp[blank]
            cpnb[:, blank] = NEG_INF
            for i, l in enumerate(beam):
                if l:
                    cpnb[i, l[-1]] = (pb[i] + lp[l[-1]]) + fuse[i, l[-1]]
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
            order_ = flat[np.lexsort((ids.ravel()[flat], -tot.ravel()[flat]))]
            if len(order_) > W:
                gap = min(gap, _gap(tot.ravel()[order_[W - 1]], tot.ravel()[order_[W]]))
            order_ = order_[:W]
            new = []
            for k in order_:
                i, c = divmod(int(k), V)
                new.append(beam[i] if c == blank else beam[i] + (c,))
            assert len(set(new)) == len(new)
            beam, pb, pnb = new, cpb.ravel()[order_], cpnb.ravel()[order_]
            if trace is not None:
                trace.append(list(beam))
    score = np.logaddexp(pb, pnb)
    for s0, s1 in zip(score[:-1], score[1:]):
        gap = min(gap, _gap(s0, s1))
    return [(list(l), float(s)) for l, s in zip(beam, score)], gap


def E(x, W, lm, order, alpha, beta, blank=None, lse=None, token_min_logp=None, rows=None, trace=None):
    return search(x, W, lm, order, alpha, beta, blank, lse, np.float64, token_min_logp, rows, trace)


def F32(x, W, lm, order, alpha, beta, blank=None, lse=None, token_min_logp=None, rows=None):
    return search(np.asarray(x, np.float32), W, lm, order, alpha, beta, blank, None if lse is None else np.asarray(lse, np.float32),
                  np.float32, None if token_min_logp is None else np.float32(token_min_logp), rows)


def margin_of(xs, W, lm, order, alpha, beta, blank=None, lses=None, token_min_logp=None):
    """ctc_beam_ref.margin_of with the LM: E's results, F32's results, and the largest |F32 - E| hypothesis-score difference
    over hypotheses that both lists hold at the same rank."""
    V = xs[0].shape[1]
    r64, r32 = Rows(lm, order, V, np.float64), Rows(lm, order, V, np.float32)
    es, fs, worst = [], [], 0.0
    for k, x in enumerate(xs):
        lse = None if lses is None else lses[k]
        e = E(x, W, lm, order, alpha, beta, blank, lse, token_min_logp, r64)
        f = F32(x, W, lm, order, alpha, beta, blank, lse, token_min_logp, r32)
        es.append(e); fs.append(f)
        for (ye, se), (yf, sf) in zip(e[0], f[0]):
            if ye == yf and np.isfinite(se) and np.isfinite(sf):
                worst = max(worst, abs(se - sf))
    return es, fs, worst


def random_lm(n_tokens, order, density, seed, skip_unigrams=()):
    """A random back-off model over the tokens 0 .. n_tokens - 1: every unigram (but `skip_unigrams`), "<s>" and "<unk>"; each
    kept n-gram of order < `order` is a context whose every token follows with probability `density`.  log10 p in [-3, -0.1],
    log10 back-off in [-1, 0] (0 at the highest order)."""
    g = np.random.default_rng(seed)

    def entry(top):
        return (round(float(g.uniform(-3, -0.1)), 4), 0.0 if top else round(float(g.uniform(-1, 0)), 4))

    lm = {("<unk>",): (round(float(g.uniform(-3, -2)), 4), 0.0), ("<s>",): (-99.0, entry(order == 1)[1])}
    level = [("<s>",)]
    for c in range(n_tokens):
        if c not in skip_unigrams:
            lm[(c,)] = entry(order == 1)
            level.append((c,))
    usable = np.array([c for c in range(n_tokens) if c not in skip_unigrams])
    for n in range(2, order + 1):
        nxt = []
        for ctx in level:
            for c in usable[g.random(len(usable)) < density]:
                lm[ctx + (int(c),)] = entry(n == order)
                nxt.append(ctx + (int(c),))
        level = nxt
    return lm


def write_arpa(path, lm, order, token_offset=100, extra=()):
    """`lm` as ARPA text: token id i is the character chr(i + token_offset); `extra` = further (n, line) pairs written as they
    are (and counted in the header)."""
    by_n = {n: [] for n in range(1, order + 1)}
    for g, (p, bo) in lm.items():
        words = " ".join(w if isinstance(w, str) else chr(w + token_offset) for w in g)
        by_n[len(g)].append(f"{p:.4f}\t{words}" + (f"\t{bo:.4f}" if len(g) < order else ""))
    for n, line in extra:
        by_n[n].append(line)
    with open(path, "w", encoding="utf-8") as f:
        f.write("\\data\\\n")
        for n in range(1, order + 1):
            f.write(f"ngram {n}={len(by_n[n])}\n")
        for n in range(1, order + 1):
            f.write(f"\n\\{n}-grams:\n" + "\n".join(by_n[n]) + "\n")
        f.write("\n\\end\\\n")
