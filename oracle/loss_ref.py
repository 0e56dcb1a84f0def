"""fp64 / fp32 restatements of the two training losses: the CTC lattice (csrc/ctc.hip) and the transducer lattice
(csrc/rnnt_loss.hip).  numpy only.

TEST INFRASTRUCTURE (see oracle/__init__.py): only tests/ import this file.

`ctc_ref(...)` and `rnnt_ref(...)` compute what the kernels compute -- forward and backward variables, the negative
log-likelihood and the gradient -- as plain array arithmetic, vectorised over the extended-label states (CTC) or over the cells
of one anti-diagonal (transducer), so a T = 3000 utterance takes a fraction of a second.

  dtype=np.float64   the reference E.  tests/test_loss_reference.py pins it to ATen's double CTC (values and autograd
                     gradients), to a brute-force sum over every alignment, to closed forms, to oracle/rnnt_oracle.py's pure-Python
                     transducer, to the recorded answers under tests/golden/ and to oracle/rnnt_ref.c.
  dtype=np.float32   the identical recurrence with every intermediate in fp32 (correctly rounded exp / log, numpy's summation
                     order).  d(F32, F64) is the noise scale fp32 arithmetic is allowed on a given case: the GPU tolerances of
                     tests/test_loss_reference_gpu.py are a fixed multiple of it, never a number taken from a kernel.

Conventions
  CTC   x [B,T,ld] batch-major, targets [B,S] padded, blank anywhere in [0,V).  alpha_t(s) and beta_t(s) both INCLUDE the
        emission of frame t (ATen's convention, the kernels' too), so occupancy_t(v) = sum_{s: l'_s = v} exp(alpha_t(s) +
        beta_t(s) - lp_t(v) + nll) and sum_v occupancy_t(v) = 1 on every live frame.
  RNNT  logits [B,T,U1,V], labels [B,U1-1]; alpha(t,u) excludes, beta(t,u) includes the emission at (t,u) (warp-transducer);
        costs = -(1 + fastemit) ll; the gradient is with respect to the LOGITS with FastEmit's extra term and the clamp of
        oracle/rnnt_ref.c (the clamp acts on the un-scaled gradient: any upstream factor multiplies the clamped value).
"""
import numpy as np

_NEG = -np.inf


def _lse_rows(x):
    """log sum exp over the last axis in x's own dtype; -inf for an all -inf row."""
    m = x.max(-1, keepdims=True)
    ms = np.where(np.isfinite(m), m, 0).astype(x.dtype)
    with np.errstate(divide="ignore"):
        return (ms + np.log(np.exp(x - ms).sum(-1, keepdims=True, dtype=x.dtype)))[..., 0]


def _lse3(a, b, c):
    m = np.maximum(a, np.maximum(b, c))
    ms = np.where(np.isfinite(m), m, 0).astype(a.dtype)
    with np.errstate(divide="ignore"):
        r = ms + np.log(np.exp(a - ms) + np.exp(b - ms) + np.exp(c - ms))
    return np.where(m == _NEG, _NEG, r).astype(a.dtype)


def _shift_r(v, k):
    """out[s] = v[s-k], -inf shifted in."""
    out = np.full_like(v, _NEG)
    if k < v.shape[0]:
        out[k:] = v[:v.shape[0] - k]
    return out


def _shift_l(v, k):
    """out[s] = v[s+k], -inf shifted in."""
    out = np.full_like(v, _NEG)
    if k < v.shape[0]:
        out[:v.shape[0] - k] = v[k:]
    return out


def ctc_ref(x, targets, in_lens, tg_lens, blank, *, logits, valid_cols=None, dtype=np.float64):
    """CTC on batch-major x [B,T,ld].  logits=True: x holds raw logits, the log-probabilities are x - lse over the first
    `valid_cols` columns; logits=False: x holds log-probabilities, used as they are (-inf allowed).  Columns >= valid_cols
    (default ld) are never read.

    Returns a dict:
      nll [B]            +inf for an utterance with no alignment (and for in_len = 0 with a non-empty transcript)
      feasible [B]       nll is finite
      alpha, beta        [B,T,2S+1] over the extended labels, -inf outside (t >= in_len, s >= 2 tg_len + 1, unreachable)
      occupancy [B,T,V]  posterior mass of class v at frame t; 0 for t >= in_len and on infeasible rows
      grad_lp            d nll / d log-prob in ATen's convention, exp(lp) - occupancy
      grad_logits        d nll / d logits = softmax - occupancy (the same array when the rows are normalised; None for
                         logits=False, where no softmax exists)
      lse [B,T]          the row normaliser (logits=True only)
    Both gradients are 0 for t >= in_len and on infeasible rows (zero_infinity)."""
    x = np.asarray(x)
    B, T, ld = x.shape
    V = ld if valid_cols is None else int(valid_cols)
    targets = np.asarray(targets, np.int64).reshape(B, -1)
    S = targets.shape[1]
    Lmax = 2 * S + 1
    nll = np.zeros(B, dtype)
    alpha = np.full((B, T, Lmax), _NEG, dtype)
    beta = np.full((B, T, Lmax), _NEG, dtype)
    occ = np.zeros((B, T, V), dtype)
    grad = np.zeros((B, T, V), dtype)
    lse_out = np.zeros((B, T), dtype) if logits else None
    for b in range(B):
        Tb, Sb = int(in_lens[b]), int(tg_lens[b])
        L = 2 * Sb + 1
        if Tb <= 0:
            nll[b] = 0.0 if Sb == 0 else np.inf
            continue
        lp = x[b, :Tb, :V].astype(dtype)
        if logits:
            z = _lse_rows(lp)
            lse_out[b, :Tb] = z
            lp = lp - z[:, None]
        lab = np.full(L, int(blank), np.int64)
        lab[1::2] = targets[b, :Sb]
        e = lp[:, lab]                                         # [Tb, L] emission of every state
        skip = np.zeros(L, bool)                               # state s may be entered from s-2
        skip[3::2] = lab[3::2] != lab[1:-2:2]
        skip_b = np.zeros(L, bool)                             # state s may be left towards s+2
        skip_b[:-2] = skip[2:]
        a = alpha[b, :Tb, :L]
        be = beta[b, :Tb, :L]
        a[0, 0] = e[0, 0]
        if L > 1:
            a[0, 1] = e[0, 1]
        for t in range(1, Tb):
            p = a[t - 1]
            p2 = np.where(skip, _shift_r(p, 2), _NEG).astype(dtype)
            a[t] = _lse3(p, _shift_r(p, 1), p2) + e[t]
        be[Tb - 1, L - 1] = e[Tb - 1, L - 1]
        if L > 1:
            be[Tb - 1, L - 2] = e[Tb - 1, L - 2]
        for t in range(Tb - 2, -1, -1):
            p = be[t + 1]
            p2 = np.where(skip_b, _shift_l(p, 2), _NEG).astype(dtype)
            be[t] = _lse3(p, _shift_l(p, 1), p2) + e[t]
        neg = np.array([_NEG], dtype)
        ll = _lse3(a[Tb - 1, L - 1:L], a[Tb - 1, L - 2:L - 1] if L > 1 else neg, neg)[0]
        nll[b] = -ll
        if not np.isfinite(ll):
            continue
        ab = a + be
        live = ab != _NEG
        with np.errstate(invalid="ignore"):
            post = np.where(live, np.exp(np.where(live, ab - e + nll[b], 0)), 0).astype(dtype)
        o = occ[b, :Tb]
        np.add.at(o, (np.arange(Tb)[:, None], lab[None, :]), post)
        grad[b, :Tb] = np.exp(lp) - o
    return dict(nll=nll, feasible=np.isfinite(nll), alpha=alpha, beta=beta, occupancy=occ, grad_lp=grad,
                grad_logits=grad if logits else None, lse=lse_out)


def ctc_brute_force(lp, target, blank):
    """-log of the sum over EVERY alignment (all V^T frame labellings that collapse to `target`) of one utterance's
    log-probabilities lp [T,V], in fp64.  Exponential: tiny cases only."""
    import itertools
    lp = np.asarray(lp, np.float64)
    T, V = lp.shape
    target = [int(v) for v in target]
    tot = _NEG
    for path in itertools.product(range(V), repeat=T):
        out, prev = [], None
        for v in path:
            if v != prev and v != blank:
                out.append(v)
            prev = v
        if out == target:
            tot = np.logaddexp(tot, sum(lp[t, v] for t, v in enumerate(path)))
    return -tot


def rnnt_ref(logits, labels, flen, glen, blank, fastemit=0.0, clamp=0.0, dtype=np.float64):
    """Transducer loss on logits [B,T,U1,V].  Returns dict(costs [B], alphas, betas [B,T,U1] (0 outside each utterance's
    lattice), grads [B,T,U1,V] with respect to the logits (0 outside), ll [B])."""
    x = np.asarray(logits).astype(dtype)
    B, T, U1, V = x.shape
    labels = np.asarray(labels, np.int64).reshape(B, U1 - 1)
    fe = dtype(fastemit)
    l1p = np.log1p(fe)
    costs = np.zeros(B, dtype)
    lls = np.zeros(B, dtype)
    alphas = np.zeros((B, T, U1), dtype)
    betas = np.zeros((B, T, U1), dtype)
    grads = np.zeros((B, T, U1, V), dtype)
    for b in range(B):
        Tb, Ub = int(flen[b]), int(glen[b]) + 1
        assert 1 <= Tb <= T and 1 <= Ub <= U1
        xb = x[b, :Tb, :Ub]
        m = xb.max(-1, keepdims=True)
        logp = xb - (m + np.log(np.exp(xb - m).sum(-1, keepdims=True, dtype=dtype)))   # [Tb,Ub,V]
        pb = logp[:, :, blank]
        pl = np.full((Tb, Ub), _NEG, dtype)
        if Ub > 1:
            pl[:, :Ub - 1] = np.take_along_axis(logp[:, :Ub - 1], labels[b, None, :Ub - 1, None], -1)[..., 0]
        a = np.full((Tb, Ub), _NEG, dtype)
        be = np.full((Tb, Ub), _NEG, dtype)
        a[0, 0] = 0
        D = Tb + Ub - 1
        for n in range(1, D):
            t = np.arange(max(0, n - Ub + 1), min(Tb - 1, n) + 1)
            u = n - t
            tm, um = np.maximum(t - 1, 0), np.maximum(u - 1, 0)
            no_emit = np.where(t > 0, a[tm, u] + pb[tm, u], _NEG).astype(dtype)
            emit = np.where(u > 0, a[t, um] + pl[t, um], _NEG).astype(dtype)
            a[t, u] = np.logaddexp(emit, no_emit)
        ll = a[Tb - 1, Ub - 1] + pb[Tb - 1, Ub - 1]
        be[Tb - 1, Ub - 1] = pb[Tb - 1, Ub - 1]
        for n in range(D - 2, -1, -1):
            t = np.arange(max(0, n - Ub + 1), min(Tb - 1, n) + 1)
            u = n - t
            tp, up = np.minimum(t + 1, Tb - 1), np.minimum(u + 1, Ub - 1)
            no_emit = np.where(t < Tb - 1, be[tp, u] + pb[t, u], _NEG).astype(dtype)
            emit = np.where(u < Ub - 1, be[t, up] + pl[t, u], _NEG).astype(dtype)
            be[t, u] = np.logaddexp(emit, no_emit)
        lls[b] = ll
        costs[b] = -(ll + ll * fe)
        alphas[b, :Tb, :Ub] = a
        betas[b, :Tb, :Ub] = be
        # gradient with respect to the logits (oracle/rnnt_ref.c, the loop over v)
        be_t1 = np.full((Tb, Ub), _NEG, dtype); be_t1[:-1] = be[1:]          # beta(t+1, u)
        be_u1 = np.full((Tb, Ub), _NEG, dtype); be_u1[:, :-1] = be[:, 1:]    # beta(t, u+1)
        g = np.exp((a + be - ll)[..., None] + logp)
        if fastemit > 0.0:
            g = g + fe * np.exp((a + pl + be_u1 - ll)[..., None] + logp)      # exp(-inf) = 0 at u = Ub-1
        gb = np.exp(a + pb - ll + be_t1)                                      # 0 on the last frame
        gb[Tb - 1, Ub - 1] = np.exp(a[Tb - 1, Ub - 1] + pb[Tb - 1, Ub - 1] - ll)
        g[:, :, blank] -= gb
        if Ub > 1:
            gl = np.exp(l1p + a + pl - ll + be_u1)[:, :Ub - 1]
            idx = labels[b, None, :Ub - 1, None]
            sub = np.take_along_axis(g[:, :Ub - 1], idx, -1) - gl[..., None]
            np.put_along_axis(g[:, :Ub - 1], idx, sub, -1)
        if clamp > 0.0:
            g = np.clip(g, -dtype(clamp), dtype(clamp))
        grads[b, :Tb, :Ub] = g
    return dict(costs=costs, alphas=alphas, betas=betas, grads=grads, ll=lls)
