"""The case tables of tests/test_loss_reference.py (CPU) and tests/test_loss_reference_gpu.py (MI355X), and the fp64 / fp32
references of every case, computed once per process and shared (oracle/loss_ref.py; numpy only, nothing here needs a GPU).

CTC: one ragged batch per padded target width S -- the width selects the `ctc_alpha_beta<K>` instantiation -- with a fixed set
of rows (see `ctc_batch`).  Transducer: one batch of four rows per (U1, T, V) (see `rnnt_batch`).

Tolerances (`bound`): for a compared quantity q of a case,  |kernel - ref64| <= MARGIN * e32 + ULPS * 2^-23 * scale,  where
e32 = max |ref32 - ref64| is measured here on the CPU from the reference alone and scale is the quantity's own magnitude.
"""
import functools

import numpy as np

from oracle import loss_ref

MARGIN = 8.0          # hardware exp2 / log2 (about 1 ulp each against numpy's correctly rounded calls) + another summation order
ULPS = 4.0            # floor: a few fp32 ulps of the quantity's own magnitude
EPS32 = 2.0 ** -23


def bound(e32, scale):
    return MARGIN * float(e32) + ULPS * EPS32 * float(scale)


def transcript(rng, n, labels, repeats):
    """n labels drawn from `labels` with exactly `repeats` adjacent equal pairs (a single label: all n-1 pairs repeat)."""
    labels = np.asarray(labels)
    if n == 0:
        return np.zeros(0, np.int64)
    if len(labels) == 1:
        return np.full(n, labels[0], np.int64)
    rep = set(rng.choice(np.arange(1, n), size=repeats, replace=False).tolist()) if repeats else set()
    out = [int(rng.choice(labels))]
    for i in range(1, n):
        out.append(out[-1] if i in rep else int(rng.choice(labels[labels != out[-1]])))
    return np.asarray(out, np.int64)


def n_repeats(seq):
    return int((seq[1:] == seq[:-1]).sum()) if len(seq) > 1 else 0


# ---------------------------------------------------------------------------------------------------------------- CTC
# (S, V, logit scale): every width boundary of the K dispatch (K=1: S<=31, K=2: <=63, K=4: <=127, K=8: <=255), every V and both
# scales under every K
CTC_TABLE = [
    (0, 17, 1.5), (0, 2, 30.0), (1, 2, 1.5), (1, 257, 30.0), (31, 65, 1.5), (31, 17, 30.0),
    (32, 2, 30.0), (32, 257, 1.5), (63, 17, 1.5), (63, 65, 30.0),
    (64, 65, 1.5), (64, 17, 30.0), (127, 2, 1.5), (127, 257, 30.0),
    (128, 17, 1.5), (128, 257, 30.0), (255, 2, 30.0), (255, 65, 1.5),
]
CTC_TABLE_LOGITS = CTC_TABLE + [(32, 600, 1.5), (64, 600, 30.0)]   # V > 512: the tail loop of the row log-sum-exp
# upstream d loss / d nll_b by row: positive, negative, exactly 0 (period 7: the zeros fall on `t2` and `len0_empty`, not on the
# tight, infeasible or unique-path rows, whose gradients are to be compared)
WEIGHTS = [1.0, -0.75, 1.5, 0.0, 0.5, -2.0, 1.25]


def ctc_batch(S, V, scale, blank=None, seed=0):
    """Rows (tl = target length, Tb = input length, R = adjacent repeats of the row's transcript):
         full        tl = S, Tb = T
         t1_empty    Tb = 1, tl = 0              t1_one   Tb = 1, tl = min(S, 1)
         t2 / t3 / t5  Tb = 2, 3, 5 (no multiple of either prefetch depth), tl = min(S, 1), min(S, 2), min(S, 2)
         empty_long  tl = 0, Tb = 7
         minimal     tl = S, Tb = tl + R exactly (feasible, tight)
         infeasible  the same transcript, Tb = tl + R - 1        (S >= 1)
         unique      S copies of one label, Tb = 2S - 1: one path (S >= 1)
         len0_empty  Tb = 0, tl = 0              len0_one  Tb = 0, tl = 1 (S >= 1): no alignment
       T = max(2S - 1, 7) is just large enough."""
    rng = np.random.default_rng(1000 * S + V + seed)
    blank = V - 1 if blank is None else blank
    labels = np.asarray([v for v in range(V) if v != blank])
    T = max(2 * S - 1, 7)
    rows = []   # (name, transcript, Tb)
    r_full = S - 1 if len(labels) == 1 else min(max(S - 1, 0), 3)
    rows.append(("full", transcript(rng, S, labels, r_full), T))
    rows.append(("t1_empty", transcript(rng, 0, labels, 0), 1))
    rows.append(("t1_one", transcript(rng, min(S, 1), labels, 0), 1))
    rows.append(("t2", transcript(rng, min(S, 1), labels, 0), 2))
    rows.append(("t3", transcript(rng, min(S, 2), labels, 0), 3))
    rows.append(("t5", transcript(rng, min(S, 2), labels, 1 if S > 1 else 0), 5))
    rows.append(("empty_long", transcript(rng, 0, labels, 0), 7))
    if S >= 1:
        r_min = S - 1 if len(labels) == 1 else min(S - 1, max(1, S // 4))
        tight = transcript(rng, S, labels, r_min)
        assert n_repeats(tight) == r_min
        rows.append(("minimal", tight, S + r_min))
        rows.append(("infeasible", tight, S + r_min - 1))
        rows.append(("unique", np.full(S, labels[int(rng.integers(len(labels)))], np.int64), 2 * S - 1))
    rows.append(("len0_empty", transcript(rng, 0, labels, 0), 0))
    if S >= 1:
        rows.append(("len0_one", transcript(rng, 1, labels, 0), 0))
    B = len(rows)
    targets = np.full((B, S), labels[0], np.int64)      # padding holds a valid class
    il = np.zeros(B, np.int64); tl = np.zeros(B, np.int64)
    for i, (_, seq, Tb) in enumerate(rows):
        targets[i, :len(seq)] = seq
        tl[i], il[i] = len(seq), Tb
        assert Tb <= T
    logits = (scale * rng.standard_normal((B, T, V))).astype(np.float32)
    z = logits.astype(np.float64)
    z = z - z.max(-1, keepdims=True)
    lp = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    w = np.asarray([WEIGHTS[i % len(WEIGHTS)] for i in range(B)], np.float32)
    return dict(S=S, V=V, T=T, B=B, blank=blank, names=[r[0] for r in rows], targets=targets, il=il, tl=tl, logits=logits,
                lp=lp, w=w)


def _ctc_refs(c, x, logits):
    r64 = loss_ref.ctc_ref(x, c["targets"], c["il"], c["tl"], c["blank"], logits=logits, dtype=np.float64)
    r32 = loss_ref.ctc_ref(x, c["targets"], c["il"], c["tl"], c["blank"], logits=logits, dtype=np.float32)
    assert (r64["feasible"] == r32["feasible"]).all()
    return r64, r32


def ctc_errors(c, r64, r32):
    """e32 and the bounds of the compared quantities of one CTC case: nll, the weighted gradient, (lse)."""
    f = r64["feasible"]
    w = c["w"].astype(np.float64)[:, None, None]
    out = {}
    nl64 = np.where(f, r64["nll"], 0.0)
    out["e_nll"] = float(np.abs(np.where(f, r32["nll"], 0.0).astype(np.float64) - nl64).max())
    out["b_nll"] = bound(out["e_nll"], max(1.0, np.abs(nl64).max()))
    out["e_grad"] = float(np.abs(w * (r32["grad_lp"].astype(np.float64) - r64["grad_lp"])).max())
    out["b_grad"] = bound(out["e_grad"], max(1.0, np.abs(w).max()))
    if r64["lse"] is not None:
        out["e_lse"] = float(np.abs(r32["lse"].astype(np.float64) - r64["lse"]).max())
        out["b_lse"] = bound(out["e_lse"], max(1.0, np.abs(r64["lse"]).max()))
    return out


@functools.lru_cache(maxsize=None)
def ctc_case(S, V, scale, form):
    """form 'lp': log-probabilities (fp32-rounded log_softmax of the logits); 'logits': the raw logits, blank = 0 for odd S."""
    if form == "lp":
        c = ctc_batch(S, V, scale)
        x = c["lp"]
    else:
        c = ctc_batch(S, V, scale, blank=0 if S % 2 else None)
        x = c["logits"]
    r64, r32 = _ctc_refs(c, x, form == "logits")
    c.update(x=x, r64=r64, r32=r32, **ctc_errors(c, r64, r32))
    for a in (x, r64["grad_lp"], r64["nll"]):
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def ctc_neginf_case(kind):
    """Log-prob form with -inf entries.  'outside': every class that is neither the blank nor in the row's transcript is -inf at
    every frame.  'label': the first label of each transcript is -inf at the frames t % 4 == 1 (this may make a tight row
    infeasible: the reference decides)."""
    c = ctc_batch(31, 17, 1.5, seed=7)
    lp = c["lp"].copy()
    for b in range(c["B"]):
        seq = c["targets"][b, :c["tl"][b]]
        if kind == "outside":
            dead = [v for v in range(c["V"]) if v != c["blank"] and v not in set(seq.tolist())]
            lp[b][:, dead] = -np.inf
        elif len(seq):
            lp[b, 1::4, seq[0]] = -np.inf
    r64, r32 = _ctc_refs(c, lp, False)
    c.update(x=lp, r64=r64, r32=r32, **ctc_errors(c, r64, r32))
    return c


@functools.lru_cache(maxsize=None)
def ctc_long_case(form):
    """B = 1, T = 3000, S = 100, V = 17: fp32 drift over the length."""
    rng = np.random.default_rng(3000)
    T, S, V = 3000, 100, 17
    seq = transcript(rng, S, np.arange(V - 1), 10)
    logits = (1.5 * rng.standard_normal((1, T, V))).astype(np.float32)
    z = logits.astype(np.float64)
    z = z - z.max(-1, keepdims=True)
    lp = (z - np.log(np.exp(z).sum(-1, keepdims=True))).astype(np.float32)
    c = dict(S=S, V=V, T=T, B=1, blank=V - 1, names=["long"], targets=seq[None], il=np.asarray([T]), tl=np.asarray([S]),
             logits=logits, lp=lp, w=np.asarray([1.0], np.float32))
    x = lp if form == "lp" else logits
    r64, r32 = _ctc_refs(c, x, form == "logits")
    c.update(x=x, r64=r64, r32=r32, **ctc_errors(c, r64, r32))
    return c


# --------------------------------------------------------------------------------------------------------------- RNNT
# (U1, T, V).  K of rnnt_alpha_beta: U1 <= 63 -> 1, <= 127 -> 2, <= 255 -> 4, <= 511 -> 8, <= 1023 -> 16; every K meets an odd
# and an even V and both of its width boundaries.  NV of rnnt_lse_gather = ceil(V / 64), generic above 512.  Long label axes go
# with V <= 5 and T <= 9, wide vocabularies with U1 <= 9 (U1 = 9 is not a boundary: it is there so that the wide rows also run
# the two-rows-in-flight loop of the gather, which needs more than four label positions).
RNNT_TABLE = [
    (1, 1, 1), (1, 7, 2), (2, 2, 3), (63, 3, 4), (63, 9, 5),
    (64, 7, 2), (64, 2, 5), (127, 9, 3), (127, 7, 4),
    (128, 1, 4), (128, 3, 5), (255, 2, 2), (255, 7, 3),
    (256, 9, 3), (256, 3, 4), (511, 2, 5), (511, 7, 2),
    (512, 3, 2), (512, 1, 5), (1023, 9, 3), (1023, 2, 4),
    (2, 17, 63), (9, 3, 64), (2, 7, 65), (9, 17, 128), (2, 1, 129), (9, 2, 192), (1, 9, 256), (9, 7, 320), (2, 3, 384),
    (9, 9, 448), (2, 2, 512), (9, 17, 513), (1, 3, 513),
]
RNNT_MODES = [(0.0, 0.0), (0.01, 0.0), (0.0, 0.05)]    # (fastemit, clamp)


def rnnt_batch(U1, T, V):
    """Four rows: (flen, glen) = (T, U1-1), (1, any), (any, 0), (any, U1-1); blank = V-1 for even V, 0 for odd V."""
    rng = np.random.default_rng(100000 * U1 + 1000 * T + V)
    blank = V - 1 if V % 2 == 0 else 0
    labels_ok = np.asarray([v for v in range(V) if v != blank])
    B = 4
    labels = rng.choice(labels_ok, size=(B, U1 - 1)) if U1 > 1 else np.zeros((B, 0), np.int64)
    flen = np.asarray([T, 1, int(rng.integers(1, T + 1)), int(rng.integers(1, T + 1))], np.int64)
    glen = np.asarray([U1 - 1, int(rng.integers(0, U1)), 0, U1 - 1], np.int64)
    logits = (2.0 * rng.standard_normal((B, T, U1, V))).astype(np.float32)
    return dict(U1=U1, T=T, V=V, B=B, blank=blank, labels=labels.astype(np.int64), flen=flen, glen=glen, logits=logits)


@functools.lru_cache(maxsize=None)
def rnnt_case(U1, T, V, fastemit, clamp):
    c = rnnt_batch(U1, T, V)
    a = (c["logits"], c["labels"], c["flen"], c["glen"], c["blank"], fastemit, clamp)
    r64 = loss_ref.rnnt_ref(*a, dtype=np.float64)
    r32 = loss_ref.rnnt_ref(*a, dtype=np.float32)
    c.update(r64=r64, r32=r32)
    for k, scale_of in (("costs", "costs"), ("alphas", "costs"), ("betas", "costs"), ("grads", None)):
        e = float(np.abs(r32[k].astype(np.float64) - r64[k]).max())
        scale = 1.0 if scale_of is None else max(1.0, float(np.abs(r64[scale_of]).max()))
        c["e_" + k], c["b_" + k] = e, bound(e, scale)
    return c
