"""Greedy transducer decoding replayed in fp64, decision by decision, with the set of hypotheses a correct fp32 kernel may return.

csrc/greedy_decode.hip returns token sequences only, so its decisions cannot be compared with a reference one by one.  Instead
the loop is replayed here in fp64 on exactly the operands the kernel multiplies with (bf16 images widened, or fp32), the
kernel's rounding points emulated:

  rounding="mfma"   relu(f_t + g) is rounded to bf16 before the head (the MFMA head of the bf16 decode)
  rounding="gemv"   nothing is rounded (the fp32 and the bf16-weight GEMV loops)
  rounding=None     exact: plain first-maximum argmax in fp64, no tolerance, no branching

State, gates, g and logits are never rounded.  Next to the fp64 replay runs an fp32 one (plain torch fp32, the same rounding
points), teacher-forced along the same path: it takes the token the fp64 path takes and carries its own fp32 state, so the
drift of fp32 over a long hypothesis is part of what it measures.

The tolerance of a micro-step, from reference quantities only (C = 4 and FLOOR = 2^-20 as tests/test_block_reference_gpu.py
and tests/test_lstm_reference_gpu.py; no other constant):

  pre = f_t + g (before ReLU and rounding)          e_pre = max_i |pre32_i - pre64_i|
  e_head_v = |head in fp32 - head in fp64|, both on the SAME activation vector for "mfma" (the fp64 path's rounded one:
             summation noise only), each on its own activation for "gemv" (which then already contains e_pre)
  "mfma" only: element i is flippable when pre64_i > -C e_pre and pre64_i lies within C e_pre of a bf16 rounding boundary
             (the midpoint of two neighbouring bf16 values); flip_v = sum over flippable i of q_i |W_head[v, i]| with
             q_i = ulp_bf16(|pre64_i| + C e_pre), plus C e_pre where the bf16 grid at pre64_i is no coarser than 2 C e_pre
  tol_v = C max_u e_head_u + flip_v + FLOOR max_u |z64_u|

Derivation.  A correct fp32 kernel computes pre' with |pre'_i - pre64_i| <= C e_pre: its state went through the same number
of fp32 operations as the fp32 replay's, in another order, and C is the factor the two merged references found sufficient
between two fp32 evaluations of one formula (the hardware exp of the gates included: it "stays well inside C").  In the GEMV
loops the activation relu(pre') enters the head unrounded: the logit differs from z64 by the propagated e_pre and by the
head's own summation noise, and e_head (own activations) samples exactly that sum.  In the MFMA loop the activation is
bf16(relu(pre')).  Where pre64_i is further than C e_pre from every rounding boundary (and from zero on the negative side)
pre'_i rounds to the SAME bf16 value: the element contributes no difference at all, which is why e_pre does not enter the
"mfma" tolerance through e_head.  Where it is within C e_pre of a boundary the kernel may land on the neighbouring value: one
ulp of the binade pre' may reach, times the weight -- that is flip_v, a worst case (every flippable element flips, every one
against the label).  One term beyond the plain flip count: near zero the bf16 grid is finer than e_pre itself (every
point is "within C e_pre of a boundary") and the two roundings differ by up to |pre' - pre64| plus one ulp, hence the added
C e_pre for those elements; it is a few 1e-6 times |W| and never decides a case.  The accumulation of the 16x16x32 MFMA is
fp32 with another summation order: e_head's C covers it.  FLOOR is the relative floor of the two references.

Candidates of a step: every v with z64_v + tol_v >= max_u (z64_u - tol_u).  One candidate: the path goes on with it.  Several:
the replay branches and follows each with its own state (blank against label changes the frame and the first-blank rule).
The acceptable set of an utterance is the set of token sequences at the leaves; the kernel's hypothesis must be a member.

The loop restated (csrc/greedy_decode.hip, rnnt_greedy_decoding.py:711-909): pending = LSTM(EW[row], (h, c)), g = W_pred h' +
b_pred, first with the SOS row (index V) on a zero state; per frame at most max_symbols evaluations of
argmax(W_head act(f_t + g) + b_head); blank ends the frame, and if it is the very first evaluation of the utterance the pending
state is rebuilt from EW[row_blank] on the zero state; a label is emitted, (h, c) <- pending, pending <- LSTM(EW[label]).
Lengths are clamped to [0, T].  cap: an utterance that emits more than `cap` tokens stops there (the kernel's overflow bit 0),
its sequences are the first `cap` tokens.
"""
import statistics

import torch

C = 4.0
FLOOR = 2.0 ** -20
MAX_SET = 16          # an acceptable set larger than this fails the case as badly chosen
TILE = 16             # frames per evaluation of the MFMA head


class BadlyChosenCase(AssertionError):
    pass


def bf16_round(x):
    """x (fp64) rounded to the nearest bf16 value, ties to even, and the bf16 ulp of its binade; no pass through fp32."""
    _, e = torch.frexp(x)
    ulp = torch.ldexp(torch.ones_like(x), e - 8)
    return torch.round(x / ulp) * ulp, ulp


def _ulp_bf16(x):
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), e - 8)


class _Side:
    """The operands of one precision."""

    def __init__(self, case, dt):
        s = "32" if dt == torch.float32 else ""
        self.f_all = case.get("f_all" + s, case["f_all"]).to(dt)
        self.EW = case.get("EW" + s, case["EW"]).to(dt)
        self.Whh, self.Wp, self.Wh = case["Whh"].to(dt), case["Wp"].to(dt), case["Wh"].to(dt)
        self.bp, self.bh = case["bp"].to(dt), case["bh"].to(dt)
        self.Hp = self.Whh.shape[1]
        self.zero = torch.zeros(self.Hp, dtype=dt)

    def pend(self, row, h, c):
        Hp = self.Hp
        g = self.Whh @ h + self.EW[row]
        i, f, gg, o = torch.sigmoid(g[:Hp]), torch.sigmoid(g[Hp:2 * Hp]), torch.tanh(g[2 * Hp:3 * Hp]), torch.sigmoid(g[3 * Hp:])
        cn = f * c + i * gg
        hn = o * torch.tanh(cn)
        return hn, cn, self.Wp @ hn + self.bp


class _Path:
    __slots__ = ("t", "s", "first", "emitted", "hc", "pend", "hyp", "main", "tile0", "over")

    def copy(self):
        p = _Path()
        for k in self.__slots__:
            setattr(p, k, getattr(self, k))
        p.hyp = list(self.hyp)
        return p


def _evaluate(S64, S32, b, path, rounding, absW):
    """One micro-step: (z64, tol [V] or None, e_pre, n_flippable)."""
    gp64 = path.pend[0][2]
    pre64 = S64.f_all[b, path.t] + gp64
    if rounding is None:
        return S64.Wh @ torch.relu(pre64) + S64.bh, None, 0.0, 0
    pre32 = S32.f_all[b, path.t] + path.pend[1][2]
    e_pre = float((pre32.double() - pre64).abs().max())
    flip, nflip = 0.0, 0
    if rounding == "mfma":
        act64, _ = bf16_round(torch.relu(pre64))
        z64 = S64.Wh @ act64 + S64.bh
        z32 = S32.Wh @ act64.float() + S32.bh
        r = C * e_pre
        ulp = _ulp_bf16(pre64.abs() + r)
        u = pre64.abs() / _ulp_bf16(pre64)
        dist = ((u - torch.floor(u)) - 0.5).abs() * _ulp_bf16(pre64)      # to the nearest midpoint of two bf16 values
        flippable = (pre64 > -r) & ((dist <= r) | (_ulp_bf16(pre64) <= 2 * r))
        nflip = int(flippable.sum())
        if nflip:
            q = ulp + torch.where(_ulp_bf16(pre64) <= 2 * r, torch.full_like(ulp, r), torch.zeros_like(ulp))
            flip = absW[:, flippable] @ q[flippable]
    else:
        z64 = S64.Wh @ torch.relu(pre64) + S64.bh
        z32 = S32.Wh @ torch.relu(pre32) + S32.bh
    e_head = float((z32.double() - z64).abs().max())
    tol = C * e_head + flip + FLOOR * float(z64.abs().max())
    if not torch.is_tensor(tol):
        tol = torch.full_like(z64, tol)
    return z64, tol, e_pre, nflip


def _decode_utterance(S64, S32, b, length, max_symbols, rounding, cap, blank, row_blank, row_sos, absW):
    sides = (S64,) if rounding is None else (S64, S32)
    root = _Path()
    root.t, root.s, root.first, root.emitted, root.hyp, root.main, root.tile0, root.over = 0, 0, True, False, [], True, 0, False
    root.hc = tuple((S.zero, S.zero) for S in sides)
    root.pend = tuple(S.pend(row_sos, S.zero, S.zero) for S in sides)
    stack, leaves, main_hyp, steps = [root], [], None, []
    counts = dict(steps=0, blanks=0, labels=0, multi=0, first_blank=0, emit_in_tile=0, cap_hits=0, overflow=False)

    def apply(p, k):
        if k == blank:
            if p.first and not p.emitted:      # no emission yet: the loop now feeds embedding[blank_idx] with a zero state
                p.pend = tuple(S.pend(row_blank, *hc) for S, hc in zip(sides, p.hc))
                if p.main:
                    counts["first_blank"] += 1
                p.tile0 = p.t + 1
            p.first = False
            p.t += 1; p.s = 0
            if p.t - p.tile0 >= TILE:
                p.tile0 += TILE
            return
        p.first = False; p.emitted = True
        if p.main and p.t > p.tile0:
            counts["emit_in_tile"] += 1
        p.hyp.append(k)
        if cap is not None and len(p.hyp) > cap:
            p.over = True
            return
        p.hc = tuple((pd[0], pd[1]) for pd in p.pend)
        p.pend = tuple(S.pend(k, *hc) for S, hc in zip(sides, p.hc))
        p.s += 1
        if p.s >= max_symbols:
            if p.main:
                counts["cap_hits"] += 1
            p.t += 1; p.s = 0
        p.tile0 = p.t

    while stack:
        p = stack.pop()
        while p.t < length and not p.over:
            z64, tol, e_pre, nflip = _evaluate(S64, S32, b, p, rounding, absW)
            best = int(torch.argmax(z64))      # torch.argmax: the first maximum
            if tol is None:
                cands = [best]
            else:
                cands = torch.nonzero(z64 + tol >= (z64 - tol).max()).flatten().tolist()
            if p.main:
                rest = z64.clone(); rest[best] = -float("inf")
                second = int(torch.argmax(rest))
                steps.append(dict(frame=p.t, symbol=p.s, choice=best, second=second, candidates=cands, margin=float(z64[best] - z64[second]),
                                  tol=0.0 if tol is None else float(tol.max()), e_pre=e_pre, flippable=nflip))
                counts["steps"] += 1
                counts["multi"] += int(len(cands) > 1)
                counts["blanks" if best == blank else "labels"] += 1
            for k in cands:
                if k != best:
                    q = p.copy(); q.main = False
                    apply(q, k)
                    stack.append(q)
            if len(stack) + len(leaves) > 4 * MAX_SET:
                raise BadlyChosenCase(f"utterance {b}: more than {4 * MAX_SET} open branches")
            apply(p, best)
        seq = tuple(p.hyp[:cap] if cap is not None else p.hyp)
        leaves.append(seq)
        if p.main:
            main_hyp = list(seq)
            counts["overflow"] = p.over
    accept = set(leaves)
    if len(accept) > MAX_SET:
        raise BadlyChosenCase(f"utterance {b}: acceptable set of {len(accept)} sequences")
    return dict(hyp=main_hyp, accept=accept, steps=steps, counts=counts)


def decode_reference(case, max_symbols, rounding, cap=None):
    """case: dict f_all [B,T,Hj], EW [V+1,4Hp], Whh [4Hp,Hp], Wp [Hj,Hp], bp, Wh [V,Hj], bh, lens [B] (the dict of
    tests/test_greedy_decode_gpu.py::_bf16_case; optional f_all32 / EW32: the fp32 images of operands given in fp64);
    blank = row_blank = V - 1, row_sos = V.  Returns one dict per utterance: hyp (main path), accept (set of tuples), steps
    (per micro-step of the main path: frame, symbol, choice, candidates, margin, tol, e_pre, flippable), counts."""
    assert rounding in ("mfma", "gemv", None)
    S64 = _Side(case, torch.float64)
    S32 = None if rounding is None else _Side(case, torch.float32)
    B, T, _ = S64.f_all.shape
    V = S64.Wh.shape[0]
    absW = S64.Wh.abs() if rounding == "mfma" else None
    out = []
    for b in range(B):
        length = min(max(int(case["lens"][b]), 0), T)
        out.append(_decode_utterance(S64, S32, b, length, int(max_symbols), rounding, cap, V - 1, V - 1, V, absW))
    return out


def summarize(results):
    """The figures of a case: micro-steps, tokens, blank share, multi-candidate steps, median / largest tol, smallest margin."""
    steps = [s for r in results for s in r["steps"]]
    n = len(steps)
    cnt = {k: sum(int(r["counts"][k]) for r in results) for k in ("blanks", "labels", "multi", "first_blank", "emit_in_tile", "cap_hits")}
    return dict(steps=n, tokens=sum(len(r["hyp"]) for r in results), blank_share=cnt["blanks"] / n if n else 0.0,
                label_share=cnt["labels"] / n if n else 0.0, multi=cnt["multi"],
                tol_median=statistics.median(s["tol"] for s in steps) if n else 0.0, tol_max=max((s["tol"] for s in steps), default=0.0),
                margin_min=min((s["margin"] for s in steps), default=float("inf")),
                sets_gt1=sum(int(len(r["accept"]) > 1) for r in results), set_max=max(len(r["accept"]) for r in results),
                first_blank=cnt["first_blank"], emit_in_tile=cnt["emit_in_tile"], cap_hits=cnt["cap_hits"])


def check_conditions(results, balanced=True):
    """The conditions that keep the acceptable set from hiding a failure, asserted on the reference alone."""
    s = summarize(results)
    B = len(results)
    assert s["multi"] <= 0.01 * s["steps"], ("multi-candidate steps", s)
    assert s["sets_gt1"] <= (0 if B <= 4 else 1), ("utterances with more than one acceptable sequence", s)
    assert s["set_max"] <= MAX_SET, s
    if balanced:
        assert s["blank_share"] >= 0.25 and s["label_share"] >= 0.25, ("blank / label balance", s)
        assert s["first_blank"] >= 1, ("no utterance starts with a blank", s)
        assert s["emit_in_tile"] >= 1, ("no emission from frame j > 0 of a tile", s)
        assert s["cap_hits"] >= 1, ("no frame reaches max_symbols", s)
    return s


def member(hyp, result):
    return tuple(hyp) in result["accept"]


@torch.no_grad()
def case_from_model(model, encoded, encoded_len, lang):
    """The operands greedy_rnnt_decode_device hands the kernel, rebuilt in fp64 from the model's parameters on the CPU: f_all =
    the joint's encoder projection, EW = W_ih embedding[row] + b_ih + b_hh over the labels, the blank / padding row and the
    zero SOS row, and -- for a model that computes in bf16 -- the bf16 images of W_hh, W_pred and the head.  f_all32 / EW32
    are the same two GEMMs in fp32, so that e_pre contains their fp32-against-fp64 difference."""
    dec, joint = model.decoder, model.joint
    cpu = lambda t: t.detach().cpu()
    head = joint.joint_net[-1][lang]
    lstm = dec.prediction["dec_rnn"].lstm
    emb = cpu(dec.prediction["embed"].weight).float()
    V = head.weight.shape[0]
    blank = V - 1
    Hp = lstm.hidden_size
    Hj = joint.pred.weight.shape[0]
    x = cpu(encoded).float().transpose(1, 2)                                            # [B, T, d]
    We, be = cpu(joint.enc.weight).float(), cpu(joint.enc.bias).float()
    rows = torch.cat([emb[:blank], emb[dec.blank_idx:dec.blank_idx + 1], torch.zeros(1, Hp)], 0)
    Wih, bih, bhh = cpu(lstm.weight_ih_l0).float(), cpu(lstm.bias_ih_l0).float(), cpu(lstm.bias_hh_l0).float()
    cfg = getattr(model, "cfg", None)
    w16 = cfg is not None and cfg.compute_dtype == "bf16" and Hp % 8 == 0 and Hj % 8 == 0
    img = (lambda p: cpu(p).float().bfloat16()) if w16 else (lambda p: cpu(p).float())
    return dict(f_all=x.double() @ We.double().t() + be.double(), f_all32=x @ We.t() + be,
                EW=rows.double() @ Wih.double().t() + bih.double() + bhh.double(), EW32=rows @ Wih.t() + (bih + bhh),
                Whh=img(lstm.weight_hh_l0), Wp=img(joint.pred.weight), bp=cpu(joint.pred.bias).float(),
                Wh=img(head.weight), bh=cpu(head.bias).float(), lens=cpu(encoded_len).long(), bf16=w16)
