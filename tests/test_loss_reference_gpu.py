"""csrc/ctc.hip and csrc/rnnt_loss.hip against the fp64 restatement of oracle/loss_ref.py, every element compared, at every
template instantiation their dispatch can select and on both sides of every width boundary (tables in tests/loss_cases.py):

  ctc_alpha_beta<K, PF, LOGITS>   K = 1, 2, 4, 8 by the padded target width S in {0, 1, 31 | 32, 63 | 64, 127 | 128, 255}, both
                                  forms (log-probabilities through losses.ctc._CTCHip, raw logits through the C ABI as ops/tail.py
                                  calls it), ragged rows inside each batch: Tb = 0, 1, 2, 3, 5, tight feasible, infeasible by one
                                  frame, the unique path, empty transcripts
  ctc_row_lse_kernel              V = 2 .. 600 (the tail loop above 512 columns), NaN in the padding columns
  rnnt_lse_gather<NV>             NV = 1 .. 8 and the generic path, V on both sides of 64 and 512
  rnnt_grad                       V = 1, 2, 3 (the per-element branch) and V >= 4
  rnnt_alpha_beta<K, PF>          K = 1, 2, 4, 8, 16 by U1 in {1, 2, 63 | 64, 127 | 128, 255 | 256, 511 | 512, 1023}

Tolerances come from the reference alone.  For each case and quantity, e32 = max |ref(float32) - ref(float64)| is the error
the identical recurrence makes in fp32 with correctly rounded exp / log; the kernel is allowed

    |kernel - ref64| <= MARGIN * e32 + ULPS * 2^-23 * scale         MARGIN = 8, ULPS = 4

(MARGIN: v_exp_f32 / v_log_f32 are about 1 ulp each where numpy rounds correctly, exp(x) = exp2(x log2 e) adds |x| 2^-24
relative, and the three-term sums run in another order; scale = max(1, max |nll|) for nll, costs and lattice values, max(1,
max |upstream weight|) for gradients.)  The bf16 gradient operand of the logits form adds half a bf16 ulp of the value being
rounded, 2^(floor(log2 |v|) - 8) with |v| <= |ref| + the fp32 bound: between 2^-9 |v| and 2^-8 |v|.

Largest e32 over the tables (CPU), the resulting largest bound, and the largest error observed on the MI355X:

    quantity                       max e32     max bound          observed (worst error / bound of its case: at most)
    CTC log-prob form   nll        4.9e-3      5.0e-2             4.9e-3   0.13
                        gradient   1.2e-2      9.4e-2             1.3e-2   0.16
    CTC logits form     lse        3.9e-6      1.0e-4             3.9e-6   0.09
                        nll        4.9e-3      4.9e-2             4.9e-3   0.15
                        gradient   1.2e-2      9.4e-2 (+ bf16)    1.6e-2   (bf16 rounding included)
    CTC T = 3000        nll        1.9e-2      1.6e-1             1.9e-2   0.12
                        gradient   1.5e-2      1.2e-1             1.6e-2   0.13
    RNNT                costs      1.5e-3      1.4e-2             1.5e-3   0.12
                        alphas     2.1e-3      1.7e-2             2.1e-3   0.15
                        betas      2.5e-3      2.1e-2             2.5e-3   0.12
                        gradient   3.0e-3      2.4e-2             3.0e-3   0.53

The large figures belong to the cases at logit scale 30 and to the long lattices, where |nll| reaches 2.2e4 (one fp32 ulp:
2e-3) and the gradient subtracts sums of that size.  Every bound is per case: over the CTC table the nll bound runs from 5e-6
(S = 0) to 1.2e-2 (S = 255, |nll| = 2.7e3) at logit scale 1.5, the transducer bounds from 5e-7 (U1 = 1) to 2e-2 (U1 = 1023).

Arithmetic mutants of the kernels this file was run against once (each fails the listed cases): the
`other != l` term of skip[] dropped in ctc_alpha_beta (every S >= 31 batch); the beta direction's cross-lane s+2 neighbour taken
from prev[0] (every S >= 32 batch with more than one label, K = 2, 4, 8); the last register column left out of rnnt_lse_gather<3>
(V = 129, 192).  The alpha direction's `n2` is dead for K >= 2 -- a lane's first state is even, a blank, and never takes the
s-2 transition -- so no test can tell which register it is taken from.
"""
import numpy as np
import pytest
import torch

import loss_cases as LC

pytestmark = pytest.mark.gpu


def _cmp(what, got, ref, limit, extra=None):
    """max |got - ref| <= limit (+ extra, elementwise); prints the figure before it asserts."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    assert not np.isnan(got).any(), what
    lim = limit if extra is None else limit + extra
    worst = float(err.max()) if err.size else 0.0
    print(f"[loss-ref] {what}: err {worst:.3e} bound {float(limit):.3e}")
    assert (err <= lim).all(), (what, worst, float(limit))


def _dev(c):
    return (torch.tensor(c["targets"]).cuda(), torch.tensor(c["il"]).cuda(), torch.tensor(c["tl"]).cuda(),
            torch.tensor(c["w"]).cuda())


def _exact_zero_mask(c):
    """[B,T]: frames whose gradient must be exactly zero: infeasible rows, upstream weight 0, t >= in_len."""
    dead = ~c["r64"]["feasible"] | (c["w"] == 0)
    return dead[:, None] | (np.arange(c["T"])[None, :] >= c["il"][:, None])


# ------------------------------------------------------------------------------------------------ CTC, log-prob form
def _check_ctc_lp(c, tag):
    from indic_cl_asr_amd.losses.ctc import _CTCHip, ctc_hip_supported
    tg, il, tl, w = _dev(c)
    r = c["r64"]
    f = r["feasible"]
    for zero_infinity in (True, False):
        lp = torch.tensor(c["x"]).cuda().requires_grad_(True)
        assert ctc_hip_supported(lp, tg)
        nll = _CTCHip.apply(lp, tg, il, tl, c["blank"], zero_infinity)
        nll.backward(w)
        got = nll.detach().cpu().numpy()
        _cmp(f"ctc-{tag} nll", got[f], r["nll"][f], c["b_nll"])
        assert (got[~f] == (0.0 if zero_infinity else np.inf)).all(), got[~f]
        g = lp.grad.cpu().numpy()
        _cmp(f"ctc-{tag} grad", g, r["grad_lp"] * c["w"].astype(np.float64)[:, None, None], c["b_grad"])
        assert not g[_exact_zero_mask(c)].any()


@pytest.mark.parametrize("S,V,scale", LC.CTC_TABLE)
def test_ctc_logprob_form_every_width(S, V, scale):
    _check_ctc_lp(LC.ctc_case(S, V, scale, "lp"), "lp")


@pytest.mark.parametrize("kind", ["outside", "label"])
def test_ctc_logprob_form_with_minus_infinity(kind):
    c = LC.ctc_neginf_case(kind)
    assert c["r64"]["feasible"][0] and np.isinf(c["x"]).any()
    _check_ctc_lp(c, "lp")


def test_ctc_logprob_form_long_utterance():
    _check_ctc_lp(LC.ctc_long_case("lp"), "lp-T3000")


@pytest.mark.parametrize("reduction", ["none", "sum", "mean", "mean_batch", "mean_volume"])
def test_ctc_wrapper_reductions(reduction):
    import torch.nn.functional as F
    from indic_cl_asr_amd.losses.ctc import CTCLoss
    c = LC.ctc_case(31, 17, 1.5, "lp")
    tg, il, tl, w = _dev(c)
    B = c["B"]
    assert (c["tl"] == 0).any() and (~c["r64"]["feasible"]).any()          # clamp(min=1) of 'mean', zero_infinity
    lp = torch.tensor(c["x"]).cuda().requires_grad_(True)
    out = CTCLoss(num_classes=c["V"] - 1, zero_infinity=True, reduction=reduction)(lp, tg, il, tl)
    (out * w).sum().backward() if reduction == "none" else out.backward()

    lpr = torch.tensor(c["x"], dtype=torch.double).requires_grad_(True)
    args = (lpr.transpose(0, 1), torch.tensor(c["targets"]), torch.tensor(c["il"]), torch.tensor(c["tl"]))
    if reduction in ("none", "sum", "mean"):
        ref = F.ctc_loss(*args, blank=c["V"] - 1, reduction=reduction, zero_infinity=True)
    else:
        ref = F.ctc_loss(*args, blank=c["V"] - 1, reduction="none", zero_infinity=True)
        ref = ref.mean() if reduction == "mean_batch" else ref.sum() / torch.tensor(c["tl"]).sum()
    (ref * torch.tensor(c["w"], dtype=torch.double)).sum().backward() if reduction == "none" else ref.backward()
    # d out / d nll_b, and the same reduction of the fp32 replay for e32
    tlc = np.maximum(c["tl"], 1).astype(np.float64)
    coef = {"none": c["w"].astype(np.float64), "sum": np.ones(B), "mean": 1.0 / tlc / B, "mean_batch": np.ones(B) / B,
            "mean_volume": np.ones(B) / c["tl"].sum()}[reduction]
    f = c["r64"]["feasible"]
    n64, n32 = np.where(f, c["r64"]["nll"], 0.0), np.where(f, c["r32"]["nll"], 0.0).astype(np.float64)
    if reduction == "none":
        e, scale = np.abs(n32 - n64).max(), np.abs(n64).max()
    else:
        e, scale = abs((coef * (n32 - n64)).sum()), abs((coef * n64).sum())
    _cmp(f"ctc-wrapper {reduction}", out.detach().cpu().numpy(), ref.detach().numpy(), LC.bound(e, max(1.0, scale)))
    eg = np.abs(coef[:, None, None] * (c["r32"]["grad_lp"].astype(np.float64) - c["r64"]["grad_lp"])).max()
    _cmp(f"ctc-wrapper {reduction} grad", lp.grad.cpu().numpy(), lpr.grad.numpy(), LC.bound(eg, max(1.0, np.abs(coef).max())))


# -------------------------------------------------------------------------------------------------- CTC, logits form
def _half_bf16_ulp(v):
    """Half a bf16 ulp (8 significand bits) of |v|: 2^(floor(log2 |v|) - 8); 0 at 0."""
    v = np.abs(v)
    out = np.zeros_like(v)
    nz = v > 0
    out[nz] = np.exp2(np.floor(np.log2(v[nz])) - 8)
    return out


def _run_logits(c, ld, nan_pad, ldg, grad_scale=1.0, zero_infinity=True):
    """The calls of ops/tail.py's CTC node on logits with row stride ld: row lse, forward, backward.  Returns (lse [B,T],
    nll [B], bf16 gradient [B,T,ldg])."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    B, T, V, S = c["B"], c["T"], c["V"], c["S"]
    tg, il, tl, w = _dev(c)
    x = torch.full((B, T, ld), float("nan") if nan_pad else 0.0, device="cuda")
    x[:, :, :V] = torch.tensor(c["x"]).cuda()
    lse = torch.empty(B * T, device="cuda")
    _lib.check(L.ia_ctc_row_lse(_lib.ptr(x), ld, B * T, V, _lib.ptr(lse), _lib.stream_ptr()), "ia_ctc_row_lse")
    n = L.ia_ctc_workspace_bytes(B, T, S)
    assert n > 0
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    nll = torch.empty(B, device="cuda")
    _lib.check(L.ia_ctc_forward_logits(_lib.ptr(x), ld, _lib.ptr(lse), _lib.ptr(tg), _lib.ptr(il), _lib.ptr(tl), B, T, V, S, c["blank"],
                                       int(zero_infinity), _lib.ptr(nll), _lib.ptr(ws), n, _lib.stream_ptr()), "ia_ctc_forward_logits")
    dy = torch.full((B, T, ldg), 7.0, dtype=torch.bfloat16, device="cuda")
    _lib.check(L.ia_ctc_backward_logits(_lib.ptr(x), ld, _lib.ptr(lse), _lib.ptr(tg), _lib.ptr(il), _lib.ptr(tl), B, T, V, S, c["blank"],
                                        _lib.ptr(w), float(grad_scale), _lib.ptr(dy), ldg, _lib.ptr(ws), n, _lib.stream_ptr()),
               "ia_ctc_backward_logits")
    torch.cuda.synchronize()
    return lse.view(B, T).cpu(), nll.cpu(), dy.cpu()


def _check_ctc_logits(c, tag):
    V, T = c["V"], c["T"]
    r = c["r64"]
    f = r["feasible"]
    v8 = (V + 7) // 8 * 8
    lse, nll, dy = _run_logits(c, v8, False, v8)
    live = np.arange(T)[None, :] < c["il"][:, None]
    _cmp(f"ctc-{tag} lse", lse.numpy()[live], r["lse"][live], c["b_lse"])
    _cmp(f"ctc-{tag} nll", nll.numpy()[f], r["nll"][f], c["b_nll"])
    assert (nll.numpy()[~f] == 0.0).all()
    g = dy.float().numpy()
    ref = r["grad_logits"] * c["w"].astype(np.float64)[:, None, None]
    _cmp(f"ctc-{tag} grad", g[:, :, :V], ref, c["b_grad"], extra=_half_bf16_ulp(np.abs(ref) + c["b_grad"]))
    assert not g[:, :, V:].any()                                             # the padding columns of the GEMM operand
    assert not g[_exact_zero_mask(c)].any()
    # a wider row stride with NaN in every padding column of the logits, a wider gradient row: nothing may change
    lse2, nll2, dy2 = _run_logits(c, V + 24, True, v8 + 8)
    assert torch.equal(lse2, lse) and torch.equal(nll2, nll)
    assert torch.equal(dy2[:, :, :V], dy[:, :, :V]) and not dy2[:, :, V:].float().abs().max() > 0
    # without zero_infinity the infeasible rows report inf and still get an exactly zero gradient
    _, nll3, dy3 = _run_logits(c, v8, False, v8, zero_infinity=False)
    assert np.isinf(nll3.numpy()[~f]).all() and torch.equal(nll3[torch.tensor(f)], nll[torch.tensor(f)]) and torch.equal(dy3, dy)
    # grad_scale: a power of two commutes with both roundings (the fp32 product, the bf16 store) wherever neither value is
    # subnormal; below 2^-100 only the magnitude is held
    for s in (0.5, 128.0):
        _, _, dys = _run_logits(c, v8, False, v8, grad_scale=s)
        want = (dy.float() * s).bfloat16()
        normal = want.float().abs() >= 2.0 ** -100
        assert torch.equal(dys[normal], want[normal]), s
        assert float((dys.float() - want.float())[~normal].abs().max() if (~normal).any() else 0.0) <= 2.0 ** -100


@pytest.mark.parametrize("S,V,scale", LC.CTC_TABLE_LOGITS)
def test_ctc_logits_form_every_width(S, V, scale):
    _check_ctc_logits(LC.ctc_case(S, V, scale, "logits"), "logits")


def test_ctc_logits_form_long_utterance():
    _check_ctc_logits(LC.ctc_long_case("logits"), "logits-T3000")


# ------------------------------------------------------------------------------------------------------------ RNNT
@pytest.mark.parametrize("U1,T,V", LC.RNNT_TABLE)
def test_rnnt_every_variant(U1, T, V):
    from indic_cl_asr_amd.losses.rnnt import rnnt_alphas_betas, rnnt_loss_hip
    for fastemit, clamp in LC.RNNT_MODES:
        c = LC.rnnt_case(U1, T, V, fastemit, clamp)
        B, r = c["B"], c["r64"]
        labels, flen, glen = (torch.tensor(c[k]).cuda() for k in ("labels", "flen", "glen"))
        acts = torch.tensor(c["logits"]).cuda()
        costs, grads, ws = rnnt_loss_hip(acts, labels, flen, glen, c["blank"], fastemit, clamp, inplace=False)
        assert torch.equal(acts.cpu(), torch.tensor(c["logits"]))            # out of place leaves the logits alone
        al, be = rnnt_alphas_betas(ws, flen, glen, B, T, U1)
        tag = f"rnnt fe={fastemit} clamp={clamp}"
        _cmp(f"{tag} costs", costs.cpu().numpy(), r["costs"], c["b_costs"])
        _cmp(f"{tag} alphas", al.cpu().numpy(), r["alphas"], c["b_alphas"])
        _cmp(f"{tag} betas", be.cpu().numpy(), r["betas"], c["b_betas"])
        g = grads.cpu().numpy()
        _cmp(f"{tag} grad", g, r["grads"], c["b_grads"])
        outside = (np.arange(T)[None, :, None] >= c["flen"][:, None, None]) | (np.arange(U1)[None, None, :] > c["glen"][:, None, None])
        assert not g[outside].any() and not al.cpu().numpy()[outside].any() and not be.cpu().numpy()[outside].any()
        acts2 = acts.clone()
        costs2, grads2, ws2 = rnnt_loss_hip(acts2, labels, flen, glen, c["blank"], fastemit, clamp, inplace=True)
        assert grads2.data_ptr() == acts2.data_ptr()
        al2, be2 = rnnt_alphas_betas(ws2, flen, glen, B, T, U1)
        assert torch.equal(costs2, costs) and torch.equal(grads2, grads) and torch.equal(al2, al) and torch.equal(be2, be)
