"""The persistent LSTM kernels (csrc/lstm.hip behind ops/lstm.py) held to a rounding-faithful fp64 reference (oracle/lstm_ref.py).

K = the kernel's result, E = exact math in fp64 (rounding=None), F64 / F32 = the kernels' bf16 rounding points emulated in fp64 /
fp32 (rounding="kernel").  Distances are relative L2 and max-abs, each scaled by the reference tensor.  The bounds and their
constants are those of tests/test_block_reference_gpu.py, and no other:

  (a) d(K, F64) <= C * d(F32, F64) + FLOOR      C = 4, FLOOR = 2^-20
  (b) d(K, E)   <= 2 * d(F64, E) + FLOOR

(S) test_kernel_steps_match_single_step_reference -- ia_lstm_forward / ia_lstm_backward through the C ABI on test-supplied Gx,
W_hh, dHout (gates and Cs of the backward are the forward launch's).  Every step t of the reference starts from the KERNEL's
own previous-step outputs -- bf16 of its Hout[t-1] and its Cs[t-1]; bf16 of its dG[t+1], the dc carry being the reference
chain's own -- so nothing crosses a bf16 boundary between the two and (a) holds in its clean form, at fp32 size, for gates, Cs,
Hout and dG, all steps stacked, rows of the last partial 16-row tile apart from the rest.  Observed worst
d(K, F64step) / d(F32step, F64step) per case (init / x3 weights), every distance between 4e-8 and 4e-7:
  (1,3,64) 1.02 / 1.60   (2,1,64) 1.09 / 1.12   (3,1,64) 1.57 / 1.05   (9,15,128) 1.31 / 1.12   (9,16,128) 1.33 / 1.03
  (9,17,128) 1.22 / 1.82   (12,32,192) 1.05 / 1.02   (6,33,64) 1.12 / 1.54   (7,40,64) 1.17 / 1.34   (37,32,640) 1.58 / 1.88
  (3,2,768) 1.08 / 1.83   (5,4,96) 1.04 / 1.23 -- the launcher takes H = 96 (H % 32 == 0) and computes it correctly.
The hardware exp of sigmoidf_ stays well inside C.

(E) test_lstm_forward_backward_match_reference_end_to_end -- ops.lstm.lstm_forward + .backward(): the Gx GEMM, the transposes,
the dx GEMM and gemm_tn included, the bf16 weight images being part of what is tested.  (b) is asserted for y, dx, dW_ih, dW_hh,
db_ih and db_hh.  Observed worst d(K, E) / d(F64, E) over both metrics: 1.000 at every case but (9,17,128) 1.013 / 1.002,
(12,32,192) 1.000 / 1.032 and (37,32,640) 1.043 / 1.053 (d(F64, E) itself: 1.3e-3 ... 1.4e-2).
d(K, F64) / d(F32, F64) (relative L2) is measured and printed for every tensor and case, and asserted at C = 4 for the tensors
not named in E_A_HELD_BY_B_ONLY -- which names all six.  One bf16 hand-off landing the other way moves a whole row of the next
step (and one dG element rounding the other way a whole dx row and a column of each weight gradient); in the small cases
d(F32, F64) holds no such quantum (1e-7 for y, 3e-9 ... 1e-5 for the gradients) while the kernel's run holds one or two, or the
other way round (ratios down to 0.003).  Observed worst ratios: y 1017 at (9,15,128)x3 (d(K, F64) 1.1e-4 against 1.1e-7) and
294 at (9,17,128)x3; dx 543 at (7,40,64)init (1.4e-6 against 2.5e-9), 11.1 and 9.1 at (9,15,128)x3 / (9,16,128)x3; dW_ih 40.9,
dW_hh 78.1, db_ih = db_hh 41.2 at (9,15,128)x3 and 8.1 ... 9.4 at (7,40,64)init.  Wherever both runs hold many quanta the ratio
is near 1: (9,17,128)init 0.98 ... 1.00, (12,32,192) 0.04 ... 1.47, (6,33,64) 0.46 ... 1.12, (37,32,640) 0.87 ... 1.17.  These
tensors are held by (b) and by (S).  Every d(K, F64) seen is below 3.3e-3, i.e. below d(F64, E) of the same tensor.
The dx that ops/lstm.py returns is the dx GEMM's bf16 output; the emulation rounds there too, and at U = 1, where nothing else
can land differently, d(K, F64) of dx and of both bias gradients is exactly 0.

Inputs: nn.LSTM's default init with the prediction network's forget-gate bias (b_ih = 1, b_hh = 0 on that slice), as is and
scaled x3 (the trained-like saturating regime), not pre-rounded to bf16; x ~ 0.7 N(0,1), dy ~ N(0,1).

Behaviours, at (9,17,128): inference (gates = Cs = NULL) vs training call, a repeated launch on the same scratch, a launch with
the exchange region of the scratch (bytes >= 256) filled with NaN patterns, NaN-prefilled outputs, the needs_input_grad subsets,
the direct accumulation into pre-filled .grad buffers, a non-default stream, the launchers' refusals, lstm_supported's edges.

Arithmetic-only single-line faults, each built once and run against this file (hand-off protocol untouched):
  cell state rounded to bf16 after each step ........ (S) Cs and Hout, all 24 cases (d 1e-3 against 1e-7); bf16-sized, so (b)
                                                      alone would admit it
  hand-off value truncated instead of rounded ....... (S) gates (and Cs, Hout), all 22 cases with U > 1; bf16-sized likewise
  cprev read from step t instead of t-1 ............. (S) dG, all 22 cases with U > 1 (d 8e-2); (E) (b) of dx and dW_ih
  dcc times the forget gate of step t-1, not t ...... (S) dG, all 22 cases with U > 1 (d 1e-1); (E) (b) of dx and dW_ih
  dW_hh from Hout[1:] instead of Hout[:-1] .......... (E) (b) of dW_hh, all 20 cases with U > 1 (d 0.9 ... 1.1)
  db returned for b_ih only ......................... (E) db_hh missing, all 22 cases; the needs_input_grad (weights_only),
                                                      pre-filled .grad and non-default stream tests
"""
import pytest
import torch

from oracle import lstm_ref as R

pytestmark = pytest.mark.gpu

C = 4.0                # as in tests/test_block_reference_gpu.py
FLOOR = 2.0 ** -20
IA_INVALID_VALUE, IA_UNSUPPORTED = -1, -4

#         (U, B, H)        what it reaches
SHAPES = [(1, 3, 64),      # no hand-off at all, dW_hh = 0, c_{t-1} = 0 at t = 0
          (2, 1, 64),      # one exchange; B = 1 row clamping
          (3, 1, 64),      # both halves of the exchange buffer
          (9, 15, 128),    # one row tile, one row short
          (9, 16, 128),    # one row tile, full
          (9, 17, 128),    # two tiles, the second with a single live row
          (12, 32, 192),   # both tiles full; the backward's K split is 48 k-steps over 4 waves
          (6, 33, 64),     # the host's 32-row split with a 1-row tail
          (7, 40, 64),     # ... with an 8-row tail
          (37, 32, 640),   # the workload's H at a short U: 40 workgroups, 20 / 80 k-steps
          (3, 2, 768)]     # the largest H lstm_supported takes (157 184 B of the 160 KiB LDS)
ABI_ONLY = [(5, 4, 96)]    # lstm_check takes H % 32 == 0, the wrapper asks for H % 64
SCALES = [1.0, 3.0]


def _params(m):
    return m.weight_ih_l0.detach(), m.weight_hh_l0.detach(), m.bias_ih_l0.detach(), m.bias_hh_l0.detach()


# ---------------------------------------------------------------------------------------------------- the C ABI
def _scratch(B, H):
    from indic_cl_asr_amd import _lib
    n = _lib.lib().ia_lstm_scratch_bytes(B, H)
    return torch.zeros(n, dtype=torch.uint8, device="cuda"), n


def _no_timeout(sc):
    w = sc.view(torch.int32)
    assert int(w[1]) == 0 and int(w[32]) == 0, "a hand-off spin gave up"


def _abi_forward(gx, whh_b, train=True, fill=0.0, scratch=None):
    """ia_lstm_forward on gx [U, B, 4H] f32, whh_b [4H, H] bf16 (batches above 32 rows in 32-row launches, as ops/lstm.py
    splits them) -> (status, Hout, gates, Cs); outputs pre-filled with `fill`."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    U, B, H4 = gx.shape
    H = H4 // 4
    Hout = torch.full((U, B, H), fill, dtype=torch.float32, device="cuda")
    gates = torch.full((U, B, H4), fill, dtype=torch.float32, device="cuda") if train else None
    Cs = torch.full((U, B, H), fill, dtype=torch.float32, device="cuda") if train else None
    for b0 in range(0, B, 32):
        sl = slice(b0, min(B, b0 + 32))
        nb = sl.stop - sl.start
        part = [None if t is None else t[:, sl].contiguous() for t in (gx, Hout, gates, Cs)]
        sc, n = scratch if scratch is not None else _scratch(nb, H)
        st = L.ia_lstm_forward(_lib.ptr(part[0]), _lib.ptr(whh_b), _lib.ptr(part[1]), _lib.ptr(part[2]), _lib.ptr(part[3]), U, nb,
                               H, _lib.ptr(sc), n, _lib.stream_ptr())
        if st != 0:
            return st, None, None, None
        torch.cuda.synchronize()
        _no_timeout(sc)
        Hout[:, sl] = part[1]
        if train:
            gates[:, sl] = part[2]; Cs[:, sl] = part[3]
    return 0, Hout, gates, Cs


def _abi_backward(dy, gates, Cs, whhT_b, fill=0.0, scratch=None):
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    U, B, H = dy.shape
    dG = torch.full((U, B, 4 * H), fill, dtype=torch.float32, device="cuda")
    for b0 in range(0, B, 32):
        sl = slice(b0, min(B, b0 + 32))
        nb = sl.stop - sl.start
        part = [t[:, sl].contiguous() for t in (dy, gates, Cs, dG)]
        sc, n = scratch if scratch is not None else _scratch(nb, H)
        st = L.ia_lstm_backward(_lib.ptr(part[0]), _lib.ptr(part[1]), _lib.ptr(part[2]), _lib.ptr(whhT_b), _lib.ptr(part[3]), U,
                                nb, H, _lib.ptr(sc), n, _lib.stream_ptr())
        if st != 0:
            return st, None
        torch.cuda.synchronize()
        _no_timeout(sc)
        dG[:, sl] = part[3]
    return 0, dG


# ---------------------------------------------------------------------------------------------------- distances
class _Log:
    """Every ratio d(K, ref) / d(other, ref) a bound holds, and every bound that failed: all are measured and printed before
    the test asserts."""

    def __init__(self):
        self.rows, self.fails = [], []

    def check(self, tag, K, ref, other, factor, sel=None, max_abs=True, enforce=True):
        """d(K, ref) <= factor * d(other, ref) + FLOOR: relative L2 and (max_abs) max-abs, both scaled by the reference."""
        k, r, o = (t.double() if sel is None else t.double()[:, sel] for t in (K, ref, other))
        if r.numel() == 0:
            return
        s2, sm = max(float(r.norm()), 1e-30), max(float(r.abs().max()), 1e-30)
        for metric, dk, do in (("L2", float((k - r).norm()) / s2, float((o - r).norm()) / s2),
                               ("max", float((k - r).abs().max()) / sm, float((o - r).abs().max()) / sm)):
            if metric == "max" and not max_abs:
                continue
            self.rows.append((tag, metric, dk / max(do, 1e-30), dk, do))
            if enforce and not dk <= factor * do + FLOOR:
                self.fails.append((tag, metric, dk, do))

    def report(self, name, every=()):
        for key in sorted({r[0].split(":")[0] for r in self.rows}):
            rows = [r for r in self.rows if r[0].split(":")[0] == key]
            for w in (rows if key in every else [max(rows, key=lambda r: r[2])]):
                print(f"{name} {'' if key in every else 'worst '}{key} ratio {w[2]:.3f} ({w[1]} of {w[0]}: d(K, ref) {w[3]:.3e}, "
                      f"d(other, ref) {w[4]:.3e})")
        assert not self.fails, self.fails


def _row_parts(B):
    """Rows of the last partial 16-row tile apart from the rest (which holds every full tile)."""
    full = (B // 16) * 16 if B % 16 else B
    parts = [("full_tiles", torch.arange(0, full)), ("partial_tile", torch.arange(full, B))]
    covered = set(int(i) for _, s in parts for i in s)
    assert {b for b in range(B) if b % 16 in (0, 15)} | {B - 1} <= covered
    return [(n, s) for n, s in parts if s.numel()]


# ---------------------------------------------------------------------------------------------------- (S) spliced, C ABI
def _spliced(U, B, H, scale, may_refuse=False):
    m, x, dy = R.make_case(U, B, H, scale)
    w_ih, w_hh, b_ih, b_hh = _params(m)
    gx = R.input_projection(x, w_ih, b_ih, b_hh, torch.float64, "kernel")[0].float()   # test-supplied: no GEMM kernel here
    whh_b = w_hh.to(torch.bfloat16)
    st, Hout, gates, Cs = _abi_forward(gx.cuda(), whh_b.cuda(), fill=float("nan"))
    if may_refuse and st == IA_UNSUPPORTED:
        return
    assert st == 0, st
    st, dG = _abi_backward(dy.cuda(), gates, Cs, whh_b.t().contiguous().cuda(), fill=float("nan"))
    assert st == 0, st
    K = {"Hout": Hout.cpu(), "gates": gates.cpu(), "Cs": Cs.cpu(), "dG": dG.cpu()}
    for k, v in K.items():
        assert bool(torch.isfinite(v).all()), k   # every element written
    ref = {}
    for dt in (torch.float64, torch.float32):
        whh = whh_b.to(dt)
        bf = lambda t: t.to(torch.bfloat16).to(dt)
        zero = torch.zeros(B, H, dtype=dt)
        out = {"Hout": [], "gates": [], "Cs": [], "dG": [None] * U}
        for t in range(U):   # each step from the KERNEL's previous-step outputs
            g, c, h = R.fwd_step(bf(K["Hout"][t - 1]) if t else zero, K["Cs"][t - 1].to(dt) if t else zero, gx[t].to(dt), whh)
            out["gates"].append(g); out["Cs"].append(c); out["Hout"].append(h)
        dc = zero
        for t in range(U - 1, -1, -1):   # the kernel's bf16(dG[t+1]); the dc carry is the reference chain's own
            out["dG"][t], dc = R.bwd_step(dy[t].to(dt), bf(K["dG"][t + 1]) if t + 1 < U else None, K["gates"][t].to(dt),
                                          K["Cs"][t].to(dt), K["Cs"][t - 1].to(dt) if t else zero, dc, whh)
        ref[dt] = {k: torch.stack(v) for k, v in out.items()}
    log = _Log()
    for k in ("gates", "Cs", "Hout", "dG"):
        for pn, sel in _row_parts(B):
            log.check(f"S:{k}/{pn}", K[k], ref[torch.float64][k], ref[torch.float32][k], C, sel)
    log.report(f"({U},{B},{H})x{scale:g}")


@pytest.mark.parametrize("scale", SCALES, ids=["init", "x3"])
@pytest.mark.parametrize("U,B,H", SHAPES + ABI_ONLY)
def test_kernel_steps_match_single_step_reference(U, B, H, scale):
    """(S): bound (a), d(K_t, F64step_t) <= C d(F32step_t, F64step_t) + FLOOR over all steps stacked, for gates, Cs, Hout, dG."""
    _spliced(U, B, H, scale, may_refuse=(U, B, H) in ABI_ONLY)


# ---------------------------------------------------------------------------------------------------- (E) end to end
E_TENSORS = ("y", "dx", "dW_ih", "dW_hh", "db_ih", "db_hh")
# tensors whose d(K, F64) / d(F32, F64) cannot hold C = 4 at the small cases (a single hand-off quantum on one side only): the
# worst observed ratio and where; see the module docstring.  They are held by (b) and by the spliced check.
E_A_HELD_BY_B_ONLY = {"y": (1017, "(9,15,128)x3"), "dx": (543, "(7,40,64)init"), "dW_ih": (40.9, "(9,15,128)x3"),
                      "dW_hh": (78.1, "(9,15,128)x3"), "db_ih": (41.2, "(9,15,128)x3"), "db_hh": (41.2, "(9,15,128)x3")}


def _references(m, x, dy):
    out = {}
    for key, dt, rnd in (("E", torch.float64, None), ("F64", torch.float64, "kernel"), ("F32", torch.float32, "kernel")):
        r = R.run_lstm(x, *_params(m), dy=dy, dtype=dt, rounding=rnd)
        out[key] = {"y": r["Hout"], "dx": r["dx"], "dW_ih": r["dW_ih"], "dW_hh": r["dW_hh"], "db_ih": r["db"], "db_hh": r["db"]}
    return out


def _run_ops(m, x, dy, need=(True, True, True), prefill=None):
    """ops.lstm.lstm_forward + backward on a fresh cuda copy of `m`; need = requires_grad of (x, weights, biases)."""
    from indic_cl_asr_amd.ops.lstm import lstm_forward
    H = m.hidden_size
    mc = torch.nn.LSTM(H, H, 1).cuda()
    mc.load_state_dict(m.state_dict())
    mc.weight_ih_l0.requires_grad_(need[1]); mc.weight_hh_l0.requires_grad_(need[1])
    mc.bias_ih_l0.requires_grad_(need[2]); mc.bias_hh_l0.requires_grad_(need[2])
    names = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
    if prefill is not None:
        for n in names:
            getattr(mc, n).grad = prefill[n].cuda().clone()
    xc = x.cuda().requires_grad_(need[0])
    y = lstm_forward(xc, mc)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    from indic_cl_asr_amd.ops import lstm as hip_lstm
    hip_lstm.raise_if_timed_out()
    g = lambda p: None if p.grad is None else p.grad.detach().cpu()
    res = {"y": y.detach().cpu(), "dx": g(xc)}
    res.update({k: g(getattr(mc, n)) for k, n in zip(("dW_ih", "dW_hh", "db_ih", "db_hh"), names)})
    return res


@pytest.mark.parametrize("scale", SCALES, ids=["init", "x3"])
@pytest.mark.parametrize("U,B,H", SHAPES)
def test_lstm_forward_backward_match_reference_end_to_end(U, B, H, scale):
    """(E): bound (b), d(K, E) <= 2 d(F64, E) + FLOOR, and d(K, F64) against C d(F32, F64) + FLOOR (relative L2)."""
    m, x, dy = R.make_case(U, B, H, scale)
    ref = _references(m, x, dy)
    K = _run_ops(m, x, dy)
    log = _Log()
    for k in E_TENSORS:
        assert K[k] is not None, k
        if k == "dW_hh" and U == 1:
            assert float(K[k].abs().max()) == 0.0   # no recurrent step: exactly zero
            continue
        e, f64, f32 = ref["E"][k], ref["F64"][k], ref["F32"][k]
        # the reference alone stays inside (b) on these very values (tests/test_lstm_reference.py, here for every shape)
        assert float((f32.double() - e).norm()) <= 2 * float((f64 - e).norm()), k
        log.check(f"E(b):{k}", K[k][None], e[None], f64[None], 2.0)
        log.check(f"E(a):{k}", K[k][None], f64[None], f32[None], C, max_abs=False, enforce=k not in E_A_HELD_BY_B_ONLY)
    log.report(f"({U},{B},{H})x{scale:g}", every=("E(a)",))


# ---------------------------------------------------------------------------------------------------- behaviours
BU, BB, BH = 9, 17, 128


def _abi_inputs(U=BU, B=BB, H=BH, scale=3.0):
    m, x, dy = R.make_case(U, B, H, scale)
    w_ih, w_hh, b_ih, b_hh = _params(m)
    gx = R.input_projection(x, w_ih, b_ih, b_hh, torch.float64, "kernel")[0].float().cuda()
    return gx, w_hh.to(torch.bfloat16).cuda(), dy.cuda()


def _nan_fill_exchange(sc):
    sc[256:] = 0xFF           # bf16 0xFFFF = NaN in every exchange slot; the 256-byte sync header stays as the launch left it


def test_inference_repeat_and_stale_exchange_buffers_give_the_same_bits():
    gx, whh, dy = _abi_inputs()
    sc = _scratch(BB, BH)
    nan = float("nan")
    st, H1, G1, C1 = _abi_forward(gx, whh, fill=nan, scratch=sc)
    assert st == 0
    for t in (H1, G1, C1):
        assert bool(torch.isfinite(t).all())                         # every element written
    st, H0, _, _ = _abi_forward(gx, whh, train=False, fill=nan, scratch=sc)    # gates = Cs = NULL
    assert st == 0 and torch.equal(H0, H1)
    st, H2, G2, C2 = _abi_forward(gx, whh, fill=nan, scratch=sc)     # second launch on the same scratch
    assert st == 0 and torch.equal(H2, H1) and torch.equal(G2, G1) and torch.equal(C2, C1)
    _nan_fill_exchange(sc[0])
    st, H3, G3, C3 = _abi_forward(gx, whh, fill=nan, scratch=sc)
    assert st == 0 and torch.equal(H3, H1) and torch.equal(G3, G1) and torch.equal(C3, C1)
    whhT = whh.t().contiguous()
    st, D1 = _abi_backward(dy, G1, C1, whhT, fill=nan, scratch=sc)
    assert st == 0 and bool(torch.isfinite(D1).all())
    st, D2 = _abi_backward(dy, G1, C1, whhT, fill=nan, scratch=sc)
    assert st == 0 and torch.equal(D2, D1)
    _nan_fill_exchange(sc[0])
    st, D3 = _abi_backward(dy, G1, C1, whhT, fill=nan, scratch=sc)
    assert st == 0 and torch.equal(D3, D1)


@pytest.fixture(scope="module")
def all_on():
    m, x, dy = R.make_case(BU, BB, BH, 3.0)
    return m, x, dy, _run_ops(m, x, dy)


@pytest.mark.parametrize("need,present", [((True, False, False), ("dx",)),
                                          ((False, True, True), ("dW_ih", "dW_hh", "db_ih", "db_hh")),
                                          ((True, True, False), ("dx", "dW_ih", "dW_hh"))],
                         ids=["x_only", "weights_only", "biases_frozen"])
def test_needs_input_grad_subsets_match_the_all_on_run_bit_for_bit(all_on, need, present):
    m, x, dy, full = all_on
    K = _run_ops(m, x, dy, need=need)
    assert torch.equal(K["y"], full["y"])
    for k in E_TENSORS[1:]:
        if k in present:
            assert torch.equal(K[k], full[k]), k
        else:
            assert K[k] is None, k


def test_prefilled_grads_are_accumulated_directly(all_on):
    """ops/tail.accumulate_or_return adds into existing fp32 .grad buffers: prefill + the returned-tensor path's gradient, within
    the fp32 rounding of that one add (FLOOR); both biases, given the same prefill, end bit-identical."""
    m, x, dy, full = all_on
    g = torch.Generator().manual_seed(5)
    names = {"dW_ih": "weight_ih_l0", "dW_hh": "weight_hh_l0", "db_ih": "bias_ih_l0", "db_hh": "bias_hh_l0"}
    prefill = {}
    for k, n in names.items():
        src = prefill["bias_ih_l0"] if k == "db_hh" else None
        prefill[n] = src.clone() if src is not None else \
            torch.randn(full[k].shape, generator=g) * 0.5 * float(full[k].pow(2).mean().sqrt())
    K = _run_ops(m, x, dy, prefill=prefill)
    assert torch.equal(K["y"], full["y"]) and torch.equal(K["dx"], full["dx"])
    for k, n in names.items():
        got, want = K[k].double() - prefill[n].double(), full[k].double()
        assert float((got - want).norm()) <= FLOOR * float(want.norm()), k
        assert float((got - want).abs().max()) <= FLOOR * float(want.abs().max()), k
        assert not torch.equal(K[k], prefill[n])
    assert torch.equal(K["db_ih"], K["db_hh"])


def test_non_default_stream_gives_the_same_bits(all_on):
    m, x, dy, full = all_on
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        K = _run_ops(m, x, dy)
    torch.cuda.current_stream().wait_stream(s)
    for k in E_TENSORS:
        assert torch.equal(K[k], full[k]), k


def test_abi_refusals():
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    U, H = 2, 64

    def fwd(B, H, sc=None, n=None, gates=True, cs=True):
        buf, nn_ = _scratch(max(B, 1), H)
        sc = buf if sc is None else sc
        n = nn_ if n is None else n
        gx = torch.zeros(U, B, 4 * H, device="cuda")
        whh = torch.zeros(4 * H, H, dtype=torch.bfloat16, device="cuda")
        ho = torch.zeros(U, B, H, device="cuda")
        ga = torch.zeros(U, B, 4 * H, device="cuda") if gates else None
        c = torch.zeros(U, B, H, device="cuda") if cs else None
        st = L.ia_lstm_forward(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(ho), _lib.ptr(ga), _lib.ptr(c), U, B, H, _lib.ptr(sc), n,
                               _lib.stream_ptr())
        torch.cuda.synchronize()
        return st

    def bwd(B, H, sc=None, n=None):
        buf, nn_ = _scratch(max(B, 1), H)
        sc = buf if sc is None else sc
        n = nn_ if n is None else n
        z = lambda *s: torch.zeros(*s, device="cuda")
        whhT = torch.zeros(H, 4 * H, dtype=torch.bfloat16, device="cuda")
        st = L.ia_lstm_backward(_lib.ptr(z(U, B, H)), _lib.ptr(z(U, B, 4 * H)), _lib.ptr(z(U, B, H)), _lib.ptr(whhT),
                                _lib.ptr(z(U, B, 4 * H)), U, B, H, _lib.ptr(sc), n, _lib.stream_ptr())
        torch.cuda.synchronize()
        return st

    assert fwd(4, H) == 0 and bwd(4, H) == 0                                  # the same calls are taken when nothing is wrong
    assert fwd(33, H) == IA_UNSUPPORTED and bwd(33, H) == IA_UNSUPPORTED
    assert fwd(4, 48) == IA_UNSUPPORTED and bwd(4, 48) == IA_UNSUPPORTED
    n = L.ia_lstm_scratch_bytes(4, H)
    assert fwd(4, H, n=n - 1) == IA_INVALID_VALUE and bwd(4, H, n=n - 1) == IA_INVALID_VALUE
    big = torch.zeros(n + 256, dtype=torch.uint8, device="cuda")
    assert big.data_ptr() % 256 == 0
    assert fwd(4, H, sc=big[128:], n=n) == IA_INVALID_VALUE and bwd(4, H, sc=big[128:], n=n) == IA_INVALID_VALUE
    assert fwd(4, H, gates=True, cs=False) == IA_INVALID_VALUE


def test_lstm_supported_edges():
    from indic_cl_asr_amd import _lib
    from indic_cl_asr_amd.ops.lstm import lstm_supported
    x = torch.zeros(1, 1, 8, device="cuda")
    assert _lib.lib().ia_lstm_lds_bytes(768, 0) == 157184 <= 160 * 1024
    assert lstm_supported(x, 768)
    assert not lstm_supported(x, 832) and not lstm_supported(x, 100)
