"""oracle/lstm_ref.py (functional LSTM with selectable rounding, the reference of tests/test_lstm_reference_gpu.py) pinned to
torch.nn.LSTM: with rounding=None in fp64 both are the same math; its single-step functions are the whole recurrence; and its
fp32 run stays close enough to its fp64 run that the reference alone cannot use up bound (b) of the GPU tests."""
import pytest
import torch

from oracle import lstm_ref as R

TENSORS = ("Hout", "gates", "Cs", "dG", "dx", "dW_ih", "dW_hh", "db")


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _params(m):
    return m.weight_ih_l0.detach(), m.weight_hh_l0.detach(), m.bias_ih_l0.detach(), m.bias_hh_l0.detach()


@pytest.mark.parametrize("U,B,H", [(5, 3, 64), (1, 2, 64)])
def test_exact_reference_equals_nn_lstm_in_double(U, B, H):
    m, x, dy = R.make_case(U, B, H, 1.0, U + B)
    m = m.double()
    xr = x.double().requires_grad_(True)
    y, _ = m(xr)
    y.backward(dy.double())
    r = R.run_lstm(x, *_params(m), dy=dy, dtype=torch.float64, rounding=None)
    assert _rel(r["Hout"], y.detach()) <= 1e-11
    assert _rel(r["dx"], xr.grad) <= 1e-11
    assert _rel(r["dW_ih"], m.weight_ih_l0.grad) <= 1e-11
    if U > 1:
        assert _rel(r["dW_hh"], m.weight_hh_l0.grad) <= 1e-11
    else:   # no recurrence: exactly zero on both sides
        assert float(r["dW_hh"].abs().max()) == 0.0 and float(m.weight_hh_l0.grad.abs().max()) == 0.0
    assert _rel(r["db"], m.bias_ih_l0.grad) <= 1e-11 and _rel(r["db"], m.bias_hh_l0.grad) <= 1e-11
    assert _rel(m.bias_ih_l0.grad, m.bias_hh_l0.grad) <= 1e-11   # both biases receive the same gradient


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["fp64", "fp32"])
@pytest.mark.parametrize("U,B,H", [(4, 17, 64), (1, 3, 64)])
def test_single_steps_chained_reproduce_the_full_function_bit_for_bit(U, B, H, dtype):
    m, x, dy = R.make_case(U, B, H, 3.0, 11)
    w_ih, w_hh, b_ih, b_hh = _params(m)
    full = R.run_lstm(x, w_ih, w_hh, b_ih, b_hh, dy=dy, dtype=dtype, rounding="kernel")
    whh = w_hh.to(dtype).to(torch.bfloat16).to(dtype)
    bf = lambda t: t.to(torch.bfloat16).to(dtype)
    zero = torch.zeros(B, H, dtype=dtype)
    for t in range(U):   # every step from the FULL run's previous-step outputs, the way the GPU test splices a kernel's
        g, c, h = R.fwd_step(bf(full["Hout"][t - 1]) if t else zero, full["Cs"][t - 1] if t else zero, full["Gx"][t], whh)
        assert torch.equal(g, full["gates"][t]) and torch.equal(c, full["Cs"][t]) and torch.equal(h, full["Hout"][t]), t
    dc = zero
    for t in range(U - 1, -1, -1):
        dg, dc = R.bwd_step(dy[t].to(dtype), bf(full["dG"][t + 1]) if t + 1 < U else None, full["gates"][t], full["Cs"][t],
                            full["Cs"][t - 1] if t else zero, dc, whh)
        assert torch.equal(dg, full["dG"][t]), t


def test_kernel_rounding_is_live_and_bf16_sized():
    m, x, dy = R.make_case(6, 5, 64, 1.0, 3)
    E = R.run_lstm(x, *_params(m), dy=dy, dtype=torch.float64, rounding=None)
    F = R.run_lstm(x, *_params(m), dy=dy, dtype=torch.float64, rounding="kernel")
    for k in TENSORS:
        assert 2e-4 < _rel(F[k], E[k]) < 2e-2, k


# the recipes of tests/test_lstm_reference_gpu.py CASES (both weight regimes of every shape but the workload-sized ones, which
# the GPU test itself holds to the same condition on the same values before it looks at the kernel)
@pytest.mark.parametrize("scale", [1.0, 3.0], ids=["init", "x3"])
@pytest.mark.parametrize("U,B,H", [(1, 3, 64), (2, 1, 64), (3, 1, 64), (9, 15, 128), (9, 16, 128), (9, 17, 128), (12, 32, 192),
                                   (6, 33, 64), (7, 40, 64), (5, 4, 96)])
def test_fp32_emulation_is_at_most_twice_as_far_from_exact_as_the_fp64_emulation(U, B, H, scale):
    """d(F32, E) <= 2 d(F64, E) for every compared tensor: the reference's own fp32 noise leaves room under bound (b)."""
    m, x, dy = R.make_case(U, B, H, scale)
    P = _params(m)
    E = R.run_lstm(x, *P, dy=dy, dtype=torch.float64, rounding=None)
    F64 = R.run_lstm(x, *P, dy=dy, dtype=torch.float64, rounding="kernel")
    F32 = R.run_lstm(x, *P, dy=dy, dtype=torch.float32, rounding="kernel")
    for k in TENSORS:
        if k == "dW_hh" and U == 1:
            assert float(F32[k].abs().max()) == 0.0 and float(F64[k].abs().max()) == 0.0
            continue
        s2, sm = float(E[k].norm()), float(E[k].abs().max())
        d32, d64 = F32[k].double() - E[k], F64[k] - E[k]
        assert float(d32.norm()) / s2 <= 2 * float(d64.norm()) / s2, (k, "rel L2")
        assert float(d32.abs().max()) / sm <= 2 * float(d64.abs().max()) / sm, (k, "max abs")
