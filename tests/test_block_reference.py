"""oracle/block_ref.py (functional ConformerLayer with selectable rounding, the reference of tests/test_block_reference_gpu.py)
pinned to oracle/step_ref.ConformerLayer: with rounding=None in fp64 both are the same math, so output, input gradient,
every parameter gradient and the BatchNorm running statistics agree to 1e-10 relative on a ragged batch with padded frames."""
import pytest
import torch

from oracle import block_ref as R
from oracle import step_ref as S


def _rel(a, b):
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


@pytest.mark.parametrize("d,H,B,T,lens", [(144, 4, 3, 20, (20, 11, 1)), (64, 2, 2, 17, (17, 9))])
def test_exact_reference_equals_step_ref_conformer_layer(d, H, B, T, lens, monkeypatch):
    # step_ref's convolution module casts to fp32 after the GLU (x.float(), conformer_modules.py:351): kept a no-op for fp64
    # tensors here so that the whole oracle block runs in fp64
    f32 = torch.Tensor.float
    monkeypatch.setattr(torch.Tensor, "float", lambda t: t if t.dtype == torch.float64 else f32(t))
    torch.manual_seed(d + T)
    m = S.ConformerLayer(d, 4 * d, H, 31).double().train()
    with torch.no_grad():
        m.self_attn.pos_bias_u.normal_(0, 0.2); m.self_attn.pos_bias_v.normal_(0, 0.2)
        m.conv.batch_norm.weight.uniform_(0.5, 1.5); m.conv.batch_norm.bias.normal_(0, 0.2)
        m.conv.batch_norm.running_mean.normal_(0, 0.1); m.conv.batch_norm.running_var.uniform_(0.5, 2.0)
    lens_t = torch.tensor(lens)
    x = torch.randn(B, T, d, dtype=torch.float64)
    pe = torch.randn(2 * T - 1, d, dtype=torch.float64) * 0.5
    dout = torch.randn(B, T, d, dtype=torch.float64)
    P = R.params_of(m, torch.float64)
    bn = m.conv.batch_norm
    state = [bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()]
    out_r, dx_r, g_r = R.run_block(x.reshape(B * T, d), P, lens_t, pe, B, T, H, dout=dout.reshape(B * T, d), bn_state=state)
    # the oracle module: NeMo's masks (conformer_encoder.py _create_masks)
    valid = torch.arange(T)[None, :] < lens_t[:, None]
    att_mask = ~(valid[:, None, :] & valid[:, :, None])
    xo = x.clone().requires_grad_(True)
    out_o = m(xo, att_mask, pe.unsqueeze(0), ~valid)
    out_o.backward(dout)
    assert _rel(out_r, out_o.detach().reshape(B * T, d)) <= 1e-10
    assert _rel(dx_r, xo.grad.reshape(B * T, d)) <= 1e-10
    for n, q in m.named_parameters():
        if n in ("conv.depthwise_conv.bias", "self_attn.linear_k.bias"):
            # structurally zero (BatchNorm removes a per-channel constant, softmax a per-query one): both sides are fp64
            # cancellation noise, held against the scale of the same module's weight gradient
            scale = float(g_r[n.replace(".bias", ".weight")].norm())
            assert float(g_r[n].norm()) <= 1e-10 * scale and float(q.grad.norm()) <= 1e-10 * scale, n
            continue
        assert _rel(g_r[n], q.grad) <= 1e-10, n
    assert _rel(state[0], bn.running_mean) <= 1e-10 and _rel(state[1], bn.running_var) <= 1e-10
    assert int(state[2]) == int(bn.num_batches_tracked) == 1
    # padded frames are covered: their rows are non-zero on both sides (norm_out of the residual) and enter the statistics
    pad = ~valid.reshape(-1)
    assert out_o.detach().reshape(B * T, d)[pad].abs().max() > 0


def test_executor_rounding_changes_values_by_bf16_sized_amounts_only():
    """rounding="executor" differs from the exact reference by a bf16-sized amount (not zero: the rounding points are live;
    not large: they are roundings, not different math), and its fp32 run is close to its fp64 run."""
    torch.manual_seed(0)
    d, H, B, T = 64, 2, 2, 17
    m = S.ConformerLayer(d, 4 * d, H, 31).train()
    lens = torch.tensor([17, 9])
    x = torch.randn(B * T, d, dtype=torch.float64)
    pe = (torch.randn(2 * T - 1, d) * 0.5).to(torch.bfloat16).double()
    dout = torch.randn(B * T, d, dtype=torch.float64)
    st = lambda dt: [torch.zeros(d, dtype=dt), torch.ones(d, dtype=dt), torch.zeros((), dtype=torch.long)]
    res = {}
    for key, dt, rnd in (("E", torch.float64, None), ("F64", torch.float64, "executor"), ("F32", torch.float32, "executor")):
        res[key] = R.run_block(x.to(dt), R.params_of(m, dt), lens, pe.to(dt), B, T, H, dout=dout.to(dt), rounding=rnd,
                               bn_state=st(dt))
    e_out, e_dx = res["E"][0], res["E"][1]
    f_out, f_dx = res["F64"][0], res["F64"][1]
    assert 1e-4 < _rel(f_out, e_out) < 3e-2 and 1e-4 < _rel(f_dx, e_dx) < 5e-2
    assert _rel(res["F32"][0].double(), f_out) < _rel(f_out, e_out)
