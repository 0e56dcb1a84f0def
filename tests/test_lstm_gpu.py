"""Persistent HIP LSTM against torch.nn.LSTM (CPU, fp32) on bf16-quantised operands, under bound (b) of
tests/test_lstm_reference_gpu.py: the kernel is at most twice as far from nn.LSTM as the fp64 emulation of its own rounding
points (oracle/lstm_ref.py) is, in relative L2 and in max-abs distance, for the output and every gradient."""
import pytest
import torch

from oracle import lstm_ref as R

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -20


@pytest.mark.parametrize("U,B,H", [(7, 5, 64), (23, 32, 128), (106, 32, 640), (9, 40, 64)])
def test_lstm_forward_backward_match_nn_lstm(U, B, H):
    from indic_cl_asr_amd.ops.lstm import lstm_forward
    torch.manual_seed(U + B)
    ref = torch.nn.LSTM(H, H, 1)
    with torch.no_grad():
        for p in ref.parameters():
            p.copy_(p.bfloat16().float() if p.dim() == 2 else p)   # weights exactly representable in bf16
    x = (torch.randn(U, B, H) * 0.7).bfloat16().float()
    xr = x.clone().requires_grad_(True)
    y_ref, _ = ref(xr)
    gy = torch.randn(U, B, H)
    y_ref.backward(gy)
    m = torch.nn.LSTM(H, H, 1).cuda()
    m.load_state_dict(ref.state_dict())
    xc = x.cuda().requires_grad_(True)
    y = lstm_forward(xc, m)
    y.backward(gy.cuda())
    torch.cuda.synchronize()
    F = R.run_lstm(x, ref.weight_ih_l0.detach(), ref.weight_hh_l0.detach(), ref.bias_ih_l0.detach(), ref.bias_hh_l0.detach(),
                   dy=gy, dtype=torch.float64, rounding="kernel")
    E = {"y": y_ref.detach(), "dx": xr.grad}
    E.update({n: p.grad for n, p in ref.named_parameters()})
    K = {"y": y.detach().cpu(), "dx": xc.grad.cpu()}
    K.update({n: p.grad.cpu() for n, p in m.named_parameters()})
    F64 = {"y": F["Hout"], "dx": F["dx"], "weight_ih_l0": F["dW_ih"], "weight_hh_l0": F["dW_hh"], "bias_ih_l0": F["db"],
           "bias_hh_l0": F["db"]}
    fails = []
    for n in E:
        e, k, f = E[n].double(), K[n].double(), F64[n]
        for metric, dk, df in (("L2", float((k - e).norm() / e.norm()), float((f - e).norm() / e.norm())),
                               ("max", float((k - e).abs().max() / e.abs().max()), float((f - e).abs().max() / e.abs().max()))):
            print(f"({U},{B},{H}) {n} {metric}: d(K, E) {dk:.3e}  d(F64, E) {df:.3e}  ratio {dk / max(df, FLOOR):.3f}")
            if not dk <= 2 * df + FLOOR:
                fails.append((n, metric, dk, df))
    assert not fails, fails
