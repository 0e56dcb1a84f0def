"""Functional fp64 / fp32 reference of the prediction-network LSTM (forward + hand-written backward) with selectable rounding.

TEST INFRASTRUCTURE (see oracle/__init__.py): only tests/ import this file.

`run_lstm(...)` computes what ops/lstm.py + csrc/lstm.hip compute -- torch.nn.LSTM(num_layers=1), zero initial state, gate
order i, f, g, o -- as plain tensor arithmetic, so that the same formulae can run

  rounding=None      plain math: the exact reference E (run it in fp64).  tests/test_lstm_reference.py pins it to
                     torch.nn.LSTM(...).double(): output and every autograd gradient.
  rounding="kernel"  rounds to bf16 exactly where the persistent kernels and their wrapper store or consume bf16.  Run in
                     fp64 (F64) and in fp32 (F32): the two differ only in fp32 rounding / summation order, so d(F32, F64) is
                     the noise scale the kernels' own fp32 arithmetic is allowed.

Rounding points of rounding="kernel" (everything else -- Gx, the gates, c_t, Hout, the dc carry, dG -- stays fp32 there):

  forward
    x, W_ih, W_hh -> bf16 ............................. ops/lstm.py forward: xb, fast.bf16_shadow(w_ih), (w_hh)
    Gx = x_b W_ih_b^T + (b_ih + b_hh) ................. one GEMM, the bias sum added in its fp32 epilogue
    h_t handed to step t+1 as bf16 (nearest-even) ..... lstm.hip ls_store_pair (Hout keeps the fp32 value)
  backward
    recurrent dh_t = bf16(dG_{t+1}) W_hh_b ............ lstm.hip lstm_bwd_kernel: the dgx exchange buffer
    dG rounded ONCE to bf16 for the dense contractions  ops/lstm.py backward: dGb
      dx    = dG_b W_ih_b, stored as bf16 .............. fast.gemm(dGb, wihT)[1] (the GEMM's bf16 output, cast to x.dtype)
      dW_ih = dG_b^T x_b
      db    = column sums of dG_b, returned for b_ih and for b_hh
      dW_hh = dG_b[1:]^T bf16(Hout[:-1]); zero when U = 1

The two single-step functions are the whole recurrence (run_lstm only chains them), so a test can feed a kernel's own
previous-step outputs into one step and compare that step alone: nothing then crosses a bf16 boundary between the kernel
and the reference, and a difference stays at fp32 size.
"""
import torch


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _rnd(t, rounding):
    return _bf16(t) if rounding == "kernel" else t


def fwd_step(h_prev, c_prev, gx_t, w_hh):
    """One forward step.  h_prev [B, H] = what step t-1 handed over (already bf16-valued under kernel rounding, zeros at
    t = 0), c_prev [B, H], gx_t [B, 4H] = the input projection with both biases, w_hh [4H, H] (already bf16-valued).
    Returns (gates_t [B, 4H] = activated i | f | g | o, c_t, h_t), nothing rounded."""
    H = h_prev.shape[1]
    pre = h_prev @ w_hh.t() + gx_t
    gi, gf, go = torch.sigmoid(pre[:, :H]), torch.sigmoid(pre[:, H:2 * H]), torch.sigmoid(pre[:, 3 * H:])
    gg = torch.tanh(pre[:, 2 * H:3 * H])
    c = gf * c_prev + gi * gg
    h = go * torch.tanh(c)
    return torch.cat([gi, gf, gg, go], 1), c, h


def bwd_step(dh_out_t, dg_next, gates_t, c_t, c_prev, dc_in, w_hh):
    """One backward step.  dh_out_t [B, H] = the incoming gradient of Hout[t], dg_next [B, 4H] = dG[t+1] as the recurrence
    reads it (bf16-valued under kernel rounding; None at t = U-1), gates_t / c_t as saved by the forward, c_prev = Cs[t-1]
    (zeros at t = 0), dc_in = the carry from step t+1 (zeros at t = U-1).  Returns (dG[t] [B, 4H], carry for step t-1)."""
    H = c_t.shape[1]
    dh = dh_out_t if dg_next is None else dh_out_t + dg_next @ w_hh
    gi, gf, gg, go = gates_t[:, :H], gates_t[:, H:2 * H], gates_t[:, 2 * H:3 * H], gates_t[:, 3 * H:]
    tc = torch.tanh(c_t)
    dct = dh * go * (1 - tc * tc) + dc_in
    di = dct * gg * gi * (1 - gi)
    df = dct * c_prev * gf * (1 - gf)
    dg = dct * gi * (1 - gg * gg)
    do = dh * tc * go * (1 - go)
    return torch.cat([di, df, dg, do], 1), dct * gf


def input_projection(x, w_ih, b_ih, b_hh, dtype, rounding):
    """Gx [U, B, 4H] and the operand images (x, W_ih) it was made from, in `dtype`."""
    U, B, H = x.shape
    xb, wih = _rnd(x.to(dtype), rounding), _rnd(w_ih.to(dtype), rounding)
    gx = (xb.reshape(U * B, H) @ wih.t() + (b_ih.to(dtype) + b_hh.to(dtype))).reshape(U, B, -1)
    return gx, xb, wih


def run_lstm(x, w_ih, w_hh, b_ih, b_hh, dy=None, dtype=torch.float64, rounding=None):
    """x [U, B, H], the four nn.LSTM parameters, dy [U, B, H] (None: forward only) -> dict of Hout, gates, Cs and, with dy,
    dG, dx, dW_ih, dW_hh, db (the gradient of b_ih and of b_hh alike), all in `dtype`."""
    assert rounding in (None, "kernel")
    U, B, H = x.shape
    gx, xb, wih = input_projection(x, w_ih, b_ih, b_hh, dtype, rounding)
    whh = _rnd(w_hh.to(dtype), rounding)
    h, c = torch.zeros(B, H, dtype=dtype), torch.zeros(B, H, dtype=dtype)
    Hout, gates, Cs = [], [], []
    for t in range(U):
        g, c, h_full = fwd_step(h, c, gx[t], whh)
        Hout.append(h_full); gates.append(g); Cs.append(c)
        h = _rnd(h_full, rounding)
    res = {"Hout": torch.stack(Hout), "gates": torch.stack(gates), "Cs": torch.stack(Cs), "Gx": gx}
    if dy is None:
        return res
    dy = dy.to(dtype)
    dG = [None] * U
    dc, nxt, zero = torch.zeros(B, H, dtype=dtype), None, torch.zeros(B, H, dtype=dtype)
    for t in range(U - 1, -1, -1):
        dG[t], dc = bwd_step(dy[t], nxt, res["gates"][t], res["Cs"][t], res["Cs"][t - 1] if t > 0 else zero, dc, whh)
        nxt = _rnd(dG[t], rounding)
    dG = torch.stack(dG)
    dGb = _rnd(dG, rounding).reshape(U * B, 4 * H)
    res["dG"] = dG
    res["dx"] = _rnd(dGb @ wih, rounding).reshape(U, B, H)
    res["dW_ih"] = dGb.t() @ xb.reshape(U * B, H)
    res["db"] = dGb.sum(0)
    if U > 1:
        res["dW_hh"] = dGb[B:].t() @ _rnd(res["Hout"][:-1], rounding).reshape((U - 1) * B, H)
    else:
        res["dW_hh"] = torch.zeros(4 * H, H, dtype=dtype)
    return res


def make_case(U, B, H, scale, seed=None):
    """The input recipe of tests/test_lstm_reference*.py: nn.LSTM's default init with the prediction network's forget-gate
    bias (decoder.py LSTMDropout: b_ih[H:2H] = 1, b_hh[H:2H] = 0), every parameter times `scale` (1: fresh, 3: the
    trained-like saturating regime), NOT pre-rounded to bf16; x ~ 0.7 N(0,1), dy ~ N(0,1).  fp32 CPU tensors."""
    seed = 1000 * U + 10 * B + H if seed is None else seed   # one recipe per shape, shared by the CPU and the GPU tests
    torch.manual_seed(seed)
    m = torch.nn.LSTM(H, H, 1)
    with torch.no_grad():
        m.bias_ih_l0[H:2 * H].fill_(1.0)
        m.bias_hh_l0[H:2 * H] *= 0.0
        for p in m.parameters():
            p.mul_(scale)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(U, B, H, generator=g) * 0.7
    dy = torch.randn(U, B, H, generator=g)
    return m, x, dy
