"""Functional references of everything in front of the first Conformer block: log-mel features, the dither noise, per-feature
normalisation + SpecAugment fill, and the striding ConvSubsampling with selectable rounding.

TEST INFRASTRUCTURE (see oracle/__init__.py): only tests/ import this file.  Plain torch functions that run in the dtype of
their inputs, so the same arithmetic gives the exact reference E (fp64) and the reference's own fp32 arithmetic F32; the
subsampling adds `rounding="kernel"`, which rounds to bf16 where the HIP path (csrc/gemm_bf16.hip conv1_relu_cl_kernel,
ia_subsample_conv2, the permuted Linear of ops/fast.conv_subsampling) stores or consumes bf16:

  conv1   fp32 weights, bias and input, taps accumulated in the kernel's order (bias, then dt-major taps); bf16 after the ReLU
  conv2   bf16 weight image, fp32 bias, the implicit GEMM's 64-deep k-steps accumulated in order; bf16 after bias + ReLU
  Linear  bf16 weight image, fp32 bias; fp32 output times alpha times mask (the GEMM epilogue's alpha * dropout(.))

tests/test_input_reference.py pins these functions (to ConvSubsampling(...).double() and the reference file's recorded outputs,
to the normalize_batch loop, to torch.stft at even and odd window lengths, and the noise to N(0,1) statistics).
"""

import numpy as np
import torch
import torch.nn.functional as F


def _bf16(t):
    return t.to(torch.bfloat16).to(t.dtype)


# ---------------------------------------------------------------------------------------------------- log-mel
def log_mel(x, window, fb, n_fft, hop, preemph, guard, noise=None):
    """FilterbankFeatures.forward (features.py:408-444) on x [B, L]: dither (`noise` [B, L], already scaled) added first, then
    pre-emphasis (first sample kept), torch.stft(center=True, reflect) with the window padded to n_fft the way torch.stft does
    it, power, fb @ power, log(. + guard).  -> log-mel [B, n_mels, Tm]."""
    dt = x.dtype
    if noise is not None:
        x = x + noise.to(dt)
    if preemph:
        x = torch.cat([x[:, :1], x[:, 1:] - preemph * x[:, :-1]], dim=1)
    spec = torch.stft(x, n_fft=n_fft, hop_length=hop, win_length=window.numel(), center=True, window=window.to(dt),
                      return_complex=True, pad_mode="reflect")
    power = spec.real ** 2 + spec.imag ** 2
    mel = torch.matmul(fb.to(dt)[:, :n_fft // 2 + 1], power)
    return torch.log(mel + guard)


# ---------------------------------------------------------------------------------------------------- dither noise
def _hash32(x):
    x = x ^ (x >> np.uint32(16)); x = x * np.uint32(0x85EBCA6B)
    x = x ^ (x >> np.uint32(13)); x = x * np.uint32(0xC2B2AE35)
    return x ^ (x >> np.uint32(16))


def randn_uniforms(seed, B, L):
    """The two uniforms behind sample (b, n) of fe_randn / ff_randn (csrc/frontend.hip, csrc/frontend_fft.hip), bit for bit:
    h1 = hash(b * 0x9E3779B1 ^ n * 0x85EBCA77 ^ seed), h2 = hash(h1 ^ 0x68E31DA4); u1 = ((h1 >> 8) + 1) * (1.0f / 16777217.0f) in
    (0, 1], u2 = (h2 >> 8) * 2^-24 in [0, 1).  (1.0f / 16777217.0f: the divisor rounds to 2^24 in fp32, so both scales are
    2^-24 and every product is exact.)  -> two float32 arrays [B, L]."""
    with np.errstate(over="ignore"):
        b = np.arange(B, dtype=np.uint32)[:, None] * np.uint32(0x9E3779B1)
        n = np.arange(L, dtype=np.uint32)[None, :] * np.uint32(0x85EBCA77)
        h1 = _hash32(b ^ n ^ np.uint32(seed & 0xFFFFFFFF))
        h2 = _hash32(h1 ^ np.uint32(0x68E31DA4))
    scale1 = np.float32(1.0) / np.float32(16777217.0)
    u1 = ((h1 >> np.uint32(8)).astype(np.float32) + np.float32(1.0)) * scale1
    u2 = (h2 >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return u1, u2


def randn_replica(seed, B, L):
    """Numpy restatement of the kernels' counter-based normal: the uniforms as above, Box-Muller sqrt(-2 ln u1) cos(2 pi u2) in
    fp64 (2 pi is the kernels' fp32 constant).  -> float64 array [B, L]."""
    u1, u2 = randn_uniforms(seed, B, L)
    two_pi = np.float64(np.float32(6.28318530717958647))
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(two_pi * u2.astype(np.float64))


# ---------------------------------------------------------------------------------------------------- normalisation
def normalize(x, seq_len, eps, spans=None, mask_value=0.0):
    """normalize_batch 'per_feature' (features.py:59-76) + the length mask (:458-462) + the SpecAugment fill
    (spec_aug_numba.py:26-95) on x [B, F, T]: mean and UNBIASED std over the frames below seq_len[b] (NaN for one frame, as
    torch.std), y = (x - mean) / (std + eps), zero beyond seq_len; spans = (freq_starts, freq_widths, time_starts,
    time_widths), each [B, n]: frequency spans fill every frame, time spans only frames below seq_len[b]."""
    B, Fd, T = x.shape
    lens = torch.as_tensor(seq_len).long()
    valid = (torch.arange(T)[None, :] < lens[:, None]).unsqueeze(1)              # [B, 1, T]
    n = lens.to(x.dtype).view(B, 1, 1)
    mean = torch.where(valid, x, torch.zeros((), dtype=x.dtype)).sum(2, keepdim=True) / n
    dev = torch.where(valid, x - mean, torch.zeros((), dtype=x.dtype))
    std = ((dev * dev).sum(2, keepdim=True) / (n - 1.0)).sqrt()
    y = torch.where(valid, (x - mean) / (std + eps), torch.zeros((), dtype=x.dtype))
    if spans is not None:
        fs, fw, ts, tw = (torch.as_tensor(s).long() for s in spans)
        f = torch.arange(Fd).view(1, 1, Fd)
        fmask = ((f >= fs.unsqueeze(-1)) & (f < (fs + fw).unsqueeze(-1))).any(1)  # [B, F]
        t = torch.arange(T).view(1, 1, T)
        tmask = ((t >= ts.unsqueeze(-1)) & (t < (ts + tw).unsqueeze(-1))).any(1) & valid.squeeze(1)
        y = torch.where(fmask.unsqueeze(2) | tmask.unsqueeze(1), torch.full((), mask_value, dtype=x.dtype), y)
    return y


# ---------------------------------------------------------------------------------------------------- subsampling
def params_of(module, dtype):
    """state_dict of a ConvSubsampling (conv.0 / conv.2 / out) as `dtype` CPU tensors."""
    return {k: v.detach().cpu().to(dtype) for k, v in module.state_dict().items()}


def conv1(x, w, b, rounding=None):
    """Conv2d(1, C, 3, stride 2, pad 1) + ReLU on x [B, T, F] -> channels-last [B, T1, F1, C] (the layout the HIP path keeps).
    Nine taps accumulated onto the bias, time-major, as conv1_relu_cl_kernel does."""
    B, T, Fd = x.shape
    T1, F1 = (T - 1) // 2 + 1, (Fd - 1) // 2 + 1
    xp = F.pad(x, (1, 2, 1, 2))                                                   # one pad row / column in front, spare ones behind
    acc = b.view(1, 1, 1, -1).expand(B, T1, F1, -1)
    for dt in range(3):
        for df in range(3):
            px = xp[:, dt:dt + 2 * T1:2, df:df + 2 * F1:2]                        # x[2 t1 + dt - 1, 2 f1 + df - 1]
            acc = acc + w[:, 0, dt, df].view(1, 1, 1, -1) * px.unsqueeze(-1)
    o = torch.relu(acc)
    return _bf16(o) if rounding else o


def conv2(o1, w, b, rounding=None):
    """Conv2d(C, N, 3, stride 2, pad 1) + ReLU on channels-last o1 [B, T1, F1, C] -> channels-last [B, T2, F2, N].
    Written as the implicit GEMM the kernel runs: patches [M, 9 C] with k = tap * C + channel against the weight image [N, 9 C],
    accumulated in the kernel's 64-deep k-steps one after the other, bias added last.  In fp64 the order is immaterial; in
    fp32 it makes d(F32, F64) the noise of a sequential accumulation like the kernel's, not of a library's blocked one."""
    if rounding:
        w = _bf16(w)
    B, T1, F1, Cc = o1.shape
    N = w.shape[0]
    T2, F2 = (T1 - 1) // 2 + 1, (F1 - 1) // 2 + 1
    xp = F.pad(o1, (0, 0, 1, 2, 1, 2))                                            # one pad row / column in front, spare ones behind
    taps = [xp[:, dt:dt + 2 * T2:2, df:df + 2 * F2:2, :] for dt in range(3) for df in range(3)]
    P = torch.cat(taps, dim=-1).reshape(B * T2 * F2, 9 * Cc)
    W = w.permute(0, 2, 3, 1).reshape(N, 9 * Cc)
    acc = torch.zeros(B * T2 * F2, N, dtype=o1.dtype)
    for k0 in range(0, 9 * Cc, 64):
        acc = acc + P[:, k0:k0 + 64] @ W[:, k0:k0 + 64].T
    o = torch.relu(acc + b).view(B, T2, F2, N)
    return _bf16(o) if rounding else o


def linear(o2, w, b, rounding=None, alpha=1.0, mask=None):
    """The module's Linear over (channel, feature) of channels-last o2 [B, T2, F2, N] (input index c * F2 + f, subsampling.py
    :430-432) -> [B, T2, d], times alpha times mask (mask [B, T2, d]: 0 or the keep scale)."""
    if rounding:
        w = _bf16(w)
    B, T2, F2, N = o2.shape
    y = F.linear(o2.permute(0, 1, 3, 2).reshape(B, T2, N * F2), w, b)
    scale = torch.full((), float(alpha), dtype=y.dtype)
    if mask is not None:
        scale = scale * mask.to(y.dtype)
    return y * scale


def subsampling(x, params, rounding, alpha=1.0, mask=None, splice=None):
    """ConvSubsampling 'striding' x4 (subsampling.py:217-253,385-437) on x [B, T, feat_in] -> (o1, o2, y): the two convolution
    outputs channels-last and the Linear's output [B, T2, d] * alpha * mask.  rounding=None: plain math; "kernel": the HIP
    path's rounding points (see the module docstring).  splice={"o1": ..., "o2": ...} feeds the NEXT stage the given tensor
    instead of the one computed here, so that each stage is judged on the kernel's own input."""
    assert rounding in (None, "kernel")
    splice = splice or {}
    dt = x.dtype
    o1 = conv1(x, params["conv.0.weight"], params["conv.0.bias"], rounding)
    i1 = splice["o1"].to(dt) if "o1" in splice else o1
    o2 = conv2(i1, params["conv.2.weight"], params["conv.2.bias"], rounding)
    i2 = splice["o2"].to(dt) if "o2" in splice else o2
    y = linear(i2, params["out.weight"], params["out.bias"], rounding, alpha, mask)
    return o1, o2, y
