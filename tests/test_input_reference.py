"""oracle/input_ref.py pinned on the CPU: the references the input-path kernels are held to (tests/test_input_reference_gpu.py)
are themselves checked against the module, the reference file's recorded outputs, the normalize_batch loop, torch.stft at
even and odd window lengths, and -- for the dither noise -- against the statistics of independent N(0,1) draws."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import input_ref as R


# ---------------------------------------------------------------------------------------------------- subsampling
@pytest.mark.parametrize("feat_in,C,d,B,Tm", [(80, 16, 24, 3, 61), (81, 8, 16, 2, 6), (7, 8, 8, 1, 1), (1, 8, 8, 2, 2)])
def test_subsampling_plain_math_equals_the_module_in_fp64(feat_in, C, d, B, Tm):
    from indic_cl_asr_amd.encoder import ConvSubsampling
    torch.manual_seed(feat_in + Tm)
    m = ConvSubsampling(feat_in, d, C).double()
    x = torch.randn(B, Tm, feat_in, dtype=torch.float64)
    with torch.no_grad():
        want, _ = m(x, torch.full((B,), Tm))
        mid = m.conv[:2](x.unsqueeze(1))                                         # [B, C, T1, F1] after the first ReLU
        o1, o2, y = R.subsampling(x, R.params_of(m, torch.float64), None)
        assert torch.allclose(o1, mid.permute(0, 2, 3, 1), rtol=0, atol=1e-13)
        assert torch.allclose(o2, m.conv(x.unsqueeze(1)).permute(0, 2, 3, 1), rtol=0, atol=1e-13)
        assert torch.allclose(y, want, rtol=0, atol=1e-12 * float(want.abs().max()))
        # alpha and mask multiply the Linear's output; a spliced stage input replaces the computed one for the NEXT stage only
        mask = (torch.rand(y.shape, dtype=torch.float64) > 0.3).double() * 1.25
        _, _, ys = R.subsampling(x, R.params_of(m, torch.float64), None, alpha=3.0, mask=mask)
        assert torch.allclose(ys, want * 3.0 * mask, rtol=0, atol=1e-11 * float(want.abs().max()))
        p1, p2, yz = R.subsampling(x, R.params_of(m, torch.float64), None, splice={"o1": torch.zeros_like(o1)})
        assert torch.equal(p1, o1) and not torch.equal(p2, o2)
        b2 = m.conv[2].bias.view(1, 1, 1, -1).clamp(min=0).expand_as(p2)         # conv2 of an all-zero image: relu(bias)
        assert torch.allclose(p2, b2, rtol=0, atol=1e-15)
        q1, q2, yq = R.subsampling(x, R.params_of(m, torch.float64), None, splice={"o2": torch.zeros_like(o2)})
        assert torch.equal(q2, o2) and torch.allclose(yq, m.out.bias.expand_as(yq), rtol=0, atol=1e-15)


@pytest.mark.parametrize("tag", ["a", "b"])
def test_subsampling_reproduces_the_reference_files_outputs(tag):
    """tests/golden/subsampling_cases.npz: what the reference's own subsampling.py returned in fp32.  E in fp64 on the same
    fp32 weights differs by fp32 summation noise only: 1e-5 of the largest output (K = 9 C and C F2 <= 320 products a sum)."""
    from conftest import GOLDEN
    Z = np.load(os.path.join(GOLDEN, "subsampling_cases.npz"))
    pre = f"sub/{tag}/param/"
    P = {k[len(pre):]: torch.tensor(Z[k]).double() for k in Z.files if k.startswith(pre)}
    x, want = torch.tensor(Z[f"sub/{tag}/x"]).double(), torch.tensor(Z[f"sub/{tag}/y"]).double()
    _, _, y = R.subsampling(x, P, None)
    assert y.shape == want.shape
    assert float((y - want).abs().max()) <= 1e-5 * float(want.abs().max())
    # the kernel's rounding points move the result by bf16-sized steps, not more: two bf16 stages and a bf16 weight image
    _, _, yk = R.subsampling(x, P, "kernel")
    rel = float((yk - y).norm() / y.norm())
    assert 1e-4 < rel < 2e-2, rel
    _, _, yk32 = R.subsampling(x.float(), {k: v.float() for k, v in P.items()}, "kernel")
    assert float((yk32.double() - yk).norm() / y.norm()) < rel / 4                # F32 and F64 differ by far less than the rounding


# ---------------------------------------------------------------------------------------------------- normalisation
def _normalize_batch_loop(x, seq_len, eps=1e-5):
    """The loop of normalize_batch 'per_feature' (features.py:59-76) restated, then the length mask (:458-462)."""
    mean = torch.zeros(x.shape[:2], dtype=x.dtype)
    std = torch.zeros(x.shape[:2], dtype=x.dtype)
    for i in range(x.shape[0]):
        mean[i, :] = x[i, :, :seq_len[i]].mean(dim=1)
        std[i, :] = x[i, :, :seq_len[i]].std(dim=1)
    std = std + eps
    y = (x - mean.unsqueeze(2)) / std.unsqueeze(2)
    mask = torch.arange(x.shape[2])[None, :] >= torch.as_tensor(seq_len)[:, None]
    return y.masked_fill(mask.unsqueeze(1), 0.0)


@pytest.mark.parametrize("F_,T,lens", [(80, 76, (76, 40, 2)), (5, 257, (257, 256, 3)), (1, 3, (3, 2))])
def test_normalize_equals_the_reference_loop(F_, T, lens):
    g = torch.Generator().manual_seed(T)
    x = torch.randn(len(lens), F_, T, generator=g, dtype=torch.float64) * 2 - 10
    x[0, 0, :] = -10.25                                                           # std 0: eps decides, the result is 0
    want = _normalize_batch_loop(x, lens)
    got = R.normalize(x, torch.tensor(lens), 1e-5)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-12)
    assert torch.equal(got[0, 0], torch.zeros(T, dtype=torch.float64))
    got32 = R.normalize(x.float(), torch.tensor(lens), 1e-5)
    assert got32.dtype == torch.float32 and torch.allclose(got32.double(), want, rtol=1e-4, atol=1e-4)


def test_normalize_of_one_frame_is_nan_like_torch_std():
    x = torch.randn(2, 4, 5, dtype=torch.float64)
    want = _normalize_batch_loop(x, (5, 1))
    got = R.normalize(x, torch.tensor((5, 1)), 1e-5)
    assert torch.equal(torch.isnan(got), torch.isnan(want))
    assert torch.isnan(got[1, :, 0]).all() and torch.equal(got[1, :, 1:], torch.zeros(4, 4, dtype=torch.float64))
    assert not torch.isnan(got[0]).any()


@pytest.mark.parametrize("freq_masks,time_masks,mask_value", [(2, 10, 0.0), (2, 10, -1.0), (0, 10, 0.0), (2, 0, 0.0)])
def test_normalize_fill_obeys_the_mask_rule(freq_masks, time_masks, mask_value):
    from test_reference_properties_gpu import _check_masks, _spec_data
    x, x_len, fs, fw, ts, tw = _spec_data(freq_masks=freq_masks, time_masks=time_masks)
    base = R.normalize(x.double(), x_len, 1e-5)
    y = R.normalize(x.double(), x_len, 1e-5, spans=(fs, fw, ts, tw), mask_value=mask_value)
    _check_masks(y, base, x_len, fs, fw, ts, tw, mask_value)


# ---------------------------------------------------------------------------------------------------- log-mel
def _signal(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, L, generator=g, dtype=torch.float64) * 0.1
    x[0, : L // 3] *= 1e-3
    return x


def _framed_power(y, window, n_fft, hop, lead):
    """The kernels' framing rule restated in fp64 (csrc/frontend.hip feat_frames_kernel, csrc/frontend_fft.hip): tap n of frame
    t reads sample reflect(t * hop + n - lead), times window[n], then the n_fft-point DFT with the window (n_fft - win) // 2
    samples into the frame.  -> power [B, n_fft / 2 + 1, Tm]."""
    B, L = y.shape
    win = window.numel()
    Tm = L // hop + 1
    p = torch.arange(Tm)[:, None] * hop + torch.arange(win)[None, :] - lead
    p = p.abs()
    p = torch.where(p >= L, 2 * L - 2 - p, p)
    assert int(p.min()) >= 0 and int(p.max()) < L
    frames = y[:, p] * window.double()                                           # [B, Tm, win]
    off = (n_fft - win) // 2
    k = torch.arange(n_fft // 2 + 1, dtype=torch.float64)[:, None]
    ang = 2.0 * math.pi * k * (torch.arange(win, dtype=torch.float64)[None, :] + off) / n_fft
    re, im = frames @ torch.cos(ang).T, frames @ torch.sin(ang).T
    return (re * re + im * im).transpose(1, 2)


def test_log_mel_at_win_400_equals_the_existing_fp64_restatement():
    from indic_cl_asr_amd.features import mel_filterbank_slaney
    from test_frontend_fft_gpu import _ref_logmel
    fb = torch.as_tensor(mel_filterbank_slaney()).float()
    window = torch.hann_window(400, periodic=False)
    x = _signal(2, 4001, 1)
    want = _ref_logmel(x, window, fb)
    got = R.log_mel(x, window, fb, 512, 160, 0.97, 2 ** -24)
    assert got.dtype == torch.float64 and torch.allclose(got, want, rtol=0, atol=1e-12)
    noise = torch.randn(x.shape, dtype=torch.float64) * 1e-3
    assert torch.allclose(R.log_mel(x, window, fb, 512, 160, 0.97, 2 ** -24, noise=noise), _ref_logmel(x + noise, window, fb),
                          rtol=0, atol=1e-12)                                    # the noise goes in before the pre-emphasis
    assert R.log_mel(x.float(), window, fb, 512, 160, 0.97, 2 ** -24).dtype == torch.float32


@pytest.mark.parametrize("win,n_fft,sr", [(400, 512, 16000), (320, 512, 16000), (512, 512, 16000), (399, 512, 16000),
                                          (321, 512, 16000), (551, 1024, 22050)])
def test_log_mel_framing_rule_for_even_and_odd_windows(win, n_fft, sr):
    """torch.stft pads the window to n_fft with (n_fft - win) // 2 zeros on the left: tap n of frame t is sample
    t * hop + n + (n_fft - win) // 2 - n_fft / 2.  The front ends frame with lead = n_fft / 2 - (n_fft - win) // 2 samples in
    front of the frame's centre; that rule equals torch.stft (through R.log_mel) at every window length, and the earlier rule
    (lead = win // 2) only at even ones: at odd lengths it reads every frame one sample late (5e-3 of the largest bin)."""
    from indic_cl_asr_amd.features import mel_filterbank_slaney
    fb = torch.as_tensor(mel_filterbank_slaney(sr, n_fft, 80)).double()
    window = torch.hann_window(win, periodic=False)
    hop, guard = 160, 2 ** -24
    x = _signal(2, 2 * n_fft + 77, win)
    y = torch.cat([x[:, :1], x[:, 1:] - 0.97 * x[:, :-1]], dim=1)
    want = R.log_mel(x, window, fb, n_fft, hop, 0.97, guard)
    lead = n_fft // 2 - (n_fft - win) // 2
    got = torch.log(fb @ _framed_power(y, window, n_fft, hop, lead) + guard)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) < 1e-9
    old = torch.log(fb @ _framed_power(y, window, n_fft, hop, win // 2) + guard)
    if win % 2 == 0:
        assert lead == win // 2 and torch.equal(old, got)
    else:
        assert lead == win // 2 + 1
        assert float((old - want).abs().max()) > 1e-3


# ---------------------------------------------------------------------------------------------------- dither noise
def _corr(a, b):
    a, b = a.ravel() - a.mean(), b.ravel() - b.mean()
    return float((a * b).mean() / math.sqrt((a * a).mean() * (b * b).mean()))


def test_randn_replica_uniforms_follow_the_kernels_constants():
    u1, u2 = R.randn_uniforms(77, 3, 1000)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    assert np.float32(1.0) / np.float32(16777217.0) == np.float32(2.0 ** -24)    # the divisor is not an fp32 number
    assert u1.min() > 0 and u1.max() <= 1 and u2.min() >= 0 and u2.max() < 1
    # sample (b, n) = (2, 5) of seed 77 by hand, in Python integers
    def h(x):
        x ^= x >> 16; x = (x * 0x85EBCA6B) & 0xFFFFFFFF; x ^= x >> 13; x = (x * 0xC2B2AE35) & 0xFFFFFFFF
        return x ^ (x >> 16)
    h1 = h(((2 * 0x9E3779B1) & 0xFFFFFFFF) ^ ((5 * 0x85EBCA77) & 0xFFFFFFFF) ^ 77)
    h2 = h(h1 ^ 0x68E31DA4)
    assert float(u1[2, 5]) == ((h1 >> 8) + 1) / 2 ** 24 and float(u2[2, 5]) == (h2 >> 8) / 2 ** 24
    z = R.randn_replica(77, 3, 1000)
    assert z[2, 5] == math.sqrt(-2.0 * math.log(float(u1[2, 5]))) * math.cos(float(np.float32(6.28318530717958647)) * float(u2[2, 5]))


def test_randn_replica_is_standard_normal_and_uncorrelated():
    """2^21 draws per seed.  Under independence: mean ~ N(0, 1/N), variance ~ N(1, 2/N), every correlation ~ N(0, 1/n) over the
    n pairs it averages; each statistic within 5 standard errors.  Lag 4 along n: the pre-emphasis kernel draws four samples
    per thread; neighbouring b and neighbouring seeds: the other two inputs of the hash."""
    B, L, seed = 4, 1 << 19, 12345
    z = R.randn_replica(seed, B, L)
    N = z.size
    assert N >= 1 << 21 and np.isfinite(z).all()
    assert abs(z.mean()) < 5 / math.sqrt(N), z.mean()
    assert abs(z.var() - 1.0) < 5 * math.sqrt(2.0 / N), z.var()
    assert abs((z ** 4).mean() - 3.0) < 5 * math.sqrt(96.0 / N)                   # kurtosis of a normal: Var(z^4) = 96
    for lag in (1, 4):
        c = _corr(z[:, :-lag], z[:, lag:])
        assert abs(c) < 5 / math.sqrt(B * (L - lag)), (lag, c)
    c = _corr(z[:-1], z[1:])
    assert abs(c) < 5 / math.sqrt((B - 1) * L), ("b", c)
    z1 = R.randn_replica(seed + 1, B, L)
    c = _corr(z, z1)
    assert abs(c) < 5 / math.sqrt(N), ("seed", c)
    assert abs(z1.mean()) < 5 / math.sqrt(N) and abs(z1.var() - 1.0) < 5 * math.sqrt(2.0 / N)
