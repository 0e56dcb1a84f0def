"""Numpy restatement of the waveform augmentation's definition (DESIGN.md "Waveform augmentation"; the kernel is
csrc/wave_augment.hip), vectorised per output sample, twice:

  E     everything in fp64
  F32   the table, e, the products and a sum in increasing k in float32 (and the factor s, the gain and the scaled noise)

Gain, shift and noise are applied step by step in list order -- the steps AudioAugmentor.draw returns: ("speed", new_sr),
("gain", dB), ("shift", samples), ("white_noise", dB, seed) -- with the noise from oracle.input_ref.randn_replica.
"""
import numpy as np

from indic_cl_asr_amd import augment as A
from oracle.input_ref import randn_replica

P = A.P


def resample(x, sr, new_sr, resample_type="kaiser_fast", mode="E", m_range=None):
    """y[m] = s sum_k x[k] (h[i] + e (h[i+1] - h[i])) over 0 <= k < n with i < Z P; D = m sr - k new_sr in int64,
    q = max(sr, new_sr), i = (|D| P) // q, e = ((|D| P) mod q) / q, s = min(1, new_sr / sr).  m_range = (lo, hi): only those
    output samples."""
    f32 = mode == "F32"
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    n_out = A.resampled_length(n, sr, new_sr)
    Z = A.RESAMPLE_TABLES[resample_type][0]
    ZP = Z * P
    h = A.resample_table(resample_type)
    q = max(sr, new_sr)
    W = -((-Z * q) // new_sr) + 1
    lo, hi = (0, n_out) if m_range is None else m_range
    m = np.arange(lo, hi, dtype=np.int64)
    k = (m * sr // new_sr)[:, None] + np.arange(-W, W + 2, dtype=np.int64)[None, :]          # increasing k along axis 1
    a = np.abs(m[:, None] * sr - k * new_sr) * P
    i, num = a // q, a % q
    valid = (k >= 0) & (k < n) & (i < ZP)
    i = np.minimum(i, ZP - 1)
    xk = x[np.clip(k, 0, n - 1)]
    if not f32:
        w = h[i] + (num / q) * (h[i + 1] - h[i])
        return min(1.0, new_sr / sr) * np.where(valid, xk * w, 0.0).sum(axis=1)
    h32 = h.astype(np.float32)
    e = num.astype(np.float32) / np.float32(q)
    w = h32[i] + e * (h32[i + 1] - h32[i])
    prod = np.where(valid, xk.astype(np.float32) * w, np.float32(0.0)).astype(np.float32)
    acc = np.zeros(m.shape[0], dtype=np.float32)
    for t in range(prod.shape[1]):
        acc = acc + prod[:, t]
    return (np.float32(min(1.0, new_sr / sr)) * acc).astype(np.float32)


def shift(y, samples):
    """perturb.py:428-433: negative delays and zeroes the head, positive advances and zeroes the tail."""
    n = y.shape[0]
    j = np.arange(n) + samples
    ok = (j >= 0) & (j < n)
    return np.where(ok, y[np.clip(j, 0, n - 1)], 0).astype(y.dtype)


def apply_chain(x, steps, sr, row, resample_type="kaiser_fast", mode="E", m_range=None):
    """One utterance through its steps, one after the other.  `row`: its row in the batch (the noise generator's b).
    m_range only with a chain whose last length-changing step is its first step."""
    f32 = mode == "F32"
    dt = np.float32 if f32 else np.float64
    y = np.asarray(x, dtype=np.float32).astype(dt)
    for step in steps:
        if step[0] == "speed":
            y = resample(y, sr, step[1], resample_type, mode, m_range).astype(dt)
        elif step[0] == "gain":
            y = y * dt(10.0 ** (step[1] / 20.0))
        elif step[0] == "shift":
            y = shift(y, step[1])
        elif step[0] == "white_noise":
            noise = randn_replica(step[2], row + 1, y.shape[0])[row] * 10.0 ** (step[1] / 20.0)
            y = y + noise.astype(dt)
        else:
            raise ValueError(step[0])
    return y.astype(np.float64)
