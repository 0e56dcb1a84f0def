"""Waveform augmentation on the device: NeMo's `train_ds.augmentor` with `speed`, `gain`, `shift` and `white_noise`
(A/parts/preprocessing/perturb.py: SpeedPerturbation :99-165, GainPerturbation :315-332, ShiftPerturbation :404-433,
WhiteNoisePerturbation :808-826, AudioAugmentor :1082-1108, process_augmentations :1111-1236).

What differs in HOW: the reference perturbs one utterance at a time on the host, in the dataset's `__getitem__`; here the
host only DRAWS -- per utterance, in list order, each perturbation with its own probability -- and folds the drawn chain
into one row of parameters (`fold_chain`); csrc/wave_augment.hip then applies every utterance's chain to the padded device
batch in one launch.  The new lengths follow from the length rule on the host, so nothing is read back.

Speed perturbation is Smith's band-limited interpolation with a Kaiser-windowed sinc table and linear interpolation
between table entries -- the algorithm family of the reference's `librosa.core.resample(res_type='kaiser_fast' |
'kaiser_best')`, not its bits (DESIGN.md has the definition).  Every draw comes from the augmentor's own generator, seeded
by (seed, rank); `state_dict()` carries its state.
"""
import random
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

P = 512                                      # table entries per zero crossing
#                       Z   rolloff             beta
RESAMPLE_TABLES = {"kaiser_fast": (16, 0.85, 8.555504641634386),
                   "kaiser_best": (64, 0.9475937167399596, 14.769656459379492)}
KINDS = ("speed", "gain", "shift", "white_noise")
UNSUPPORTED = ("time_stretch", "noise", "impulse", "rir_noise_aug", "transcode_aug", "silence")

# numpy image of ia_wave_params (include/indicasr.h)
PARAMS_DTYPE = np.dtype([("n_in", "<i4"), ("n_out", "<i4"), ("new_sr", "<i4"), ("shift_pre", "<i4"), ("shift_post", "<i4"),
                         ("noise_shift", "<i4"), ("noise_stage", "<i4"), ("noise_seed", "<u4"), ("gain", "<f4"),
                         ("noise_amp", "<f4"), ("pad", "<i4", (2,))])


# ---------------------------------------------------------------------------------------------------- the definition
def resample_table(resample_type: str) -> np.ndarray:
    """h[0 .. Z P] in fp64: rolloff sinc(rolloff j/P) I0(beta sqrt(1 - (j/(Z P))^2)) / I0(beta), h[Z P] = 0."""
    if resample_type in ("fft", "scipy"):
        raise NotImplementedError(f"resample_type={resample_type!r}: only the Kaiser-windowed sinc tables "
                                  f"{tuple(RESAMPLE_TABLES)} run on the device")
    if resample_type not in RESAMPLE_TABLES:
        raise ValueError("Supported `resample_type` values are ('kaiser_best', 'kaiser_fast', 'fft', 'scipy')")
    Z, rolloff, beta = RESAMPLE_TABLES[resample_type]
    t = np.arange(Z * P + 1, dtype=np.float64) / P
    h = rolloff * np.sinc(rolloff * t) * np.i0(beta * np.sqrt(np.maximum(1.0 - (t / Z) ** 2, 0.0))) / np.i0(beta)
    h[Z * P] = 0.0
    return h


def resampled_length(n: int, sr: int, new_sr: int) -> int:
    """ceil(n new_sr / sr): the reference resamples from sr to new_sr and keeps calling the rate sr."""
    return -((-int(n) * int(new_sr)) // int(sr))


def shift_samples(shift_ms: float, sr: int) -> int:
    """perturb.py:426 -- floor division, so a negative shift rounds away from zero."""
    return int(shift_ms * sr // 1000)


# ---------------------------------------------------------------------------------------------------- perturbations
class Perturbation:
    kind = None

    def __init__(self, rng=None):
        self.rng = rng                       # mixed into the augmentor's seed; the augmentor's generator draws


class SpeedPerturbation(Perturbation):
    kind = "speed"

    def __init__(self, sr, resample_type, min_speed_rate=0.9, max_speed_rate=1.1, num_rates=5, rng=None):
        super().__init__(rng)
        if min(min_speed_rate, max_speed_rate) < 0.0:
            raise ValueError("Minimum sampling rate modifier must be > 0.")
        if resample_type not in RESAMPLE_TABLES:
            resample_table(resample_type)    # NotImplementedError for fft / scipy, ValueError for anything else
        self._sr, self._res_type = int(sr), resample_type
        self._min_rate, self._max_rate, self._num_rates = min_speed_rate, max_speed_rate, num_rates
        if num_rates > 0:
            self._rates = np.linspace(min_speed_rate, max_speed_rate, num_rates, endpoint=True)

    def draw(self, rng):
        """new_sr, or None when the drawn rate is 1.0 (:159) or maps onto sr itself."""
        rate = float(rng.choice(list(self._rates))) if self._num_rates > 0 else rng.uniform(self._min_rate, self._max_rate)
        if rate == 1.0:
            return None
        new_sr = int(self._sr * rate)
        if new_sr <= 0:
            raise ValueError(f"speed rate {rate} gives new_sr = {new_sr}")
        return None if new_sr == self._sr else new_sr


class GainPerturbation(Perturbation):
    kind = "gain"

    def __init__(self, min_gain_dbfs=-10, max_gain_dbfs=10, rng=None):
        super().__init__(rng)
        self._min_gain_dbfs, self._max_gain_dbfs = min_gain_dbfs, max_gain_dbfs

    def draw(self, rng):
        return rng.uniform(self._min_gain_dbfs, self._max_gain_dbfs)


class ShiftPerturbation(Perturbation):
    kind = "shift"

    def __init__(self, min_shift_ms=-5.0, max_shift_ms=5.0, rng=None):
        super().__init__(rng)
        self._min_shift_ms, self._max_shift_ms = min_shift_ms, max_shift_ms

    def draw(self, rng):
        return rng.uniform(self._min_shift_ms, self._max_shift_ms)


class WhiteNoisePerturbation(Perturbation):
    kind = "white_noise"

    def __init__(self, min_level=-90, max_level=-46, rng=None):
        super().__init__(rng)
        self.min_level, self.max_level = int(min_level), int(max_level)

    def draw(self, rng):
        """(level in dB from [min_level, max_level), the noise's own seed)."""
        return rng.randrange(self.min_level, self.max_level), rng.getrandbits(32)


perturbation_types = {"speed": SpeedPerturbation, "gain": GainPerturbation, "shift": ShiftPerturbation,
                      "white_noise": WhiteNoisePerturbation}


# ---------------------------------------------------------------------------------------------------- folding a chain
def fold_chain(steps, n: int, sr: int) -> Tuple[dict, int]:
    """One utterance's drawn steps, in order -- ("speed", new_sr), ("gain", dB), ("shift", samples), ("white_noise", dB, seed)
    -- as the fields of ia_wave_params, and the new length.  Gain commutes with shift and resampling and so becomes one factor;
    a gain after the noise scales the noise too.  Noise drawn before the resampling is added while the input is staged
    (noise_stage 1) at amplitude amp / gain, since the gain is applied to the resampled sum; a shift that follows the noise
    inside the same stage moves the noise with the signal (noise_shift)."""
    n = int(n)
    f = dict(n_in=n, n_out=n, new_sr=0, shift_pre=0, shift_post=0, noise_shift=0, noise_stage=0, noise_seed=0, gain=1.0,
             noise_amp=0.0)
    gain, amp, noise_open = 1.0, 0.0, False
    for step in steps:
        kind = step[0]
        if kind == "speed":
            if f["new_sr"]:
                raise ValueError("speed appears twice in one chain")
            f["new_sr"] = int(step[1])
            f["n_out"] = resampled_length(n, sr, f["new_sr"])
            f["shift_pre"], f["shift_post"] = f["shift_post"], 0          # a shift drawn so far acts on the input
            if noise_open:
                f["noise_stage"], noise_open = 1, False
        elif kind == "gain":
            g = 10.0 ** (step[1] / 20.0)
            gain *= g
            amp *= g
        elif kind == "shift":
            f["shift_post"] = int(step[1])
            if noise_open:
                f["noise_shift"] = int(step[1])
        elif kind == "white_noise":
            amp, f["noise_seed"], noise_open = 10.0 ** (step[1] / 20.0), int(step[2]) & 0xFFFFFFFF, True
        else:
            raise ValueError(f"unknown step {kind!r}")
    f["gain"] = gain
    f["noise_amp"] = amp / gain if f["noise_stage"] == 1 else amp
    return f, f["n_out"]


def pack_params(folded: Sequence[dict]) -> np.ndarray:
    rows = np.zeros(len(folded), dtype=PARAMS_DTYPE)
    for i, f in enumerate(folded):
        for k, v in f.items():
            rows[k][i] = v
    return rows


_TABLES = {}


def _device_table(resample_type, device):
    key = (resample_type, torch.device(device))
    if key not in _TABLES:
        _TABLES[key] = torch.from_numpy(resample_table(resample_type).astype(np.float32)).to(device)
    return _TABLES[key]


def wave_augment(signal: torch.Tensor, rows: np.ndarray, sr: int, resample_type: str = "kaiser_fast",
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """ia_wave_augment on a device batch [B, L_in] f32 with one PARAMS_DTYPE row per utterance -> [B, max n_out].  The rows go
    through pinned memory and an asynchronous copy; the launch is enqueued on the current stream and nothing is waited for."""
    if not signal.is_cuda:
        raise RuntimeError("waveform augmentation runs on the device (csrc/wave_augment.hip) and has no host path")
    if signal.dtype != torch.float32 or signal.dim() != 2 or rows.dtype != PARAMS_DTYPE or len(rows) != signal.shape[0]:
        raise ValueError("signal must be [B, L] float32 with one parameter row per utterance")
    signal = signal.contiguous()
    B, L_in = signal.shape
    L_out = max(1, int(rows["n_out"].max()))
    if out is None:
        out = torch.empty(B, L_out, dtype=torch.float32, device=signal.device)
    elif out.shape != (B, L_out) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != signal.device:
        raise ValueError(f"out must be a contiguous float32 [{B}, {L_out}] on the signal's device")
    active = rows["new_sr"][rows["new_sr"] > 0]
    min_new_sr = int(active.min()) if active.size else 0
    if resample_type not in RESAMPLE_TABLES:
        resample_table(resample_type)        # raises
    Z = RESAMPLE_TABLES[resample_type][0]
    table = _device_table(resample_type, signal.device) if min_new_sr else None
    host = torch.from_numpy(np.ascontiguousarray(rows).view(np.uint8).copy()).pin_memory()
    dev = host.to(signal.device, non_blocking=True)
    _lib.check(_lib.lib().ia_wave_augment(_lib.ptr(signal), B, L_in, _lib.ptr(out), L_out, _lib.ptr(dev), _lib.ptr(table), Z,
                                          int(sr), min_new_sr, _lib.stream_ptr()), "ia_wave_augment")
    return out


# ---------------------------------------------------------------------------------------------------- the augmentor
class AudioAugmentor:
    """`AudioAugmentor(perturbations=[(prob, p), ...], seed=0, rank=0)`; `aug(batch, host_lengths)` -> (batch', host_lengths')
    on a device batch in the training tuple's layout (signal, signal_len, tokens, tokens_len)."""

    def __init__(self, perturbations=None, rng=None, seed=0, rank=0, sample_rate=16000):
        self._pipeline = [(float(prob), p) for prob, p in (perturbations or [])]
        kinds = [p.kind for _, p in self._pipeline]
        for prob, p in self._pipeline:
            if p.kind not in KINDS:
                raise ValueError(f"{type(p).__name__} is not a waveform perturbation of this package")
            if prob < 0.0 or prob > 1.0:
                raise ValueError("`prob` must be a float value between 0 and 1.")
        if len(set(kinds)) != len(kinds):
            raise ValueError(f"each perturbation may appear once in a chain, got {kinds}")
        self.seed, self.rank, self.sample_rate = int(seed), int(rank), int(sample_rate)
        speed = [p for _, p in self._pipeline if p.kind == "speed"]
        self.sr = speed[0]._sr if speed else self.sample_rate
        self.resample_type = speed[0]._res_type if speed else "kaiser_fast"
        self._rng = random.Random(f"{self.seed}:{self.rank}:{rng}:{[p.rng for _, p in self._pipeline]}")

    # ---- draws (host only)
    def draw(self, lengths: Sequence[int]) -> List[list]:
        """Per utterance, the steps that apply, in list order (AudioAugmentor.perturb :1087-1091).  A shift longer than the
        utterance as it stands at that point is skipped (:423-425)."""
        plans = []
        for n in lengths:
            cur, steps = int(n), []
            for prob, p in self._pipeline:
                if not self._rng.random() < prob:
                    continue
                d = p.draw(self._rng)
                if p.kind == "speed":
                    if d is not None:
                        steps.append(("speed", d))
                        cur = resampled_length(cur, p._sr, d)
                elif p.kind == "gain":
                    steps.append(("gain", d))
                elif p.kind == "shift":
                    if not abs(d) / 1000 > cur / self.sample_rate:
                        steps.append(("shift", shift_samples(d, self.sample_rate)))
                else:
                    steps.append(("white_noise", d[0], d[1]))
            plans.append(steps)
        return plans

    def fold(self, plans, lengths) -> Tuple[np.ndarray, List[int]]:
        folded = [fold_chain(steps, n, self.sr) for steps, n in zip(plans, lengths)]
        return pack_params([f for f, _ in folded]), [m for _, m in folded]

    def max_augmentation_length(self, length):
        for _, p in self._pipeline:
            if p.kind == "speed":
                length = length * p._max_rate
        return length

    # ---- the device pass
    def __call__(self, batch, host_lengths):
        signal, signal_len, tokens, tokens_len = batch
        h_sig, h_tok = host_lengths
        if not signal.is_cuda:
            raise RuntimeError("AudioAugmentor takes a device batch: its pass is a HIP kernel and has no host path")
        plans = self.draw(h_sig)
        if not any(plans):
            return batch, host_lengths
        rows, new_lens = self.fold(plans, h_sig)
        out = wave_augment(signal, rows, self.sr, self.resample_type)
        lens = torch.tensor(new_lens, dtype=signal_len.dtype).pin_memory().to(signal.device, non_blocking=True)
        return (out, lens, tokens, tokens_len), (new_lens, h_tok)

    # ---- resumable draws
    def state_dict(self):
        version, internal, gauss = self._rng.getstate()
        return {"seed": self.seed, "rank": self.rank, "rng_state": [version, list(internal), gauss]}

    def load_state_dict(self, state):
        version, internal, gauss = state["rng_state"]
        self._rng.setstate((version, tuple(internal), gauss))
        return self


def process_augmentations(augmenter, global_rank=0, world_size=1, seed=0, sample_rate=16000) -> Optional[AudioAugmentor]:
    """The `train_ds.augmentor` mapping of a NeMo yaml -- {name: {prob: ..., **kwargs}} with the names `speed`, `gain`, `shift`
    and `white_noise`, applied in the mapping's order -- as an AudioAugmentor; None and a ready AudioAugmentor pass through."""
    if augmenter is None or isinstance(augmenter, AudioAugmentor):
        return augmenter
    if not hasattr(augmenter, "items"):
        raise ValueError("Cannot parse augmenter. Must be a dict or an AudioAugmentor object ")
    refused = [k for k in augmenter if k not in perturbation_types]
    if refused:
        known = [k for k in refused if k in UNSUPPORTED]
        raise NotImplementedError(
            f"augmentor keys {refused} are not available: this package runs {list(perturbation_types)} on the device"
            + (f"; {known} need audio files, codecs or a phase vocoder" if known else ""))
    chain = []
    for name, kwargs in augmenter.items():
        kwargs = dict(kwargs)
        if kwargs.get("prob") is None:
            raise KeyError(f'Augmentation "{name}" will not be applied as keyword argument "prob" was not defined for this '
                           'augmentation.')
        prob = kwargs.pop("prob")
        if prob < 0.0 or prob > 1.0:
            raise ValueError("`prob` must be a float value between 0 and 1.")
        chain.append((prob, perturbation_types[name](**kwargs)))
    return AudioAugmentor(perturbations=chain, seed=seed, rank=global_rank, sample_rate=sample_rate)
