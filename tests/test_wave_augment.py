"""Waveform augmentation, host side (indic_cl_asr_amd/augment.py): draws, the length rule, parsing, the folding of a chain into
the kernel's parameters, and a sanity anchor on the fp64 definition itself (tests/wave_augment_ref.py).  No device."""
import ctypes

import numpy as np
import pytest

import wave_augment_ref as R
from indic_cl_asr_amd import augment as A

SR = 16000


def _chain(seed=0, rank=0):
    return A.AudioAugmentor([(0.8, A.ShiftPerturbation(-20.0, 20.0)),
                             (0.9, A.SpeedPerturbation(SR, "kaiser_fast", 0.9, 1.1, num_rates=-1)),
                             (0.7, A.GainPerturbation(-6, 6)),
                             (0.6, A.WhiteNoisePerturbation(-60, -40))], seed=seed, rank=rank)


LENGTHS = [16000, 8000, 24000, 12000, 4000, 1, 37]


# ---------------------------------------------------------------------------------------------------- draws
def test_draws_are_reproducible_from_the_seed():
    a, b = _chain(3), _chain(3)
    assert [a.draw(LENGTHS) for _ in range(3)] == [b.draw(LENGTHS) for _ in range(3)]
    assert _chain(4).draw(LENGTHS) != _chain(3).draw(LENGTHS)


def test_draws_resume_across_a_state_dict_round_trip():
    a = _chain(5)
    a.draw(LENGTHS)
    state = a.state_dict()
    import json
    state = json.loads(json.dumps(state))            # plain data: survives a checkpoint's serialisation
    want = [a.draw(LENGTHS) for _ in range(2)]
    b = _chain(5).load_state_dict(state)
    assert [b.draw(LENGTHS) for _ in range(2)] == want


def test_two_ranks_draw_different_chains():
    assert _chain(0, rank=0).draw(LENGTHS) != _chain(0, rank=1).draw(LENGTHS)


def test_every_step_kind_appears_and_probabilities_gate_them():
    plans = _chain(1).draw([16000] * 200)
    kinds = [[s[0] for s in p] for p in plans]
    for k in A.KINDS:
        assert 0 < sum(k in ks for ks in kinds) < 200
    for ks in kinds:                                    # list order is kept
        assert ks == [k for k in ("shift", "speed", "gain", "white_noise") if k in ks]
    never = A.AudioAugmentor([(0.0, A.GainPerturbation())]).draw([100] * 50)
    assert not any(never)
    levels = {s[1] for p in plans for s in p if s[0] == "white_noise"}
    assert levels <= set(range(-60, -40)) and all(isinstance(v, int) for v in levels)


# ---------------------------------------------------------------------------------------------------- lengths
@pytest.mark.parametrize("n", [1, 2, 9, 10, 11, 1199, 1200, 240000])
@pytest.mark.parametrize("new_sr", [14400, 17600, 15273])
def test_length_rule_is_the_ceiling(n, new_sr):
    from fractions import Fraction
    import math
    want = math.ceil(Fraction(n * new_sr, SR))
    assert A.resampled_length(n, SR, new_sr) == want
    f, m = A.fold_chain([("speed", new_sr)], n, SR)
    assert m == want == f["n_out"] and f["n_in"] == n
    assert len(R.resample(np.ones(min(n, 1200)), SR, new_sr)) == A.resampled_length(min(n, 1200), SR, new_sr)


def test_length_rule_rounds_up_where_floor_differs():
    assert A.resampled_length(1, SR, 14400) == 1 and A.resampled_length(1, SR, 17600) == 2
    assert A.resampled_length(11, SR, 14400) == 10 and A.resampled_length(9, SR, 14400) == 9


def test_rate_one_leaves_the_utterance_alone():
    aug = A.AudioAugmentor([(1.0, A.SpeedPerturbation(SR, "kaiser_fast", 1.0, 1.0, num_rates=1))])
    assert aug.draw([123, 1]) == [[], []]
    rows, lens = aug.fold(aug.draw([123, 1]), [123, 1])
    assert lens == [123, 1] and rows["new_sr"].tolist() == [0, 0] and rows["n_out"].tolist() == [123, 1]
    # a rate that maps onto sr itself (int(16000 * 1.00001) == 16000) is no resampling either
    near = A.SpeedPerturbation(SR, "kaiser_fast", 1.00001, 1.00001, num_rates=1)
    assert near.draw(__import__("random").Random(0)) is None


def test_speed_rates_follow_the_reference_rule():
    sp = A.SpeedPerturbation(SR, "kaiser_best", 0.9, 1.1, num_rates=3)
    import random
    rng = random.Random(0)
    got = {sp.draw(rng) for _ in range(100)}
    assert got == {int(SR * 0.9), None, int(SR * 1.1)}
    with pytest.raises(NotImplementedError):
        A.SpeedPerturbation(SR, "fft")
    with pytest.raises(NotImplementedError):
        A.SpeedPerturbation(SR, "scipy")
    with pytest.raises(ValueError):
        A.SpeedPerturbation(SR, "sinc_best")


# ---------------------------------------------------------------------------------------------------- shift
def test_shift_samples_uses_floor_division():
    assert A.shift_samples(-2.53, SR) == -41 and A.shift_samples(2.53, SR) == 40       # int(shift_ms * sr // 1000)
    assert A.shift_samples(-0.03, SR) == -1 and A.shift_samples(0.03, SR) == 0
    assert A.shift_samples(-5.0, SR) == -80 and A.shift_samples(5.0, SR) == 80


def test_a_shift_longer_than_the_utterance_is_skipped():
    aug = A.AudioAugmentor([(1.0, A.ShiftPerturbation(-10.0, -10.0))])
    plans = aug.draw([159, 160, 161])                   # 10 ms = 160 samples: skipped when 0.010 > n / sr
    assert plans == [[], [("shift", -160)], [("shift", -160)]]
    # after a speed step the comparison uses the length at that point
    aug = A.AudioAugmentor([(1.0, A.SpeedPerturbation(SR, "kaiser_fast", 1.1, 1.1, num_rates=1)),
                            (1.0, A.ShiftPerturbation(10.0, 10.0))])
    plans = aug.draw([146])                             # 146 -> 161 samples
    assert plans == [[("speed", 17600), ("shift", 160)]]


def test_shift_sign_in_the_reference():
    x = np.arange(1.0, 6.0)
    assert R.shift(x, -2).tolist() == [0, 0, 1, 2, 3]   # negative delays, zeroes the head
    assert R.shift(x, 2).tolist() == [3, 4, 5, 0, 0]    # positive advances, zeroes the tail
    assert R.shift(x, 5).tolist() == [0] * 5 and R.shift(x, -4).tolist() == [0, 0, 0, 0, 1]


# ---------------------------------------------------------------------------------------------------- folding
def test_fold_places_shift_and_noise_by_list_order():
    n = 1000
    f, _ = A.fold_chain([("shift", 7), ("speed", 14400)], n, SR)
    assert (f["shift_pre"], f["shift_post"]) == (7, 0)
    f, _ = A.fold_chain([("speed", 14400), ("shift", 7)], n, SR)
    assert (f["shift_pre"], f["shift_post"]) == (0, 7)
    f, _ = A.fold_chain([("gain", 20.0), ("white_noise", -20, 9)], n, SR)
    assert f["gain"] == pytest.approx(10.0) and f["noise_amp"] == pytest.approx(0.1) and f["noise_stage"] == 0
    f, _ = A.fold_chain([("white_noise", -20, 9), ("gain", 20.0)], n, SR)
    assert f["gain"] == pytest.approx(10.0) and f["noise_amp"] == pytest.approx(1.0)
    f, _ = A.fold_chain([("white_noise", -20, 9), ("shift", -3), ("speed", 17600), ("gain", 20.0)], n, SR)
    assert (f["noise_stage"], f["noise_shift"], f["shift_pre"]) == (1, -3, -3) and f["noise_amp"] == pytest.approx(0.1)
    f, _ = A.fold_chain([("shift", -3), ("white_noise", -20, 9), ("speed", 17600)], n, SR)
    assert (f["noise_stage"], f["noise_shift"], f["shift_pre"]) == (1, 0, -3)
    f, _ = A.fold_chain([("white_noise", -20, 9), ("speed", 17600), ("shift", 4)], n, SR)
    assert (f["noise_stage"], f["noise_shift"], f["shift_post"]) == (1, 0, 4)
    f, _ = A.fold_chain([("speed", 17600), ("white_noise", -20, 9), ("shift", 4)], n, SR)
    assert (f["noise_stage"], f["noise_shift"], f["shift_post"]) == (0, 4, 4)


def test_parameter_rows_match_the_c_struct():
    from indic_cl_asr_amd import _lib
    assert A.PARAMS_DTYPE.itemsize == ctypes.sizeof(_lib.WaveParams) == 48
    for name, _ in _lib.WaveParams._fields_:
        assert A.PARAMS_DTYPE.fields[name][1] == getattr(_lib.WaveParams, name).offset
    rows = A.pack_params([A.fold_chain([("speed", 17600), ("gain", 6.0)], 10, SR)[0]])
    c = _lib.WaveParams.from_buffer_copy(rows.tobytes())
    assert (c.n_in, c.n_out, c.new_sr) == (10, 11, 17600) and c.gain == pytest.approx(10 ** 0.3)


def test_entry_point_refuses_bad_arguments_before_device_work():
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    assert L.ia_wave_augment_tile() > 0 and L.ia_wave_augment_tile() % 256 == 0
    assert L.ia_wave_augment(None, 1, 16, None, 16, None, None, 16, SR, 0, None) == -1
    x, y, p, t = (ctypes.c_void_p(4096 * (i + 1)) for i in range(4))    # never dereferenced: every call is refused
    assert L.ia_wave_augment(x, 1, 16, x, 16, p, t, 16, SR, 0, None) == -1            # in place
    assert L.ia_wave_augment(x, 0, 16, y, 16, p, t, 16, SR, 0, None) == -1
    assert L.ia_wave_augment(x, 1, 16, y, 0, p, t, 16, SR, 0, None) == -1
    assert L.ia_wave_augment(x, 1, 16, y, 16, p, t, 32, SR, 14400, None) == -1        # no such table
    assert L.ia_wave_augment(x, 1, 16, y, 16, p, None, 16, SR, 14400, None) == -1     # resampling without a table
    assert L.ia_wave_augment(x, 1, 16, y, 16, p, t, 16, 0, 14400, None) == -1
    assert L.ia_wave_augment(x, 1, 16, y, 16, p, t, 16, SR, -1, None) == -1
    assert L.ia_wave_augment(x, 1, 16, y, 16, p, t, 16, SR, 100, None) == -4          # a span that does not fit in LDS


# ---------------------------------------------------------------------------------------------------- parsing
def test_process_augmentations_builds_the_chain_in_mapping_order():
    cfg = {"speed": {"prob": 0.5, "sr": SR, "resample_type": "kaiser_best", "min_speed_rate": 0.9, "max_speed_rate": 1.1,
                     "num_rates": 3},
           "gain": {"prob": 1.0, "min_gain_dbfs": -3, "max_gain_dbfs": 3},
           "white_noise": {"prob": 0.25, "min_level": -70, "max_level": -50},
           "shift": {"prob": 0.75, "min_shift_ms": -2.0, "max_shift_ms": 2.0}}
    aug = A.process_augmentations(cfg, global_rank=2, seed=11)
    assert [(prob, type(p).__name__) for prob, p in aug._pipeline] == [
        (0.5, "SpeedPerturbation"), (1.0, "GainPerturbation"), (0.25, "WhiteNoisePerturbation"), (0.75, "ShiftPerturbation")]
    assert aug.resample_type == "kaiser_best" and aug.rank == 2 and aug.seed == 11
    assert cfg["gain"]["prob"] == 1.0                   # the caller's mapping is left alone
    assert A.process_augmentations(None) is None and A.process_augmentations(aug) is aug
    with pytest.raises(KeyError):
        A.process_augmentations({"gain": {"min_gain_dbfs": -3}})
    with pytest.raises(ValueError):
        A.process_augmentations({"gain": {"prob": 1.5}})


@pytest.mark.parametrize("key", ["time_stretch", "noise", "impulse", "rir_noise_aug", "transcode_aug", "silence", "bogus"])
def test_process_augmentations_refuses_what_it_cannot_run(key):
    with pytest.raises(NotImplementedError, match=key):
        A.process_augmentations({"gain": {"prob": 1.0}, key: {"prob": 1.0}})


def test_a_repeated_kind_is_refused():
    with pytest.raises(ValueError):
        A.AudioAugmentor([(1.0, A.GainPerturbation()), (0.5, A.GainPerturbation(-1, 1))])
    with pytest.raises(ValueError):
        A.fold_chain([("speed", 14400), ("speed", 17600)], 100, SR)


def test_compat_path_resolves_to_the_same_names():
    from indic_cl_asr_amd.compat.NeMo.nemo.collections.asr.parts.preprocessing import perturb
    for name in ("SpeedPerturbation", "GainPerturbation", "ShiftPerturbation", "WhiteNoisePerturbation", "AudioAugmentor",
                 "process_augmentations", "perturbation_types"):
        assert getattr(perturb, name) is getattr(A, name)


def test_the_augmentor_has_no_host_path():
    import torch
    aug = _chain()
    batch = (torch.zeros(2, 100), torch.tensor([100, 50]), torch.zeros(2, 1, dtype=torch.long), torch.tensor([1, 1]))
    with pytest.raises(RuntimeError, match="device"):
        aug(batch, ([100, 50], [1, 1]))


# ---------------------------------------------------------------------------------------------------- the table and E
def test_tables_have_the_stated_shape():
    for name, (Z, rolloff, _) in A.RESAMPLE_TABLES.items():
        h = A.resample_table(name)
        assert h.shape == (Z * A.P + 1,) and abs(h[0] - rolloff) < 1e-15 and h[-1] == 0.0
        assert abs(h[A.P]) < 0.2 * rolloff and np.all(np.abs(h) <= rolloff)


@pytest.mark.parametrize("new_sr", [14400, 17600, 15273])
@pytest.mark.parametrize("freq", [300.0, 3000.0])
def test_a_passband_sinusoid_comes_out_on_the_new_grid(freq, new_sr):
    """The anchor on E: kaiser_fast, 1,200 samples, 60 ignored at each edge.  Measured worst max-abs error over these six cases:
    6.7e-5 (3 kHz -> 17,600); bound 2e-4.  (5.5 kHz lies in the kaiser_fast transition band at 14,400 and is not part of the test.)"""
    n = 1200
    x = np.sin(2 * np.pi * freq * np.arange(n) / SR)
    y = R.resample(x, SR, new_sr, "kaiser_fast", "E")
    want = np.sin(2 * np.pi * freq * np.arange(len(y)) / new_sr)
    err = np.abs(y - want)[60:-60].max()
    print(f"{freq:.0f} Hz -> {new_sr}: max |E - sinusoid| = {err:.2e}")
    assert err < 2e-4


def test_f32_reference_stays_at_rounding_distance_from_e():
    rng = np.random.default_rng(0)
    x = rng.standard_normal(700).astype(np.float32)
    for new_sr in (14400, 17600):
        e, f = R.resample(x, SR, new_sr, mode="E"), R.resample(x, SR, new_sr, mode="F32")
        assert f.dtype == np.float32 and 0 < np.abs(f - e).max() < 32 * 2.0 ** -24 * np.abs(e).max()
