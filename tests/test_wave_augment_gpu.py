"""csrc/wave_augment.hip against the definition (tests/wave_augment_ref.py), through the C ABI (augment.wave_augment) and through
AudioAugmentor / BatchLoader.

Bound -- the project's rounding rule, C = 4 and FLOOR = 2^-20 of tests/test_block_reference_gpu.py:
    d(K, E) <= C * d(F32, E) + FLOOR        in relative L2 and in max-abs, per utterance of every case
on unit-scale inputs (white noise; one case of an impulse train).  E is the definition in fp64, F32 its float32 restatement with
the sum in increasing k; the kernel sums each wing outward from the centre with fma and adds the two, another order of the same
roundings.  The worst ratio d(K, E) / max(d(F32, E), FLOOR) is printed per case (observed: d(K, E) 0.9-1.5 x d(F32, E), both
1e-7 to 5e-7 relative, so the printed ratios stay below 1).

White noise: the kernel draws it with the project's counter-based generator in fp32 with the hardware log and cosine
(csrc/frontend_fft.hip ff_randn), the references take oracle.input_ref.randn_replica, its fp64 restatement.  The project holds that
pair to 1e-4 absolute per unit of amplitude (tests/test_input_reference_gpu.py::test_preemph_kernel_noise_equals_the_replica: what
the hardware log / cos may differ by; a wrong constant or swapped uniforms give O(1)).  A case with noise of amplitude a (after the
gains that follow it) therefore adds NOISE_TOL * a to the max-abs bound and NOISE_TOL * a * sqrt(n) to the L2 bound; noise that
passes through the resampler is a sum of at most 2 Z / s + 2 products with sum |w| < 2, hence the factor 2 there.

Every case pre-fills the output with NaN, requires every element of [B, L_out] finite and every element at or beyond an utterance's
new length exactly 0, and launches twice: bit-identical.
"""
import math

import numpy as np
import pytest
import torch

import wave_augment_ref as R
from indic_cl_asr_amd import augment as A
from test_block_reference_gpu import C, FLOOR, _dist

pytestmark = pytest.mark.gpu

SR = 16000
NOISE_TOL = 1e-4
RATES = (14400, 17600, 15273)       # s < 1 and q = sr; s = 1 and q = new_sr; a uniform draw with no small polyphase period


def _tile():
    from indic_cl_asr_amd import _lib
    return _lib.lib().ia_wave_augment_tile()


def _white(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(np.float32)


def _len_for(n_out, new_sr):
    """An input length whose resampled length is n_out (new_sr < sr: every length is reached)."""
    n = n_out * SR // new_sr
    while A.resampled_length(n, SR, new_sr) < n_out:
        n += 1
    assert A.resampled_length(n, SR, new_sr) == n_out
    return n


def _noise_amp(steps):
    """Amplitude of the chain's noise where it is compared: the level times every gain that follows it; and whether it is resampled."""
    amp, through = 0.0, False
    for s in steps:
        if s[0] == "white_noise":
            amp, through = 10.0 ** (s[1] / 20.0), False
        elif s[0] == "gain":
            amp *= 10.0 ** (s[1] / 20.0)
        elif s[0] == "speed" and amp:
            through = True
    return amp * (2.0 if through else 1.0)


def _launch(xs, chains, rtype):
    B, L_in = len(xs), max(len(x) for x in xs)
    sig = torch.zeros(B, L_in)
    for b, x in enumerate(xs):
        sig[b, :len(x)] = torch.from_numpy(x)
    folded = [A.fold_chain(steps, len(x), SR) for steps, x in zip(chains, xs)]
    rows, lens = A.pack_params([f for f, _ in folded]), [m for _, m in folded]
    dev = sig.cuda()
    outs = []
    for _ in range(2):
        out = torch.full((B, max(1, max(lens))), float("nan"), device="cuda")
        A.wave_augment(dev, rows, SR, rtype, out=out)
        outs.append(out.cpu())
    torch.cuda.synchronize()
    assert outs[0].view(torch.int32).equal(outs[1].view(torch.int32)), "two launches differ"
    K = outs[0]
    assert bool(torch.isfinite(K).all()), "an element of the output was not written"
    for b, n in enumerate(lens):
        assert not K[b, n:].any(), f"row {b}: padding beyond {n} is not zero"
    return K.double().numpy(), lens


def _hold(tag, K, E, F32, noise_amp=0.0):
    E, F32 = torch.from_numpy(E), torch.from_numpy(F32)
    K = torch.from_numpy(K)
    s2, sm = max(float(E.norm()), 1e-30), max(float(E.abs().max()), 1e-30)
    kl, km = _dist(K, E, s2, sm)
    ol, om = _dist(F32, E, s2, sm)
    tl, tm = NOISE_TOL * noise_amp * math.sqrt(E.numel()) / s2, NOISE_TOL * noise_amp / sm
    ratio = max(kl / max(ol, FLOOR), km / max(om, FLOOR))
    print(f"{tag}: L2 {kl:.3e} vs {ol:.3e}, max {km:.3e} vs {om:.3e}, ratio {ratio:.2f}" + (f", noise +{tm:.1e}" if noise_amp else ""))
    assert kl <= C * ol + FLOOR + tl, (tag, "rel L2", kl, ol)
    assert km <= C * om + FLOOR + tm, (tag, "max abs", km, om)
    return ratio


def _case(tag, xs, chains, rtype="kaiser_fast"):
    K, lens = _launch(xs, chains, rtype)
    worst = 0.0
    for b, (x, steps) in enumerate(zip(xs, chains)):
        E = R.apply_chain(x, steps, SR, b, rtype, "E")
        F32 = R.apply_chain(x, steps, SR, b, rtype, "F32")
        assert len(E) == lens[b]
        worst = max(worst, _hold(f"{tag}[{b}] n={len(x)}->{lens[b]}", K[b, :lens[b]], E, F32, _noise_amp(steps)))
    print(f"{tag}: worst ratio {worst:.2f}")


# ---------------------------------------------------------------------------------------------------- resampling
@pytest.mark.parametrize("rtype", ["kaiser_fast", "kaiser_best"])
@pytest.mark.parametrize("new_sr", [14400, 15273])
def test_output_lengths_around_the_tile(new_sr, rtype):
    T = _tile()
    xs = [_white(_len_for(n_out, new_sr), 10 + i) for i, n_out in enumerate((T - 1, T, T + 1, 2 * T + 3))]
    _case(f"tile/{new_sr}/{rtype}", xs, [[("speed", new_sr)]] * 4, rtype)


@pytest.mark.parametrize("rtype", ["kaiser_fast", "kaiser_best"])
@pytest.mark.parametrize("new_sr", RATES)
def test_utterances_shorter_than_the_filter(new_sr, rtype):
    Z = A.RESAMPLE_TABLES[rtype][0]
    xs = [_white(n, 20 + n) for n in (1, 5, 2 * Z)]
    _case(f"short/{new_sr}/{rtype}", xs, [[("speed", new_sr)]] * 3, rtype)


@pytest.mark.parametrize("rtype", ["kaiser_fast", "kaiser_best"])
def test_ragged_batch_with_an_untouched_utterance(rtype):
    xs = [_white(700, 1), _white(2100, 2), _white(1300, 3)]
    K, lens = _launch(xs, [[("speed", 17600)], [], [("speed", 14400)]], rtype)
    assert lens == [770, 2100, 1170]
    assert np.array_equal(K[1, :2100], xs[1].astype(np.float64))          # rate 1.0: the samples themselves
    _case(f"ragged/{rtype}", xs, [[("speed", 17600)], [], [("speed", 14400)]], rtype)


@pytest.mark.parametrize("new_sr", RATES)
def test_upsampled_tile_edges_and_the_uniform_rate(new_sr):
    T = _tile()
    xs = [_white(n, 30 + i) for i, n in enumerate((T, T + 1, 2 * T + 77))]
    _case(f"mid/{new_sr}", xs, [[("speed", new_sr)]] * 3)


def test_impulse_train():
    x = np.zeros(1500, dtype=np.float32)
    x[::37] = 1.0
    x[0], x[-1] = 1.0, -1.0
    _case("impulses", [x, x], [[("speed", 15273)], [("speed", 17600)]])


def test_long_utterance_where_m_sr_passes_2_31():
    """150,000 samples, silent but for 500 random samples ending at the last one, at 17,600; compared on the last two tiles
    (m sr >= 2^31 from m = 134,218 on: a 32-bit D(k) lands its taps elsewhere)."""
    T = _tile()
    n = 150000
    x = np.zeros(n, dtype=np.float32)
    x[-500:] = _white(500, 5)
    K, lens = _launch([x], [[("speed", 17600)]], "kaiser_fast")
    n_out = lens[0]
    assert n_out == 165000 and (n_out // T - 1) * T * SR >= 2 ** 31
    lo = (n_out // T - 1) * T                                              # the last full tile and the partial one behind it
    E = R.resample(x, SR, 17600, "kaiser_fast", "E", (lo, n_out))
    F32 = R.resample(x, SR, 17600, "kaiser_fast", "F32", (lo, n_out)).astype(np.float64)
    assert np.abs(E).max() > 0.5
    _hold("long", K[0, lo:n_out], E, F32)
    assert not K[0, :n_out - 600 - 40].any()                                # silence stays silence (500 samples and 2 Z taps away)


# ---------------------------------------------------------------------------------------------------- chains
CHAINS = {
    "shift_before_speed": [("shift", 7), ("speed", 14400)],
    "shift_after_speed": [("speed", 14400), ("shift", 7)],
    "neg_shift_before_speed": [("shift", -9), ("speed", 17600)],
    "neg_shift_after_speed": [("speed", 17600), ("shift", -9)],
    "gain_before_noise": [("gain", 6.0), ("white_noise", -6, 1234)],
    "gain_after_noise": [("white_noise", -6, 1234), ("gain", 6.0)],
    "speed_gain_noise": [("speed", 15273), ("gain", -4.5), ("white_noise", -12, 99)],
    "speed_noise_gain_shift": [("speed", 17600), ("white_noise", -12, 99), ("gain", -4.5), ("shift", 11)],
    "noise_shift": [("white_noise", -6, 7), ("shift", -5)],
    "shift_noise": [("shift", -5), ("white_noise", -6, 7)],
    "noise_speed": [("gain", 3.0), ("white_noise", -6, 7), ("speed", 14400), ("gain", 2.0)],
    "noise_shift_speed": [("white_noise", -6, 7), ("shift", 4), ("speed", 17600)],
    "shift_noise_speed": [("shift", 4), ("white_noise", -6, 7), ("speed", 17600)],
    "noise_speed_shift": [("white_noise", -6, 7), ("speed", 15273), ("shift", -3)],
}


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_chain_against_the_step_by_step_reference(name):
    T = _tile()
    xs = [_white(T + 300, 40), _white(333, 41)]
    _case(f"chain/{name}", xs, [CHAINS[name]] * 2)


@pytest.mark.parametrize("speed", [None, 14400])
def test_shifts_of_one_and_of_all_but_one_sample(speed):
    n = 1100
    x = _white(n, 50)
    m = n if speed is None else A.resampled_length(n, SR, speed)
    pre = [] if speed is None else [("speed", speed)]
    shifts = (-1, 1, -(m - 1), m - 1)
    _case(f"shift/{speed}", [x] * 4, [pre + [("shift", s)] for s in shifts])
    if speed is None:                                                      # the copy path is exact
        K, _ = _launch([x] * 4, [[("shift", s)] for s in shifts], "kaiser_fast")
        for b, s in enumerate(shifts):
            assert np.array_equal(K[b, :n], R.shift(x, s).astype(np.float64)), s
    else:                                                                   # ... and a shift in front of the resampling
        _case(f"shift/pre/{speed}", [x] * 4, [[("shift", s)] + pre for s in (-1, 1, -(n - 1), n - 1)])


def test_noise_equals_the_replica_and_stays_inside_the_utterance():
    """Silence plus noise at 0 dB is the noise itself: the replica of each row's own seed, none at or beyond the length."""
    from oracle.input_ref import randn_replica
    T = _tile()
    lens = [T + 5, 3, 2 * T]
    seeds = [0xC0FFEE, 1, 0xFFFFFFFF]
    xs = [np.zeros(n, dtype=np.float32) for n in lens]
    K, out_lens = _launch(xs, [[("white_noise", 0, s)] for s in seeds], "kaiser_fast")       # _launch: zero beyond each length
    assert out_lens == lens
    for b, (n, s) in enumerate(zip(lens, seeds)):
        err = np.abs(K[b, :n] - randn_replica(s, b + 1, n)[b]).max()
        print(f"noise row {b}: max |kernel - replica| = {err:.3e}")
        assert err < NOISE_TOL
        assert np.abs(K[b, :n]).max() > (1.0 if n > 100 else 0.0)
    K2, _ = _launch(xs, [[("white_noise", 0, s + 1 & 0xFFFFFFFF)] for s in seeds], "kaiser_fast")
    assert np.abs(K2[0, :lens[0]] - K[0, :lens[0]]).max() > 1.0            # another seed, other noise


def test_a_row_the_launch_was_not_sized_for_is_loud():
    """min_new_sr sizes the LDS span; a row below it is written as NaN instead of reading past the span."""
    from indic_cl_asr_amd import _lib
    x = torch.from_numpy(_white(3000, 60)).cuda().view(1, -1)
    rows = A.pack_params([A.fold_chain([("speed", 8000)], 3000, SR)[0]])
    out = torch.zeros(1, 1500, device="cuda")
    table = torch.from_numpy(A.resample_table("kaiser_fast").astype(np.float32)).cuda()
    dev = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
    _lib.check(_lib.lib().ia_wave_augment(_lib.ptr(x), 1, 3000, _lib.ptr(out), 1500, _lib.ptr(dev), _lib.ptr(table), 16, SR, 16000,
                                          _lib.stream_ptr()), "ia_wave_augment")
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------------------------------------------- the public path
def _augmentor(seed=7):
    return A.AudioAugmentor([(1.0, A.ShiftPerturbation(-3.0, 3.0)),
                             (1.0, A.SpeedPerturbation(SR, "kaiser_fast", 0.9, 1.1, num_rates=3)),
                             (0.5, A.GainPerturbation(-6, 6)),
                             (0.5, A.WhiteNoisePerturbation(-40, -20))], seed=seed)


def test_augmentor_on_a_device_batch_matches_its_own_draws():
    lens = [900, 2300, 1, 1500, 640]
    xs = [_white(n, 70 + i) for i, n in enumerate(lens)]
    sig = torch.zeros(len(xs), max(lens))
    for b, x in enumerate(xs):
        sig[b, :len(x)] = torch.from_numpy(x)
    tok, tok_len = torch.zeros(len(xs), 2, dtype=torch.long).cuda(), torch.full((len(xs),), 2).cuda()
    batch = (sig.cuda(), torch.tensor(lens).cuda(), tok, tok_len)
    aug, twin = _augmentor(), _augmentor()
    (y, y_len, tok2, tok_len2), (h_sig, h_tok) = aug(batch, (lens, [2] * len(xs)))
    plans = twin.draw(lens)
    assert tok2 is tok and tok_len2 is tok_len and h_tok == [2] * len(xs)
    assert y_len.tolist() == h_sig and y_len.dtype == batch[1].dtype and y.shape == (len(xs), max(h_sig))
    assert {s[0] for p in plans for s in p} == set(A.KINDS)
    K = y.cpu().double().numpy()
    for b, (x, steps) in enumerate(zip(xs, plans)):
        E, F32 = R.apply_chain(x, steps, SR, b, mode="E"), R.apply_chain(x, steps, SR, b, mode="F32")
        assert len(E) == h_sig[b]
        _hold(f"augmentor[{b}]", K[b, :h_sig[b]], E, F32, _noise_amp(steps))
        assert not K[b, h_sig[b]:].any()


class _Items:
    """Three utterances of a few hundred milliseconds with token rows, as data.SpeechDataset yields them."""

    def __init__(self):
        self.x = [torch.from_numpy(0.1 * _white(n, 80 + i)) for i, n in enumerate((4800, 6400, 3521))]
        self.t = [torch.tensor([3, 1, 4]), torch.tensor([1, 5]), torch.tensor([9, 2, 6, 5])]
        self.dur = [x.numel() / SR for x in self.x]

    def __len__(self):
        return len(self.x)

    def __getitem__(self, i):
        return self.x[i], torch.tensor(self.x[i].numel()), self.t[i], torch.tensor(self.t[i].numel())


def test_loader_without_an_augmentor_is_the_plain_collate():
    from indic_cl_asr_amd import data as D
    ds = _Items()
    want = D.speech_collate([ds[i] for i in range(3)])
    (batch, lens), = list(D.BatchLoader(ds, batch_size=3, device="cuda", augmentor=None))
    for got, ref in zip(batch, want):
        assert got.is_cuda and got.dtype == ref.dtype and torch.equal(got.cpu(), ref)
    assert lens == (want[1].tolist(), want[3].tolist())


def test_loader_with_an_augmentor_feeds_training_step():
    from indic_cl_asr_amd import data as D
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.features import mel_frame_count
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    ds = _Items()
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny', vocab_per_lang=64, compute_dtype='fp32')).cuda().train()
    plans = _augmentor(3).draw([x.numel() for x in ds.x])
    (batch, host_lens), = list(D.BatchLoader(ds, batch_size=3, device="cuda", augmentor=_augmentor(3)))
    want = [A.fold_chain(p, x.numel(), SR)[1] for p, x in zip(plans, ds.x)]
    assert host_lens[0] == want == batch[1].tolist() and host_lens[0] != [x.numel() for x in ds.x]
    assert batch[0].shape == (3, max(want)) and host_lens[1] == [3, 2, 4]
    _, flen = m.preprocessor(input_signal=batch[0], length=batch[1], dither=False)
    assert flen.tolist() == [mel_frame_count(n, m.cfg.n_fft, m.cfg.n_window_stride) for n in want]
    loss, _ = m.training_step(batch, ['hi'] * 3, host_lengths=host_lens, compute_wer=False)
    assert torch.isfinite(loss)
    with pytest.raises(RuntimeError):
        D.BatchLoader(ds, batch_size=3, augmentor=_augmentor(3))           # no device, no kernel: refused, not skipped


def test_transcribe_applies_its_augmentor():
    """transcribe(augmentor=...) used to drop the argument: a gain of -200 dB now silences the audio the model hears."""
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, TranscribeConfig
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny', vocab_per_lang=64, compute_dtype='fp32')).cuda()
    audio = [0.1 * _white(4000, 90), 0.1 * _white(3000, 91)]
    cfg = TranscribeConfig(batch_size=2, augmentor={"gain": {"prob": 1.0, "min_gain_dbfs": -200, "max_gain_dbfs": -200}})
    cfg._internal = None
    (plain,), (quiet,) = (list(m._transcribe_input_processing(audio, c)) for c in (TranscribeConfig(batch_size=2), cfg))
    assert float(plain[0].abs().max()) > 0.1 and float(quiet[0].abs().max()) < 1e-9
    assert torch.equal(plain[1], quiet[1])
    with pytest.raises(NotImplementedError):
        m.transcribe(audio, batch_size=2, language_id='hi', augmentor={"time_stretch": {"prob": 1.0}})
