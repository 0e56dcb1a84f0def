"""ia_wave_augment on the benchmark's batch (32 utterances of 15 s at 16 kHz, speed rates 0.9 / 1.0 / 1.1 mixed over the rows)
for both tables, beside the time of the log-mel front end it runs in front of (ia_feat_preemph + ia_feat_logmel_fft through
ops.frontend.log_mel, dither on) in the same process.  Legs: `fast_us` / `best_us` the launch alone (kaiser_fast / kaiser_best,
rows of parameters already on the device); `fast_chain_us` the same with shift, gain and output-stage noise folded in; `copy_us` a
batch in which no utterance is resampled (gain and noise only); `augmentor_host_us` the host wall-clock of one AudioAugmentor call
(draws, folding, the pinned copies, the launch; nothing waited for); `logmel_us` the front end.  Device time between two events.
Developer tool; one JSON line."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timeit(fn, warmup=5, n=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def host_timeit(fn, warmup=5, n=50):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    return (t1 - t0) / n * 1e6


def main():
    from indic_cl_asr_amd import _lib
    from indic_cl_asr_amd import augment as A
    from indic_cl_asr_amd.features import mel_filterbank_slaney
    from indic_cl_asr_amd.ops import frontend
    torch.manual_seed(0)
    B, L, sr = 32, 240000, 16000
    x = (0.1 * torch.randn(B, L)).cuda()
    rates = [(14400, 0, 17600)[b % 3] for b in range(B)]
    L_ = _lib.lib()

    def leg(chains, rtype):
        folded = [A.fold_chain(c, L, sr)[0] for c in chains]
        rows = A.pack_params(folded)
        dev = torch.from_numpy(rows.view(np.uint8).copy()).cuda()
        L_out = int(rows["n_out"].max())
        out = torch.empty(B, L_out, device="cuda")
        active = rows["new_sr"][rows["new_sr"] > 0]
        mn = int(active.min()) if active.size else 0
        table = torch.from_numpy(A.resample_table(rtype).astype(np.float32)).cuda()
        Z = A.RESAMPLE_TABLES[rtype][0]

        def run():
            _lib.check(L_.ia_wave_augment(_lib.ptr(x), B, L, _lib.ptr(out), L_out, _lib.ptr(dev), _lib.ptr(table), Z, sr, mn,
                                          _lib.stream_ptr()), "ia_wave_augment")
        return timeit(run)

    speed = [[("speed", r)] if r else [] for r in rates]
    full = [[("shift", 40)] + s + [("gain", 3.0), ("white_noise", -50, 1000 + b)] for b, s in enumerate(speed)]
    res = {"batch": [B, L], "new_sr": sorted(set(rates))}
    res["fast_us"] = round(leg(speed, "kaiser_fast"), 1)
    res["best_us"] = round(leg(speed, "kaiser_best"), 1)
    res["fast_chain_us"] = round(leg(full, "kaiser_fast"), 1)
    res["copy_us"] = round(leg([[("gain", 3.0), ("white_noise", -50, b)] for b in range(B)], "kaiser_fast"), 1)

    aug = A.AudioAugmentor([(1.0, A.SpeedPerturbation(sr, "kaiser_fast", 0.9, 1.1, num_rates=3)), (1.0, A.GainPerturbation()),
                            (1.0, A.ShiftPerturbation()), (1.0, A.WhiteNoisePerturbation())])
    batch = (x, torch.full((B,), L, device="cuda"), torch.zeros(B, 1, dtype=torch.long, device="cuda"),
             torch.ones(B, dtype=torch.long, device="cuda"))
    res["augmentor_host_us"] = round(host_timeit(lambda: aug(batch, ([L] * B, [1] * B))), 1)

    window = torch.hann_window(400, periodic=False).cuda()
    fb = torch.as_tensor(mel_filterbank_slaney(sr, 512, 80)).float().cuda()
    res["logmel_us"] = round(timeit(lambda: frontend.log_mel(x, window, fb, n_fft=512, hop=160, preemph=0.97, dither=1e-5, seed=1)), 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
