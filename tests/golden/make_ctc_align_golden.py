"""Writes tests/golden/ctc_align_cases.npz: CTC forced-alignment cases and what the reference's aligner returns for them.

Run by hand where the reference tree is at hand; never imported by a test:

    python tests/golden/make_ctc_align_golden.py [/path/to/NeMo]        (default /root/reference/NeMo)

The reference is NeMo forced aligner's viterbi_decoding (tools/nemo_forced_aligner/utils/viterbi_decoding.py), loaded by file
path with that tool's directory on sys.path and run ONE UTTERANCE AT A TIME (B = 1, T_max = T_b): its treatment of a shorter
utterance's padded frames is not part of the contract.

Every input lies on a dyadic grid: log-prob = -g * step with g an integer, step = 2^-6 on [-8, 0] (fine grid) or 1.0 on
[-4, 0] (coarse grid: most decisions are ties).  With T <= 376 every partial sum is an integer multiple of 2^-6 below
376 * 8 = 3008 < 2^12, i.e. needs at most 12 + 6 + 1 = 19 bits: every fp32 addition is exact, in the reference, in the host
routine and in the kernel, so the comparison is exact equality of path, spans and score, ties included.  The logits mode
adds a synthetic per-frame lse = z * step (z in [0, 8 / step]): logit = log-prob + lse and logit - lse are exact as well.

Stored per utterance i (grid indices as int16, npz compressed): g{i} [T,V], z{i} [T], y{i} [S], path{i} [T] (the reference's
alignment; empty when infeasible); per-file arrays: step [n], score [n] f64 (the reference path rescored; -inf when
infeasible), name [n], batch [k] (the utterances that form the ragged batch case).  blank = V - 1.

Before writing, the script asserts that the reference and an fp64 restatement of the recurrence with the contract's
tie-break (stay over s-1 over s-2; L-2 over L-1; L = 1 ends in state 0) agree exactly on every feasible case, and that
every infeasible case (T_b < labels + adjacent repeats) scores -inf in the restatement.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))

SHAPES = [(1, 0), (1, 1), (3, 0), (5, 2), (40, 31), (70, 32), (130, 63), (140, 64), (150, 127), (160, 128), (300, 255)]
WIDE = {("random", 70, 32), ("random", 140, 64)}      # V = 257 (ld = 264 in the device test); everything else V = 33


def load_reference(nemo_root):
    tool = os.path.join(nemo_root, "tools", "nemo_forced_aligner")
    sys.path.insert(0, tool)
    spec = importlib.util.spec_from_file_location("nfa_viterbi_decoding", os.path.join(tool, "utils", "viterbi_decoding.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.viterbi_decoding


def targets_for(rng, S, V, mode):
    y = rng.integers(0, V - 1, size=S)
    if mode == "repeats":                      # every third target repeats its predecessor: the skip is forbidden there
        for i in range(2, S, 3):
            y[i] = y[i - 1]
    return y.astype(np.int64)


def min_frames(y):
    return len(y) + int(np.sum(y[1:] == y[:-1]))


def restate_fp64(lp, y, blank):
    """(path or None, score) of the recurrence in fp64 with the contract's tie-break."""
    T, S = lp.shape[0], len(y)
    L = 2 * S + 1
    ext = np.full(L, blank, dtype=np.int64)
    ext[1::2] = y
    skip = np.zeros(L, dtype=bool)
    skip[3::2] = ext[3::2] != ext[1:-2:2]
    v = np.full(L, -np.inf)
    v[:2] = lp[0, ext[:2]]
    bps = np.zeros((T, L), dtype=np.int8)
    for t in range(1, T):
        a1 = np.concatenate([[-np.inf], v[:-1]])
        a2 = np.concatenate([[-np.inf, -np.inf], v[:-2]])[:L]
        a2 = np.where(skip, a2, -np.inf)
        m, bp = v.copy(), np.zeros(L, dtype=np.int8)
        take = a1 > m
        m, bp = np.where(take, a1, m), np.where(take, 1, bp)
        take = a2 > m
        m, bp = np.where(take, a2, m), np.where(take, 2, bp)
        v, bps[t] = m + lp[t, ext], bp
    s = L - 1 if (L == 1 or v[L - 1] > v[L - 2]) else L - 2
    score = v[s]
    if score == -np.inf:
        return None, score
    path = [s]
    for t in range(T - 1, 0, -1):
        s -= int(bps[t, s])
        path.insert(0, s)
    return np.array(path), score


def main():
    nemo_root = sys.argv[1] if len(sys.argv) > 1 else "/root/reference/NeMo"
    viterbi_decoding = load_reference(nemo_root)
    rng = np.random.default_rng(20240607)
    cases = []          # (name, T, y, V, step)

    for T, S in SHAPES:
        for mode in ("random", "repeats", "coarse"):
            V = 257 if (mode, T, S) in WIDE else 33
            cases.append((f"{mode}_T{T}_S{S}", T, targets_for(rng, S, V, mode), V, 1.0 if mode == "coarse" else 2.0 ** -6))
    y = targets_for(rng, 24, 33, "repeats")
    cases.append(("min_feasible", min_frames(y), y, 33, 2.0 ** -6))
    cases.append(("below_min", min_frames(y) - 1, y.copy(), 33, 2.0 ** -6))
    batch = []
    for T, S in ((37, 9), (50, 0), (23, 11), (61, 30)):      # lengths that are no multiples of the prefetch depths 2 and 4
        batch.append(len(cases))
        cases.append((f"batch_T{T}_S{S}", T, targets_for(rng, S, 33, "repeats" if S == 11 else "random"), 33, 2.0 ** -6))

    out = {}
    steps, scores, names = [], [], []
    n_feasible = n_infeasible = 0
    for i, (name, T, y, V, step) in enumerate(cases):
        blank = V - 1
        g = rng.integers(0, int((4 if step == 1.0 else 8) / step) + 1, size=(T, V))
        z = rng.integers(0, int(8 / step) + 1, size=T)
        lp32 = (-(g.astype(np.float64)) * step).astype(np.float32)
        assert np.all(lp32.astype(np.float64) == -(g * step))
        path64, score64 = restate_fp64(lp32.astype(np.float64), y, blank)
        feasible = T >= min_frames(y)
        assert feasible == (path64 is not None), name
        if feasible:
            ext = np.full(2 * len(y) + 1, blank, dtype=np.int64)
            ext[1::2] = y
            ref = viterbi_decoding(torch.from_numpy(lp32).unsqueeze(0), torch.from_numpy(ext).unsqueeze(0),
                                   torch.tensor([T]), torch.tensor([len(ext)]), torch.device("cpu"))[0]
            ref = np.array(ref, dtype=np.int64)
            assert ref.shape == (T,) and np.array_equal(ref, path64), f"{name}: reference and fp64 restatement differ"
            rescored = float(np.sum(lp32.astype(np.float64)[np.arange(T), ext[ref]]))
            assert rescored == score64, name
            n_feasible += 1
        else:
            ref, rescored = np.zeros(0, dtype=np.int64), -np.inf
            n_infeasible += 1
        out[f"g{i}"], out[f"z{i}"] = g.astype(np.int16), z.astype(np.int16)
        out[f"y{i}"], out[f"path{i}"] = y.astype(np.int16), ref.astype(np.int16)
        steps.append(step); scores.append(rescored); names.append(name)
    out["step"], out["score"] = np.array(steps, dtype=np.float64), np.array(scores, dtype=np.float64)
    out["name"], out["batch"] = np.array(names), np.array(batch, dtype=np.int64)
    dst = os.path.join(HERE, "ctc_align_cases.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {len(cases)} utterances, {n_feasible} feasible (reference == fp64 restatement on all), "
          f"{n_infeasible} infeasible, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    main()
