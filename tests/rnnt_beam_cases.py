"""The cases of the transducer beam search tests (tests/test_rnnt_beam.py on the host, tests/test_rnnt_beam_gpu.py on the
device): operands from tests/test_greedy_decode_gpu.py::_bf16_case, the reference = decoding.beam_rnnt_alsd_host with the
kernel's rounding points, computed once per (case, weight type) and shared.

Both weight types run on the same values: "bf16" hands the kernel the bf16 images (rounding "mfma": the head's operand is
rounded to bf16), "fp32" the same values widened (rounding "gemv": nothing is rounded).

The blank biases were tuned on the reference alone until the conditions of `check_conditions` held: at most a quarter of a
case's utterances undecided; in a balanced case at least one recombination and a non-empty finished list in at least half of
its utterances."""
import functools

import torch

# name: B, T, Hp, Hj, V, W, lens, blank bias, seed, alsd_max_target_len, balanced
CASES = {
    "w4":         (8, 24, 64, 64, 17, 4, None, 3.0, 11, 3, True),
    "full_tile":  (8, 20, 128, 96, 33, 16, None, 6.0, 22, 0.5, True),       # 16 rows; the last head tile holds one label
    "w2":         (8, 16, 64, 64, 40, 2, None, 3.0, 143, 1.0, True),
    "production": (8, 12, 640, 640, 257, 8, None, 5.0, 74, 3, True),
    "w1":         (8, 16, 64, 64, 17, 1, None, 2.0, 15, 1.0, True),         # one member: nothing to recombine with
    "clamped":    (4, 20, 64, 64, 40, 4, (20, 0, -3, 25), 5.0, 26, 0.5, True),
    "all_blank":  (4, 12, 64, 64, 17, 4, None, 50.0, 37, 1.0, False),
    "never_blank": (8, 10, 64, 64, 17, 2, None, -50.0, 98, 3, False),       # F stays empty: sequences of len + u_max labels
}
ROUNDING = {"bf16": "mfma", "fp32": "gemv"}


@functools.lru_cache(maxsize=None)
def operands(name):
    from test_greedy_decode_gpu import _bf16_case
    B, T, Hp, Hj, V, W, lens, bias, seed, a, _ = CASES[name]
    return _bf16_case(B, T, Hp, Hj, V, seed, bias, None if lens is None else torch.tensor(lens))


def case_for(name, weights):
    c = dict(operands(name))
    if weights == "fp32":
        for k in ("Whh", "Wp", "Wh"):
            c[k] = c[k].float()
    return c


@functools.lru_cache(maxsize=None)
def reference(name, weights):
    """The host routine's results of a case (never modified by a test)."""
    from indic_cl_asr_amd import decoding as D
    W, a = CASES[name][5], CASES[name][9]
    return D.beam_rnnt_alsd_host(case_for(name, weights), W, a, True, ROUNDING[weights])


def figures(results):
    return dict(utterances=len(results), undecided=sum(not r["decided"] for r in results),
                recombinations=sum(r["recombinations"] for r in results), finished=sum(r["n_finished"] > 0 for r in results),
                slack_max=max((max(r["slack"], default=0.0) for r in results), default=0.0),
                steps=sum(r["steps"] for r in results))


def check_conditions(name, results):
    """What keeps `decided` from hiding a failure, asserted on the reference alone."""
    f = figures(results)
    assert 4 * f["undecided"] <= f["utterances"], (name, f)
    if CASES[name][10]:
        assert f["recombinations"] >= 1 or CASES[name][5] == 1, (name, f)      # a beam of one member never holds a duplicate
        assert 2 * f["finished"] >= f["utterances"], (name, f)
    return f


def assert_matches(name, ref, got, K):
    """`got` (alsd_unpack of the kernel's result, the first K of every list) against the reference: for a decided utterance the
    same sequences, order, alignment steps and finished count, every score within its slack + 2^-20 max(1, |score|)."""
    assert len(ref) == len(got)
    for b, (r, g) in enumerate(zip(ref, got)):
        if not r["decided"]:
            continue
        want = r["hyps"][:K]
        assert g["n_finished"] == r["n_finished"], (name, b, g["n_finished"], r["n_finished"])
        assert [h[0] for h in g["hyps"]] == [h[0] for h in want], (name, b)
        assert [h[2] for h in g["hyps"]] == [h[2] for h in want], (name, b)
        for (_, s, _), (_, e, _), slack in zip(g["hyps"], want, r["slack"]):
            assert abs(s - e) <= slack + 2.0 ** -20 * max(1.0, abs(e)), (name, b, s, e, slack)
