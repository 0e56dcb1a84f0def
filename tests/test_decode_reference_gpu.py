"""csrc/greedy_decode.hip -- the fp32 GEMV loop, the bf16-weight GEMV loop and the MFMA head with clusters of 1, 2 and 4
workgroups per utterance -- held to the fp64 replay of oracle/decode_ref.py: every hypothesis a kernel returns must be a member of
the acceptable set of its rounding mode ("gemv" for the two GEMV loops, "mfma" for the MFMA head).  No utterance is left out and
no count of agreeing utterances is used.  The tolerance behind the set is derived in oracle/decode_ref.py (C = 4, FLOOR = 2^-20,
as tests/test_block_reference_gpu.py; nothing in it comes from a kernel's output), and the conditions that keep the set from
hiding a failure are asserted on the reference alone, before a kernel's output is looked at (tests/test_decode_reference.py
asserts the same on a machine without a GPU).

Figures of the reference per case, "mfma" / "gemv" (measurements of the reference, not limits taken from the kernels; the
three kernels and every cluster size return the reference's main-path hypothesis in every case, so there is one row per case):
  case          micro-steps  tokens     blank share   multi-candidate  median tol       largest tol      smallest margin
  medium        347 / 356    168 / 178  0.52 / 0.50   0 / 0            3.8e-6 / 3.7e-6  9.8e-4 / 6.3e-6  4.3e-4 / 1.1e-3
  second-group  207 / 206    149 / 147  0.28 / 0.29   0 / 0            1.9e-6 / 2.2e-6  3.2e-3 / 4.4e-6  2.1e-3 / 5.4e-4
  nks21         107 / 107    69 / 69    0.36 / 0.36   0 / 0            2.1e-6 / 2.1e-6  3.2e-4 / 3.4e-6  4.5e-4 / 8.2e-4
  small         169 / 170    64 / 65    0.62 / 0.62   0 / 0            2.5e-6 / 2.8e-6  1.6e-4 / 4.7e-6  2.8e-3 / 9.7e-4
  tile-edges    69 / 69      41 / 41    0.41 / 0.41   0 / 0            3.2e-6 / 3.5e-6  2.6e-3 / 5.1e-6  1.0e-3 / 6.1e-4
  one-frame     5 / 5        4 / 4      0.20 / 0.20   0 / 0            1.3e-6 / 1.7e-6  1.5e-6 / 2.1e-6  5.9e-3 / 6.4e-3
  lens          64 / 64      45 / 45    0.30 / 0.30   0 / 0            2.4e-6 / 2.8e-6  2.5e-4 / 3.9e-6  7.2e-4 / 4.3e-4
  all-blank     44 / 44      0 / 0      1 / 1         0 / 0            5.1e-5 / 5.1e-5  5.5e-5 / 5.4e-5  46 / 46
  never-blank   120 / 120    120 / 120  0 / 0         0 / 0            5.1e-5 / 5.1e-5  2.1e-4 / 5.6e-5  3.2e-3 / 3.2e-3
  tie8          112 / 112    83 / 83    0.26 / 0.26   0 / 0            1.6e-6 / 1.8e-6  1.1e-4 / 3.4e-6  2.1e-3 / 2.3e-3
  tie24         93 / 93      54 / 54    0.42 / 0.42   0 / 0            2.4e-6 / 2.7e-6  4.2e-6 / 4.3e-6  2.6e-2 / 2.7e-2
  tie8-b9       141 / 141    101 / 101  0.28 / 0.28   0 / 0            1.5e-6 / 1.8e-6  6.3e-5 / 3.5e-6  1.2e-2 / 1.2e-2
  tie24-b2      47 / 47      25 / 25    0.47 / 0.47   0 / 0            2.3e-6 / 2.6e-6  3.9e-6 / 4.6e-6  5.5e-3 / 5.1e-3
  model fp32    181          86         0.52          0                2.9e-6           4.8e-6           2.5e-3           ("gemv")
  model bf16    179          83         0.54          0                2.3e-6           1.4e-3           3.5e-4           ("mfma")
Every acceptable set of these cases holds exactly one sequence: the kernels are held to the fp64 hypothesis itself.  The largest
"mfma" tolerances are steps with a flippable element (one bf16 ulp of an activation times a head weight); the median is what the
fp32 summation of the head and FLOOR give.  The blank biases are tuned (on the reference alone) so that the conditions hold and,
in the cases of ROUNDING_VISIBLE, so that the two rounding modes decode different hypotheses.

"one-frame" (T = 1, B = 2) cannot meet the balance conditions: with one frame an utterance that starts with a blank makes one
decision, and one that reaches the cap of 4 makes four, so "a first blank", "a frame at the cap" and "a quarter of the decisions
blank" exclude each other, and no emission can come from frame j > 0 of a tile.  It asserts a first blank, a frame at the cap and
both kinds of decision instead.

Shapes: see CASES.  Exact ties, the output contract (sentinel-filled token matrix, a small cap, the launchers' refusals, the
cluster choice) and the model-level path (greedy_rnnt_decode_device / greedy_rnnt_decode on fp32 and bf16 models, deferred
results, a mixed-language batch, the decode after a fused optimizer step) follow the ABI cases.

Wrong-answer single-line faults, each built once and run once against this file (none indexes out of bounds, touches the
hand-off protocol or changes a loop's termination); B of the failing cases in brackets:
  s = (j == 0 ? s : 0) + 1 turned into s + 1 ......... NOT A FAULT: all 26 tests pass, and rightly.  The scan over the tile's frames
                                                      sets s = 0 at every blank it passes, so s is already 0 whenever j > 0:
                                                      the two expressions are equal on every path.  In its place:
  the cap test s >= max_symbols turned into s > ..... every ABI case but all-blank [11, 9, 8, 5, 3, 2, 4], all 8 tie tests, the
                                                      cap test, the three bf16 model tests
  first-blank restart from row_sos (all kernels) .... medium, second-group, nks21, small, tile-edges, lens [11, 9, 8, 5, 3, 4], the
                                                      4 first-maximum tie tests [4, 9, 2], the cap test, all 5 model tests; not
                                                      one-frame, where the utterance ends with its first blank
  c not committed on an emission (all kernels) ...... the same six and never-blank, 7 of the 8 tie tests, the cap test, all 5
                                                      model tests [11, 9, 8, 5, 3, 4, 2]
  tile reduction's tie rule oi < bi -> oi > bi ...... both tie tests of tie8 and tie8-b9 [4, 9] (copies in one tile); nothing else
                                                      holds an exact tie, as it should be
  ... the same rule in the GEMV loops' argmax ....... the first-maximum test of all four tie cases, blank-tied tie8 / tie8-b9 [4, 9, 2]
  cross-tile scan's > turned into >= ................ the first-maximum test of tie24 and tie24-b2 [4, 2] (copies in different tiles)
  bias added after the per-tile maximum, tile 1 ..... one-frame, never-blank, blank-tied tie24 [2, 4].  Tile 1 is labels 16..31: one
                                                      padded label at V = 17, absent at V = 16, a sixteenth of the labels at
                                                      V = 257, and the biases are a tenth of the logits' spread; the B = 11, 9, 8
                                                      and 3 cases have those V by their definition.  The same fault on tile 0:
                                                      second-group, nks21, small, never-blank, all 8 tie tests, the cap test,
                                                      the three bf16 model tests [9, 8, 5, 4, 2]
  vr clamped to V - 2 (the blank reads its neighbour) every ABI case but never-blank [11, 9, 8, 5, 3, 2, 4], the 4 first-maximum tie
                                                      tests, the cap test, the three bf16 model tests
  bf16 rounding of the activation dropped (the head
  on a hi + lo bf16 split of the fp32 activation) ... the ROUNDING_VISIBLE cases medium, second-group, small, lens [11, 9, 5, 4],
                                                      blank-tied tie24 / tie24-b2 [4, 2], the cap test, two bf16 model tests [5];
                                                      no decision of nks21, tile-edges or one-frame hinges on the rounding
"""
import functools

import pytest
import torch

from oracle import decode_ref as R
from test_greedy_decode_gpu import _bf16_case

pytestmark = pytest.mark.gpu

IA_INVALID_VALUE, IA_WORKSPACE_TOO_SMALL, IA_UNSUPPORTED = -1, -2, -4
SENTINEL = -7

#  name           B   T   Hp   Hj   V   max_symbols blank_bias lens               conditions    what it reaches
CASES = {
    "medium":       (11, 45, 640, 640, 257, 10, 3.0, None, "balanced"),            # B > 8, no multiple of 8; nks = 20; three frame tiles
    "second-group": (9, 33, 128, 64, 17, 2, 1.3, None, "balanced"),                # one utterance in the second id group; V = 17: a
                                                                                   # 1-label last tile, the vr clamp; nks = 2; cap of 2
    "nks21":        (8, 17, 64, 672, 16, 1, 1.0, None, "balanced"),                # a third fragment group of one with the ks clamp; V = 16;
                                                                                   # cap of 1; len - t = 1 in the second tile
    "small":        (5, 37, 64, 96, 33, 3, 2.2, None, "balanced"),                 # Hp / 4 = 16 units per workgroup
    "tile-edges":   (3, 16, 128, 64, 257, 10, 2.5, (16, 15, 1), "balanced"),       # exactly one tile, one frame short, one frame
    "one-frame":    (2, 1, 64, 64, 33, 4, 0.5, None, "one-frame"),                 # T = 1
    "lens":         (4, 20, 64, 64, 40, 2, 1.2, (20, 0, -3, 25), "balanced"),      # empty, negative and too long
    "all-blank":    (3, 20, 128, 64, 17, 10, 50.0, None, "extreme"),
    "never-blank":  (4, 18, 64, 64, 40, 2, -50.0, None, "extreme"),
    # the bases of the exact-tie constructions (V0 labels + blank) and of the cap test
    "tie8":         (4, 20, 64, 64, 9, 3, 1.0, None, "balanced"),
    "tie24":        (4, 20, 64, 64, 25, 3, 0.75, None, "balanced"),
    "tie8-b9":      (9, 20, 64, 64, 9, 3, 0.5, None, "balanced"),                  # ... with an utterance in the second id group
    "tie24-b2":     (2, 20, 64, 64, 25, 3, 2.5, None, "balanced"),
}
TIES = ["tie8", "tie24", "tie8-b9", "tie24-b2"]
# cases in which a decision hinges on the bf16 rounding of the head's input: their "mfma" and "gemv" hypotheses differ, so a kernel
# that rounds where it should not (or the other way round) is outside its set.  No blank bias that meets the conditions gives
# "nks21", "tile-edges" or "one-frame" such a decision (their seeds are fixed by B and T).
ROUNDING_VISIBLE = ["medium", "second-group", "small", "lens"]


@functools.lru_cache(maxsize=None)
def make_case(name):
    B, T, Hp, Hj, V, ms, bias, lens, _ = CASES[name]
    return _bf16_case(B, T, Hp, Hj, V, seed=B * 100 + T, blank_bias=bias, lens=None if lens is None else torch.tensor(lens))


_REF = {}


def reference(key, case, ms, rounding, cap=None):
    """decode_reference, computed once per (case, rounding, cap) and shared by the tests; never modified."""
    k = (key, ms, rounding, cap)
    if k not in _REF:
        _REF[k] = R.decode_reference(case, ms, rounding, cap)
    return _REF[k]


def check_case_conditions(res, kind):
    if kind == "one-frame":
        s = R.check_conditions(res, balanced=False)
        assert s["first_blank"] >= 1 and s["cap_hits"] >= 1 and s["blank_share"] > 0 and s["label_share"] > 0, s
        return s
    return R.check_conditions(res, balanced=(kind == "balanced"))


# ----------------------------------------------------------------------------------------------------------- the C ABI
def run_kernel(kernel, case, ms, cluster=0, cap=None, scratch_bytes=None):
    """kernel: "f32" (ia_greedy_rnnt_decode on the widened images), "bf16w" (ia_greedy_rnnt_decode_bf16w) or "ex"
    (ia_greedy_rnnt_decode_bf16w_ex with `cluster`).  The token matrix is pre-filled with a sentinel, and entries at and behind
    counts[b] must come back untouched.  -> (status, hypotheses, overflow, counts)"""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    c = {k: v.cuda().contiguous() for k, v in case.items() if torch.is_tensor(v)}
    if kernel == "f32":
        for k in ("Whh", "Wp", "Wh"):
            c[k] = c[k].float().contiguous()
    B, T, Hj = c["f_all"].shape
    Hp, V = c["Whh"].shape[1], c["Wh"].shape[0]
    cap = T * ms if cap is None else cap
    tokens = torch.full((B, cap), SENTINEL, dtype=torch.int32, device="cuda")
    counts = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    args = (_lib.ptr(c["f_all"]), _lib.ptr(c["lens"]), _lib.ptr(c["EW"]), _lib.ptr(c["Whh"]), _lib.ptr(c["Wp"]), _lib.ptr(c["bp"]),
            _lib.ptr(c["Wh"]), _lib.ptr(c["bh"]), B, T, Hp, Hj, V, V - 1, V - 1, V, ms, _lib.ptr(tokens), cap, _lib.ptr(counts),
            _lib.ptr(ovf))
    if kernel == "f32":
        st = L.ia_greedy_rnnt_decode(*args, _lib.stream_ptr())
    elif kernel == "bf16w":
        st = L.ia_greedy_rnnt_decode_bf16w(*args, _lib.stream_ptr())
    else:
        n = int(L.ia_greedy_decode_scratch_bytes(B, Hp, Hj)) if scratch_bytes is None else scratch_bytes
        scratch = torch.empty(max(n, 16), dtype=torch.uint8, device="cuda")
        st = L.ia_greedy_rnnt_decode_bf16w_ex(*args, cluster, _lib.ptr(scratch), n, _lib.stream_ptr())
    torch.cuda.synchronize()
    tk, n = tokens.cpu(), counts.cpu().tolist()
    if st != 0:
        assert bool((tk == SENTINEL).all()) and all(v == SENTINEL for v in n) and int(ovf.item()) == 0, "a refused call wrote"
        return st, None, 0, n
    assert all(0 <= n[b] <= cap for b in range(B)), n
    for b in range(B):
        assert bool((tk[b, n[b]:] == SENTINEL).all()), ("entries behind counts[b] were written", b, n[b])
        assert bool(((tk[b, :n[b]] >= 0) & (tk[b, :n[b]] < V)).all()), ("a token outside [0, V)", b)
    return 0, [tk[b, :n[b]].tolist() for b in range(B)], int(ovf.item()), n


def clusters_for(case):
    Hp, Hj = case["Whh"].shape[1], case["Wh"].shape[1]
    return [nw for nw in (1, 2, 4) if Hj % 32 == 0 and Hp % (8 * nw) == 0 and Hj % (4 * nw) == 0]


def all_kernels(case, ms, cap=None):
    """Every kernel on one case -> {label: (hypotheses, overflow, rounding mode)}; the clusters agree exactly."""
    out = {}
    for kernel in ("f32", "bf16w"):
        st, hyp, ovf, _ = run_kernel(kernel, case, ms, cap=cap)
        assert st == 0, (kernel, st)
        out[kernel] = (hyp, ovf, "gemv" if kernel == "f32" or not clusters_for(case) else "mfma")
    for nw in [0] + clusters_for(case):
        st, hyp, ovf, _ = run_kernel("ex", case, ms, cluster=nw, cap=cap)
        assert st == 0, (nw, st)
        out[f"ex{nw}"] = (hyp, ovf, "gemv" if nw == 0 else "mfma")
    for nw in clusters_for(case):
        assert out[f"ex{nw}"][0] == out["ex1"][0], ("clusters disagree", nw)      # the same dot products, whoever computes them
    if clusters_for(case):
        assert out["bf16w"][0] == out["ex1"][0]
    return out


def assert_members(got, refs, what):
    for label, (hyp, ovf, mode) in got.items():
        bad = [b for b in range(len(hyp)) if not R.member(hyp[b], refs[mode][b])]
        assert not bad, (what, label, mode, "utterances outside their acceptable set", bad,
                         [(hyp[b], sorted(refs[mode][b]["accept"])) for b in bad[:2]])


@pytest.mark.parametrize("name", ["medium", "second-group", "nks21", "small", "tile-edges", "one-frame", "lens", "all-blank",
                                  "never-blank"])
def test_every_kernel_decodes_a_member_of_the_acceptable_set(name):
    B, T, Hp, Hj, V, ms, bias, lens, kind = CASES[name]
    case = make_case(name)
    refs = {}
    for mode in ("mfma", "gemv"):
        refs[mode] = reference(name, case, ms, mode)
        s = check_case_conditions(refs[mode], kind)                 # on the reference alone, before any kernel output
        print(name, mode, {k: (float(f"{v:.3g}") if isinstance(v, float) else v) for k, v in s.items()})
    if name in ROUNDING_VISIBLE:
        assert [r["hyp"] for r in refs["mfma"]] != [r["hyp"] for r in refs["gemv"]]
    got = all_kernels(case, ms)
    assert len(got) == 3 + len(clusters_for(case)) and len(clusters_for(case)) == 3
    assert all(ovf == 0 for _, ovf, _ in got.values())
    assert_members(got, refs, name)
    L = case["lens"].clamp(0, T).tolist()
    for label, (hyp, _, mode) in got.items():
        if name == "all-blank":
            assert all(h == [] for h in hyp), label
        if name == "never-blank":
            assert [len(h) for h in hyp] == [ms * l for l in L], label
        if name == "lens":
            assert hyp[1] == [] and hyp[2] == [], label
            assert max(s["frame"] for s in refs[mode][3]["steps"]) == T - 1         # the too-long one decodes T frames


# ---------------------------------------------------------------------------------------------------------- exact ties
def _tie_case(name):
    """Head rows [A; A; blank] with equal biases: labels v and v + V0 are bit-identical, the first maximum is always < V0."""
    base = make_case(name)
    V0 = base["Wh"].shape[0] - 1
    c = dict(base)
    c["Wh"] = torch.cat([base["Wh"][:V0], base["Wh"][:V0], base["Wh"][V0:]], 0).contiguous()
    c["bh"] = torch.cat([base["bh"][:V0], base["bh"][:V0], base["bh"][V0:]], 0).contiguous()
    c["EW"] = torch.cat([base["EW"][:V0], base["EW"][:V0], base["EW"][V0:]], 0).contiguous()     # labels, copies, blank row, SOS row
    return c, V0


@pytest.mark.parametrize("name", TIES)        # V0 = 8: both copies in one 16-label tile; V0 = 24, V = 49: in different tiles
def test_exact_ties_take_the_first_maximum(name):
    ms = CASES[name][5]
    base = make_case(name)
    refs = {mode: reference(name, base, ms, mode) for mode in ("mfma", "gemv")}     # the rows masked to one copy
    for mode in refs:
        check_case_conditions(refs[mode], "balanced")
    tied, V0 = _tie_case(name)
    got = all_kernels(tied, ms)
    for label, (hyp, ovf, _) in got.items():
        assert ovf == 0
        assert all(k < V0 for h in hyp for k in h), (label, "a later copy of a tied label won")
    assert sum(len(h) for h in got["ex1"][0]) > 0
    assert_members(got, refs, name)


@pytest.mark.parametrize("name", TIES)
def test_a_blank_tied_with_label_0_never_wins(name):
    B, T, Hp, Hj, V, ms = CASES[name][:6]
    base = make_case(name)
    c = dict(base)
    c["Wh"] = base["Wh"].clone(); c["bh"] = base["bh"].clone()
    c["Wh"][V - 1] = base["Wh"][0]; c["bh"][V - 1] = base["bh"][0]
    never = dict(c)
    never["bh"] = c["bh"].clone(); never["bh"][V - 1] = -50.0                         # the same labels with a blank that cannot win
    refs = {mode: reference(name + "-never", never, ms, mode) for mode in ("mfma", "gemv")}
    for mode in refs:
        check_case_conditions(refs[mode], "extreme")
        assert all(len(r["hyp"]) == ms * int(l) for r, l in zip(refs[mode], base["lens"]))
    got = all_kernels(c, ms)
    for label, (hyp, ovf, _) in got.items():
        assert ovf == 0 and [len(h) for h in hyp] == [ms * int(l) for l in base["lens"]], label
    assert_members(got, refs, name)


# ----------------------------------------------------------------------------------------------------- output contract
def test_a_small_cap_sets_the_overflow_bit_and_truncates_only_the_long_utterances():
    name = "small"
    ms = CASES[name][5]
    case = make_case(name)
    full = reference(name, case, ms, "mfma")
    n = sorted(len(r["hyp"]) for r in full)
    cap = n[len(n) // 2]                                   # the median length: some utterances overflow, the others fit
    assert n[0] <= cap < n[-1]
    refs = {mode: reference(name, case, ms, mode, cap) for mode in ("mfma", "gemv")}
    for mode in refs:
        check_case_conditions(refs[mode], "extreme")
    got = all_kernels(case, ms, cap=cap)
    for label, (hyp, ovf, mode) in got.items():
        assert ovf == 1, label
        for b, r in enumerate(refs[mode]):
            if r["counts"]["overflow"]:
                assert len(hyp[b]) == cap, (label, b)
            else:                                          # unaffected: the hypothesis of the uncapped run
                assert tuple(hyp[b]) in reference(name, case, ms, mode)[b]["accept"], (label, b)
    assert_members(got, refs, "cap")                       # the first `cap` tokens are the prefix of an acceptable sequence


def _refusal_case(Hp, Hj, V=17, B=2, T=4):
    """Operands of the stated dimensions, zero-filled (nothing is launched; were a refusal missing, zeros decode harmlessly)."""
    return dict(f_all=torch.zeros(B, T, Hj), EW=torch.zeros(V + 1, 4 * Hp), Whh=torch.zeros(4 * Hp, Hp).bfloat16(),
                Wp=torch.zeros(Hj, Hp).bfloat16(), bp=torch.zeros(Hj), Wh=torch.zeros(V, Hj).bfloat16(), bh=torch.zeros(V),
                lens=torch.full((B,), T, dtype=torch.long))


def test_the_launchers_refuse_without_launching():
    assert run_kernel("f32", _refusal_case(66, 64), 2)[0] == IA_UNSUPPORTED                          # Hp % 4
    assert run_kernel("ex", _refusal_case(68, 64), 2, cluster=0)[0] == IA_UNSUPPORTED                # bf16 with Hp % 8
    assert run_kernel("bf16w", _refusal_case(68, 64), 2)[0] == IA_UNSUPPORTED
    assert run_kernel("ex", _refusal_case(64, 64), 2, cluster=9)[0] == IA_INVALID_VALUE              # cluster > 8
    assert run_kernel("ex", _refusal_case(64, 64), 2, cluster=-1)[0] == IA_INVALID_VALUE
    assert run_kernel("ex", _refusal_case(64, 80), 2, cluster=1)[0] == IA_UNSUPPORTED                # cluster with Hj % 32
    assert run_kernel("ex", _refusal_case(64, 64), 2, cluster=3)[0] == IA_UNSUPPORTED                # Hp % (8 cluster)
    assert run_kernel("ex", _refusal_case(64, 4096), 2, cluster=1)[0] == IA_UNSUPPORTED              # the MFMA kernel's LDS: 165 440 B
    assert run_kernel("ex", _refusal_case(64, 4096), 2, cluster=0)[0] == 0                           # ... the GEMV loop's fits
    c = _refusal_case(64, 64)
    for nw in (2, 4):                                                                                # scratch too small for a cluster
        from indic_cl_asr_amd import _lib
        need = int(_lib.lib().ia_greedy_decode_scratch_bytes(2, 64, 64))
        assert need == 2 * 256 + 2 * 128 * 4
        assert run_kernel("ex", c, 2, cluster=nw, scratch_bytes=need - 1)[0] == IA_WORKSPACE_TOO_SMALL
        assert run_kernel("ex", c, 2, cluster=nw, scratch_bytes=0)[0] == IA_WORKSPACE_TOO_SMALL
    assert run_kernel("ex", c, 2, cluster=1, scratch_bytes=0)[0] == 0                                # none needed for one workgroup
    for kernel in ("f32", "bf16w", "ex"):
        assert run_kernel(kernel, c, 0, cluster=1, cap=8)[0] == IA_INVALID_VALUE                     # max_symbols = 0


def _launch_raw(Hp, Hj, V=17, B=2, T=4, shift=None, lds_case=False):
    """ia_greedy_rnnt_decode / _bf16w_ex on raw pointers: one operand `shift`ed by 4 bytes, or the LDS-limit dimensions."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    big = torch.zeros(1 << 20, dtype=torch.float32, device="cuda")             # every operand points into zeros
    lens = torch.full((B,), T, dtype=torch.long, device="cuda")
    tokens = torch.full((B, 8), SENTINEL, dtype=torch.int32, device="cuda")
    counts = torch.full((B,), SENTINEL, dtype=torch.int32, device="cuda")
    ovf = torch.zeros(1, dtype=torch.int32, device="cuda")
    import ctypes
    p = {k: big.data_ptr() for k in ("f_all", "EW", "Whh", "Wp", "Wh")}
    if shift:
        p[shift] += 4
    vp = ctypes.c_void_p
    st = L.ia_greedy_rnnt_decode(vp(p["f_all"]), _lib.ptr(lens), vp(p["EW"]), vp(p["Whh"]), vp(p["Wp"]), _lib.ptr(big), vp(p["Wh"]),
                                 _lib.ptr(big), B, T, Hp, Hj, V, V - 1, V - 1, V, 2, _lib.ptr(tokens), 8, _lib.ptr(counts), _lib.ptr(ovf),
                                 _lib.stream_ptr())
    torch.cuda.synchronize()
    assert bool((tokens == SENTINEL).all()) and bool((counts == SENTINEL).all()) and int(ovf.item()) == 0
    return st


def test_misaligned_operands_and_the_lds_limit_are_refused():
    for k in ("f_all", "EW", "Whh", "Wp", "Wh"):
        assert _launch_raw(64, 64, shift=k) == IA_INVALID_VALUE, k
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    assert int(L.ia_greedy_decode_lds_bytes(5096, 64, 17)) == (8 * 5096 + 128 + 17 + 16) * 4 <= 160 * 1024
    assert int(L.ia_greedy_decode_lds_bytes(5120, 64, 17)) > 160 * 1024
    assert _launch_raw(5120, 64) == IA_UNSUPPORTED                              # LDS above 160 KiB: refused before any launch
    assert int(L.ia_greedy_decode_lds_bytes(0, 64, 17)) == 0 and int(L.ia_greedy_decode_scratch_bytes(0, 64, 64)) == 0


def test_the_cluster_choice_at_its_edges(monkeypatch):
    from indic_cl_asr_amd import _lib
    f = lambda *a: int(_lib.lib().ia_greedy_decode_cluster(*a))
    monkeypatch.delenv("IA_DECODE_CLUSTER", raising=False)
    assert f(32, 640, 640) == 4 and f(1, 640, 640) == 4
    assert f(56, 640, 640) == 4 and f(57, 640, 640) == 4 and f(64, 640, 640) == 4      # 57 rounds up to 64 ids: 256 workgroups fit
    assert f(65, 640, 640) == 2 and f(128, 640, 640) == 2                                # 72 x 4 does not; 3 does not divide 640
    assert f(129, 640, 640) == 1 and f(1000, 640, 640) == 1
    assert f(8, 64, 64) == 4 and f(8, 72, 64) == 1 and f(8, 48, 96) == 3 and f(8, 16, 64) == 2 and f(8, 8, 32) == 1
    assert f(32, 640, 100) == 0 and f(32, 636, 640) == 0 and f(0, 640, 640) == 0 and f(8, 0, 64) == 0 and f(8, 64, 0) == 0
    monkeypatch.setenv("IA_DECODE_CLUSTER", "0")
    assert f(32, 640, 640) == 0
    monkeypatch.setenv("IA_DECODE_CLUSTER", "2")
    assert f(32, 640, 640) == 2 and f(129, 640, 640) == 1
    monkeypatch.setenv("IA_DECODE_CLUSTER", "16")                                        # clamped to 8
    assert f(8, 640, 640) == 8 and f(32, 640, 640) == 8 and f(33, 640, 640) == 5         # 40 x 8 > 256; 7, 6 do not divide; 5 does
    monkeypatch.setenv("IA_DECODE_CLUSTER", "1")
    assert f(32, 640, 640) == 1


# --------------------------------------------------------------------------------------------------------- model level
MODEL_KW = dict(d_model=64, n_layers=2, n_heads=4, pred_hidden=64, joint_hidden=64, languages=['hi', 'ta'], vocab_per_lang=16,
                fused_batch_size=2)
MODEL_BIAS = {"hi": 2.0, "ta": 1.5}
MODEL_MS = 3


def make_model(compute_dtype, seed=0):
    """A tiny model on the CPU whose heads emit blanks and labels in comparable numbers, the blank / padding embedding row made
    non-zero so that the restart after a first blank is visible."""
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(seed)
    m = EncDecHybridRNNTCTCModel(model_config('tiny', compute_dtype=compute_dtype, dither=0.0, **MODEL_KW)).eval()
    g = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        m.decoder.prediction["embed"].weight[m.decoder.blank_idx] = torch.randn(MODEL_KW["pred_hidden"], generator=g)
        for lang, bias in MODEL_BIAS.items():
            head = m.joint.joint_net[-1][lang]
            head.weight.mul_(3.0)
            head.bias[-1] += bias
    return m


def model_inputs(B=5, T=37, seed=5):
    g = torch.Generator().manual_seed(seed)
    enc = torch.randn(B, MODEL_KW["d_model"], T, generator=g)
    lens = torch.tensor([T, T - 7, 1, T // 2, T - 1][:B])
    return enc, lens


def model_rounding(case):
    Hp, Hj = case["Whh"].shape[1], case["Wh"].shape[1]
    return "mfma" if case["bf16"] and Hj % 32 == 0 and Hp % 8 == 0 else "gemv"


@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_model_level_decode_is_acceptable_for_the_models_own_operands(compute_dtype, monkeypatch):
    from indic_cl_asr_amd import decoding as D
    monkeypatch.delenv("IA_DECODE_CLUSTER", raising=False)
    m = make_model(compute_dtype)
    enc, lens = model_inputs()
    case = R.case_from_model(m, enc, lens, 'hi')
    assert case["bf16"] == (compute_dtype == "bf16")
    ref = R.decode_reference(case, MODEL_MS, model_rounding(case))
    print(compute_dtype, check_case_conditions(ref, "balanced"))
    m = m.cuda()
    enc, lens = enc.cuda(), lens.cuda()
    B = enc.shape[0]
    dev = D.greedy_rnnt_decode_device(m, enc, lens, ['hi'] * B, MODEL_MS)
    bad = [b for b in range(B) if not R.member(dev[b], ref[b])]
    assert not bad, (bad, [(dev[b], sorted(ref[b]["accept"])) for b in bad[:2]])
    assert D.greedy_rnnt_decode(m, enc, lens, ['hi'] * B, MODEL_MS) == dev                    # the dispatching entry
    pend = D.greedy_rnnt_decode_device(m, enc, lens, ['hi'] * B, MODEL_MS, defer=True)
    assert isinstance(pend, D.PendingHyps) and pend.result() == dev and pend.result() == dev


@pytest.mark.parametrize("compute_dtype", ["fp32", "bf16"])
def test_mixed_language_batch_decodes_each_utterance_through_its_own_head(compute_dtype):
    from indic_cl_asr_amd import decoding as D
    m = make_model(compute_dtype)
    enc, lens = model_inputs(B=4, seed=6)
    langs = ['hi', 'ta', 'ta', 'hi']
    refs = []
    for i, lang in enumerate(langs):
        case = R.case_from_model(m, enc[i:i + 1], lens[i:i + 1], lang)
        refs.append(R.decode_reference(case, MODEL_MS, model_rounding(case))[0])
    assert R.summarize(refs)["sets_gt1"] == 0 and R.summarize(refs)["multi"] == 0
    assert refs[0]["hyp"] != R.decode_reference(R.case_from_model(m, enc[:1], lens[:1], 'ta'), MODEL_MS, None)[0]["hyp"]   # the heads differ
    m = m.cuda()
    hyp = D.greedy_rnnt_decode(m, enc.cuda(), lens.cuda(), langs, MODEL_MS)
    bad = [i for i in range(4) if not R.member(hyp[i], refs[i])]
    assert not bad, (bad, [(hyp[i], sorted(refs[i]["accept"])) for i in bad])
    assert sum(len(h) for h in hyp) > 0


def test_decode_after_a_fused_optimizer_step_uses_the_updated_weights():
    """bf16 model: the decode reads the bf16 images the fused optimizer keeps current.  After one step the hypotheses must be
    acceptable for the updated weights and not for the old ones (stale shadows, a pending update not flushed)."""
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd import decoding as D
    from test_optimizer_decode_gpu import _batch
    m = make_model("bf16")
    enc, lens = model_inputs()
    B = enc.shape[0]
    old = R.decode_reference(R.case_from_model(m, enc, lens, 'hi'), MODEL_MS, "mfma")
    m = m.disable_dropout().cuda().train(); m.spec_augment_enabled = False
    flat = cl.FlatParams(m)
    opt = cl.FusedAdamW(flat, lr=2e-2)
    before = D.greedy_rnnt_decode_device(m, enc.cuda(), lens.cuda(), ['hi'] * B, MODEL_MS)   # (also fills the shadow cache)
    assert all(R.member(h, r) for h, r in zip(before, old))
    opt.zero_grad()
    loss, _ = m.training_step(tuple(t.cuda() for t in _batch()), ['hi'] * 4)
    loss.backward(); opt.step()
    m.eval()
    after = D.greedy_rnnt_decode_device(m, enc.cuda(), lens.cuda(), ['hi'] * B, MODEL_MS)
    torch.cuda.synchronize()
    case = R.case_from_model(m, enc, lens, 'hi')
    new = R.decode_reference(case, MODEL_MS, "mfma")
    s = R.check_conditions(new, balanced=False)
    print("after the step", s)
    differ = [b for b in range(B) if not (new[b]["accept"] & old[b]["accept"])]
    assert len(differ) >= 2, "the step was too small: the acceptable sets before and after it overlap"
    bad = [b for b in range(B) if not R.member(after[b], new[b])]
    assert not bad, (bad, [(after[b], sorted(new[b]["accept"])) for b in bad[:2]])
    assert all(not R.member(after[b], old[b]) for b in differ)
