"""CTC forced alignment of long transcripts, the parts that need no GPU: the host routine against the long golden cases
recorded from the reference's aligner, the ia_ctc_align_long* entry points' limit, workspace size and argument refusals."""
import ctypes

import numpy as np
import pytest
import torch

from ctc_align_fixture import assert_case, make_batch
from ctc_align_long_fixture import load_long_cases

NAMES = ["random_T328_S256", "repeats_T754_S512", "coarse_T1400_S1023", "random_T2342_S2047", "repeats_T5831_S4096", "below_min"]


def test_fixture_holds_the_cases():
    cases = load_long_cases()
    assert [c["name"] for c in cases] == NAMES and all(c["V"] == 9 for c in cases)
    assert [len(c["y"]) for c in cases] == [256, 512, 1023, 2047, 4096, 600]
    assert [c["lp"].shape[0] for c in cases[:5]] == [328, 754, 1400, 2342, 5831]
    assert cases[5]["path"] is None and all(c["path"] is not None for c in cases[:5])


@pytest.mark.parametrize("logits_mode", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_host_routine_reproduces_the_long_fixture(name, logits_mode):
    """Exact: every partial sum is an integer number of grid units below 2^24 (see the fixture script)."""
    from indic_cl_asr_amd import align as A
    c = next(c for c in load_long_cases() if c["name"] == name)
    x, lse, tg, il, tl = make_batch([c], logits_mode)
    path, spans, score = A.ctc_forced_align_host(x, il, tg, tl, c["blank"], lse=lse)
    assert_case(c, path[0].numpy(), spans[0].numpy(), float(score[0]))


def test_entry_points_limit_and_workspace():
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    for name in ("ia_ctc_align_long_max_targets", "ia_ctc_align_long_workspace_bytes", "ia_ctc_align_long"):
        assert hasattr(L, name), name
    limit = L.ia_ctc_align_long_max_targets()
    assert limit >= 8191 and (limit + 1) & limit == 0                        # 2^k - 1
    ws = L.ia_ctc_align_long_workspace_bytes
    assert ws(0, 5, 2) == 0 and ws(1, 0, 2) == 0 and ws(1, 5, -1) == 0 and ws(1, 5, limit + 1) == 0
    for B, T, S in ((1, 5, 256), (1, 45000, limit)):
        n = ws(B, T, S)
        assert n > 0 and n % 256 == 0 and n >= T * ((2 * S + 1 + 3) // 4), (B, T, S, n)      # 2 bits per state and frame
    assert ws(1, 5, 0) > 0 and ws(3, 7, 255) >= 3 * ws(1, 7, 255) - 2 * 255


def test_entry_point_refuses_bad_arguments_before_device_work():
    """Every call below is refused before any device work: the pointers are never dereferenced.  The checks and their order
    are ia_ctc_align's."""
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    limit = L.ia_ctc_align_long_max_targets()
    # lp, lse, targets, input_lens, target_lens, path, spans, score, workspace
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(9)]
    B, T, V, S = 2, 10, 17, 300
    need = L.ia_ctc_align_long_workspace_bytes(B, T, S)
    assert need > 0

    def call(ptrs=None, ld=V, B=B, T=T, V=V, S=S, blank=V - 1, nbytes=need):
        q = p if ptrs is None else ptrs
        return L.ia_ctc_align_long(q[0], ld, q[1], q[2], q[3], q[4], B, T, V, S, blank, q[5], q[6], q[7], q[8], nbytes, None)

    for i in (0, 2, 3, 4, 5, 6, 7, 8):                                              # (lse may be NULL: log-probs)
        q = list(p); q[i] = None
        assert call(q) == -1, i                                                      # IA_INVALID_VALUE: null pointers
    q = list(p); q[2] = None; q[6] = None
    assert call(q, S=0, nbytes=0) == -2 and call(q, S=1, nbytes=0) == -1             # S = 0 needs neither targets nor spans
    q = list(p); q[8] = ctypes.c_void_p(4096 * 9 + 128)
    assert call(q) == -1                                                             # the workspace: 256 bytes
    assert call(ld=V - 1) == -1 and call(blank=V) == -1 and call(blank=-1) == -1
    assert call(B=0) == -1 and call(T=0) == -1 and call(V=0, ld=0) == -1 and call(S=-1) == -1
    assert call(S=limit + 1) == -4                                                   # IA_UNSUPPORTED
    assert call(nbytes=need - 1) == -2 and call(nbytes=0) == -2                      # IA_WORKSPACE_TOO_SMALL
    # the order of the checks: values, then the limit, then the workspace's pointer, then its size
    assert call(S=limit + 1, blank=V) == -1 and call(S=limit + 1, nbytes=0) == -4
    q = list(p); q[8] = None
    assert call(q, S=limit + 1) == -4 and call(q, nbytes=0) == -1


def test_ctc_forced_align_long_on_cpu_tensors_is_the_host_routine():
    from indic_cl_asr_amd import align as A
    g = torch.Generator().manual_seed(5)
    B, T, V, S = 2, 400, 17, 300
    x = torch.randn(B, T, V, generator=g).log_softmax(-1)
    tg = torch.randint(0, V - 1, (B, S), generator=g)
    il, tl = torch.tensor([T, T - 30]), torch.tensor([S - 10, S])
    got = A.ctc_forced_align_long(x, il, tg, tl, V - 1)
    ref = A.ctc_forced_align_host(x, il, tg, tl, V - 1)
    assert all(not a.is_cuda and a.dtype == r.dtype and torch.equal(a, r) for a, r in zip(got, ref))
    assert float(ref[2][0]) > -np.inf
    with pytest.raises(ValueError):
        A.ctc_forced_align_long(x, il, tg, tl, V)
    with pytest.raises(ValueError):
        A.ctc_forced_align_long(x[0], il, tg, tl, V - 1)
