"""GEM on the host: EpisodicMemory.sample(language=...) and the float64 yardstick tests/test_gem_gpu.py holds ia_gem_solve to.

`enumerate_qp` solves  min 1/2 v'Pv + d'v  subject to  v >= gamma  exactly in the sense of an active-set method with nothing
left to chance: for every subset F of free coordinates it fixes the others at gamma, solves P_FF v_F = -(d_F + P_FB gamma) in
float64 and keeps the candidate that satisfies the KKT conditions (v_F > gamma, lambda_B = (Pv + d)_B >= 0).  P is positive
definite, so the program has one solution and exactly the candidates of that solution's faces pass; 2^K subsets, K <= 5 in the
tests.  `kkt_residuals` measures a candidate against the same conditions; the last test checks the enumerator with it on a
hand-made 3-constraint case whose solution is known in closed form."""
import itertools

import pytest
import torch

from test_episodic_memory import LANGS, fill, make_batch, same_batch


def enumerate_qp(P, d, gamma):
    """P [K, K] float64 positive definite, d [K] float64 -> (v, free mask) of the one KKT point."""
    K = d.numel()
    best = None
    for bits in itertools.product((False, True), repeat=K):
        free = torch.tensor(bits)
        v = torch.full((K,), float(gamma), dtype=torch.float64)
        if free.any():
            rhs = -(d[free] + P[free][:, ~free] @ v[~free])
            v[free] = torch.linalg.solve(P[free][:, free], rhs)
        lam = P @ v + d
        if bool((v[free] > gamma).all()) and bool((lam[~free] >= 0).all()):
            worst = float(lam[free].abs().max()) if free.any() else 0.0
            if best is None or worst < best[2]:
                best = (v, free, worst)
    assert best is not None, "no subset satisfies the KKT conditions: P is not positive definite?"
    return best[0], best[1]


def kkt_residuals(P, d, v, gamma):
    """(min(v - gamma), min(lambda), max |(v - gamma) * lambda|) in float64, lambda = Pv + d."""
    lam = P @ v + d
    return float((v - gamma).min()), float(lam.min()), float(((v - gamma) * lam).abs().max())


def test_sample_language_draws_only_that_language():
    from indic_cl_asr_amd import cl
    mem = cl.EpisodicMemory(per_language=3, seed=4)
    fill(mem)
    kept = {lang: [(x.clone(), t.clone()) for x, t in items] for lang, items in mem.state_dict()["items"].items()}
    for lang in ("hi", "ta", "bn"):
        (sig, sl, tok, tl), ids = mem.sample(7, language=lang)
        assert ids == [lang] * 7 and sig.shape[0] == 7
        for i in range(7):
            x, t = sig[i, :int(sl[i])], tok[i, :int(tl[i])]
            assert any(torch.equal(x, kx) and torch.equal(t, kt) for kx, kt in kept[lang]), (lang, i)
    (sig, *_), ids = mem.sample(40, language="hi")
    assert set(ids) == {"hi"}


def test_sample_default_sequence_is_unchanged():
    from indic_cl_asr_amd import cl
    a, b = cl.EpisodicMemory(3, seed=9), cl.EpisodicMemory(3, seed=9)
    fill(a); fill(b)
    for n in (1, 5, 8):
        assert same_batch(a.sample(n), b.sample(n, language=None))
    # a per-language draw consumes the generator exactly as a mixed draw of the same size does: the sequences stay in step
    a.sample(4)
    b.sample(4, language="ta")
    assert same_batch(a.sample(6), b.sample(6))
    assert sorted(set(a.sample(64)[1])) == ["bn", "hi", "ta"]


def test_sample_unknown_language_raises():
    from indic_cl_asr_amd import cl
    mem = cl.EpisodicMemory(2, seed=0)
    mem.add(make_batch(0), LANGS)
    state = mem.gen.get_state()
    with pytest.raises(ValueError, match="te"):
        mem.sample(2, language="te")
    assert torch.equal(mem.gen.get_state(), state)                  # the refusal drew nothing
    with pytest.raises(ValueError):
        cl.EpisodicMemory(2, seed=0).sample(1, language="hi")


def test_enumerator_satisfies_kkt_on_a_known_case():
    # P = diag(2, 1, 4) + a coupling between the first two; d pulls v0 up strongly, v1 slightly, pushes v2 down
    P = torch.tensor([[2.0, 0.5, 0.0], [0.5, 1.0, 0.0], [0.0, 0.0, 4.0]], dtype=torch.float64)
    d = torch.tensor([-3.0, 0.1, 1.0], dtype=torch.float64)
    gamma = 0.5
    v, free = enumerate_qp(P, d, gamma)
    # by hand: v2 sits at the bound (lambda_2 = 4 * 0.5 + 1 = 3 > 0); with v1 at the bound 2 v0 + 0.25 - 3 = 0 gives
    # v0 = 1.375 and lambda_1 = 0.5 * 1.375 + 0.5 + 0.1 = 1.2875 > 0: the solution is (1.375, 0.5, 0.5) with only v0 free
    assert free.tolist() == [True, False, False]
    assert torch.allclose(v, torch.tensor([1.375, 0.5, 0.5], dtype=torch.float64), rtol=0, atol=1e-14)
    lo, lam_min, comp = kkt_residuals(P, d, v, gamma)
    assert lo >= 0.0 and lam_min >= -1e-14 and comp <= 1e-14
    # the yardstick tells a wrong answer from the right one: the unconstrained minimiser violates the bound on v2
    u = torch.linalg.solve(P, -d)
    assert kkt_residuals(P, d, u, gamma)[0] < 0
    # gamma = 0 with nothing pulling up: every coordinate at the bound
    v0, free0 = enumerate_qp(P, d.abs(), 0.0)
    assert not free0.any() and not v0.any()
