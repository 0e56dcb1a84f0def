"""cl.EpisodicMemory on the host: per-language reservoirs, seeded draws, utterances kept without their padding and re-padded by
data.speech_collate's rules, and a state that resumes the same sequence of draws (also through checkpoint.save_memory)."""
import pytest
import torch


def make_batch(seed, B=4, L=64, U=6):
    """A padded training batch whose padding is NOT zero / pad_id, so that padding surviving add() would show."""
    g = torch.Generator().manual_seed(seed)
    sl = torch.tensor([L] + [int(torch.randint(8, L, (1,), generator=g)) for _ in range(B - 1)])
    tl = torch.tensor([U] + [int(torch.randint(1, U + 1, (1,), generator=g)) for _ in range(B - 1)])
    sig = torch.randn(B, L, generator=g)
    tok = torch.randint(1, 16, (B, U), generator=g)
    for i in range(B):
        sig[i, sl[i]:] = 7.0
        tok[i, tl[i]:] = 99
    return sig, sl, tok, tl


def utterances(batch):
    sig, sl, tok, tl = batch
    return [(sig[i, :int(sl[i])].clone(), tok[i, :int(tl[i])].clone()) for i in range(sig.shape[0])]


LANGS = ["hi", "ta", "hi", "bn"]


def fill(mem, seeds=range(6)):
    added = []
    for s in seeds:
        b = make_batch(s)
        mem.add(b, LANGS)
        added += utterances(b)
    return added


def stored(mem):
    return {lang: [(x.clone(), t.clone()) for x, t in kept] for lang, kept in mem.state_dict()["items"].items()}


def same_batch(a, b):
    return a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))


def test_reservoir_is_capped_per_language():
    from indic_cl_asr_amd import cl
    mem = cl.EpisodicMemory(per_language=3, seed=0)
    assert len(mem) == 0 and mem.languages() == []
    for s in range(6):
        mem.add(make_batch(s), LANGS)
        items = stored(mem)
        assert all(len(v) <= 3 for v in items.values())
    # 12 `hi`, 6 `ta`, 6 `bn` utterances offered: every language is full, and the cap is its own
    assert {k: len(v) for k, v in stored(mem).items()} == {"hi": 3, "ta": 3, "bn": 3}
    assert len(mem) == 9 and sorted(mem.languages()) == ["bn", "hi", "ta"]
    small = cl.EpisodicMemory(per_language=8, seed=0)
    small.add(make_batch(0), LANGS)
    assert {k: len(v) for k, v in stored(small).items()} == {"hi": 2, "ta": 1, "bn": 1}
    with pytest.raises(ValueError):
        cl.EpisodicMemory(per_language=0)


def test_same_seed_same_memory_and_same_draws():
    from indic_cl_asr_amd import cl
    a, b = cl.EpisodicMemory(2, seed=5), cl.EpisodicMemory(2, seed=5)
    fill(a); fill(b)
    ia, ib = stored(a), stored(b)
    assert ia.keys() == ib.keys()
    for lang in ia:
        assert all(torch.equal(x, y) and torch.equal(t, u) for (x, t), (y, u) in zip(ia[lang], ib[lang]))
    draws = [(a.sample(4), b.sample(4)) for _ in range(3)]
    assert all(same_batch(x, y) for x, y in draws)
    c = cl.EpisodicMemory(2, seed=6)
    fill(c)
    assert not all(same_batch(c.sample(4), x) for x, _ in draws)       # another seed: another sequence


def test_samples_are_added_utterances_without_their_padding():
    from indic_cl_asr_amd import cl, data
    mem = cl.EpisodicMemory(3, seed=1)
    added = fill(mem)
    for x, t in (u for kept in stored(mem).values() for u in kept):
        assert not (x == 7.0).any() and not (t == 99).any()
    seen_langs = set()
    for _ in range(4):
        (sig, sl, tok, tl), langs = mem.sample(5)
        assert sig.dtype == torch.float32 and sl.dtype == tok.dtype == tl.dtype == torch.long and len(langs) == 5
        assert sig.shape == (5, int(sl.max())) and tok.shape == (5, max(1, int(tl.max())))
        seen_langs |= set(langs)
        samples = []
        for i in range(5):
            n, m = int(sl[i]), int(tl[i])
            hits = [k for k, (x, t) in enumerate(added) if x.shape[0] == n and torch.equal(x, sig[i, :n]) and torch.equal(t, tok[i, :m])]
            assert hits, i
            assert all(LANGS[k % 4] == langs[i] for k in hits)
            assert not sig[i, n:].any() and not tok[i, m:].any()     # speech_collate: zeros and pad_id 0
            samples.append((sig[i, :n], sl[i], tok[i, :m], tl[i]))
        again = data.speech_collate(samples)
        assert all(torch.equal(p, q) for p, q in zip(again, (sig, sl, tok, tl)))
    assert len(seen_langs) > 1                                         # one batch may mix languages


def test_state_dict_continues_the_sequence(tmp_path):
    from indic_cl_asr_amd import checkpoint, cl
    a = cl.EpisodicMemory(2, seed=3)
    fill(a, range(3))
    a.sample(4)
    sd = a.state_dict()
    assert torch.is_tensor(sd["generator"]) and isinstance(sd["items"], dict) and isinstance(sd["seen"], dict)
    b = cl.EpisodicMemory(7, seed=99)
    b.load_state_dict(sd)
    checkpoint.save_memory(a, tmp_path / "memory.pt")
    c = checkpoint.load_memory(cl.EpisodicMemory(1), tmp_path / "memory.pt")
    assert b.per_language == c.per_language == 2 and len(b) == len(c) == len(a)
    first = a.sample(4)
    assert same_batch(first, b.sample(4)) and same_batch(first, c.sample(4))
    # the reservoirs go on identically too: further adds replace the same slots, further draws agree
    for m in (a, b, c):
        fill(m, range(3, 6))
    ia, ib, ic = stored(a), stored(b), stored(c)
    for lang in ia:
        for (x, t), (y, u), (z, w) in zip(ia[lang], ib[lang], ic[lang]):
            assert torch.equal(x, y) and torch.equal(t, u) and torch.equal(x, z) and torch.equal(t, w)
    last = a.sample(3)
    assert same_batch(last, b.sample(3)) and same_batch(last, c.sample(3))


def test_sample_on_an_empty_memory_raises():
    from indic_cl_asr_amd import cl
    with pytest.raises(ValueError):
        cl.EpisodicMemory(2).sample(1)
