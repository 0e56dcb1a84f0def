"""Limited-context rel-pos attention (change_attention_model("rel_pos", [L, R], att_context_style=...),
ops.rel_pos_attention(context=...)) on the host.

The golden cases are outputs and autograd gradients of the reference's RelPositionMultiHeadAttention in fp64 under the mask of
ConformerEncoder._create_masks (tests/golden/make_limited_context_golden.py; linear_out = identity, so the stored output is the
attention context and a padded row is exactly zero).  The bounds are those of tests/test_local_attention.py (1e-9 absolute on the
outputs) and tests/test_local_attention_bwd.py (1e-10 relative per gradient tensor): two fp64 evaluations of the same function.
"""
import os
import random

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from indic_cl_asr_amd import _lib, ops
from indic_cl_asr_amd import checkpoint as ck
from indic_cl_asr_amd.config import model_config
from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
from indic_cl_asr_amd.ops.attention import context_interval_mask

Z = np.load(os.path.join(GOLDEN, "limited_context_cases.npz"))
NAMES = [str(n) for n in Z["name"]]
STYLES = ("regular", "chunked_limited")


def _case(i, grad=False):
    B, T, H, dk, style, L, R = (int(v) for v in Z["shape"][i])
    f = lambda k, den: torch.from_numpy(Z[f"{k}{i}"].astype(np.float64) / den)
    W = {k: f(k, 32.0).requires_grad_(grad and k in ("wq", "wk", "wv", "wp", "u", "v"))
         for k in ("wq", "wk", "wv", "wp", "bq", "bk", "bv", "u", "v")}
    return (B, T, H, dk, STYLES[style], L, R), f("x", 16.0).requires_grad_(grad), W, torch.from_numpy(Z[f"pe{i}"]).double(), \
        torch.from_numpy(Z[f"lens{i}"])


def _context(i, grad=False):
    (B, T, H, dk, style, L, R), x, W, pe, lens = _case(i, grad)
    proj = lambda wn, bn: (x @ W[wn].T + W[bn]).view(B, T, H, dk).transpose(1, 2)
    q, k, v = proj("wq", "bq"), proj("wk", "bk"), proj("wv", "bv")
    p = (pe @ W["wp"].T).view(-1, H, dk).transpose(0, 1)
    assert p.shape[1] == 2 * T - 1
    ctx = ops.rel_pos_attention(q, k, v, p, W["u"], W["v"], lens, context=(style, L, R))
    assert ctx.dtype == torch.float64
    return ctx.transpose(1, 2).reshape(B, T, H * dk), x, W, lens


def test_fixture_holds_the_issue_cases():
    got = [(STYLES[int(s[4])], int(s[5]), int(s[6])) for s in Z["shape"]]
    assert got == [("regular", 8, 3), ("regular", 5, 0), ("regular", -1, 4), ("chunked_limited", 8, 3), ("chunked_limited", -1, 6),
                   ("chunked_limited", 12, -1), ("chunked_limited", 70, 13)]
    lens = [int(n) for i in range(len(NAMES)) for n in Z[f"lens{i}"]]
    assert 1 in lens and 64 in lens


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_composition_matches_reference_fp64(i):
    out, _, _, lens = _context(i)
    ref = torch.from_numpy(Z[f"out{i}"])
    valid = torch.arange(out.shape[1])[None, :] < lens[:, None]
    err = float((out - ref)[valid].abs().max())
    print(f"{NAMES[i]}: max |composition - reference| on valid rows = {err:.3e} (outputs up to {float(ref.abs().max()):.3f})")
    assert err <= 1e-9
    assert float(out[~valid].abs().max()) == 0.0 if (~valid).any() else True
    assert float(ref[~valid].abs().max()) == 0.0 if (~valid).any() else True


@pytest.mark.parametrize("i", range(len(NAMES)), ids=NAMES)
def test_composition_gradients_match_reference_fp64(i):
    out, x, W, _ = _context(i, grad=True)
    g = torch.from_numpy(Z[f"g{i}"].astype(np.float64) / 8.0)
    (out * g).sum().backward()
    got = dict(dx=x.grad, dwq=W["wq"].grad, dwk=W["wk"].grad, dwv=W["wv"].grad, dwp=W["wp"].grad, du=W["u"].grad, dv=W["v"].grad)
    for name, t in got.items():
        ref = torch.from_numpy(Z[f"{name}{i}"])
        rel = float((t - ref).abs().max()) / float(ref.abs().max())
        print(f"{NAMES[i]} {name}: max |composition - reference| / max|reference| = {rel:.3e}")
        assert rel <= 1e-10, (name, rel)


def test_interval_mask_is_the_pair_rule_and_defaults_are_unchanged():
    T = 41
    for style, L, R in (("regular", 8, 3), ("regular", 0, 0), ("regular", -1, 4), ("regular", 5, -1), ("chunked_limited", 8, 3),
                        ("chunked_limited", -1, 6), ("chunked_limited", 12, -1), ("chunked_limited", 0, 0), ("chunked_limited", 26, 12)):
        m = context_interval_mask(T, style, L, R)
        for i in range(T):
            for j in range(T):
                if style == "regular" or R < 0:
                    ok = (L < 0 or i - j <= L) and (R < 0 or j - i <= R)
                else:
                    C = R + 1
                    ok = 0 <= i // C - j // C and (L < 0 or i // C - j // C <= L // C)
                assert bool(m[i, j]) == (not ok), (style, L, R, i, j)
            assert not bool(m[i, i])                                     # every query keeps its own key
    with pytest.raises(ValueError, match="Invalid att_context_style"):
        context_interval_mask(T, "sliding", 4, 4)
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(2, 2, 9, 4, generator=g, dtype=torch.float64) for _ in range(3))
    p = torch.randn(2, 17, 4, generator=g, dtype=torch.float64)
    u, vb = torch.randn(2, 4, generator=g, dtype=torch.float64), torch.randn(2, 4, generator=g, dtype=torch.float64)
    lens = torch.tensor([9, 5])
    base = ops.rel_pos_attention(q, k, v, p, u, vb, lens)
    assert torch.equal(ops.rel_pos_attention(q, k, v, p, u, vb, lens, context=None), base)
    assert torch.equal(ops.rel_pos_attention(q, k, v, p, u, vb, lens, context=("regular", -1, -1)), base)
    assert not torch.equal(ops.rel_pos_attention(q, k, v, p, u, vb, lens, context=("regular", 2, 0)), base)
    with pytest.raises(ValueError):
        ops.rel_pos_attention(q, k, v, p[:, :5], u, vb, lens, window=2, context=("regular", 2, 0))


def test_new_symbols_exist():
    L = _lib.lib()
    for name in ("ia_relpos_attention_context_supported", "ia_relpos_attention_context", "ia_relpos_attention_context_lse",
                 "ia_relpos_attention_context_bwd_dims", "ia_relpos_attention_context_bwd_ws_elems", "ia_relpos_attention_context_bwd"):
        assert hasattr(L, name), name
    from indic_cl_asr_amd.ops import fast
    for name in ("attention_context_supported", "relpos_attention_context", "relpos_attention_context_bwd"):
        assert callable(getattr(fast, name))
    names = [n for n, _ in _lib.BlockParams._fields_]
    assert names[-4:] == ["att_window", "att_style", "att_left", "att_right"]
    S = L.ia_relpos_attention_context_supported                          # host-only answers
    assert S(64, 64, 0, 4, 4) == 1 and S(64, 64, 1, 8, 3) == 1 and S(64, 64, 1, 9, 3) == 0 and S(64, 64, 2, 4, 4) == 0
    assert S(64, 64, 0, -2, 4) == 0 and S(64, 64, 0, 4, -2) == 0 and S(64, 68, 0, 4, 4) == 0 and S(64, 64, 1, 12, -1) == 1


# ------------------------------------------------------------------------------------------------------------- surface
def _tiny(seed=5, **kw):
    torch.manual_seed(seed)
    kw.setdefault("compute_dtype", "fp32")
    return EncDecHybridRNNTCTCModel(model_config("tiny", **kw))


def test_unset_style_keeps_refusing_a_limited_context():
    m = _tiny()
    assert m.cfg.att_context_style is None and m.encoder.att_context_style is None
    for target in (m, m.encoder):
        with pytest.raises(NotImplementedError, match="att_context_style"):
            target.change_attention_model("rel_pos", [8, 8])
        with pytest.raises(NotImplementedError, match="att_context_style"):
            target.change_attention_model("rel_pos", [[8, 8], [-1, -1]])
    assert m.encoder.att_context_size == [-1, -1] and all(l.self_attn.att_context is None for l in m.encoder.layers)
    n = _tiny(att_context_style="regular")                              # NeMo's yaml says regular: behaves as NeMo
    n.change_attention_model("rel_pos", [8, 8])
    assert n.encoder.att_context_size == [8, 8] and n.cfg.att_context_size == [8, 8]
    assert all(l.self_attn.att_context == ("regular", 8, 8) for l in n.encoder.layers)


def test_validation_rules():
    m = _tiny()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    for target in (m, m.encoder):
        with pytest.raises(ValueError, match="Invalid att_context_style"):
            target.change_attention_model("rel_pos", [8, 3], att_context_style="sliding")
        with pytest.raises(ValueError, match=r"att_context_size\[0\]\[0\] % \(att_context_size\[0\]\[1\] \+ 1\) should be zero!"):
            target.change_attention_model("rel_pos", [9, 3], att_context_style="chunked_limited")
        with pytest.raises(ValueError, match="can not be unlimited for chunked_limited style!"):
            target.change_attention_model("rel_pos", [12, -1], att_context_style="chunked_limited")
        with pytest.raises(ValueError, match=r"att_context_size\[1\]\[0\]"):
            target.change_attention_model("rel_pos", [[8, 3], [9, 3]], att_context_style="chunked_limited")
        with pytest.raises(ValueError, match="size of the att_context_probs"):
            target.change_attention_model("rel_pos", [[8, 3], [12, 3]], att_context_style="chunked_limited", att_context_probs=[1.0])
        with pytest.raises(ValueError, match="should be equal to one"):
            target.change_attention_model("rel_pos", [[8, 3], [12, 3]], att_context_style="chunked_limited", att_context_probs=[0.5, 0.25])
        with pytest.raises(ValueError, match="must be \\[left, right\\]"):
            target.change_attention_model("rel_pos", [8, 3, 1], att_context_style="regular")
        with pytest.raises(ValueError, match="multi-look-ahead"):
            target.change_attention_model("rel_pos_local_attn", [[8, 8], [4, 4]])
        with pytest.raises(NotImplementedError, match="wrong columns"):        # local attention is unchanged
            target.change_attention_model("rel_pos_local_attn", [8, 3])
        with pytest.raises(ValueError, match="local attention .* has no context style"):   # ... and reads no style
            target.change_attention_model("rel_pos_local_attn", [8, 8], att_context_style="regular")
    assert m.encoder.self_attention_model == "rel_pos" and m.encoder.att_context_size == [-1, -1]
    assert m.encoder.att_context_style is None and m.cfg.att_context_style is None     # a refused call changes nothing
    assert all(l.self_attn.att_context is None and l.self_attn.att_window is None for l in m.encoder.layers)
    after = m.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)


def test_switching_leaves_state_dict_and_returns_to_full_attention():
    m = _tiny()
    keys = list(m.state_dict().keys())
    before = {k: v.clone() for k, v in m.state_dict().items()}
    m.change_attention_model("rel_pos", [8, 3], att_context_style="chunked_limited", update_config=False)
    assert m.encoder.att_context_size == [8, 3] and m.encoder.att_context_style == "chunked_limited"
    assert m.cfg.att_context_size == [-1, -1] and m.cfg.att_context_style is None                  # config left alone
    m.change_attention_model("rel_pos", (16, 0), att_context_style="regular")
    assert m.cfg.att_context_size == [16, 0] and m.cfg.att_context_style == "regular" and m.cfg.self_attention_model == "rel_pos"
    assert all(l.self_attn.att_context == ("regular", 16, 0) and l.self_attn.att_window is None for l in m.encoder.layers)
    assert m.encoder.pos_enc.local_window is None and m.encoder.pos_enc.pos_emb_for(30).shape == (1, 59, m.cfg.d_model)
    m.change_attention_model(att_context_size=[4, 4])                                               # model and style are kept
    assert all(l.self_attn.att_context == ("regular", 4, 4) for l in m.encoder.layers)
    after = m.state_dict()
    assert list(after.keys()) == keys and all(torch.equal(before[k], after[k]) for k in keys)
    m.change_attention_model("rel_pos_local_attn", [5, 5])                                          # to local attention and back
    assert all(l.self_attn.att_context is None and l.self_attn.att_window == 5 for l in m.encoder.layers)
    m.change_attention_model("rel_pos")
    assert m.cfg.self_attention_model == "rel_pos" and m.cfg.att_context_size == [-1, -1] and m.encoder.att_context_size == [-1, -1]
    assert all(l.self_attn.att_context is None and l.self_attn.att_window is None for l in m.encoder.layers)
    assert m.encoder.att_context_size_all == [[-1, -1]]


def _is_full(m):
    e = m.encoder
    return (e.self_attention_model == "rel_pos" and e.att_context_size == [-1, -1] and e.att_context_size_all == [[-1, -1]]
            and e.att_context_probs == [1.0] and e.pos_enc.local_window is None
            and all(l.self_attn.att_context is None and l.self_attn.att_window is None for l in e.layers)
            and m.cfg.self_attention_model == "rel_pos" and m.cfg.att_context_size == [-1, -1] and m.cfg.att_context_probs is None)


@pytest.mark.parametrize("how", ["model", "encoder"])
def test_full_attention_returns_from_the_chunked_style(how):
    """change_attention_model("rel_pos") -- [-1, -1] implied or spelled out -- is the way back while the retained style is
    'chunked_limited': directly, by way of local attention, and at the end of the sequence INTEGRATION.md shows, as written."""
    m = _tiny()
    target = m if how == "model" else m.encoder
    for size in ((), ([-1, -1],)):
        target.change_attention_model("rel_pos", [8, 3], att_context_style="chunked_limited")
        target.change_attention_model("rel_pos", *size)
        assert _is_full(m) and m.encoder.att_context_style == "chunked_limited"
        target.change_attention_model("rel_pos", [8, 3], att_context_style="chunked_limited")
        target.change_attention_model("rel_pos_local_attn", [5, 5])
        assert all(l.self_attn.att_window == 5 and l.self_attn.att_context is None for l in m.encoder.layers)
        target.change_attention_model("rel_pos", *size)
        assert _is_full(m)
    # INTEGRATION.md, the limited-context block, line by line
    model = m
    model.change_attention_model("rel_pos", att_context_size=[70, 13], att_context_style="chunked_limited")
    model.change_attention_model("rel_pos", att_context_size=[64, 0], att_context_style="regular")
    model.change_attention_model("rel_pos", [[70, 13], [70, 6], [70, 1], [70, 0]], att_context_style="chunked_limited",
                                 att_context_probs=[0.25] * 4)
    model.set_default_att_context_size([70, 6])
    assert all(l.self_attn.att_context == ("chunked_limited", 70, 6) for l in m.encoder.layers)
    model.change_attention_model("rel_pos")
    assert _is_full(m)
    # a limited context with an unlimited right side stays refused under the chunked style
    with pytest.raises(ValueError, match="can not be unlimited for chunked_limited style!"):
        target.change_attention_model("rel_pos", [12, -1])
    assert _is_full(m)


def test_the_style_keyword_alone_applies_to_the_contexts_in_force():
    m = _tiny()
    m.change_attention_model()                                          # nothing given: nothing changes
    assert _is_full(m) and m.encoder.att_context_style is None
    m.change_attention_model(att_context_style="regular")              # full attention under a named style
    assert _is_full(m) and m.encoder.att_context_style == "regular" and m.cfg.att_context_style == "regular"
    m.change_attention_model(att_context_size=[8, 3])
    m.change_attention_model(att_context_style="chunked_limited")      # [8, 3] is a legal chunked context: kept, re-styled
    assert all(l.self_attn.att_context == ("chunked_limited", 8, 3) for l in m.encoder.layers)
    assert m.cfg.att_context_style == "chunked_limited" and m.cfg.att_context_size == [8, 3]
    m.change_attention_model("rel_pos", [9, 3], att_context_style="regular")
    with pytest.raises(ValueError, match="should be zero!"):           # [9, 3] is not: refused, nothing changes
        m.change_attention_model(att_context_style="chunked_limited")
    assert m.encoder.att_context_style == "regular" and all(l.self_attn.att_context == ("regular", 9, 3) for l in m.encoder.layers)
    all_ctx, probs = [[12, 3], [12, 1], [8, 3]], [0.5, 0.25, 0.25]
    m.change_attention_model("rel_pos", all_ctx, att_context_style="regular", att_context_probs=probs)
    m.set_default_att_context_size([12, 1])
    m.encoder.change_attention_model(att_context_style="chunked_limited")   # the list, its probabilities and the default stay
    e = m.encoder
    assert e.att_context_size_all == all_ctx and e.att_context_probs == probs and e.att_context_size == [12, 1]
    assert all(l.self_attn.att_context == ("chunked_limited", 12, 1) for l in e.layers) and m.cfg.att_context_size == all_ctx
    m.change_attention_model("rel_pos_local_attn", [5, 5])
    with pytest.raises(ValueError, match="has no context style"):
        m.change_attention_model(att_context_style="regular")
    assert e.self_attention_model == "rel_pos_local_attn" and e.att_context_style == "chunked_limited"


def test_forward_changes_with_the_context_and_full_attention_returns_bit_for_bit():
    m = _tiny().eval()
    g = torch.Generator().manual_seed(1)
    feats, fl = torch.randn(2, m.cfg.feat_in, 101, generator=g), torch.tensor([101, 57])   # (no host front end: log-mel features)
    run = lambda: m.encoder(feats, fl)[0]
    with torch.no_grad():
        full = run()
        m.change_attention_model("rel_pos", [4, 0], att_context_style="regular")
        causal = run()
        m.change_attention_model("rel_pos", [-1, -1])
        again = run()
        m.change_attention_model("rel_pos", [4, 1], att_context_style="chunked_limited")
        chunked = run()
        m.change_attention_model("rel_pos")
        back = run()
    assert torch.equal(full, again) and not torch.equal(full, causal)
    assert torch.equal(full, back) and not torch.equal(full, chunked) and not torch.equal(causal, chunked)


def test_config_and_checkpoint_round_trip(tmp_path):
    m = _tiny()
    m.change_attention_model("rel_pos", [70, 13], att_context_style="chunked_limited")
    y = ck.nemo_yaml_from_config(m.cfg)
    assert y["encoder"]["att_context_style"] == "chunked_limited" and y["encoder"]["att_context_size"] == [70, 13]
    cfg = ck.config_from_nemo_yaml(y, languages=m.cfg.languages, vocab_per_lang=m.cfg.vocab_per_lang, compute_dtype="fp32")
    assert cfg.att_context_style == "chunked_limited" and cfg.att_context_size == [70, 13] and cfg.self_attention_model == "rel_pos"
    path = str(tmp_path / "ctx.nemo")
    ck.write_nemo(m, path)
    n, _ = ck.model_from_nemo(path, strict=True, languages=m.cfg.languages, vocab_per_lang=m.cfg.vocab_per_lang, compute_dtype="fp32")
    assert n.encoder.att_context_style == "chunked_limited" and n.encoder.att_context_size == [70, 13]
    assert all(l.self_attn.att_context == ("chunked_limited", 70, 13) for l in n.encoder.layers)
    # multi-look-ahead travels as a list of pairs with its probabilities
    m.change_attention_model("rel_pos", [[70, 13], [70, 6], [70, 1], [70, 0]], att_context_style="chunked_limited",
                             att_context_probs=[0.25, 0.25, 0.25, 0.25])
    y = ck.nemo_yaml_from_config(m.cfg)
    assert y["encoder"]["att_context_size"] == [[70, 13], [70, 6], [70, 1], [70, 0]] and y["encoder"]["att_context_probs"] == [0.25] * 4
    cfg = ck.config_from_nemo_yaml(y, languages=m.cfg.languages, vocab_per_lang=m.cfg.vocab_per_lang, compute_dtype="fp32")
    k = EncDecHybridRNNTCTCModel(cfg)
    assert k.encoder.att_context_size_all == [[70, 13], [70, 6], [70, 1], [70, 0]] and k.encoder.att_context_size == [70, 13]
    assert k.encoder.att_context_probs == [0.25] * 4
    # a default config writes no style and reads back as before
    y = ck.nemo_yaml_from_config(_tiny().cfg)
    assert "att_context_style" not in y["encoder"] and "att_context_probs" not in y["encoder"]
    d = ck.config_from_nemo_yaml(y)
    assert d.att_context_style is None and d.att_context_size == [-1, -1]


# ---------------------------------------------------------------------------------------------------- multi-look-ahead
def test_multi_look_ahead_draws_one_context_per_training_forward(monkeypatch):
    """With random.seed(k) the contexts the layers see over several training forwards are the random.choices sequence, one draw
    per forward shared by every layer; evaluation uses the default, which set_default_att_context_size changes."""
    from indic_cl_asr_amd import encoder as enc_mod
    all_ctx = [[12, 3], [12, 1], [12, -1], [-1, -1]]
    probs = [0.4, 0.3, 0.2, 0.1]
    m = _tiny(n_layers=3)
    m.change_attention_model("rel_pos", all_ctx, att_context_style="chunked_limited", att_context_probs=probs)
    assert m.encoder.att_context_size_all == all_ctx and m.encoder.att_context_size == [12, 3] and m.encoder.att_context_probs == probs
    assert m.cfg.att_context_size == all_ctx and m.cfg.att_context_probs == probs
    seen = []
    orig = ops.rel_pos_attention
    monkeypatch.setattr(enc_mod.ops, "rel_pos_attention", lambda *a, **kw: (seen.append(kw.get("context")), orig(*a, **kw))[1])
    g = torch.Generator().manual_seed(1)
    feats, fl = torch.randn(2, m.cfg.feat_in, 101, generator=g), torch.tensor([101, 57])   # (no host front end: log-mel features)
    as_layer = lambda c: None if c == [-1, -1] else ("chunked_limited", c[0], c[1])
    m.train()
    random.seed(7)
    with torch.no_grad():
        for _ in range(8):
            m.encoder(feats, fl)
    random.seed(7)
    want = [random.choices(all_ctx, weights=probs)[0] for _ in range(8)]
    assert len(set(map(tuple, want))) > 1                                # the seed shows more than one context
    assert seen == [as_layer(c) for c in want for _ in range(3)]         # one draw per forward, all three layers alike
    del seen[:]
    m.eval()
    with torch.no_grad():
        m.encoder(feats, fl)
    assert seen == [("chunked_limited", 12, 3)] * 3                      # the default: the first entry
    del seen[:]
    for target in (m, m.encoder):
        with pytest.raises(ValueError, match="is not among the list of the supported look-aheads"):
            target.set_default_att_context_size([12, 7])
    m.set_default_att_context_size([12, 1])
    assert m.encoder.att_context_size == [12, 1] and m.encoder.att_context_size_all == all_ctx
    with torch.no_grad():
        m.encoder(feats, fl)
    assert seen == [("chunked_limited", 12, 1)] * 3
    # uniform probabilities by default
    m.change_attention_model("rel_pos", [[8, 3], [8, 1]], att_context_style="chunked_limited")
    assert m.encoder.att_context_probs == [0.5, 0.5]
