"""Local rel-pos attention (change_attention_model, ops.rel_pos_attention(window=...)) on the host.

The golden cases are outputs of the reference's RelPositionMultiHeadAttentionLongformer + LocalAttRelPositionalEncoding in fp64
(tests/golden/make_local_attention_golden.py; linear_out = identity, so the stored output is the attention context and a padded
row is exactly zero).  The reference against a band-masked restatement measured 1.3e-15 there; the bound here, 1e-9 absolute on
outputs of scale 3 - 5, leaves room for another summation order and nothing else.
"""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

from indic_cl_asr_amd import checkpoint as ck
from indic_cl_asr_amd import ops
from indic_cl_asr_amd.config import model_config
from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel

Z = np.load(os.path.join(GOLDEN, "local_attention_cases.npz"))
NAMES = [str(n) for n in Z["name"]]
SYM = [i for i, s in enumerate(Z["shape"]) if s[4] == s[5]]
ASYM = [i for i, s in enumerate(Z["shape"]) if s[4] != s[5]]


def _case(i):
    B, T, H, dk, L, R = (int(v) for v in Z["shape"][i])
    f = lambda k, den: torch.from_numpy(Z[f"{k}{i}"].astype(np.float64) / den)
    W = {k: f(k, 32.0) for k in ("wq", "wk", "wv", "wp", "bq", "bk", "bv", "u", "v")}
    return (B, T, H, dk, L, R), f("x", 16.0), W, torch.from_numpy(Z[f"pe{i}"]).double(), torch.from_numpy(Z[f"lens{i}"]), \
        torch.from_numpy(Z[f"out{i}"])


def test_fixture_holds_the_issue_cases():
    assert len(SYM) == 4 and len(ASYM) == 2
    assert [tuple(int(v) for v in Z["shape"][i]) for i in SYM] == [(2, 50, 2, 8, 4, 4), (2, 130, 2, 8, 16, 16), (1, 65, 4, 4, 64, 64),
                                                                  (2, 200, 2, 8, 5, 5)]
    assert [Z[f"lens{i}"].tolist() for i in SYM] == [[50, 33], [130, 70], [65], [200, 1]]
    assert [tuple(int(v) for v in Z["shape"][i][4:]) for i in ASYM] == [(8, 3), (3, 8)]


@pytest.mark.parametrize("i", SYM, ids=[NAMES[i] for i in SYM])
def test_composition_matches_reference_fp64(i):
    (B, T, H, dk, w, _), x, W, pe, lens, ref = _case(i)
    proj = lambda wn, bn: (x @ W[wn].T + W[bn]).view(B, T, H, dk).transpose(1, 2)
    q, k, v = proj("wq", "bq"), proj("wk", "bk"), proj("wv", "bv")
    p = (pe @ W["wp"].T).view(-1, H, dk).transpose(0, 1)
    assert p.shape[1] == 2 * w + 1
    ctx = ops.rel_pos_attention(q, k, v, p, W["u"], W["v"], lens, window=w)
    assert ctx.dtype == torch.float64
    out = ctx.transpose(1, 2).reshape(B, T, H * dk)
    valid = torch.arange(T)[None, :] < lens[:, None]
    err = float((out - ref)[valid].abs().max())
    print(f"{NAMES[i]}: max |composition - reference| on valid rows = {err:.3e} (outputs up to {float(ref.abs().max()):.3f})")
    assert err <= 1e-9
    assert float(out[~valid].abs().max()) == 0.0 if (~valid).any() else True
    assert float(ref[~valid].abs().max()) == 0.0 if (~valid).any() else True


def _tiny(seed=5, **kw):
    torch.manual_seed(seed)
    kw.setdefault("compute_dtype", "fp32")
    return EncDecHybridRNNTCTCModel(model_config("tiny", **kw))


@pytest.mark.parametrize("i", ASYM, ids=[NAMES[i] for i in ASYM])
def test_asymmetric_windows_are_refused(i):
    L, R = (int(v) for v in Z["shape"][i][4:])
    m = _tiny()
    with pytest.raises(NotImplementedError, match="wrong columns"):
        m.change_attention_model("rel_pos_local_attn", [L, R])
    with pytest.raises(NotImplementedError, match="wrong columns"):
        m.encoder.change_attention_model("rel_pos_local_attn", [L, R])
    assert m.encoder.self_attention_model == "rel_pos" and m.cfg.att_context_size == [-1, -1]


def test_surface_errors_and_noop():
    m = _tiny()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.change_attention_model() is None and m.encoder.change_attention_model() is None        # both None: nothing changes
    assert m.cfg.self_attention_model == "rel_pos" and m.cfg.att_context_size == [-1, -1]
    assert m.encoder.pos_enc.local_window is None and all(l.self_attn.att_window is None for l in m.encoder.layers)
    for target in (m, m.encoder):
        with pytest.raises(ValueError, match="When using local attention, context size must be set > 0"):
            target.change_attention_model("rel_pos_local_attn")                                     # context still [-1, -1]
        with pytest.raises(ValueError, match="When using local attention, context size must be set > 0"):
            target.change_attention_model("rel_pos_local_attn", [0, 0])
        with pytest.raises(ValueError, match="Not valid self_attention_model"):
            target.change_attention_model("rel_pos_global", [4, 4])
        with pytest.raises(NotImplementedError):
            target.change_attention_model("abs_pos")
        with pytest.raises(NotImplementedError):
            target.change_attention_model("rel_pos", [8, 8])                                        # limited context under rel_pos
        with pytest.raises(NotImplementedError):
            target.change_attention_model("rel_pos_local_attn", [8, 3])
    assert m.cfg.self_attention_model == "rel_pos" and m.encoder.self_attention_model == "rel_pos"
    after = m.state_dict()
    assert before.keys() == after.keys() and all(torch.equal(before[k], after[k]) for k in before)


def test_state_dict_and_config():
    m = _tiny()
    keys = list(m.state_dict().keys())
    saved_full = {k: v.clone() for k, v in m.state_dict().items()}
    m.change_attention_model("rel_pos_local_attn", [5, 5], update_config=False)
    assert m.encoder.self_attention_model == "rel_pos_local_attn" and m.encoder.att_context_size == [5, 5]
    assert m.cfg.self_attention_model == "rel_pos" and m.cfg.att_context_size == [-1, -1]           # config left alone
    m.change_attention_model("rel_pos_local_attn", (7, 7))
    assert m.cfg.self_attention_model == "rel_pos_local_attn" and m.cfg.att_context_size == [7, 7]
    assert m.encoder.pos_enc.pos_emb_for(123).shape == (1, 15, m.cfg.d_model)
    assert all(l.self_attn.att_window == 7 for l in m.encoder.layers)
    m.change_attention_model(att_context_size=[9, 9])                                                # the model is kept
    assert m.cfg.self_attention_model == "rel_pos_local_attn" and m.cfg.att_context_size == [9, 9]
    assert list(m.state_dict().keys()) == keys                                                       # same keys in local mode
    saved_local = {k: v.clone() for k, v in m.state_dict().items()}
    # strict load both ways: a checkpoint from before the switch into the switched model, and one from after into a fresh one
    m.load_state_dict(saved_full, strict=True)
    fresh = _tiny(seed=6)
    fresh.load_state_dict(saved_local, strict=True)
    assert all(torch.equal(fresh.state_dict()[k], saved_local[k]) for k in keys)
    # a model built from a config that names local attention starts in that mode
    n = _tiny(self_attention_model="rel_pos_local_attn", att_context_size=[3, 3])
    assert n.encoder.self_attention_model == "rel_pos_local_attn" and n.encoder.pos_enc.local_window == 3
    assert all(l.self_attn.att_window == 3 for l in n.encoder.layers) and list(n.state_dict().keys()) == keys
    m.change_attention_model("rel_pos")
    assert m.cfg.self_attention_model == "rel_pos" and m.cfg.att_context_size == [-1, -1]
    assert m.encoder.pos_enc.local_window is None and all(l.self_attn.att_window is None for l in m.encoder.layers)


def test_nemo_yaml_round_trip(tmp_path):
    m = _tiny()
    m.change_attention_model("rel_pos_local_attn", [64, 64])
    y = ck.nemo_yaml_from_config(m.cfg)
    assert y["encoder"]["self_attention_model"] == "rel_pos_local_attn" and y["encoder"]["att_context_size"] == [64, 64]
    cfg = ck.config_from_nemo_yaml(y)
    assert cfg.self_attention_model == "rel_pos_local_attn" and cfg.att_context_size == [64, 64]
    p = tmp_path / "local.nemo"
    ck.write_nemo(m, p)
    b, _ = ck.model_from_nemo(p, strict=True, languages=m.cfg.languages, vocab_per_lang=m.cfg.vocab_per_lang, compute_dtype="fp32")
    assert b.cfg.self_attention_model == "rel_pos_local_attn" and b.cfg.att_context_size == [64, 64]
    assert b.encoder.pos_enc.local_window == 64
    full = ck.config_from_nemo_yaml(ck.nemo_yaml_from_config(_tiny().cfg))
    assert full.self_attention_model == "rel_pos" and full.att_context_size == [-1, -1]
    assert ck.config_from_nemo_yaml({"encoder": {"d_model": 32}}).self_attention_model == "rel_pos"   # older yaml: the default


def test_executors_validate_the_window_before_any_device_work():
    """ia_block_params.att_window: all layers of a prefix call agree (else IA_INVALID_VALUE), the position-row check becomes
    pos_rows >= 2w+1, and the trainable-block executor takes only 0.  Every answer below comes before the first launch (the
    pointers are host scratch that is never read)."""
    import ctypes
    from indic_cl_asr_amd import _lib
    L = _lib.lib()
    scratch = ctypes.create_string_buffer(256)
    ptr = ctypes.c_void_p(ctypes.addressof(scratch))
    B, T = 1, 100

    def layers(*windows):
        arr = (_lib.BlockParams * len(windows))()
        for bp, w in zip(arr, windows):
            bp.d, bp.d_ff, bp.n_heads, bp.ksz, bp.att_window = 64, 256, 4, 9, w
        return arr

    def prefix(arr, pos_rows, ws_bytes=0):
        return L.ia_conformer_prefix_fwd(ctypes.addressof(arr), len(arr), ptr, ptr, pos_rows, ptr, B, T, 0, 16, 0, ptr, ws_bytes, None)

    assert prefix(layers(4, 0), 199) == -1                       # layers disagree: IA_INVALID_VALUE
    assert prefix(layers(0, 4), 199) == -1
    assert prefix(layers(-1, -1), 199) == -1
    assert prefix(layers(4, 4), 8) == -1                         # fewer than 2w+1 position rows
    assert prefix(layers(4, 4), 9) == -2                         # 2w+1 rows are enough (next check: IA_WORKSPACE_TOO_SMALL) ...
    assert prefix(layers(0, 0), 9) == -1                         # ... for full attention they are not: 2T-1
    assert prefix(layers(0, 0), 199) == -2
    one = layers(4)
    assert L.ia_conformer_block_supported(64, 256, 4, 9, T) == 1    # (so the refusal below is the window's)
    saved = _lib.BlockSaved()
    st = L.ia_conformer_block_fwd(ctypes.addressof(one), ptr, ptr, 199, ptr, B, T, 0, ctypes.addressof(saved), ptr, ptr, None)
    assert st == -4                                              # the trainable block: IA_UNSUPPORTED under a window
    assert L.ia_relpos_attention_local(None, None, None, None, None, 1, 64, 1, 64, 4, 0.0, 0, None, None) == -1
    assert L.ia_relpos_attention_local_supported(64, 64, 0) == 0 and L.ia_relpos_attention_local_supported(64, 64, 1) == 1
    assert L.ia_relpos_attention_local_supported(64, 68, 4) == 0 and L.ia_relpos_attention_local_supported(64, 36, 4) == 1


def _features(B=2, Tm=200, lens=(200, 147), seed=3, feat=80):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, feat, Tm, generator=g), torch.tensor(lens)


def _encode(m, feats, lens):
    with torch.no_grad():
        out, olen = m.encoder(feats, lens)
    return out, olen


def test_switching_back_is_bit_exact():
    m = _tiny().eval()
    feats, lens = _features()
    a, alen = _encode(m, feats, lens)
    m.change_attention_model("rel_pos_local_attn", [5, 5])
    b, _ = _encode(m, feats, lens)
    m.change_attention_model("rel_pos")
    c, clen = _encode(m, feats, lens)
    assert torch.equal(a, c) and torch.equal(alen, clen)
    assert not torch.equal(a, b)


def test_wide_window_equals_full_and_narrow_does_not():
    m = _tiny().eval()
    feats, lens = _features()
    full, olen = _encode(m, feats, lens)
    T = full.shape[2]
    valid = (torch.arange(T)[None, :] < olen[:, None]).unsqueeze(1)
    scale = float((full * valid).abs().max())
    m.change_attention_model("rel_pos_local_attn", [T - 1, T - 1])
    wide, _ = _encode(m, feats, lens)
    m.change_attention_model("rel_pos_local_attn", [2, 2])
    narrow, _ = _encode(m, feats, lens)
    e_wide = float(((wide - full) * valid).abs().max()) / scale
    e_narrow = float(((narrow - full) * valid).abs().max()) / scale
    print(f"T' = {T}: wide window vs full {e_wide:.3e}, [2,2] vs full {e_narrow:.3e} (relative to {scale:.3f})")
    assert e_wide <= 1e-5          # the executor-agreement tolerance of tests/test_block_native_gpu.py
    assert e_narrow > 1e-5


def test_table_does_not_depend_on_pos_emb_max_len():
    m = _tiny(pos_emb_max_len=16).eval()
    feats, lens = _features(Tm=160, lens=(160, 101))
    m.change_attention_model("rel_pos_local_attn", [6, 6])
    out, olen = _encode(m, feats, lens)
    assert out.shape[2] == 40 and olen.tolist() == [40, 26] and torch.isfinite(out).all()
    # the same window on a model whose table is long enough: the same arithmetic
    big = _tiny(pos_emb_max_len=5000).eval()
    big.change_attention_model("rel_pos_local_attn", [6, 6])
    out2, _ = _encode(big, feats, lens)
    assert torch.equal(out, out2)
    assert torch.equal(m.encoder.pos_enc.pos_emb_for(40), big.encoder.pos_enc.pe[:, 5000 - 7: 5000 + 6])   # positions 6 .. -6


def _host_front_end(monkeypatch):
    """The log-mel front end is HIP only; on the host the test stands in for its two ops (what is under test starts at the
    encoder)."""
    from indic_cl_asr_amd import features

    def log_mel(signal, window, fb, n_fft=512, hop=160, **kw):
        win = torch.nn.functional.pad(window, ((n_fft - window.numel()) // 2, (n_fft - window.numel() + 1) // 2))
        p = torch.stft(signal, n_fft, hop_length=hop, window=win, center=True, return_complex=True).abs() ** 2
        return torch.log(fb @ p + 2.0 ** -24)

    def normalize_mask(x, seq_len, spec_aug=None):
        keep = (torch.arange(x.shape[-1]).unsqueeze(0) < seq_len.unsqueeze(1)).unsqueeze(1)
        n = seq_len.view(-1, 1, 1).float()
        mean = (x * keep).sum(-1, keepdim=True) / n
        var = (((x - mean) * keep) ** 2).sum(-1, keepdim=True) / (n - 1).clamp(min=1)
        return ((x - mean) / (var.sqrt() + 1e-5)) * keep

    monkeypatch.setattr(features.ops, "log_mel", log_mel)
    monkeypatch.setattr(features.ops, "normalize_mask", normalize_mask)


def _host_transducer_loss(acts, labels, act_lens, label_lens, blank, *unused):
    """The transducer loss is HIP only as well; on the host the test stands in for it with the plain forward recursion on
    autograd (per-utterance costs [B], as the HIP loss returns them to RNNTLoss)."""
    lp = torch.log_softmax(acts.float(), dim=-1)
    costs = []
    for b in range(acts.shape[0]):
        T, U = int(act_lens[b]), int(label_lens[b])
        row = [lp.new_zeros(())]
        for u in range(1, U + 1):
            row.append(row[u - 1] + lp[b, 0, u - 1, labels[b, u - 1]])
        for t in range(1, T):
            new = [row[0] + lp[b, t - 1, 0, blank]]
            for u in range(1, U + 1):
                new.append(torch.logaddexp(row[u] + lp[b, t - 1, u, blank], new[u - 1] + lp[b, t, u - 1, labels[b, u - 1]]))
            row = new
        costs.append(-(row[U] + lp[b, T - 1, U, blank]))
    return torch.stack(costs)


def test_training_step_under_local_attention(monkeypatch):
    _host_front_end(monkeypatch)
    m = _tiny().train()
    monkeypatch.setattr(m.loss._loss, "loss", _host_transducer_loss)
    m.spec_augment_enabled = False
    m.change_attention_model("rel_pos_local_attn", [4, 4])
    with torch.no_grad():   # (zero-initialised in the reference and here: give the position term something to carry)
        for l in m.encoder.layers:
            l.self_attn.pos_bias_v.normal_(0.0, 0.1)
    g = torch.Generator().manual_seed(11)
    sig = torch.randn(3, 8000, generator=g) * 0.1
    sl = torch.tensor([8000, 6000, 4000]); tr = torch.randint(0, 16, (3, 6), generator=g); tl = torch.tensor([6, 3, 1])
    loss, _ = m.training_step((sig, sl, tr, tl), ["hi"] * 3, compute_wer=False)
    loss.backward()
    assert math.isfinite(float(loss.detach()))
    att = m.encoder.layers[-1].self_attn
    for name in ("linear_pos.weight", "pos_bias_v"):
        gr = dict(att.named_parameters())[name].grad
        assert gr is not None and torch.isfinite(gr).all() and float(gr.abs().max()) > 0.0, name
