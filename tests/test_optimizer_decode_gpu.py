"""Optimizer / decoding behaviours at the drop-in boundary that the step-level parity tests do not reach:
  * AdamW over the flat buffer must skip tensors that received no gradient exactly like torch.optim.AdamW skips
    `p.grad is None` (R/cl_baseline.py:137,187-196: optimizer.zero_grad() -> set_to_none) -- the other languages' joint
    heads and, after a task switch, the previous language's head;
  * greedy decoding / in-step WER on the default bf16 configuration (persistent HIP LSTM in the training step, stateful
    library LSTM in the decode loop);
  * a lost hand-off of the persistent LSTM surfaces as RuntimeError instead of silently wrong outputs."""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import step_ref as S


def _batch(B=4, L=12000, U=6, seed=1, vocab=16):
    g = torch.Generator().manual_seed(seed)
    sl = torch.tensor([L] + [int(L * (0.55 + 0.45 * torch.rand(1, generator=g))) for _ in range(B - 1)])
    sig = torch.randn(B, L, generator=g) * 0.1
    for i in range(B):
        sig[i, sl[i]:] = 0
    tl = torch.tensor([U] + [int(torch.randint(1, U + 1, (1,), generator=g)) for _ in range(B - 1)])
    tr = torch.randint(0, vocab, (B, U), generator=g)
    return sig, sl, tr, tl


def test_adamw_skips_tensors_without_gradient_across_a_language_switch():
    """Oracle model + torch.optim.AdamW with zero_grad(set_to_none) vs product + FusedAdamW: 3 steps on 'hi', then 3 on
    'ta'.  The 'ta' head must not move (no weight decay) during the first task, the 'hi' head must freeze -- momentum
    and all -- after the switch, and the per-tensor step counters must give the 'ta' head bias corrections of a fresh
    parameter."""
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel, freeze_layer
    torch.manual_seed(0)
    o = S.OracleHybridModel(d_model=32, n_layers=2, n_heads=4, pred_hidden=24, joint_hidden=24, languages=['hi', 'ta'],
                            vocab_per_lang=16, fused_batch_size=2)
    m = EncDecHybridRNNTCTCModel(model_config('tiny', compute_dtype='fp32', dither=0.0))
    m.load_state_dict(o.state_dict())
    m = m.disable_dropout().cuda().train(); o.train()
    m.spec_augment_enabled = False
    S.freeze_layer(o, 0); freeze_layer(m, 0); m.encoder.encoder_frozen_till = 0
    flat = cl.FlatParams(m)
    opt = cl.FusedAdamW(flat, lr=1e-3, weight_decay=0.1)
    oref = torch.optim.AdamW([p for p in o.parameters() if p.requires_grad], lr=1e-3, weight_decay=0.1)
    batch = _batch()
    cb = tuple(t.cuda() for t in batch)
    ta0 = dict(o.named_parameters())["joint.joint_net.2.ta.weight"].detach().clone()
    p0 = {n: p.detach().clone() for n, p in o.named_parameters()}
    for step in range(6):
        lang = 'hi' if step < 3 else 'ta'
        oref.zero_grad(set_to_none=True); opt.zero_grad()
        lo, _ = o.training_step(batch, [lang] * 4); lo.backward(); oref.step()
        lp, _ = m.training_step(cb, [lang] * 4); lp.backward(); opt.step()
        if step == 2:
            hi3 = dict(o.named_parameters())["joint.joint_net.2.hi.weight"].detach().clone()
            # untouched during task 1: bit-identical to its initial value on both sides (no decay)
            assert torch.equal(dict(o.named_parameters())["joint.joint_net.2.ta.weight"], ta0)
            assert torch.equal(flat.params_dict()["joint.joint_net.2.ta.weight"].cpu(), ta0)
    po = dict(o.named_parameters())
    assert torch.equal(po["joint.joint_net.2.hi.weight"], hi3)                         # reference: frozen after the switch
    torch.cuda.synchronize()
    for n in flat.names:
        # Adam normalises every gradient component to an O(lr) step, so components that are rounding noise (structurally
        # zero gradients: a bias in front of train-mode BatchNorm, the key bias; near-zero components elsewhere) move
        # differently under the CPU and GPU fp32 kernels: bound the error by the distance the tensor travelled, and pin
        # the tensors this test is about (the two language heads, the joint projections) tightly
        if n.endswith("depthwise_conv.bias") or n.endswith("self_attn.linear_k.bias"):
            continue
        a, b, b0 = flat.params_dict()[n].cpu().double(), po[n].detach().double(), p0[n].double()
        moved = (b - b0).norm().item()
        assert (a - b).norm().item() <= 0.35 * moved + 1e-7, (n, (a - b).norm().item(), moved)
        if n.startswith("joint."):
            assert torch.allclose(a, b, rtol=2e-4, atol=1e-4), (n, (a - b).abs().max().item())
    assert torch.allclose(flat.params_dict()["joint.joint_net.2.hi.weight"].cpu(), hi3, rtol=2e-4, atol=2e-4)
    # step counters: 'hi' head 3 updates, 'ta' head 3 updates, shared tensors 6
    steps = dict(zip(flat.names, opt.seg_step.tolist()))
    assert steps["joint.joint_net.2.hi.weight"] == 3 and steps["joint.joint_net.2.ta.weight"] == 3
    assert steps["joint.enc.weight"] == 6
    # the bf16 weight images the HIP GEMMs read stay in step with theta for updated AND skipped tensors
    assert torch.equal(opt.shadow[:flat.numel].float(), flat.theta.bfloat16().float())


def test_adamw_updates_every_tensor_when_a_penalty_was_preloaded():
    """EWC (task > 0): set_grads gives EVERY trainable tensor a gradient (R/utils.py:316-321), zeros included, so
    torch.optim.AdamW decays all of them -- the flat optimizer must do the same."""
    from indic_cl_asr_amd import cl
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(0)
    m = EncDecHybridRNNTCTCModel(model_config('tiny', compute_dtype='fp32', dither=0.0)).disable_dropout().cuda().train()
    m.spec_augment_enabled = False
    flat = cl.FlatParams(m)
    opt = cl.FusedAdamW(flat, lr=1e-2, weight_decay=0.1)
    fish = cl.get_zero_params(m); ck = cl.get_params_clone(m)
    ta = flat.params_dict()["joint.joint_net.2.ta.weight"]
    before = ta.clone()
    opt.zero_grad()
    loss, _ = m.training_step(tuple(t.cuda() for t in _batch()), ['hi'] * 4)
    cl.ewc_penalty_into_grads(flat, fish, ck, 10.0)      # zero Fisher: zero penalty, but every .grad is now "set"
    loss.backward(); opt.step()
    assert torch.allclose(ta, before * (1 - 1e-2 * 0.1), rtol=1e-6, atol=0)   # pure weight decay, as torch does
    assert opt.seg_step.min().item() == 1


@pytest.mark.parametrize("pred_hidden", [64, 128])
def test_greedy_decode_and_in_step_wer_on_the_bf16_configuration(pred_hidden):
    """decode() / training_step(compute_wer=True) with compute_dtype='bf16' and pred_hidden % 64 == 0: the training step
    uses the persistent HIP LSTM (no final state), the greedy loop needs (h, c) and must get the stateful LSTM."""
    from indic_cl_asr_amd.config import model_config
    from indic_cl_asr_amd.model import EncDecHybridRNNTCTCModel
    torch.manual_seed(1)
    kw = dict(d_model=64, n_layers=2, n_heads=4, pred_hidden=pred_hidden, joint_hidden=64, languages=['hi', 'ta'],
              vocab_per_lang=16, fused_batch_size=2)
    o = S.OracleHybridModel(**kw)
    with torch.no_grad():  # bias the head away from blank so that hypotheses are non-empty
        o.joint.joint_net[-1]['hi'].bias[-1] -= 2.0
    m = EncDecHybridRNNTCTCModel(model_config('tiny', compute_dtype='bf16', dither=0.0, **kw))
    m.load_state_dict(o.state_dict())
    m = m.disable_dropout().cuda().train(); m.spec_augment_enabled = False
    batch = _batch()
    cb = tuple(t.cuda() for t in batch)
    loss, mon = m.training_step(cb, ['hi'] * 4, compute_wer=True)
    loss.backward()
    assert math.isfinite(float(mon['training_batch_wer'])) and math.isfinite(float(mon['training_batch_wer_ctc']))
    with torch.no_grad():
        enc, elen = m(input_signal=cb[0], input_signal_length=cb[1])
        hyp = m.decode(enc, elen, ['hi'] * 4)
    assert sum(len(h) for h in hyp) > 0                     # the stateful path really ran
    # same hypotheses as the per-utterance restatement of the reference loop on the product's own encoder output
    o.eval()
    ref = S.greedy_rnnt_decode_ref(o, enc.float().cpu(), elen.cpu(), 'hi')
    agree = sum(int(a == b) for a, b in zip(hyp, ref))
    print("identical to the fp32 restatement:", agree, "of 4")
    # ... and every utterance a member of the acceptable set of the fp64 replay on the operands the device decode builds (the EW
    # table, the fp32 set-up GEMMs, the bf16 images of W_hh / W_pred / the head, activations rounded to bf16 for the MFMA head)
    from oracle import decode_ref as R
    case = R.case_from_model(m, enc, elen, 'hi')
    assert case["bf16"]
    acc = R.decode_reference(case, 10, "mfma")
    print(R.summarize(acc))
    assert all(R.member(h, r) for h, r in zip(hyp, acc)), (hyp, [sorted(r["accept"]) for r in acc])


def test_lost_lstm_handoff_raises_instead_of_returning_wrong_outputs():
    from indic_cl_asr_amd.ops import lstm as hip_lstm
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(128, 128).cuda()
    x = torch.randn(12, 4, 128, device="cuda")
    y = hip_lstm.lstm_forward(x, lstm)
    torch.cuda.synchronize()
    hip_lstm.raise_if_timed_out()                            # healthy run: nothing raised
    ref, _ = lstm(x)
    assert (y - ref).abs().max().item() < 2e-2
    os.environ["IA_LSTM_SPIN_LIMIT"] = "0"                   # every wait gives up at its first poll
    try:
        hip_lstm.lstm_forward(x, lstm)
        torch.cuda.synchronize()
    finally:
        del os.environ["IA_LSTM_SPIN_LIMIT"]
    flag = hip_lstm.timeout_flags(x.device)
    assert flag is not None and flag.item() >= 1
    with pytest.raises(RuntimeError, match="hand-off timed out"):
        hip_lstm.raise_if_timed_out()
    hip_lstm.raise_if_timed_out()                            # the flag was cleared by the raise
    # shapes whose W_hh slice cannot fit the LDS are refused up front (nn.LSTM fallback), not at launch
    assert not hip_lstm.lstm_supported(x, 1024 * 2)
