"""Writes tests/golden/rnnt_alsd_cases.npz: small transducer decode operands and the lists NeMo's own
BeamRNNTInfer(search_type="alsd") returns for them in float64.  Run by hand, never imported:

    python tests/golden/make_rnnt_alsd_golden.py /path/to/NeMo

NeMo's rnnt_beam_decoding.py and rnnt_utils.py are loaded unchanged from that checkout.  Their heavy imports are stood in for:
nemo.core.classes by a bare Typing and an identity typecheck; rnnt_abstract and modules.rnnt by the small prediction network /
joint below, which work on the decode operands of this repository (EW = the input half of the LSTM cell per row, W_hh, W_pred,
the head) and offer what the search calls: initialize_state, batch_select_state, batch_initialize_states,
batch_score_hypothesis with its sequence-keyed cache, blank_idx, vocab_size, blank_as_pad.

The file holds data only.  Per case c: the operands (f_all, EW, Whh, Wp, bp, Wh, bh, lens), W, and per utterance u the returned
hypotheses as flat arrays (len [n], tok / ts concatenated, score [n]); NeMo's sequences keep the leading blank, dropped here.
Cases: (T, Hp, Hj, V, W) = (12, 8, 8, 6, 2), (20, 16, 16, 9, 4), (24, 16, 24, 17, 16) at blank bias 5 (finished lists longer
than the beam, an utterance whose finished list stays empty, more than 10 recombinations), and one case found by seed search
in which a record of the finished list receives a recombination in the step that appended it."""
import contextlib
import importlib.util
import io
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def load_reference(nemo_root):
    sys.path.insert(0, nemo_root)
    import nemo.utils  # noqa: F401

    def pkg(name):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [os.path.join(nemo_root, *name.split("."))]
            sys.modules[name] = m
        return sys.modules[name]

    def load(path, name):
        spec = importlib.util.spec_from_file_location(name, path)
        m = importlib.util.module_from_spec(spec)
        sys.modules[name] = m
        spec.loader.exec_module(m)
        return m

    cc = types.ModuleType("nemo.core.classes")
    cc.Typing = type("Typing", (), {})
    cc.typecheck = lambda *a, **k: (lambda f: f)
    sys.modules["nemo.core.classes"] = cc
    for n in ("nemo.collections", "nemo.collections.asr", "nemo.collections.asr.parts", "nemo.collections.asr.parts.utils",
              "nemo.collections.asr.parts.submodules", "nemo.collections.asr.modules"):
        pkg(n)
    ra = types.ModuleType("nemo.collections.asr.modules.rnnt_abstract")
    ra.AbstractRNNTDecoder = ra.AbstractRNNTJoint = type("Abstract", (), {})
    sys.modules["nemo.collections.asr.modules.rnnt_abstract"] = ra
    sys.modules["nemo.collections.asr.modules"].rnnt_abstract = ra
    rm = types.ModuleType("nemo.collections.asr.modules.rnnt")
    rm.RNNTDecoder, rm.StatelessTransducerDecoder = Decoder, type("StatelessTransducerDecoder", (), {})
    sys.modules["nemo.collections.asr.modules.rnnt"] = rm
    load(os.path.join(nemo_root, "nemo/collections/asr/parts/utils/rnnt_utils.py"), "nemo.collections.asr.parts.utils.rnnt_utils")
    return load(os.path.join(nemo_root, "nemo/collections/asr/parts/submodules/rnnt_beam_decoding.py"), "ref_rnnt_beam_decoding")


class Decoder(torch.nn.Module):
    """The prediction network on the decode operands: one LSTM layer, state = [h, c] as lists over layers."""

    def __init__(self, case):
        super().__init__()
        self.c, self.Hp = case, case["Whh"].shape[1]
        V = case["Wh"].shape[0]
        self.blank_idx, self.vocab_size, self.blank_as_pad = V - 1, V - 1, True
        self.p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))

    def as_frozen(self):
        return contextlib.nullcontext()

    def initialize_state(self, y):
        return [torch.zeros(1, y.size(0), self.Hp, dtype=y.dtype), torch.zeros(1, y.size(0), self.Hp, dtype=y.dtype)]

    def batch_select_state(self, states, idx):
        return [[x[0][idx]] for x in states]

    def batch_initialize_states(self, batch_states, decoder_states):
        for sid in range(len(decoder_states[0])):
            batch_states[sid][0] = torch.stack([d[sid][0] for d in decoder_states])
        return batch_states

    def cell(self, row, h, c):
        Hp = self.Hp
        g = self.c["Whh"] @ h + self.c["EW"][row]
        i, f, gg, o = torch.sigmoid(g[:Hp]), torch.sigmoid(g[Hp:2 * Hp]), torch.tanh(g[2 * Hp:3 * Hp]), torch.sigmoid(g[3 * Hp:])
        cn = f * c + i * gg
        return o * torch.tanh(cn), cn

    def batch_score_hypothesis(self, hyps, cache, batch_states):
        done = []
        for hyp in hyps:
            seq = tuple(hyp.y_sequence)
            if seq not in cache:
                hn, cn = self.cell(hyp.y_sequence[-1], hyp.dec_state[0][0], hyp.dec_state[1][0])
                cache[seq] = (hn.view(1, -1), [[hn], [cn]])
            done.append(cache[seq])
        return torch.stack([y for y, _ in done]), self.batch_initialize_states(batch_states, [d for _, d in done]), None


class Joint(torch.nn.Module):
    def __init__(self, case):
        super().__init__()
        self.c = case
        self.p = torch.nn.Parameter(torch.zeros(1, dtype=torch.float64))

    def as_frozen(self):
        return contextlib.nullcontext()

    def joint(self, f, g):          # f [B,1,Hj]: already the encoder projection; g [B,1,Hp]
        pre = f.unsqueeze(2) + (g @ self.c["Wp"].t() + self.c["bp"]).unsqueeze(1)
        return torch.relu(pre) @ self.c["Wh"].t() + self.c["bh"]


def make_case(seed, B, T, Hp, Hj, V, scale, bias):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    EW = r(V + 1, 4 * Hp) * 0.5
    bh = torch.cat([r(V - 1) * 0.1, torch.tensor([bias], dtype=torch.float64)])
    return dict(f_all=r(B, T, Hj) * scale, EW=EW, Whh=r(4 * Hp, Hp) / math.sqrt(Hp), Wp=r(Hj, Hp) / math.sqrt(Hp), bp=r(Hj) * 0.1,
                Wh=r(V, Hj) * scale / math.sqrt(Hj), bh=bh, lens=torch.tensor([T, T - 3][:B]))


def run_reference(bd, case, W):
    inf = bd.BeamRNNTInfer(Decoder(case), Joint(case), beam_size=W, search_type="alsd", score_norm=True, return_best_hypothesis=False)
    with contextlib.redirect_stderr(io.StringIO()):
        out = inf(encoder_output=case["f_all"].transpose(1, 2), encoded_lengths=case["lens"])[0]
    return [[(h.y_sequence.tolist()[1:], float(h.score), list(h.timestep)) for h in nb.n_best_hypotheses] for nb in out]


def main():
    from indic_cl_asr_amd import decoding as D
    bd = load_reference(sys.argv[1])
    specs = [(3, 2, 12, 8, 8, 6, 2.0, 5.0, 2), (3, 2, 20, 16, 16, 9, 2.0, 5.0, 4), (3, 2, 24, 16, 24, 17, 3.0, 5.0, 16)]
    for seed in range(100, 400):      # a finished record that a recombination of its own step changes
        spec = (seed, 1, 10, 8, 8, 6, 2.0, 4.0, 4)
        if D.beam_rnnt_alsd_host(make_case(*spec[:8]), 4)[0]["finished_recombined"]:
            specs.append(spec)
            break
    store = {"n_cases": np.array(len(specs))}
    for c, spec in enumerate(specs):
        case, W = make_case(*spec[:8]), spec[8]
        for k, v in case.items():
            store[f"c{c}_{k}"] = v.numpy()
        store[f"c{c}_W"] = np.array(W)
        for u, hyps in enumerate(run_reference(bd, case, W)):
            store[f"c{c}_u{u}_len"] = np.array([len(h[0]) for h in hyps], dtype=np.int64)
            store[f"c{c}_u{u}_tok"] = np.array([t for h in hyps for t in h[0]], dtype=np.int64)
            store[f"c{c}_u{u}_ts"] = np.array([t for h in hyps for t in h[2]], dtype=np.int64)
            store[f"c{c}_u{u}_score"] = np.array([h[1] for h in hyps], dtype=np.float64)
            mine = D.beam_rnnt_alsd_host(case, W)[u]
            print("case", c, spec, "utterance", u, "hypotheses", len(hyps), "finished", mine["n_finished"], "recombinations",
                  mine["recombinations"], "into a finished record", mine["finished_recombined"])
    np.savez_compressed(os.path.join(HERE, "rnnt_alsd_cases.npz"), **store)


if __name__ == "__main__":
    main()
