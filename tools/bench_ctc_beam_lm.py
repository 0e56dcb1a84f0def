"""DESIGN.md section 6, "n-gram LM shallow fusion": ia_ctc_beam_search_lm on the batch of tools/bench_ctc_beam.py (32 utterances,
T = 375, V = 257, row stride 264) at W = 4 and 16 with a synthetic token-level model of order 3 and of order 5, about 1e5
n-grams each, generated here (every unigram; each kept n-gram is a context that a token follows with a fixed probability).
Device events over 20 launches after 5 warm-up launches; beside it, in the same process and on the same batch, the LM-free
ia_ctc_beam_search (what the model costs) and, for order 3, the float64 host routine with the model (wall clock, one run).
One JSON line."""
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from indic_cl_asr_amd import _lib, decoding  # noqa: E402
from indic_cl_asr_amd.ngram_lm import NGramLM  # noqa: E402

L = _lib.lib()
B, T, V, ld = 32, 375, 257, 264
ALPHA, BETA = 0.7, 0.5
g = torch.Generator().manual_seed(0)
buf = torch.randn(B * T, ld, generator=g) * 4
buf[:, V - 1] += 4
logits = buf.cuda().view(B, T, ld)[..., :V]
lens = torch.full((B,), T, dtype=torch.long).cuda()
lse = torch.empty(B, T, device="cuda")
_lib.check(L.ia_ctc_row_lse(_lib.ptr(logits), ld, B * T, V, _lib.ptr(lse), _lib.stream_ptr()), "lse")
res = {"shape": [B, T, V], "ld": ld, "alpha": ALPHA, "beta": BETA}


def synthetic_lm(order, density, seed):
    """Natural logs, as NGramLM keeps them: log p in ln 10 * [-3, -0.1], back-off in ln 10 * [-1, 0] (0 at the highest order)."""
    rng = np.random.default_rng(seed)
    n_tok, ln10 = V - 1, float(np.log(10.0))
    entry = lambda top: (float(np.float32(rng.uniform(-3, -0.1) * ln10)), 0.0 if top else float(np.float32(rng.uniform(-1, 0) * ln10)))
    ngrams = {(n_tok,): (float(np.float32(-99 * ln10)), entry(order == 1)[1])}
    level = [(n_tok,)]
    for c in range(n_tok):
        ngrams[(c,)] = entry(order == 1)
        level.append((c,))
    for n in range(2, order + 1):
        nxt = []
        for ctx in level:
            for c in np.nonzero(rng.random(n_tok) < density)[0]:
                ngrams[ctx + (int(c),)] = entry(n == order)
                nxt.append(ctx + (int(c),))
        level = nxt
    return NGramLM(ngrams, order, n_tok, float(np.float32(-2.5 * ln10)))


def timed(launch):
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        launch()
    b.record()
    b.synchronize()
    return round(a.elapsed_time(b) * 1000.0 / 20, 1)


lms = {3: synthetic_lm(3, 0.075, 3), 5: synthetic_lm(5, 0.0164, 5)}
for N, lm in lms.items():
    res[f"lm{N}_ngrams"], res[f"lm{N}_states"], res[f"lm{N}_nbytes"] = len(lm.ngrams), lm.n_states, lm.nbytes

for W in (4, 16):
    tok = torch.empty(B, W, T, dtype=torch.int32, device="cuda")
    ln = torch.empty(B, W, dtype=torch.int32, device="cuda")
    sc = torch.empty(B, W, device="cuda")
    n0 = L.ia_ctc_beam_workspace_bytes(B, T, V, W)
    ws0 = torch.empty(n0, dtype=torch.uint8, device="cuda")
    res[f"beam_w{W}_us"] = timed(lambda: _lib.check(L.ia_ctc_beam_search(
        _lib.ptr(logits), _lib.ptr(lse), _lib.ptr(lens), B, T, ld, V, V - 1, W, float("-inf"), _lib.ptr(tok), _lib.ptr(ln),
        _lib.ptr(sc), _lib.ptr(ws0), n0, _lib.stream_ptr()), "beam"))
    n = L.ia_ctc_beam_lm_workspace_bytes(B, T, V, W)
    ws = torch.empty(n, dtype=torch.uint8, device="cuda")
    res[f"beam_lm_w{W}_workspace_bytes"] = int(n)
    for N, lm in lms.items():
        image = lm.to("cuda")[1]
        res[f"beam_lm{N}_w{W}_us"] = timed(lambda: _lib.check(L.ia_ctc_beam_search_lm(
            _lib.ptr(logits), _lib.ptr(lse), _lib.ptr(lens), B, T, ld, V, V - 1, W, float("-inf"), ctypes.byref(image), ALPHA, BETA,
            _lib.ptr(tok), _lib.ptr(ln), _lib.ptr(sc), _lib.ptr(ws), n, _lib.stream_ptr()), "beam_lm"))
    kw = dict(beam_size=W, lse=lse, lm=lms[3], beam_alpha=ALPHA, beam_beta=BETA)
    t0 = time.perf_counter()
    dev = decoding.beam_ctc_decode(logits, lens, **kw)
    res[f"beam_lm3_w{W}_python_entry_ms"] = round((time.perf_counter() - t0) * 1e3, 2)
    t0 = time.perf_counter()
    host = decoding.beam_ctc_decode_host(logits.cpu(), lens.cpu(), **dict(kw, lse=lse.cpu()))
    res[f"host_lm3_w{W}_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    res[f"lm3_w{W}_best_equal_to_host"] = sum(d.y_sequence == h.y_sequence for d, h in zip(dev, host))
print(json.dumps(res))
