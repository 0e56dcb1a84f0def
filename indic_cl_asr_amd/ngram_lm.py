"""Back-off n-gram language models for the CTC prefix beam search (decoding.beam_ctc_decode, csrc/ctc_beam_lm.hip).

NeMo's LM for BPE models is a TOKEN-level n-gram: scripts/asr_language_modeling/ngram_lm/train_kenlm.py writes token id i as the
character chr(i + 100) and ctc_beam_decoding.py reads it back the same way, so the model scores the units the search extends by.
KenLM's text format (ARPA) is read here in plain Python; KenLM binaries are not.

The definition (include/indicasr.h has it too): lm(l, c) = ln P(c | h), h = the last N - 1 symbols of (<s>, l_1 .. l_k), N the
order.  For k = |h| .. 0: if h[-k:] + c is in the model, acc + log p of it; otherwise acc += backoff(h[-k:]) (0 if that context
is not in the model or k = 0).  A token without a unigram scores acc + log p(<unk>) and leaves the empty history behind.  </s> is
never scored.  ARPA's log10 values become natural logs in float64 and are rounded to float32 once, here; `score` adds them in
float64, the kernel in float32.
"""
import math
import re
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

_LN10 = math.log(10.0)
_BLANKS = " \t\r\n"      # KenLM's separators; str.split() would also cut at chr(133) and chr(160), which are the tokens 33 and 60


def _natural(log10_value: float) -> float:
    return float(np.float32(log10_value * _LN10))


class NGramLM:
    """A loaded model.  `ngrams`: {token tuple: (log p, back-off)} in natural logs, <s> being the token `bos` = num_tokens and
    only ever first; `order`; `unk_logp`; `dropped` = the n-grams of the file that were not kept.

    The flat image (`arrays`, and `to(device)` for the kernel; the layout is ia_ngram_lm's in include/indicasr.h): states = the
    root + every kept n-gram of order < N, sorted by (order, tokens); per state its back-off weight, the link to its longest
    proper suffix that is a state, and its arcs (token, log p, next state) sorted by token; a dense unigram row."""

    def __init__(self, ngrams: Dict[Tuple[int, ...], Tuple[float, float]], order: int, num_tokens: int, unk_logp: float,
                 dropped: int = 0):
        self.ngrams, self.order, self.num_tokens, self.unk_logp, self.dropped = ngrams, int(order), int(num_tokens), unk_logp, dropped
        self.bos = self.num_tokens
        self.nbytes = 0
        self._rows = {}
        self._device = {}
        self._build()

    # ------------------------------------------------------------------------------------------------------------- ARPA
    @classmethod
    def from_arpa(cls, path, num_tokens: int, token_offset: int = 100, vocabulary: Optional[Sequence[str]] = None):
        """Reads an ARPA file.  A word is <s>, </s>, <unk>, or ONE character with ord(word) - token_offset in [0, num_tokens)
        (with `vocabulary`, a list: the word's index in it).  N-grams that hold an unmapped word, </s>, or <s> beyond the first
        position are dropped and counted in `dropped`."""
        with open(path, "rb") as f:
            raw = f.read()
        try:
            text = raw.decode("utf-8")
            first = next((ln.strip(_BLANKS) for ln in text.split("\n") if ln.strip(_BLANKS)), "")
        except UnicodeDecodeError:
            first = None
        if first != "\\data\\":
            raise NotImplementedError(f"kenlm_path: {path} does not start as ARPA text (\\data\\); KenLM binary files are not read, "
                                      "ARPA only")
        index = {w: i for i, w in enumerate(vocabulary)} if vocabulary is not None else None

        def token(word):
            if index is not None:
                i = index.get(word, -1)
            else:
                i = ord(word) - token_offset if len(word) == 1 else -1
            return i if 0 <= i < num_tokens else None

        def bad(no, why):
            return ValueError(f"{path}, line {no}: {why}")

        counts, found, ngrams, dropped = {}, {}, {}, 0
        unk = None
        section, ended = None, False             # None: before \data\; 0: the header; n: the n-grams of order n
        last = end_no = 0                        # the last line that holds text; the line of \\end\\
        for no, line in enumerate(text.split("\n"), 1):
            line = line.strip(_BLANKS)
            if not line:
                continue
            last = no
            if ended:
                raise bad(no, "text after \\end\\")
            if line == "\\data\\":
                if section is not None:
                    raise bad(no, "a second \\data\\")
                section = 0
            elif line == "\\end\\":
                if not section:
                    raise bad(no, "\\end\\ before any n-gram section")
                ended, end_no = True, no
            elif line.startswith("\\"):
                if not line.endswith("-grams:") or not line[1:-7].isdigit():
                    raise bad(no, f"unknown section {line!r}")
                n = int(line[1:-7])
                if section is None or n != section + 1 or n not in counts:
                    raise bad(no, f"section {line!r} out of order or not in the header")
                section = n
                found[n] = 0
            elif section == 0:
                head, _, value = line.partition("=")
                if not head.startswith("ngram ") or not head[6:].strip().isdigit() or not value.strip().isdigit():
                    raise bad(no, f"expected `ngram n=count`, got {line!r}")
                n = int(head[6:])
                if n != len(counts) + 1:
                    raise bad(no, f"order {n} after order {len(counts)}")
                counts[n] = int(value)
            elif section is None:
                raise bad(no, "text before \\data\\")
            else:
                fields = [f for f in re.split("[ \t]+", line) if f]
                if len(fields) not in (section + 1, section + 2):
                    raise bad(no, f"a {section}-gram line has {section + 1} or {section + 2} fields, got {len(fields)}")
                try:
                    logp = float(fields[0])
                    backoff = float(fields[section + 1]) if len(fields) == section + 2 else 0.0
                except ValueError:
                    raise bad(no, f"not a number in {line!r}") from None
                if not (math.isfinite(logp) and math.isfinite(backoff)):
                    raise bad(no, "log-probabilities and back-offs must be finite")
                found[section] += 1
                words = fields[1:section + 1]
                if section == 1 and words[0] == "<unk>":
                    unk = _natural(logp)
                    continue
                key = []
                for pos, w in enumerate(words):
                    t = num_tokens if (w == "<s>" and pos == 0) else (None if w in ("<s>", "</s>", "<unk>") else token(w))
                    if t is None:
                        break
                    key.append(t)
                if len(key) != section:
                    dropped += 1
                    continue
                key = tuple(key)
                if key in ngrams:
                    raise bad(no, f"the n-gram {' '.join(words)} appears twice")
                ngrams[key] = (_natural(logp), _natural(backoff))
        if not ended:
            raise bad(last, "no \\end\\")
        for n, c in counts.items():
            if found.get(n) != c:
                raise bad(end_no, f"the header announces {c} {n}-grams, the file holds {found.get(n, 0)}")
        if unk is None:
            raise ValueError(f"{path}: no <unk> unigram")
        for key in ngrams:
            if len(key) > 1 and key[:-1] not in ngrams:
                raise ValueError(f"{path}: the n-gram {key} is kept but its prefix {key[:-1]} is not in the model")
        return cls(ngrams, len(counts), num_tokens, unk, dropped)

    # ------------------------------------------------------------------------------------------------------------ scoring
    def history(self, tokens: Sequence[int]) -> Tuple[int, ...]:
        """h(l): the last order - 1 symbols of (<s>, l)."""
        keep = self.order - 1
        return tuple(([self.bos] + [int(t) for t in tokens])[-keep:]) if keep > 0 else ()

    def score(self, history_tokens: Sequence[int], c: int) -> float:
        """ln P(c | h(history_tokens)) in float64 by the back-off formula; history_tokens is the prefix l (without <s>)."""
        return self._score(self.history(history_tokens), int(c))

    def _score(self, h: Tuple[int, ...], c: int) -> float:
        known = 0 <= c < self.num_tokens and (c,) in self.ngrams
        acc = 0.0
        for k in range(len(h), -1, -1):
            ctx = h[len(h) - k:]
            if known and ctx + (c,) in self.ngrams:
                return acc + self.ngrams[ctx + (c,)][0]
            if k > 0 and ctx in self.ngrams:
                acc += self.ngrams[ctx][1]
        return acc + self.unk_logp

    def row(self, history_tokens: Sequence[int], n: int):
        """[score(history_tokens, c) for c < n] as a float64 array, kept per history: what the host search adds per member.
        Built from the flat image the way the kernel builds its rows (the unigram row, then the arcs of each state on the
        back-off chain, shortest context first); the sums run in the order of `score`, so the values are its values."""
        h = self.history(history_tokens)
        got = self._rows.get((h, n))
        if got is None:
            a = self.arrays
            s, chain, acc = self._suffix_state(h, self._index), [], 0.0
            while s > 0:
                chain.append((s, acc))
                acc += float(a["backoff"][s])
                s = int(a["states"][s, 0])
            got = np.full(n, acc + self.unk_logp, np.float64)
            k = min(n, self.num_tokens)
            got[:k] = acc + a["uni_logp"][:k].astype(np.float64)
            for s, above in reversed(chain):
                a0, a1 = int(a["states"][s, 1]), int(a["states"][s, 2])
                toks = a["arcs"][a0:a1, 0]
                keep = toks < n
                got[toks[keep]] = above + a["arc_logp"][a0:a1].astype(np.float64)[keep]
            self._rows[(h, n)] = got
        return got

    # -------------------------------------------------------------------------------------------------------- flat image
    def _suffix_state(self, key, index):
        """The longest suffix of `key`, at most order - 1 long, that is a state."""
        for start in range(max(0, len(key) - (self.order - 1)), len(key) + 1):
            s = index.get(key[start:])
            if s is not None:
                return s
        return 0

    def _build(self):
        N, V = self.order, self.num_tokens
        contexts = sorted((k for k in self.ngrams if len(k) < N), key=lambda k: (len(k), k))
        index = {(): 0}
        for k in contexts:
            index[k] = len(index)
        S, self._index = len(index), index
        states = np.zeros((S, 3), np.int32)
        backoff = np.zeros(S, np.float32)
        children = {}
        for g in self.ngrams:
            if len(g) > 1:
                children.setdefault(g[:-1], []).append(g)
        arcs, arc_logp = [], []
        for k in contexts:
            s = index[k]
            backoff[s] = self.ngrams[k][1]
            states[s, 0] = self._suffix_state(k[1:], index)
            states[s, 1] = len(arcs)
            for g in sorted(children.get(k, ())):
                arcs.append((g[-1], index[g] if len(g) < N else self._suffix_state(g[1:], index)))
                arc_logp.append(self.ngrams[g][0])
            states[s, 2] = len(arcs)
        uni_logp = np.full(V, self.unk_logp, np.float32)
        uni_next = np.zeros(V, np.int32)
        for c in range(V):
            if (c,) in self.ngrams:
                uni_logp[c] = self.ngrams[(c,)][0]
                uni_next[c] = index.get((c,), 0)
        self.n_states, self.n_arcs = S, len(arcs)
        self.start = index.get((self.bos,), 0)
        self.arrays = dict(states=states, backoff=backoff,
                           arcs=np.array(arcs, np.int32).reshape(-1, 2) if arcs else np.zeros((1, 2), np.int32),   # never empty:
                           arc_logp=np.array(arc_logp, np.float32) if arcs else np.zeros(1, np.float32),           # a pointer to pass
                           uni_logp=uni_logp, uni_next=uni_next)
        self.nbytes = int(sum(a.nbytes for a in self.arrays.values()))

    def to(self, device):
        """The image on `device`: (tensors by name, the ia_ngram_lm structure that points at them), built once per device."""
        import torch
        from . import _lib
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        got = self._device.get(device)
        if got is None:
            t = {k: torch.from_numpy(v).to(device).contiguous() for k, v in self.arrays.items()}
            image = None
            if device.type == "cuda":
                image = _lib.NGramLM(**{k: _lib.ptr(v) for k, v in t.items()}, n_states=self.n_states, n_arcs=self.n_arcs,
                                     n_tokens=self.num_tokens, order=self.order, start=self.start, unk_logp=self.unk_logp)
            got = self._device[device] = (t, image)
        return got
