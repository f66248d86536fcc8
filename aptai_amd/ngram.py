"""A token-level back-off n-gram language model for the CTC beam search (`lm=` / `lm_weight=` of ops.ctc_beam_search and of
hostlogic.ctc_beam_search, the half of flashlight's LexiconFreeDecoder that the reference leaves at lm=None).  Host only, numpy.

The model is compiled to a dense automaton that the search walks with two table reads per extension:
  states  the empty context, and every context of 1 .. order-1 words that is a listed k-gram (k < order) or a proper prefix of a
          listed n-gram; index 0 is the empty context, the others follow sorted by (length, words)
  score   fp64 [C][V]  natural-log probability of token w after context c, back-off fully resolved: the longest listed n-gram
          c+w, else bow(c) + score(c[1:], w); a missing back-off weight is 0
  next    int32 [C][V] the state of the longest suffix of (c+w)[-(order-1):] that is a state
  final   fp64 [C]     the same as `score` for </s>
  start   the state of (<s>,) if the model has it, else 0
The blank column is 0 with next = c and is never read.  Contexts that hold </s> or the blank cannot be reached and are no states.
Parity with KenLM / torchaudio is unpinned: neither is available to this project."""
import math
import os

import numpy as np

BOS, EOS, UNK = -1, -2, -3
MAX_ORDER = 5
MAX_TOKENS = 256
MAX_TABLE = 1 << 24
_LN10 = math.log(10.0)


class NGramLM:
    def __init__(self, score, next, final, start=0, blank=0):
        """A model given as its automaton, checked: no n-grams behind it (to_arpa and _logprob_by_definition refuse).  Models of
        n-grams come from `from_arpa` or `estimate`."""
        score = np.ascontiguousarray(score, dtype=np.float64)
        if score.ndim != 2:
            raise ValueError("NGramLM: score must be [C][V]")
        C, V = score.shape
        if V > MAX_TOKENS or V < 1:
            raise ValueError(f"NGramLM: V must be 1..{MAX_TOKENS}, not {V}")
        if C < 1 or C * V > MAX_TABLE:
            raise ValueError(f"NGramLM: C * V = {C} * {V} must be 1..2**24")
        nxt = np.ascontiguousarray(next, dtype=np.int32)
        final = np.ascontiguousarray(final, dtype=np.float64)
        if nxt.shape != (C, V) or final.shape != (C,) or not np.array_equal(nxt, np.asarray(next)):
            raise ValueError("NGramLM: next must be integers [C][V] and final [C]")
        if not (np.isfinite(score).all() and np.isfinite(final).all()):
            raise ValueError("NGramLM: every table entry must be finite")
        if nxt.min() < 0 or nxt.max() >= C:
            raise ValueError(f"NGramLM: entries of next must lie in [0, {C})")
        if not 0 <= int(start) < C or not 0 <= int(blank) < V:
            raise ValueError("NGramLM: start state or blank out of range")
        self.score, self.next, self.final = score, nxt, final
        self.start, self.blank = int(start), int(blank)
        self.n_states, self.n_tokens = C, V
        self.order = None
        self.tokens = None
        self._prob = self._bow = None
        self._names = ("<s>", "</s>")
        self._host, self._device = {}, {}

    # ------------------------------------------------------------------------------------------------ construction
    @classmethod
    def _compile(cls, prob, bow, order, tokens, blank, names=("<s>", "</s>")):
        """prob {(w1..wk): natural-log P(wk | w1..wk-1)}, bow {(w1..wk): natural-log back-off weight}, words = token ids, BOS, EOS."""
        V = len(tokens)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"NGramLM: order must be 1..{MAX_ORDER}, not {order}")
        if V > MAX_TOKENS:
            raise ValueError(f"NGramLM: at most {MAX_TOKENS} tokens, not {V}")
        if not 0 <= blank < V:
            raise ValueError(f"NGramLM: blank {blank} is no token id")
        for table in (prob, bow):
            for g, v in table.items():
                if not math.isfinite(v):
                    raise ValueError(f"NGramLM: entry of n-gram {g} is not finite")
        if (EOS,) not in prob:
            raise ValueError(f"NGramLM: the model has no unigram {names[1]!r}")
        real = [w for w in range(V) if w != blank]
        missing = [tokens[w] for w in real if (w,) not in prob]
        if missing:
            raise ValueError(f"NGramLM: tokens without a unigram: {missing}")

        def is_context(c):
            return 1 <= len(c) < order and EOS not in c and blank not in c and BOS not in c[1:]
        states = set()
        for g in list(prob) + list(bow):
            if is_context(g):
                states.add(g)
            for k in range(1, len(g)):
                if is_context(g[:k]):
                    states.add(g[:k])
        states = [()] + sorted(states, key=lambda c: (len(c), c))
        C = len(states)
        if C * V > MAX_TABLE:
            raise ValueError(f"NGramLM: {C} states x {V} tokens exceed 2**24 table entries")
        index = {c: i for i, c in enumerate(states)}

        def longest(c):
            while c not in index:
                c = c[1:]
            return index[c]
        listed = {}
        for g, p in prob.items():
            if g[:-1] in index:
                listed.setdefault(g[:-1], []).append((g[-1], p))
        score = np.zeros((C, V), dtype=np.float64)
        final = np.zeros(C, dtype=np.float64)
        nxt = np.zeros((C, V), dtype=np.int32)
        for i, c in enumerate(states):                 # shorter contexts first: the back-off row of c is complete
            if c:
                j = longest(c[1:])
                b = bow.get(c, 0.0)
                score[i] = b + score[j]
                final[i] = b + final[j]
            for w, p in listed.get(c, ()):
                if w == EOS:
                    final[i] = p
                elif w >= 0:
                    score[i, w] = p
            score[i, blank] = 0.0
            for w in real:
                nxt[i, w] = longest((c + (w,))[-(order - 1):]) if order > 1 else 0
            nxt[i, blank] = i
        lm = cls(score, nxt, final, index.get((BOS,), 0), blank)
        lm.order, lm.tokens, lm._prob, lm._bow, lm._names = order, list(tokens), dict(prob), dict(bow), names
        return lm

    @classmethod
    def from_arpa(cls, path_or_text, tokens, bos="<s>", eos="</s>", unk="<unk>", log10=False, blank=0):
        """Read an ARPA file (a path, or the text itself).  `tokens` is the id-ordered vocabulary, e.g. list(model.vocab); `blank`
        is the id that is never scored.  The silence token '(...)' is an ordinary word, as in flashlight.

        ARPA values are log10; they are multiplied by ln 10 in fp64 so that the model adds natural-log probabilities to the
        acoustic scores.  log10=True leaves them as they stand, which is how KenLM hands them to flashlight.  Which of the two
        torchaudio's decoder effectively uses is UNVERIFIED here (the package is not available to this project): pick by PER.

        A token without a unigram takes the entry of `unk`; without an `unk` unigram that is a ValueError naming the tokens.  A
        word that is neither a token nor bos / eos / unk is a ValueError.  N-grams of order 2 and up that hold `unk` are skipped
        (no token reaches them), and so is every n-gram that predicts `bos` (its back-off weight is kept)."""
        text = path_or_text
        if not (isinstance(text, str) and ("\n" in text or "\\data\\" in text)):
            with open(os.fspath(path_or_text), "r", encoding="utf-8") as f:
                text = f.read()
        tokens = list(tokens)
        word = {bos: BOS, eos: EOS, unk: UNK}
        word.update({t: i for i, t in enumerate(tokens)})
        scale = 1.0 if log10 else _LN10
        prob, bow, k, order = {}, {}, 0, 0
        for raw in text.splitlines():
            line = raw.strip()
            if not line or line == "\\data\\" or line.startswith("ngram "):
                continue
            if line == "\\end\\":
                break
            if line.startswith("\\") and line.endswith("-grams:"):
                k = int(line[1:-len("-grams:")])
                order = max(order, k)
                continue
            f = line.split()
            if k == 0 or len(f) not in (k + 1, k + 2):
                raise ValueError(f"NGramLM.from_arpa: cannot read line {raw!r}")
            unknown = [w for w in f[1:k + 1] if w not in word]
            if unknown:
                raise ValueError(f"NGramLM.from_arpa: {unknown} in {raw!r} are no tokens")
            g = tuple(word[w] for w in f[1:k + 1])
            if UNK in g and k > 1:
                continue
            if g[-1] != BOS:
                prob[g] = float(f[0]) * scale
            if len(f) == k + 2:
                bow[g] = float(f[k + 1]) * scale
        if order == 0:
            raise ValueError("NGramLM.from_arpa: no n-gram section")
        if not 0 <= blank < len(tokens):
            raise ValueError(f"NGramLM: blank {blank} is no token id")
        missing = [i for i in range(len(tokens)) if i != blank and (i,) not in prob]
        if missing and (UNK,) not in prob:
            raise ValueError(f"NGramLM.from_arpa: no unigram and no {unk!r} for tokens {[tokens[i] for i in missing]}")
        for i in missing:
            prob[(i,)] = prob[(UNK,)]
        prob.pop((UNK,), None)
        bow.pop((UNK,), None)
        return cls._compile(prob, bow, order, tokens, blank, (bos, eos))

    @classmethod
    def estimate(cls, sequences, tokens, order=3, blank=0):
        """Interpolated Witten-Bell from token id sequences, in fp64, so that a model can be made without KenLM:
            P(w | c) = (n(c, w) + N1+(c .) P(w | c')) / (n(c) + N1+(c .))
        with c' = c without its first word and N1+(c .) the number of different words seen after c; the unigram level is
        interpolated with the uniform distribution over the non-blank tokens plus </s>.  Written in back-off form: the seen
        n-grams carry P, bow(c) = log(N1+(c .) / (n(c) + N1+(c .))).  Every sequence is framed by <s> and </s>."""
        tokens = list(tokens)
        V = len(tokens)
        if not 1 <= order <= MAX_ORDER:
            raise ValueError(f"NGramLM: order must be 1..{MAX_ORDER}, not {order}")
        if V > MAX_TOKENS:
            raise ValueError(f"NGramLM: at most {MAX_TOKENS} tokens, not {V}")
        if not 0 <= blank < V:
            raise ValueError(f"NGramLM: blank {blank} is no token id")
        counts = [{} for _ in range(order)]            # counts[k][context of k words][w]
        for seq in sequences:
            ids = [int(w) for w in seq]
            if any(w < 0 or w >= V or w == blank for w in ids):
                raise ValueError("NGramLM.estimate: a sequence holds the blank or an id outside the vocabulary")
            s = [BOS] + ids + [EOS]
            for i in range(1, len(s)):
                for k in range(min(order - 1, i) + 1):
                    row = counts[k].setdefault(tuple(s[i - k:i]), {})
                    row[s[i]] = row.get(s[i], 0) + 1
        words = [w for w in range(V) if w != blank] + [EOS]
        uniform = 1.0 / len(words)
        uni = counts[0].get((), {})
        n, n1 = float(sum(uni.values())), float(len(uni))
        p_of = {(): {w: ((uni.get(w, 0) + n1 * uniform) / (n + n1) if n else uniform) for w in words}}
        prob = {(w,): math.log(p) for w, p in p_of[()].items()}
        bow = {}

        def p_backoff(c, w):                           # P(w | c) for any context, through the contexts that were seen
            while c not in p_of:
                c = c[1:]
            if w in p_of[c]:
                return p_of[c][w]
            row = counts[len(c)][c]
            n, n1 = float(sum(row.values())), float(len(row))
            return n1 * p_backoff(c[1:], w) / (n + n1)
        for k in range(1, order):
            for c in sorted(counts[k]):
                row = counts[k][c]
                n, n1 = float(sum(row.values())), float(len(row))
                p_of[c] = {w: (cnt + n1 * p_backoff(c[1:], w)) / (n + n1) for w, cnt in row.items()}
                bow[c] = math.log(n1 / (n + n1))
                for w, p in p_of[c].items():
                    prob[c + (w,)] = math.log(p)
        return cls._compile(prob, bow, order, tokens, blank)

    # ------------------------------------------------------------------------------------------------ use
    def _need_ngrams(self, what):
        if self._prob is None:
            raise ValueError(f"NGramLM.{what}: this model was given as tables, it has no n-grams")

    def to_arpa(self) -> str:
        """The model as ARPA text: log10 values with 17 significant digits."""
        self._need_ngrams("to_arpa")
        name = {BOS: self._names[0], EOS: self._names[1]}
        name.update({i: t for i, t in enumerate(self.tokens)})
        grams = [[] for _ in range(self.order)]
        for g in set(self._prob) | set(self._bow):
            grams[len(g) - 1].append(g)
        lines = ["\\data\\"] + [f"ngram {k + 1}={len(gs)}" for k, gs in enumerate(grams)]
        for k, gs in enumerate(grams):
            lines += ["", f"\\{k + 1}-grams:"]
            for g in sorted(gs):
                p = self._prob[g] / _LN10 if g in self._prob else -99.0
                row = f"{p:.17g}\t" + " ".join(name[w] for w in g)
                if g in self._bow:
                    row += f"\t{self._bow[g] / _LN10:.17g}"
                lines.append(row)
        return "\n".join(lines + ["", "\\end\\", ""])

    def logprob(self, ids) -> float:
        """Natural-log probability of the sequence framed by <s> and </s>, by walking the tables."""
        total, s = 0.0, self.start
        for w in ids:
            total += float(self.score[s, int(w)])
            s = int(self.next[s, int(w)])
        return total + float(self.final[s])

    def _logprob_by_definition(self, ids) -> float:
        """The same number from the raw n-grams by the back-off recursion; kept for the tests."""
        self._need_ngrams("_logprob_by_definition")

        def cond(c, w):
            if c + (w,) in self._prob:
                return self._prob[c + (w,)]
            return self._bow.get(c, 0.0) + cond(c[1:], w)
        total, hist = 0.0, [BOS]
        for w in list(ids) + [EOS]:
            w = int(w)
            total += cond(tuple(hist[max(0, len(hist) - (self.order - 1)):]) if self.order > 1 else (), w)
            hist.append(w)
        return total

    def host_tables(self, lm_weight):
        """(W = lm_weight * score, next, Wf = lm_weight * final, start) as numpy arrays: the one place the weight is applied."""
        w = float(lm_weight)
        if not math.isfinite(w):
            raise ValueError(f"NGramLM: lm_weight must be finite, not {lm_weight}")
        if w not in self._host:
            self._host[w] = (w * self.score, self.next, w * self.final, self.start)
        return self._host[w]

    def device_tables(self, lm_weight, device):
        """(W fp64 [C][V], next int32 [C][V], Wf fp64 [C], C, start) with W and Wf on `device`, multiplied once on the host in
        fp64 and cached per (weight, device)."""
        import torch
        W, nxt, Wf, start = self.host_tables(lm_weight)
        key = (float(lm_weight), str(torch.device(device)))
        if key not in self._device:
            self._device[key] = (torch.from_numpy(W).to(device), torch.from_numpy(nxt).to(device), torch.from_numpy(Wf).to(device))
        return self._device[key] + (self.n_states, start)
