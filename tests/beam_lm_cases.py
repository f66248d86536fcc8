"""Inputs of the language-model beam search tests: the emissions of tests/beam_cases.py, each paired with a seeded random n-gram
that goes through generated ARPA text and NGramLM.from_arpa, so the real reader is in the loop.  tests/test_cpu_beam_lm.py
qualifies them with the oracle's `stats` (the seeds were picked on the CPU); tests/test_gpu_beam_lm.py decodes them on the device.
Bigrams for V = 46 and V = 200, trigrams for V <= 12, weight 0.8; one case has a negative weight, one an order-1 model."""
import collections
import functools

import numpy as np

import beam_cases
from aptai_amd import hostlogic
from aptai_amd.ngram import NGramLM

LMCase = collections.namedtuple("LMCase", "name case order seed lm_weight")


def token_names(V, blank, sil):
    return ["(blank)" if i == blank else "(...)" if i == sil else f"p{i}" for i in range(V)]


def random_arpa(seed, names, blank, order, keep=(1.0, 0.5, 0.3)):
    """ARPA text of a random back-off model over the non-blank `names`: every unigram, a `keep[k]` share of the k+1-grams whose
    context is listed (so that the higher orders back off on most queries), log10 values of 6 decimals as in a real file, back-off
    weights on about three contexts in four (a missing one is 0)."""
    rs = np.random.RandomState(seed)
    words = [n for i, n in enumerate(names) if i != blank]
    level = [("<s>",)] + [(w,) for w in words] + [("</s>",)]
    lines, heads = ["\\data\\"], []
    body = []
    for k in range(order):
        rows = []
        for g in level:
            p = -99.0 if g[-1] == "<s>" else -(0.1 + 2.9 * rs.rand())
            row = f"{p:.6f}\t" + " ".join(g)
            if k + 1 < order and g[-1] != "</s>" and rs.rand() < 0.75:
                row += f"\t{-1.5 * rs.rand():.6f}"
            rows.append(row)
        heads.append(f"ngram {k + 1}={len(rows)}")
        body += ["", f"\\{k + 1}-grams:"] + rows
        if k + 1 < order:
            ctx = [g for g in level if g[-1] != "</s>"]
            level = [g + (w,) for g in ctx for w in words + ["</s>"] if rs.rand() < keep[k + 1]]
    return "\n".join(lines + heads + body + ["", "\\end\\", ""])


_BASE = {c.name: c for c in beam_cases.CASES}
_PLAN = (
    ("ref46-max", 2, 101, 0.8), ("ref46-logadd", 2, 102, 0.8), ("beam32", 3, 103, 0.8), ("tokbeam", 2, 104, 0.8),
    ("v4-max", 3, 225, 0.8), ("v4-logadd", 3, 409, -0.6), ("v3", 3, 488, 0.8), ("short", 1, 108, 0.8), ("beam1", 3, 109, 0.8),
)
CASES = tuple(LMCase(f"{name}-lm{order}", _BASE[name], order, seed, w) for name, order, seed, w in _PLAN)
CASE_IDS = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def model(name):
    """The case's NGramLM, read from its generated ARPA text.  One per process; do not modify."""
    c = CASES[CASE_IDS.index(name)]
    names = token_names(c.case.em.shape[2], c.case.blank, c.case.sil)
    return NGramLM.from_arpa(random_arpa(c.seed, names, c.case.blank, c.order), names, blank=c.case.blank)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Per row of the case: (hypotheses, stats) of hostlogic.ctc_beam_search with the case's model.  Computed once per process."""
    c = CASES[CASE_IDS.index(name)]
    out = []
    for b, length in enumerate(c.case.lens):
        stats = {}
        hyps = hostlogic.ctc_beam_search(c.case.em[b, :length], c.case.blank, c.case.sil, stats=stats, lm=model(name),
                                         lm_weight=c.lm_weight, **c.case.opts)
        out.append((hyps, stats))
    return out
