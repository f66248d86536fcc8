"""Inputs of the CTC beam search tests, shared by tests/test_cpu_beam_search.py (which qualifies them: no decision of the oracle
rests on a score difference below 1e-9, the small vocabularies revive pruned histories, one case merges three candidates) and
tests/test_gpu_beam_search.py (which decodes them on the device).  Emissions come from fixed RandomState seeds that were picked on
the CPU with the oracle's `stats`; every row of a case is decoded in ONE launch, each with its own length."""
import collections
import functools

import numpy as np

from aptai_amd import hostlogic

Case = collections.namedtuple("Case", "name em lens ldl rows_per_b blank sil opts small_vocab")


def iid(seed, T, V, scale):
    return (np.random.RandomState(seed).randn(T, V) * scale).astype(np.float32)


def peaky(seed, T, V, blank, scale=1.0):
    """A random label path with runs and blanks, +4 on the path's token: repeats and blank merges on every other frame."""
    rs = np.random.RandomState(seed)
    em = rs.randn(T, V) * scale
    tok = blank
    for t in range(T):
        u = rs.rand()
        if u < 0.3:
            tok = blank
        elif u >= 0.65 or tok == blank:
            tok = int(rs.randint(V))
        em[t, tok] += 4.0
    return em.astype(np.float32)


def _case(name, rows, T, V, ldl, blank, sil, small_vocab=False, rows_per_b=None, **opts):
    """rows: (kind, seed, scale, length).  Frames at and past a row's length hold other random values: they must not be read."""
    em = np.zeros((len(rows), T, V), dtype=np.float32)
    for b, (kind, seed, scale, length) in enumerate(rows):
        em[b] = iid(seed + 1000, T, V, 3.0)
        em[b, :length] = (iid(seed, T, V, scale) if kind == "iid" else peaky(seed, T, V, blank, scale))[:length]
    o = dict(beam_size=10, beam_size_token=None, beam_threshold=50.0, log_add=False, sil_score=0.0, nbest=1)
    o.update(opts)
    return Case(name, em, tuple(r[3] for r in rows), ldl, rows_per_b or T, blank, sil, o, small_vocab)


def _both(name, *args, **kw):
    return [_case(f"{name}-max", *args, log_add=False, **kw), _case(f"{name}-logadd", *args, log_add=True, **kw)]


CASES = (
    # the reference's settings, padded pitch
    _both("ref46", [("iid", 11, 1.0, 37), ("peaky", 12, 1.0, 37), ("iid", 13, 3.0, 30)], 37, 46, 64, 0, 45, nbest=4)
    # maximum beam, floor pruning, nbest = beam
    + [_case("beam32", [("iid", 21, 1.0, 64), ("peaky", 22, 1.0, 64), ("iid", 23, 0.5, 51)], 64, 12, 12, 3, 7,
             beam_size=32, beam_threshold=2.5, log_add=True, sil_score=-0.75, nbest=32)]
    # token beam, V wider than one wave
    + [_case("tokbeam", [("iid", 31, 1.0, 23), ("peaky", 32, 1.0, 23), ("iid", 33, 2.0, 17)], 23, 200, 256, 0, 199,
             beam_size=8, beam_size_token=7, beam_threshold=4.0, log_add=True, sil_score=0.5, nbest=4)]
    # small vocabularies: a history leaves the beam and is reached again
    + _both("v4", [("iid", 41, 1.0, 24), ("iid", 42, 1.0, 24), ("peaky", 43, 1.0, 24)], 24, 4, 4, 0, 1, small_vocab=True,
            beam_size=8, nbest=8)
    + [_case("v3", [("iid", 51, 1.0, 16), ("iid", 52, 1.0, 16), ("peaky", 53, 0.5, 16)], 16, 3, 8, 0, 1, small_vocab=True,
             beam_size=6, log_add=True, nbest=6)]
    # fewer hypotheses than nbest: two states of the empty history merge at the end (row 0), the floor leaves few (row 2)
    + [_case("short", [("iid", 69, 1.0, 1), ("iid", 62, 1.0, 2), ("iid", 63, 30.0, 2)], 2, 46, 64, 0, 45, nbest=10)]
    # beam 1, threshold 0: the framed best path
    + [_case("beam1", [("iid", 71, 1.0, 12), ("peaky", 72, 1.0, 12)], 12, 5, 8, 0, 1, beam_size=1, beam_threshold=0.0, nbest=1)]
)
CASE_IDS = [c.name for c in CASES]


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Per row of the case: (hypotheses, stats) of hostlogic.ctc_beam_search.  Computed once per process; do not modify."""
    case = CASES[CASE_IDS.index(name)]
    out = []
    for b, length in enumerate(case.lens):
        stats = {}
        hyps = hostlogic.ctc_beam_search(case.em[b, :length], case.blank, case.sil, stats=stats, **case.opts)
        out.append((hyps, stats))
    return out
