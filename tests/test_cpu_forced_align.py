"""Forced alignment on the host (no GPU): hostlogic.ctc_forced_align against exhaustive enumeration, the tie rule clause by
clause, and the span / blank-filling helpers on written-out examples."""
import itertools
import re

import numpy as np
import pytest

from aptai_amd import hostlogic


def _log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=1, keepdims=True))


def _valid(pi, targets, blank, topology):
    """Is the frame labelling `pi` an alignment of `targets`?"""
    if topology == "ctc":
        col = [p for i, p in enumerate(pi) if i == 0 or p != pi[i - 1]]
        return [p for p in col if p != blank] == list(targets)
    pat = "".join(f"{chr(97 + t)}+" for t in targets)                  # l1+ l2+ ... lL+
    return len(targets) > 0 and re.fullmatch(pat, "".join(chr(97 + p) for p in pi)) is not None


def _brute(x, targets, blank, topology):
    lp = _log_softmax64(x)
    T, V = lp.shape
    best = -np.inf
    for pi in itertools.product(range(V), repeat=T):
        if _valid(pi, targets, blank, topology):
            best = max(best, float(lp[np.arange(T), list(pi)].sum()))
    return best


def _labels(ft, targets, blank):
    t = np.asarray(list(targets) + [blank], dtype=np.int64)
    return np.where(ft >= 0, t[np.clip(ft, 0, None)], blank)


@pytest.mark.parametrize("topology", ["ctc", "monotonic"])
def test_matches_exhaustive_enumeration(topology):
    rng = np.random.RandomState(5 if topology == "ctc" else 6)
    V, blank = 3, 0
    seen_feasible = seen_infeasible = 0
    for case in range(60):
        T = int(rng.randint(1, 7))
        L = int(rng.randint(0, 5))
        lo = 1 if topology == "ctc" else 0
        targets = [int(v) for v in rng.randint(lo, V, size=L)]
        x = rng.randn(T, V) * 2.0                                       # float64 run
        ft, score = hostlogic.ctc_forced_align(x, T, targets, blank=blank, topology=topology)
        want = _brute(x, targets, blank, topology)
        assert ft.dtype == np.int32 and ft.shape == (T,)
        if want == -np.inf:
            seen_infeasible += 1
            assert score == -np.inf and (ft == -2).all(), (case, T, targets)
            continue
        seen_feasible += 1
        assert abs(score - want) <= 1e-12, (case, T, targets, score, want)
        pi = _labels(ft, targets, blank)
        assert _valid([int(p) for p in pi], targets, blank, topology)
        assert abs(float(_log_softmax64(x)[np.arange(T), pi].sum()) - want) <= 1e-12
    assert seen_feasible >= 15 and seen_infeasible >= 5


def test_infeasible_and_length_conventions():
    x = np.zeros((4, 3), dtype=np.float32)
    ft, score = hostlogic.ctc_forced_align(x, 2, [1, 2, 1], blank=0)             # three labels, two frames
    assert score == -np.inf and ft.tolist() == [-2, -2, -2, -2]
    ft, score = hostlogic.ctc_forced_align(x, 4, [1, 7], blank=0)                # a label outside the vocabulary
    assert score == -np.inf and (ft == -2).all()
    ft, score = hostlogic.ctc_forced_align(x, 0, [1], blank=0)
    assert score == -np.inf and (ft == -2).all()
    ft, score = hostlogic.ctc_forced_align(x, 0, [], blank=0)
    assert score == 0.0 and (ft == -2).all()
    ft, score = hostlogic.ctc_forced_align(x, 3, [1], blank=0)                   # frames beyond the length are -2
    assert ft[3] == -2 and (ft[:3] != -2).all() and np.isfinite(score)
    ft, score = hostlogic.ctc_forced_align(x, 3, [], topology="monotonic")       # no label can own the frames
    assert score == -np.inf and (ft == -2).all()
    with pytest.raises(ValueError):
        hostlogic.ctc_forced_align(x, 3, [1], topology="star")


# ---- the tie rule, one clause per case; every expected path is written out
def test_tie_stay_beats_equal_previous_state():
    # monotonic, two labels, three frames, all logits equal: switching at frame 1 or at frame 2 scores the same.  At frame 2 state 1
    # compares stay (0) with its s-1 predecessor (0): the tie keeps STAY, so the switch happened at frame 1.
    x = np.zeros((3, 3), dtype=np.float32)
    ft, _ = hostlogic.ctc_forced_align(x, 3, [1, 2], topology="monotonic")
    assert ft.tolist() == [0, 1, 1]


def test_tie_previous_state_beats_equal_skip():
    # CTC, labels 1 2, states b 1 b 2 b.  At frame 2 state 3 (label 2) sees stay = -9, s-1 (blank, state 2) = 0 and
    # s-2 (label 1, state 1) = 0: s-1 replaces stay (strictly greater), s-2 does NOT replace s-1 (equal) -> frame 1 is blank.
    x = np.array([[-5, 0, -5], [0, 0, -9], [-9, -9, 0]], dtype=np.float32)
    ft, _ = hostlogic.ctc_forced_align(x, 3, [1, 2], blank=0)
    assert ft.tolist() == [0, -1, 1]


def test_tie_final_state_is_the_last_unless_the_one_before_is_strictly_greater():
    # CTC, one label, two frames: the paths (1, blank) and (1, 1) tie -> the path ends in the LAST state (the trailing blank)
    x = np.array([[-5, 0], [0, 0]], dtype=np.float32)
    ft, _ = hostlogic.ctc_forced_align(x, 2, [1], blank=0)
    assert ft.tolist() == [0, -1]
    # ... and with the label strictly better at frame 1 it ends in the state before the last
    x = np.array([[-5, 0], [-1, 0]], dtype=np.float32)
    ft, _ = hostlogic.ctc_forced_align(x, 2, [1], blank=0)
    assert ft.tolist() == [0, 0]


def test_strictly_greater_predecessors_replace():
    # CTC, labels 1 2, blank never attractive: the skip transition (s-2) must be taken between frames 0 and 1
    x = np.array([[-9, 0, -9], [-9, -9, 0]], dtype=np.float32)
    ft, _ = hostlogic.ctc_forced_align(x, 2, [1, 2], blank=0)
    assert ft.tolist() == [0, 1]


def test_repeated_label_needs_a_blank_between():
    x = np.array([[-9, 0], [-9, 0], [-9, 0]], dtype=np.float32)          # blank is never attractive, and still required
    ft, score = hostlogic.ctc_forced_align(x, 3, [1, 1], blank=0)
    assert ft.tolist() == [0, -1, 1] and np.isfinite(score)
    ft, score = hostlogic.ctc_forced_align(x, 2, [1, 1], blank=0)        # two frames cannot hold a a
    assert score == -np.inf and ft.tolist() == [-2, -2, -2]
    ft, score = hostlogic.ctc_forced_align(x, 2, [1, 1], topology="monotonic")   # without blank they can
    assert ft.tolist() == [0, 1, -2] and np.isfinite(score)


def test_empty_transcript_is_all_blank():
    rng = np.random.RandomState(0)
    x = rng.randn(7, 4).astype(np.float32)
    ft, score = hostlogic.ctc_forced_align(x, 5, [], blank=2)
    assert ft.tolist() == [-1] * 5 + [-2] * 2
    assert abs(score - float(_log_softmax64(x)[:5, 2].sum())) <= 1e-12


@pytest.mark.parametrize("seed", range(6))
def test_aligning_the_best_path_decode_returns_the_frame_argmax(seed):
    rng = np.random.RandomState(100 + seed)
    T, V, blank = 499, 46, 0
    cuts = np.sort(rng.choice(np.arange(1, T), size=69, replace=False))
    bounds = np.concatenate([[0], cuts, [T]])
    x = np.empty((T, V), dtype=np.float32)
    for a, b in zip(bounds[:-1], bounds[1:]):
        row = rng.randn(V).astype(np.float32)
        planted = blank if rng.rand() < 0.3 else int(rng.randint(1, V))
        row[planted] = row.max() + 1.0                                  # a margin far above the fp32 rounding of a 499-term sum
        x[a:b] = row
    ids = hostlogic.ctc_best_path(x, T, blank)
    assert 1 <= len(ids) <= 255
    ft, score = hostlogic.ctc_forced_align(x, T, ids, blank=blank)
    assert np.isfinite(score)
    np.testing.assert_array_equal(_labels(ft, ids, blank), x.argmax(axis=1))


def test_alignment_spans_examples():
    ft = np.array([-1, 0, 0, -1, 1, 2, 2, 2, -1, -2, -2], dtype=np.int32)
    assert hostlogic.alignment_spans(ft, 4).tolist() == [[1, 3], [4, 5], [5, 8], [-1, -1]]
    assert hostlogic.alignment_spans(np.full(5, -2, dtype=np.int32), 2).tolist() == [[-1, -1], [-1, -1]]
    assert hostlogic.alignment_spans(ft, 0).shape == (0, 2)


def test_fill_blank_frames_examples():
    # leading blanks -> first token; odd run (3) between 0 and 1 -> the earlier token takes 2; even run (2) between 1 and 2 -> 1 + 1;
    # trailing blank -> last token; padding stays
    ft = np.array([-1, -1, 0, -1, -1, -1, 1, -1, -1, 2, -1, -2, -2], dtype=np.int32)
    assert hostlogic.fill_blank_frames(ft).tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 2, 2, 2, -2, -2]
    assert ft[0] == -1                                                  # the input is not modified
    # a single blank between two tokens goes to the earlier one
    assert hostlogic.fill_blank_frames([0, -1, 1]).tolist() == [0, 0, 1]
    # nothing to fill / nothing to fill from
    assert hostlogic.fill_blank_frames([0, 0, 1]).tolist() == [0, 0, 1]
    assert hostlogic.fill_blank_frames([-1, -1, -2]).tolist() == [-1, -1, -2]
    assert hostlogic.fill_blank_frames([-2, -2]).tolist() == [-2, -2]
