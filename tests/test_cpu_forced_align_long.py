"""CPU: the host statement of long-form forced alignment (hostlogic.long_form_force_align) and the C ABI of the wide Viterbi
(include/aptai_hip.h read through aptai_amd/_abi.py, as tests/test_cpu_abi.py does for the rest)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from aptai_amd import _abi, hostlogic

CK, CS = (10, 3, 3, 3, 3, 2, 2), (5, 2, 2, 2, 2, 2, 2)
PLAN = dict(window_frames=24, hop_frames=16, trim_frames=2)


def _windows(rng, plan, C, integer=False):
    return [rng.integers(0, 3, (n, C)).astype(np.float32) if integer else rng.standard_normal((n, C)).astype(np.float32) * 2
            for n in plan.window_len]


def _distinct(rng, n, C):
    out = rng.integers(1, C, n)
    for k in range(1, n):
        while out[k] == out[k - 1]:
            out[k] = rng.integers(1, C)
    return out


@pytest.mark.parametrize("frames, kind, integer", [(24, "linear", False), (25, "linear", False), (72, "linear", True),
                                                   (61, "cut", False), (72, "cut", True)])
def test_it_is_stitching_followed_by_the_alignment(frames, kind, integer):
    rng = np.random.default_rng(frames)
    plan = hostlogic.long_form_plan(400 + 320 * (frames - 1), CK, CS, **PLAN)
    assert plan.frames == frames
    wins = _windows(rng, plan, 9, integer)
    wins = [np.concatenate([w, np.full((2, 9), 3e30, np.float32)]) for w in wins]          # rows a window does not own are ignored
    tg = _distinct(rng, 11, 9)
    tg[4] = tg[3]                                                                          # one repeat: a blank is forced between
    ramp = hostlogic.long_form_ramp(plan, kind)
    stitched, _ = hostlogic.long_form_stitch(wins, plan, ramp)
    want_ft, want_score = hostlogic.ctc_forced_align(stitched, frames, tg, blank=0)
    for r in (kind, ramp):                                                                 # the kind or its table
        ft, spans, score, logits = hostlogic.long_form_force_align(wins, plan, r, tg.tolist(), blank=0)
        assert ft.dtype == np.int32 and ft.shape == (frames,) and np.array_equal(ft, want_ft) and score == want_score
        assert np.array_equal(spans, hostlogic.alignment_spans(want_ft, 11)) and spans.shape == (11, 2)
        assert logits.dtype == np.float32 and np.array_equal(logits.view(np.int32), stitched.view(np.int32))
    assert np.isfinite(want_score)
    # a blank other than 0
    ft7, _, score7, _ = hostlogic.long_form_force_align(wins, plan, kind, np.where(tg == 7, 0, tg), blank=7)
    assert np.array_equal(ft7, hostlogic.ctc_forced_align(stitched, frames, np.where(tg == 7, 0, tg), blank=7)[0]) and np.isfinite(score7)
    with pytest.raises(ValueError, match="windows"):
        hostlogic.long_form_force_align(wins[:-1] if plan.K else wins + wins, plan, kind, tg)


def test_a_300_label_transcript_collapses_to_itself_and_beats_random_paths():
    rng = np.random.default_rng(300)
    C, L, W, hop = 46, 300, 100, 80
    frames = 500
    plan = hostlogic.long_form_plan(400 + 320 * (frames - 1), CK, CS, window_frames=W, hop_frames=hop, trim_frames=3)
    assert plan.frames == frames and plan.K == 5
    wins = _windows(rng, plan, C)
    tg = rng.integers(1, C, L)
    tg[10:14] = tg[10]                                                                     # repeats, which need their blanks
    ft, spans, score, logits = hostlogic.long_form_force_align(wins, plan, "linear", tg)
    assert np.isfinite(score) and (ft >= -1).all()
    tok = ft[ft >= 0]
    first = np.concatenate([[True], tok[1:] != tok[:-1]])
    assert np.array_equal(tok[first], np.arange(L)) and np.array_equal(tg[tok[first]], tg)
    assert (spans[:, 0] < spans[:, 1]).all() and (spans[1:, 0] >= spans[:-1, 1]).all()
    # 200 valid paths of the same lattice, drawn at random: dwell times over the states the path visits
    x64 = logits.astype(np.float64)
    lp = x64 - (x64.max(1) + np.log(np.exp(x64 - x64.max(1, keepdims=True)).sum(1)))[:, None]
    ext = np.zeros(2 * L + 1, dtype=np.int64)
    ext[1::2] = tg
    need = np.ones(2 * L + 1, dtype=bool)                                                  # every label; a blank only between equal labels
    need[0::2] = False
    need[2:-1:2] = tg[1:] == tg[:-1]
    best_random = -np.inf
    for _ in range(200):
        visit = need | ((rng.random(2 * L + 1) < 0.2) & (np.arange(2 * L + 1) % 2 == 0))
        states = np.nonzero(visit)[0]
        if len(states) > frames:
            visit = need
            states = np.nonzero(visit)[0]
        cuts = np.sort(rng.choice(np.arange(1, frames), len(states) - 1, replace=False))
        dwell = np.diff(np.concatenate([[0], cuts, [frames]]))
        path = np.repeat(states, dwell)
        assert len(path) == frames and set(np.diff(path).tolist()) <= {0, 1, 2}
        best_random = max(best_random, float(lp[np.arange(frames), ext[path]].sum()))
    assert score >= best_random - 1e-9 * abs(score), (score, best_random)


def test_the_header_declares_the_wide_entry_points():
    abi = _abi.header()
    assert abi.constants["APTAI_CTC_VITERBI_WIDE_MAX_LABELS"] == 8191
    P, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    narrow = abi.prototypes["aptai_ctc_viterbi"]
    assert abi.prototypes["aptai_ctc_viterbi_wide"] == narrow == (I, [P, I64, I64, P, I64, P, P, P, I64, I64, I64, I, I, P, P, P, P, P, P])
    assert abi.prototypes["aptai_ctc_viterbi_wide_workspace_bytes"] == (I64, [I64, I64, I64])
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "aptai_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+aptai_ctc_viterbi_wide\s*\(([^()]*)\)\s*;", text)
    assert m and m.group(1).count(",") + 1 == 19
    names = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert names[:5] == ["logits", "ldl", "rows_per_b", "targets", "ldt"] and names[12:] == ["topology", "workspace", "frame_token", "spans",
                                                                                             "score", "token_score", "stream"]
    from aptai_amd import _lib
    assert {"aptai_ctc_viterbi_wide", "aptai_ctc_viterbi_wide_workspace_bytes"} <= set(_lib.declared_symbols())
    L = _lib.lib()
    assert L.aptai_ctc_viterbi_wide.argtypes == _lib.ARGTYPES["aptai_ctc_viterbi_wide"]
    # the size function needs no device: lz, then two bits per state in rows of whole words
    assert L.aptai_ctc_viterbi_wide_workspace_bytes(1, 15000, 4000) == 15000 * 4 + 15000 * ((8001 + 15) // 16) * 4
    assert L.aptai_ctc_viterbi_wide_workspace_bytes(3, 5, 1) == 64 + 3 * 5 * 4
