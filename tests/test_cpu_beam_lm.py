"""hostlogic.ctc_beam_search with a language model, as the oracle of aptai_ctc_beam_search_lm: against a brute force over every
frame path, unchanged without an LM, bit-equal to the plain search with an all-zero model; then the inputs of
tests/beam_lm_cases.py (what tests/test_gpu_beam_lm.py decodes on the device) are qualified with the oracle's `stats`.  As in
tests/test_cpu_beam_search.py the 1e-9 bound is a condition on the INPUTS, not a tolerance."""
import itertools

import numpy as np
import pytest

import beam_cases
import beam_lm_cases
from aptai_amd import hostlogic
from aptai_amd.ngram import NGramLM


def _brute_force(em, blank, sil, sil_score, W, nxt, Wf, start):
    """Every frame path scored by the rule of the search: history -> [(score, tokens, timesteps)], one entry per path."""
    T, V = em.shape
    groups = {}
    for path in itertools.product(range(V), repeat=T):
        score, hist, state, prev, flag = 0.0, (), start, sil, False
        for t, n in enumerate(path):
            sc = score + em[t, n] + (sil_score if n == sil else 0.0)
            if n != blank and (n != prev or flag):
                sc = sc + W[state, n]
                hist, state = hist + (n,), int(nxt[state, n])
            score, prev, flag = sc, n, n == blank
        score = score + Wf[state]
        row = np.asarray((sil,) + path + (sil,))
        keep = np.ones(len(row), dtype=bool)
        keep[1:] = row[1:] != row[:-1]
        keep &= row != blank
        groups.setdefault(hist, []).append((float(score), tuple(row[keep]), tuple(np.nonzero(keep)[0])))
    return groups


@pytest.mark.parametrize("T,seed,weight,sil_score", [(5, 1, 0.8, 0.0), (4, 2, -0.7, 0.25), (3, 3, 0.8, -0.5), (1, 4, 1.0, 0.0)])
def test_oracle_equals_the_brute_force_over_all_paths(T, seed, weight, sil_score):
    V, blank, sil = 3, 0, 1
    names = beam_lm_cases.token_names(V, blank, sil)
    lm = NGramLM.from_arpa(beam_lm_cases.random_arpa(seed, names, blank, 3, keep=(1.0, 0.7, 0.5)), names)
    em = beam_cases.iid(seed + 10, T, V, 1.0).astype(np.float64)
    groups = _brute_force(em, blank, sil, sil_score, *lm.host_tables(weight))
    big = dict(beam_size=10 ** 6, beam_threshold=1e9, nbest=10 ** 6, sil_score=sil_score, lm=lm, lm_weight=weight)
    got = hostlogic.ctc_beam_search(em, blank, sil, log_add=False, **big)
    want = sorted((max(g) for g in groups.values()), reverse=True)
    assert len(got) == len(want)
    for (tok, ts, sc), (wsc, wtok, wts) in zip(got, want):                     # max mode: the best path of every history, exactly
        assert sc == wsc and tuple(tok) == wtok and tuple(ts) == wts
    got = hostlogic.ctc_beam_search(em, blank, sil, log_add=True, **big)
    want = sorted((float(np.logaddexp.reduce([p[0] for p in g])) for g in groups.values()), reverse=True)
    assert len(got) == len(want)
    assert max(abs(h[2] - w) for h, w in zip(got, want)) <= 1e-12


def test_empty_utterance_scores_the_final_of_the_start_state():
    lm = beam_lm_cases.model("v3-lm3")
    (tok, ts, sc), = hostlogic.ctc_beam_search(np.zeros((0, 3)), 0, 1, lm=lm, lm_weight=0.8)
    assert list(tok) == [1] and list(ts) == [0] and sc == lm.host_tables(0.8)[2][lm.start]


@pytest.mark.parametrize("name", beam_cases.CASE_IDS)
def test_without_a_model_nothing_changes_and_a_zero_model_is_the_plain_search(name):
    case = beam_cases.CASES[beam_cases.CASE_IDS.index(name)]
    V = case.em.shape[2]
    zero = NGramLM(np.zeros((2, V)), np.tile(np.asarray([[1], [0]], dtype=np.int32), (1, V)), np.zeros(2), start=1, blank=case.blank)
    for b, (hyps, stats) in enumerate(beam_cases.oracle(name)):
        em = case.em[b, :case.lens[b]]
        s_none, s_zero = {}, {}
        none = hostlogic.ctc_beam_search(em, case.blank, case.sil, stats=s_none, lm=None, lm_weight=0.3, **case.opts)
        fused = hostlogic.ctc_beam_search(em, case.blank, case.sil, stats=s_zero, lm=zero, lm_weight=0.8, **case.opts)
        assert s_none == stats and set(s_none) == {"min_decision_gap", "revived_histories", "max_merge"}
        assert set(s_zero) == set(stats) | {"best_not_from_slot0"} and s_zero["best_not_from_slot0"] == 0
        for other in (none, fused):
            assert len(other) == len(hyps)
            for (t0, p0, s0), (t1, p1, s1) in zip(other, hyps):
                assert np.array_equal(t0, t1) and np.array_equal(p0, p1) and s0 == s1 and np.float64(s0).tobytes() == np.float64(s1).tobytes()


@pytest.mark.parametrize("name", beam_lm_cases.CASE_IDS)
def test_the_inputs_qualify(name):
    c = beam_lm_cases.CASES[beam_lm_cases.CASE_IDS.index(name)]
    rows = beam_lm_cases.oracle(name)
    for b, (hyps, stats) in enumerate(rows):
        assert len(hyps) >= 1
        assert stats["min_decision_gap"] >= 1e-9, (name, b, stats)
        assert 1 <= stats["max_merge"] <= 3, (name, b, stats)
    if c.case.opts["beam_size"] > 1 and c.case.em.shape[1] > 2:
        assert any(st["best_not_from_slot0"] >= 1 for _, st in rows), name
    if c.case.small_vocab:
        assert all(st["revived_histories"] >= 1 for _, st in rows), name


def test_the_cases_cover_what_they_are_there_for():
    by = {c.name: c for c in beam_lm_cases.CASES}
    assert len(by) == len(beam_cases.CASES) and {c.case.name for c in by.values()} == set(beam_cases.CASE_IDS)
    for c in by.values():
        V, lm = c.case.em.shape[2], beam_lm_cases.model(c.name)
        assert lm.n_tokens == V and lm.order == c.order and lm.blank == c.case.blank
        assert c.order == 2 if V in (46, 200) and c.name != "short-lm1" else c.order in (1, 3)
        assert c.order < 3 or V <= 12
        assert c.order == 1 or 1 < lm.n_states < 1 + V + V * V          # random subsets of the n-grams: back-off happens
    assert sorted(c.lm_weight for c in by.values()) == [-0.6] + [0.8] * 8
    assert by["short-lm1"].order == 1 and beam_lm_cases.model("short-lm1").n_states == 1
    changed = total = 0
    for c in by.values():                                    # the model changes the top hypothesis on at least half the rows
        for (hyps, _), (plain, _) in zip(beam_lm_cases.oracle(c.name), beam_cases.oracle(c.case.name)):
            total += 1
            changed += not (np.array_equal(hyps[0][0], plain[0][0]) and np.array_equal(hyps[0][1], plain[0][1]))
    assert total == 26 and 2 * changed >= total, (changed, total)


def test_the_training_script_has_the_flags_and_refuses_them_without_the_beam_decoder(tmp_path):
    from aptai_amd import train_phoneme_recognizer as tpr
    a = tpr.parse_args(["--decoder", "beam", "--lm_order", "2", "--lm_weight", "0.5"])
    assert (a.lm_arpa, a.lm_order, a.lm_weight) == (None, 2, 0.5)
    a = tpr.parse_args(["--decoder", "beam", "--lm_arpa", "x.arpa"])
    assert (a.lm_arpa, a.lm_order, a.lm_weight) == ("x.arpa", None, None)
    a = tpr.parse_args([])
    assert (a.lm_arpa, a.lm_order, a.lm_weight) == (None, None, None)
    for argv in (["--lm_order", "2"], ["--lm_arpa", "x.arpa"], ["--lm_weight", "0.5"], ["--decoder", "flashlight", "--lm_order", "2"],
                 ["--decoder", "beam", "--lm_weight", "0.5"], ["--decoder", "beam", "--lm_order", "2", "--lm_arpa", "x.arpa"]):
        with pytest.raises(SystemExit):
            tpr.parse_args(argv)
    # --lm_order estimates from the training items' labels; --lm_arpa reads the file: the same model after the round trip
    vocab = tpr.default_vocab(12)
    data = tpr.SyntheticCommonPhone(6, 1.0, len(vocab), seed=1)
    lm = tpr.language_model(tpr.parse_args(["--decoder", "beam", "--lm_order", "2"]), vocab, data)
    assert lm.order == 2 and lm.n_tokens == 12 and lm.blank == 0 and abs(np.exp(lm.score[:, 1:]).sum(axis=1) + np.exp(lm.final) - 1).max() <= 1e-12
    path = tmp_path / "lm.arpa"
    path.write_text(lm.to_arpa())
    back = tpr.language_model(tpr.parse_args(["--decoder", "beam", "--lm_arpa", str(path)]), vocab, data)
    assert np.array_equal(back.next, lm.next) and np.abs(back.score - lm.score).max() <= 1e-12
    assert tpr.language_model(tpr.parse_args([]), vocab, data) is None
