"""aptai_amd/ngram.py NGramLM on the CPU: the ARPA reader against tables written out by hand, the compiled automaton against the
back-off recursion on the raw n-grams (bit for bit), the refusals, and the Witten-Bell estimator (normalised, round trip through
ARPA text, unseen contexts back off)."""
import math

import numpy as np
import pytest

import beam_lm_cases
from aptai_amd.ngram import NGramLM

TOK = ["(blank)", "a", "b"]
HAND = """\\data\\
ngram 1=4
ngram 2=3
ngram 3=1

\\1-grams:
-99\t<s>\t-0.5
-1.0\t</s>
-0.5\ta\t-0.25
-0.75\tb

\\2-grams:
-0.2\t<s> a\t-0.1
-0.3\ta b\t-0.4
-0.6\tb </s>

\\3-grams:
-0.05\ta b a

\\end\\
"""
# states: 0 (), 1 (<s>), 2 (a), 3 (b), 4 (<s> a), 5 (a b); (b) has no back-off weight: 0
HAND_SCORE = [[0.0, -0.5, -0.75],
              [0.0, -0.2, -0.5 + -0.75],
              [0.0, -0.25 + -0.5, -0.3],
              [0.0, 0.0 + -0.5, 0.0 + -0.75],
              [0.0, -0.1 + (-0.25 + -0.5), -0.1 + -0.3],
              [0.0, -0.05, -0.4 + (0.0 + -0.75)]]
HAND_FINAL = [-1.0, -0.5 + -1.0, -0.25 + -1.0, -0.6, -0.1 + (-0.25 + -1.0), -0.4 + -0.6]
HAND_NEXT = [[0, 2, 3], [1, 4, 3], [2, 2, 5], [3, 2, 3], [4, 2, 5], [5, 2, 3]]


def test_reader_against_tables_written_by_hand(tmp_path):
    lm = NGramLM.from_arpa(HAND, TOK, log10=True)
    assert (lm.order, lm.n_states, lm.n_tokens, lm.start, lm.blank) == (3, 6, 3, 1, 0)
    assert lm.score.dtype == np.float64 and lm.next.dtype == np.int32 and lm.final.dtype == np.float64
    assert np.array_equal(lm.score, np.asarray(HAND_SCORE)) and np.array_equal(lm.final, np.asarray(HAND_FINAL))
    assert np.array_equal(lm.next, np.asarray(HAND_NEXT))
    path = tmp_path / "hand.arpa"
    path.write_text(HAND)
    nat = NGramLM.from_arpa(path, TOK)                       # a path, natural logarithms: every log10 value times ln 10
    assert np.array_equal(nat.next, lm.next)
    assert np.allclose(nat.score, lm.score * math.log(10.0), rtol=0, atol=1e-15)
    assert nat.score[0, 1] == -0.5 * math.log(10.0) and nat.final[3] == -0.6 * math.log(10.0)
    # <s> a b a </s>: (<s> a) listed, (<s> a b) backs off to (a b), (a b a) listed, then (b a </s>) -> (a </s>) -> bow(a) + </s>
    assert lm.logprob([1, 2, 1]) == ((-0.2 + (-0.1 + -0.3)) + -0.05) + (-0.25 + -1.0)
    assert lm.logprob([]) == -0.5 + -1.0


@pytest.mark.parametrize("name", ["ref46-max-lm2", "beam32-lm3", "v3-lm3", "short-lm1"])
def test_tables_equal_the_backoff_recursion_bit_for_bit(name):
    lm = beam_lm_cases.model(name)
    rs = np.random.RandomState(5)
    real = [w for w in range(lm.n_tokens) if w != lm.blank]
    for _ in range(200):
        ids = rs.choice(real, size=rs.randint(0, 9))
        assert lm.logprob(ids) == lm._logprob_by_definition(ids)
    assert (lm.score[:, lm.blank] == 0).all() and np.array_equal(lm.next[:, lm.blank], np.arange(lm.n_states))


def test_unk_fallback_and_the_refusals():
    with_unk = HAND.replace("ngram 1=4", "ngram 1=5").replace("-0.75\tb\n", "-0.75\tb\n-2.5\t<unk>\n")
    lm = NGramLM.from_arpa(with_unk, TOK + ["c"], log10=True)
    # c took <unk>'s unigram, which makes (c) a state of its own (4, after (b)) with no back-off weight
    assert lm.n_tokens == 4 and lm.n_states == 7
    assert (lm.score[:, 3] == [-2.5, -0.5 + -2.5, -0.25 + -2.5, -2.5, -2.5, -0.1 + (-0.25 + -2.5), -0.4 + -2.5]).all()
    assert (lm.next[:, 3] == 4).all() and np.array_equal(lm.score[4], lm.score[0]) and lm.final[4] == lm.final[0]
    with pytest.raises(ValueError, match="'c'"):             # no unigram and no <unk>
        NGramLM.from_arpa(HAND, TOK + ["c"])
    with pytest.raises(ValueError, match="no tokens"):       # an ARPA word that is no token
        NGramLM.from_arpa(HAND, ["(blank)", "a"])
    with pytest.raises(ValueError, match="finite"):
        NGramLM.from_arpa(HAND.replace("-0.3\ta b", "-inf\ta b"), TOK)
    with pytest.raises(ValueError, match="finite"):
        NGramLM.from_arpa(HAND.replace("\t-0.4", "\tnan"), TOK)
    with pytest.raises(ValueError, match="</s>"):
        NGramLM.from_arpa(HAND.replace("-1.0\t</s>\n", ""), TOK)
    six = "\\data\\\n\\1-grams:\n-1 a\n-1 </s>\n\\6-grams:\n-1 a a a a a a\n\\end\\\n"
    with pytest.raises(ValueError, match="order"):
        NGramLM.from_arpa(six, ["(blank)", "a"])
    for order in (0, 6):
        with pytest.raises(ValueError, match="order"):
            NGramLM.estimate([[1, 2]], TOK, order=order)
    many = ["(blank)"] + [f"p{i}" for i in range(1, 257)]
    with pytest.raises(ValueError, match="256"):
        NGramLM.estimate([[1, 2]], many, order=2)
    with pytest.raises(ValueError, match=r"2\*\*24"):        # C * V: 65537 states x 256 tokens (untouched zero pages)
        NGramLM(np.zeros((65537, 256)), np.zeros((1, 1), dtype=np.int32), np.zeros(65537))
    with pytest.raises(ValueError, match="blank"):
        NGramLM.estimate([[1, 0, 2]], TOK, order=2)
    z = np.zeros((2, 3))
    with pytest.raises(ValueError, match="next"):            # what the device does not check is checked here
        NGramLM(z, np.full((2, 3), 2), np.zeros(2))
    with pytest.raises(ValueError, match="finite"):
        NGramLM(np.full((2, 3), -np.inf), np.zeros((2, 3), dtype=np.int32), np.zeros(2))
    with pytest.raises(ValueError, match="no n-grams"):
        NGramLM(z, np.zeros((2, 3), dtype=np.int32), np.zeros(2)).to_arpa()


def _training_set(V, n, seed):
    rs = np.random.RandomState(seed)
    return [rs.randint(1, V, size=rs.randint(1, 12)) for _ in range(n)]


@pytest.mark.parametrize("order", [1, 2, 3, 4])
def test_estimator_is_normalised_and_survives_the_round_trip(order):
    V = 7
    tokens = ["(blank)", "(...)"] + [f"p{i}" for i in range(2, V)]
    lm = NGramLM.estimate(_training_set(V, 40, order), tokens, order=order)
    assert lm.order == order and (lm.n_states > 1) == (order > 1) and (lm.start != 0) == (order > 1)
    total = np.exp(lm.score[:, 1:]).sum(axis=1) + np.exp(lm.final)
    assert np.abs(total - 1.0).max() <= 1e-12, total
    back = NGramLM.from_arpa(lm.to_arpa(), tokens)
    assert np.array_equal(back.next, lm.next) and back.start == lm.start
    assert np.abs(back.score - lm.score).max() <= 1e-12 and np.abs(back.final - lm.final).max() <= 1e-12
    for ids in _training_set(V, 20, 99):
        assert lm.logprob(ids) == lm._logprob_by_definition(ids)


def test_estimator_by_hand_and_unseen_contexts_back_off():
    """One sentence <s> a b </s> over {a, b, c}: n = 3 unigram events of 3 types, uniform 1/4 (a, b, c, </s>)."""
    tokens = ["(blank)", "a", "b", "c"]
    lm = NGramLM.estimate([[1, 2]], tokens, order=2)
    p_a = (1 + 3 * 0.25) / (3 + 3)
    p_c = (0 + 3 * 0.25) / (3 + 3)
    assert lm.score[0, 1] == math.log(p_a) and lm.score[0, 3] == math.log(p_c) and lm.final[0] == math.log(p_a)
    a = int(lm.next[0, 1])                                   # context (a): seen once, followed by b only
    assert lm.score[a, 2] == math.log((1 + 1 * p_a) / (1 + 1))
    assert lm.score[a, 3] == math.log(1 / (1 + 1)) + math.log(p_c)              # unseen after a: bow(a) + P(c)
    c = int(lm.next[0, 3])                                   # (c) is a state, as every listed unigram, but was never a context:
    assert c not in (0, a) and lm.next[a, 3] == c            # no back-off weight, its rows are the empty context's
    assert np.array_equal(lm.score[c], lm.score[0]) and lm.final[c] == lm.final[0]


def test_weighted_tables_are_multiplied_once_and_cached():
    lm = beam_lm_cases.model("v3-lm3")
    W, nxt, Wf, start = lm.host_tables(0.8)
    assert np.array_equal(W, 0.8 * lm.score) and np.array_equal(Wf, 0.8 * lm.final) and nxt is lm.next and start == lm.start
    assert lm.host_tables(0.8)[0] is W
    dw, dn, df, C, s = lm.device_tables(0.8, "cpu")
    assert np.array_equal(dw.numpy(), W) and np.array_equal(dn.numpy(), nxt) and (C, s) == (lm.n_states, lm.start)
    assert lm.device_tables(0.8, "cpu")[0] is dw and lm.device_tables(-0.5, "cpu")[0] is not dw
    with pytest.raises(ValueError, match="finite"):
        lm.host_tables(float("nan"))
