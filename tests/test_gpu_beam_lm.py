"""CTC beam search with a fused n-gram language model on the MI355X (aptai_ctc_beam_search_lm through ops.ctc_beam_search(lm=),
i.e. the C ABI) against its oracle hostlogic.ctc_beam_search(lm=) on the inputs of tests/beam_lm_cases.py, which
tests/test_cpu_beam_lm.py qualifies: no decision of the oracle rests on a score difference below 1e-9, so hypotheses, lengths,
tokens and timesteps must be EQUAL; scores are equal bit for bit in max mode (fp64 additions in the oracle's order, the table
multiplied by the weight once on the host for both) and within 1e-9 with log_add, the bounds of tests/test_gpu_beam_search.py.
Then the recogniser with "lm" / "lm_weight" in its beam_options."""
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import beam_cases
import beam_lm_cases
from conftest import load_golden

pytestmark = pytest.mark.gpu

GUARD = -77


def _device_logits(case):
    """The batch as the kernel reads it: row b*rows_per_b + t, pitch ldl, the padding filled with large values that must not be read."""
    B, T, V = case.em.shape
    full = np.full((B, case.rows_per_b, case.ldl), 1.0e4, dtype=np.float32)
    full[:, :T, :V] = case.em
    return torch.from_numpy(full.reshape(B * case.rows_per_b, case.ldl)).cuda()


def _decode(case, **over):
    from aptai_amd import ops
    B, T, V = case.em.shape
    lens = torch.tensor(case.lens, dtype=torch.int32).cuda()
    opts = dict(case.opts)
    opts.update(over)
    return ops.ctc_beam_search(_device_logits(case), case.ldl, case.rows_per_b, B, T, V, case.blank, case.sil, input_lens_i32=lens, **opts)


def _check_row(got, b, hyps, nbest, log_add, tag):
    tokens, timesteps, n_tok, score, n_hyp = got
    assert int(n_hyp[b]) == len(hyps), (tag, b, int(n_hyp[b]), len(hyps))
    for r, (tok, ts, sc) in enumerate(hyps):
        n = int(n_tok[b, r])
        assert n == len(tok), (tag, b, r)
        assert np.array_equal(tokens[b, r, :n], tok) and np.array_equal(timesteps[b, r, :n], ts), (tag, b, r)
        assert not tokens[b, r, n:].any() and not timesteps[b, r, n:].any(), (tag, b, r, "padding")
        err = abs(float(score[b, r]) - sc)
        print(f"[beam-lm] {tag} row {b} rank {r}: score {float(score[b, r]):.12f} oracle {sc:.12f} |diff| {err:.3e}")
        if log_add:
            assert err <= 1e-9, (tag, b, r, err)
        else:
            assert float(score[b, r]) == sc, (tag, b, r, err)
    for r in range(len(hyps), nbest):
        assert int(n_tok[b, r]) == 0 and score[b, r] == -np.inf and not tokens[b, r].any() and not timesteps[b, r].any(), (tag, b, r)


@pytest.mark.parametrize("name", beam_lm_cases.CASE_IDS)
def test_beam_search_with_a_model_equals_the_oracle(name):
    c = beam_lm_cases.CASES[beam_lm_cases.CASE_IDS.index(name)]
    case = c.case
    got = [x.cpu().numpy() for x in _decode(case, lm=beam_lm_cases.model(name), lm_weight=c.lm_weight)]
    assert got[0].shape == (len(case.lens), case.opts["nbest"], case.em.shape[1] + 2) and got[3].dtype == np.float64
    for b, (hyps, _) in enumerate(beam_lm_cases.oracle(name)):
        _check_row(got, b, hyps, case.opts["nbest"], case.opts["log_add"], name)


def _zero_model(V, blank):
    """All-zero scores over two states that every token toggles: the state machinery runs, the scores cannot change."""
    from aptai_amd.ngram import NGramLM
    return NGramLM(np.zeros((2, V)), np.tile(np.asarray([[1], [0]], dtype=np.int32), (1, V)), np.zeros(2), start=1, blank=blank)


@pytest.mark.parametrize("name", ["ref46-max", "beam32", "tokbeam", "v3", "short"])
def test_zero_model_gives_the_bytes_of_the_plain_search(name):
    case = beam_cases.CASES[beam_cases.CASE_IDS.index(name)]
    plain = [x.cpu().numpy().tobytes() for x in _decode(case)]
    fused = [x.cpu().numpy().tobytes() for x in _decode(case, lm=_zero_model(case.em.shape[2], case.blank), lm_weight=0.8)]
    assert plain == fused


def test_rows_of_a_batch_equal_their_own_decode_and_the_empty_row():
    """input_lens = [T, T // 2, 0] in one launch: every row byte-equal to its single-utterance decode; T_b == 0 gives [sil] at 0 with
    score Wf[start]."""
    from aptai_amd import hostlogic, ops
    from aptai_amd.ngram import NGramLM
    T, V, ldl, blank, sil = 20, 9, 16, 0, 4
    names = beam_lm_cases.token_names(V, blank, sil)
    lm = NGramLM.from_arpa(beam_lm_cases.random_arpa(7, names, blank, 3), names)
    em = np.stack([beam_cases.iid(81, T, V, 1.0), beam_cases.peaky(82, T, V, blank), beam_cases.iid(83, T, V, 1.0)])
    lens = [T, T // 2, 0]
    opts = dict(beam_size=10, beam_threshold=50.0, log_add=True, nbest=5, lm=lm, lm_weight=0.8)

    def run(rows, lengths):
        full = np.full((len(rows), T, ldl), 1.0e4, dtype=np.float32)
        full[:, :T, :V] = rows
        li = torch.tensor(lengths, dtype=torch.int32).cuda()
        out = ops.ctc_beam_search(torch.from_numpy(full.reshape(-1, ldl)).cuda(), ldl, T, len(rows), T, V, blank, sil, input_lens_i32=li, **opts)
        return [x.cpu().numpy() for x in out]
    batch = run(em, lens)
    for b in range(3):
        alone = run(em[b:b + 1], lens[b:b + 1])
        for x, y in zip(batch, alone):
            assert x[b].tobytes() == y[0].tobytes(), b
    wf = lm.host_tables(0.8)[2][lm.start]
    assert wf != 0.0
    assert batch[4][2] == 1 and batch[2][2, 0] == 1 and batch[0][2, 0, 0] == sil and batch[1][2, 0, 0] == 0 and batch[3][2, 0] == wf
    for b in range(2):
        stats = {}
        hyps = hostlogic.ctc_beam_search(em[b, :lens[b]], blank, sil, stats=stats, **opts)
        assert stats["min_decision_gap"] >= 1e-9
        _check_row(batch, b, hyps, 5, True, "lens")


def test_same_call_twice_gives_the_same_bits():
    c = beam_lm_cases.CASES[beam_lm_cases.CASE_IDS.index("beam32-lm3")]
    first = [x.cpu().numpy().tobytes() for x in _decode(c.case, lm=beam_lm_cases.model(c.name), lm_weight=c.lm_weight)]
    assert first == [x.cpu().numpy().tobytes() for x in _decode(c.case, lm=beam_lm_cases.model(c.name), lm_weight=c.lm_weight)]


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing():
    from aptai_amd import _lib, ops
    c = beam_lm_cases.CASES[beam_lm_cases.CASE_IDS.index("v3-lm3")]
    case, lm = c.case, beam_lm_cases.model(c.name)
    B, T, V = case.em.shape
    logits = _device_logits(case)
    w, nxt, wf, C, start = lm.device_tables(c.lm_weight, logits.device)
    ws = torch.empty(_lib.lib().aptai_ctc_beam_search_workspace_bytes(B, T, 6, 6), dtype=torch.uint8, device="cuda")
    n_out, wide = B * 6 * (T + 2), 9
    outs = [torch.full((n_out + wide,), GUARD, dtype=torch.int32, device="cuda") for _ in range(4)]
    score = torch.full((B * 6 + wide,), float(GUARD), dtype=torch.float64, device="cuda")

    def call(beam=6, w_=w.data_ptr(), nxt_=nxt.data_ptr(), wf_=wf.data_ptr(), C_=C, start_=start):
        return _lib.lib().aptai_ctc_beam_search_lm(logits.data_ptr(), case.ldl, case.rows_per_b, None, B, T, V, case.blank, case.sil, beam, 0,
                                                   50.0, 1, 0.0, min(beam, 6), T + 2, ws.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                                   outs[2].data_ptr(), score.data_ptr(), outs[3].data_ptr(), w_, nxt_, wf_, C_, start_,
                                                   ops._stream())
    for kw, word in ((dict(w_=None), "null"), (dict(nxt_=None), "null"), (dict(wf_=None), "null"), (dict(C_=0), "lm_states"),
                     (dict(start_=-1), "lm_start"), (dict(start_=C), "lm_start"), (dict(C_=(1 << 24) // V + 1), "2^24"),
                     (dict(beam=33), "beam_size")):
        assert call(**kw) == -1, kw
        msg = _lib.lib().aptai_last_error().decode()
        assert "aptai_ctc_beam_search_lm" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert all((o == GUARD).all().item() for o in outs) and (score == GUARD).all().item()
    assert call() == 0
    torch.cuda.synchronize()
    assert all((o[n_out:] == GUARD).all().item() for o in outs[:2]) and (outs[2][B * 6:] == GUARD).all().item()
    assert (outs[3][B:] == GUARD).all().item() and (score[B * 6:] == GUARD).all().item() and not (score[:B * 6] == GUARD).any().item()
    kw = dict(beam_size=6, nbest=6)
    for bad in (dict(lm=beam_lm_cases.model("v4-max-lm3")), dict(lm=(w, nxt, wf)), dict(lm=lm, lm_weight=float("nan")),
                dict(lm=lm, lm_weight=float("inf"))):
        with pytest.raises(ValueError):
            ops.ctc_beam_search(logits, case.ldl, case.rows_per_b, B, T, V, case.blank, case.sil, **kw, **bad)


# ------------------------------------------------------------------------------------------------ the recogniser
@pytest.fixture(scope="module")
def pr():
    """The mini recogniser of tests/test_gpu_beam_search.py (random init, silence token 5, 2 x 1 s) and a trigram over its 40 tokens
    estimated from random label sequences."""
    from aptai_amd.config import W2V2Config
    from aptai_amd.ngram import NGramLM
    from aptai_amd.w2v2_pr import Wav2Vec2_PR
    from oracle import synth
    from safetensors.torch import save_file
    z, meta = load_golden("pr_base_mini_2x1s")
    cfg = W2V2Config.from_any(meta["cfg"])
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), meta["seed"])
    sd["pr_head.bias"][0] += 1.0
    vocab = {"(blank)": 0}
    vocab.update({("(...)" if i == 5 else f"p{i}"): i for i in range(1, 40)})
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "config.json"), "w") as f:
            json.dump(cfg.to_dict(), f)
        save_file({k[len("wav2vec2."):]: v.contiguous() for k, v in sd.items() if k.startswith("wav2vec2.")},
                  os.path.join(tmp, "model.safetensors"))
        model = Wav2Vec2_PR(cfg, None, tmp, vocab)
    model.load_state_dict(sd)
    wav = torch.randn(16000, generator=torch.Generator().manual_seed(21)).numpy()
    x = torch.from_numpy(np.stack([wav, np.roll(wav, 3000)])).cuda()
    rs = np.random.RandomState(3)
    lm = NGramLM.estimate([rs.randint(1, 40, size=rs.randint(3, 15)) for _ in range(60)], list(vocab), order=3)
    return model.cuda().eval(), wav, x, torch.tensor([16000, 12000]).cuda(), lm


def test_decode_nbest_and_predict_nbest_with_a_model_equal_the_oracle_on_the_models_logits(pr):
    from aptai_amd import hostlogic
    model, wav, x, lens, lm = pr
    full = torch.tensor([16000, 16000]).cuda()
    res = model.decode_nbest(x, full, nbest=3, log_add=True, lm=lm, lm_weight=0.8)
    emb = model.get_embeddings(x, full)
    got = [res[k].cpu().numpy() for k in ("tokens", "timesteps", "n_tok", "score", "n_hyp")]
    kw = dict(beam_size=10, beam_threshold=50.0, log_add=True, nbest=3, lm=lm, lm_weight=0.8)
    for b in range(2):
        stats = {}
        hyps = hostlogic.ctc_beam_search(emb["phoneme_logits"][b].T, 0, 5, stats=stats, **kw)
        assert stats["min_decision_gap"] >= 1e-9, stats
        _check_row(got, b, hyps, 3, True, "model")
    one = model.predict_nbest(wav, model.vocab, nbest=3, log_add=True, lm=lm, lm_weight=0.8)
    lg = model.get_ctc_logits(wav)
    stats = {}
    hyps = hostlogic.ctc_beam_search(lg, 0, 5, stats=stats, **kw)
    assert stats["min_decision_gap"] >= 1e-9, stats
    assert len(one) == len(hyps) == 3
    for h, (tok, ts, sc) in zip(one, hyps):
        assert list(h["phn_seq_idx"]) == list(tok) and abs(h["score"] - sc) <= 1e-9
        assert np.array_equal(np.asarray(h["phn_seq_dur"]), np.asarray([int(t) * (len(wav) / lg.shape[0] / 16000) for t in ts]))


def test_beam_options_with_a_model_feed_the_decodes_and_removing_them_restores_the_outputs(pr):
    from aptai_amd import hostlogic
    model, wav, x, lens, lm = pr
    full = torch.tensor([16000, 16000]).cuda()
    try:
        model.decoder = "beam"
        before = model.get_embeddings(x, full)["phn_pred_seq_idx"]
        before_dur = model.predict_phonemes_durations(wav, model.vocab)
        model.beam_options = dict(type(model).beam_options, lm=lm, lm_weight=2.0)
        emb = model.get_embeddings(x, full)
        differ = 0
        for b in range(2):
            stats = {}
            (tok, ts, _), = hostlogic.ctc_beam_search(emb["phoneme_logits"][b].T, 0, 5, stats=stats, lm=lm, lm_weight=2.0)
            assert stats["min_decision_gap"] >= 1e-9, stats
            assert list(emb["phn_pred_seq_idx"][b]) == list(tok)
            differ += list(tok) != list(before[b])
        assert differ >= 1                                   # at this weight the model changes what the recogniser returns
        dur = model.predict_phonemes_durations(wav, model.vocab)
        lg = model.get_ctc_logits(wav)
        (tok, ts, _), = hostlogic.ctc_beam_search(lg, 0, 5, lm=lm, lm_weight=2.0)
        assert list(dur["phn_seq_idx"]) == list(tok)
        assert np.array_equal(np.asarray(dur["phn_seq_dur"]), np.asarray([int(t) * (len(wav) / lg.shape[0] / 16000) for t in ts]))
        del model.beam_options                               # back to the class default: today's outputs, bit for bit
        assert model.beam_options == {"beam_size": 10, "beam_threshold": 50.0, "log_add": False, "nbest": 1}
        after = model.get_embeddings(x, full)["phn_pred_seq_idx"]
        assert all(list(a) == list(b) for a, b in zip(after, before))
        after_dur = model.predict_phonemes_durations(wav, model.vocab)
        assert list(after_dur["phn_seq_idx"]) == list(before_dur["phn_seq_idx"])
        assert np.array_equal(np.asarray(after_dur["phn_seq_dur"]), np.asarray(before_dur["phn_seq_dur"]))
    finally:
        model.decoder = "best_path"
        model.__dict__.pop("beam_options", None)


def test_batch_invariant_rows_with_a_model_equal_the_utterance_alone(pr):
    model, wav, x, lens, lm = pr
    try:
        model.batch_invariant = True
        model.decoder = "beam"
        model.beam_options = dict(type(model).beam_options, lm=lm, lm_weight=0.8)
        both = model.decode_nbest(x, lens, nbest=3, log_add=True)
        ids = model.get_embeddings(x, lens)["phn_pred_seq_idx"]
        for b in range(2):
            n_audio = int(lens[b])
            alone = model.decode_nbest(x[b:b + 1, :n_audio], lens[b:b + 1], nbest=3, log_add=True)
            w = alone["tokens"].shape[2]
            for k in ("tokens", "timesteps"):
                assert torch.equal(both[k][b, :, :w], alone[k][0]) and not both[k][b, :, w:].any()
            for k in ("n_tok", "score", "n_hyp", "frame_seq_lens"):
                assert torch.equal(both[k][b], alone[k][0]), (k, b)
            assert list(ids[b]) == list(model.get_embeddings(x[b:b + 1, :n_audio], lens[b:b + 1])["phn_pred_seq_idx"][0])
    finally:
        model.batch_invariant = False
        model.decoder = "best_path"
        model.__dict__.pop("beam_options", None)
