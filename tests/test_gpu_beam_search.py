"""CTC beam search on the MI355X (aptai_ctc_beam_search through ops.ctc_beam_search, i.e. the C ABI) against its oracle
hostlogic.ctc_beam_search on the inputs of tests/beam_cases.py, which tests/test_cpu_beam_search.py qualifies: no decision of the
oracle rests on a score difference below 1e-9, so hypotheses, lengths, tokens and timesteps must be EQUAL; scores are equal bit
for bit in max mode (fp64 additions in the oracle's order) and within 1e-9 with log_add (fp64 logaddexp chains differ between
numpy and the device by ~1e-13 at |score| ~ 1e2).  Then the recogniser's decoder = "beam", decode_nbest and predict_nbest."""
import ctypes
import json
import os
import tempfile

import numpy as np
import pytest
import torch

import beam_cases
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
        print(f"[beam] {tag} row {b} rank {r}: score {float(score[b, r]):.12f} oracle {sc:.12f} |diff| {err:.3e}")
        if log_add:
            assert err <= 1e-9, (tag, b, r, err)
        else:
            assert float(score[b, r]) == sc, (tag, b, r, err)
    for r in range(len(hyps), nbest):
        assert int(n_tok[b, r]) == 0 and score[b, r] == -np.inf and not tokens[b, r].any() and not timesteps[b, r].any(), (tag, b, r)


@pytest.mark.parametrize("name", beam_cases.CASE_IDS)
def test_beam_search_equals_the_oracle(name):
    case = beam_cases.CASES[beam_cases.CASE_IDS.index(name)]
    got = [x.cpu().numpy() for x in _decode(case)]
    ref = beam_cases.oracle(name)
    assert got[0].shape == (len(case.lens), case.opts["nbest"], case.em.shape[1] + 2) and got[3].dtype == np.float64
    for b, (hyps, _) in enumerate(ref):
        _check_row(got, b, hyps, case.opts["nbest"], case.opts["log_add"], name)
    if name == "short":
        assert (got[4] < case.opts["nbest"]).any()
    if name == "beam1":                                # beam 1 / threshold 0 is the framed best path
        from aptai_amd import hostlogic
        for b, length in enumerate(case.lens):
            tok, ts = hostlogic.ctc_bracketed_best_path(case.em[b], length, case.blank, case.sil)
            n = int(got[2][b, 0])
            assert np.array_equal(got[0][b, 0, :n], tok) and np.array_equal(got[1][b, 0, :n], ts)


def test_rows_of_a_batch_equal_their_own_decode_and_the_empty_row():
    """input_lens = [T, T // 2, 0] in one launch: every row bit-equal to its single-utterance decode; T_b == 0 gives [sil] at 0 with
    score 0.  Then input_lens null on a padded rows_per_b > T: all T frames of every row."""
    from aptai_amd import hostlogic, ops
    T, V, ldl, blank, sil = 20, 9, 16, 0, 4
    em = np.stack([beam_cases.iid(81, T, V, 1.0), beam_cases.peaky(82, T, V, blank), beam_cases.iid(83, T, V, 1.0)])
    lens = [T, T // 2, 0]
    opts = dict(beam_size=10, beam_threshold=50.0, log_add=True, nbest=5)

    def run(rows, lengths, rows_per_b):
        full = np.full((len(rows), rows_per_b, ldl), 1.0e4, dtype=np.float32)
        full[:, :T, :V] = rows
        li = None if lengths is None else torch.tensor(lengths, dtype=torch.int32).cuda()
        out = ops.ctc_beam_search(torch.from_numpy(full.reshape(-1, ldl)).cuda(), ldl, rows_per_b, len(rows), T, V, blank, sil,
                                  input_lens_i32=li, **opts)
        return [x.cpu().numpy() for x in out]
    batch = run(em, lens, T)
    for b in range(3):
        alone = run(em[b:b + 1], lens[b:b + 1], T)
        for x, y in zip(batch, alone):
            assert x[b].tobytes() == y[0].tobytes(), b
    assert batch[4][2] == 1 and batch[2][2, 0] == 1 and batch[0][2, 0, 0] == sil and batch[1][2, 0, 0] == 0 and batch[3][2, 0] == 0.0
    for b in range(2):
        stats = {}
        hyps = hostlogic.ctc_beam_search(em[b, :lens[b]], blank, sil, stats=stats, **opts)
        assert stats["min_decision_gap"] >= 1e-9
        _check_row(batch, b, hyps, 5, True, "lens")
    padded = run(em, None, T + 5)
    for b in range(3):
        stats = {}
        hyps = hostlogic.ctc_beam_search(em[b], blank, sil, stats=stats, **opts)
        assert stats["min_decision_gap"] >= 1e-9
        _check_row(padded, b, hyps, 5, True, "null-lens")


def test_max_n_cuts_the_row_and_writes_nothing_past_it():
    """max_n smaller than a hypothesis: n_tok is the full length, the first max_n entries are right, the guard behind every row of a
    wider output buffer survives (the C ABI is called directly to own the buffers)."""
    from aptai_amd import _lib, ops
    case = beam_cases.CASES[beam_cases.CASE_IDS.index("ref46-logadd")]
    B, T, V = case.em.shape
    nbest, max_n, wide = case.opts["nbest"], 5, 9
    ref = beam_cases.oracle(case.name)
    assert any(len(h[0]) > max_n for hyps, _ in ref for h in hyps)
    logits = _device_logits(case)
    lens = torch.tensor(case.lens, dtype=torch.int32).cuda()
    ws = torch.empty(_lib.lib().aptai_ctc_beam_search_workspace_bytes(B, T, case.opts["beam_size"], nbest), dtype=torch.uint8, device="cuda")
    tok = torch.full((B * nbest * max_n + wide,), GUARD, dtype=torch.int32, device="cuda")
    ts = torch.full((B * nbest * max_n + wide,), GUARD, dtype=torch.int32, device="cuda")
    n_tok = torch.full((B * nbest + wide,), GUARD, dtype=torch.int32, device="cuda")
    score = torch.full((B * nbest + wide,), float(GUARD), dtype=torch.float64, device="cuda")
    n_hyp = torch.full((B + wide,), GUARD, dtype=torch.int32, device="cuda")
    _lib.call("aptai_ctc_beam_search", logits.data_ptr(), case.ldl, case.rows_per_b, lens.data_ptr(), B, T, V, case.blank, case.sil,
              case.opts["beam_size"], 0, case.opts["beam_threshold"], 1, 0.0, nbest, max_n, ws.data_ptr(), tok.data_ptr(), ts.data_ptr(),
              n_tok.data_ptr(), score.data_ptr(), n_hyp.data_ptr(), ops._stream())
    tok, ts, n_tok, score, n_hyp = (x.cpu().numpy() for x in (tok, ts, n_tok, score, n_hyp))
    for x, n in ((tok, B * nbest * max_n), (ts, B * nbest * max_n), (n_tok, B * nbest), (score, B * nbest), (n_hyp, B)):
        assert (x[n:] == GUARD).all() and not (x[:n] == GUARD).any()
    tok, ts = tok[:B * nbest * max_n].reshape(B, nbest, max_n), ts[:B * nbest * max_n].reshape(B, nbest, max_n)
    for b, (hyps, _) in enumerate(ref):
        for r, (want, pos, _) in enumerate(hyps):
            assert n_tok[b * nbest + r] == len(want)
            k = min(len(want), max_n)
            assert np.array_equal(tok[b, r, :k], want[:k]) and np.array_equal(ts[b, r, :k], pos[:k])
            assert not tok[b, r, k:].any() and not ts[b, r, k:].any()


def test_same_call_twice_gives_the_same_bits():
    case = beam_cases.CASES[beam_cases.CASE_IDS.index("beam32")]
    first = [x.cpu().numpy().tobytes() for x in _decode(case)]
    assert first == [x.cpu().numpy().tobytes() for x in _decode(case)]


def test_bad_arguments_are_refused_with_a_message_and_launch_nothing():
    from aptai_amd import _lib, ops
    case = beam_cases.CASES[beam_cases.CASE_IDS.index("v3")]
    B, T, V = case.em.shape
    logits = _device_logits(case)
    ws = torch.empty(_lib.lib().aptai_ctc_beam_search_workspace_bytes(B, T, 32, 32) + 16, dtype=torch.uint8, device="cuda")
    assert ws.data_ptr() % 16 == 0
    outs = [torch.full((B * 32 * (T + 2),), GUARD, dtype=torch.int32, device="cuda") for _ in range(4)]
    score = torch.full((B * 32,), float(GUARD), dtype=torch.float64, device="cuda")

    def call(beam=6, nbest=6, V_=V, thr=50.0, ws_off=0):
        return _lib.lib().aptai_ctc_beam_search(logits.data_ptr(), case.ldl, case.rows_per_b, None, B, T, V_, case.blank, case.sil, beam, 0,
                                                thr, 1, 0.0, nbest, T + 2, ws.data_ptr() + ws_off, outs[0].data_ptr(), outs[1].data_ptr(),
                                                outs[2].data_ptr(), score.data_ptr(), outs[3].data_ptr(), ops._stream())
    for kw, word in ((dict(beam=0, nbest=1), "beam_size"), (dict(beam=33, nbest=1), "beam_size"), (dict(beam=4, nbest=5), "nbest"),
                     (dict(V_=257), "V="), (dict(thr=-1.0), "beam_threshold"), (dict(ws_off=4), "aligned")):
        assert call(**kw) == -1, kw
        msg = _lib.lib().aptai_last_error().decode()
        assert "aptai_ctc_beam_search" in msg and word in msg, (kw, msg)
    torch.cuda.synchronize()
    assert all((o == GUARD).all().item() for o in outs) and (score == GUARD).all().item()
    assert call() == 0
    for kw in (dict(beam_size=0), dict(beam_size=33), dict(beam_size=4, nbest=5), dict(beam_threshold=-1.0), dict(beam_size_token=0)):
        with pytest.raises(ValueError):
            ops.ctc_beam_search(logits, case.ldl, case.rows_per_b, B, T, V, case.blank, case.sil, **kw)
    with pytest.raises(ValueError):
        ops.ctc_beam_search(logits, 512, case.rows_per_b, B, T, 257, case.blank, case.sil)
    with pytest.raises(_lib.AptaiHipError):
        ops.ctc_beam_search(logits.cpu(), case.ldl, case.rows_per_b, B, T, V, case.blank, case.sil)


# ------------------------------------------------------------------------------------------------ the recogniser
@pytest.fixture(scope="module")
def pr():
    """The smallest random-init recogniser of the GPU tests (tests/test_gpu_parity2.py _pr_setup) with a silence token, 2 x 1 s."""
    from aptai_amd.config import W2V2Config
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
    return model.cuda().eval(), wav, x, torch.tensor([16000, 12000]).cuda()


def test_model_beam_decoder_equals_flashlight_and_best_path_is_untouched(pr):
    """decoder = "beam" with the default options (the reference's: max-merge, 1-best) returns what the closed form returns, ids and
    durations; decoder = "best_path" is ops.ctc_greedy_decode, bit for bit; an unknown name is refused."""
    from aptai_amd import ops
    model, wav, x, lens = pr
    full = torch.tensor([16000, 16000]).cuda()
    try:
        model.decoder = "flashlight"
        want = model.get_embeddings(x, full)["phn_pred_seq_idx"]
        want_dur = model.predict_phonemes_durations(wav, model.vocab)
        want_seq = model.pred_phn_seq(wav, model.vocab)
        model.decoder = "beam"
        emb = model.get_embeddings(x, full)
        for b in range(2):
            assert list(emb["phn_pred_seq_idx"][b]) == list(want[b]) and len(want[b]) >= 3
        dur = model.predict_phonemes_durations(wav, model.vocab)
        assert list(dur["phn_seq_idx"]) == list(want_dur["phn_seq_idx"]) and dur["phn_seq_ipa"] == want_dur["phn_seq_ipa"]
        assert np.array_equal(np.asarray(dur["phn_seq_dur"]), np.asarray(want_dur["phn_seq_dur"]))
        assert list(model.pred_phn_seq(wav, model.vocab)["phn_seq_idx"]) == list(want_seq["phn_seq_idx"])
        model.decoder = "best_path"
        out, _ = model._logits_eval(x, full[:, None])
        g, lf = out._geom, out._logits_full
        ids, n = model._decode_device(out, g.T + 2)
        ids0, n0 = ops.ctc_greedy_decode(lf, lf.shape[1], g.Tp, g.B, g.T, model.pr_head.weight.shape[0], 0, g.T + 2)
        assert torch.equal(ids, ids0) and torch.equal(n, n0)
        model.decoder = "viterbi"
        with pytest.raises(ValueError):
            model.pred_phn_seq(wav, model.vocab)
    finally:
        model.decoder = "best_path"


def test_decode_nbest_and_predict_nbest_equal_the_oracle_on_the_models_logits(pr):
    from aptai_amd import hostlogic
    model, wav, x, lens = pr
    full = torch.tensor([16000, 16000]).cuda()
    res = model.decode_nbest(x, full, nbest=3, log_add=True)
    emb = model.get_embeddings(x, full)
    got = [res[k].cpu().numpy() for k in ("tokens", "timesteps", "n_tok", "score", "n_hyp")]
    assert res["frame_seq_lens"].cpu().tolist() == list(emb["frame_seq_lens"])
    for b in range(2):
        lg = emb["phoneme_logits"][b].T
        stats = {}
        hyps = hostlogic.ctc_beam_search(lg, 0, 5, beam_size=10, beam_threshold=50.0, log_add=True, nbest=3, stats=stats)
        assert stats["min_decision_gap"] >= 1e-9
        _check_row(got, b, hyps, 3, True, "model")
    one = model.predict_nbest(wav, model.vocab, nbest=3, log_add=True)
    lg = model.get_ctc_logits(wav)
    hyps = hostlogic.ctc_beam_search(lg, 0, 5, beam_size=10, beam_threshold=50.0, log_add=True, nbest=3)
    inv = {v: k for k, v in model.vocab.items()}
    assert len(one) == len(hyps) == 3
    for h, (tok, ts, sc) in zip(one, hyps):
        assert list(h["phn_seq_idx"]) == list(tok) and h["phn_seq_ipa"] == [inv[int(i)] for i in tok] and abs(h["score"] - sc) <= 1e-9
        assert np.array_equal(np.asarray(h["phn_seq_dur"]), np.asarray([int(t) * (len(wav) / lg.shape[0] / 16000) for t in ts]))


def test_batch_invariant_beam_rows_equal_the_utterance_alone(pr):
    model, wav, x, lens = pr
    try:
        model.batch_invariant = True
        model.decoder = "beam"
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


def test_batch_invariant_framed_rows_equal_the_utterance_alone(pr):
    """batch_invariant with decoder = "flashlight": the closing silence meets each row's own last frame, so every row of the padded
    batch decodes as the utterance does alone, and the shorter clip alone is the oracle on its own logits, ids and durations."""
    from aptai_amd import hostlogic
    model, wav, x, lens = pr
    try:
        model.batch_invariant = True
        model.decoder = "flashlight"
        ids = model.get_embeddings(x, lens)["phn_pred_seq_idx"]
        for b in range(2):
            n_audio = int(lens[b])
            alone = model.get_embeddings(x[b:b + 1, :n_audio], lens[b:b + 1])["phn_pred_seq_idx"][0]
            assert list(ids[b]) == list(alone) and len(alone) >= 3
        short = x[1, :int(lens[1])].cpu().numpy()
        dur = model.predict_phonemes_durations(short, model.vocab)
        lg = model.get_ctc_logits(short)
        want, ts = hostlogic.ctc_bracketed_best_path(lg, lg.shape[0], 0, 5)
        assert list(dur["phn_seq_idx"]) == list(want) == list(ids[1])
        assert np.array_equal(np.asarray(dur["phn_seq_dur"]), ts * (len(short) / lg.shape[0] / 16000))
    finally:
        model.batch_invariant = False
        model.decoder = "best_path"
