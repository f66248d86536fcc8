"""CPU: what the bucketed graph runner asks a task head about a batch (aptai_amd.task_heads): padding to a bucket, the extra part of
the runner cache key, and the cut back to the batch's own frame count."""
import torch

TV = ("LA", "LP", "JA", "TTCL", "TTCD", "TMCL", "TMCD", "TBCL", "TBCD")


def _aptai_batch(T, S=12000):
    batch = {"audio_inputs": torch.randn(2, S), "audio_lengths": torch.tensor([S, S - 100]),
             "phn_frames_49hz": torch.randint(1, 46, (2, T))}
    batch.update({n: torch.randn(2, T, dtype=torch.float64) for n in TV})
    return batch


def _pr_batch(width, S=12000):
    return {"input_values": torch.randn(2, S), "input_lengths": torch.tensor([S, S - 100]),
            "phoneme_labels": torch.randint(1, 40, (2, width))}


def test_ctc_labels_pad_to_the_label_bucket():
    from aptai_amd.task_heads import CtcHead
    batch = _pr_batch(5)
    out = CtcHead().pad_batch(batch, 16000, 49, 32)
    assert out["input_values"].shape == (2, 16000) and torch.equal(out["input_values"][:, :12000], batch["input_values"])
    assert (out["input_values"][:, 12000:] == 0).all()
    assert out["phoneme_labels"].shape == (2, 32) and torch.equal(out["phoneme_labels"][:, :5], batch["phoneme_labels"])
    assert (out["phoneme_labels"][:, 5:] == -100).all()
    assert out["input_lengths"] is batch["input_lengths"]
    assert CtcHead().pad_batch(_pr_batch(32), 16000, 49, 32)["phoneme_labels"].shape == (2, 32)      # a full bucket stays
    assert CtcHead().pad_batch(_pr_batch(33), 16000, 49, 32)["phoneme_labels"].shape == (2, 64)


def test_aptai_tracks_pad_to_the_bucket_frames():
    from aptai_amd.task_heads import AptaiHead
    batch = _aptai_batch(40)
    out = AptaiHead().pad_batch(batch, 16000, 49, 32)
    assert out["audio_inputs"].shape == (2, 16000) and (out["audio_inputs"][:, 12000:] == 0).all()
    assert out["audio_lengths"] is batch["audio_lengths"]
    for n in TV:
        assert out[n].shape == (2, 49) and out[n].dtype == torch.float64
        assert torch.equal(out[n][:, :40], batch[n]) and (out[n][:, 40:] == -100.0).all()
    phn = out["phn_frames_49hz"]
    assert phn.shape == (2, 49) and torch.equal(phn[:, :40], batch["phn_frames_49hz"]) and (phn[:, 40:] == 0).all()


def test_aptai_tracks_longer_than_the_bucket_are_cut():
    from aptai_amd.task_heads import AptaiHead
    batch = _aptai_batch(55)
    batch["phoneme_labels"] = torch.randint(1, 40, (2, 60))
    out = AptaiHead().pad_batch(batch, 16000, 49, 32)
    for n in TV + ("phn_frames_49hz",):
        assert torch.equal(out[n], batch[n][:, :49]), n
    assert out["phoneme_labels"] is batch["phoneme_labels"]                # not a frame-rate entry: neither padded nor cut
    exact = _aptai_batch(49)
    assert all(v is exact[k] for k, v in AptaiHead().pad_batch(exact, 12000, 49, 32).items())


def test_cache_key_carries_the_label_width_for_ctc_only():
    from aptai_amd.task_heads import AptaiHead, CtcHead
    ctc = CtcHead()
    assert ctc.cache_key(ctc.pad_batch(_pr_batch(5), 16000, 49, 32)) == (32,)
    assert ctc.cache_key(ctc.pad_batch(_pr_batch(40), 16000, 49, 32)) == (64,)
    batch = dict(_aptai_batch(40), phoneme_labels=torch.randint(1, 40, (2, 5)))
    assert AptaiHead().cache_key(AptaiHead().pad_batch(batch, 16000, 49, 32)) == ()


def test_cut_returns_the_batchs_own_frames():
    from aptai_amd.task_heads import AptaiHead, CtcHead
    T = 37
    out = {"loss": torch.tensor(1.5), "mse_loss": torch.tensor(1.0), "ce_loss": torch.tensor(2.0), "tvs_pred": torch.randn(2, 49, 9),
           "phn_fc_pred": torch.randint(0, 46, (2, 49))}
    cut = AptaiHead().cut(out, T)
    assert set(cut) == set(out)
    for k in ("loss", "mse_loss", "ce_loss"):
        assert cut[k] is out[k]
    for k in ("tvs_pred", "phn_fc_pred"):
        assert torch.equal(cut[k], out[k][:, :T])
    out = {"loss": torch.tensor(1.5), "phoneme_logits": torch.randn(2, 49, 40), "log_probs": torch.randn(49, 2, 40),
           "hidden_states": torch.randn(2, 49, 16)}
    cut = CtcHead().cut(out, T)
    assert set(cut) == set(out) and cut["loss"] is out["loss"]
    assert torch.equal(cut["log_probs"], out["log_probs"][:T])
    for k in ("phoneme_logits", "hidden_states"):
        assert torch.equal(cut[k], out[k][:, :T])
