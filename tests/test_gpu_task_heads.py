"""GPU: each model's eager forward + backward against a direct ``head.fwd`` / ``head.bwd`` of its task head (aptai_amd.task_heads) on
the same input activation and an identically built state: the loss and every head parameter's gradient are equal bit for bit.
None of the three heads has a gradient that differs between two calls of one path (the Force embedding gradient and the
forward-sum sums are order-fixed: csrc/force.hip embed_bwd_kernel, csrc/ctc.hip ctc_grad_kernel), so nothing here takes a tolerance.
Both sides run the same `fwd` / `bwd`, so this pins what HeadFn adds (which gradient goes to which parameter, the state, the seed); that
a head's `bwd` files each gradient under the right name is pinned by the reference comparisons of tests/test_gpu_force.py,
test_gpu_aptai.py and test_gpu_ctc_pr.py.  Two encoder layers, batch 2 x 16000 samples (49 frames), every dropout 0."""
import pytest
import torch

pytestmark = pytest.mark.gpu

TV = ("LA", "LP", "JA", "TTCL", "TTCD", "TMCL", "TMCD", "TBCL", "TBCD")


def _cfg(vocab_size, **kw):
    from aptai_amd.config import W2V2Config
    return W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0., feat_proj_dropout=0.,
                           final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=vocab_size, **kw)


def _record(model, encoder):
    """Shadows the class's head with one that notes what the eager path hands `fwd`, and the encoder step its seed was made from."""
    seen = {}

    class Recording(type(model.task_head)):
        def fwd(self, h, params, st):
            seen.update(h=h, st=st, step=encoder._step)
            return super().fwd(h, params, st)
    model.task_head = Recording()
    return seen


def _check_direct(model, encoder, seen, loss, targets):
    head = type(model).task_head
    params = head.params(model)
    st = head.state(model, seen["st"].g, (encoder.base_seed, seen["step"]), True, *targets)
    assert st.seed == seen["st"].seed
    with torch.no_grad():
        outs, saved = head.fwd(seen["h"].detach(), params, st)
        grads = head.bwd(saved, st, params, seen["h"].detach(), None)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], loss.detach())
    assert len(grads) == 1 + len(params)
    names = {id(p): n for n, p in model.named_parameters()}
    for p, gt in zip(params, grads[1:]):
        assert p.grad is not None and torch.equal(p.grad, gt), names[id(p)]
    return grads[0]


def test_aptai_head_direct_equals_eager():
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = _cfg(46)
    model = _build(cfg, synth.make_state_dict(synth.aptai_param_shapes(cfg), 0), tv_drop=0.0, phn_drop=0.0).train()
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 2, 16000, seed=3).items()}
    seen = _record(model, model.wav2vec2)
    out = model(0, **batch)
    out["loss"].backward()
    dh = _check_direct(model, model.wav2vec2, seen, out["loss"],
                       (torch.stack([batch[n] for n in TV], dim=-1).float(), batch["phn_frames_49hz"]))
    assert dh.shape == seen["h"].shape and torch.isfinite(dh.float()).all()


def test_ctc_head_direct_equals_eager():
    from aptai_amd import hostlogic
    from oracle import synth
    from test_gpu_ctc_pr import _build_pr
    cfg = _cfg(40, ctc_loss_reduction="mean", ctc_zero_infinity=True)
    model = _build_pr(cfg, synth.make_state_dict(synth.pr_param_shapes(cfg), 0)).train()
    sb = synth.synth_aptai_batch(cfg, 2, 16000, seed=3)
    lab = torch.full((2, 12), -100, dtype=torch.int64)
    gen = torch.Generator().manual_seed(5)
    for b, n in enumerate((12, 7)):
        lab[b, :n] = torch.randint(1, 40, (n,), generator=gen)
    lens = sb["audio_lengths"].reshape(-1).cuda()
    seen = _record(model, model.wav2vec2)
    out = model(sb["audio_inputs"].cuda(), lens, lab.cuda())
    out["loss"].backward()
    dh = _check_direct(model, model.wav2vec2, seen, out["loss"],
                       (lab.cuda(), model.wav2vec2._get_feat_extract_output_lengths(lens), hostlogic.ctc_target_lengths(lab.cuda())))
    assert dh.shape == seen["h"].shape and torch.isfinite(dh.float()).all()


@pytest.mark.parametrize("B", [2, 1])           # batch 1: the branch where the LSTM runs over all frames (models/modules.py:209-212)
def test_force_head_direct_equals_eager(B):
    from aptai_amd.task_heads import ForceParams
    from oracle import synth
    from test_gpu_force import _build
    cfg = _cfg(40, ctc_loss_reduction="mean", ctc_zero_infinity=True)
    model, _ = _build({"pr_cfg": cfg.to_dict()}, synth.make_state_dict(synth.force_aptai_param_shapes(cfg, 40), 0))
    model.train()
    model.hidden_drop = model.rnn_drop = 0.0
    assert model.max_phn_seq_len == 60                                     # the default slot count
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, B, 16000, seed=5, n_phn=40).items()}
    batch["phoneme_labels"] = torch.zeros(B, 4, dtype=torch.int32).cuda()
    gen = torch.Generator().manual_seed(7)
    given = [torch.randint(2, 40, (n,), generator=gen).numpy() for n in (23, 17)[:B]]
    encoder = model.w2v2_pr.wav2vec2
    seen = _record(model, encoder)
    out = model(0, **batch, _phn_pred_list=given)
    out["loss"].backward()
    st = seen["st"]
    assert (st.rnn_lens is st.frame_lens) == (B > 1)
    none = _check_direct(model, encoder, seen, out["loss"],
                         (st.ids, st.text_lens, st.frame_lens, torch.stack([batch[n] for n in TV], dim=-1).float()))
    assert none is None                                                    # the frozen encoder's output gets no gradient
    assert isinstance(type(model).task_head.params(model), ForceParams)
    assert all(p.grad is None for n, p in model.named_parameters() if n.startswith("w2v2_pr."))
