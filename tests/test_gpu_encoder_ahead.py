"""The frozen recogniser's pass one batch ahead has ONE owner (force_aptai.EncoderAhead) for the eager loop's prefetch and for
GraphedForceStep, and the scratch the captured Force graphs hold on to never moves (ops.ScratchPool).  Mini recogniser of the
`force_aptai_1x2s` fixture with its blank bias, head dropouts 0, B = 2, S = 16000."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _case(seed=1, B=2, S=16000):
    """(fresh model in train mode, its optimiser, a batch) - the same initial state on every call."""
    from aptai_amd.config import W2V2Config
    from aptai_amd.optim import Adam
    from oracle import synth
    from test_gpu_force import _build
    z, meta = load_golden("force_aptai_1x2s")
    pr_cfg = W2V2Config.from_any(meta["pr_cfg"])
    sd = synth.make_state_dict(synth.force_aptai_param_shapes(pr_cfg, meta["vocab_len"]), meta["seed"])
    sd["w2v2_pr.pr_head.bias"][0] += meta["blank_bias"]
    model, _ = _build(meta, sd)
    model.train()
    model.hidden_drop = 0.0
    model.rnn_drop = 0.0

    def batch(B, S, seed):
        bt = {k: v.cuda() for k, v in synth.synth_aptai_batch(pr_cfg, B, S, seed=seed, n_phn=40).items()}
        bt["phoneme_labels"] = torch.zeros(B, 4, dtype=torch.int32).cuda()
        return bt
    opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4)
    return model, opt, batch(B, S, seed), batch


def _inline(model, bt):
    with torch.no_grad():
        ref = model._encode(bt["audio_inputs"], bt["audio_lengths"])
    torch.cuda.synchronize()
    return ref


def test_runner_and_eager_loop_share_one_captured_encoder_pass():
    from aptai_amd.graphed import GraphedForceStep
    model, opt, bt, _ = _case()
    ahead = model.encoder_ahead
    runner = GraphedForceStep(model, opt, bt)
    assert ahead.captures == 1 and len(ahead.entries) == 1
    (key, entry), = ahead.entries.items()
    assert entry is not None and key[0] == (2, 16000)
    assert not any(hasattr(runner, a) for a in ("g_enc", "_enc_stream", "enc"))        # no encoder graph or stream of its own
    for _ in range(2):
        out = runner.step(bt)
    ref = _inline(model, bt)
    assert torch.equal(runner.h_ac, ref.ac) and torch.equal(out["ids"], ref.ids)
    runner.close()
    assert len(ahead.entries) == 1 and ahead.entries[key] is entry                     # close() leaves the model's entries alone
    nxt = (bt["audio_inputs"], bt["audio_lengths"])
    for _ in range(2):                                                                 # the eager loop on the same model replays that entry
        before = entry.last
        res = model(0, **bt, _prefetch_next=nxt, _device_outputs=True)
        assert entry.last > before and torch.equal(res["ctc_ids"], ref.ids)
    enc = model._take_prefetched(*nxt)
    torch.cuda.synchronize()
    assert ahead.captures == 1 and len(ahead.entries) == 1 and ahead.entries[key] is entry
    assert torch.equal(enc.ac, ref.ac) and torch.equal(enc.ids, ref.ids)


def test_reloaded_weights_reach_a_live_runner():
    """load_state_dict under a live GraphedForceStep: the captured pass holds addresses of compute copies that are rebuilt, and the pass
    already launched ahead ran with the old weights - both are dropped, and the next step() hands the heads what the NEW weights give."""
    from aptai_amd.graphed import GraphedForceStep
    model, opt, bt, _ = _case()
    runner = GraphedForceStep(model, opt, bt)
    out = runner.step(bt)
    ac0, ids0 = runner.h_ac.clone(), out["ids"].clone()
    torch.cuda.synchronize()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    last = model.w2v2_pr.wav2vec2.config.num_hidden_layers - 1
    k = f"w2v2_pr.wav2vec2.encoder.layers.{last}.feed_forward.output_dense.bias"
    sd[k] += 0.05 * torch.randn(sd[k].shape, generator=torch.Generator().manual_seed(5)).to(sd[k])
    model.load_state_dict(sd)
    out = runner.step(bt)                                                              # before any eager forward
    ac1, ids1 = runner.h_ac.clone(), out["ids"].clone()
    ref = _inline(model, bt)
    runner.close()
    assert not torch.equal(ac1, ac0)
    assert torch.equal(ac1, ref.ac) and torch.equal(ids1, ref.ids)
    assert not (torch.equal(ac0, ref.ac) and torch.equal(ids0, ref.ids))


def test_scratch_of_a_captured_heads_graph_does_not_move():
    """An eager step at a larger batch shape between replays asks for larger split-K slabs: the buffers the heads graph has baked in
    stay where they are, and the replays after it compute what uninterrupted replays compute."""
    from aptai_amd import ops
    from aptai_amd.graphed import GraphedForceStep
    purposes = ("sgemm", "colsum", "ln32_bwd", "lstm")

    def held():
        return {p: [(st, t.data_ptr(), t.numel()) for st, t in ops.SCRATCH.buffers(p)] for p in purposes}

    def run(interrupt):
        model, opt, bt, batch = _case()
        runner = GraphedForceStep(model, opt, bt)
        losses = [runner.step(bt)["loss"].clone()]
        if interrupt:
            before = held()
            assert all(before[p] for p in purposes), before
            model(0, **batch(4, 32000, 2), _device_outputs=True)["loss"].backward()
            model.zero_grad(set_to_none=True)
            after = held()
            for p in purposes:
                assert after[p][:len(before[p])] == before[p], p                       # still held, same address
        for _ in range(2):
            losses.append(runner.step(bt)["loss"].clone())
        torch.cuda.synchronize()
        runner.close()
        return losses, {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}

    l0, p0 = run(False)
    l1, p1 = run(True)
    assert all(torch.isfinite(a) for a in l0)
    assert all(torch.equal(a, b) for a, b in zip(l0, l1)), (l0, l1)
    bad = [n for n in p0 if not torch.equal(p0[n], p1[n])]
    assert not bad, bad
