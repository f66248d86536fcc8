"""GPU: the hipGraph-captured train step replays the same kernels as the eager autograd loop — with all stochastic
regularisers at 0 the losses and the updated parameters of the two paths agree after several optimiser steps."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_graphed_step_matches_eager():
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import GraphedAPTAIStep
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=3, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 2, 16000, seed=3).items()}
    losses = {}
    finals = {}
    for mode in ("eager", "graph"):
        model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
        model.train()
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-4, fused=True)
        ls = []
        if mode == "eager":
            for _ in range(4):
                opt.zero_grad(set_to_none=True)
                out = model(0, **batch)
                out["loss"].backward()
                opt.step()
                ls.append(out["loss"].item())
        else:
            runner = GraphedAPTAIStep(model, opt, batch)
            for _ in range(4):
                ls.append(runner.step()["loss"].item())
            runner.close()
        losses[mode] = ls
        finals[mode] = {n: p.detach().float().cpu().clone() for n, p in model.named_parameters()}
    assert losses["eager"][-1] < losses["eager"][0]                    # it trains
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) <= 2e-3 * abs(a), (losses["eager"], losses["graph"])
    for n in finals["eager"]:
        d = (finals["eager"][n] - finals["graph"][n]).abs().max().item()
        assert d <= 2e-4, (n, d)                                          # lr 1e-4 x 4 steps: updates are <= 4e-4


def test_graphed_step_with_regularisers_runs_and_varies():
    """LayerDrop / SpecAugment / dropout active: replays draw fresh randomness (loss differs step to step), stays finite,
    and dropped layers' parameters get no gradient."""
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import GraphedAPTAIStep
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=4, layerdrop=0.5, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 2, 16000, seed=3).items()}
    model = _build(cfg, sd)
    model.train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=0.0, fused=True)
    runner = GraphedAPTAIStep(model, opt, batch)
    ls, dropped_seen = [], False
    for _ in range(6):
        out = runner.step()
        ls.append(out["loss"].item())
        for layer in model.wav2vec2.encoder.layers:
            if layer.attention.q_proj.weight.grad is None:
                dropped_seen = True
    runner.close()
    assert all(torch.isfinite(torch.tensor(ls))) and len(set(round(x, 6) for x in ls)) > 1, ls
    assert dropped_seen


def test_eager_loop_sees_fused_optimizer_updates():
    """torch.optim.Adam(fused=True) updates parameters without bumping Tensor._version: the bf16 compute copies must
    still follow (regression test for a stale-weight bug)."""
    from aptai_amd.config import W2V2Config
    from oracle import heads_ref, synth
    from test_gpu_aptai import _build, TV
    cfg = W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    cb = synth.synth_aptai_batch(cfg, 2, 16000, seed=3)
    batch = {k: v.cuda() for k, v in cb.items()}
    model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
    model.train()
    opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=3e-4, fused=True)
    for _ in range(2):
        opt.zero_grad(set_to_none=True)
        model(0, **batch)["loss"].backward()
        opt.step()
    got = model(0, **batch)["loss"].item()
    sdc = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = heads_ref.aptai_forward(sdc, cfg, cb["audio_inputs"], cb["audio_lengths"], cb["phn_frames_49hz"], [cb[n] for n in TV],
                                  training=False)["loss"].item()
    assert abs(got - ref) <= 2e-2 * abs(ref), (got, ref)


def test_graphed_step_takes_host_batches():
    """The collate_fn's view of the boundary: a new HOST batch handed to every replay (pinned staging ring, asynchronous
    copies) gives the same losses as the eager loop on the same batches, in order."""
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import GraphedAPTAIStep
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    host_batches = [synth.synth_aptai_batch(cfg, 2, 16000, seed=10 + i) for i in range(5)]
    losses = {}
    for mode in ("eager", "graph"):
        model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
        model.train()
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, fused=True)
        ls = []
        if mode == "eager":
            for hb in host_batches:
                opt.zero_grad(set_to_none=True)
                out = model(0, **{k: v.cuda() for k, v in hb.items()})
                out["loss"].backward()
                opt.step()
                ls.append(out["loss"].item())
        else:
            runner = GraphedAPTAIStep(model, opt, {k: v.cuda() for k, v in host_batches[0].items()})
            outs = [runner.step(hb)["loss"].clone() for hb in host_batches]     # no host sync between the steps
            ls = [o.item() for o in outs]
            runner.close()
        losses[mode] = ls
    assert len(set(round(v, 4) for v in losses["eager"])) > 1                  # the batches differ
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) <= 2e-3 * abs(a), losses


def test_graphed_pr_step_with_trainable_conv_stack_matches_eager():
    """Wav2Vec2_PR fine-tuning (everything trainable incl. the 7-layer feature encoder, CTC head) through the same segment
    graphs: with the stochastic regularisers off, losses and updated parameters follow the eager autograd loop over several
    optimiser steps, a second batch with a narrower label block goes through set_batch, and a wider one is refused."""
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import GraphedAPTAIStep
    from oracle import synth
    from test_gpu_ctc_pr import _build_pr
    cfg = W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=40,
                          ctc_loss_reduction="mean", ctc_zero_infinity=True)
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 0)
    g = torch.Generator().manual_seed(5)

    def mk_batch(seed, width):
        sb = synth.synth_aptai_batch(cfg, 2, 16000, seed=seed)
        lab = torch.full((2, width), -100, dtype=torch.int64)
        for b in range(2):
            n = int(torch.randint(5, width + 1, (1,), generator=g))
            lab[b, :n] = torch.randint(1, 40, (n,), generator=g)
        return {"input_values": sb["audio_inputs"].cuda(), "input_lengths": sb["audio_lengths"].reshape(-1).cuda(), "phoneme_labels": lab.cuda()}
    batches = [mk_batch(3, 12), mk_batch(4, 9)]
    losses, finals = {}, {}
    for mode in ("eager", "graph"):
        model = _build_pr(cfg, sd)
        model.train()
        assert any(p.requires_grad for p in model.wav2vec2.feature_extractor.parameters())
        params = [p for p in model.parameters() if p.requires_grad]
        opt = torch.optim.Adam(params, lr=1e-4, fused=True)
        ls = []
        if mode == "eager":
            for i in range(4):
                opt.zero_grad(set_to_none=True)
                out = model(**batches[i % 2])
                out["loss"].backward()
                opt.step()
                ls.append(out["loss"].item())
        else:
            runner = GraphedAPTAIStep(model, opt, batches[0])
            for i in range(4):
                out = runner.step(batches[i % 2])
                ls.append(out["loss"].item())
            assert out["phoneme_logits"].shape == (2, 49, 40)
            wide = dict(batches[0], phoneme_labels=torch.full((2, 20), 3, dtype=torch.int64).cuda())
            with pytest.raises(ValueError):
                runner.step(wide)
            runner.close()
        losses[mode] = ls
        finals[mode] = {n: p.detach().float().cpu().clone() for n, p in model.named_parameters()}
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) <= 2e-3 * abs(a), (losses["eager"], losses["graph"])
    moved = 0
    for n in finals["eager"]:
        d = (finals["eager"][n] - finals["graph"][n]).abs().max().item()
        assert d <= 2e-4, (n, d)
        moved += int((finals["eager"][n] - sd[n].float()).abs().max().item() > 0)
    assert moved > 20                                                    # conv stack, encoder and head were all updated


def test_graphed_force_step_matches_eager_and_varies_with_dropout():
    """GraphedForceStep: encoder graph (side stream, one batch ahead) + heads graph.  With the head dropouts at 0 the losses and
    the updated head parameters follow the eager loop over alternating batches; with the reference's dropouts on, replays of
    one batch draw different masks (the per-stream salt), and lists() returns the reference's Python lists."""
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import GraphedForceStep
    from aptai_amd.optim import Adam
    from oracle import synth
    from test_gpu_force import _build, load_golden
    z, meta = load_golden("force_aptai_1x2s")
    pr_cfg = W2V2Config.from_any(meta["pr_cfg"])
    sd = synth.make_state_dict(synth.force_aptai_param_shapes(pr_cfg, meta["vocab_len"]), meta["seed"])
    B, S = 4, 32000
    batches = []
    for seed in (8, 9):
        bt = {k: v.cuda() for k, v in synth.synth_aptai_batch(pr_cfg, B, S, seed=seed, n_phn=40).items()}
        bt["phoneme_labels"] = torch.zeros(B, 4, dtype=torch.int32).cuda()
        batches.append(bt)

    def fresh(drop):
        model, _ = _build(meta, sd)
        model.train()
        if not drop:
            model.hidden_drop = 0.0
            model.rnn_drop = 0.0
        with torch.no_grad():                                   # the random-weight recogniser must decode 1..59 phonemes
            blank = model.w2v2_pr._blank()
            for _ in range(60):
                n = [len(l) for bt in batches for l in model.w2v2_pr._decode(model.w2v2_pr._logits_eval(bt["audio_inputs"], bt["audio_lengths"].reshape(-1)[:, None])[0])]
                if max(n) < 60 and min(n) >= 1:
                    break
                model.w2v2_pr.pr_head.bias[blank] += 0.25 if max(n) >= 60 else -0.25
            else:
                pytest.skip("no blank bias gives 1..59 phonemes on both batches")
        params = [p for p in model.parameters() if p.requires_grad]
        return model, params, Adam(params, lr=1e-4)

    losses, finals = {}, {}
    for mode in ("eager", "graph"):
        model, params, opt = fresh(False)
        ls = []
        if mode == "eager":
            for i in range(4):
                opt.zero_grad(set_to_none=True)
                out = model(0, **batches[i % 2])
                out["loss"].backward()
                opt.step()
                ls.append(out["loss"].item())
        else:
            runner = GraphedForceStep(model, opt, batches[0])
            for i in range(4):
                out = runner.step(batches[i % 2], next_batch=batches[(i + 1) % 2])
                ls.append(out["loss"].item())
            lists = runner.lists(out)
            assert len(lists["pred_frame_phns"]) == B and len(lists["pred_ctc_phn_seq"]) == B
            assert out["tvs_pred"].shape[0] == B and out["tvs_pred"].shape[2] == 9
            runner.close()
        losses[mode] = ls
        finals[mode] = {n: p.detach().float().cpu().clone() for n, p in model.named_parameters() if p.requires_grad}
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) <= 1e-4 * abs(a), (losses["eager"], losses["graph"])
    for n in finals["eager"]:
        d = (finals["eager"][n] - finals["graph"][n]).abs().max().item()
        assert d <= 2e-5, (n, d)                                       # fp32 heads, same kernels: atomics-level differences only
    # dropout on: two replays of the same batch draw different masks
    model, params, opt = fresh(True)
    runner = GraphedForceStep(model, opt, batches[0])
    a = runner.step(batches[0])["tvs_pred"].clone()
    b = runner.step(batches[0])["tvs_pred"].clone()
    runner.close()
    assert torch.isfinite(a).all() and not torch.equal(a, b)


def test_bucketed_graphs_equal_the_eager_loop_on_variable_length_batches():
    """BucketedGraphedStep: the reference's collate pads every batch to its own longest utterance (train/train_aptai.py:268-285),
    so consecutive batches have different shapes.  A variable-length synthetic epoch (five batches, three padded lengths, two
    buckets, host tensors as the collate_fn produces them) through the bucketed graph runner and through the eager loop on the
    un-bucketed shapes, from the same initial state: same losses, same trajectories on every valid frame, same updated parameters.
    wav2vec2-base shape: its first conv layer normalises over ALL frames of the padded batch (GroupNorm), the case that needs the
    per-step frame bounds; the low-pass filter's zero padding is the other."""
    from aptai_amd import hostlogic
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import BucketedGraphedStep
    from aptai_amd.train_aptai import SyntheticHPRC
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batches = []
    for i, sec in enumerate((1.3, 1.9, 1.45, 2.0, 1.3)):
        ds = SyntheticHPRC(3, sec, vary_length=True, seed=10 + i, cfg=cfg)
        batches.append(hostlogic.collate_aptai([ds[j] for j in range(3)]))
    assert len({b["audio_inputs"].shape[1] for b in batches}) >= 3
    rec = {}
    for mode in ("eager", "bucketed"):
        model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
        model.train()
        opt = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4, fused=True)
        out_rec = []
        if mode == "eager":
            for b in batches:
                cb = {k: v.cuda() for k, v in b.items()}
                opt.zero_grad(set_to_none=True)
                out = model(0, **cb)
                out["loss"].backward()
                opt.step()
                out_rec.append((out["loss"].item(), out["tvs_pred"].detach().float().cpu(), out["phn_fc_pred"].cpu()))
        else:
            with BucketedGraphedStep(model, opt, bucket_samples=[24000, 32000]) as runner:
                for b in batches:
                    out = runner.step(b)                               # HOST batch, padded up to its bucket inside
                    out_rec.append((out["loss"].item(), out["tvs_pred"].detach().float().cpu().clone(), out["phn_fc_pred"].cpu().clone()))
                assert len(runner.runners) == 2
                # an eager forward in between (validation) and more steps: the captured buckets survive
                runner.suspend()
                model.eval()
                with torch.no_grad():
                    model(0, **{k: v.cuda() for k, v in batches[0].items()})
                model.train()
                out_rec.append((runner.step(batches[1])["loss"].item(), None, None))
        rec[mode] = out_rec
    for i, ((l0, tv0, p0), (l1, tv1, p1)) in enumerate(zip(rec["eager"], rec["bucketed"])):
        assert abs(l0 - l1) <= 2e-3 * abs(l0), (i, l0, l1)
        assert tv0.shape == tv1.shape, (tv0.shape, tv1.shape)
        lens = hostlogic.feat_extract_output_lengths(batches[i]["audio_lengths"], cfg.conv_kernel, cfg.conv_stride)
        for u, n in enumerate(lens.tolist()):
            assert (tv0[u, :n] - tv1[u, :n]).abs().max().item() <= 2e-2 * tv0[u, :n].abs().max().item(), (i, u)
            assert (p0[u, :n] != p1[u, :n]).float().mean().item() <= 0.1, (i, u)       # near-uniform random-init logits: a few bf16 near-ties flip once the two runs' parameters differ in their last bits (4 of 99 frames measured)
    assert rec["eager"][-1][0] < rec["eager"][0][0] * 1.5


def test_bucketed_pr_step_gradients_equal_the_eager_step_from_identical_parameters():
    """What a loss-after-N-Adam-steps comparison cannot separate (round-3 verdict, item 1a): the gradients of EVERY parameter after one
    backward, graph replay inside a bucket vs the eager step on the batch as collated, from identical parameters (optimiser at lr 0).
    Bucket with the same padded frame count (1.2 s -> 2 s: Tp = 128 both): the same kernels on the same rows -> bit-identical.
    Bucket with another padded frame count (-> 3 s: Tp = 256, other split-K / tile choices): equal to summation order, rel-L2 <= 2e-3."""
    from aptai_amd import hostlogic, train_phoneme_recognizer as T
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import BucketedGraphedStep
    from aptai_amd.optim import Adam
    from oracle import synth
    from test_gpu_ctc_pr import _build_pr
    cfg = W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0., feat_proj_dropout=0.,
                          final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=40, ctc_loss_reduction="mean",
                          ctc_zero_infinity=True)
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 0)
    ds = T.SyntheticCommonPhone(4, 1.2, 40, seed=1)
    batches = [{k: v.cuda() for k, v in hostlogic.collate_pr([ds[2 * i], ds[2 * i + 1]]).items()} for i in range(2)]
    assert batches[0]["input_values"].shape[1] == 19200            # an utterance fills the batch: frame T(S) sees real samples
    model = _build_pr(cfg, sd)
    model.train()
    ref = []
    for b in batches:
        model.zero_grad(set_to_none=True)
        out = model(**b)
        out["loss"].backward()
        ref.append((out["loss"].detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}))
    for buckets, exact in (([32000], True), ([48000], False)):
        model.zero_grad(set_to_none=True)
        opt = Adam([p for p in model.parameters() if p.requires_grad], lr=0.0).publish_to(model)
        worst = 0.0
        with BucketedGraphedStep(model, opt, bucket_samples=buckets) as runner:
            for b, (loss, grads) in zip(batches, ref):
                out = runner.step(b)
                assert abs(out["loss"].item() - loss.item()) <= (0 if exact else 1e-4 * abs(loss.item()))
                assert len(grads) > 40
                for n, p in model.named_parameters():
                    if n not in grads:
                        continue
                    if exact:
                        assert torch.equal(p.grad, grads[n]), (buckets, n, (p.grad - grads[n]).abs().max().item())
                    else:
                        rel = ((p.grad.double() - grads[n].double()).norm() / (grads[n].double().norm() + 1e-30)).item()
                        worst = max(worst, rel)
                        assert rel <= 2e-3, (buckets, n, rel)
        model.wav2vec2._cache_mode = None
        model.wav2vec2._cache.clear()
        if not exact:
            print(f"[bands] bucketed PR step vs eager, other padded frame count: worst per-parameter gradient rel-L2 {worst:.2e}")


def test_bucketed_runner_cache_is_bounded_and_eviction_changes_nothing():
    """BucketedGraphedStep(max_runners=...): beyond the cap the least recently used runner is closed (salt / bounds slots of the library and
    GBs of saved activations are per runner; a corpus spans many (length bucket, label width) shapes) and re-captured if its shape returns.
    Alternating two buckets through a cache of ONE runner must give the losses of an unbounded cache, bit for bit, and release the
    stream-bound slots it used (a 65th binding would be refused)."""
    from aptai_amd import hostlogic
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import BucketedGraphedStep
    from aptai_amd.optim import Adam
    from aptai_amd.train_aptai import SyntheticHPRC
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=2, hidden_dropout=0., activation_dropout=0., attention_dropout=0.,
                          feat_proj_dropout=0., final_dropout=0., layerdrop=0., apply_spec_augment=False, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batches = []
    for i, sec in enumerate((1.3, 1.9, 1.4, 2.0)):
        ds = SyntheticHPRC(2, sec, vary_length=True, seed=20 + i, cfg=cfg)
        batches.append(hostlogic.collate_aptai([ds[j] for j in range(2)]))
    rec = {}
    for cap in (8, 1):
        model = _build(cfg, sd, tv_drop=0.0, phn_drop=0.0)
        model.train()
        opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-4).publish_to(model)
        lines = []
        with BucketedGraphedStep(model, opt, bucket_samples=[24000, 32000], max_runners=cap, log=lines.append) as runner:
            rec[cap] = [runner.step(b)["loss"].item() for b in batches]
            assert len(runner.runners) == min(cap, 2)
            assert runner.evictions == (0 if cap == 8 else 3), runner.evictions
        assert sum("captured shape" in l for l in lines) == (2 if cap == 8 else 4)
    assert rec[1] == rec[8], rec


def test_optimiser_under_the_backward_pass_changes_no_bit(monkeypatch):
    """APTAI_ADAM_OVERLAP=1 (an experiment, off by default: aptai_amd/graphed.py): each layer's weights and biases are updated on a side
    stream as soon as the layer's backward segment has finished, the rest in the usual launch at the end of the step (Adam.prepare /
    launch_early / finish).  Adam is element-wise per parameter, so every parameter, both moments and every step count must equal the
    one-launch step bit for bit - with LayerDrop on (a skipped layer gets NO update and no step count) and with the compute copies the
    optimiser publishes (the next step's forward reads them)."""
    from aptai_amd.config import W2V2Config
    from aptai_amd.graphed import GraphedAPTAIStep
    from aptai_amd.optim import Adam
    from oracle import synth
    from test_gpu_aptai import _build
    cfg = W2V2Config.base(num_hidden_layers=3, layerdrop=0.3, vocab_size=46)
    sd = synth.make_state_dict(synth.aptai_param_shapes(cfg), 0)
    batch = {k: v.cuda() for k, v in synth.synth_aptai_batch(cfg, 2, 24000, seed=3).items()}
    rec = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("APTAI_ADAM_OVERLAP", flag)
        model = _build(cfg, sd, tv_drop=0.1, phn_drop=0.1)
        model.train()
        model.wav2vec2._layerdrop_gen = torch.Generator().manual_seed(5)
        opt = Adam([p for p in model.parameters() if p.requires_grad], lr=1e-3, weight_decay=1e-2).publish_to(model)
        with GraphedAPTAIStep(model, opt, batch) as runner:
            assert runner.adam_overlap == (flag == "1")
            runner._salt_gen.seed(7)
            losses = [runner.step()["loss"].item() for _ in range(5)]
        torch.cuda.synchronize()
        rec[flag] = (losses, {n: p.detach().clone() for n, p in model.named_parameters()},
                     {n: (opt.state[p]["step"], opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone())
                      for n, p in model.named_parameters() if p in opt.state and len(opt.state[p])})
    assert rec["0"][0] == rec["1"][0], (rec["0"][0], rec["1"][0])
    steps = set()
    for n, p in rec["0"][1].items():
        assert torch.equal(p, rec["1"][1][n]), n
    for n, (st, m, v) in rec["0"][2].items():
        st1, m1, v1 = rec["1"][2][n]
        assert st == st1 and torch.equal(m, m1) and torch.equal(v, v1), n
        steps.add(st)
    assert len(steps) > 1, steps          # LayerDrop did skip a layer in some step: the case the early launches must get right


def test_pinned_ring_delivers_every_value_in_order():
    """Seven values back to back through a ring of two slots, no host synchronisation in between: each slot is reused three
    times, so a slot refilled before its previous copy had been read would show as a wrong or repeated row."""
    import numpy as np
    from aptai_amd.ops import PinnedRing as _PinnedRing
    dst = torch.zeros(2, device="cuda", dtype=torch.int32)
    got = torch.zeros((7, 2), device="cuda", dtype=torch.int32)
    ring = _PinnedRing((dst,), 2)
    want = np.arange(14, dtype=np.int32).reshape(7, 2) * 1000003 - 5
    for i in range(7):
        buf, = ring.next()
        buf[:] = want[i]
        ring.send()
        got[i].copy_(dst)
    torch.cuda.synchronize()
    assert ring.turn == 7 % 2
    assert torch.equal(got.cpu(), torch.from_numpy(want))
