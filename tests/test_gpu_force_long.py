"""Force_APTAI beyond 60 phoneme slots (`max_phn_seq_len` up to 255): the wide cross-attention softmax pair of csrc/force.hip
(a lane holds slots l, l + 64, l + 128, l + 192), forward-sum rows at pitch round_up(N + 1, 64), and the model on top of them,
against float64 restatements and the CPU oracle (oracle/heads_ref.py takes the cap).  The mini recogniser of the
`force_aptai_1x2s` fixture throughout."""
import tempfile

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu
TV = ("LA", "LP", "JA", "TTCL", "TTCD", "TMCL", "TMCD", "TBCL", "TBCD")
B, T = 2, 128                      # kernel-level shape: 256 rows = 64 workgroups of four waves


def _ld(N):
    return (N + 64) // 64 * 64


def _problem(N, n, seed=0):
    """raw ~ 8 N(0,1) [B][T][N]; ids with n[b] real slots followed by zeros."""
    g = torch.Generator().manual_seed(1000 * N + seed)
    raw = 8.0 * torch.randn(B, T, N, generator=g)
    ids = torch.zeros(B, N, dtype=torch.int32)
    for b in range(B):
        ids[b, :n[b]] = torch.randint(1, 40, (n[b],), generator=g, dtype=torch.int32)
    return raw, ids


def _fwd(raw, ids, rows=True):
    from aptai_amd import ops
    N = raw.shape[-1]
    fs = torch.full((B * T, _ld(N)), float("nan"), device="cuda") if rows else None
    e, a, al, align = ops.xattn_softmax_fwd(raw.reshape(B * T, N).contiguous().cuda(), ids.cuda(), B, T, N, fs_rows=fs)
    torch.cuda.synchronize()
    return e.view(B, T, N).cpu(), a.view(B, T, N).cpu(), al.view(B, T, N).cpu(), align.cpu(), (fs.cpu() if rows else None)


def _ref64(raw, ids):
    m = torch.where(ids != 0, 0.0, -1000.0).double()[:, None, :]
    energy = raw.double() + m
    return energy, torch.softmax(energy, -1), torch.log_softmax(energy + m, -1)


# ------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("N", [61, 64, 65, 127, 128, 129, 191, 192, 193, 255])
def test_wide_softmax_values_and_forward_sum_rows(N):
    """Full row (N real slots) and single-slot row against float64, the bounds of
    test_xattn_softmax_and_alignment_bit_exact_on_golden_energy (values reach -2000); forward-sum rows [-1 | att_log | 0]."""
    raw, ids = _problem(N, (N, 1))
    e, a, al, align, fs = _fwd(raw, ids)
    re, ra, ral = _ref64(raw, ids)
    for name, got, ref in (("energy", e, re), ("att", a, ra), ("att_log", al, ral)):
        err = (got.double() - ref).abs()
        print(f"[long] N={N} {name}: max |err| {err.max().item():.3e}")
        assert np.allclose(got.numpy(), ref.numpy(), rtol=3e-7, atol=2e-5), name
    dev = (a.double().sum(-1) - 1).abs().max().item()
    print(f"[long] N={N} |sum(att) - 1| max {dev:.3e}")
    assert dev <= 1e-6
    ld = _ld(N)
    assert fs.shape == (B * T, ld)
    assert torch.equal(fs[:, 0], torch.full((B * T,), -1.0))
    assert torch.equal(fs[:, 1:N + 1], al.reshape(B * T, N))                       # bitwise the returned att_log
    assert torch.equal(fs[:, N + 1:], torch.zeros(B * T, ld - N - 1))
    assert torch.equal(align, al.argmax(-1))


@pytest.mark.parametrize("N", [130, 255])
def test_wide_argmax_picks_the_raised_slot(N):
    """+40 on one real slot per row, cycling through every slot group and through lanes 0 and 63.  (The raised slot first takes
    the row's maximum: +40 on a plain draw of 8 N(0,1) does not always beat the largest of 254 others.)"""
    n = (N, N // 2)
    raw, ids = _problem(N, n, seed=1)
    want = torch.zeros(B, T, dtype=torch.int64)
    for b in range(B):
        cand = [c for c in (0, 63, 64, 127, 128, 191, 192, 254, 5, 70) if c < n[b]]
        for t in range(T):
            c = cand[t % len(cand)]
            raw[b, t, c] = raw[b, t, :n[b]].max()
            raw[b, t, c] += 40.0
            want[b, t] = c
    assert len(set(want[0].tolist())) >= (8 if N == 255 else 5)
    _, _, _, align, _ = _fwd(raw, ids, rows=False)
    assert torch.equal(align, want)


@pytest.mark.parametrize("lo,hi", [(5, 70), (3, 66), (64, 65), (130, 194)])
def test_wide_argmax_tie_goes_to_the_lowest_slot_index(lo, hi):
    """Two real slots with one raw value, maximal: att_log is bitwise equal in both and the lower SLOT wins - (3, 66): slot 66
    lives in lane 2, below lane 3, so a tie broken by lane would answer 66."""
    N = 255
    raw, ids = _problem(N, (N, 200), seed=2)
    top = raw.amax(-1) + 5.0
    raw[:, :, lo] = top
    raw[:, :, hi] = top
    _, _, al, align, _ = _fwd(raw, ids, rows=False)
    assert torch.equal(al[:, :, lo], al[:, :, hi]) and torch.equal(al.amax(-1), al[:, :, lo])
    assert torch.equal(align, torch.full((B, T), lo, dtype=torch.int64))


# rel-L2 deviation of the NARROW backward kernel (unchanged by the wide pair) from the float64 formula at N = 60, inputs drawn as
# below: 5.124e-8, measured once on MI355X (the wide kernels measured 4.8e-8 .. 5.9e-8).  The wide kernel may
# deviate twice as much.
_BWD_NARROW_RELL2 = 5.124e-8


def _bwd_rell2(N):
    from aptai_amd import ops
    raw, ids = _problem(N, (N, N // 2), seed=3)
    _, a, al, _, _ = _fwd(raw, ids, rows=False)
    g = torch.Generator().manual_seed(77 + N)
    ld = _ld(N)
    d_att = torch.randn(B * T, N, generator=g)
    d_rows = torch.randn(B * T, ld, generator=g)                                   # d_attlog = columns 1..N of rows at pitch ld
    a2, al2 = a.reshape(B * T, N), al.reshape(B * T, N)
    d_rows_c = d_rows.cuda()
    got = ops.xattn_softmax_bwd(a2.cuda().contiguous(), al2.cuda().contiguous(), d_att.cuda(), d_rows_c[:, 1:], ld_dattlog=ld).cpu()
    dl = d_rows[:, 1:N + 1].double()
    ref = a2.double() * (d_att.double() - (a2.double() * d_att.double()).sum(-1, keepdim=True)) + dl \
        - al2.double().exp() * dl.sum(-1, keepdim=True)
    return ((got.double() - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("N", [65, 130, 192, 255])
def test_wide_softmax_backward(N):
    narrow = _bwd_rell2(60)
    wide = _bwd_rell2(N)
    print(f"[long] softmax backward rel-L2 vs float64: narrow N=60 {narrow:.3e}, wide N={N} {wide:.3e}")
    assert wide <= 2 * _BWD_NARROW_RELL2, (wide, narrow)


def test_the_cap_does_not_change_a_short_transcript():
    """N = 130 with ids zero from slot 60 on against the narrow kernel at N = 60 on raw[:, :, :60]: equal bits in columns < 60
    and equal indices (masked slots sit near -1000 / -2000: their exponentials are exactly 0)."""
    raw, ids = _problem(130, (60, 17), seed=4)
    e, a, al, align, _ = _fwd(raw, ids)
    e0, a0, al0, align0, _ = _fwd(raw[:, :, :60].contiguous(), ids[:, :60].contiguous())
    assert torch.equal(e[:, :, :60], e0) and torch.equal(a[:, :, :60], a0) and torch.equal(al[:, :, :60], al0)
    assert torch.equal(align, align0)
    # fs_rows=True: the op allocates the rows at the right pitch and returns them; a buffer at another pitch is refused
    from aptai_amd import ops
    from aptai_amd._lib import AptaiHipError
    rc, ic = raw.reshape(B * T, 130).contiguous().cuda(), ids.cuda()
    out = ops.xattn_softmax_fwd(rc, ic, B, T, 130, fs_rows=True)
    assert len(out) == 5 and tuple(out[4].shape) == (B * T, 192) and torch.equal(out[4].cpu()[:, 1:131], al.reshape(B * T, 130))
    with pytest.raises(AptaiHipError):
        ops.xattn_softmax_fwd(rc, ic, B, T, 130, fs_rows=torch.empty(B * T, 128, device="cuda"))
    with pytest.raises(AptaiHipError):
        ops.xattn_softmax_fwd(torch.empty(B * T, 256, device="cuda"), torch.ones(B, 256, dtype=torch.int32, device="cuda"), B, T, 256)


# ------------------------------------------------------------------------------------------------ modules
def _rel(a, b):
    return ((a.detach().cpu().double() - b.detach().double()).norm() / (b.detach().double().norm() + 1e-30)).item()


@pytest.mark.parametrize("N,text,Tm,mel", [(130, (129, 70), 149, (149, 140)), (255, (254, 61), 259, (259, 124))])
def test_forward_sum_loss_beyond_63_slots(N, text, Tm, mel):
    """ForwardSumLoss on its own (also: the CTC loss / gradient kernels at up to 254 labels and 255 classes) against
    heads_ref.forward_sum_loss, the bounds tests/test_gpu_parity2.py uses at 60 slots."""
    from aptai_amd import modules as M
    from oracle import heads_ref
    g = torch.Generator().manual_seed(N)
    x = 8.0 * torch.randn(2, Tm, N, generator=g)
    for b in range(2):
        x[b, :, text[b]:] -= 2000.0
    att = torch.log_softmax(x, -1)
    a_g = att.cuda().unsqueeze(1).requires_grad_(True)
    loss = M.ForwardSumLoss()(a_g, list(text), list(mel))
    loss.backward()
    a_o = att.clone().unsqueeze(1).requires_grad_(True)
    ref = heads_ref.forward_sum_loss(a_o, list(text), list(mel))
    ref.backward()
    print(f"[long] forward-sum N={N}: loss {loss.item():.6f} oracle {ref.item():.6f}, grad rel-L2 {_rel(a_g.grad, a_o.grad):.3e}")
    assert abs(loss.item() - ref.item()) < 2e-4 * abs(ref.item())
    assert _rel(a_g.grad, a_o.grad) < 2e-3


def test_cross_attention_at_130_slots():
    from aptai_amd import modules as M
    from aptai_amd.config import W2V2Config
    from oracle import heads_ref, synth
    z, meta = load_golden("force_aptai_1x2s")
    pr_cfg = W2V2Config.from_any(meta["pr_cfg"])
    sd = synth.make_state_dict(synth.force_aptai_param_shapes(pr_cfg, meta["vocab_len"]), meta["seed"])
    g = torch.Generator().manual_seed(9)
    N, Tm = 130, 149
    xatt = M.CrossAttention(128, 128, 128).cuda()
    xatt.load_state_dict({k[len("xatt."):]: v for k, v in sd.items() if k.startswith("xatt.")})
    scale = float(torch.from_numpy(z["b2/frame"]).std()), float(torch.from_numpy(z["b2/phn_embs"]).std())
    frame, phn = scale[0] * torch.randn(2, Tm, 128, generator=g), scale[1] * torch.randn(2, N, 128, generator=g)
    mask = (torch.arange(N)[None, :] < torch.tensor([129, 70])[:, None]).to(torch.int)
    fr_g, ph_g = frame.cuda().requires_grad_(True), phn.cuda().requires_grad_(True)
    att_out, energy = xatt(fr_g, ph_g, mask.cuda())
    wgt = torch.randn(att_out.shape, generator=g)
    (att_out * wgt.cuda()).sum().backward()
    sdo = {k: v.clone().requires_grad_(v.dtype == torch.float32) for k, v in sd.items() if k.startswith("xatt.")}
    fr_o, ph_o = frame.clone().requires_grad_(True), phn.clone().requires_grad_(True)
    ao, eo = heads_ref.cross_attention(sdo, fr_o, ph_o, mask)
    (ao * wgt).sum().backward()
    print(f"[long] CrossAttention N=130: att_out max err {(att_out.detach().cpu() - ao.detach()).abs().max().item():.3e}, "
          f"grads rel-L2 frame {_rel(fr_g.grad, fr_o.grad):.3e} phn {_rel(ph_g.grad, ph_o.grad):.3e}")
    assert np.allclose(att_out.detach().cpu().numpy(), ao.detach().numpy(), atol=2e-4)
    assert np.allclose(energy.detach().cpu().numpy(), eo.detach().numpy(), rtol=1e-5, atol=2e-4)
    assert _rel(fr_g.grad, fr_o.grad) < 2e-3 and _rel(ph_g.grad, ph_o.grad) < 2e-3
    for n, p in xatt.named_parameters():
        assert _rel(p.grad, sdo["xatt." + n].grad) < 2e-3, n


# ------------------------------------------------------------------------------------------------ model
def _setup():
    from aptai_amd.config import W2V2Config
    from oracle import synth
    z, meta = load_golden("force_aptai_1x2s")
    pr_cfg = W2V2Config.from_any(meta["pr_cfg"])
    sd = synth.make_state_dict(synth.force_aptai_param_shapes(pr_cfg, meta["vocab_len"]), meta["seed"])
    sd["w2v2_pr.pr_head.bias"][0] += meta["blank_bias"]
    return pr_cfg, sd


def _build_cap(pr_cfg, sd, cap=None):
    from aptai_amd.force_aptai import Force_APTAI
    from test_gpu_force import _pr_ckpt
    vocab = {"(blank)": 0, "(...)": 1}
    vocab.update({f"p{i}": i for i in range(2, 40)})
    with tempfile.TemporaryDirectory() as tmp:
        path = _pr_ckpt(tmp, pr_cfg, sd, vocab)
        model = Force_APTAI(path, "cuda", vocab) if cap is None else Force_APTAI(path, "cuda", vocab, max_phn_seq_len=cap)
    model.load_state_dict(sd)                         # sd carries the 60-row pe_phn.pe: a cap-60 checkpoint into any cap
    return model.cuda()


def _batch(pr_cfg, S, lens, seed):
    from oracle.w2v2_ref import feat_extract_output_lengths
    g = torch.Generator().manual_seed(seed)
    lens = torch.tensor(lens, dtype=torch.long)
    audio = torch.randn(2, S, generator=g) * (torch.arange(S)[None, :] < lens[:, None])
    Tm = int(feat_extract_output_lengths(torch.tensor(S), pr_cfg))
    fl = feat_extract_output_lengths(lens, pr_cfg)
    valid = torch.arange(Tm)[None, :] < fl[:, None]
    out = {"audio_inputs": audio, "audio_lengths": lens, "phn_frames_49hz": (torch.randint(1, 40, (2, Tm), generator=g) * valid).long()}
    for n in TV:
        tv = torch.randn(2, Tm, generator=g, dtype=torch.float64)
        out[n] = torch.where(valid, tv, torch.full_like(tv, -100.0))
    return out, [int(v) for v in fl]


def _case(cap, S, lens, frames, text, seed):
    """One model-level case: oracle forward + backward at `cap`, and the model's step on the oracle's fp32 embeddings with the
    same transcripts (dropouts 0), as the second half of test_force_aptai_b2_against_oracle does."""
    from oracle import heads_ref
    pr_cfg, sd = _setup()
    batch, fl = _batch(pr_cfg, S, lens, seed)
    assert tuple(fl) == frames
    g = torch.Generator().manual_seed(seed + 1)
    lists = [torch.randint(1, 40, (n,), generator=g).numpy() for n in text]
    sdo = {k: v.clone() for k, v in sd.items()}
    sdo["pe_phn.pe"] = heads_ref.positional_encoding(128, cap)
    for k, v in sdo.items():
        if v.dtype == torch.float32 and not k.startswith("w2v2_pr.") and k != "pe_phn.pe":
            v.requires_grad_(True)
    ref = heads_ref.force_aptai_forward(sdo, pr_cfg, batch["audio_inputs"], batch["audio_lengths"], [batch[n] for n in TV],
                                        phn_pred_list=lists, max_phn_seq_len=cap)
    ref["loss"].backward()
    with torch.no_grad():
        e = heads_ref.pr_get_embeddings(sd, pr_cfg, batch["audio_inputs"], batch["audio_lengths"], prefix="w2v2_pr.")
    model = _build_cap(pr_cfg, sd, cap)
    model.train()
    model.hidden_drop = 0.0
    model.rnn_drop = 0.0
    geo = model.w2v2_pr.wav2vec2._geometry(2, S)
    ac = torch.zeros(2, geo.Tp, pr_cfg.hidden_size)
    ac[:, :geo.T] = e["last_transf_hidden"].permute(0, 2, 1)
    ac = ac.view(2 * geo.Tp, -1).cuda().contiguous()
    cb = {k: v.cuda() for k, v in batch.items()}
    labels = torch.full((2, max(text)), -100, dtype=torch.int32)
    for b, l in enumerate(lists):
        labels[b, :len(l)] = torch.from_numpy(l).int()
    cb["phoneme_labels"] = labels.cuda()
    out = model(0, **cb, _phn_pred_list=lists, _ac_override=ac)
    out["loss"].backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    model.zero_grad(set_to_none=True)
    from types import SimpleNamespace
    return SimpleNamespace(cap=cap, pr_cfg=pr_cfg, sd=sd, sdo=sdo, ref=ref, model=model, cb=cb, ac=ac, lists=lists, out=out, grads=grads,
                           frames=frames)


@pytest.fixture(scope="module")
def case130():
    return _case(130, 48000, (48000, 45000), (149, 140), (129, 70), seed=21)


def _check_against_oracle(c):
    out, ref = c.out, c.ref
    for k in ("loss", "tv_loss", "align_loss"):
        print(f"[long] cap {c.cap} {k}: {out[k].item():.6f} oracle {ref[k].item():.6f}")
        assert abs(out[k].item() - ref[k].item()) <= 2e-4 * abs(ref[k].item()), (k, out[k].item(), ref[k].item())
    err = (out["tvs_pred"].detach().cpu() - ref["tvs_pred"].detach()).abs().max().item()
    print(f"[long] cap {c.cap} tvs_pred max |err| {err:.3e}")
    assert err <= 2e-4
    for b in range(2):
        assert out["pred_frame_phns"][b] == ref["pred_frame_phns"][b]
    bad, worst = [], {}
    for k, v in c.sdo.items():
        if v.grad is None:
            continue
        rel = _rel(c.grads[k], v.grad)
        fam = k.split(".")[0]
        worst[fam] = max(worst.get(fam, 0.0), rel)
        if rel > 2e-3:
            bad.append((k, round(rel, 5)))
    print(f"[long] cap {c.cap} head gradients rel-L2: " + ", ".join(f"{f} {r:.5f}" for f, r in worst.items()))
    assert not bad, bad


def test_force_aptai_cap_130_against_oracle(case130):
    _check_against_oracle(case130)


def test_force_aptai_cap_255_against_oracle():
    _check_against_oracle(_case(255, 83200, (83200, 40000), (259, 124), (254, 61), seed=22))


def test_monotonic_readout_at_cap_130(case130):
    """alignment_readout = "monotonic": the indices are the host Viterbi of the returned att_log rows."""
    from aptai_amd import hostlogic
    c, m = case130, case130.model
    m.alignment_readout = "monotonic"
    try:
        with torch.no_grad():
            res, geo, dec = m._run(c.cb["audio_inputs"], c.cb["audio_lengths"], None, c.lists, c.ac)
        torch.cuda.synchronize()
    finally:
        m.alignment_readout = "argmax"
    att_log = res[5].view(2, geo.Tp, c.cap).cpu().numpy()
    align = res[8].view(2, geo.Tp).cpu().numpy()
    for b in range(2):
        Tb, n = c.frames[b], len(c.lists[b])
        x = np.ascontiguousarray(att_log[b, :Tb, :n])
        ft, score = hostlogic.ctc_forced_align(x, Tb, list(range(n)), topology="monotonic")
        assert np.isfinite(score)
        assert align[b, :Tb].tolist() == [int(v) for v in ft]
        assert ft[0] == 0 and ft[-1] == n - 1


def test_transcript_from_labels_equals_the_given_lists(case130):
    """transcript = "labels": the batch's phoneme_labels (int, -100 padded) stand in for the decode - every output and gradient
    equals the `_phn_pred_list` run bit for bit, and the device-output route synchronises nothing."""
    c, m = case130, case130.model
    m.transcript = "labels"
    try:
        out = m(0, **c.cb, _ac_override=c.ac)
        out["loss"].backward()
        torch.cuda.synchronize()
        for k in ("loss", "tv_loss", "align_loss", "tvs_pred"):
            assert torch.equal(out[k], c.out[k]), k
        assert out["pred_frame_phns"] == c.out["pred_frame_phns"]
        assert [list(map(int, q)) for q in out["pred_ctc_phn_seq"]] == [list(map(int, q)) for q in c.lists]
        for n, p in m.named_parameters():
            assert (p.grad is None) == (n not in c.grads) and (p.grad is None or torch.equal(p.grad, c.grads[n])), n
        m.zero_grad(set_to_none=True)
        # no host synchronisation on the device-output route - if this build's sync debug mode catches one at all
        torch.cuda.set_sync_debug_mode("error")
        try:
            try:
                torch.ones(1, device="cuda").item()
                works = False
            except RuntimeError:
                works = True
            print(f"[long] torch.cuda sync debug mode catches a .item(): {works}")
            with torch.no_grad():
                dev_out = m(0, **c.cb, _ac_override=c.ac, _device_outputs=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(dev_out["loss"], c.out["loss"].detach())
        assert dev_out["ctc_lens"].tolist() == [len(l) for l in c.lists]
        # a transcript that does not fit: the count reaches the host uncut and trips the reference's assertion
        long = torch.randint(1, 40, (2, c.cap), dtype=torch.int32).cuda()
        with pytest.raises(AssertionError, match="max_phn_seq_len"):
            m(0, **{**c.cb, "phoneme_labels": long}, _ac_override=c.ac)
        m.transcript = "spoken"
        with pytest.raises(ValueError):
            m(0, **c.cb, _ac_override=c.ac)
    finally:
        m.transcript = "decoded"
        m.zero_grad(set_to_none=True)


def test_graphed_force_step_at_cap_130(case130):
    """GraphedForceStep picks the cap up from the model's head state: losses and updated parameters follow the eager loop, the
    assertion of test_graphed_force_step_matches_eager_and_varies_with_dropout."""
    from aptai_amd.graphed import GraphedForceStep
    from aptai_amd.optim import Adam
    c = case130
    batches = []
    for seed in (31, 32):
        bt = {k: v.cuda() for k, v in _batch(c.pr_cfg, 48000, (48000, 45000), seed)[0].items()}
        bt["phoneme_labels"] = torch.zeros(2, 4, dtype=torch.int32).cuda()
        batches.append(bt)

    def fresh():
        model = _build_cap(c.pr_cfg, c.sd, 130)
        model.train()
        model.hidden_drop = 0.0
        model.rnn_drop = 0.0
        with torch.no_grad():                                   # the random-weight recogniser must decode 1..129 phonemes
            blank = model.w2v2_pr._blank()
            for _ in range(60):
                n = [len(l) for bt in batches for l in
                     model.w2v2_pr._decode(model.w2v2_pr._logits_eval(bt["audio_inputs"], bt["audio_lengths"].reshape(-1)[:, None])[0])]
                if max(n) < 130 and min(n) >= 1:
                    break
                model.w2v2_pr.pr_head.bias[blank] += 0.25 if max(n) >= 130 else -0.25
            assert max(n) < 130 and min(n) >= 1, n
        params = [p for p in model.parameters() if p.requires_grad]
        return model, params, Adam(params, lr=1e-4)

    losses, finals = {}, {}
    for mode in ("eager", "graph"):
        model, params, opt = fresh()
        ls = []
        if mode == "eager":
            for i in range(3):
                opt.zero_grad(set_to_none=True)
                out = model(0, **batches[i % 2])
                out["loss"].backward()
                opt.step()
                ls.append(out["loss"].item())
        else:
            runner = GraphedForceStep(model, opt, batches[0])
            assert runner.st.nphn == 130
            for i in range(3):
                out = runner.step(batches[i % 2], next_batch=batches[(i + 1) % 2])
                ls.append(out["loss"].item())
            assert out["ids"].shape == (2, 130)
            runner.close()
        losses[mode] = ls
        finals[mode] = {n: p.detach().float().cpu().clone() for n, p in model.named_parameters() if p.requires_grad}
    for a, b in zip(losses["eager"], losses["graph"]):
        assert abs(a - b) <= 1e-4 * abs(a), (losses["eager"], losses["graph"])
    for n in finals["eager"]:
        d = (finals["eager"][n] - finals["graph"][n]).abs().max().item()
        assert d <= 2e-5, (n, d)


def test_checkpoints_across_caps_and_constructor_range(case130):
    from aptai_amd.force_aptai import Force_APTAI
    c = case130
    m60, m130 = _build_cap(c.pr_cfg, c.sd), c.model
    assert m60.max_phn_seq_len == 60 and m130.max_phn_seq_len == 130
    # the default-cap model saves what it always saved: the keys and shapes of the synthetic reference state dict
    sd60 = m60.state_dict()
    assert {k: tuple(v.shape) for k, v in sd60.items()} == {k: tuple(v.shape) for k, v in c.sd.items()}
    assert "max_phn_seq_len" not in m60.get_config() and m130.get_config()["max_phn_seq_len"] == 130
    sd130 = m130.state_dict()
    assert tuple(sd130["pe_phn.pe"].shape) == (130, 1, 128)
    assert torch.equal(sd130["pe_phn.pe"][:60], sd60["pe_phn.pe"])
    own = sd130["pe_phn.pe"].clone()
    m130.load_state_dict(sd60)                                   # cap 60 -> cap 130: the module keeps its own table
    assert torch.equal(m130.pe_phn.pe, own)
    m60.load_state_dict(sd130)                                   # and the reverse
    assert tuple(m60.pe_phn.pe.shape) == (60, 1, 128) and torch.equal(m60.pe_phn.pe, sd60["pe_phn.pe"])
    with pytest.raises(RuntimeError):                            # strict loading otherwise, as before
        m60.load_state_dict({k: v for k, v in sd60.items() if k != "frame_lin.bias"})
    for bad in (256, 1, 0, 60.0):
        with pytest.raises(ValueError):
            _build_cap(c.pr_cfg, c.sd, bad)
    # a transcript of `cap` phonemes does not fit: the reference's assertion, naming the knob
    with pytest.raises(AssertionError, match="Need longer max phoneme sequence length.*max_phn_seq_len="):
        m60(0, **c.cb, _phn_pred_list=[np.arange(1, 61) % 39 + 1, np.arange(1, 20)])
