"""GPU: the device evaluation metrics (csrc/eval.hip, aptai_amd.device_metrics) against the host implementation they replace in
validate() / test(): aptai_amd.metrics, itself pinned to the reference by tests/golden/metrics_small.npz (tests/test_cpu_metrics.py).
The Levenshtein yardstick is metrics.edit_distance plus the hand-checked cases of that file; its parity with the `editdistance`
package the reference calls is unpinned there, and therefore here.

Bounds.  u = 2^-53.  A fixed-order fp64 sum of T products over its norms is within (T+2)u of the exact value (Cauchy-Schwarz), the
two means and the final divide / square root add a few u more, and host and device each carry that error: RMSE is held to
4 (T+4) u relative and r to 4 (T+4) u absolute.  Tracks are generated with |mean| <= std so the centring error stays second order.
Counts, collapsed sequences and distances are integers: exact."""
import warnings

import numpy as np
import pytest
import torch

from aptai_amd import metrics

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
TVN = metrics.TV_NAMES


def _bound(T):
    return 4 * (T + 4) * U


def _host_tv(gt, pred):
    """metrics.tvs_metric_rmse / tvs_metric_ppc of fp32 [T][C] arrays -> (rmse [C], r [C]).  scipy refuses a single frame; the
    kernel's answer there is NaN (every track of one frame is constant)."""
    C = gt.shape[1]
    names = [str(i) for i in range(C)]
    rm = metrics.tvs_metric_rmse(gt, pred, names)
    if gt.shape[0] < 2:
        return np.array([rm[k] for k in names]), np.full(C, np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                  # scipy warns about the constant track
        pc = metrics.tvs_metric_ppc(gt, pred, names)
    return np.array([rm[k] for k in names]), np.array([pc[k][0] for k in names])


def _check_tv(rmse, pcc, want_rmse, want_pcc, T, what):
    b = _bound(T)
    err_rmse = np.max(np.abs(rmse - want_rmse) / np.abs(want_rmse))
    nan_w = np.isnan(want_pcc)
    print(f"[bands] {what}: T={T} rmse rel err {err_rmse:.2e}, r abs err "
          f"{np.max(np.abs(pcc - want_pcc)[~nan_w], initial=0.0):.2e}, bound {b:.2e}")
    assert err_rmse <= b, what
    assert np.array_equal(np.isnan(pcc), nan_w), (what, pcc, want_pcc)   # NaN where and only where the host gives NaN
    assert np.all(np.abs(pcc - want_pcc)[~nan_w] <= b), what


def test_tv_scores_on_the_golden_vectors(golden):
    from aptai_amd import device_metrics as dm
    gold = golden("metrics_small")[0]
    gt, pred = gold["tv/gt"].astype(np.float32), gold["tv/pred"].astype(np.float32)      # the loops hand over fp32 (`.float()`)
    rmse, pcc = dm.tv_scores(torch.from_numpy(gt).cuda(), torch.from_numpy(pred).cuda())
    assert rmse.dtype == pcc.dtype == torch.float64 and rmse.shape == pcc.shape == (9,)
    want_rmse, want_pcc = _host_tv(gt, pred)
    _check_tv(rmse.cpu().numpy(), pcc.cpu().numpy(), want_rmse, want_pcc, gt.shape[0], "golden tv")


@pytest.mark.parametrize("C", [9, 12])
@pytest.mark.parametrize("lens", [(1, 2, 63), (64, 65, 499)])
def test_tv_scores_random_lengths_pitches_poison_and_constant_track(C, lens):
    from aptai_amd import device_metrics as dm
    g = np.random.RandomState(100 * C + lens[0])
    B, Tmax = 3, max(lens)
    rows, ld = Tmax + 3, C + 5                                           # padded pitches: more rows and wider rows than used

    def make():
        std = g.uniform(0.5, 2.0, size=(B, 1, C))
        mean = g.uniform(-1.0, 1.0, size=(B, 1, C)) * std                # |mean| <= std
        return (g.randn(B, Tmax, C) * std + mean).astype(np.float32)
    gt, pred = make(), make()
    gt[1, :, 2] = np.float32(0.1)                                        # constant tracks: r is NaN, like scipy
    pred[0, :, 4] = np.float32(-3.25)
    bufs = []
    for a in (gt, pred):
        buf = torch.full((B, rows, ld), float("nan"))
        for b in range(B):
            buf[b, :lens[b], :C] = torch.from_numpy(a[b, :lens[b]])      # everything at or beyond lens[b] stays NaN
        bufs.append(buf.cuda())
    n = torch.tensor(lens, dtype=torch.int32).cuda()
    view = lambda t: t[:, :Tmax, :C]
    rmse, pcc = dm.tv_scores(view(bufs[0]), view(bufs[1]), n)
    rmse2, pcc2 = dm.tv_scores(view(bufs[0]), view(bufs[1]), n)
    assert torch.equal(rmse.view(torch.int64), rmse2.view(torch.int64)) and torch.equal(pcc.view(torch.int64), pcc2.view(torch.int64))
    rmse, pcc = rmse.cpu().numpy(), pcc.cpu().numpy()
    assert rmse.shape == (B, C) and not np.isnan(rmse).any()
    for b in range(B):
        want_rmse, want_pcc = _host_tv(gt[b, :lens[b]], pred[b, :lens[b]])
        _check_tv(rmse[b], pcc[b], want_rmse, want_pcc, lens[b], f"C={C} len={lens[b]}")
    assert np.isnan(pcc[1, 2]) and np.isnan(pcc[0, 4])


def test_tv_scores_empty_utterance_gives_nan_rows():
    from aptai_amd import device_metrics as dm
    x = torch.full((2, 8, 9), float("nan"))
    x[1, :5] = torch.randn(5, 9)
    y = x.clone()
    y[1, :5] += 0.5
    rmse, pcc = dm.tv_scores(x.cuda(), y.cuda(), torch.tensor([0, 5], dtype=torch.int32).cuda())
    assert torch.isnan(rmse[0]).all() and torch.isnan(pcc[0]).all()
    assert not torch.isnan(rmse[1]).any() and not torch.isnan(pcc[1]).any()


# ------------------------------------------------------------------------------------------------ labels
def _label_cases(golden):
    """(gt, pred) int64 label sequences: golden ovl/* plus random ones at lengths 1, 64, 65, 499, a run straddling 63 | 64, an
    all-equal sequence and an alternating one."""
    gold = golden("metrics_small")[0]
    g = np.random.RandomState(7)
    cases = [(gold[f"ovl/{i}/gt"], gold[f"ovl/{i}/pred"]) for i in range(3)]
    for T in (1, 64, 65, 499):
        gt = np.repeat(g.randint(1, 46, size=T // 3 + 1), 3)[:T]
        pred = np.where(g.rand(T) < 0.7, gt, g.randint(1, 46, size=T))
        cases.append((gt, pred))
    straddle = np.repeat(g.randint(1, 46, size=40), 4)[:130].copy()
    straddle[60:68] = 45                                                 # one run across positions 63 | 64
    straddle[59], straddle[68] = 3, 4
    cases.append((straddle, np.roll(straddle, 2)))
    cases.append((np.full(200, 7), np.full(200, 7)))                     # all equal
    cases.append((np.arange(129) % 2 + 1, (np.arange(129) + 1) % 2 + 1))  # alternating, never equal
    return [(np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)) for a, b in cases], gold


def _pack(seqs, width, poison, dtype):
    out = torch.full((len(seqs), width), poison, dtype=dtype)
    for i, s in enumerate(seqs):
        out[i, :len(s)] = torch.as_tensor(np.asarray(s)).to(dtype)
    return out


def test_frame_scores_boundary_counts_and_collapse_match_the_host(golden):
    from aptai_amd import device_metrics as dm
    cases, gold = _label_cases(golden)
    B, W = len(cases), 512
    gt = _pack([c[0] for c in cases], W, 12345, torch.int64).cuda()      # poison beyond the lengths
    pred = _pack([c[1] for c in cases], W + 8, 12345, torch.int64).cuda()
    n = torch.tensor([len(c[0]) for c in cases], dtype=torch.int32).cuda()
    fs = dm.frame_scores(gt, pred, n).cpu()
    bc = dm.boundary_counts(gt, n, pred, n, tolerance=0.02).cpu()
    (cg, ng), (cp, np_) = dm.collapse_runs(gt, n), dm.collapse_runs(pred, n)
    assert fs.dtype == bc.dtype == cg.dtype == ng.dtype == torch.int32
    cg, ng, cp, np_ = cg.cpu(), ng.cpu(), cp.cpu(), np_.cpu()
    for i, (a, b) in enumerate(cases):
        assert torch.equal(fs[i], torch.tensor([len(a), int((a == b).sum())], dtype=torch.int32)), i
        assert fs[i, 1].item() / fs[i, 0].item() == metrics.evaluate_overlap([a], [b])
        # get_metrics is injective in the two counters: equal scores <=> equal counts
        got = metrics.get_metrics(int(bc[i, 0]), int(bc[i, 1]), len(b), len(a))
        assert tuple(float(v) for v in got) == tuple(float(v) for v in metrics.get_stats(a, b, tolerance=0.02)), i
        for seq, c, m in ((a, cg, ng), (b, cp, np_)):
            want = metrics.phn_frame_id2phn(seq.tolist())
            assert int(m[i]) == len(want) and c[i, :len(want)].tolist() == want and not c[i, len(want):].any(), i
    for i in range(3):
        assert cg[i, :int(ng[i])].tolist() == gold[f"rle/{i}/phn"].tolist()
    assert int(ng[-2]) == 1 and int(ng[-1]) == 129


def test_boundary_counts_on_boundary_times(golden):
    from aptai_amd import device_metrics as dm
    gold = golden("metrics_small")[0]
    g = np.random.RandomState(3)
    pairs = [(gold[f"seg/{i}/y"], gold[f"seg/{i}/yhat"]) for i in range(3)]
    # 1500 x 1100 values on a 10 ms grid: more than one tile of owners, more than one staged chunk, many distances at 0.02
    pairs.append((np.sort(g.randint(0, 4000, size=1500)) * 0.01, np.sort(g.randint(0, 4000, size=1100)) * 0.01))
    pairs.append((np.array([0.5]), np.array([0.52])))
    pairs.append((np.array([1.0]), np.empty(0)))
    y = _pack([p[0] for p in pairs], 1536, float("nan"), torch.float64).cuda()
    yhat = _pack([p[1] for p in pairs], 1200, float("nan"), torch.float64).cuda()
    ny = torch.tensor([len(p[0]) for p in pairs], dtype=torch.int32).cuda()
    nh = torch.tensor([len(p[1]) for p in pairs], dtype=torch.int32).cuda()
    bc = dm.boundary_counts(y, ny, yhat, nh, tolerance=0.02).cpu()
    for i, (a, b) in enumerate(pairs[:-1]):
        d = np.abs(a[:, None] - b[None, :])
        want = [int((d.min(axis=0) <= 0.02).sum()), int((d.min(axis=1) <= 0.02).sum())]
        assert bc[i].tolist() == want, (i, bc[i].tolist(), want)
        got = metrics.get_metrics(int(bc[i, 0]), int(bc[i, 1]), len(b), len(a))
        assert tuple(float(v) for v in got) == tuple(float(v) for v in metrics.get_stats(a, b, tolerance=0.02)), i
    for i in range(3):
        got = metrics.get_metrics(int(bc[i, 0]), int(bc[i, 1]), len(pairs[i][1]), len(pairs[i][0]))
        np.testing.assert_allclose([float(v) for v in got], gold[f"seg/{i}/prf"], rtol=1e-12, atol=1e-15)
    assert bc[-1].tolist() == [0, 0]                                     # an empty side
    # a distance EXACTLY equal to the tolerance counts (dyadic values: 1.25 - 1.0 == 0.25 in fp64), one ulp beyond does not
    yy = torch.tensor([[1.0, 3.0], [1.0, 3.0]], dtype=torch.float64).cuda()
    hh = torch.tensor([[1.25, 2.0], [np.nextafter(1.25, 2.0), 2.0]], dtype=torch.float64).cuda()
    two = torch.tensor([2, 2], dtype=torch.int32).cuda()
    assert dm.boundary_counts(yy, two, hh, two, tolerance=0.25).cpu().tolist() == [[1, 1], [0, 0]]


# ------------------------------------------------------------------------------------------------ Levenshtein
def _edit(a_seqs, b_seqs, wa, wb):
    from aptai_amd import device_metrics as dm
    a = _pack(a_seqs, wa, 77777, torch.int32).cuda()
    b = _pack(b_seqs, wb, 88888, torch.int32).cuda()
    na = torch.tensor([len(s) for s in a_seqs], dtype=torch.int32).cuda()
    nb = torch.tensor([len(s) for s in b_seqs], dtype=torch.int32).cuda()
    d1, d2 = dm.edit_distance(a, na, b, nb), dm.edit_distance(a, na, b, nb)
    assert d1.dtype == torch.int32 and torch.equal(d1, d2)               # two calls: the same bits
    return d1.cpu().tolist()


@pytest.mark.parametrize("NS", [1, 4, 8, 16, 32])
def test_edit_distance_every_instantiation_at_its_edges(NS):
    """`a` is 64*NS symbols wide and `b` at least as wide, so `a` stays on the lanes and the NS instantiation is the one under test."""
    g = np.random.RandomState(NS)
    wa = 64 * NS
    a_lens = sorted({n for n in (0, 1, 63, 64, 65, 64 * NS, 64 * NS - 1) if n <= wa})
    a_seqs, b_seqs = [], []
    for na in a_lens:
        for nb in (0, 1, 2, 64, 200):
            a_seqs.append(g.randint(1, 6, size=na))
            b_seqs.append(g.randint(1, 6, size=nb))
    n0 = min(wa, 200)
    same = g.randint(1, 40, size=n0)
    a_seqs += [same, g.randint(1, 20, size=n0), g.randint(1, 20, size=wa)]
    b_seqs += [same.copy(), g.randint(20, 40, size=150), g.randint(20, 40, size=200)]      # equal; disjoint alphabets twice
    got = _edit(a_seqs, b_seqs, wa, max(wa, 200))
    want = [metrics.edit_distance(a.tolist(), b.tolist()) for a, b in zip(a_seqs, b_seqs)]
    assert got == want
    assert got[-3] == 0 and got[-2] == max(n0, 150) and got[-1] == max(wa, 200)


def test_edit_distance_hand_checked_mixed_batch_swap_and_refusal():
    from aptai_amd import device_metrics as dm
    from aptai_amd._lib import AptaiHipError
    k, s = [ord(c) for c in "kitten"], [ord(c) for c in "sitting"]
    assert _edit([[1, 2, 3, 4], [1, 2, 3, 4], [1, 2, 3], k], [[1, 2, 3, 4], [1, 3, 4], [1, 9, 2, 3, 7], s], 8, 8) == [0, 1, 2, 3]
    g = np.random.RandomState(0)
    # one batch: an empty pair, a short pair and a pair with a 2048-symbol side
    a_seqs = [np.empty(0, dtype=np.int64), g.randint(1, 5, size=7), g.randint(1, 5, size=2048)]
    b_seqs = [np.empty(0, dtype=np.int64), g.randint(1, 5, size=5), g.randint(1, 5, size=300)]
    want = [metrics.edit_distance(a.tolist(), b.tolist()) for a, b in zip(a_seqs, b_seqs)]
    assert want[0] == 0
    assert _edit(a_seqs, b_seqs, 2048, 2048) == want
    # only `b` fits the lanes: the wrapper swaps the sides, the distance is symmetric
    long_a, short_b = [g.randint(1, 5, size=2500), g.randint(1, 5, size=3)], [g.randint(1, 5, size=100), np.empty(0, dtype=np.int64)]
    want = [metrics.edit_distance(a.tolist(), b.tolist()) for a, b in zip(long_a, short_b)]
    assert _edit(long_a, short_b, 3000, 100) == want and want[1] == 3
    assert _edit(short_b, long_a, 100, 3000) == want
    # both sides beyond 2048: refused, and the text names the two lengths
    a = torch.zeros((1, 2049), dtype=torch.int32).cuda()
    b = torch.zeros((1, 2100), dtype=torch.int32).cuda()
    one = torch.tensor([5], dtype=torch.int32).cuda()
    with pytest.raises(AptaiHipError) as e:
        dm.edit_distance(a, one, b, one)
    assert "2049" in str(e.value) and "2100" in str(e.value) and "2048" in str(e.value)


# ------------------------------------------------------------------------------------------------ loops
INT_KEYS = ("FER", "PER", "overlap", "F1", "_p", "_r", "Rval")


def _compare(host, dev, T):
    """Same keys; integer-derived entries equal; RMSE / loss relative and PCC absolute within the bound for the longest utterance."""
    assert set(host) == set(dev)
    b = _bound(T)
    for k, v in host.items():
        if any(k.endswith(s) for s in INT_KEYS):
            assert dev[k] == v, (k, v, dev[k])
        elif k.endswith("pcc"):
            print(f"[bands] {k}: |dev - host| = {abs(dev[k] - v):.2e} (bound {b:.2e})")
            assert abs(dev[k] - v) <= b, (k, v, dev[k])
        else:
            print(f"[bands] {k}: rel |dev - host| = {abs(dev[k] - v) / abs(v):.2e} (bound {b:.2e})")
            assert abs(dev[k] - v) <= b * abs(v), (k, v, dev[k])


def _aptai_model(tmp_path):
    from aptai_amd import train_aptai as T
    from aptai_amd.config import W2V2Config
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    w2v = W2V2Config.base(vocab_size=T.VOCAB_SIZE, num_hidden_layers=2)
    torch.manual_seed(0)
    d = tmp_path / "w2v"
    Wav2Vec2Model(w2v).save_pretrained(str(d))
    cfg = T.default_cfg(huggingface_model_id=str(d), pretrain_cfg=w2v)
    model, _, _ = T.load_model_optimizer(cfg)
    model.eval()
    return T, cfg, w2v, model


def test_train_aptai_validate_and_test_device_path(tmp_path):
    from aptai_amd import hostlogic
    T, cfg, w2v, model = _aptai_model(tmp_path)
    dl = torch.utils.data.DataLoader(T.SyntheticHPRC(3, 1.0, seed=5, cfg=w2v), batch_size=1, collate_fn=hostlogic.collate_aptai)
    host = T.validate(model, "cuda", cfg.vocab, 0, None, "synthetic", dl)
    dev = T.validate(model, "cuda", cfg.vocab, 0, None, "synthetic", dl, device_metrics=True)
    _compare(host, dev, 49)
    host = T.test(model, "cuda", cfg.vocab, None, "synthetic", dl, "F", num_epochs=2)
    dev = T.test(model, "cuda", cfg.vocab, None, "synthetic", dl, "F", num_epochs=2, device_metrics=True)
    _compare(host, dev, 49)


def test_train_aptai_device_path_at_batch_size_three(tmp_path):
    """Three utterances of three lengths in ONE batch through the device path, against aptai_amd.metrics applied per utterance to
    the same batched outputs cut to their lengths (the forward is deterministic: a second pass gives the same tensors)."""
    from aptai_amd import hostlogic
    T, cfg, w2v, model = _aptai_model(tmp_path)
    ds = torch.utils.data.ConcatDataset([T.SyntheticHPRC(1, sec, vary_length=False, seed=9 + i, cfg=w2v)
                                         for i, sec in enumerate((1.0, 0.8, 0.6))])
    dl = torch.utils.data.DataLoader(ds, batch_size=3, collate_fn=hostlogic.collate_aptai)
    dev = T.validate(model, "cuda", cfg.vocab, 0, None, "synthetic", dl, device_metrics=True)
    batch = next(iter(dl))
    with torch.no_grad():
        out = model(0, **{k: v.cuda() for k, v in batch.items()})
    lens = [int(hostlogic.feat_extract_output_lengths(int(n), w2v.conv_kernel, w2v.conv_stride)) for n in batch["audio_lengths"]]
    assert len(set(lens)) == 3
    tvs_gt = T._stack_gt(batch).numpy()
    tvs_pred, pf, gf = out["tvs_pred"].float().cpu().numpy(), out["phn_fc_pred"].cpu().numpy(), batch["phn_frames_49hz"].numpy()
    rm, pc, ov, st, ed, nph, corr = [], [], [], [], [], [], 0
    for b, L in enumerate(lens):
        g, p, y, yhat = tvs_gt[b, :L], tvs_pred[b, :L], gf[b, :L], pf[b, :L]
        rm.append(np.mean(list(metrics.tvs_metric_rmse(g, p).values())))
        pc.append(np.mean([v[0] for v in metrics.tvs_metric_ppc(g, p).values()]))
        ov.append(metrics.evaluate_overlap([y], [yhat]))
        st.append(metrics.get_stats(y, yhat, tolerance=0.02))
        y_grp, h_grp = metrics.phn_frame_id2phn(y.tolist()), metrics.phn_frame_id2phn(yhat.tolist())
        ed.append(metrics.compute_PER(y_grp, h_grp) / 100.0 * len(y_grp))
        nph.append(len(y_grp))
        corr += int((y == yhat).sum())
    host = {"val_mean_loss": float(out["loss"].item()), "val_mean_rmse": float(np.mean(rm)), "val_mean_pcc": float(np.mean(pc)),
            "val_mean_FER": 1 - (corr / sum(lens)), "val_mean_PER": float(np.sum(ed) / np.sum(nph)),
            "val_mean_F1": float(np.mean([s[2] for s in st])), "val_mean_p": float(np.mean([s[0] for s in st])),
            "val_mean_r": float(np.mean([s[1] for s in st])), "val_mean_Rval": float(np.mean([s[3] for s in st])),
            "val_mean_overlap": float(np.mean(ov))}
    _compare(host, dev, max(lens))


def test_train_force_aptai_validate_and_test_device_path(tmp_path):
    import pickle
    from aptai_amd import train_force_aptai as T
    from aptai_amd.config import W2V2Config
    from aptai_amd.w2v2_pr import Wav2Vec2_PR
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    cfg0 = T.default_cfg()
    w2v = W2V2Config.base(vocab_size=len(cfg0.vocab), num_hidden_layers=2, ctc_loss_reduction="mean", ctc_zero_infinity=True)
    torch.manual_seed(0)
    mdir = tmp_path / "w2v2"
    Wav2Vec2Model(w2v).save_pretrained(str(mdir))
    pr = Wav2Vec2_PR(w2v, None, str(mdir), cfg0.vocab)
    with torch.no_grad():
        pr.pr_head.bias[0] += 3.0                                        # a trained recogniser's regime: mostly blank frames
    ck = tmp_path / "pr" / "best-model-ckpt"
    ck.mkdir(parents=True)
    torch.save(pr.state_dict(), ck / "pytorch_model.bin")
    pickle.dump({"pretrain_cfg": w2v.to_dict(), "cache_dir": None, "huggingface_model_id": str(mdir)}, open(ck / "model_cfg.pkl", "wb"))
    cfg = T.default_cfg(pr_model_path=str(tmp_path / "pr"))
    torch.manual_seed(1)
    model, _, _ = T.load_model_optimizer(cfg)
    model.eval()
    dl = torch.utils.data.DataLoader(T.SyntheticHPRCWithLabels(3, 1.0, seed=2, cfg=w2v, vocab_size=40), batch_size=1,
                                     collate_fn=T.collate)
    host = T.validate(model, "cuda", cfg.vocab, 0, None, "synthetic", dl)
    dev = T.validate(model, "cuda", cfg.vocab, 0, None, "synthetic", dl, device_metrics=True)
    _compare(host, dev, 49)
    host = T.test(model, "cuda", cfg.vocab, None, "synthetic", dl, "N")
    dev = T.test(model, "cuda", cfg.vocab, None, "synthetic", dl, "N", device_metrics=True)
    assert "test_N_std_PER" in dev and "test_N_std_overlap" in dev
    _compare(host, dev, 49)


def test_train_phoneme_recognizer_validate_and_test_device_path(tmp_path):
    from aptai_amd import hostlogic, train_phoneme_recognizer as T
    from aptai_amd.config import W2V2Config
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    vocab = T.default_vocab()
    w2v = W2V2Config.base(num_hidden_layers=2, layerdrop=0.0)
    torch.manual_seed(0)
    d = tmp_path / "w2v"
    Wav2Vec2Model(w2v).save_pretrained(str(d))
    cfg = T.default_cfg(huggingface_model_id=str(d), pretrain_cfg=w2v)
    model, _, _ = T.load_model_optimizer(cfg, vocab)
    model.eval()
    dl = torch.utils.data.DataLoader(T.SyntheticCommonPhone(3, 1.0, len(vocab), seed=2), batch_size=1, collate_fn=hostlogic.collate_pr)
    host = T.validate(model, "cuda", vocab, 0, dl)
    dev = T.validate(model, "cuda", vocab, 0, dl, device_metrics=True)
    assert set(host) == set(dev) == {"mean_val_per", "mean_val_loss"}
    assert dev["mean_val_per"] == host["mean_val_per"]
    assert abs(dev["mean_val_loss"] - host["mean_val_loss"]) <= _bound(49) * abs(host["mean_val_loss"])
    assert T.test(model, "cuda", vocab, dl, "synthetic", device_metrics=True) == T.test(model, "cuda", vocab, dl, "synthetic")
