"""CPU: the three training loops (train_aptai, train_force_aptai, train_phoneme_recognizer) and their host validate() / test()
paths, end to end on `device="cpu"` with a stub model, `torch.optim.Adam` and the real collates over the synthetic corpora.

What is pinned is what the loops promise besides their arithmetic: the exact log lines, `history` value for value and key for
key, the order of the checkpoint writes (a tie on the target metric saves again), the order of loader pulls, train steps and
validation passes, the life cycle of the graphed runner and of the clip monitor, and the key order of every evaluation dictionary.

The stub's arithmetic is exact: its loss is `0 * w` plus a multiple of 1/4, so the gradient is zero, Adam leaves `w` alone and
every logged loss and learning rate is a binary fraction.  The counting metrics (FER, PER, overlap, boundary scores) are ratios
of small integers formed in scalar Python.  Only the RMSE / Pearson entries go through numpy reductions and scipy over random
trajectories, whose last bit may depend on the host's vector width: those are compared to 1e-12 relative, everything else
exactly."""
import pickle
import random
from pathlib import Path

import pytest
import torch

from aptai_amd import hostlogic, metrics
from aptai_amd.config import W2V2Config

TVN = metrics.TV_NAMES
VAL_KEYS = ["val_mean_loss", "val_mean_rmse", "val_mean_pcc", "val_mean_FER", "val_mean_PER", "val_mean_F1", "val_mean_p",
            "val_mean_r", "val_mean_Rval", "val_mean_overlap"]


def _test_keys(rate, with_std):
    std = lambda k: [f"test_{rate}_std_{k}"] if with_std else []
    return ([f"test_{rate}_mean_rmse", f"test_{rate}_mean_pcc"] + std("rmse") + std("pcc")
            + [f"test_{rate}_mean_{n}_pcc" for n in TVN] + [f"test_{rate}_mean_{n}_rmse" for n in TVN]
            + [f"test_{rate}_mean_FER", f"test_{rate}_mean_PER"] + std("PER") + [f"test_{rate}_mean_overlap"] + std("overlap")
            + [f"test_{rate}_mean_F1", f"test_{rate}_mean_p", f"test_{rate}_mean_r", f"test_{rate}_mean_Rval"])


def _same(got, want):
    """Equal key for key, in order; RMSE / Pearson entries to 1e-12 relative (module docstring), the rest exactly."""
    assert list(got) == list(want)
    for k, v in want.items():
        if "rmse" in k or "pcc" in k:
            assert got[k] == pytest.approx(v, rel=1e-12, abs=1e-12), k
        else:
            assert got[k] == v and type(got[k]) is type(v), (k, got[k], v)


class _Loader:
    """The batches of a DataLoader, collated once; every pull of a batch is an event."""

    def __init__(self, dl, events, extra_len=0):
        self.batches, self.events, self.extra_len = list(dl), events, extra_len

    def __len__(self):
        return len(self.batches) + self.extra_len

    def __iter__(self):
        for i, b in enumerate(self.batches):
            self.events.append(("pull", i))
            yield b


class _Stub(torch.nn.Module):
    """Training: loss = 0 * w + (number of the train step) / 4.  Evaluation: loss 1/2.  Predictions are fixed functions of the batch."""

    def __init__(self, events):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))
        self.events, self.steps = events, 0

    def get_config(self):
        return {"stub": True}

    def _loss(self):
        if self.training:
            self.steps += 1
        return self.w * 0 + (self.steps / 4 if self.training else 0.5)


class _TVStub(_Stub):
    def forward(self, epoch, **batch):
        self.events.append(("train" if self.training else "eval", epoch, tuple(batch["audio_inputs"].shape)))
        loss = self._loss()
        gt = torch.stack([batch[n] for n in TVN], dim=-1).float()
        pred = batch["phn_frames_49hz"].clone()
        pred[:, ::3] = 1
        return {"loss": loss, "mse_loss": loss * 0.5, "ce_loss": loss * 0.25, "tvs_pred": torch.roll(gt, 1, dims=1) * 0.5,
                "phn_fc_pred": pred}


class _ForceStub(_Stub):
    def forward(self, epoch, _prefetch_next="absent", **batch):
        self.events.append(("train" if self.training else "eval", epoch, tuple(batch["audio_inputs"].shape), _prefetch_next))
        loss = self._loss()
        gt = torch.stack([batch[n] for n in TVN], dim=-1).float()
        pred = batch["phn_frames_49hz"].clone()
        pred[:, 1::4] = 2
        ctc = [[int(v) for i, v in enumerate(row) if v >= 0 and i % 4] for row in batch["phoneme_labels"].tolist()]
        return {"loss": loss, "tv_loss": loss * 0.5, "align_loss": loss * 0.25, "tvs_pred": torch.roll(gt, 2, dims=1) * 0.25,
                "pred_ctc_phn_seq": ctc, "pred_frame_phns": pred.tolist()}


class _PRStub(_Stub):
    def _blank(self):
        return 0

    def forward(self, **batch):
        self.events.append(("train" if self.training else "eval", tuple(batch["input_values"].shape)))
        B, S = batch["input_values"].shape
        return {"loss": self._loss(), "phoneme_logits": torch.zeros(B, S // 320, 8)}


def _fake_decode(lg, ldv, ldt, B, T, V, blank, max_n):
    """Stands for ops.ctc_greedy_decode (a device kernel): T // 2 ids counting up from 3."""
    n = T // 2
    ids = torch.zeros(B, T, dtype=torch.int32)
    ids[:, :n] = torch.arange(3, 3 + n, dtype=torch.int32)
    return ids, torch.full((B,), n, dtype=torch.int32)


@pytest.fixture
def writes(monkeypatch, tmp_path):
    """Every torch.save / pickle.dump under tmp_path, in order."""
    rec = []
    real_save, real_dump = torch.save, pickle.dump

    def save(obj, f, *a, **k):
        rec.append(str(Path(f).relative_to(tmp_path)))
        return real_save(obj, f, *a, **k)

    def dump(obj, f, *a, **k):
        rec.append(str(Path(f.name).relative_to(tmp_path)))
        return real_dump(obj, f, *a, **k)
    monkeypatch.setattr(torch, "save", save)
    monkeypatch.setattr(pickle, "dump", dump)
    return rec


def _files(path):
    return {str(p.relative_to(path)) for p in Path(path).rglob("*") if p.is_file()}


def _optim(T, model, **kw):
    """Adam + LambdaLR as load_model_optimizer builds them, on the stub's parameter.  Factors 2.5, 5, 7.5 over lr 1/8."""
    cfg = T.default_cfg(device="cpu", num_epochs=2, batch_size=2, learning_rate=0.125, num_warmup_epochs=4, **kw)
    opt = torch.optim.Adam(model.parameters(), lr=cfg.learning_rate, betas=(cfg.adam_beta1, cfg.adam_beta2), eps=cfg.adam_epsilon,
                           weight_decay=cfg.adam_weight_decay)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, hostlogic.get_lr_schedule(cfg.num_warmup_epochs, cfg.num_static_epochs, cfg.lr_decay))
    return cfg, opt, sched


class _Runner:
    """Recorder in the place of aptai_amd.graphed.BucketedGraphedStep: runs the eager step so the loop goes on."""
    call = None                     # how the loop's model is called: set per test
    made = []

    def __init__(self, model, optimizer):
        self.model, self.optimizer = model, optimizer
        _Runner.made.append(self)

    def step(self, batch):
        self.model.events.append(("runner.step", batch))
        self.optimizer.zero_grad()
        out = _Runner.call(self.model, batch)
        out["loss"].backward()
        self.optimizer.step()
        return out

    def suspend(self):
        self.model.events.append(("runner.suspend",))

    def close(self):
        self.model.events.append(("runner.close",))


@pytest.fixture
def runner(monkeypatch):
    from aptai_amd import graphed
    _Runner.made = []
    monkeypatch.setattr(graphed, "BucketedGraphedStep", _Runner)
    return _Runner


class _Clip:
    """In the place of aptai_amd.optim.ClipMonitor (which reads the HIP optimiser's device scalars)."""
    made = []

    def __init__(self, optimizer):
        self.optimizer, self.updates, self.per_epoch = optimizer, 0, []
        _Clip.made.append(self)

    def update(self):
        self.updates += 1

    def epoch_log(self):
        self.per_epoch.append(self.updates)
        out = dict(mean_grad_norm=self.updates / 2, clipped_steps=self.updates)
        self.updates = 0
        return out


@pytest.fixture
def clip(monkeypatch):
    from aptai_amd import optim
    _Clip.made = []
    monkeypatch.setattr(optim, "ClipMonitor", _Clip)
    return _Clip


# ------------------------------------------------------------------------------------------------------------ recorded values
# What the loops returned and logged before their shared parts were factored out, on the stubs above.
APTAI_VAL = {"val_mean_loss": 0.5, "val_mean_rmse": 1.1579896234677078, "val_mean_pcc": -0.0869905722104546,
             "val_mean_FER": 0.32608695652173914, "val_mean_PER": 1.66665, "val_mean_F1": 0.8999947060876787,
             "val_mean_p": 0.8333329671718783, "val_mean_r": 0.9999995643941295, "val_mean_Rval": 0.7866114956903416,
             "val_mean_overlap": 0.6742424242424242}
APTAI_TEST = {"test_F_mean_rmse": 1.1579896234677076, "test_F_mean_pcc": -0.08699057221045461,
              "test_F_mean_LA_pcc": 0.07885058558158109, "test_F_mean_LP_pcc": -0.11836280166686192,
              "test_F_mean_JA_pcc": -0.1144557385183334, "test_F_mean_TTCL_pcc": -0.14417943163116081,
              "test_F_mean_TTCD_pcc": -0.014983703871741721, "test_F_mean_TMCL_pcc": -0.09376475929482105,
              "test_F_mean_TMCD_pcc": -0.21691939528114584, "test_F_mean_TBCL_pcc": -0.04506843018076122,
              "test_F_mean_TBCD_pcc": -0.11403147503084657, "test_F_mean_LA_rmse": 1.124391670542578,
              "test_F_mean_LP_rmse": 1.2805692014253172, "test_F_mean_JA_rmse": 1.1815115526014566,
              "test_F_mean_TTCL_rmse": 1.210211510331246, "test_F_mean_TTCD_rmse": 1.0760733801217977,
              "test_F_mean_TMCL_rmse": 1.0455429899550865, "test_F_mean_TMCD_rmse": 1.1678098775952268,
              "test_F_mean_TBCL_rmse": 1.1111540188539728, "test_F_mean_TBCD_rmse": 1.2246424097826898,
              "test_F_mean_FER": 0.32608695652173914, "test_F_mean_PER": 1.6666666666666667,
              "test_F_mean_overlap": 0.6742424242424242, "test_F_mean_F1": 0.8999947060876787,
              "test_F_mean_p": 0.8333329671718783, "test_F_mean_r": 0.9999995643941295, "test_F_mean_Rval": 0.7866114956903416}
FORCE_VAL = {"val_mean_loss": 0.5, "val_mean_rmse": 1.0354408253557785, "val_mean_pcc": -0.0038642389174654655,
             "val_mean_FER": 0.23913043478260865, "val_mean_PER": 0.2608695652173913, "val_mean_F1": 0.9285660737743526,
             "val_mean_p": 0.8749996164774412, "val_mean_r": 0.9999995643941295, "val_mean_Rval": 0.8577409247530781,
             "val_mean_overlap": 0.7613636363636364}
FORCE_TEST = {"test_N_mean_rmse": 1.0354408253557785, "test_N_mean_pcc": -0.003864238917465466,
              "test_N_std_rmse": 0.057916768389329895, "test_N_std_pcc": 0.14708005178214778,
              "test_N_mean_LA_pcc": 0.060343793811832504, "test_N_mean_LP_pcc": 0.1813192048901287,
              "test_N_mean_JA_pcc": -0.12286342999155847, "test_N_mean_TTCL_pcc": -0.16399902969783825,
              "test_N_mean_TTCD_pcc": 0.2258910942174981, "test_N_mean_TMCL_pcc": -0.2413410704845403,
              "test_N_mean_TMCD_pcc": -0.045950083077478256, "test_N_mean_TBCL_pcc": 0.0702273763347713,
              "test_N_mean_TBCD_pcc": 0.0015939937399954765, "test_N_mean_LA_rmse": 1.055662177404432,
              "test_N_mean_LP_rmse": 1.0990231340627896, "test_N_mean_JA_rmse": 1.0747256757406973,
              "test_N_mean_TTCL_rmse": 1.1034996553907694, "test_N_mean_TTCD_rmse": 0.9291038134856471,
              "test_N_mean_TMCL_rmse": 0.9804162055768193, "test_N_mean_TMCD_rmse": 1.0017541978580793,
              "test_N_mean_TBCL_rmse": 0.9921995520039457, "test_N_mean_TBCD_rmse": 1.0825830166788268,
              "test_N_mean_FER": 0.23913043478260865, "test_N_mean_PER": 0.2608695652173913,
              "test_N_std_PER": 0.010135135135135143, "test_N_mean_overlap": 0.7613636363636364,
              "test_N_std_overlap": 0.011363636363636354, "test_N_mean_F1": 0.9285660737743526,
              "test_N_mean_p": 0.8749996164774412, "test_N_mean_r": 0.9999995643941295, "test_N_mean_Rval": 0.8577409247530781}
PR_VAL = {"mean_val_per": 1.6153846153846154, "mean_val_loss": 0.5}
APTAI_LINES = [
    "\tepoch 1 ~ batch 1/2, train_loss: 0.2500, train_mse_loss: 0.1250, train_ce_loss: 0.0625, lr: 0.312500",
    "\tepoch 1 ~ batch 2/2, train_loss: 0.5000, train_mse_loss: 0.2500, train_ce_loss: 0.1250, lr: 0.312500",
    "Epoch 1/2 -> val_mean_loss: 0.5000 | val_mean_rmse: 1.1580 | val_mean_pcc: -0.0870 | val_mean_FER: 0.3261 | "
    "val_mean_PER: 1.6666 | val_mean_F1: 0.9000 | val_mean_p: 0.8333 | val_mean_r: 1.0000 | val_mean_Rval: 0.7866 | "
    "val_mean_overlap: 0.6742 | mean_train_loss: 0.3750 | lr: 0.6250",
    "\tepoch 2 ~ batch 1/2, train_loss: 0.7500, train_mse_loss: 0.3750, train_ce_loss: 0.1875, lr: 0.625000",
    "\tepoch 2 ~ batch 2/2, train_loss: 1.0000, train_mse_loss: 0.5000, train_ce_loss: 0.2500, lr: 0.625000",
    "Epoch 2/2 -> val_mean_loss: 0.5000 | val_mean_rmse: 1.1580 | val_mean_pcc: -0.0870 | val_mean_FER: 0.3261 | "
    "val_mean_PER: 1.6666 | val_mean_F1: 0.9000 | val_mean_p: 0.8333 | val_mean_r: 1.0000 | val_mean_Rval: 0.7866 | "
    "val_mean_overlap: 0.6742 | mean_train_loss: 0.8750 | lr: 0.9375",
]
FORCE_LINES = [
    "\tepoch 1 ~ batch 1/3, train_loss: 0.2500, train_tv_loss: 0.1250, train_align_loss: 0.0625, lr: 0.312500",
    "\tepoch 1 ~ batch 2/3, train_loss: 0.5000, train_tv_loss: 0.2500, train_align_loss: 0.1250, lr: 0.312500",
    "\tepoch 1 ~ batch 3/3, train_loss: 0.7500, train_tv_loss: 0.3750, train_align_loss: 0.1875, lr: 0.312500",
    "Epoch 1/2 -> val_mean_loss: 0.5000 | val_mean_rmse: 1.0354 | val_mean_pcc: -0.0039 | val_mean_FER: 0.2391 | "
    "val_mean_PER: 0.2609 | val_mean_F1: 0.9286 | val_mean_p: 0.8750 | val_mean_r: 1.0000 | val_mean_Rval: 0.8577 | "
    "val_mean_overlap: 0.7614 | mean_train_loss: 0.5000 | lr: 0.6250",
    "\tepoch 2 ~ batch 1/3, train_loss: 1.0000, train_tv_loss: 0.5000, train_align_loss: 0.2500, lr: 0.625000",
    "\tepoch 2 ~ batch 2/3, train_loss: 1.2500, train_tv_loss: 0.6250, train_align_loss: 0.3125, lr: 0.625000",
    "\tepoch 2 ~ batch 3/3, train_loss: 1.5000, train_tv_loss: 0.7500, train_align_loss: 0.3750, lr: 0.625000",
    "Epoch 2/2 -> val_mean_loss: 0.5000 | val_mean_rmse: 1.0354 | val_mean_pcc: -0.0039 | val_mean_FER: 0.2391 | "
    "val_mean_PER: 0.2609 | val_mean_F1: 0.9286 | val_mean_p: 0.8750 | val_mean_r: 1.0000 | val_mean_Rval: 0.8577 | "
    "val_mean_overlap: 0.7614 | mean_train_loss: 1.2500 | lr: 0.9375",
]
PR_LINES = [
    "\tepoch 1 ~ batch 1/2, train_loss: 0.2500",
    "\tepoch 1 ~ batch 2/2, train_loss: 0.5000",
    "Epoch 1/2 -> lr: 0.625| mean_train_loss: 0.375| mean_val_loss: 0.5| val_per: 1.6153846153846154",
    "\tepoch 2 ~ batch 1/2, train_loss: 0.7500",
    "\tepoch 2 ~ batch 2/2, train_loss: 1.0000",
    "Epoch 2/2 -> lr: 0.9375| mean_train_loss: 0.875| mean_val_loss: 0.5| val_per: 1.6153846153846154",
]
PR_SUBSETS = [[1, 2], [1, 3]]


# ----------------------------------------------------------------------------------------------------------------- train_aptai
def _aptai_loaders(events, n_train=4):
    from aptai_amd import train_aptai as T
    w2v = W2V2Config.base()
    mk = lambda n, seed, bs: torch.utils.data.DataLoader(T.SyntheticHPRC(n, 0.5, seed=seed, cfg=w2v), batch_size=bs,
                                                         collate_fn=hostlogic.collate_aptai)
    return _Loader(mk(n_train, 1, 2), events), _Loader(mk(2, 2, 1), [])


def test_train_aptai_log_history_and_checkpoints(tmp_path, writes):
    from aptai_amd import train_aptai as T
    events, lines = [], []
    model = _TVStub(events)
    cfg, opt, sched = _optim(T, model)
    tr, va = _aptai_loaders(events)
    hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / "best", log=lines.append)
    assert lines == APTAI_LINES
    # lr is the one AFTER lr_scheduler.step(); a tie on the target metric counts as better: saved, and written, in both epochs
    _same(hist[0], dict(APTAI_VAL, epoch=0, mean_train_loss=0.375, lr=0.625, saved=True))
    _same(hist[1], dict(APTAI_VAL, epoch=1, mean_train_loss=0.875, lr=0.9375, saved=True))
    assert len(hist) == 2
    assert writes == ["best/pytorch_model.bin", "best/model_cfg.pkl"] * 2
    assert _files(tmp_path) == {"best/pytorch_model.bin", "best/model_cfg.pkl"}
    assert pickle.load(open(tmp_path / "best" / "model_cfg.pkl", "rb")) == {"stub": True}
    assert set(torch.load(tmp_path / "best" / "pytorch_model.bin", weights_only=True)) == {"w"}
    # no look-ahead: a batch is pulled, then trained on; validation follows the epoch's last step with the epoch number
    S = (2, 8000)
    ev = lambda e: [("pull", 0), ("train", e, S), ("pull", 1), ("train", e, S), ("eval", e, (1, 8000)), ("eval", e, (1, 7381))]
    assert events == ev(0) + ev(1)
    assert float(model.w.detach()) == 1.0 and not model.training


def test_train_aptai_only_a_strictly_worse_epoch_is_not_saved(tmp_path, writes, monkeypatch):
    from aptai_amd import train_aptai as T
    for bigger, want in ((False, [True, True, False, True]), (True, [True, False, True, True])):
        vals = iter([2.0, 1.0, 1.5, 1.0] if not bigger else [1.0, 0.5, 1.0, 1.0])
        monkeypatch.setattr(T, "validate", lambda *a, **k: {"m": next(vals)})
        model = _TVStub([])
        cfg, opt, sched = _optim(T, model, target_metric="m", target_metric_bigger_better=bigger)
        cfg.num_epochs = 4
        tr, va = _aptai_loaders([], n_train=2)
        del writes[:]
        hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / "best", log=lambda s: None)
        assert [h["saved"] for h in hist] == want
        assert len(writes) == 2 * sum(want)
        assert list(hist[0]) == ["m", "epoch", "mean_train_loss", "lr", "saved"]


def test_train_aptai_graphed_runner_life_cycle(tmp_path, runner):
    """Without a front end the runner takes the collate's HOST batch itself; one suspend() per epoch after the last step and
    before validation; one close() at the end; the loop itself never calls the model in training mode."""
    from aptai_amd import train_aptai as T
    events = []
    model = _TVStub(events)
    cfg, opt, sched = _optim(T, model, graphed=True)
    tr, va = _aptai_loaders(events)
    runner.call = lambda m, b: m(0, **b)
    hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / "best", log=lambda s: None)
    assert len(runner.made) == 1 and runner.made[0].model is model and runner.made[0].optimizer is opt
    kinds = [e[0] for e in events]
    epoch = ["pull", "runner.step", "train", "pull", "runner.step", "train", "runner.suspend", "eval", "eval"]
    assert kinds == epoch * 2 + ["runner.close"]
    stepped = [e[1] for e in events if e[0] == "runner.step"]
    assert all(a is b for a, b in zip(stepped, tr.batches * 2))
    assert [h["mean_train_loss"] for h in hist] == [0.375, 0.875]


def test_train_aptai_clip_monitor(tmp_path, clip):
    from aptai_amd import train_aptai as T
    model = _TVStub([])
    cfg, opt, sched = _optim(T, model, max_grad_norm=1.0)
    tr, va = _aptai_loaders([])
    hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / "best", log=lambda s: None)
    assert len(clip.made) == 1 and clip.made[0].optimizer is opt and clip.made[0].per_epoch == [2, 2]
    for h in hist:
        assert list(h) == VAL_KEYS + ["epoch", "mean_train_loss", "lr", "saved", "mean_grad_norm", "clipped_steps"]
        assert h["mean_grad_norm"] == 1.0 and h["clipped_steps"] == 2


def test_train_aptai_validate_and_test_dictionaries():
    from aptai_amd import train_aptai as T
    model = _TVStub([])
    _, va = _aptai_loaders([])
    model.eval()
    _same(T.validate(model, "cpu", None, 3, None, "synthetic", va), APTAI_VAL)
    model.train()
    T.validate(model, "cpu", None, 3, None, "synthetic", va)
    assert model.training                       # validate() leaves the mode alone, test() switches to eval
    res = T.test(model, "cpu", None, None, "synthetic", va, "F", num_epochs=7)
    assert not model.training and [e[1] for e in model.events[-2:]] == [7, 7]
    _same(res, APTAI_TEST)
    assert list(res) == _test_keys("F", False)
    with pytest.raises(AssertionError):
        T.test(model, "cpu", None, None, "synthetic", va, "X")


# ----------------------------------------------------------------------------------------------------------- train_force_aptai
def _force_loaders(events):
    from aptai_amd import train_force_aptai as T
    w2v = W2V2Config.base()
    mk = lambda n, seed, bs: torch.utils.data.DataLoader(T.SyntheticHPRCWithLabels(n, 0.5, seed=seed, cfg=w2v, vocab_size=40),
                                                         batch_size=bs, collate_fn=T.collate)
    return _Loader(mk(6, 1, 2), events), _Loader(mk(2, 2, 1), [])


def test_train_force_aptai_log_history_lookahead_and_checkpoints(tmp_path, writes):
    from aptai_amd import train_force_aptai as T
    events, lines = [], []
    model = _ForceStub(events)
    cfg, opt, sched = _optim(T, model)
    tr, va = _force_loaders(events)
    hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / "best", log=lines.append)
    assert lines == FORCE_LINES
    _same(hist[0], dict(FORCE_VAL, epoch=0, mean_train_loss=0.5, lr=0.625, saved=True))
    _same(hist[1], dict(FORCE_VAL, epoch=1, mean_train_loss=1.25, lr=0.9375, saved=True))
    assert len(hist) == 2
    assert writes == ["best/pytorch_model.bin", "best/model_cfg.pkl"] * 2
    assert _files(tmp_path) == {"best/pytorch_model.bin", "best/model_cfg.pkl"}
    # one batch of look-ahead: batch i + 1 is pulled (collated) before step i runs; `_prefetch_next=None` is passed on the CPU
    S = (2, 8000)
    ev = lambda e: [("pull", 0), ("pull", 1), ("train", e, S, None), ("pull", 2), ("train", e, S, None), ("train", e, S, None),
                    ("eval", e, (1, 8000), "absent"), ("eval", e, (1, 7381), "absent")]
    assert events == ev(0) + ev(1)


def test_train_force_aptai_clip_monitor_and_no_graphed_branch(tmp_path, clip, runner):
    from aptai_amd import train_force_aptai as T
    model = _ForceStub([])
    cfg, opt, sched = _optim(T, model, max_grad_norm=1.0, graphed=True)
    tr, va = _force_loaders([])
    hist = T.train(cfg, model, opt, sched, tr, va, "synthetic", tmp_path / "best", log=lambda s: None)
    assert runner.made == []
    assert len(clip.made) == 1 and clip.made[0].per_epoch == [3, 3]
    assert list(hist[1]) == VAL_KEYS + ["epoch", "mean_train_loss", "lr", "saved", "mean_grad_norm", "clipped_steps"]


def test_train_force_aptai_validate_and_test_dictionaries():
    from aptai_amd import train_force_aptai as T
    model = _ForceStub([])
    _, va = _force_loaders([])
    model.eval()
    _same(T.validate(model, "cpu", None, 3, None, "synthetic", va), FORCE_VAL)
    model.train()
    T.validate(model, "cpu", None, 3, None, "synthetic", va)
    assert model.training
    res = T.test(model, "cpu", None, None, "synthetic", va, "N", num_epochs=7)
    assert not model.training and [e[1] for e in model.events[-2:]] == [7, 7]
    _same(res, FORCE_TEST)
    assert list(res) == _test_keys("N", True)


# ---------------------------------------------------------------------------------------------------- train_phoneme_recognizer
def _pr_loaders(events, extra_len=0):
    from aptai_amd import train_phoneme_recognizer as T
    mk = lambda n, seed, bs: torch.utils.data.DataLoader(T.SyntheticCommonPhone(n, 0.5, 40, seed=seed), batch_size=bs,
                                                         collate_fn=hostlogic.collate_pr)
    return _Loader(mk(8, 1, 2), events, extra_len), _Loader(mk(2, 2, 1), [])


def _pr_train(tmp_path, model, tr, va, lines, **kw):
    from aptai_amd import train_phoneme_recognizer as T
    cfg, opt, sched = _optim(T, model, samples_per_epoch=4, **kw)
    random.seed(3)
    hist = T.train(cfg, model, opt, sched, T.default_vocab(), tr, va, tmp_path / "best", tmp_path / "last", tmp_path / "all",
                   log=lines.append)
    return cfg, opt, hist


def test_train_phoneme_recognizer_log_history_subset_and_checkpoints(tmp_path, writes, monkeypatch):
    from aptai_amd import ops
    monkeypatch.setattr(ops, "ctc_greedy_decode", _fake_decode)
    events, lines = [], []
    model = _PRStub(events)
    tr, va = _pr_loaders(events)
    cfg, opt, hist = _pr_train(tmp_path, model, tr, va, lines, save_all_epochs=True)
    assert lines == PR_LINES
    _same(hist[0], dict(PR_VAL, epoch=0, mean_train_loss=0.375, lr=0.625, saved=True, trained_batches=2))
    _same(hist[1], dict(PR_VAL, epoch=1, mean_train_loss=0.875, lr=0.9375, saved=True, trained_batches=2))
    assert len(hist) == 2
    # the epoch's subset is drawn once from `random`, before the loader is iterated; skipped batches are still pulled
    random.seed(3)
    subsets = [sorted(random.sample(range(4), 2)) for _ in range(2)]
    assert subsets == PR_SUBSETS
    want = []
    for e, sub in enumerate(subsets):
        for i in range(4):
            want.append(("pull", i))
            if i in sub:
                want.append(("train", tuple(tr.batches[i]["input_values"].shape)))
        want += [("eval", (1, 8000)), ("eval", (1, 7381))]
    assert events == want
    # best (a tie saves again), every epoch with its configuration written once, last with optimiser and scheduler state
    last = ["last/optimizer.pt", "last/scheduler.pt", "last/pytorch_model.bin", "last/model_cfg.pkl"]
    assert writes == (["best/pytorch_model.bin", "best/model_cfg.pkl", "all/e0000.bin", "all/model_cfg.pkl"] + last
                      + ["best/pytorch_model.bin", "best/model_cfg.pkl", "all/e0001.bin"] + last)
    assert _files(tmp_path) == set(writes)
    assert torch.load(tmp_path / "last" / "scheduler.pt", weights_only=True) == {"last_epoch": 2}
    assert set(torch.load(tmp_path / "last" / "optimizer.pt", weights_only=True)) == {"state", "param_groups"}


def test_train_phoneme_recognizer_without_save_all_epochs(tmp_path, writes, monkeypatch):
    from aptai_amd import ops
    monkeypatch.setattr(ops, "ctc_greedy_decode", _fake_decode)
    tr, va = _pr_loaders([])
    _pr_train(tmp_path, _PRStub([]), tr, va, [])
    assert _files(tmp_path) == {"best/pytorch_model.bin", "best/model_cfg.pkl", "last/optimizer.pt", "last/scheduler.pt",
                                "last/pytorch_model.bin", "last/model_cfg.pkl"}
    assert not (tmp_path / "all").exists()


def test_train_phoneme_recognizer_mean_train_loss_divides_by_the_planned_steps(tmp_path, monkeypatch):
    """A loader that reports one batch more than it yields: an index drawn past the end trains nothing, and the mean still
    divides by samples_per_epoch / batch_size."""
    from aptai_amd import ops
    monkeypatch.setattr(ops, "ctc_greedy_decode", _fake_decode)
    monkeypatch.setattr(random, "sample", lambda population, k: [1, 4][:k])
    tr, va = _pr_loaders([], extra_len=1)
    lines = []
    _, _, hist = _pr_train(tmp_path, _PRStub([]), tr, va, lines)
    assert [h["trained_batches"] for h in hist] == [1, 1]
    assert [h["mean_train_loss"] for h in hist] == [0.125, 0.25]          # (1/4) / 2, (2/4) / 2
    assert lines[0] == "\tepoch 1 ~ batch 1/2, train_loss: 0.2500"


def test_train_phoneme_recognizer_graphed_runner_and_clip_monitor(tmp_path, runner, clip, monkeypatch):
    """The runner always takes the uploaded batch (a new dictionary with the collate's entries), never the collate's own."""
    from aptai_amd import ops
    monkeypatch.setattr(ops, "ctc_greedy_decode", _fake_decode)
    events = []
    model = _PRStub(events)
    tr, va = _pr_loaders(events)
    runner.call = lambda m, b: m(**b)
    _, opt, hist = _pr_train(tmp_path, model, tr, va, [], graphed=True, max_grad_norm=1.0)
    assert len(runner.made) == 1 and runner.made[0].model is model and runner.made[0].optimizer is opt
    kinds = [e[0] for e in events if e[0] != "pull"]
    assert kinds == ["runner.step", "train", "runner.step", "train", "runner.suspend", "eval", "eval"] * 2 + ["runner.close"]
    stepped = [e[1] for e in events if e[0] == "runner.step"]
    trained = [tr.batches[i] for sub in PR_SUBSETS for i in sub]
    for got, host in zip(stepped, trained):
        assert got is not host and list(got) == list(host) and all(torch.equal(got[k], host[k]) for k in host)
    assert clip.made[0].per_epoch == [2, 2]
    assert list(hist[0]) == ["mean_val_per", "mean_val_loss", "epoch", "mean_train_loss", "lr", "saved", "trained_batches",
                             "mean_grad_norm", "clipped_steps"]


def test_train_phoneme_recognizer_validate_and_test_dictionaries(monkeypatch):
    from aptai_amd import ops, train_phoneme_recognizer as T
    monkeypatch.setattr(ops, "ctc_greedy_decode", _fake_decode)
    model = _PRStub([])
    _, va = _pr_loaders([])
    model.eval()
    _same(T.validate(model, "cpu", None, 0, va), PR_VAL)
    model.train()
    T.validate(model, "cpu", None, 0, va)
    assert model.training
    _same(T.test(model, "cpu", None, va, "synthetic"), {"mean_test_per": PR_VAL["mean_val_per"]})
    assert not model.training
    n = len(model.events)
    one = T.test(model, "cpu", None, va, "synthetic", laptop=True)          # the first utterance only
    assert len(model.events) == n + 1 and list(one) == ["mean_test_per"]
