"""CPU: the host side of the device evaluation metrics (aptai_amd.device_metrics, csrc/eval.hip): every new entry point is declared,
exported and typed; CPU tensors are refused (no fallback); EvalAccumulator.result() forms the loops' final dictionaries from
per-utterance values exactly as validate() / test() of the three training loops form them."""
import numpy as np
import pytest
import torch

from aptai_amd import metrics

NEW = ("aptai_eval_tv_scores", "aptai_eval_frame_scores", "aptai_eval_boundary_counts", "aptai_eval_collapse_runs",
       "aptai_eval_edit_distance")
TVN = metrics.TV_NAMES


def test_new_entry_points_are_declared_exported_and_typed():
    from aptai_amd import _lib, ops
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in NEW:
        assert n in names and n in _lib.ARGTYPES and hasattr(L, n), n
        assert getattr(L, n).argtypes == _lib.ARGTYPES[n]
    for w in ("eval_tv_scores", "eval_frame_scores", "eval_boundary_counts", "eval_collapse_runs", "eval_edit_distance"):
        assert callable(getattr(ops, w))


def test_cpu_tensors_are_refused():
    from aptai_amd import device_metrics as dm
    from aptai_amd._lib import AptaiHipError
    x, lab = torch.zeros(2, 8, 9), torch.zeros(2, 8, dtype=torch.int64)
    n = torch.full((2,), 8, dtype=torch.int32)
    with pytest.raises(AptaiHipError):
        dm.tv_scores(x, x, n)
    with pytest.raises(AptaiHipError):
        dm.frame_scores(lab, lab, n)
    with pytest.raises(AptaiHipError):
        dm.boundary_counts(lab.double(), n, lab.double(), n)
    with pytest.raises(AptaiHipError):
        dm.collapse_runs(lab, n)
    with pytest.raises(AptaiHipError):
        dm.edit_distance(lab.int(), n, lab.int(), n)
    acc = dm.EvalAccumulator("val")
    with pytest.raises(AptaiHipError):
        acc.add_tv(x, x, n)
    with pytest.raises(AptaiHipError):
        acc.add_frames(lab, lab, n)
    with pytest.raises(AptaiHipError):
        acc.add_edit(lab.int(), n, lab.int(), n)


def _utterances(n, seed):
    """Per-utterance values as the host loops hold them after their metric calls."""
    g = np.random.RandomState(seed)
    utts = []
    for _ in range(n):
        T = int(g.randint(20, 60))
        gt, pred = g.randint(1, 6, size=T), g.randint(1, 6, size=T)
        y_grp, h_grp = metrics.phn_frame_id2phn(gt.tolist()), metrics.phn_frame_id2phn(pred.tolist())
        d = np.abs(gt[:, None].astype(np.float64) - pred[None, :].astype(np.float64))
        lab, dec = g.randint(1, 40, size=int(g.randint(5, 30))), g.randint(1, 40, size=int(g.randint(0, 30)))
        utts.append(dict(loss=float(np.float32(g.rand() * 3)), rmse=g.rand(9), pcc=g.rand(9) * 2 - 1, frames=T,
                         correct=int((gt == pred).sum()), prec=int((d.min(axis=0) <= 0.02).sum()), rec=int((d.min(axis=1) <= 0.02).sum()),
                         gt=gt, pred=pred, grp_n=len(y_grp), grp_dist=metrics.edit_distance(y_grp, h_grp),
                         edit_n=len(lab), edit_dist=metrics.edit_distance(lab.tolist(), dec.tolist())))
    return utts


def _fill(acc, utts, batch=2):
    """Push the values batch by batch, as the add_* methods do with their kernels' outputs."""
    for i in range(0, len(utts), batch):
        chunk = utts[i:i + batch]
        acc.add_loss(torch.tensor(chunk[0]["loss"], dtype=torch.float32))
        for u in chunk[1:]:
            acc.add_loss(torch.tensor(u["loss"], dtype=torch.float32))
        acc.push("rmse", torch.tensor(np.stack([u["rmse"] for u in chunk])))
        acc.push("pcc", torch.tensor(np.stack([u["pcc"] for u in chunk])))
        for k in ("frames", "correct", "prec", "rec", "grp_n", "grp_dist", "edit_n", "edit_dist"):
            acc.push(k, torch.tensor([u[k] for u in chunk], dtype=torch.int32))


def _host_val(utts, per):
    """validate() of train_aptai.py (per='frames_rounded') / train_force_aptai.py (per='edit'), from the same values."""
    val_losses = [u["loss"] for u in utts]
    val_rmses = [np.mean(list(dict(zip(TVN, u["rmse"].tolist())).values())) for u in utts]
    val_pccs = [np.mean([v for v in u["pcc"].tolist()]) for u in utts]
    stats = [metrics.get_stats(u["gt"], u["pred"], tolerance=0.02) for u in utts]
    overlaps = [metrics.evaluate_overlap(u["gt"][None], u["pred"][None]) for u in utts]
    if per == "frames_rounded":
        edit_d = [metrics.compute_PER(metrics.phn_frame_id2phn(u["gt"].tolist()), metrics.phn_frame_id2phn(u["pred"].tolist())) / 100.0
                  * u["grp_n"] for u in utts]
        n_phn = [u["grp_n"] for u in utts]
    else:
        edit_d, n_phn = [u["edit_dist"] for u in utts], [u["edit_n"] for u in utts]
    total, corr = sum(u["frames"] for u in utts), sum(u["correct"] for u in utts)
    return {
        "val_mean_loss": float(np.mean(val_losses)), "val_mean_rmse": float(np.mean(val_rmses)),
        "val_mean_pcc": float(np.mean(val_pccs)), "val_mean_FER": 1 - (corr / total),
        "val_mean_PER": float(np.sum(edit_d) / np.sum(n_phn)), "val_mean_F1": float(np.mean([s[2] for s in stats])),
        "val_mean_p": float(np.mean([s[0] for s in stats])), "val_mean_r": float(np.mean([s[1] for s in stats])),
        "val_mean_Rval": float(np.mean([s[3] for s in stats])), "val_mean_overlap": float(np.mean(overlaps)),
    }


def _host_test(utts, rate, force):
    """test() of train_aptai.py (force=False) / train_force_aptai.py (force=True), from the same values."""
    from aptai_amd.train_aptai import _tv_test_summary
    rmse_tvs = {n: [u["rmse"][i] for u in utts] for i, n in enumerate(TVN)}
    pcc_tvs = {n: [u["pcc"][i] for u in utts] for i, n in enumerate(TVN)}
    stats = [metrics.get_stats(u["gt"], u["pred"], tolerance=0.02) for u in utts]
    overlaps = [metrics.evaluate_overlap(u["gt"][None], u["pred"][None]) for u in utts]
    key = ("edit_dist", "edit_n") if force else ("grp_dist", "grp_n")
    edit_d, n_phn = [u[key[0]] for u in utts], [u[key[1]] for u in utts]
    total, corr = sum(u["frames"] for u in utts), sum(u["correct"] for u in utts)
    out = _tv_test_summary(rate, rmse_tvs, pcc_tvs, with_std=force)
    out.update({f"test_{rate}_mean_FER": 1 - (corr / total), f"test_{rate}_mean_PER": float(np.sum(edit_d) / np.sum(n_phn)),
                f"test_{rate}_mean_overlap": float(np.mean(overlaps)), f"test_{rate}_mean_F1": float(np.mean([s[2] for s in stats])),
                f"test_{rate}_mean_p": float(np.mean([s[0] for s in stats])), f"test_{rate}_mean_r": float(np.mean([s[1] for s in stats])),
                f"test_{rate}_mean_Rval": float(np.mean([s[3] for s in stats]))})
    if force:
        out[f"test_{rate}_std_PER"] = float(np.std([d / n for d, n in zip(edit_d, n_phn)]))
        out[f"test_{rate}_std_overlap"] = float(np.std(overlaps))
    return out


@pytest.mark.parametrize("per", ["frames_rounded", "edit"])
def test_accumulator_reproduces_validate(per):
    from aptai_amd.device_metrics import EvalAccumulator
    utts = _utterances(7, 3)
    acc = EvalAccumulator("val", per=per)
    _fill(acc, utts)
    assert acc.result() == _host_val(utts, per)                          # same operations in the same order: equal, key for key


@pytest.mark.parametrize("force", [False, True])
def test_accumulator_reproduces_test(force):
    from aptai_amd.device_metrics import EvalAccumulator
    utts = _utterances(5, 11)
    acc = EvalAccumulator("test", rate="N", per="edit" if force else "frames", with_std=force)
    _fill(acc, utts, batch=3)
    assert acc.result() == _host_test(utts, "N", force)


def test_accumulator_phoneme_recognizer_keys_and_checks():
    from aptai_amd.device_metrics import EvalAccumulator
    utts = _utterances(4, 5)
    want_per = float(np.sum([u["edit_dist"] for u in utts]) / np.sum([u["edit_n"] for u in utts]))
    for kind in ("pr_val", "pr_test"):
        acc = EvalAccumulator(kind)
        for u in utts:
            acc.add_loss(torch.tensor(u["loss"], dtype=torch.float32))
            acc.push("edit_dist", torch.tensor([u["edit_dist"]], dtype=torch.int32))
            acc.push("edit_n", torch.tensor([u["edit_n"]], dtype=torch.int32))
        res = acc.result()
        if kind == "pr_val":
            assert res == {"mean_val_per": want_per, "mean_val_loss": float(np.mean([u["loss"] for u in utts]))}
        else:
            assert res == {"mean_test_per": want_per}
    # the decoded-length check of Force_APTAI._lists, made once at the end
    acc = EvalAccumulator("pr_test", max_phonemes=60)
    acc.push("edit_dist", torch.tensor([1], dtype=torch.int32)); acc.push("edit_n", torch.tensor([2], dtype=torch.int32))
    acc.add_decoded_lengths(torch.tensor([12, 60], dtype=torch.int32))
    with pytest.raises(AssertionError, match="longer max phoneme"):
        acc.result()
    with pytest.raises(ValueError):
        EvalAccumulator("test")                                          # a rate is part of the test keys
