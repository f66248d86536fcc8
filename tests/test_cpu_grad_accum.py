"""CPU: the host-side contract of gradient accumulation (aptai_amd.optim.Adam(gradient_accumulation_steps=N)): the constructor's
checks, the C-ABI entry being declared (tests/test_cpu_host.py then checks every declared symbol against the built library), its
argument refusals, which need no device, and what loops.EpochDriver does with an accumulating optimiser (a stub stands for it)."""
from types import SimpleNamespace

import pytest
import torch


def _cpu_param(n=8):
    p = torch.nn.Parameter(torch.randn(n))
    p.grad = torch.randn(n)
    return p


def test_constructor_checks_gradient_accumulation_steps():
    from aptai_amd.optim import Adam
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            Adam([_cpu_param()], gradient_accumulation_steps=bad)
    opt = Adam([_cpu_param()])
    assert opt.gradient_accumulation_steps == 1 and opt.micro_step == 0 and opt.last_step_updated is False
    assert opt.accumulated_grad(opt.param_groups[0]["params"][0]) is None
    opt = Adam([_cpu_param()], gradient_accumulation_steps=4)
    assert opt.gradient_accumulation_steps == 4
    opt.gradient_accumulation_steps = 2                 # no window is open: reassignable
    assert opt.gradient_accumulation_steps == 2
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            opt.gradient_accumulation_steps = bad
    assert opt.gradient_accumulation_steps == 2
    assert "gradient_accumulation_steps" not in opt.param_groups[0]
    assert "gradient_accumulation_steps" not in opt.state_dict()["param_groups"][0]
    assert opt.flush() is False                         # nothing open: nothing to launch, no device needed


def test_the_entry_is_declared():
    from aptai_amd import _lib
    assert "aptai_grad_accum_multi" in _lib.declared_symbols() and "aptai_grad_accum_multi" in _lib.ARGTYPES
    assert len(_lib.ARGTYPES["aptai_grad_accum_multi"]) == 7


def test_bad_arguments_are_refused_before_any_launch():
    from aptai_amd import _lib
    for table, dyn, acc in ((None, 16, 16), (16, None, 16), (16, 16, None)):
        with pytest.raises(_lib.AptaiHipError, match="aptai_grad_accum_multi: bad arguments"):
            _lib.call("aptai_grad_accum_multi", table, dyn, acc, 1, 1, 1.0, None)
    for njobs in (0, 70000):
        with pytest.raises(_lib.AptaiHipError, match="aptai_grad_accum_multi: bad arguments"):
            _lib.call("aptai_grad_accum_multi", 16, 16, 16, njobs, 1, 1.0, None)
    with pytest.raises(_lib.AptaiHipError, match="aptai_grad_accum_multi: bad arguments"):
        _lib.call("aptai_grad_accum_multi", 16, 16, 16, 1, 0, 1.0, None)
    for scale in (float("nan"), 0.0, -0.5, float("inf")):
        with pytest.raises(_lib.AptaiHipError, match="aptai_grad_accum_multi: scale"):
            _lib.call("aptai_grad_accum_multi", 16, 16, 16, 1, 1, scale, None)


# ------------------------------------------------------------------------------------------------------------------ EpochDriver
class _Opt:
    """In the place of an accumulating aptai_amd.optim.Adam: windows of `n` step() calls."""

    def __init__(self, n=None):
        self.n, self.calls, self.flushes = n, 0, 0
        self.param_groups = [dict(lr=0.5)]
        self.max_grad_norm = 1.0
        if n is not None:
            self.micro_step, self.last_step_updated = 0, False

    def zero_grad(self):
        pass

    def step(self):
        self.calls += 1
        if self.n is not None:
            self.micro_step = (self.micro_step + 1) % self.n
            self.last_step_updated = self.micro_step == 0

    def flush(self):
        self.flushes += 1
        self.micro_step, self.last_step_updated = 0, True
        return True


class _Clip:
    def __init__(self, optimizer):
        self.seen = []
        self.optimizer = optimizer

    def update(self):
        self.seen.append(self.optimizer.calls)

    def epoch_log(self):
        return dict(mean_grad_norm=1.0, clipped_steps=len(self.seen))


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))

    def get_config(self):
        return {}


def _driver(tmp_path, monkeypatch, opt, **cfg):
    from aptai_amd import loops, optim
    monkeypatch.setattr(optim, "ClipMonitor", _Clip)
    cfg = SimpleNamespace(target_metric="loss", target_metric_bigger_better=False, max_grad_norm=1.0, **cfg)
    sched = SimpleNamespace(steps=[], step=lambda: sched.steps.append((opt.calls, opt.flushes)))
    model = _Model()
    drv = loops.EpochDriver(cfg, model, opt, sched, tmp_path / "best")
    return drv, model, sched


def _train(drv, model, n):
    for _ in range(n):
        drv.eager_step(lambda: {"loss": model.w * 0.0 + 1.0})


def test_epoch_driver_keeps_the_clip_monitor_to_update_steps_and_flushes_the_remainder(tmp_path, monkeypatch):
    opt = _Opt(2)
    drv, model, sched = _driver(tmp_path, monkeypatch, opt, gradient_accumulation_steps=2)
    _train(drv, model, 5)                               # updates behind calls 2 and 4; call 5 leaves a window open
    assert drv.clip.seen == [2, 4] and opt.flushes == 0
    log = drv.end_epoch(0, lambda: {"loss": 0.5})
    assert opt.flushes == 1 and sched.steps == [(5, 1)]                 # flushed once, before the schedule step
    assert drv.clip.seen == [2, 4, 5]
    assert log["optimizer_updates"] == 3 and log["clipped_steps"] == 3
    _train(drv, model, 4)                               # no window open at the end of this epoch: nothing to flush
    log = drv.end_epoch(1, lambda: {"loss": 0.5})
    assert opt.flushes == 1 and log["optimizer_updates"] == 2


def test_epoch_driver_at_the_default_logs_no_updates_and_never_flushes(tmp_path, monkeypatch):
    opt = _Opt()                                        # an optimiser without the new members, as torch's
    drv, model, sched = _driver(tmp_path, monkeypatch, opt)
    _train(drv, model, 3)
    log = drv.end_epoch(0, lambda: {"loss": 0.5})
    assert drv.clip.seen == [1, 2, 3] and opt.flushes == 0
    assert "optimizer_updates" not in log


def test_the_flag_reaches_the_optimiser():
    import argparse
    from aptai_amd import loops
    ap = argparse.ArgumentParser()
    loops.add_shared_arguments(ap)
    assert loops.shared_arguments(ap.parse_args([]))["gradient_accumulation_steps"] == 1
    assert loops.shared_arguments(ap.parse_args(["--gradient_accumulation_steps", "4"]))["gradient_accumulation_steps"] == 4
    cfg = loops.default_cfg(dict(gradient_accumulation_steps=3, learning_rate=1e-3))
    opt, _ = loops.adam_and_schedule([_cpu_param()], cfg)
    assert opt.gradient_accumulation_steps == 3
    opt, _ = loops.adam_and_schedule([_cpu_param()], loops.default_cfg(dict(learning_rate=1e-3)))
    assert opt.gradient_accumulation_steps == 1
