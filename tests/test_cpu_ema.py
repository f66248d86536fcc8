"""CPU: the host-side contract of the exponential moving average of the weights (aptai_amd.optim.Adam(ema_decay=...)): the
constructor's and setter's checks, the two C-ABI entries being declared, their argument refusals (which need no device), the
decay rule as a value table, the flags' way into the optimiser, and where loops.EpochDriver opens and closes the averaged-weights
scope (a recording stub stands for the optimiser)."""
import contextlib
from types import SimpleNamespace

import pytest
import torch


def _cpu_param(n=8):
    p = torch.nn.Parameter(torch.randn(n))
    p.grad = torch.randn(n)
    return p


def test_constructor_and_setter_check_ema_decay():
    from aptai_amd.optim import Adam
    for bad in (-0.1, 1.0, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError):
            Adam([_cpu_param()], ema_decay=bad)
    p = _cpu_param()
    opt = Adam([p])
    assert opt.ema_decay is None and opt.ema_warmup is False and opt.ema_updates == 0 and opt.ema_parameter(p) is None
    for bad in (-0.1, 1.0, 1.5, float("nan"), "x"):
        with pytest.raises(ValueError):
            opt.ema_decay = bad
    assert opt.ema_decay is None
    opt.ema_decay = 0.999                               # reassignable between steps
    assert opt.ema_decay == 0.999
    opt.ema_decay = 0                                   # 0 is a decay: the average IS the last iterate
    assert opt.ema_decay == 0.0
    opt.ema_decay = None
    opt = Adam([p], ema_decay=0.9, ema_warmup=True)
    assert opt.ema_decay == 0.9 and opt.ema_warmup is True
    assert opt.ema_parameter(p) is None                 # not on the device path: no average
    assert "ema_decay" not in opt.param_groups[0] and "ema_warmup" not in opt.param_groups[0]
    sd = opt.state_dict()
    assert "ema_decay" not in sd["param_groups"][0] and set(sd) == {"state", "param_groups"}
    esd = opt.ema_state_dict()
    assert set(esd) == {"decay", "warmup", "updates", "ema"} and esd["decay"] == 0.9 and esd["warmup"] is True
    assert esd["updates"] == 0 and esd["ema"] == [None]


def test_ema_weights_needs_averages():
    from aptai_amd.optim import Adam
    opt = Adam([_cpu_param()])
    with pytest.raises(RuntimeError, match="ema_decay"):
        opt.swap_ema()
    with pytest.raises(RuntimeError, match="ema_decay"):
        with opt.ema_weights():
            pass


def test_the_entries_are_declared():
    from aptai_amd import _lib
    declared = _lib.declared_symbols()
    for name, nargs in (("aptai_ema_multi", 6), ("aptai_swap_multi", 5)):
        assert name in declared and name in _lib.ARGTYPES and len(_lib.ARGTYPES[name]) == nargs


def test_bad_arguments_are_refused_before_any_launch():
    from aptai_amd import _lib
    for name, tail in (("aptai_ema_multi", (0.5, None)), ("aptai_swap_multi", (None,))):
        bad = f"{name}: bad arguments"
        for table, ema in ((None, 16), (16, None)):
            with pytest.raises(_lib.AptaiHipError, match=bad):
                _lib.call(name, table, ema, 1, 1, *tail)
        for njobs in (0, -1, 65536, 70000):
            with pytest.raises(_lib.AptaiHipError, match=bad):
                _lib.call(name, 16, 16, njobs, 1, *tail)
        for max_n in (0, -4):
            with pytest.raises(_lib.AptaiHipError, match=bad):
                _lib.call(name, 16, 16, 1, max_n, *tail)
    for weight in (float("nan"), 0.0, -0.5, 1.5, float("inf")):
        with pytest.raises(_lib.AptaiHipError, match="aptai_ema_multi: weight"):
            _lib.call("aptai_ema_multi", 16, 16, 1, 1, weight, None)


def test_decay_rule_value_table():
    from aptai_amd.optim import ema_decay_at
    for k in (1, 2, 10, 1000, 10 ** 6):
        assert ema_decay_at(k, 0.999, False) == 0.999 and ema_decay_at(k, 0.0, False) == 0.0
    # warm-up: (1 + k) / (10 + k) = 2/11, 3/12, 4/13, ... until it crosses the decay
    assert [ema_decay_at(k, 0.999, True) for k in (1, 2, 3, 4)] == [2 / 11, 3 / 12, 4 / 13, 5 / 14]
    assert ema_decay_at(80, 0.9, True) == 81 / 90 == 0.9 and ema_decay_at(79, 0.9, True) == 80 / 89 < 0.9
    assert ema_decay_at(81, 0.9, True) == 0.9 and ema_decay_at(10 ** 6, 0.9, True) == 0.9
    assert ema_decay_at(8989, 0.999, True) == 8990 / 8999 < 0.999 and ema_decay_at(8992, 0.999, True) == 0.999
    assert ema_decay_at(1, 0.1, True) == 0.1            # a decay below 2/11 is never raised
    seq = [ema_decay_at(k, 0.999, True) for k in range(1, 10000)]
    assert all(a <= b for a, b in zip(seq, seq[1:])) and seq[-1] == 0.999


def test_the_flags_reach_the_optimiser():
    import argparse
    from aptai_amd import loops
    ap = argparse.ArgumentParser()
    loops.add_shared_arguments(ap)
    off = loops.shared_arguments(ap.parse_args([]))
    assert off["ema_decay"] is None and off["ema_warmup"] is False
    on = loops.shared_arguments(ap.parse_args(["--ema_decay", "0.99", "--ema_warmup"]))
    assert on["ema_decay"] == 0.99 and on["ema_warmup"] is True
    cfg = loops.default_cfg(dict(learning_rate=1e-3))
    assert cfg.ema_decay is None and cfg.ema_warmup is False
    opt, _ = loops.adam_and_schedule([_cpu_param()], cfg)
    assert opt.ema_decay is None and opt.ema_warmup is False
    opt, _ = loops.adam_and_schedule([_cpu_param()], loops.default_cfg(dict(learning_rate=1e-3, **on)))
    assert opt.ema_decay == 0.99 and opt.ema_warmup is True
    with pytest.raises(ValueError):
        loops.adam_and_schedule([_cpu_param()], loops.default_cfg(dict(learning_rate=1e-3, ema_decay=1.0)))
    from aptai_amd import train_aptai, train_force_aptai, train_phoneme_recognizer
    for mod in (train_aptai, train_force_aptai, train_phoneme_recognizer):
        assert mod.default_cfg().ema_decay is None and mod.default_cfg(ema_decay=0.5).ema_decay == 0.5


# ------------------------------------------------------------------------------------------------------------------ EpochDriver
class _Plain:
    """An optimiser without the new members, as torch's."""

    def __init__(self, events):
        self.events = events
        self.param_groups = [dict(lr=0.5)]

    def zero_grad(self):
        pass

    def step(self):
        self.events.append("step")


class _Averaging(_Plain):
    """In the place of aptai_amd.optim.Adam(ema_decay=...): records where the averaged-weights scope opens and closes."""
    ema_updates = 7

    @contextlib.contextmanager
    def ema_weights(self, model=None):
        self.events.append(("enter", model))
        try:
            yield self
        finally:
            self.events.append("exit")


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(()))

    def get_config(self):
        return {}


def _epoch(tmp_path, monkeypatch, opt_cls, validate=None, **cfg):
    from aptai_amd import loops
    events = []
    opt = opt_cls(events)
    monkeypatch.setattr(loops, "save_checkpoint", lambda model, path: events.append("best"))
    cfg = SimpleNamespace(target_metric="loss", target_metric_bigger_better=False, **cfg)
    sched = SimpleNamespace(step=lambda: events.append("sched"))
    model = _Model()
    drv = loops.EpochDriver(cfg, model, opt, sched, tmp_path / "best")
    drv.eager_step(lambda: {"loss": model.w * 0.0 + 1.0})

    def val():
        events.append("validate")
        return {"loss": 0.5}
    log = drv.end_epoch(0, validate or val, extra_checkpoints=lambda: events.append("extra"))
    return events, log, model


TODAY = ["step", "sched", "validate", "best", "extra"]


def test_epoch_driver_validates_and_saves_the_best_checkpoint_inside_the_scope(tmp_path, monkeypatch):
    events, log, model = _epoch(tmp_path, monkeypatch, _Averaging, ema_decay=0.5)
    assert events == ["step", "sched", ("enter", model), "validate", "best", "exit", "extra"]
    assert log["ema_updates"] == 7 and log["saved"] is True


def test_epoch_driver_leaves_the_scope_when_validation_raises(tmp_path, monkeypatch):
    from aptai_amd import loops
    events = []

    def boom():
        events.append("validate")
        raise KeyError("boom")
    opt = _Averaging(events)
    drv = loops.EpochDriver(SimpleNamespace(target_metric="loss", target_metric_bigger_better=False, ema_decay=0.5), _Model(), opt,
                            SimpleNamespace(step=lambda: None), tmp_path / "best")
    with pytest.raises(KeyError):
        drv.end_epoch(0, boom, extra_checkpoints=lambda: events.append("extra"))
    assert [e if isinstance(e, str) else e[0] for e in events] == ["enter", "validate", "exit"]


def test_epoch_driver_without_ema_does_what_it_did(tmp_path, monkeypatch):
    for opt_cls, cfg in ((_Plain, dict(ema_decay=0.5)),           # a stub (or torch's optimiser) without the members
                         (_Averaging, dict()),                    # a cfg without the entry
                         (_Averaging, dict(ema_decay=None))):     # the default
        events, log, _ = _epoch(tmp_path, monkeypatch, opt_cls, **cfg)
        assert events == TODAY, (opt_cls, cfg, events)
        assert "ema_updates" not in log
