"""GPU: ONE aptai_amd.optim.Adam object driven through every mode in turn - plain, early launches, clipping, an accumulation window
with clipping, a window with averaging, early launches again - over the one job table and ring the modes share; and the guard of
launch_early() against a row span that would update another early parameter.  The shapes, the two-group split and the bit-for-bit
contract are those of tests/test_gpu_grad_accum.py."""
import pytest
import torch

from test_gpu_ema import _lerp, _w32
from test_gpu_grad_accum import NEVER, _assert_same_optimiser_state, _assign, _grads, _groups, _mean, _params

pytestmark = pytest.mark.gpu


def _early_step(A, a, gen, calls):
    """One step in pieces with the first two parameters (of group 0) launched early; `calls` then holds this step's launches."""
    grads = _grads(a, gen)
    _assign(a, grads)
    del calls[:]
    A.prepare(early=a[:2])
    A.launch_early(a[:2])
    A.finish()
    return grads


def drive_through_every_mode(A, a, gen, calls):
    """Steps (a) - (f) on optimiser A.  After each UPDATE yields (step, the effective gradient of every parameter, whether A clipped
    it at 1.0).  `calls`: the list a wrapped _lib.call appends to."""
    grads = _grads(a, gen, absent=(1,))                                  # (a) plain, one parameter absent
    _assign(a, grads)
    A.step()
    yield "a", grads, False
    yield "b", _early_step(A, a, gen, calls), False                      # (b) early launches
    A.max_grad_norm = 1.0                                                 # (c) clipping
    grads = _grads(a, gen)
    _assign(a, grads)
    A.step()
    assert float(A.last_clip_coef) < 1
    yield "c", grads, True
    A.gradient_accumulation_steps = 2                                     # (d) a window, clipping still on, a parameter absent in
    micro = [_grads(a, gen), _grads(a, gen, absent=(2,))]                 # its second micro-step
    for m in micro:
        _assign(a, m)
        A.step()
    assert A.last_step_updated and float(A.last_clip_coef) < 1
    yield "d", _mean(micro, 0.5), True
    A.max_grad_norm, A.ema_decay = None, 0.9                              # (e) a window with averaging
    before = [p.detach().cpu() for p in a]
    micro = [_grads(a, gen), _grads(a, gen)]
    for m in micro:
        _assign(a, m)
        A.step()
    assert A.last_step_updated and A.ema_updates == 1
    for i, (p, e) in enumerate(zip(a, before)):                           # the averages started as the parameters BEFORE the update
        assert torch.equal(A.ema_parameter(p).cpu(), _lerp(e, p.detach().cpu(), _w32(0.9))), i
    yield "e", _mean(micro, 0.5), False
    A.gradient_accumulation_steps, A.ema_decay = 1, None                  # (f) early launches again
    grads = _early_step(A, a, gen, calls)
    # `early` is honoured again after the modes that ignore it: group 0 early and late, group 1 late
    assert calls == ["aptai_adam_multi"] * 3, calls
    yield "f", grads, False


def test_one_optimiser_through_every_mode_matches_a_plain_twin(monkeypatch):
    from aptai_amd import _lib
    from aptai_amd.optim import clip_grad_norm_
    a, b = _params(1), _params(1)
    A, B = _groups(a), _groups(b)
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    seen = []
    for step, effective, clipped in drive_through_every_mode(A, a, torch.Generator().manual_seed(2), calls):
        assert effective[NEVER] is None
        _assign(b, [None if g is None else g.clone() for g in effective])     # the twin's own: clip_grad_norm_ rescales in place
        if clipped:
            clip_grad_norm_(b, 1.0)
        B.step()
        _assert_same_optimiser_state(A, a, B, b)
        seen.append(step)
    assert seen == list("abcdef")
    assert A.state[a[NEVER]]["step"] == 0 and A.state[a[0]]["step"] == 6 and A.state[a[1]]["step"] == 5


def test_launch_early_refuses_an_interleaved_span(monkeypatch):
    from aptai_amd import _lib
    from aptai_amd.optim import Adam
    g = torch.Generator().manual_seed(3)
    a0, b0, a1, b1 = ps = [torch.nn.Parameter(torch.randn(s, generator=g).cuda()) for s in ((5, 7), (13,), (4096,), (3,))]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g).cuda()
    opt = Adam(ps, lr=1e-3)
    calls = []
    orig = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *args: (calls.append(name), orig(name, *args))[1])
    opt.prepare(early=ps)
    with pytest.raises(RuntimeError, match="parameter 1 of group 0"):
        opt.launch_early([a0, a1])                                        # the span a0 .. a1 holds b0, early in a call of its own
    assert calls == []
