"""Adam for the train step (train/train_aptai.py:350-356: betas, eps, weight_decay; no amsgrad) as ONE hand-written
multi-tensor kernel per parameter group (csrc/optim.hip) — a drop-in for ``torch.optim.Adam(model.parameters(), ...)`` with the
same constructor arguments, ``param_groups`` (LambdaLR works unchanged) and ``state`` keys (``step``, ``exp_avg``,
``exp_avg_sq``), so optimizer checkpoints interchange with torch's.

It can also refresh the model's compute copies in the same pass (``publish_to(model)``): the updated fp32 parameter is written
back AND converted into the persistent bf16 buffer the GEMMs read, which removes the separate per-step cast launch.

Global-norm gradient clipping (``torch.nn.utils.clip_grad_norm_(params, max_norm)`` before ``optimizer.step()``, the HF Trainer's
``max_grad_norm``) is fused into the step: ``Adam(..., max_grad_norm=1.0)`` measures the 2-norm of every gradient of every parameter
group with an order-fixed two-stage reduction, leaves the coefficient on the device and the Adam kernel multiplies each gradient by
it as it reads it.  ``.grad`` is NOT modified in this form: it still holds the unclipped gradient after ``step()``.
``clip_grad_norm_`` below is the in-place drop-in for a loop that wants torch's two calls.

Gradient accumulation (the HF Trainer's ``gradient_accumulation_steps``) lives here too: ``Adam(..., gradient_accumulation_steps=N)``
makes every ``step()`` one micro-step of a window of N.  The first N - 1 add the gradients into fp32 accumulators the optimiser owns
(one streaming launch, nothing else moves); the N-th multiplies them by 1/N and hands the mean to the norm and Adam kernels above.

An exponential moving average of the weights (``torch._foreach_lerp_(ema, params, 1 - decay)`` after every ``optimizer.step()``) is
the last launch of an update: ``Adam(..., ema_decay=0.999)`` keeps one fp32 average per parameter, moves it once per update (not per
micro-step of a window) and exchanges parameters and averages in place for evaluation (``with opt.ema_weights(model): ...``), telling
the model that its derived weight copies are stale.
"""
from __future__ import annotations

import contextlib
import math
import operator
from typing import Dict, Optional

import torch

from . import _lib, ops


def _check_max_norm(max_norm) -> float:
    max_norm = float(max_norm)
    if not max_norm >= 0:                           # negative or NaN
        raise ValueError(f"max_grad_norm must be >= 0 (float('inf') measures the norm without clipping), got {max_norm}")
    return max_norm


def _check_accum_steps(steps) -> int:
    try:
        steps = operator.index(steps)
    except TypeError:
        raise ValueError(f"gradient_accumulation_steps must be an integer >= 1, got {steps!r}") from None
    if steps < 1:
        raise ValueError(f"gradient_accumulation_steps must be an integer >= 1, got {steps}")
    return steps


def _check_ema_decay(decay) -> float:
    if isinstance(decay, bool) or not isinstance(decay, (int, float)) or not 0 <= decay < 1:       # also NaN
        raise ValueError(f"ema_decay must be None or a float with 0 <= ema_decay < 1, got {decay!r}")
    return float(decay)


def ema_decay_at(k: int, decay: float, warmup: bool = False) -> float:
    """Decay of the k-th averaged update, k = 1, 2, ...: `decay`, or with warm-up min(decay, (1 + k) / (10 + k)) - 2/11, 3/12, ...
    until it reaches `decay` - so that the first updates are not averaged with the initial weights at full weight.  The kernel's
    weight is (float)(1.0 - ema_decay_at(k, ...)), evaluated in double here."""
    return min(decay, (1.0 + k) / (10.0 + k)) if warmup else decay


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, gradient_accumulation_steps: int = 1, ema_decay: Optional[float] = None,
                 ema_warmup: bool = False):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameters")
        # an attribute, not a param_groups key (one norm spans all groups; state_dict() stays interchangeable with torch's)
        self.max_grad_norm = max_grad_norm
        self._accum = None                          # accumulation: accumulators, pointer tables and the open window (_accum_tables)
        self.gradient_accumulation_steps = gradient_accumulation_steps      # an attribute as well: one window spans all groups
        self.last_step_updated = False              # did the last step() / flush() update the parameters (False inside a window)
        self.ema_decay = ema_decay                  # attributes as well: one average spans all groups
        self.ema_warmup = bool(ema_warmup)
        self._ema = None                            # averaging: the averages by parameter and their pointer table (_ema_tables)
        self._ema_updates = 0
        self._ema_swapped = False                   # swap_ema(): the parameters hold the averages right now
        self._pending_ema = None
        self._models = []                           # publish_to(): the encoders whose weight copies follow these parameters
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self._copies: Dict[int, tuple] = {}         # id(param) -> (destination tensor, kind)
        self._tables: Dict[int, tuple] = {}         # group index -> (key, table tensor, max_n)
        self._plans = []
        self._span = None                           # clipping: one job table over every group (_span_tables)
        self._clip_result = None                    # clipping: device fp32 {total norm, coefficient, gradient elements}
        self._pending_clip = None
        self._pending_accum = None

    # ------------------------------------------------------------------ global-norm clipping
    @property
    def max_grad_norm(self) -> Optional[float]:
        """None: the plain step.  A value: clip the gradients of ALL parameter groups at this global 2-norm inside step() (`.grad`
        keeps the unclipped gradient); float('inf') measures the norm and clips nothing.  May be reassigned between steps."""
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, value) -> None:
        self._max_grad_norm = None if value is None else _check_max_norm(value)

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """0-dim device view of the last clipped step's global gradient norm (before clipping).  Valid after step(), overwritten by
        the next one, NOT synchronised: reading it on the host waits for the step."""
        return None if self._clip_result is None else self._clip_result[0]

    @property
    def last_clip_coef(self) -> Optional[torch.Tensor]:
        """0-dim device view of min(1, max_grad_norm / (norm + 1e-6)) of the last clipped step (see last_grad_norm)."""
        return None if self._clip_result is None else self._clip_result[1]

    # ------------------------------------------------------------------ gradient accumulation
    @property
    def gradient_accumulation_steps(self) -> int:
        """1: every step() updates.  N > 1: every step() is one micro-step of a window of N; the N-th applies the MEAN of the window's
        gradients (a parameter without a gradient in some micro-steps counts zeros for them; one without any is skipped).  `.grad`
        is never written.  May be reassigned only while no window is open."""
        return self._accum_steps

    @gradient_accumulation_steps.setter
    def gradient_accumulation_steps(self, value) -> None:
        value = _check_accum_steps(value)
        if self.micro_step:
            raise RuntimeError("gradient_accumulation_steps cannot change inside an open window: flush() first")
        self._accum_steps = value

    @property
    def micro_step(self) -> int:
        """Micro-steps the open window holds so far; 0 after an update (and always at gradient_accumulation_steps=1)."""
        return 0 if self._accum is None else self._accum["k"]

    def accumulated_grad(self, p) -> Optional[torch.Tensor]:
        """The fp32 accumulator of `p` (a view shaped like `p`, not synchronised): the sum over the open window so far or, with no
        window open, the mean gradient the last update applied.  None when `p` contributed nothing to that window, or when
        nothing has been accumulated yet."""
        acc = self._accum
        if acc is None:
            return None
        row = acc["rows"].get(id(p))
        if row is None or not (acc["seen"] if acc["k"] else acc["applied"])[row]:
            return None
        return acc["views"][row]

    # ------------------------------------------------------------------ exponential moving average of the weights
    @property
    def ema_decay(self) -> Optional[float]:
        """None: no averaging, nothing is allocated or launched.  A value d in [0, 1): every step() / flush() that updates the
        parameters ends with ONE launch that moves an fp32 average of every parameter of every group, ema += (1 - d_k) * (p - ema),
        d_k = ema_decay_at(k, d, ema_warmup) for the k-th such update.  The averages start as a copy of the parameters at the first
        step with averaging on; a parameter without a gradient in an update still averages.  May be reassigned between steps."""
        return self._ema_decay

    @ema_decay.setter
    def ema_decay(self, value) -> None:
        self._ema_decay = None if value is None else _check_ema_decay(value)

    @property
    def ema_updates(self) -> int:
        """k: how many updates the averages have taken."""
        return self._ema_updates

    def ema_parameter(self, p) -> Optional[torch.Tensor]:
        """The average of `p` (a view shaped like `p`, not synchronised); None when averaging is off, has not started, or `p` is not
        updated on the device."""
        if self._ema_decay is None or self._ema is None:
            return None
        return self._ema["views"].get(id(p))

    def _ema_tables(self, span, ts):
        """Averaging: one fp32 average per row of the span table (slices of ONE buffer, each 16-byte aligned so that the kernels take
        their vector paths) and their device pointer table.  The averages are kept BY PARAMETER: a rebuilt span (publish_to,
        load_state_dict) only rebuilds the pointer table; a parameter seen for the first time starts as a copy of itself."""
        ema = self._ema
        if ema is not None and ema["span"] is span:
            return ema
        views, bufs = ({}, []) if ema is None else (ema["views"], ema["bufs"])
        params = [p for t, _ in ts for p in t["params"]]
        fresh = [p for p in params if id(p) not in views]
        if fresh:
            offs, total = [], 0
            for p in fresh:
                offs.append(total)
                total += (p.numel() + 3) // 4 * 4
            buf = torch.empty(total, dtype=torch.float32, device=span["dev"])
            for o, p in zip(offs, fresh):
                views[id(p)] = buf[o:o + p.numel()].view(p.shape)
                views[id(p)].copy_(p.detach())
            bufs.append(buf)
        ptrs = [views[id(p)].data_ptr() for p in params]
        self._ema = dict(span=span, views=views, bufs=bufs, ptrs_dev=torch.tensor(ptrs, dtype=torch.int64).to(span["dev"]))
        return self._ema

    @torch.no_grad()
    def _ema_ready(self):
        """The averages and their pointer table over the current job tables (allocated and filled on first use), or None without
        parameters on the device."""
        ts = [(self._group_tables(gi, g), g) for gi, g in enumerate(self.param_groups) if any(p.is_cuda for p in g["params"])]
        if not ts:
            return None
        return self._ema_tables(self._span_tables([t for t, _ in ts], clip=False), ts)

    def ema_state_dict(self) -> dict:
        """What a resumed run needs beside state_dict() (whose keys stay torch's): the settings, k and a copy of every average in
        `param_groups` order (None for a parameter that has none)."""
        ema = self._ema_ready() if self._ema_decay is not None else self._ema
        views = {} if ema is None else ema["views"]
        return dict(decay=self._ema_decay, warmup=self.ema_warmup, updates=self._ema_updates,
                    ema=[views[id(p)].clone() if id(p) in views else None for g in self.param_groups for p in g["params"]])

    @torch.no_grad()
    def load_ema_state_dict(self, sd: dict) -> None:
        params = [p for g in self.param_groups for p in g["params"]]
        if len(sd["ema"]) != len(params):
            raise ValueError(f"load_ema_state_dict: {len(sd['ema'])} averages for {len(params)} parameters")
        self.ema_decay, self.ema_warmup, self._ema_updates = sd["decay"], bool(sd["warmup"]), int(sd["updates"])
        ema = self._ema_ready() if self._ema_decay is not None else None
        for p, t in zip(params, sd["ema"]):
            if t is not None and ema is not None and id(p) in ema["views"]:
                ema["views"][id(p)].copy_(t)

    @torch.no_grad()
    def swap_ema(self, model=None) -> None:
        """Exchanges parameters and averages in place, one launch: pointers do not move, so job tables, captured graphs and
        data-parallel buckets stay valid.  `model` (default: the models of publish_to()) is told that its weights moved
        (Wav2Vec2Model.weights_moved): its eval-mode weight copies miss and the published bf16 copies are re-cast.  A second call
        puts everything back, bit for bit.  Not while a window is open; step() refuses to run on the averages."""
        if self._ema_decay is None:
            raise RuntimeError("swap_ema() needs ema_decay: this optimiser keeps no averages")
        if self.micro_step:
            raise RuntimeError("swap_ema() inside an open accumulation window: flush() first")
        ema = self._ema_ready()
        if ema is not None:
            span = ema["span"]
            ops.swap_multi(span["table"].data_ptr(), ema["ptrs_dev"].data_ptr(), span["n"], span["max_n"])
        self._ema_swapped = not self._ema_swapped
        if model is None:
            moved = self._models
        else:
            moved = [getattr(model, "wav2vec2", None) or getattr(getattr(model, "w2v2_pr", None), "wav2vec2", None) or model]
        for w2v in moved:
            if hasattr(w2v, "weights_moved"):       # a module without derived weight copies has nothing to be told
                w2v.weights_moved()

    @contextlib.contextmanager
    def ema_weights(self, model=None):
        """`with opt.ema_weights(model):` the model's parameters ARE the averages inside the block (validation, checkpoints) and the
        training weights again behind it, also when the block raises.  Does not nest."""
        if self._ema_swapped:
            raise RuntimeError("ema_weights() does not nest: the parameters already hold the averages")
        self.swap_ema(model)
        try:
            yield self
        finally:
            self.swap_ema(model)

    # ------------------------------------------------------------------ compute copies
    def publish_to(self, model) -> "Adam":
        """Refresh the wav2vec2 layer compute copies (ops.CastPlan destinations) inside the optimiser kernel."""
        w2v = getattr(model, "wav2vec2", None) or getattr(getattr(model, "w2v2_pr", None), "wav2vec2", None) or model
        plan = w2v._layer_plan()
        by_ptr = {p.data_ptr(): p for g in self.param_groups for p in g["params"]}
        for src, dst in plan.jobs:
            p = by_ptr.get(src.data_ptr())
            if p is not None and p.numel() == dst.numel():
                self._copies[id(p)] = (dst, 0 if dst.dtype == torch.bfloat16 else 1)
        self._plans.append(plan)
        self._models.append(w2v)
        self._tables.clear()
        self._span = None
        self._accum = None
        return self

    # ------------------------------------------------------------------ step
    def _group_tables(self, gi: int, group):
        """Static job table of a parameter group (all its parameters, whether or not they get a gradient this step) and a
        small ring of pinned host buffers for the per-step columns {grad pointer, step count} (two planes: prepare())."""
        key = tuple(p.data_ptr() for p in group["params"])
        cached = self._tables.get(gi)
        if cached is not None and cached["key"] == key:
            return cached
        # parameters the kernel cannot update (e.g. the float64 low-pass taps, which are never trained) stay out of the table;
        # step() raises if one of them ever shows up with a gradient
        params = [p for p in group["params"] if p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()]
        others = [p for p in group["params"] if not (p.is_cuda and p.dtype == torch.float32 and p.is_contiguous())]
        rows = []
        for p in params:
            st = self.state[p]
            if len(st) == 0:
                st["step"] = 0                        # python int here; state_dict() emits torch's tensor form
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            dst, kind = self._copies.get(id(p), (None, 0))
            rows.append([p.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), 0 if dst is None else dst.data_ptr(),
                         p.numel(), kind])
        dev = params[0].device
        cached = dict(key=key, table=torch.tensor(rows, dtype=torch.int64).to(dev), max_n=max(r[4] for r in rows),
                      numels=[r[4] for r in rows], dyn_dev=torch.zeros((2, len(params), 2), dtype=torch.int64, device=dev),
                      ring=[torch.zeros((2, len(params), 2), dtype=torch.int64).pin_memory() for _ in range(4)],
                      events=[None] * 4, turn=0, states=[self.state[p] for p in params], params=params, others=others)
        self._tables[gi] = cached
        return cached

    def _span_tables(self, ts, clip: bool = True):
        """Clipping and accumulation: ONE job table over the rows of every group (`ts`: the groups' tables in group order), so that one norm spans
        them and its summation order depends on the tables alone; per-step rows, pinned ring, partial-sum workspace and the result
        words are allocated here, never inside a step.  The groups' Adam launches read row ranges of this table.  `clip` False (accumulation
        without clipping): the table alone; the norm's workspace and result words follow when clipping is first asked for."""
        span = self._span
        if span is None or len(span["tables"]) != len(ts) or not all(a is t["table"] for a, t in zip(span["tables"], ts)):
            devs = {t["table"].device for t in ts}
            if len(devs) != 1:
                raise _lib.AptaiHipError("aptai_amd.optim.Adam(max_grad_norm=... / gradient_accumulation_steps=...): one global norm or "
                                         "one window needs every parameter group on one device")
            dev = devs.pop()
            offs, n = {}, 0
            for t in ts:
                offs[id(t)] = n
                n += len(t["params"])
            numels = [m for t in ts for m in t["numels"]]
            span = dict(tables=[t["table"] for t in ts], table=torch.cat([t["table"] for t in ts]).contiguous(), offs=offs, n=n,
                        max_n=max(numels), numels=numels, dev=dev, dyn_dev=torch.zeros((n, 2), dtype=torch.int64, device=dev),
                        partials=None, ring=[torch.zeros((n, 2), dtype=torch.int64).pin_memory() for _ in range(4)], events=[None] * 4,
                        turn=0)
            self._span = span
        if clip and span["partials"] is None:
            if self._clip_result is None or self._clip_result.device != span["dev"]:
                self._clip_result = torch.zeros(3, dtype=torch.float32, device=span["dev"])
            span["partials"] = torch.zeros(ops.grad_norm_chunks(span["numels"]), dtype=torch.float32, device=span["dev"])
        return span

    def _accum_tables(self, span, ts):
        """Accumulation: one fp32 accumulator per row of the span table (slices of ONE buffer, each 16-byte aligned so that the
        accumulate and Adam kernels take their vector paths), their device pointer table, the per-call rows - plane 0 what the norm
        and Adam launches of a closing step read {accumulator, step count}, plane 1 what the accumulate launch reads {grad, mode} -
        and their pinned ring.  Allocated when the first window opens; a rebuilt span (publish_to, load_state_dict) discards the
        open window with the old accumulators."""
        acc = self._accum
        if acc is not None and acc["span"] is span:
            return acc
        n, offs, total = span["n"], [], 0
        for m in span["numels"]:
            offs.append(total)
            total += (m + 3) // 4 * 4
        buf = torch.empty(total, dtype=torch.float32, device=span["dev"])
        params = [p for t, _ in ts for p in t["params"]]
        views = [buf[o:o + m].view(p.shape) for o, m, p in zip(offs, span["numels"], params)]
        ptrs = [v.data_ptr() for v in views]
        acc = dict(span=span, buf=buf, views=views, ptrs=ptrs, ptrs_dev=torch.tensor(ptrs, dtype=torch.int64).to(span["dev"]),
                   rows={id(p): r for r, p in enumerate(params)}, dyn_dev=torch.zeros((2, n, 2), dtype=torch.int64, device=span["dev"]),
                   ring=[torch.zeros((2, n, 2), dtype=torch.int64).pin_memory() for _ in range(4)], events=[None] * 4, turn=0,
                   seen=[False] * n, applied=[False] * n, k=0)
        self._accum = acc
        return acc

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.prepare()
        self.finish()
        return loss

    # ------------------------------------------------------------------ the step in pieces (aptai_amd.graphed: optimiser under the backward pass)
    @torch.no_grad()
    def prepare(self, early=()) -> None:
        """Host half of step(): step counts and the per-step {gradient pointer, step} column of every group, copied to the device
        on the current stream.  `early` names parameters whose update will be launched by launch_early() (once their gradient is
        final, on any stream ordered behind this call) before finish() updates the rest.  Every parameter's `.grad` must already
        be the tensor its gradient WILL be in (static gradient buffers): the kernel reads it only when it is launched."""
        stream = torch.cuda.current_stream()
        self._pending = []
        self._pending_clip = None
        self._pending_accum = None
        self._prepare_ema()
        # the averaging launch follows EVERY update of the step: with it on, every row goes to finish() and `early` is ignored, too
        early_ids = set() if self._pending_ema is not None else {id(p) for p in early}
        if self._accum_steps > 1:
            # a window's mean does not exist before its last gradient does: every row goes to finish(), `early` is ignored
            return self._prepare_accum(stream, True)
        if self._max_grad_norm is not None:
            # the global norm does not exist before the last gradient does: every row goes to finish(), `early` is ignored
            # (launch_early() then finds nothing to do and the step is the one-launch step, bit for bit)
            return self._prepare_clipped(stream)
        for gi, group in enumerate(self.param_groups):
            if not any(p.is_cuda for p in group["params"]):
                if any(p.grad is not None for p in group["params"]):
                    raise _lib.AptaiHipError("aptai_amd.optim.Adam needs parameters on the MI355X (no CPU fallback)")
                continue
            t = self._group_tables(gi, group)
            params = t["params"]
            if any(p.grad is not None for p in t["others"]):
                raise _lib.AptaiHipError("aptai_amd.optim.Adam updates contiguous fp32 parameters on the MI355X only")
            slot = t["turn"]
            t["turn"] = (slot + 1) % len(t["ring"])
            if t["events"][slot] is not None:
                t["events"][slot].synchronize()        # the copy that last used this pinned buffer has been consumed
            host = t["ring"][slot].numpy()             # [2][n][2]: plane 0 = rows finish() updates, plane 1 = rows launch_early() updates
            host[:, :, 0] = 0
            any_late = any_early = False
            for j, (p, st) in enumerate(zip(params, t["states"])):
                g = p.grad
                if g is None:
                    continue
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise _lib.AptaiHipError("aptai_amd.optim.Adam needs contiguous fp32 gradients")
                st["step"] += 1
                plane = 1 if id(p) in early_ids else 0
                host[plane, j, 0] = g.data_ptr()
                host[plane, j, 1] = st["step"]
                any_early |= plane == 1
                any_late |= plane == 0
            if not (any_late or any_early):
                continue
            t["dyn_dev"].copy_(t["ring"][slot], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            t["events"][slot] = ev
            self._pending.append((t, group, any_late))

    def _prepare_ema(self) -> None:
        """Averaging on: the averages exist (a copy of the parameters as they are BEFORE the first averaged update) and their pointer
        table matches the job tables before finish() launches anything."""
        if self._ema_swapped:
            raise RuntimeError("the parameters hold their averages (swap_ema() / ema_weights()): swap back before the next step")
        self._pending_ema = None if self._ema_decay is None else self._ema_ready()

    def _device_groups(self):
        """[(table, group)] of the groups with parameters on the device, after prepare()'s checks."""
        ts = []
        for gi, group in enumerate(self.param_groups):
            if not any(p.is_cuda for p in group["params"]):
                if any(p.grad is not None for p in group["params"]):
                    raise _lib.AptaiHipError("aptai_amd.optim.Adam needs parameters on the MI355X (no CPU fallback)")
                continue
            t = self._group_tables(gi, group)
            if any(p.grad is not None for p in t["others"]):
                raise _lib.AptaiHipError("aptai_amd.optim.Adam updates contiguous fp32 parameters on the MI355X only")
            ts.append((t, group))
        return ts

    def _prepare_accum(self, stream, contribute: bool) -> None:
        """prepare() with accumulation on: one micro-step (`contribute`) or the early close of flush().  Plane 1 of the per-call rows
        names this micro-step's gradients for the accumulate launch; a micro-step that closes the window also fills plane 0 with the
        accumulators as gradient pointers and the step counts of the rows that contributed, which finish() hands to the usual
        launches.  One pinned buffer, one copy."""
        ts = self._device_groups()
        if not ts:
            return
        span = self._span_tables([t for t, _ in ts], clip=self._max_grad_norm is not None)
        acc = self._accum_tables(span, ts)
        if not contribute and acc["k"] == 0:
            return
        slot = acc["turn"]
        acc["turn"] = (slot + 1) % len(acc["ring"])
        if acc["events"][slot] is not None:
            acc["events"][slot].synchronize()          # the copy that last used this pinned buffer has been consumed
        host = acc["ring"][slot].numpy()               # [2][rows of all groups][2]
        host[:] = 0
        seen, any_grad = acc["seen"], False
        for t, group in ts:
            off = span["offs"][id(t)]
            for j, p in enumerate(t["params"]):
                g = p.grad if contribute else None
                if g is not None:
                    if g.dtype != torch.float32 or not g.is_contiguous():
                        raise _lib.AptaiHipError("aptai_amd.optim.Adam needs contiguous fp32 gradients")
                    host[1, off + j, 0] = g.data_ptr()
                    host[1, off + j, 1] = 2 if seen[off + j] else 1
                    seen[off + j] = any_grad = True
                elif seen[off + j]:
                    host[1, off + j, 1] = 2
        if contribute:
            if not any_grad and acc["k"] == 0:
                return                                 # nothing has a gradient and no window is open: nothing to do, as at N = 1
            acc["k"] += 1
        close = not contribute or acc["k"] >= self._accum_steps
        scale = 1.0 / acc["k"] if close else 1.0
        if close:
            for t, group in ts:
                off, any_seen = span["offs"][id(t)], False
                for j, st in enumerate(t["states"]):
                    if seen[off + j]:
                        st["step"] += 1
                        host[0, off + j, 0] = acc["ptrs"][off + j]
                        host[0, off + j, 1] = st["step"]
                        any_seen = True
                if any_seen:
                    self._pending.append((t, group, True))
            acc["applied"], acc["seen"], acc["k"] = seen, [False] * span["n"], 0
        acc["dyn_dev"].copy_(acc["ring"][slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        acc["events"][slot] = ev
        # scale == 1 without a gradient (a flush() after one micro-step): the accumulators already hold the mean
        self._pending_accum = (span, acc, scale, close, any_grad or scale != 1.0, self._max_grad_norm)

    def _prepare_clipped(self, stream) -> None:
        """prepare() with clipping on: the same checks and step counts, the per-step rows of ALL groups in one table, one copy."""
        ts = self._device_groups()
        if not ts:
            return
        span = self._span_tables([t for t, _ in ts])
        slot = span["turn"]
        span["turn"] = (slot + 1) % len(span["ring"])
        if span["events"][slot] is not None:
            span["events"][slot].synchronize()         # the copy that last used this pinned buffer has been consumed
        host = span["ring"][slot].numpy()              # [rows of all groups][2]
        host[:, 0] = 0
        for t, group in ts:
            off, any_grad = span["offs"][id(t)], False
            for j, (p, st) in enumerate(zip(t["params"], t["states"])):
                g = p.grad
                if g is None:
                    continue
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise _lib.AptaiHipError("aptai_amd.optim.Adam needs contiguous fp32 gradients")
                st["step"] += 1
                host[off + j, 0] = g.data_ptr()
                host[off + j, 1] = st["step"]
                any_grad = True
            if any_grad:
                self._pending.append((t, group, True))
        if not self._pending:
            return
        span["dyn_dev"].copy_(span["ring"][slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        span["events"][slot] = ev
        self._pending_clip = (span, self._max_grad_norm)

    def _launch(self, t, group, plane: int, r0: int, r1: int, stream) -> None:
        b1, b2 = group["betas"]
        _lib.call("aptai_adam_multi", t["table"][r0].data_ptr(), t["dyn_dev"][plane, r0].data_ptr(), r1 - r0, max(t["numels"][r0:r1]),
                  float(group["lr"]), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]), stream.cuda_stream)

    @torch.no_grad()
    def launch_early(self, params, stream=None) -> None:
        """Update `params` (named in prepare(early=...)) now, on `stream`: one launch per parameter group over the row range that
        spans them (rows in between that were not named `early` carry no gradient pointer in this plane and are skipped)."""
        stream = stream or torch.cuda.current_stream()
        if self._pending_clip is not None or self._pending_accum is not None or self._pending_ema is not None:
            return
        ids = {id(p) for p in params}
        for t, group, _ in self._pending:
            rows = [j for j, p in enumerate(t["params"]) if id(p) in ids]
            if rows:
                self._launch(t, group, 1, min(rows), max(rows) + 1, stream)

    @torch.no_grad()
    def finish(self, stream=None) -> None:
        """Update every parameter that has a gradient and was not named `early`."""
        stream = stream or torch.cuda.current_stream()
        self.last_step_updated = self._accum_steps == 1
        applied = bool(self._pending)               # some parameter is updated by this call (inside a window: none)
        if self._pending_accum is not None:
            self._finish_accum(stream)
        elif self._pending_clip is not None:
            # here, not in prepare(): every gradient is final now (and, under data parallelism, already averaged: the norm is that
            # of the averaged gradient and the same on every rank).  Two norm launches, then the groups' Adam launches read the
            # coefficient from the device on the same stream
            span, max_norm = self._pending_clip
            tab, dyn, coef = span["table"].data_ptr(), span["dyn_dev"].data_ptr(), self._clip_result[1:2]
            ops.grad_sqnorm_multi(tab, dyn, span["n"], span["max_n"], span["partials"], self._clip_result, max_norm, stream.cuda_stream)
            for t, group, _ in self._pending:
                off = span["offs"][id(t)]
                b1, b2 = group["betas"]
                ops.adam_multi_scaled(tab + off * 48, dyn + off * 16, len(t["params"]), t["max_n"], group["lr"], b1, b2, group["eps"],
                                      group["weight_decay"], coef, stream.cuda_stream)
            self._pending_clip = None
        else:
            for t, group, any_late in self._pending:
                if any_late:
                    self._launch(t, group, 0, 0, len(t["params"]), stream)
        self._pending = []
        for plan in self._plans:                    # the copies of every parameter that had a gradient are fresh now;
            plan.optimizer_synced = True            # parameters without one did not move (nor did any inside a window)
        ema, self._pending_ema = self._pending_ema, None
        if ema is not None and applied and self._ema_decay is not None:
            # ONE launch over the rows of all groups, behind every Adam launch of this call on the same stream
            self._ema_updates += 1
            span = ema["span"]
            ops.ema_multi(span["table"].data_ptr(), ema["ptrs_dev"].data_ptr(), span["n"], span["max_n"],
                          1.0 - ema_decay_at(self._ema_updates, self._ema_decay, self.ema_warmup), stream.cuda_stream)

    def _finish_accum(self, stream) -> None:
        """finish() with accumulation on: the accumulate launch and, when the micro-step closes the window, today's launches on the
        accumulated mean - the groups' Adam launches, behind the norm launches under clipping - over row ranges of the span table."""
        span, acc, scale, close, launch, max_norm = self._pending_accum
        self._pending_accum = None
        tab, dyn = span["table"].data_ptr(), acc["dyn_dev"]
        if launch:
            ops.grad_accum_multi(tab, dyn[1].data_ptr(), acc["ptrs_dev"].data_ptr(), span["n"], span["max_n"], scale, stream.cuda_stream)
        self.last_step_updated = close
        if not close:
            return
        dyn = dyn[0].data_ptr()
        if max_norm is not None:
            coef = self._clip_result[1:2]
            ops.grad_sqnorm_multi(tab, dyn, span["n"], span["max_n"], span["partials"], self._clip_result, max_norm, stream.cuda_stream)
        for t, group, _ in self._pending:
            off = span["offs"][id(t)]
            b1, b2 = group["betas"]
            if max_norm is not None:
                ops.adam_multi_scaled(tab + off * 48, dyn + off * 16, len(t["params"]), t["max_n"], group["lr"], b1, b2, group["eps"],
                                      group["weight_decay"], coef, stream.cuda_stream)
            else:
                _lib.call("aptai_adam_multi", tab + off * 48, dyn + off * 16, len(t["params"]), t["max_n"], float(group["lr"]), float(b1),
                          float(b2), float(group["eps"]), float(group["weight_decay"]), stream.cuda_stream)

    @torch.no_grad()
    def flush(self) -> bool:
        """Close the open window now: the update applies the mean over the micro-steps the window holds (a remainder at the end of an
        epoch).  Returns whether an update happened; with no window open it launches nothing."""
        if self.micro_step == 0:
            self.last_step_updated = False
            return False
        self._pending = []
        self._pending_clip = None
        self._prepare_ema()
        self._prepare_accum(torch.cuda.current_stream(), False)
        self.finish()
        return True

    @property
    def publishes_copies(self) -> bool:
        return bool(self._plans)

    # ------------------------------------------------------------------ checkpoints interchange with torch.optim.Adam
    def state_dict(self):
        sd = super().state_dict()
        for st in sd["state"].values():
            if "step" in st and not torch.is_tensor(st["step"]):
                st["step"] = torch.tensor(float(st["step"]), dtype=torch.float32)
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if torch.is_tensor(st.get("step")):
                st["step"] = int(st["step"].item())
        self._tables.clear()                        # the moment buffers were replaced: rebuild the job tables
        self._span = None
        self._accum = None                          # an open window is discarded with them


def clip_grad_norm_(parameters, max_norm: float, norm_type: float = 2.0, error_if_nonfinite: bool = False, foreach=None) -> torch.Tensor:
    """Drop-in for ``torch.nn.utils.clip_grad_norm_`` in a loop of the user's own: the order-fixed norm kernel of
    ``Adam(max_grad_norm=...)``, then the gradients are multiplied IN PLACE by min(1, max_norm / (norm + 1e-6)) read from the device.
    Returns the total norm as a 0-dim device tensor, not synchronised.  2-norm only; contiguous fp32 gradients on one MI355X only (no
    fallback).  ``error_if_nonfinite=True`` reads the norm back - a host synchronisation - and raises before anything is scaled.
    ``foreach`` is accepted and ignored.  The pointer table is built per call from pageable memory: a convenience, not the hot path
    (that is ``Adam(max_grad_norm=...)``, which reads each gradient once more instead of rewriting it)."""
    if float(norm_type) != 2.0:
        raise ValueError(f"aptai_amd.optim.clip_grad_norm_ computes the 2-norm only (norm_type={norm_type})")
    max_norm = _check_max_norm(max_norm)
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [p.grad for p in parameters if p.grad is not None]
    for g in grads:
        if not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
            raise _lib.AptaiHipError("aptai_amd.optim.clip_grad_norm_ needs contiguous fp32 gradients on the MI355X (no CPU fallback)")
    if len({g.device for g in grads}) > 1:
        raise _lib.AptaiHipError("aptai_amd.optim.clip_grad_norm_: gradients on more than one device")
    grads = [g for g in grads if g.numel() > 0]
    if not grads:
        return torch.zeros(())
    dev = grads[0].device
    numels = [g.numel() for g in grads]
    table = torch.tensor([[0, 0, 0, 0, n, 0] for n in numels], dtype=torch.int64).to(dev)
    dyn = torch.tensor([[g.data_ptr(), 0] for g in grads], dtype=torch.int64).to(dev)
    partials = torch.empty(ops.grad_norm_chunks(numels), dtype=torch.float32, device=dev)
    result = torch.empty(3, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    ops.grad_sqnorm_multi(table.data_ptr(), dyn.data_ptr(), len(grads), max(numels), partials, result, max_norm, stream)
    if error_if_nonfinite and not math.isfinite(result[0].item()):
        raise RuntimeError("The total norm for gradients from `parameters` is non-finite, so it cannot be clipped. To disable this "
                           "error and scale the gradients by the non-finite norm anyway, set `error_if_nonfinite=False`")
    ops.scale_multi(table.data_ptr(), dyn.data_ptr(), len(grads), max(numels), result[1:2], stream)
    return result[0]


class ClipMonitor:
    """What the training loops log about clipping: adds the optimiser's device-side norm and `coef < 1` into two device scalars after
    each step and reads them back ONCE per epoch (epoch_log())."""

    def __init__(self, optimizer):
        if getattr(optimizer, "max_grad_norm", None) is None:
            raise _lib.AptaiHipError("cfg.max_grad_norm needs an aptai_amd.optim.Adam built with max_grad_norm=... (no clipping fallback)")
        self.opt = optimizer
        self.acc = None
        self.steps = 0

    def update(self) -> None:
        norm, coef = self.opt.last_grad_norm, self.opt.last_clip_coef
        if norm is None:                            # no step with clipping yet (nothing had a gradient)
            return
        if self.acc is None:
            self.acc = torch.zeros(2, dtype=torch.float32, device=norm.device)
        self.acc[0] += norm
        self.acc[1] += coef < 1
        self.steps += 1

    def epoch_log(self) -> dict:
        sums = [0.0, 0.0] if self.acc is None else self.acc.tolist()
        out = dict(mean_grad_norm=sums[0] / max(self.steps, 1), clipped_steps=int(sums[1]))
        if self.acc is not None:
            self.acc.zero_()
        self.steps = 0
        return out
