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
from types import SimpleNamespace
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


# Bytes per row of the two tables every launch takes by address (AdamArgs in csrc/optim.hip): `table` rows of six int64
# {param, exp_avg, exp_avg_sq, copy_dst, n, copy_kind}, `dyn` rows of two {pointer, step count or mode}.
_TABLE_ROW, _DYN_ROW = 48, 16


def _addr(t, plane: int, r0: int = 0):
    """(job table address, per-call row address) of row `r0` of the job table `t`, the rows in `plane` of its row buffer."""
    return t.table_ptr + r0 * _TABLE_ROW, t.rows_ptr + (plane * t.n + r0) * _DYN_ROW


def _updatable(p) -> bool:
    return p.is_cuda and p.dtype == torch.float32 and p.is_contiguous()


def _packed_fp32(params, dev) -> list:
    """One fp32 view shaped like each of `params`: slices of ONE new buffer, each 16-byte aligned so that the kernels take their
    vector paths."""
    offs, total = [], 0
    for p in params:
        offs.append(total)
        total += (p.numel() + 3) // 4 * 4
    buf = torch.empty(total, dtype=torch.float32, device=dev)
    return [buf[o:o + p.numel()].view(p.shape) for o, p in zip(offs, params)]


def _encoder_of(model):
    """The wav2vec2 encoder behind an APTAI / Wav2Vec2_PR / Force_APTAI model, or the model itself."""
    return getattr(model, "wav2vec2", None) or getattr(getattr(model, "w2v2_pr", None), "wav2vec2", None) or model


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 max_grad_norm: Optional[float] = None, gradient_accumulation_steps: int = 1, ema_decay: Optional[float] = None,
                 ema_warmup: bool = False):
        if lr < 0 or eps < 0 or not (0 <= betas[0] < 1) or not (0 <= betas[1] < 1) or weight_decay < 0:
            raise ValueError("invalid Adam hyper-parameters")
        # an attribute, not a param_groups key (one norm spans all groups; state_dict() stays interchangeable with torch's)
        self.max_grad_norm = max_grad_norm
        self._accum = None                          # accumulation: accumulators, their pointer table and the open window (_accumulators)
        self.gradient_accumulation_steps = gradient_accumulation_steps      # an attribute as well: one window spans all groups
        self.last_step_updated = False              # did the last step() / flush() update the parameters (False inside a window)
        self.ema_decay = ema_decay                  # attributes as well: one average spans all groups
        self.ema_warmup = bool(ema_warmup)
        self._ema = None                            # averaging: the averages by parameter and their pointer table (_ema_tables)
        self._ema_updates = 0
        self._ema_swapped = False                   # swap_ema(): the parameters hold the averages right now
        self._models = []                           # publish_to(): the encoders whose weight copies follow these parameters
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay))
        self._copies: Dict[int, tuple] = {}         # id(param) -> (destination tensor, kind)
        self._plans = []
        self._table = None                          # the job table over every group, its per-call rows and their ring (_job_table)
        self._clip_result = None                    # clipping: device fp32 {total norm, coefficient, gradient elements}
        self._pending = None                        # what prepare() decided, for launch_early() and finish()

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
        return 0 if self._accum is None else self._accum.k

    def accumulated_grad(self, p) -> Optional[torch.Tensor]:
        """The fp32 accumulator of `p` (a view shaped like `p`, not synchronised): the sum over the open window so far or, with no
        window open, the mean gradient the last update applied.  None when `p` contributed nothing to that window, or when
        nothing has been accumulated yet."""
        acc = self._accum
        if acc is None:
            return None
        row = acc.table.row_of.get(id(p))
        if row is None or not (acc.seen if acc.k else acc.applied)[row]:
            return None
        return acc.views[row]

    def _accumulators(self, t):
        """Accumulation: one fp32 accumulator per row of the job table and their device pointer table, allocated when the first
        window opens.  A rebuilt job table (publish_to, load_state_dict) discards the open window with the old accumulators."""
        acc = self._accum
        if acc is None or acc.table is not t:
            views = _packed_fp32(t.params, t.dev)
            ptrs = [v.data_ptr() for v in views]
            acc = self._accum = SimpleNamespace(table=t, views=views, ptrs=ptrs, ptrs_dev=torch.tensor(ptrs, dtype=torch.int64).to(t.dev),
                                                seen=[False] * t.n, applied=[False] * t.n, k=0)
        return acc

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
        return self._ema.views.get(id(p))

    @torch.no_grad()
    def _ema_tables(self):
        """Averaging: one fp32 average per row of the current job table and their device pointer table (allocated and filled on
        first use), or None without parameters on the device.  The averages are kept BY PARAMETER: a rebuilt job table (publish_to,
        load_state_dict) only rebuilds the pointer table; a parameter seen for the first time starts as a copy of itself."""
        t = self._job_table()
        if t.n == 0:
            return None
        ema = self._ema
        if ema is None or ema.table is not t:
            views = {} if ema is None else ema.views
            fresh = [p for p in t.params if id(p) not in views]
            for p, v in zip(fresh, _packed_fp32(fresh, t.dev)):
                views[id(p)] = v.copy_(p.detach())
            ptrs = [views[id(p)].data_ptr() for p in t.params]
            ema = self._ema = SimpleNamespace(table=t, views=views, ptrs_dev=torch.tensor(ptrs, dtype=torch.int64).to(t.dev))
        return ema

    def ema_state_dict(self) -> dict:
        """What a resumed run needs beside state_dict() (whose keys stay torch's): the settings, k and a copy of every average in
        `param_groups` order (None for a parameter that has none)."""
        ema = self._ema_tables() if self._ema_decay is not None else self._ema
        views = {} if ema is None else ema.views
        return dict(decay=self._ema_decay, warmup=self.ema_warmup, updates=self._ema_updates,
                    ema=[views[id(p)].clone() if id(p) in views else None for g in self.param_groups for p in g["params"]])

    @torch.no_grad()
    def load_ema_state_dict(self, sd: dict) -> None:
        params = [p for g in self.param_groups for p in g["params"]]
        if len(sd["ema"]) != len(params):
            raise ValueError(f"load_ema_state_dict: {len(sd['ema'])} averages for {len(params)} parameters")
        self.ema_decay, self.ema_warmup, self._ema_updates = sd["decay"], bool(sd["warmup"]), int(sd["updates"])
        ema = self._ema_tables() if self._ema_decay is not None else None
        for p, t in zip(params, sd["ema"]):
            if t is not None and ema is not None and id(p) in ema.views:
                ema.views[id(p)].copy_(t)

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
        ema = self._ema_tables()
        if ema is not None:
            t = ema.table
            ops.swap_multi(t.table_ptr, ema.ptrs_dev.data_ptr(), t.n, t.max_n)
        self._ema_swapped = not self._ema_swapped
        for w2v in self._models if model is None else [_encoder_of(model)]:
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
        w2v = _encoder_of(model)
        plan = w2v._layer_plan()
        by_ptr = {p.data_ptr(): p for g in self.param_groups for p in g["params"]}
        for src, dst in plan.jobs:
            p = by_ptr.get(src.data_ptr())
            if p is not None and p.numel() == dst.numel():
                self._copies[id(p)] = (dst, 0 if dst.dtype == torch.bfloat16 else 1)
        self._plans.append(plan)
        self._models.append(w2v)
        self._table = None
        self._accum = None
        return self

    @property
    def publishes_copies(self) -> bool:
        return bool(self._plans)

    # ------------------------------------------------------------------ step
    def _job_table(self):
        """The ONE job table of the optimiser: a static row per updatable parameter of every device-resident group, in group order
        (whether or not it gets a gradient this step), so that one norm, one window and one average span the groups and the norm's
        summation order depends on the table alone; each group is a row range of it.  With it the per-call rows, int64 [2][n][2] on
        the device - plane 0 is what the norm and Adam launches of finish() read {gradient or accumulator pointer, step count}, plane 1
        what runs before them: the `early` rows of launch_early() or the {gradient, mode} rows of the accumulate launch - and the ring
        of pinned buffers that feeds them.  Everything a step needs is allocated here or when a mode is first used, never later."""
        key = tuple(tuple(p.data_ptr() for p in g["params"]) for g in self.param_groups)
        t = self._table
        if t is not None and t.key == key:
            return t
        # parameters the kernel cannot update (e.g. the float64 low-pass taps, which are never trained) stay out of the table;
        # prepare() raises if one of them, or one of a group that lives on the CPU, ever shows up with a gradient
        params, others, cpu, groups = [], [], [], []
        for gi, group in enumerate(self.param_groups):
            if not any(p.is_cuda for p in group["params"]):
                cpu += group["params"]
                continue
            mine = [p for p in group["params"] if _updatable(p)]
            others += [p for p in group["params"] if not _updatable(p)]
            if mine:
                groups.append((gi, len(params), len(params) + len(mine), max(p.numel() for p in mine)))     # (group, r0, r1, max_n)
                params += mine
        if len({p.device for p in params}) > 1:
            raise _lib.AptaiHipError("aptai_amd.optim.Adam(max_grad_norm=... / gradient_accumulation_steps=...): one global norm or "
                                     "one window needs every parameter group on one device")
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
        t = SimpleNamespace(key=key, n=len(params), params=params, states=[self.state[p] for p in params], others=others, cpu=cpu,
                            groups=groups, row_of={id(p): r for r, p in enumerate(params)}, numels=[r[4] for r in rows],
                            partials=None)         # clipping: the norm's partial sums, allocated when clipping is first asked for
        if params:
            t.dev, t.max_n = params[0].device, max(t.numels)
            t.table = torch.tensor(rows, dtype=torch.int64).to(t.dev)
            t.rows = torch.zeros((2, t.n, 2), dtype=torch.int64, device=t.dev)
            t.table_ptr, t.rows_ptr = t.table.data_ptr(), t.rows.data_ptr()
            t.ring = ops.PinnedRing((t.rows,), 4)
        self._table, self._accum = t, None
        return t

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
        """Host half of step(): step counts and the per-call rows of every group, copied to the device on the current stream.
        `early` names parameters whose update will be launched by launch_early() (once their gradient is final, on any stream
        ordered behind this call) before finish() updates the rest.  Every parameter's `.grad` must already be the tensor its
        gradient WILL be in (static gradient buffers): the kernel reads it only when it is launched."""
        self._pending = self._prepare(early, True)

    def _prepare(self, early, contribute: bool):
        """What finish() will launch, or None for nothing: one micro-step or plain step (`contribute`) or the early close of flush().
        One pass over the table's rows, one pinned buffer, one copy."""
        if self._ema_swapped:
            raise RuntimeError("the parameters hold their averages (swap_ema() / ema_weights()): swap back before the next step")
        t = self._job_table()
        if any(p.grad is not None for p in t.cpu):
            raise _lib.AptaiHipError("aptai_amd.optim.Adam needs parameters on the MI355X (no CPU fallback)")
        if any(p.grad is not None for p in t.others):
            raise _lib.AptaiHipError("aptai_amd.optim.Adam updates contiguous fp32 parameters on the MI355X only")
        if t.n == 0:
            return None
        # averaging on: the averages exist (a copy of the parameters as they are BEFORE the first averaged update)
        ema = None if self._ema_decay is None else self._ema_tables()
        clip, acc = self._max_grad_norm, None
        if clip is not None and t.partials is None:
            if self._clip_result is None or self._clip_result.device != t.dev:
                self._clip_result = torch.zeros(3, dtype=torch.float32, device=t.dev)
            t.partials = torch.zeros(ops.grad_norm_chunks(t.numels), dtype=torch.float32, device=t.dev)
        if self._accum_steps > 1 or not contribute:
            acc = self._accumulators(t)
            if not contribute and acc.k == 0:
                return None
        # A window's mean and the global norm do not exist before the last gradient does, and the averaging launch follows EVERY
        # update of the step: in these modes every row goes to finish() and `early` is ignored (launch_early() then finds nothing to
        # do and the step is the one-launch step, bit for bit)
        plain = acc is None and clip is None and ema is None
        early_ids = {id(p) for p in early} if plain else ()
        host, = t.ring.next()
        host[:] = 0
        groups, early_rows, any_grad = [], set(), False
        params, states, seen = t.params, t.states, None if acc is None else acc.seen
        for gi, r0, r1, max_n in t.groups:
            late = hit = False
            for r in range(r0, r1):
                g = params[r].grad if contribute else None
                if g is None:
                    if seen is not None and seen[r]:
                        host[1, r, 1] = 2              # no gradient in this micro-step, but part of the window: scaled at its close
                    continue
                if g.dtype != torch.float32 or not g.is_contiguous():
                    raise _lib.AptaiHipError("aptai_amd.optim.Adam needs contiguous fp32 gradients")
                hit = True
                if seen is not None:                   # plane 1 = {gradient, mode: 1 first contribution of the window, 2 a later one}
                    host[1, r, 0] = g.data_ptr()
                    host[1, r, 1] = 2 if seen[r] else 1
                    seen[r] = True
                    continue
                st = states[r]
                st["step"] += 1
                if early_ids and id(params[r]) in early_ids:
                    host[1, r, 0] = g.data_ptr()
                    host[1, r, 1] = st["step"]
                    early_rows.add(r)
                else:
                    host[0, r, 0] = g.data_ptr()
                    host[0, r, 1] = st["step"]
                    late = True
            any_grad |= hit
            if hit and acc is None:
                groups.append((gi, r0, r1, max_n, late))
        window = None
        if acc is not None:
            if contribute:
                if not any_grad and acc.k == 0:
                    return None                        # nothing has a gradient and no window is open: nothing to do, as at N = 1
                acc.k += 1
            close = not contribute or acc.k >= self._accum_steps
            scale = 1.0 / acc.k if close else 1.0
            if close:
                # plane 0 = the accumulators as gradient pointers and the step counts of the rows that contributed to the window
                for gi, r0, r1, max_n in t.groups:
                    rows = [r for r in range(r0, r1) if seen[r]]
                    for r in rows:
                        st = states[r]
                        st["step"] += 1
                        host[0, r, 0] = acc.ptrs[r]
                        host[0, r, 1] = st["step"]
                    if rows:
                        groups.append((gi, r0, r1, max_n, True))
                acc.applied, acc.seen, acc.k = seen, [False] * t.n, 0
            # scale == 1 without a gradient (a flush() after one micro-step): the accumulators already hold the mean
            window = SimpleNamespace(ptrs_dev=acc.ptrs_dev, scale=scale, close=close, launch=any_grad or scale != 1.0)
        elif not groups:
            return None
        t.ring.send()
        return SimpleNamespace(table=t, groups=groups, clip=clip, accum=window, ema=ema, early=early_rows if plain else None)

    def _launch(self, t, gi: int, plane: int, r0: int, r1: int, max_n: int, coef, stream: int) -> None:
        """The Adam launch over rows [r0, r1) of the table, their gradients multiplied by the device scalar `coef` if there is one."""
        group = self.param_groups[gi]
        b1, b2 = group["betas"]
        args = (*_addr(t, plane, r0), r1 - r0, max_n, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                float(group["weight_decay"]))
        if coef is None:
            _lib.call("aptai_adam_multi", *args, stream)
        else:
            ops.adam_multi_scaled(*args, coef, stream)

    @torch.no_grad()
    def launch_early(self, params, stream=None) -> None:
        """Update `params` (named in prepare(early=...)) now, on `stream`: one launch per parameter group over the row range that
        spans them (rows in between that were not named `early` carry no gradient pointer in this plane and are skipped).  A row
        in between that WAS named `early` but is not one of `params` would be updated now, with a gradient that may not be final,
        and again by its own call: that is refused before anything is launched."""
        stream = stream or torch.cuda.current_stream()
        pend = self._pending
        if pend is None or pend.early is None:
            return
        t, ids, spans = pend.table, {id(p) for p in params}, []
        for gi, r0, r1, _, _ in pend.groups:
            rows = [r for r in range(r0, r1) if id(t.params[r]) in ids]
            if not rows:
                continue
            lo, hi = min(rows), max(rows) + 1
            for r in range(lo, hi):
                if r in pend.early and id(t.params[r]) not in ids:
                    at = [[q is t.params[x] for q in self.param_groups[gi]["params"]].index(True) for x in (r, lo, hi - 1)]
                    raise RuntimeError(f"launch_early(): parameter {at[0]} of group {gi} was named `early` in prepare() but is not "
                                       f"among this call's parameters, whose rows span parameters {at[1]} to {at[2]} of the group: "
                                       f"it would be updated twice")
            spans.append((gi, lo, hi))
        for gi, lo, hi in spans:
            self._launch(t, gi, 1, lo, hi, max(t.numels[lo:hi]), None, stream.cuda_stream)

    @torch.no_grad()
    def finish(self, stream=None) -> None:
        """Update every parameter that has a gradient and was not named `early`."""
        stream = (stream or torch.cuda.current_stream()).cuda_stream
        pend, self._pending = self._pending, None
        acc = None if pend is None else pend.accum
        self.last_step_updated = self._accum_steps == 1 if acc is None else acc.close
        for plan in self._plans:                    # the copies of every parameter that had a gradient are fresh now;
            plan.optimizer_synced = True            # parameters without one did not move (nor did any inside a window)
        if pend is None:
            return
        t = pend.table
        if acc is not None:
            if acc.launch:
                ops.grad_accum_multi(*_addr(t, 1), acc.ptrs_dev.data_ptr(), t.n, t.max_n, acc.scale, stream)
            if not acc.close:
                return
        coef = None
        if pend.clip is not None:
            # here, not in prepare(): every gradient is final now (and, under data parallelism, already averaged: the norm is that
            # of the averaged gradient and the same on every rank).  Two norm launches, then the groups' Adam launches read the
            # coefficient from the device on the same stream
            ops.grad_sqnorm_multi(*_addr(t, 0), t.n, t.max_n, t.partials, self._clip_result, pend.clip, stream)
            coef = self._clip_result[1:2]
        for gi, r0, r1, max_n, late in pend.groups:
            if late:
                self._launch(t, gi, 0, r0, r1, max_n, coef, stream)
        if pend.ema is not None and pend.groups and self._ema_decay is not None:
            # ONE launch over the rows of all groups, behind every Adam launch of this call on the same stream
            self._ema_updates += 1
            ops.ema_multi(t.table_ptr, pend.ema.ptrs_dev.data_ptr(), t.n, t.max_n,
                          1.0 - ema_decay_at(self._ema_updates, self._ema_decay, self.ema_warmup), stream)

    @torch.no_grad()
    def flush(self) -> bool:
        """Close the open window now: the update applies the mean over the micro-steps the window holds (a remainder at the end of an
        epoch).  Returns whether an update happened; with no window open it launches nothing."""
        if self.micro_step == 0:
            self.last_step_updated = False
            return False
        self._pending = self._prepare((), False)
        self.finish()
        return True

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
        self._table = None                          # the moment buffers were replaced: rebuild the job table
        self._accum = None                          # an open window is discarded with it


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
