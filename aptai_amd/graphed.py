"""hipGraph-captured APTAI train step (HIP streams + graphs instead of a tracing compiler).

The eager drop-in loop (``model(epoch, **batch)``; ``loss.backward()``; ``optimizer.step()``) issues ~340 kernel
launches per step from Python and autograd callbacks; that, not the GPU, sets its step time (13.7 ms against 10.4 ms of kernels).  ``GraphedAPTAIStep`` captures
the same kernels, through the same C ABI and the same fwd/bwd implementations the autograd path uses, into SEGMENT
graphs:

    prep (bf16 weight copies) | conv stack + encoder front | layer i forward ... | heads fwd+bwd | layer i backward ... | front bwd

and replays them (~30 ``hipGraphLaunch`` per step).  Host-side randomness keeps the reference's semantics:
 * LayerDrop (HF:701-703 / 774-776): a dropped layer's two graphs are simply not replayed (its activations / gradients are
   forwarded by one device copy) and its parameters get ``grad = None`` that step, exactly like eager;
 * SpecAugment (HF:101-217): the span mask is sampled by a kernel at the head of the front segment (ops.spec_augment_mask:
   HF's span-count rule, fresh spans on every replay through the salted seed) - no host copy, no synchronisation; with
   ``mask_feature_prob > 0`` a second launch of the same sampler draws the mask along the hidden axis into ``runner.feat``;
 * dropout: kernels XOR a per-step device salt into their counter-RNG seeds (``aptai_set_seed_salt``), so every replay
   draws fresh masks while the forward and backward of one step regenerate identical ones.
The optimiser step is issued eagerly after the last segment (aptai_amd.optim.Adam: one launch per parameter group; or any
torch optimiser).  Nothing in a step synchronises host and device: the host words a step sends (salt, frame bounds, a host
batch) travel through ``ops.PinnedRing``.  ``_CapturingRunner`` holds what this runner shares with ``GraphedForceStep``: capture
stream, salt and its binding, and the way back to the eager loop.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib, ops
from .wav2vec2 import _FEATURE_MASK_STREAM, _LAYER_STREAM_BASE, _TIME_MASK_STREAM, _FinalLNImpl, _FrontImpl, _LayerImpl, _seed


# stream handle -> the device tensor whose two words that stream's kernels XOR into their dropout seeds (kept alive here for
# as long as the library holds the pointer)
_SALTS: Dict[int, torch.Tensor] = {}


def _bind_salt(stream_handle: int, salt: torch.Tensor) -> None:
    _SALTS[stream_handle] = salt
    _lib.call("aptai_set_seed_salt", stream_handle, salt.data_ptr())


def _unbind_salt(stream_handle: int) -> None:
    _lib.call("aptai_set_seed_salt", stream_handle, None)
    _lib.call("aptai_set_frame_bounds", stream_handle, None)
    _SALTS.pop(stream_handle, None)
    _BOUNDS.pop(stream_handle, None)


# stream handle -> the device tensor with that stream's frame bounds {conv0 GroupNorm frame count, FIR frame bound}
_BOUNDS: Dict[int, torch.Tensor] = {}


def _bind_bounds(stream_handle: int, bounds: torch.Tensor) -> None:
    _BOUNDS[stream_handle] = bounds
    _lib.call("aptai_set_frame_bounds", stream_handle, bounds.data_ptr())


class _CapturingRunner:
    """What the two capturing runners share: the capture stream, the per-step dropout salt bound to it, and the way back."""

    def _init_capture(self, dev, salt_seed: int) -> None:
        # the per-step salt travels through a small ring of pinned buffers.  It is bound to THIS runner's capture stream
        # (include/aptai_hip.h: no process-global state); the module-level registry keeps the two words alive until the binding
        # is cleared, whatever happens to the runner object
        self.salt = torch.zeros(2, device=dev, dtype=torch.int32)
        self._salt_ring = ops.PinnedRing((self.salt,), 4)
        self._salt_gen = np.random.RandomState(salt_seed)
        self._cap_stream = torch.cuda.Stream(device=dev)
        _bind_salt(self._cap_stream.cuda_stream, self.salt)

    def _next_salt(self) -> None:
        buf, = self._salt_ring.next()
        buf[:] = self._salt_gen.randint(-2 ** 31, 2 ** 31 - 1, size=2).astype(np.int32)
        self._salt_ring.send()

    def _unbind(self) -> bool:
        """Drops the salt and bounds bindings of the capture stream; False when that had been done already."""
        if getattr(self, "_cap_stream", None) is None:
            return False
        _unbind_salt(self._cap_stream.cuda_stream)
        self._cap_stream = None
        return True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        # a runner dropped without close() must not leave the library a pointer into a freed tensor; the model's weight
        # cache is left alone here (a newer runner of the same model may own it by now)
        try:
            self._unbind()
        except Exception:               # noqa: BLE001 - interpreter shutdown
            pass


class GraphedAPTAIStep(_CapturingRunner):
    def __init__(self, model, optimizer: torch.optim.Optimizer, batch: Dict[str, torch.Tensor], reducer=None):
        assert model.training, "call model.train() first"
        self.model, self.opt, self.reducer = model, optimizer, reducer
        # data parallel: gradients are averaged per graph segment (dp.GradGroupReducer), overlapped with the next segment
        self.group_reducer = None
        if reducer is not None and getattr(reducer, "world", 1) > 1:
            from .dp import GradGroupReducer
            self.group_reducer = GradGroupReducer(comm_dtype=reducer.comm_dtype, process_group=reducer.group)
        w = model.wav2vec2
        self.w, self.cfg = w, w.config
        cfg = self.cfg
        dev = next(model.parameters()).device
        self.dev = dev
        # the models share the segments and differ in their task head (task_heads.py): APTAI (regression + frame classification heads,
        # models/aptai.py) and Wav2Vec2_PR (CTC head, models/w2v2_pr.py).  A trainable feature encoder (the recogniser's fine-tuning,
        # train/train_phoneme_recognizer.py) adds its backward to the front-backward segment.
        self.head = model.task_head
        self.train_conv = any(p.requires_grad for p in w.feature_extractor.parameters())
        # ---- static inputs
        self.audio = batch[self.head.audio_key].float().contiguous().clone()
        B, S = self.audio.shape
        self.g = w._geometry(B, S)
        g = self.g
        self.lens_i32 = torch.zeros(B, device=dev, dtype=torch.int32)
        self.spec = torch.zeros((B, g.T), device=dev, dtype=torch.uint8)
        # SpecAugment along the hidden axis (mask_feature_prob): a static [B][H] mask and the sampler's constant row lengths (= H);
        # None, and nothing more captured, when it is off
        self.feat = self.feat_lens = None
        if cfg.apply_spec_augment and cfg.mask_feature_prob > 0:
            ops.feature_mask_span_check(cfg.hidden_size, cfg.mask_feature_prob, cfg.mask_feature_length, cfg.mask_feature_min_masks)
            self.feat = torch.zeros((B, cfg.hidden_size), device=dev, dtype=torch.uint8)
            self.feat_lens = torch.full((B,), cfg.hidden_size, device=dev, dtype=torch.int32)
        self.targets = self.head.static_targets(model, g, batch, dev)         # name -> static buffer: the target arguments of head.state
        self._init_capture(dev, 0xC0FFEE + w.base_seed)
        # frame bounds of the batch inside the captured shape (BucketedGraphedStep feeds shorter batches): by default the shape itself
        self.bounds = torch.tensor([g.Tl[0], g.T], device=dev, dtype=torch.int32)
        self._bounds_ring = ops.PinnedRing((self.bounds,), 4)
        self._bounds_host = (g.Tl[0], g.T)
        # what head.set_batch writes; ring: pinned staging of host batches, made on the first one
        self.static = SimpleNamespace(cfg=cfg, g=g, audio=self.audio, lens=self.lens_i32, targets=self.targets, ring=None)
        _bind_bounds(self._cap_stream.cuda_stream, self.bounds)
        self.set_batch(batch)
        # one eager step first: allocates every persistent scratch buffer, loads the code objects and sets the kernel
        # attributes outside of stream capture
        if w._cache_mode == "frozen":                            # another runner of this model froze the cache: the eager step rebuilds
            w._cache_mode = None
        model.zero_grad(set_to_none=True)
        model(*self.head.forward_args, **batch)["loss"].backward()
        model.zero_grad(set_to_none=True)
        try:
            self._capture()
        finally:
            ops.ln_defer_end()                 # whatever happened during capture, eager LayerNorm backwards reduce their own partials again

    # ------------------------------------------------------------------ inputs
    def set_batch(self, batch: Dict[str, torch.Tensor]) -> None:
        """Copies a batch (the collate_fn's dict, host or device tensors) into the static input buffers of the graphs."""
        self.head.set_batch(self.static, batch)

    def set_bounds(self, conv0_frames: int, frames: int) -> None:
        """Frame bounds of the NEXT step's batch inside the captured shape (see aptai_set_frame_bounds): how many first-conv-layer
        frames count for the GroupNorm statistics and where the low-pass filter's zero padding begins.  No synchronisation (the
        two words travel through a ring of pinned buffers)."""
        if (conv0_frames, frames) == self._bounds_host:
            return
        buf, = self._bounds_ring.next()
        buf[0], buf[1] = int(conv0_frames), int(frames)
        self._bounds_ring.send()
        self._bounds_host = (conv0_frames, frames)

    def _host_randomness(self):
        """A fresh salt for the step (the SpecAugment mask is sampled by a kernel inside the front segment from the same salt) and
        LayerDrop's choice of the layers that run."""
        cfg = self.cfg
        self._next_salt()
        keep = [True] * cfg.num_hidden_layers
        if cfg.layerdrop > 0:
            keep = [float(torch.rand([], generator=self.w._layerdrop_gen)) >= cfg.layerdrop for _ in keep]
        return keep

    # ------------------------------------------------------------------ capture
    def _capture(self):
        # fault injection for the multi-rank fallback rehearsal (bench.py, tests/test_gpu_bench.py): "1" = every rank,
        # "rank<k>" = that rank only.  Placed here, after the constructor's eager step, where a real capture failure would occur.
        inject = os.environ.get("APTAI_GRAPH_FAIL_CAPTURE")
        if inject and inject in ("1", f"rank{os.environ.get('RANK', '0')}"):
            raise RuntimeError("APTAI_GRAPH_FAIL_CAPTURE is set")
        model, w, cfg, g = self.model, self.w, self.cfg, self.g
        L = cfg.num_hidden_layers
        pool = torch.cuda.graph_pool_handle()
        seed = _seed(w.base_seed, 0xABCD)
        mk = torch.cuda.CUDAGraph
        torch.cuda.synchronize()

        # -- prep: every bf16 compute copy, rebuilt from the fp32 parameters on each replay
        w._cache.clear()
        w._cache_mode = "build"
        w._layer_plan()                                      # persistent copies + job table exist before capture
        w._cache_mode = None
        w._refresh_layer_copies(force=True)                  # copies valid before the first replay whoever refreshes them later
        w._cache_mode = "build"
        torch.cuda.synchronize()
        if not self.train_conv:
            w._conv_weights()                                # frozen feature encoder: its bf16 weight copies are built once, here
            torch.cuda.synchronize()
        self.g_prep = mk()
        with torch.cuda.graph(self.g_prep, pool=pool, stream=self._cap_stream, capture_error_mode=ops.CAPTURE_MODE):
            if self.train_conv:
                w._conv_weights()
            if not getattr(self.opt, "publishes_copies", False):     # else the optimiser kernel refreshes the copies itself
                w._refresh_layer_copies(force=True)
            self.lw = [w._layer_weights(i) for i in range(L)]
            w._proj_weight()
            w._posconv_weights()
        w._cache_mode = "frozen"

        # -- front: conv stack (frozen) + projection + masking + positional conv (+ LN)
        self.fparams = w._front_params(with_embed=True)
        embed = self.fparams.embed
        self.front = _FrontImpl(cfg, g, self.lens_i32, self.spec if embed is not None else None, True, _seed(seed, 1), w,
                                feat=self.feat)
        self.g_front = mk()
        with torch.cuda.graph(self.g_front, pool=pool, stream=self._cap_stream, capture_error_mode=ops.CAPTURE_MODE):
            if embed is not None and cfg.apply_spec_augment and cfg.mask_time_prob > 0:
                ops.spec_augment_mask(self.lens_i32, g.B, g.T, cfg.mask_time_prob, cfg.mask_time_length, cfg.mask_time_min_masks,
                                      _seed(seed, _TIME_MASK_STREAM), out=self.spec)        # fresh spans on every replay (salted seed)
            if self.feat is not None:                                        # a seed stream of its own: independent of the time mask
                ops.spec_augment_mask(self.feat_lens, g.B, cfg.hidden_size, cfg.mask_feature_prob, cfg.mask_feature_length,
                                      cfg.mask_feature_min_masks, _seed(seed, _FEATURE_MASK_STREAM), out=self.feat)
            feats, self.sv_conv = w._conv_forward(self.audio, g, save=self.train_conv)
            (h,), self.s_front = self.front.fwd(feats, self.fparams, True)
        self.X = [h]

        # -- layers forward
        self.impl, self.s_layer, self.g_fwd, self.lparams = [], [], [], []
        for i in range(L):
            wt, lin = self.lw[i]
            impl = _LayerImpl(cfg, g, self.lens_i32, wt, True, _seed(seed, _LAYER_STREAM_BASE + i))
            params = w._layer_ln_params(i) + lin
            gr = mk()
            with torch.cuda.graph(gr, pool=pool, stream=self._cap_stream, capture_error_mode=ops.CAPTURE_MODE):
                (y,), s = impl.fwd(self.X[i], params, True)
            self.impl.append(impl); self.s_layer.append(s); self.g_fwd.append(gr); self.lparams.append(params)
            self.X.append(y)

        # -- tail: [final LN] + heads forward + loss + heads backward + [final LN backward]
        self.fin = _FinalLNImpl(cfg, g) if cfg.do_stable_layer_norm else None
        self.hparams = self.head.params(model)
        self.st_heads = self.head.state(model, g, (seed,), True, **self.targets)
        # data parallel: the loss backward inside the tail graph reads the global valid counts / world from this static buffer
        self.loss_norm = getattr(model, "dp_loss_norm", None) if self.head.global_loss_norm else None
        if self.loss_norm is not None:
            self.st_heads.norm_scalars = self.loss_norm.buffer(self.dev)
        # single GPU: the ~24 LayerNorm parameter-gradient reductions of the backward pass (one 4.8 us launch + a kernel boundary each)
        # are collected here and replayed as ONE launch behind the front-end backward; nothing reads them before the optimiser.
        # Data parallel keeps them per call: a layer's gradients leave for the all-reduce right after its segment.
        self._ln_jobs = ops.ln_defer_begin() if (self.group_reducer is None and os.environ.get("APTAI_LN_DEFER", "1") != "0") else None
        self.g_tail = mk()
        with torch.cuda.graph(self.g_tail, pool=pool, stream=self._cap_stream, capture_error_mode=ops.CAPTURE_MODE):
            hl = self.X[L]
            if self.fin is not None:
                (hl,), s_fin = self.fin.fwd(hl, [w.encoder.layer_norm.weight, w.encoder.layer_norm.bias], True)
            self.outs, s_heads = self.head.fwd(hl, self.hparams, self.st_heads)
            dh, *hgrads = self.head.bwd(s_heads, self.st_heads, self.hparams, hl, None)
            fin_grads = []
            if self.fin is not None:
                dh, fin_grads = self.fin.bwd(s_fin, (dh,), True)
        self.dX: List[Optional[torch.Tensor]] = [None] * (L + 1)
        self.dX[L] = dh
        self.grads: Dict[torch.nn.Parameter, torch.Tensor] = {}
        for p, gt in zip(self.hparams, hgrads):
            self.grads[p] = gt
        if self.fin is not None:
            self.grads[w.encoder.layer_norm.weight], self.grads[w.encoder.layer_norm.bias] = fin_grads

        # -- layers backward (reverse capture order = replay order)
        self.g_bwd = [None] * L
        self.layer_grads = [None] * L
        for i in range(L - 1, -1, -1):
            gr = mk()
            with torch.cuda.graph(gr, pool=pool, stream=self._cap_stream, capture_error_mode=ops.CAPTURE_MODE):
                dx, pg = self.impl[i].bwd(self.s_layer[i], (self.dX[i + 1],), True)
            self.g_bwd[i] = gr
            self.dX[i] = dx
            self.layer_grads[i] = list(zip(self.lparams[i], pg))

        # -- front backward
        self.g_front_bwd = mk()
        with torch.cuda.graph(self.g_front_bwd, pool=pool, stream=self._cap_stream, capture_error_mode=ops.CAPTURE_MODE):
            dfeats, fg = self.front.bwd(self.s_front, (self.dX[0],), self.train_conv)
            conv_grads = w._conv_backward(self.sv_conv, g, dfeats.contiguous())[1] if self.train_conv else []
        for p, gt in zip(self.fparams, fg):
            if p is not None and gt is not None:
                self.grads[p] = gt
        for p, gt in zip(w._conv_params(), conv_grads):
            self.grads[p] = gt
        self.g_ln = None
        if self._ln_jobs is not None:
            ops.ln_defer_end()
            if self._ln_jobs:
                torch.cuda.synchronize()
                self._ln_table, n_jobs, max_cols = ops.ln_defer_table(self._ln_jobs)        # host-to-device copy: outside capture
                torch.cuda.synchronize()
                self.g_ln = mk()
                with torch.cuda.graph(self.g_ln, pool=pool, stream=self._cap_stream, capture_error_mode=ops.CAPTURE_MODE):
                    ops.ln_finalize_multi(self._ln_table, n_jobs, max_cols)
        # optimiser under the backward pass (step()): the parameters of layer i whose gradients are final when its backward segment ends
        self.adam_overlap = (self.group_reducer is None and hasattr(self.opt, "launch_early")
                             and os.environ.get("APTAI_ADAM_OVERLAP", "0") != "0")
        self._o_stream = torch.cuda.Stream(device=self.dev) if self.adam_overlap else None
        self._early_params = [[p for k, (p, _) in enumerate(self.layer_grads[i]) if p.requires_grad and (k >= 4 or self.g_ln is None)]
                              for i in range(L)]
        # the graphs hold raw addresses of the compute copies in the model's cache: keep them alive for this runner's lifetime (a
        # second runner of the same model - another shape bucket - clears and rebuilds the cache for its own capture)
        self._keep_cache = dict(w._cache)
        torch.cuda.synchronize()

    def _assign_grads(self, keep) -> None:
        """Every trainable parameter's `.grad` = its static gradient buffer (None for a layer LayerDrop skipped this step)."""
        for p, gt in self.grads.items():
            if p.requires_grad:
                p.grad = gt
        for i in range(self.cfg.num_hidden_layers):
            for p, gt in self.layer_grads[i]:
                if p.requires_grad:
                    p.grad = gt if keep[i] else None
        if not getattr(self, "_checked", False):
            names = {id(p): n for n, p in self.model.named_parameters()}
            for p in self.model.parameters():
                if p.grad is not None and (p.grad.dtype != p.dtype or p.grad.shape != p.shape or not p.grad.is_contiguous()
                                           or p.grad.device != p.device):
                    raise RuntimeError(f"static gradient of {names[id(p)]} has dtype {p.grad.dtype} shape {tuple(p.grad.shape)} "
                                       f"contiguous={p.grad.is_contiguous()} (parameter: {p.dtype} {tuple(p.shape)})")
            self._checked = True

    # ------------------------------------------------------------------ one optimiser step
    def step(self, batch: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
        if batch is not None:
            self.set_batch(batch)
        keep = self._host_randomness()
        L = self.cfg.num_hidden_layers
        self.w._train_marker += 1                                # eval-mode weight copies built before this step are stale
        if self.loss_norm is not None:
            self.loss_norm.begin(self.st_heads.tv_tgt, self.st_heads.phn_tgt)      # travels under the encoder forward
        # Optimiser under the backward pass (APTAI_ADAM_OVERLAP=1; experiment, OFF by default; single GPU, aptai_amd.optim.Adam): a
        # layer's six weight / bias pairs are updated on a side stream as soon as its backward segment has finished - an HBM-bound
        # launch beside the next layers' matrix-bound ones.  Adam is element-wise per parameter, so WHEN a parameter is updated
        # changes no bit (tests/test_gpu_graphed.py).  Measured, interleaved on one box: 8.97 / 8.97 / 8.97 ms without, 9.15 / 9.15 /
        # 9.21 ms with - the 0.34 ms of Adam cost 0.52 ms beside the GEMMs (2.8 GB streamed through the L2s their operand panels
        # live in).  (The layer's LayerNorm gradients are final only after the deferred finalize launch: they stay with finish().)
        overlap_opt = self.adam_overlap
        if overlap_opt:
            self._assign_grads(keep)
            early = [self._early_params[i] if keep[i] else [] for i in range(L)]
            self.opt.prepare(early=[p for lst in early for p in lst])
        self.g_prep.replay()
        self.g_front.replay()
        for i in range(L):
            if keep[i]:
                self.g_fwd[i].replay()
            else:
                self.X[i + 1].copy_(self.X[i])
        red = self.group_reducer
        if self.loss_norm is not None:
            self.loss_norm.scalars()                 # counts launched at the top of the step have arrived
        self.g_tail.replay()
        if red is not None:
            red.launch("heads", self._head_front_grads()[0])
        cur = torch.cuda.current_stream(self.dev) if overlap_opt else None
        for i in range(L - 1, -1, -1):
            if keep[i]:
                self.g_bwd[i].replay()
                if overlap_opt and early[i]:
                    self._o_stream.wait_stream(cur)
                    self.opt.launch_early(early[i], self._o_stream)
                if red is not None:            # layer i's gradients travel while layer i-1's backward runs
                    red.launch(("layer", i), self._layer_grad_tensors(i))
            else:
                self.dX[i].copy_(self.dX[i + 1])
        self.g_front_bwd.replay()
        if self.g_ln is not None:
            self.g_ln.replay()                 # every LayerNorm dgamma / dbeta of the step in one launch
        if red is not None:
            red.launch("front", self._head_front_grads()[1])
            red.finish()
        if not overlap_opt:
            self._assign_grads(keep)
        if overlap_opt:
            cur.wait_stream(self._o_stream)    # (the next step's prep segment reads what these launches wrote)
            self.opt.finish()
        else:
            self.opt.step()
        return self.head.result(self.outs, self.g, self.hparams)

    def plan_groups(self):
        """[(name, gradient elements)] of the per-segment gradient groups in the order step() hands them to dp.GradGroupReducer
        (heads, layers L-1 .. 0, front): input of dp.collective_plan."""
        heads, front = self._head_front_grads()
        out = [("heads", sum(t.numel() for t in heads))]
        for i in range(self.cfg.num_hidden_layers - 1, -1, -1):
            out.append((f"layer{i}", sum(t.numel() for t in self._layer_grad_tensors(i))))
        out.append(("front", sum(t.numel() for t in front)))
        return out

    def _head_front_grads(self):
        """(heads, front): the gradient buffers of the trainable parameters outside the layers, split by the segment that writes them."""
        heads, front = [], []
        for p, gt in self.grads.items():
            if p.requires_grad:
                (heads if any(p is q for q in self.hparams) else front).append(gt)
        return heads, front

    def _layer_grad_tensors(self, i: int) -> List[torch.Tensor]:
        """Distinct gradient buffers of layer i (the q/k/v weight and bias gradients are row slices of one buffer each)."""
        out, seen = [], set()
        for p, gt in self.layer_grads[i]:
            if not p.requires_grad:
                continue
            base = gt._base if gt._base is not None else gt
            if base.data_ptr() not in seen:
                seen.add(base.data_ptr())
                out.append(base)
        return out

    def close(self):
        """Back to the eager loop: drop the salt binding of the capture stream and the frozen weight cache."""
        if self._unbind():
            self.w._cache_mode = None
            self.w._cache.clear()


class BucketedGraphedStep:
    """hipGraph replay for REAL batches.  The reference's collate pads every batch to ITS OWN longest utterance
    (train/train_aptai.py:268-285, train/train_phoneme_recognizer.py:224-239), so the tensor shapes change from step to step,
    while a captured graph has one shape.  This wrapper keeps a small cache of GraphedAPTAIStep runners, one per (batch size, BUCKET
    length): a batch is zero-padded up to the next bucket, fed to that bucket's graphs (captured on first use, sharing the model's
    parameters, persistent weight copies and the optimiser), and the outputs are cut back to the batch's own frame count.

    Results equal the eager loop on the un-bucketed batch: every length-dependent quantity is dynamic inside the graphs -
    per-utterance frame counts travel as device tensors (attention key mask, padded-frame zeroing, SpecAugment span counts, loss
    masks, CTC lengths), and the two places where the reference sees the batch's PADDED length (GroupNorm statistics of the first
    conv layer over all frames of the collated batch; the 'same' zero padding of LowPassFilterLayer) read per-step frame bounds
    (aptai_set_frame_bounds).  Extra frames of the bucket are padded frames like the reference's own: zeroed, masked as keys, outside
    every loss, zero gradient.  288 GB of HBM hold a dozen buckets of saved activations (~3.5 GB each at 16 x 10 s)."""

    DEFAULT_SECONDS = (1, 2, 3, 4, 5, 6, 8, 10, 12, 15, 20, 25, 30)

    def __init__(self, model, optimizer, bucket_samples=None, reducer=None, label_bucket: int = 32, max_runners: int = 8, log=None):
        self.model, self.opt, self.reducer = model, optimizer, reducer
        # Every runner holds a capture stream with a salt and a bounds slot (64 of each in the library, csrc/runtime.hip) and several GB of
        # saved activations and graph pools; a real corpus spans 13 length buckets x several label widths (+ a short last batch), so the
        # cache is bounded: beyond `max_runners` the least recently used runner is closed (its graphs are re-captured if its shape returns).
        self.max_runners, self.log, self.evictions = max(1, int(max_runners)), log, 0
        self.head = model.task_head
        self.buckets = sorted(bucket_samples) if bucket_samples else [16000 * s for s in self.DEFAULT_SECONDS]
        self.label_bucket = label_bucket
        self.runners: Dict[tuple, GraphedAPTAIStep] = {}
        self.w = model.wav2vec2

    def bucket_of(self, S: int) -> int:
        for b in self.buckets:
            if b >= S:
                return b
        return -(-S // 16000) * 16000                      # longer than every bucket: whole seconds

    def step(self, batch: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        B, S = batch[self.head.audio_key].shape
        Sb = self.bucket_of(S)
        g_s, g_b = self.w._geometry(B, S), self.w._geometry(B, Sb)
        padded = self.head.pad_batch(batch, Sb, g_b.T, self.label_bucket)
        key = (B, Sb) + self.head.cache_key(padded)
        r = self.runners.pop(key, None)
        if r is None:
            while len(self.runners) >= self.max_runners:
                old_key = next(iter(self.runners))              # dicts keep insertion order: the first key is the least recently used
                self.runners.pop(old_key).close()
                self.evictions += 1
                if self.log is not None:
                    self.log(f"[graphed] closed the runner of shape {old_key} (cache of {self.max_runners} is full)")
            dev = next(self.model.parameters()).device
            r = GraphedAPTAIStep(self.model, self.opt, {k: v.to(dev) for k, v in padded.items()}, reducer=self.reducer)
            if self.log is not None:
                self.log(f"[graphed] captured shape {key}: {len(self.runners) + 1} runner(s), "
                         f"{torch.cuda.memory_allocated(dev) / 2 ** 30:.1f} GiB allocated")
        self.runners[key] = r                                   # (re-)inserted last = most recently used
        r.set_bounds(g_s.Tl[0], g_s.T)
        return self.head.cut(r.step(padded), g_s.T)

    def suspend(self) -> None:
        """Before an EAGER phase on the same model (validation between epochs): un-freeze the model's compute-copy cache so that
        eager forwards rebuild their copies from the current parameters.  The captured graphs keep their own copies (refreshed by
        their prep segment on every replay), so the next step() needs nothing."""
        self.w._cache_mode = None
        self.w._cache.clear()

    def close(self):
        for r in self.runners.values():
            r.close()
        self.runners = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class GraphedForceStep(_CapturingRunner):
    """hipGraph runner for the Force_APTAI train step (models/force_aptai.py:80-178, train/train_force_aptai.py:392-531): TWO graphs,

        encoder (frozen recogniser in inference mode + best-path decode, on a side stream)  |  heads forward + loss + heads backward

    replayed one batch apart: while the heads of batch n replay on the caller's stream, the encoder of batch n+1 (handed to step() as
    `next_batch`, or the same batch again) replays on the side stream.  The encoder graph, its stream and the hand-over are the model's
    (force_aptai.EncoderAhead, shared with the eager loop's prefetch; close() leaves them to it).  Same kernels and the same two Python
    functions (task_heads.ForceHead.fwd / .bwd) as the eager autograd path; dropout draws fresh masks per replay through the per-stream
    salt; nothing synchronises host and device (`lists()` makes the Python lists of the reference's return value on demand).  The
    optimiser step is issued eagerly after the heads graph.  The captured heads keep the ARGMAX read-out of `pred_frame_phns` whatever
    `Force_APTAI.alignment_readout` says (the monotonic read-out is an eager-path option)."""

    def __init__(self, model, optimizer, batch: Dict[str, torch.Tensor]):
        from .force_aptai import Force_APTAI
        assert isinstance(model, Force_APTAI) and model.training, "a Force_APTAI model in train() mode"
        if getattr(model, "dp_loss_norm", None) is not None:
            raise NotImplementedError("GraphedForceStep is single-process (the eager step carries the DP loss normalisation)")
        self.model, self.opt = model, optimizer
        dev = next(model.parameters()).device
        self.dev = dev
        self._tracks = [k for k in batch if k not in ("audio_inputs", "audio_lengths", "phn_frames_49hz", "phoneme_labels")]
        w = model.w2v2_pr.wav2vec2
        B, S = batch["audio_inputs"].shape
        self.g = w._geometry(B, S)
        g = self.g
        n_tv = model.rnn.linear[3].weight.shape[0]
        self.tv_tgt = torch.zeros((B, g.T, n_tv), device=dev, dtype=torch.float32)
        self._init_capture(dev, 0xF0CE + w.base_seed)
        # one eager step: scratch buffers, code objects, weight copies
        model.zero_grad(set_to_none=True)
        model(0, **batch)["loss"].backward()
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        # ---- encoder pass: the model's own (force_aptai.EncoderAhead), captured now for this batch shape
        e = model.encoder_ahead.capture(batch["audio_inputs"].float(), batch["audio_lengths"]).out
        # ---- heads graph: its own copies of the encoder outputs (the next encoder replay overwrites the graph-owned ones)
        self.h_ac, self.h_ids, self.h_nlen, self.h_fl = (torch.empty_like(t) for t in (e.ac, e.ids, e.nlen, e.frame_lens))
        self.h_nfull = torch.empty_like(e.nlen_full)          # the uncut decoded length: what lists() checks
        self.head = model.task_head
        self.P = self.head.params(model)
        self.st = self.head.state(model, g, (w.base_seed, 0xF0), True, self.h_ids, self.h_nlen, self.h_fl, self.tv_tgt)
        self.st.readout = "argmax"
        self.g_heads = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.g_heads, stream=self._cap_stream, capture_error_mode=ops.CAPTURE_MODE):
            self.st.vocab_sizes = self.h_nlen + 1             # derived from a static input: recomputed on every replay
            self.outs, saved = self.head.fwd(self.h_ac, self.P, self.st)
            self.pgrads = self.head.bwd(saved, self.st, self.P, self.h_ac, None)[1:]
        torch.cuda.synchronize()
        self._ahead = None                                    # handle of the pass launched for the next step()
        self._last = batch
        self.set_batch(batch)

    # ------------------------------------------------------------------ inputs of the HEADS (targets) and of the encoder
    def set_batch(self, batch: Dict[str, torch.Tensor]) -> None:
        """Targets of the batch whose heads run in the next step()."""
        self.tv_tgt.copy_(torch.stack([batch[k] for k in self._tracks], dim=-1).float(), non_blocking=True)

    # ------------------------------------------------------------------ one optimiser step
    def step(self, batch: Optional[Dict[str, torch.Tensor]] = None, next_batch: Optional[Dict[str, torch.Tensor]] = None):
        """Heads of `batch` (default: the batch given last) + optimiser step; the encoder pass of `next_batch` (default: `batch`
        again) goes out on the side stream first.  The very first call encodes `batch` itself, and so does one whose pass ahead was
        dropped meanwhile (EncoderAhead.take: the weights were reloaded, or another caller replayed the pass)."""
        if batch is not None:
            self.set_batch(batch)
            self._last = batch
        batch = batch if batch is not None else self._last
        ahead, into = self.model.encoder_ahead, (self.h_ac, self.h_ids, self.h_nlen, self.h_fl, self.h_nfull)
        if self._ahead is None or ahead.take(self._ahead, into) is None:
            ahead.take(ahead.launch(batch["audio_inputs"].float(), batch["audio_lengths"]), into)
        nxt = next_batch if next_batch is not None else batch
        self._ahead = ahead.launch(nxt["audio_inputs"].float(), nxt["audio_lengths"])     # (a host batch is copied in)
        self._next_salt()
        self.g_heads.replay()
        for p, gt in zip(self.P, self.pgrads):
            if p.requires_grad:
                p.grad = gt                                    # (bias_ih / bias_hh of a direction share one gradient buffer)
        self.opt.step()
        return dict(self.head.result(self.outs, self.g, self.P), ids=self.h_ids, n_ids=self.h_nfull, frame_lens=self.h_fl)

    def lists(self, out) -> Dict[str, list]:
        """The Python lists of Force_APTAI.forward (pred_frame_phns, pred_ctc_phn_seq) for a step() result: the only transfers."""
        given, fl, n, table = self.model._lists((out["ids"], out["n_ids"], out["frame_lens"], None))
        fp = out["frame_phns"].cpu().numpy()
        return {"pred_frame_phns": [fp[b, :fl[b]].tolist() for b in range(self.g.B)], "pred_ctc_phn_seq": given}

    def close(self):
        if getattr(self, "_cap_stream", None) is not None:
            torch.cuda.synchronize(self.dev)
            self._unbind()
