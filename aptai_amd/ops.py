"""Tensor-level wrappers over the C ABI (include/aptai_hip.h).  torch is plumbing here: it owns the
device buffers and the stream; every computation is a hand-written HIP kernel in libaptai_hip.so.
All wrappers raise (no fallback) when the tensors are not on a HIP device.
"""
from __future__ import annotations

import ctypes
import math
from typing import Optional

import numpy as np
import torch

from . import _lib

_C = _lib.ABI.constants     # the header's enum values and #defines, under the names this module has always exported
EPI_BIAS = _C["APTAI_EPI_BIAS"]
EPI_GELU = _C["APTAI_EPI_GELU"]
EPI_RESIDUAL = _C["APTAI_EPI_RESIDUAL"]
EPI_DROPOUT = _C["APTAI_EPI_DROPOUT"]
EPI_DGELU = _C["APTAI_EPI_DGELU"]
EPI_ALPHA = _C["APTAI_EPI_ALPHA"]
EPI_PRE_DGELU = _C["APTAI_EPI_PRE_DGELU"]
EPI_MUL_AUX = _C["APTAI_EPI_MUL_AUX"]
EPI_RESIDUAL_F32 = _C["APTAI_EPI_RESIDUAL_F32"]
EPI_SPLIT_OUT = _C["APTAI_EPI_SPLIT_OUT"]
EPI_BIAS_ROW = _C["APTAI_EPI_BIAS_ROW"]


class GemmDesc(ctypes.Structure):
    _fields_ = _lib.ABI.structs["aptai_gemm_desc"]


class GemmPlanInfo(ctypes.Structure):
    _fields_ = _lib.ABI.structs["aptai_gemm_plan_info"]


def gemm_plan(d: GemmDesc) -> GemmPlanInfo:
    """What aptai_gemm_bf16 would launch for `d` in this process (aptai_gemm_plan: host only, no device needed); raises where
    aptai_gemm_bf16 would refuse the descriptor, with the same text."""
    info = GemmPlanInfo()
    _lib.call("aptai_gemm_plan", ctypes.byref(d), ctypes.byref(info))
    return info


# thread-local capture for every hipGraph of the package: under data parallelism the process group's watchdog thread polls its events
# while this thread captures, and in the default "global" mode a call from ANY thread can invalidate the capture
CAPTURE_MODE = "thread_local"


class ScratchPool:
    """Persistent scratch buffers that NEVER move: a buffer handed out for (purpose, device, stream, dtype, size class) is not
    replaced and not freed while the pool lives, because captured hipGraphs hold its address (a buffer that grew used to be swapped
    out from under them: the next replays read freed memory).  The size class is the next power of two at or above the request (at
    least 16 elements), so a purpose keeps at most a few dozen buffers; `exact` keeps the element count.  `stream` is whatever the
    caller keys by (the raw handle of the launch stream, or None for one buffer whatever the stream): "every consumer of a scratch
    runs on the launch stream right after its producer" only holds per stream."""

    def __init__(self):
        self._bufs = {}

    def get(self, purpose, numel: int, device, stream, dtype=torch.float32, *, exact=False, zero=False) -> torch.Tensor:
        n = int(numel) if exact else 1 << (max(int(numel), 16) - 1).bit_length()
        key = (purpose, str(device), stream, dtype, n)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = (torch.zeros if zero else torch.empty)(n, device=device, dtype=dtype)
        return t

    def buffers(self, purpose, device=None):
        """[(stream, buffer)] of one purpose (on one device), in the order they were made."""
        return [(k[2], t) for k, t in self._bufs.items() if k[0] == purpose and (device is None or k[1] == str(device))]


SCRATCH = ScratchPool()        # the package's own: split-K slabs / column-sum / LayerNorm partials of the fp32 heads, LSTM and stream-K areas
TILE_STREAMK = 257


def gemm_sk_check(device=None) -> None:
    """Raises if a bounded wait of a stream-K GEMM launch gave up since the last check (its output tile was then incomplete).
    Synchronises: call where the host waits for the device anyway (loss logging, end of an epoch, after a timed region)."""
    for st, ws in SCRATCH.buffers("sk", device):
        out = ctypes.c_int(0)
        _lib.call("aptai_gemm_sk_status", ws.data_ptr(), st, ctypes.byref(out))
        if out.value != 0:
            raise _lib.AptaiHipError("aptai_gemm_bf16 (stream-K): a wait for another workgroup's partial tile timed out; "
                                     "the output of that launch is incomplete")


class GemmProbe:
    """Brackets every aptai_gemm_bf16 launch of one operand-layout family with HIP events on the launch stream and
    accumulates (algorithmic flops, elapsed ms): bench.py's live roofline measurement of the dominant kernel."""

    def __init__(self, a_kmajor=False, b_kmajor=False, out_f32=False):
        self.key = (bool(a_kmajor), bool(b_kmajor), bool(out_f32))
        self.records = []

    def summary(self):
        torch.cuda.synchronize()
        flops = sum(f for f, _, _ in self.records)
        ms = sum(s.elapsed_time(e) for _, s, e in self.records)
        return dict(launches=len(self.records), flops=flops, ms=ms)


_probe: Optional["GemmProbe"] = None


def set_gemm_probe(p: Optional["GemmProbe"]) -> None:
    global _probe
    _probe = p


def _stream() -> int:
    # raw handle of torch's current stream; ~10x cheaper than torch.cuda.current_stream().cuda_stream, which was 0.9 ms of host
    # time per eager train step (1000+ launches)
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _dev(*ts) -> None:
    for t in ts:
        if t is not None and not t.is_cuda:
            raise _lib.AptaiHipError("aptai_amd ops need tensors on the MI355X (no CPU fallback)")


def _gemm_desc(d: "GemmDesc", a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, *, lda=None, ldb=None, out=None, ldc=None,
               a_kmajor=False, b_kmajor=False, out_f32=False, bias=None, gelu=False, residual=None, out_pre=None,
               dgelu_aux=None, alpha: Optional[float] = None, dropout_p: float = 0.0, seed: int = 0, split_k: int = 1,
               accumulate: bool = False, workspace: Optional[torch.Tensor] = None, batch=None, ldr=None, tile: int = 0,
               ldaux=None, pre_dgelu: bool = False, mul_aux=None, colscale=None, residual_f32=None, split_out=None, split_bcol=None, bias_row=None):
    """Fills one aptai_gemm_desc in place; returns (out, workspace) - the caller keeps them alive across the launch."""
    _dev(a, b, out, bias, residual, out_pre, dgelu_aux, mul_aux)
    if out is None:
        if split_out:          # exact-index mode: fp32 result written as `split_out` bf16 pieces (EPI_SPLIT_OUT); ldc in bf16 elements
            out = torch.empty((M, N * int(split_out)), device=a.device, dtype=torch.bfloat16)
        else:
            out = torch.empty((M, N), device=a.device, dtype=torch.float32 if out_f32 else torch.bfloat16)
    d.A, d.lda = a.data_ptr(), lda if lda is not None else (a.stride(0))
    d.B, d.ldb = b.data_ptr(), ldb if ldb is not None else (b.stride(0))
    d.C, d.ldc = out.data_ptr(), ldc if ldc is not None else out.stride(0)
    d.M, d.N, d.K = M, N, K
    d.a_kmajor, d.b_kmajor, d.out_f32 = int(a_kmajor), int(b_kmajor), int(out_f32)
    flags = 0
    if bias is not None:
        flags |= EPI_BIAS
        d.bias = bias.data_ptr()
    if gelu:
        flags |= EPI_GELU
    if residual is not None:
        flags |= EPI_RESIDUAL
        d.residual, d.ldr = residual.data_ptr(), residual.stride(0)
    if residual_f32 is not None:   # fp32 output += fp32 residual (the inference-only encoder's fp32 residual stream)
        _dev(residual_f32)
        flags |= EPI_RESIDUAL_F32
        d.residual, d.ldr = residual_f32.data_ptr(), residual_f32.stride(0)
    if out_pre is not None:
        d.out_pre = out_pre.data_ptr()
    if dgelu_aux is not None:
        flags |= EPI_DGELU
        d.aux, d.ldaux = dgelu_aux.data_ptr(), dgelu_aux.stride(0)
    if mul_aux is not None:        # backward partner of pre_dgelu: *= saved dropmask * gelu'(pre-activation)
        flags |= EPI_MUL_AUX
        d.aux, d.ldaux = mul_aux.data_ptr(), mul_aux.stride(0)
    if pre_dgelu:                  # out_pre receives dropmask/(1-p) * gelu'(pre-activation) instead of the pre-activation
        flags |= EPI_PRE_DGELU
    if alpha is not None:
        flags |= EPI_ALPHA
        d.alpha = alpha
    if dropout_p > 0:
        flags |= EPI_DROPOUT
        d.dropout_p, d.seed = dropout_p, seed
    if bias_row is not None:       # fp32-output launches: bias indexed by the output row (a product evaluated transposed)
        _dev(bias_row)
        flags |= EPI_BIAS_ROW
        d.bias = bias_row.data_ptr()
    if split_out:
        if out.dtype != torch.bfloat16 or not out_f32:
            raise ValueError("split_out writes bf16 pieces from an out_f32 launch")
        flags |= EPI_SPLIT_OUT
        d.split_out_pieces = int(split_out)
        d.split_out_bcol = int(split_bcol) if split_bcol is not None else int(N)
    d.flags = flags
    d.split_k, d.accumulate = split_k, int(accumulate)
    d.tile = tile if tile else _AUTO_TILE
    if tile == TILE_STREAMK:          # opt-in only: measured slower than the tile rule's choice on every hot-path shape
        # one 256 x 256 fp32 slab per CU + self-cleaning ready flags + status word, zeroed once, per STREAM: launches on one stream are
        # serialised, so they share it; another stream gets its own
        ws_sk = SCRATCH.get("sk", _lib.lib().aptai_gemm_sk_workspace_bytes(), a.device, _stream(), torch.uint8, exact=True, zero=True)
        d.sk_workspace, d.sk_workspace_bytes = ws_sk.data_ptr(), ws_sk.numel()
    if colscale is not None:       # (n_cols, factor): output columns [0, n_cols) *= factor after alpha / bias
        d.colscale_n, d.colscale = int(colscale[0]), float(colscale[1])
    if ldaux is not None:
        d.ldaux = ldaux
    if ldr is not None:
        d.ldr = ldr
    if batch is not None:
        # batch = dict(outer=, inner=, a=(so,si), b=(so,si), c=(so,si), bias=(so,si), res=(so,si), aux=(so,si))
        d.batch_outer, d.batch_inner = batch.get("outer", 1), batch.get("inner", 1)
        for key, field in (("a", "batch_stride_a"), ("b", "batch_stride_b"), ("c", "batch_stride_c"),
                           ("bias", "batch_stride_bias"), ("res", "batch_stride_res"), ("aux", "batch_stride_aux")):
            so, si = batch.get(key, (0, 0))
            getattr(d, field)[0], getattr(d, field)[1] = so, si
    if out_f32 and (split_k > 1 or accumulate):
        need = _lib.lib().aptai_gemm_workspace_bytes(M, N, split_k)
        if workspace is None or workspace.numel() * workspace.element_size() < need:
            workspace = torch.empty(need, device=a.device, dtype=torch.uint8)
        d.workspace, d.workspace_bytes = workspace.data_ptr(), workspace.numel() * workspace.element_size()
    return out, workspace


_AUTO_TILE = 0        # what `tile = 0` means to _gemm_desc: 0 = the library's rule


class auto_tile:
    """Context: GEMMs that leave the tile to the library run with `tile` instead (0 restores the rule).  Force_APTAI captures its side-stream
    encoder pass under auto_tile(128): a 256 x 256 workgroup owns a whole CU (128 KiB of LDS, 2 x 240 registers per SIMD), so while such a
    launch runs the cooperative BiLSTM workgroups of the heads cannot start beside it - the pipelined step measured 7.70 ms with 128-row
    tiles in the encoder against 8.1-8.4 ms with the rule's 256-row launches, although the encoder alone is slower that way."""

    def __init__(self, tile: int):
        self.tile = int(tile)

    def __enter__(self):
        global _AUTO_TILE
        self.prev, _AUTO_TILE = _AUTO_TILE, self.tile
        return self

    def __exit__(self, *exc):
        global _AUTO_TILE
        _AUTO_TILE = self.prev
        return False


def gemm(a: torch.Tensor, b: torch.Tensor, M: int, N: int, K: int, **kw) -> torch.Tensor:
    """C[M,N] = rowop(A)[M,K] . colop(B)[N,K]^T.  See aptai_gemm_bf16 in include/aptai_hip.h (keywords: _gemm_desc)."""
    d = GemmDesc()
    out, _ws_keep = _gemm_desc(d, a, b, M, N, K, **kw)
    pr = _probe
    timed = pr is not None and pr.key == (bool(d.a_kmajor), bool(d.b_kmajor), bool(d.out_f32)) and not torch.cuda.is_current_stream_capturing()
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    _lib.call("aptai_gemm_bf16", ctypes.byref(d), _stream())
    if timed:
        e1.record()
        batch = kw.get("batch")
        nb = (batch.get("outer", 1) * batch.get("inner", 1)) if batch else 1
        pr.records.append((2.0 * M * N * K * nb, e0, e1))
    return out


def gemm_grouped(problems) -> list:
    """One launch for up to 8 independent GEMMs of one operand layout (aptai_gemm_bf16_grouped).
    problems: iterable of (a, b, M, N, K, kwargs-dict) with the keywords of gemm(); returns the outputs in order.
    A problem whose dict carries rowsum=True or rowsum=<fp32 tensor [M]> (both operands K-major, fp32 output) also yields the fp32 vector [M] of the column sums of
    its K-major A (aptai_gemm_bf16_grouped_rowsum) - the bias gradient beside a weight gradient dY^T X; these vectors follow the outputs
    in the returned list, in problem order."""
    problems = list(problems)
    descs = (GemmDesc * len(problems))()
    outs, keep, sums = [], [], []
    rs_ptrs = (ctypes.c_void_p * len(problems))()
    flops = 0.0
    for i, (d, (a, b, M, N, K, kw)) in enumerate(zip(descs, problems)):
        kw = dict(kw)
        want_sum = kw.pop("rowsum", False)
        out, ws = _gemm_desc(d, a, b, M, N, K, **kw)
        outs.append(out)
        keep.append(ws)
        if want_sum is not False and want_sum is not None:
            # True = a fresh vector; a caller's own fp32 tensor of M elements is written in place
            rs = want_sum if isinstance(want_sum, torch.Tensor) else torch.empty((M,), device=a.device, dtype=torch.float32)
            _dev(rs)
            if rs.dtype != torch.float32 or rs.numel() != M or not rs.is_contiguous():
                raise ValueError("rowsum takes a contiguous fp32 tensor of M elements")
            rs_ptrs[i] = rs.data_ptr()
            sums.append(rs)
        flops += 2.0 * M * N * K

    def launch():
        if sums:
            _lib.call("aptai_gemm_bf16_grouped_rowsum", descs, rs_ptrs, len(problems), _stream())
        else:
            _lib.call("aptai_gemm_bf16_grouped", descs, len(problems), _stream())

    pr = _probe
    d0 = descs[0]
    if pr is not None and pr.key == (bool(d0.a_kmajor), bool(d0.b_kmajor), bool(d0.out_f32)) and not torch.cuda.is_current_stream_capturing():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        launch()
        e1.record()
        pr.records.append((flops, e0, e1))
        return outs + sums
    launch()
    return outs + sums


_ONES = {}


def ones_kmajor(K: int, device) -> torch.Tensor:
    """[K][8] bf16 ones: the A operand that turns a column sum into a grouped-GEMM problem (bias gradients)."""
    key = (K, str(device))
    t = _ONES.get(key)
    if t is None:
        t = torch.ones((K, 8), device=device, dtype=torch.bfloat16)
        _ONES[key] = t
    return t


# ----------------------------------------------------------------------------- MX block-scaled FP8 (inference-only encoder)
def mx_quantize(x: torch.Tensor, out=None):
    """bf16 [rows][K] -> (q uint8 [rows][K], scales uint8 [rows][K/32]) in OCP MXFP8 (E4M3 elements, E8M0 block scales)."""
    _dev(x)
    rows, K = x.shape
    if out is None:
        q = torch.empty((rows, K), device=x.device, dtype=torch.uint8)
        s = torch.empty((rows, K // 32), device=x.device, dtype=torch.uint8)
    else:
        q, s = out
    _lib.call("aptai_mx_quantize_bf16", x.data_ptr(), x.stride(0), q.data_ptr(), q.stride(0), s.data_ptr(), s.stride(0), rows, K, _stream())
    return q, s


def gemm_mxfp8(aq, a_s, bq, b_s, M, N, K, *, bias=None, gelu=False, residual=None, out=None):
    """C bf16 [M][N] = dequant(A) . dequant(B)^T + bias [-> GELU] [+ residual] (aptai_gemm_mxfp8)."""
    _dev(aq, a_s, bq, b_s, bias, residual, out)
    if out is None:
        out = torch.empty((M, N), device=aq.device, dtype=torch.bfloat16)
    _lib.call("aptai_gemm_mxfp8", aq.data_ptr(), a_s.data_ptr(), aq.stride(0), a_s.stride(0), bq.data_ptr(), b_s.data_ptr(), bq.stride(0),
              b_s.stride(0), out.data_ptr(), out.stride(0), _ptr(bias), int(gelu), _ptr(residual), residual.stride(0) if residual is not None else 0,
              M, N, K, _stream())
    return out


def layernorm_fwd_mx(x, gamma, beta, eps, *, want_bf16=False):
    """nn.LayerNorm -> (bf16 | None, q uint8 [rows][cols], scales uint8 [rows][cols/32]) in one launch (aptai_layernorm_fwd_mx)."""
    _dev(x, gamma, beta)
    rows, cols = x.shape
    y = torch.empty_like(x) if want_bf16 else None
    q = torch.empty((rows, cols), device=x.device, dtype=torch.uint8)
    s = torch.empty((rows, cols // 32), device=x.device, dtype=torch.uint8)
    _lib.call("aptai_layernorm_fwd_mx", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(y), q.data_ptr(), q.stride(0), s.data_ptr(), s.stride(0),
              rows, cols, eps, _stream())
    return y, q, s


def gemm_mxfp8_mxout(aq, a_s, bq, b_s, M, N, K, *, bias=None, gelu=False, out=None):
    """(q uint8 [M][N], scales uint8 [M][N/32]) = mx_quantize(bf16(dequant(A) . dequant(B)^T + bias [-> GELU])) in one launch
    (aptai_gemm_mxfp8_mxout): the next MX GEMM's A operand without the bf16 tensor in between."""
    _dev(aq, a_s, bq, b_s, bias)
    if out is None:
        q = torch.empty((M, N), device=aq.device, dtype=torch.uint8)
        s = torch.empty((M, N // 32), device=aq.device, dtype=torch.uint8)
    else:
        q, s = out
    _lib.call("aptai_gemm_mxfp8_mxout", aq.data_ptr(), a_s.data_ptr(), aq.stride(0), a_s.stride(0), bq.data_ptr(), b_s.data_ptr(), bq.stride(0),
              b_s.stride(0), q.data_ptr(), q.stride(0), s.data_ptr(), s.stride(0), _ptr(bias), int(gelu), M, N, K, _stream())
    return q, s


# ----------------------------------------------------------------------------- exact (fp32-class) inference path
def split_f32(x32: torch.Tensor, pieces: int, *, weight_side: bool = False, gelu: bool = False, rows=None, cols=None, ldx=None) -> torch.Tensor:
    """fp32 [rows][cols] -> bf16 pieces [rows][cols * pieces] in the K-tile-interleaved layout of aptai_split_f32."""
    _dev(x32)
    rows = x32.shape[0] if rows is None else rows
    cols = x32.shape[1] if cols is None else cols
    out = torch.empty((rows, cols * pieces), device=x32.device, dtype=torch.bfloat16)
    _lib.call("aptai_split_f32", x32.data_ptr(), ldx if ldx is not None else x32.stride(0), rows, cols, int(weight_side), pieces, int(gelu),
              out.data_ptr(), cols * pieces, _stream())
    return out


def bias_act_res_f32(x32, *, bias=None, res=None, gelu=False, lens_i32=None, rows_per_b=0, out=None):
    """y = [res +] gelu_erf?(x + bias) in fp32; rows t >= lens[b] zeroed when lens_i32 is given (aptai_bias_act_res_f32)."""
    _dev(x32, bias, res, lens_i32, out)
    rows, cols = x32.shape
    y = out if out is not None else torch.empty((rows, cols), device=x32.device, dtype=torch.float32)
    _lib.call("aptai_bias_act_res_f32", x32.data_ptr(), x32.stride(0), _ptr(bias), _ptr(res), res.stride(0) if res is not None else 0,
              y.data_ptr(), y.stride(0), rows, cols, int(gelu), _ptr(lens_i32), rows_per_b, _stream())
    return y


def softmax_rows_f32(s32, lens_i32, B, heads, Tp):
    _dev(s32, lens_i32)
    _lib.call("aptai_softmax_rows_f32", s32.data_ptr(), lens_i32.data_ptr(), B, heads, Tp, _stream())
    return s32


def conv0_fwd_split(audio, weight, bias, gamma, beta, mode, out_split, pieces, T_real, T_alloc, stats, eps=1e-5):
    """The exact mode's first conv layer with its (already activated) result written as split bf16 pieces (aptai_conv0_fwd_split)."""
    _dev(audio, weight, bias, gamma, beta, out_split, stats)
    B, S = audio.shape
    _lib.call("aptai_conv0_fwd_split", audio.data_ptr(), B, S, weight.data_ptr(), _ptr(bias), gamma.data_ptr(), beta.data_ptr(), mode, eps,
              out_split.data_ptr(), pieces, T_real, T_alloc, _ptr(stats), _stream())
    return out_split


def softmax_split_f32(s32, lens_i32, B, heads, Tp, pieces):
    """Masked softmax of the fp32 scores [B][heads][Tp][Tp] written as split bf16 pieces [B heads Tp][pieces Tp] (aptai_softmax_split_f32)."""
    _dev(s32, lens_i32)
    out = torch.empty((B * heads * Tp, pieces * Tp), device=s32.device, dtype=torch.bfloat16)
    _lib.call("aptai_softmax_split_f32", s32.data_ptr(), lens_i32.data_ptr(), B, heads, Tp, pieces, out.data_ptr(), pieces * Tp, _stream())
    return out


def attention_exact_fwd(qkv_s, lens_i32, B, Tp, H, heads, pieces, scale, out=None):
    """Fused attention core of the exact-index mode (aptai_attention_exact_fwd): qkv_s bf16 [B Tp][3 pieces H] split Q | K | V as the
    q|k|v projection's split-out epilogue wrote them -> the context as split pieces [B Tp][pieces H] (the out-projection's A operand)."""
    _dev(qkv_s, lens_i32, out)
    if qkv_s.dtype != torch.bfloat16 or qkv_s.stride(1) != 1 or qkv_s.shape[0] != B * Tp or qkv_s.shape[1] != 3 * pieces * H:
        raise _lib.AptaiHipError("attention_exact_fwd: qkv_s must be bf16 [B Tp][3 pieces H] with unit column stride")
    if out is None:
        out = torch.empty((B * Tp, pieces * H), device=qkv_s.device, dtype=torch.bfloat16)
    _lib.call("aptai_attention_exact_fwd", qkv_s.data_ptr(), qkv_s.stride(0), lens_i32.data_ptr(), out.data_ptr(), out.stride(0), B, Tp, H,
              heads, pieces, float(scale), _stream())
    return out


def conv0_fwd_f32(audio, weight, bias, gamma, beta, mode, out32, T_real, T_alloc, stats, eps=1e-5):
    _dev(audio, weight, bias, gamma, beta, out32, stats)
    B, S = audio.shape
    _lib.call("aptai_conv0_fwd_f32", audio.data_ptr(), B, S, weight.data_ptr(), _ptr(bias), gamma.data_ptr(), beta.data_ptr(), mode, eps,
              out32.data_ptr(), T_real, T_alloc, _ptr(stats), _stream())
    return out32


def gemm_split(a_s: torch.Tensor, w_s: torch.Tensor, M: int, N: int, K: int, pieces: int, *, lda=None, bias=None, residual_f32=None,
               out=None, ldc=None, split_out: bool = False, gelu: bool = False, split_bcol=None) -> torch.Tensor:
    """fp32 C[M][N] = A . W^T (+ bias) (+ fp32 residual) from split operands (split_f32): one NT launch of K' = pieces * K.
    split_out: the result (after the erf GELU when `gelu`) is returned as split bf16 pieces [M][pieces N] instead - the next product's A."""
    # fp32-output launches name their tile (include/aptai_hip.h); whole rounds of 256 x 256 tiles where the output has them (the conv
    # stack's [B x 16384 ...] x 512 outputs: 3 x the bf16 work at K' = 3 K is the longest loop of the build), 128-row tiles elsewhere
    t256 = -(-M // 256) * -(-N // 256)
    tile = 256 if (M >= 256 and N >= 256 and t256 >= 1024) else 128
    # one round of full 128 x 192 tiles (the [8192] x 768 outputs of out-proj / FFN2 at K' = 3 K): the 3-stage-ring kernel, as on the bf16 path
    if tile == 128 and M % 128 == 0 and N % 192 == 0 and 192 < (M // 128) * (N // 192) <= 256:
        tile = 192
    return gemm(a_s, w_s, M, N, K * pieces, lda=(lda * pieces if lda is not None else None), out_f32=True, bias=bias, gelu=(gelu and split_out),
                residual_f32=residual_f32, out=out, ldc=ldc, tile=tile, split_out=(pieces if split_out else None), split_bcol=split_bcol)


# ----------------------------------------------------------------------------- LayerNorm
def _ws(nbytes: int, device) -> torch.Tensor:
    return torch.empty(max(int(nbytes), 16), device=device, dtype=torch.uint8)


def layernorm_fwd(x, gamma, beta, eps, *, gelu_after=False, save_stats=True, out=None):
    _dev(x, gamma, beta)
    rows, cols = x.shape[0], x.shape[1]
    y = out if out is not None else torch.empty_like(x)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    _lib.call("aptai_layernorm_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), _ptr(mean), _ptr(rstd),
              rows, cols, eps, int(gelu_after), _stream())
    return y, mean, rstd


_LN_DEFER = None      # list of (workspace, dgamma, dbeta, blocks, cols) while a graph runner collects the parameter-gradient reductions


def ln_defer_begin() -> list:
    """From here on layernorm_bwd only writes its per-block partials and registers the reduction; ln_finalize_multi() runs them all in
    ONE launch (aptai_layernorm_bwd_finalize_multi).  Used by the graph runner around the capture of its backward segments: the
    returned dgamma / dbeta tensors are filled by that launch, which the runner replays at the end of the backward pass."""
    global _LN_DEFER
    _LN_DEFER = []
    return _LN_DEFER


def ln_defer_end() -> None:
    global _LN_DEFER
    _LN_DEFER = None


def ln_defer_table(jobs: list):
    """Device job table of the registered reductions (build it OUTSIDE stream capture: it is a host-to-device copy); the caller
    keeps it, and the job list (workspaces, outputs), alive for as long as it launches ln_finalize_multi on it."""
    rows = [[ws.data_ptr(), dg.data_ptr(), db.data_ptr(), blocks, cols] for ws, dg, db, blocks, cols in jobs]
    return torch.tensor(rows, dtype=torch.int64).to(jobs[0][0].device), len(rows), max(r[4] for r in rows)


def ln_finalize_multi(table, n: int, max_cols: int) -> None:
    """Every registered dgamma / dbeta reduction in ONE launch (aptai_layernorm_bwd_finalize_multi); capturable."""
    _lib.call("aptai_layernorm_bwd_finalize_multi", table.data_ptr(), n, max_cols, _stream())


def layernorm_bwd(dy, x, mean, rstd, gamma, *, dres=None, dropout_p=0.0, seed=0, need_param_grads=True, beta_gelu=None):
    """Returns (dx, dx_drop | None, dgamma | None, dbeta | None)."""
    _dev(dy, x, mean, rstd, gamma, dres)
    rows, cols = x.shape
    dx = torch.empty_like(x)
    dx_drop = torch.empty_like(x) if dropout_p > 0 else None
    dgamma = dbeta = None
    if need_param_grads:
        dgamma = torch.empty(cols, device=x.device, dtype=torch.float32)
        dbeta = torch.empty(cols, device=x.device, dtype=torch.float32)
    nbytes = _lib.lib().aptai_layernorm_bwd_workspace_bytes(rows, cols)
    ws = _ws(nbytes, x.device)
    defer = need_param_grads and _LN_DEFER is not None
    _lib.call("aptai_layernorm_bwd", dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
              _ptr(dres), dx.data_ptr(), _ptr(dx_drop), dropout_p, seed, None if defer else _ptr(dgamma), None if defer else _ptr(dbeta),
              ws.data_ptr(), rows, cols, _ptr(beta_gelu), _stream())
    if defer:
        _LN_DEFER.append((ws, dgamma, dbeta, nbytes // (8 * cols), cols))
    return dx, dx_drop, dgamma, dbeta


# ----------------------------------------------------------------------------- attention
ATTN_LOG2E = 1.4426950408889634


def layernorm_fwd_f32in(x32, gamma, beta, eps, *, want_bf16=True, want_f32=True):
    """nn.LayerNorm on an fp32 activation [rows][cols] -> (bf16 copy | None, fp32 copy | None) (aptai_layernorm_fwd_f32in)."""
    _dev(x32, gamma, beta)
    rows, cols = x32.shape
    y = torch.empty((rows, cols), device=x32.device, dtype=torch.bfloat16) if want_bf16 else None
    y32 = torch.empty((rows, cols), device=x32.device, dtype=torch.float32) if want_f32 else None
    _lib.call("aptai_layernorm_fwd_f32in", x32.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(y), _ptr(y32), rows, cols, eps, _stream())
    return y, y32


def layernorm_fwd_f32in_split(x32, gamma, beta, eps, pieces, *, want_f32=True):
    """nn.LayerNorm on an fp32 activation -> (fp32 copy | None, split bf16 pieces [rows][pieces cols]) (aptai_layernorm_fwd_f32in_split)."""
    _dev(x32, gamma, beta)
    rows, cols = x32.shape
    y32 = torch.empty((rows, cols), device=x32.device, dtype=torch.float32) if want_f32 else None
    ys = torch.empty((rows, cols * pieces), device=x32.device, dtype=torch.bfloat16)
    _lib.call("aptai_layernorm_fwd_f32in_split", x32.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _ptr(y32), ys.data_ptr(), pieces, rows, cols, eps, _stream())
    return y32, ys


def attention_qscale(H: int, heads: int) -> float:
    """The factor the fused q|k|v projection applies to its Q columns (gemm(..., colscale=(H, this))) for q_prescaled attention."""
    return (H // heads) ** -0.5 * ATTN_LOG2E


def attention_fwd(qkv, lens_i32, B, Tp, H, heads, *, dropout_p=0.0, seed=0, save_lse=True, q_prescaled=False):
    _dev(qkv, lens_i32)
    ctx = torch.empty((B * Tp, H), device=qkv.device, dtype=torch.bfloat16)
    lse2 = torch.empty((B, heads, Tp), device=qkv.device, dtype=torch.float32) if save_lse else None
    ctx32 = torch.empty((B * Tp, H), device=qkv.device, dtype=torch.float32) if save_lse else None
    _lib.call("aptai_attention_fwd", qkv.data_ptr(), lens_i32.data_ptr(), ctx.data_ptr(), _ptr(lse2), _ptr(ctx32), B, Tp, H,
              heads, (H // heads) ** -0.5, dropout_p, seed, int(q_prescaled), _stream())
    return ctx, (lse2, ctx32) if save_lse else None


def attention_bwd(qkv, lens_i32, ctx, dctx, stats, B, Tp, H, heads, *, dropout_p=0.0, seed=0, dctx_zero_beyond_len=False,
                  q_prescaled=False):
    """``stats`` = the (lse2, ctx_f32) pair returned by attention_fwd."""
    lse2, ctx32 = stats
    _dev(qkv, lens_i32, ctx, dctx, lse2)
    dqkv = torch.empty_like(qkv)
    delta = torch.empty((B, heads, Tp), device=qkv.device, dtype=torch.float32)
    _lib.call("aptai_attention_bwd", qkv.data_ptr(), lens_i32.data_ptr(), ctx.data_ptr(), _ptr(ctx32), dctx.data_ptr(), lse2.data_ptr(),
              delta.data_ptr(), dqkv.data_ptr(), B, Tp, H, heads, (H // heads) ** -0.5, dropout_p, seed,
              int(dctx_zero_beyond_len), int(q_prescaled), _stream())
    return dqkv


def attention_probs_fwd(qkv, lens_i32, lse2, B, Tp, H, heads, *, dropout_p=0.0, seed=0, q_prescaled=False):
    """The attention map of one layer, fp32 [B][heads][Tp][Tp] (aptai_attention_probs_fwd): softmax after dropout, from the ``lse2`` that
    attention_fwd saved for the same qkv / seed / q_prescaled.  Callers view [:, :, :T, :T]."""
    _dev(qkv, lens_i32, lse2)
    probs = torch.empty((B, heads, Tp, Tp), device=qkv.device, dtype=torch.float32)
    _lib.call("aptai_attention_probs_fwd", qkv.data_ptr(), lens_i32.data_ptr(), lse2.data_ptr(), probs.data_ptr(), B, Tp, H, heads,
              (H // heads) ** -0.5, dropout_p, seed, int(q_prescaled), _stream())
    return probs


def attention_probs_bwd(qkv, lens_i32, lse2, dprobs, B, Tp, H, heads, *, dropout_p=0.0, seed=0, q_prescaled=False, dqkv=None):
    """Gradient of a loss on the map (aptai_attention_probs_bwd).  ``dprobs`` fp32 [B][heads][Tp][Tp] contiguous.  With ``dqkv`` (what
    attention_bwd returned for the same layer) dQ and dK are ADDED to its Q and K thirds in place; without, a new tensor with a zero V
    third is returned."""
    _dev(qkv, lens_i32, lse2, dprobs)
    if dprobs.dtype != torch.float32 or tuple(dprobs.shape) != (B, heads, Tp, Tp) or not dprobs.is_contiguous():
        raise _lib.AptaiHipError("attention_probs_bwd: dprobs must be contiguous fp32 [B][heads][Tp][Tp]")
    accumulate = dqkv is not None
    if dqkv is None:
        dqkv = torch.zeros_like(qkv)
    rowsum = torch.empty((B, heads, Tp), device=qkv.device, dtype=torch.float32)
    _lib.call("aptai_attention_probs_bwd", qkv.data_ptr(), lens_i32.data_ptr(), lse2.data_ptr(), dprobs.data_ptr(), rowsum.data_ptr(),
              dqkv.data_ptr(), B, Tp, H, heads, (H // heads) ** -0.5, dropout_p, seed, int(q_prescaled), int(accumulate), _stream())
    return dqkv


# ----------------------------------------------------------------------------- parameter prep
def cast_bf16(src: torch.Tensor, dst: Optional[torch.Tensor] = None, ld_dst: Optional[int] = None) -> torch.Tensor:
    """fp32 [rows][cols] -> bf16 (optionally into a row slice of a wider buffer)."""
    _dev(src, dst)
    src2 = src.reshape(src.shape[0], -1) if src.dim() > 1 else src.reshape(1, -1)
    rows, cols = src2.shape
    if dst is None:
        dst = torch.empty(src.shape, device=src.device, dtype=torch.bfloat16)
    _lib.call("aptai_cast_f32_to_bf16", src2.data_ptr(), dst.data_ptr(), rows, cols, ld_dst if ld_dst else cols, _stream())
    return dst


class CastPlan:
    """A fixed list of (fp32 source, destination) pairs converted by ONE aptai_cast_multi launch.  The destinations are
    persistent, so a plan replays unchanged inside a hipGraph; sources are re-read on every run (parameters move only
    through in-place optimiser updates, so their addresses are stable; `stale()` detects re-allocated parameters)."""

    optimizer_synced = False    # the optimiser's own kernel writes the destinations with every update
    after_training = False      # the last run() came from a training forward: an optimiser step since is unseen
    version = None              # the parameter versions the destinations were last built from
    entries = None              # per-layer views of the destinations

    def __init__(self, jobs):
        # jobs: list of (src fp32 tensor, dst tensor [bf16 or fp32])
        self.jobs = list(jobs)
        rows = []
        for src, dst in self.jobs:
            _dev(src, dst)
            n = src.numel()
            if not (src.is_contiguous() and dst.is_contiguous() and src.dtype == torch.float32 and n == dst.numel() and n % 8 == 0
                    and src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0):
                raise _lib.AptaiHipError("CastPlan: jobs must be contiguous, 16-byte aligned fp32 sources of n % 8 == 0 elements")
            kind = {torch.bfloat16: 0, torch.float32: 1}[dst.dtype]
            rows.append([src.data_ptr(), dst.data_ptr(), n, kind])
        self.max_n = max(r[2] for r in rows)
        self.table = torch.tensor(rows, dtype=torch.int64).to(self.jobs[0][0].device)
        self._src_ptrs = [r[0] for r in rows]

    def stale(self) -> bool:
        return any(src.data_ptr() != p for (src, _), p in zip(self.jobs, self._src_ptrs))

    def run(self) -> None:
        _lib.call("aptai_cast_multi", self.table.data_ptr(), len(self.jobs), self.max_n, _stream())


class PinnedRing:
    """`slots` sets of pinned host buffers, one buffer per device tensor in `dst`, that take turns carrying a value to the device:
    a pageable host-to-device copy would block the host until the GPU has drained, and one pinned buffer could be refilled while
    its copy is still in flight.  The only wait is for the copy that last read the slot being handed out."""

    def __init__(self, dst, slots: int):
        self.dst = tuple(dst)
        self.host = [tuple(torch.empty(t.shape, dtype=t.dtype).pin_memory() for t in self.dst) for _ in range(slots)]
        self.views = [tuple(t.numpy() for t in bufs) for bufs in self.host]       # numpy views of the pinned buffers
        self.events = [None] * slots
        self.turn = 0

    def next(self):
        """The numpy views of the next slot, to be filled and then sent with send()."""
        ev = self.events[self.turn]
        if ev is not None:
            ev.synchronize()                                    # the copies that last read this slot have finished
        return self.views[self.turn]

    def send(self) -> None:
        """Asynchronous copies of the slot next() handed out into the device tensors, on the current stream."""
        slot = self.turn
        self.turn = (slot + 1) % len(self.host)
        for d, h in zip(self.dst, self.host[slot]):
            d.copy_(h, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[slot] = ev


GRAD_NORM_CHUNK = 4096      # elements per partial sum of grad_sqnorm_multi (ADAM_CHUNK of csrc/optim.hip)


def grad_norm_chunks(numels) -> int:
    """fp32 words of the partial-sum workspace grad_sqnorm_multi needs for jobs of these sizes."""
    return sum((int(n) + GRAD_NORM_CHUNK - 1) // GRAD_NORM_CHUNK for n in numels)


def grad_sqnorm_multi(table_ptr: int, dyn_ptr: int, njobs: int, max_n: int, partials, result, max_norm: float, stream=None) -> None:
    """result fp32 [3] = {global 2-norm, clip coefficient, gradient elements} of the jobs' gradients (aptai_grad_sqnorm_multi: Adam
    job tables by address, so a row range of a larger table works); order-fixed, no synchronisation."""
    _dev(partials, result)
    _lib.call("aptai_grad_sqnorm_multi", table_ptr, dyn_ptr, njobs, max_n, partials.data_ptr(), result.data_ptr(), float(max_norm),
              _stream() if stream is None else stream)


def adam_multi_scaled(table_ptr: int, dyn_ptr: int, njobs: int, max_n: int, lr, beta1, beta2, eps, weight_decay, scale,
                      stream=None) -> None:
    """aptai_adam_multi on gradients multiplied by the device scalar `scale` (aptai_adam_multi_scaled); `.grad` is not written."""
    _dev(scale)
    _lib.call("aptai_adam_multi_scaled", table_ptr, dyn_ptr, njobs, max_n, float(lr), float(beta1), float(beta2), float(eps),
              float(weight_decay), scale.data_ptr(), _stream() if stream is None else stream)


def scale_multi(table_ptr: int, dyn_ptr: int, njobs: int, max_n: int, scale, stream=None) -> None:
    """Gradients of the jobs *= the device scalar `scale`, in place (aptai_scale_multi)."""
    _dev(scale)
    _lib.call("aptai_scale_multi", table_ptr, dyn_ptr, njobs, max_n, scale.data_ptr(), _stream() if stream is None else stream)


def grad_accum_multi(table_ptr: int, dyn_ptr: int, acc_ptr: int, njobs: int, max_n: int, scale: float = 1.0, stream=None) -> None:
    """One micro-step of gradient accumulation over Adam job tables given by address (aptai_grad_accum_multi): per job acc = grad on
    the window's first contribution, acc += grad later, then acc *= scale when scale != 1 (the close: scale = 1 / micro-steps)."""
    _lib.call("aptai_grad_accum_multi", table_ptr, dyn_ptr, acc_ptr, njobs, max_n, float(scale), _stream() if stream is None else stream)


def ema_multi(table_ptr: int, ema_ptr: int, njobs: int, max_n: int, weight: float, stream=None) -> None:
    """Averages of the jobs += weight * (parameter - average) over Adam job tables given by address (aptai_ema_multi): three
    rounded fp32 operations per element, the bits of torch's e + w * (p - e) on CPU tensors."""
    _lib.call("aptai_ema_multi", table_ptr, ema_ptr, njobs, max_n, float(weight), _stream() if stream is None else stream)


def swap_multi(table_ptr: int, ema_ptr: int, njobs: int, max_n: int, stream=None) -> None:
    """Parameters and averages of the jobs exchanged in place (aptai_swap_multi); two calls are the identity."""
    _lib.call("aptai_swap_multi", table_ptr, ema_ptr, njobs, max_n, _stream() if stream is None else stream)


def conv_weight_bf16(w: torch.Tensor) -> torch.Tensor:
    """[N][C][Kw] fp32 -> [N][Kw*C] bf16."""
    _dev(w)
    N, C, Kw = w.shape
    out = torch.empty((N, Kw * C), device=w.device, dtype=torch.bfloat16)
    _lib.call("aptai_conv_weight_to_bf16", w.data_ptr(), out.data_ptr(), N, C, Kw, _stream())
    return out


def posconv_weight(v, gain, groups, want_dgrad=True):
    _dev(v, gain)
    H, Cg, Kw = v.shape
    norm_ws = torch.empty(257 * Kw, device=v.device, dtype=torch.float32)     # [Kw] result + [256][Kw] reduction scratch
    norm = norm_ws[:Kw]
    wf = torch.empty((groups, Cg, Kw * Cg), device=v.device, dtype=torch.bfloat16)
    wd = torch.empty_like(wf) if want_dgrad else None
    _lib.call("aptai_posconv_weight", v.data_ptr(), gain.data_ptr(), norm_ws.data_ptr(), wf.data_ptr(), _ptr(wd), H, groups, Kw,
              _stream())
    return wf, wd, norm


def posconv_weight_bwd(dw_fwd, v, gain, norm, groups):
    """Weight-norm backward of the positional conv: (dv [H][Cg][Kw], dgain [Kw]) from the weight gradient in the forward layout."""
    _dev(dw_fwd, v, gain, norm)
    H, Cg, Kw = v.shape
    dv = torch.empty_like(v)
    dgain = torch.empty(Kw, device=v.device, dtype=torch.float32)
    ws = torch.empty((H + 1) * Kw, device=v.device, dtype=torch.float32)
    _lib.call("aptai_posconv_weight_bwd", dw_fwd.data_ptr(), v.data_ptr(), gain.data_ptr(), norm.data_ptr(), dv.data_ptr(), dgain.data_ptr(),
              ws.data_ptr(), H, groups, Kw, _stream())
    return dv, dgain


def posconv_gemm(xg, w, out, B, Tp, H, groups, Kw, pad, *, first_row=0, bias=None, gelu=False, residual=None, out_pre=None):
    """Grouped positional convolution on the packed copy (aptai_posconv_gemm: 48 channels per group, 128 taps)."""
    _dev(xg, w, out, bias, residual, out_pre)
    _lib.call("aptai_posconv_gemm", xg.data_ptr(), first_row, w.data_ptr(), _ptr(bias), _ptr(residual), out.data_ptr(), _ptr(out_pre),
              B, Tp, H, groups, Kw, pad, int(gelu), _stream())
    return out


def posconv_wgrad(du_g, x_g, dw, B, Tp, H, groups, Kw, pad):
    """dW of the grouped positional convolution from the two packed copies (aptai_posconv_wgrad); dw fp32 [groups][48][Kw*48]."""
    _dev(du_g, x_g, dw)
    _lib.call("aptai_posconv_wgrad", du_g.data_ptr(), x_g.data_ptr(), dw.data_ptr(), B, Tp, H, groups, Kw, pad, _stream())
    return dw


def posconv_kernel_fits(H: int, groups: int, Kw: int, wgrad: bool = False) -> bool:
    """The dedicated kernels cover 48 channels per group (wav2vec2-base; forward, data and weight gradient) and 64 (large; forward
    and data gradient).  APTAI_POSCONV_KERNEL=0 forces the batched implicit-GEMM path (A/B)."""
    import os
    ok = (H == groups * 48) or (H == groups * 64 and not wgrad)
    return ok and Kw == 128 and os.environ.get("APTAI_POSCONV_KERNEL", "1") != "0"


def posconv_pack(x, xg, B, Tp, H, groups, pad, *, u=None, rowmajor_out=None):
    _dev(x, xg, u, rowmajor_out)
    _lib.call("aptai_posconv_pack", x.data_ptr(), _ptr(u), xg.data_ptr(), _ptr(rowmajor_out), B, Tp, H, groups, pad, _stream())


def spec_augment_mask(frame_lens_i32, B, T, mask_prob, mask_length, min_masks, seed, out=None):
    """SpecAugment time mask [B][T] uint8 sampled on the device (no host round trip of the lengths)."""
    _dev(frame_lens_i32, out)
    m = out if out is not None else torch.empty((B, T), device=frame_lens_i32.device, dtype=torch.uint8)
    _lib.call("aptai_spec_augment_mask", frame_lens_i32.data_ptr(), m.data_ptr(), B, T, float(mask_prob), mask_length, min_masks, seed,
              _stream())
    return m


def frame_mask_fwd(h, lens_i32, spec_mask_u8, embed, B, Tp, T, H, feat_mask_u8=None):
    """SpecAugment time fill + padded-frame zeroing, in place, one pass; feat_mask_u8 [B][H] uint8 adds SpecAugment along the hidden
    axis (channels zeroed on every valid frame after the time fill), None launches the time-only entry."""
    _dev(h, lens_i32, spec_mask_u8, embed, feat_mask_u8)
    entry, feat = ("aptai_frame_mask_fwd", ()) if feat_mask_u8 is None else ("aptai_frame_feature_mask_fwd", (feat_mask_u8.data_ptr(),))
    _lib.call(entry, h.data_ptr(), lens_i32.data_ptr(), _ptr(spec_mask_u8), _ptr(embed), *feat, B, Tp, T, H, _stream())


def frame_mask_bwd(dy, lens_i32, spec_mask_u8, B, Tp, T, H, want_dembed, feat_mask_u8=None):
    """Backward of frame_mask_fwd, in place on dy; returns dembed (None without a time mask or when not wanted)."""
    _dev(dy, lens_i32, spec_mask_u8, feat_mask_u8)
    dembed = ws = None
    if want_dembed and spec_mask_u8 is not None:
        dembed = torch.empty(H, device=dy.device, dtype=torch.float32)
        ws = _ws(_lib.lib().aptai_frame_mask_bwd_workspace_bytes(B, Tp, H), dy.device)
    entry, feat = ("aptai_frame_mask_bwd", ()) if feat_mask_u8 is None else ("aptai_frame_feature_mask_bwd", (feat_mask_u8.data_ptr(),))
    _lib.call(entry, dy.data_ptr(), lens_i32.data_ptr(), _ptr(spec_mask_u8), *feat, _ptr(dembed), _ptr(ws), B, Tp, T, H, _stream())
    return dembed


SPEC_MAX_SPANS = 256                         # csrc/elementwise.hip: spans per row of aptai_spec_augment_mask


def feature_mask_span_check(H, mask_prob, mask_length, min_masks):
    """The span sampler caps a row at SPEC_MAX_SPANS spans without a word; on the feature axis the count is known on the host
    (every row has length H), so a setting it cannot honour is refused before anything is launched."""
    most = max(int(mask_prob * H / mask_length + 1), int(min_masks))
    if most > SPEC_MAX_SPANS:
        raise ValueError(f"mask_feature_prob={mask_prob}, mask_feature_length={mask_length}, mask_feature_min_masks={min_masks} "
                         f"ask for up to {most} spans over {H} channels; the device sampler draws at most {SPEC_MAX_SPANS} per row")


def colsum(x, rows, N, *, ld=None, out=None, accumulate=False):
    _dev(x, out)
    if out is None:
        out = torch.empty(N, device=x.device, dtype=torch.float32)
    ws = _ws(_lib.lib().aptai_colsum_workspace_bytes(rows, N), x.device)
    _lib.call("aptai_colsum_bf16", x.data_ptr(), ld if ld else x.stride(0), out.data_ptr(), ws.data_ptr(), rows, N,
              int(accumulate), _stream())
    return out


def dropout(x, p, seed):
    _dev(x)
    y = torch.empty_like(x)
    _lib.call("aptai_dropout_bf16", x.data_ptr(), y.data_ptr(), x.numel(), p, seed, _stream())
    return y


def dgelu(dy, u):
    _dev(dy, u)
    out = torch.empty_like(dy)
    _lib.call("aptai_dgelu_bf16", dy.data_ptr(), u.data_ptr(), out.data_ptr(), dy.numel(), _stream())
    return out


# ----------------------------------------------------------------------------- conv layer 0
def _lens_vec(lens, B, what):
    """A per-utterance length vector of the batch-invariant entries: int32 [B], contiguous, on the device."""
    _dev(lens)
    if lens.dtype != torch.int32 or lens.shape != (B,) or not lens.is_contiguous():
        raise ValueError(f"{what} must be a contiguous int32 tensor of shape ({B},), got {lens.dtype} {tuple(lens.shape)}")
    return lens


def conv0_fwd(audio, weight, bias, gamma, beta, mode, out, T_real, T_alloc, eps=1e-5, want_stats=False, frame_lens0=None):
    """Returns the (mean, rstd) block [B][2][512] in group mode when ``want_stats`` (needed by conv0_bwd).  ``frame_lens0`` (int32
    [B] on the device, hostlogic.conv0_frame_lengths): the batch-invariant entry aptai_conv0_fwd_lens - every row normalised
    over its own frames and zero beyond them, bit for bit what it gets alone; None is the plain call."""
    _dev(audio, weight, bias, gamma, beta, out)
    B, S = audio.shape
    C, _, Kw = weight.shape
    ws = _ws(_lib.lib().aptai_conv0_workspace_bytes(B, T_real), audio.device) if mode == 0 else None
    stats = torch.empty((B, 2, C), device=audio.device, dtype=torch.float32) if (want_stats and mode == 0) else None
    if frame_lens0 is not None:
        _lib.call("aptai_conv0_fwd_lens", audio.data_ptr(), B, S, weight.data_ptr(), _ptr(bias), gamma.data_ptr(), beta.data_ptr(),
                  mode, eps, out.data_ptr(), T_real, T_alloc, C, Kw, 5, _ptr(ws), _ptr(stats),
                  _lens_vec(frame_lens0, B, "frame_lens0").data_ptr(), _stream())
        return stats
    _lib.call("aptai_conv0_fwd", audio.data_ptr(), B, S, weight.data_ptr(), _ptr(bias), gamma.data_ptr(), beta.data_ptr(), mode,
              eps, out.data_ptr(), T_real, T_alloc, C, Kw, 5, _ptr(ws), _ptr(stats), _stream())
    return stats


def conv0_bwd(audio, weight, bias, gamma, beta, mode, dy, T_real, T_alloc, stats, eps=1e-5):
    """Returns (dweight [512][1][10], dbias | None, dgamma, dbeta)."""
    _dev(audio, weight, bias, gamma, beta, dy, stats)
    B, S = audio.shape
    C = weight.shape[0]
    dev = audio.device
    dw = torch.empty_like(weight)
    db = torch.empty(C, device=dev, dtype=torch.float32) if bias is not None else None
    dg = torch.empty(C, device=dev, dtype=torch.float32)
    dbt = torch.empty(C, device=dev, dtype=torch.float32)
    ws = _ws(_lib.lib().aptai_conv0_bwd_workspace_bytes(B, T_real), dev)
    _lib.call("aptai_conv0_bwd", audio.data_ptr(), B, S, weight.data_ptr(), _ptr(bias), gamma.data_ptr(), beta.data_ptr(), mode, eps,
              dy.data_ptr(), T_real, T_alloc, _ptr(stats), dw.data_ptr(), _ptr(db), dg.data_ptr(), dbt.data_ptr(), ws.data_ptr(),
              _stream())
    return dw, db, dg, dbt


def conv0_bwd_data(audio, weight, bias, gamma, beta, mode, dy, T_real, T_alloc, stats, eps=1e-5):
    """Gradient w.r.t. the waveform of the first conv layer (aptai_conv0_bwd_data): daudio fp32 [B][S], arguments as conv0_bwd."""
    _dev(audio, weight, bias, gamma, beta, dy, stats)
    B, S = audio.shape
    daudio = torch.empty((B, S), device=audio.device, dtype=torch.float32)
    ws = _ws(_lib.lib().aptai_conv0_bwd_data_workspace_bytes(B, T_real), audio.device)
    _lib.call("aptai_conv0_bwd_data", audio.data_ptr(), B, S, weight.data_ptr(), _ptr(bias), gamma.data_ptr(), beta.data_ptr(), mode, eps,
              dy.data_ptr(), T_real, T_alloc, _ptr(stats), daudio.data_ptr(), ws.data_ptr(), _stream())
    return daudio


# ----------------------------------------------------------------------------- APTAI heads
def head_act_fwd(h, p_tv, p_ph, seed):
    _dev(h)
    a_tv, a_ph = torch.empty_like(h), torch.empty_like(h)
    _lib.call("aptai_head_act_fwd", h.data_ptr(), a_tv.data_ptr(), a_ph.data_ptr(), h.numel(), p_tv, p_ph, seed, _stream())
    return a_tv, a_ph


def head_act_bwd(h, d_tv, d_ph, p_tv, p_ph, seed):
    _dev(h, d_tv, d_ph)
    dh = torch.empty_like(h)
    _lib.call("aptai_head_act_bwd", h.data_ptr(), d_tv.data_ptr(), d_ph.data_ptr(), dh.data_ptr(), h.numel(), p_tv, p_ph, seed,
              _stream())
    return dh


def lowpass_fir(x, ldx, rows_per_b_in, taps_f64, y, ldy, rows_per_b_out, B, T, T_out, C, C_out, frame_lens=None):
    """``frame_lens`` (int32 [B] on the device): aptai_lowpass_fir_lens - the zero padding of each row starts at its own frame
    count, zeros beyond; None is the plain call (one T for the batch)."""
    _dev(x, taps_f64, y)
    if frame_lens is not None:
        _lib.call("aptai_lowpass_fir_lens", x.data_ptr(), ldx, rows_per_b_in, taps_f64.data_ptr(), taps_f64.numel(), y.data_ptr(), ldy,
                  rows_per_b_out, int(y.dtype == torch.bfloat16), B, T, T_out, C, C_out,
                  _lens_vec(frame_lens, B, "frame_lens").data_ptr(), _stream())
        return y
    _lib.call("aptai_lowpass_fir", x.data_ptr(), ldx, rows_per_b_in, taps_f64.data_ptr(), taps_f64.numel(), y.data_ptr(), ldy,
              rows_per_b_out, int(y.dtype == torch.bfloat16), B, T, T_out, C, C_out, _stream())
    return y


def aptai_loss_fwd(tv_pred, tv_tgt, logits, ldl, rows_per_b, phn_tgt, B, T, n_tv, n_phn, w_mse, w_ce, want_pred=True):
    _dev(tv_pred, tv_tgt, logits, phn_tgt)
    scalars = torch.empty(5, device=tv_pred.device, dtype=torch.float32)
    pred = torch.empty((B, T), device=tv_pred.device, dtype=torch.int64) if want_pred else None
    ws = _ws(_lib.lib().aptai_aptai_loss_workspace_bytes(), tv_pred.device)
    _lib.call("aptai_aptai_loss_fwd", tv_pred.data_ptr(), tv_tgt.data_ptr(), logits.data_ptr(), ldl, rows_per_b,
              phn_tgt.data_ptr(), B, T, n_tv, n_phn, w_mse, w_ce, scalars.data_ptr(), _ptr(pred), ws.data_ptr(), _stream())
    return scalars, pred


def aptai_loss_bwd(tv_pred, tv_tgt, logits, ldl, rows_per_b, phn_tgt, B, T, n_tv, n_phn, w_mse, w_ce, scalars, grad_out, ldd=64):
    _dev(tv_pred, tv_tgt, logits, phn_tgt, scalars, grad_out)
    d_tv = torch.empty((B, T, n_tv), device=tv_pred.device, dtype=torch.float32)
    d_logits = torch.empty((B * rows_per_b, ldd), device=tv_pred.device, dtype=torch.bfloat16)
    _lib.call("aptai_aptai_loss_bwd", tv_pred.data_ptr(), tv_tgt.data_ptr(), logits.data_ptr(), ldl, rows_per_b,
              phn_tgt.data_ptr(), B, T, n_tv, n_phn, w_mse, w_ce, scalars.data_ptr(), _ptr(grad_out), d_tv.data_ptr(),
              d_logits.data_ptr(), ldd, _stream())
    return d_tv, d_logits


# ----------------------------------------------------------------------------- CTC
_REDUCTION = {"none": 0, "mean": 1, "sum": 2}


def ctc_fwd(logits, ldl, rows_per_b, targets_i32, input_lens_i32, target_lens_i32, B, T, V, *, blank=0, reduction="mean",
            zero_infinity=True, vocab_sizes_i32=None, want_log_probs=True, want_beta=None):
    """Returns (loss scalar tensor, nll [B], log_probs (T,B,V) | None, workspace [alpha | beta | per-state log-probs]).
    want_beta (default: when gradients are enabled) also runs the beta recursion, beside alpha in the same launch."""
    _dev(logits, targets_i32, input_lens_i32, target_lens_i32, vocab_sizes_i32)
    dev = logits.device
    ldt = targets_i32.shape[1]
    alpha = torch.empty(_lib.lib().aptai_ctc_workspace_bytes(B, T, ldt) // 4, device=dev, dtype=torch.float32)
    nll = torch.empty(B, device=dev, dtype=torch.float32)
    loss = torch.zeros(1, device=dev, dtype=torch.float32)
    lp = torch.empty((T, B, V), device=dev, dtype=torch.float32) if want_log_probs else None
    if want_beta is None:
        want_beta = True
    _lib.call("aptai_ctc_fwd", logits.data_ptr(), ldl, rows_per_b, targets_i32.data_ptr(), ldt, input_lens_i32.data_ptr(),
              target_lens_i32.data_ptr(), _ptr(vocab_sizes_i32), B, T, V, blank, _REDUCTION[reduction], int(zero_infinity),
              _ptr(lp), alpha.data_ptr(), nll.data_ptr(), loss.data_ptr(), int(want_beta), _stream())
    alpha._beta_ready = bool(want_beta)
    return loss, nll, lp, alpha


def ctc_bwd(logits, ldl, rows_per_b, targets_i32, input_lens_i32, target_lens_i32, B, T, V, alpha, nll, grad_out, *, blank=0,
            reduction="mean", zero_infinity=True, vocab_sizes_i32=None, ldd=64, out_dtype=torch.bfloat16, extra_scale=1.0):
    _dev(logits, targets_i32, alpha, nll, grad_out)
    d = torch.empty((B * rows_per_b, ldd), device=logits.device, dtype=out_dtype)
    _lib.call("aptai_ctc_bwd", logits.data_ptr(), ldl, rows_per_b, targets_i32.data_ptr(), targets_i32.shape[1],
              input_lens_i32.data_ptr(), target_lens_i32.data_ptr(), _ptr(vocab_sizes_i32), B, T, V, blank, _REDUCTION[reduction],
              int(zero_infinity), alpha.data_ptr(), nll.data_ptr(), _ptr(grad_out), extra_scale, d.data_ptr(), ldd,
              int(out_dtype == torch.bfloat16), int(getattr(alpha, "_beta_ready", False)), _stream())
    return d


def ctc_greedy_decode(logits, ldl, rows_per_b, B, T, V, blank, max_n, *, input_lens_i32=None, sil=None, want_timesteps=False):
    """Device best-path decode: (ids int32 [B][max_n] zero-padded, n int32 [B] = full length), with want_timesteps
    (ids, timesteps int32 [B][max_n], n) - see aptai_ctc_greedy_decode.  input_lens_i32 = None decodes all T frames of every row;
    sil = a token id frames every row with it like the beam search does."""
    _dev(logits, input_lens_i32)
    if input_lens_i32 is not None and (input_lens_i32.dtype != torch.int32 or input_lens_i32.numel() != B
                                       or not input_lens_i32.is_contiguous()):
        raise ValueError(f"ctc_greedy_decode: input_lens_i32 must be a contiguous int32 vector of {B} entries")
    ids = torch.empty((B, max_n), device=logits.device, dtype=torch.int32)
    ts = torch.empty((B, max_n), device=logits.device, dtype=torch.int32) if want_timesteps else None
    n = torch.empty(B, device=logits.device, dtype=torch.int32)
    _lib.call("aptai_ctc_greedy_decode", logits.data_ptr(), ldl, rows_per_b, _ptr(input_lens_i32), B, T, V, blank,
              -1 if sil is None else int(sil), ids.data_ptr(), _ptr(ts), max_n, n.data_ptr(), _stream())
    return (ids, ts, n) if want_timesteps else (ids, n)


BEAM_MAX = _C["APTAI_BEAM_MAX"]
BEAM_MAX_V = _C["APTAI_BEAM_MAX_V"]


def ctc_beam_search(logits, ldl, rows_per_b, B, T, V, blank, sil, *, input_lens_i32=None, beam_size=10, beam_size_token=None,
                    beam_threshold=50.0, log_add=False, sil_score=0.0, nbest=1, max_n=None, lm=None, lm_weight=1.0):
    """Lexicon-free CTC beam search on the device (aptai_ctc_beam_search, which states the semantics and the tie rule):
    (tokens int32 [B][nbest][max_n], timesteps int32 [B][nbest][max_n], n_tok int32 [B][nbest], score fp64 [B][nbest],
    n_hyp int32 [B]), best hypothesis first.  `logits` is read like ctc_greedy_decode reads it; input_lens_i32 = None decodes all T
    frames of every row; beam_size_token = None uses all V tokens; max_n defaults to T + 2, the longest a hypothesis can be.
    lm = an ngram.NGramLM over the V tokens fuses it into the search with weight lm_weight (aptai_ctc_beam_search_lm; the tables
    are multiplied by the weight once on the host and cached on the model).  Nothing here synchronises host and device."""
    _dev(logits, input_lens_i32)
    if lm is not None:
        from .ngram import NGramLM
        if not isinstance(lm, NGramLM):
            raise ValueError(f"ctc_beam_search: lm must be an ngram.NGramLM or None, not {type(lm).__name__}")
        if lm.n_tokens != V:
            raise ValueError(f"ctc_beam_search: the language model has {lm.n_tokens} tokens, the logits V = {V}")
        if not math.isfinite(lm_weight):
            raise ValueError(f"ctc_beam_search: lm_weight must be finite, not {lm_weight}")
    max_n = T + 2 if max_n is None else int(max_n)
    k_tok = 0 if beam_size_token is None else int(beam_size_token)
    if not 1 <= beam_size <= BEAM_MAX:
        raise ValueError(f"ctc_beam_search: beam_size must be 1..{BEAM_MAX}, not {beam_size}")
    if not 1 <= nbest <= beam_size:
        raise ValueError(f"ctc_beam_search: nbest must be 1..beam_size ({beam_size}), not {nbest}")
    if not 1 <= V <= BEAM_MAX_V:
        raise ValueError(f"ctc_beam_search: V must be 1..{BEAM_MAX_V}, not {V}")
    if beam_size_token is not None and k_tok < 1:
        raise ValueError(f"ctc_beam_search: beam_size_token must be None (all tokens) or >= 1, not {beam_size_token}")
    if not beam_threshold >= 0:
        raise ValueError(f"ctc_beam_search: beam_threshold must be >= 0, not {beam_threshold}")
    if not (0 <= blank < V and 0 <= sil < V and blank != sil):
        raise ValueError(f"ctc_beam_search: blank ({blank}) and sil ({sil}) must be different tokens below V = {V}")
    if B < 1 or T < 1 or max_n < 1 or ldl < V or rows_per_b < T:
        raise ValueError(f"ctc_beam_search: bad sizes (B={B}, T={T}, max_n={max_n}, ldl={ldl}, rows_per_b={rows_per_b})")
    if input_lens_i32 is not None and (input_lens_i32.dtype != torch.int32 or input_lens_i32.numel() != B
                                       or not input_lens_i32.is_contiguous()):
        raise ValueError(f"ctc_beam_search: input_lens_i32 must be a contiguous int32 vector of {B} entries")
    dev = logits.device
    ws = torch.empty(_lib.lib().aptai_ctc_beam_search_workspace_bytes(B, T, beam_size, nbest), device=dev, dtype=torch.uint8)
    tokens = torch.empty((B, nbest, max_n), device=dev, dtype=torch.int32)
    timesteps = torch.empty((B, nbest, max_n), device=dev, dtype=torch.int32)
    n_tok = torch.empty((B, nbest), device=dev, dtype=torch.int32)
    score = torch.empty((B, nbest), device=dev, dtype=torch.float64)
    n_hyp = torch.empty(B, device=dev, dtype=torch.int32)
    args = (logits.data_ptr(), ldl, rows_per_b, _ptr(input_lens_i32), B, T, V, blank, sil, beam_size, k_tok, float(beam_threshold),
            int(bool(log_add)), float(sil_score), nbest, max_n, ws.data_ptr(), tokens.data_ptr(), timesteps.data_ptr(),
            n_tok.data_ptr(), score.data_ptr(), n_hyp.data_ptr())
    if lm is None:
        _lib.call("aptai_ctc_beam_search", *args, _stream())
    else:
        w, nxt, wf, n_states, start = lm.device_tables(lm_weight, dev)
        _lib.call("aptai_ctc_beam_search_lm", *args, w.data_ptr(), nxt.data_ptr(), wf.data_ptr(), n_states, start, _stream())
    return tokens, timesteps, n_tok, score, n_hyp


_TOPOLOGY = {"ctc": 0, "monotonic": 1}


def ctc_viterbi(logits, ldl, rows_per_b, targets_i32, input_lens_i32, target_lens_i32, B, T, V, *, blank=0, topology="ctc",
                vocab_sizes_i32=None, want_token_score=True):
    """Forced alignment on the device (aptai_ctc_viterbi): (frame_token int32 [B][T], spans int32 [B][ldt][2], score fp32 [B],
    token_score fp32 [B][ldt] | None).  `logits` may be a view that starts inside a row (its data pointer is what the kernel
    reads, with row stride ldl).  Nothing here synchronises host and device."""
    _dev(logits, targets_i32, input_lens_i32, target_lens_i32, vocab_sizes_i32)
    dev = logits.device
    if targets_i32.shape[1] == 0:                      # an all-empty batch still needs one (unread) label slot per row
        targets_i32 = torch.zeros((B, 1), device=dev, dtype=torch.int32)
    ldt = targets_i32.shape[1]
    ws = torch.empty(_lib.lib().aptai_ctc_viterbi_workspace_bytes(B, T, ldt), device=dev, dtype=torch.uint8)
    frame_token = torch.empty((B, T), device=dev, dtype=torch.int32)
    spans = torch.empty((B, ldt, 2), device=dev, dtype=torch.int32)
    score = torch.empty(B, device=dev, dtype=torch.float32)
    token_score = torch.empty((B, ldt), device=dev, dtype=torch.float32) if want_token_score else None
    _lib.call("aptai_ctc_viterbi", logits.data_ptr(), ldl, rows_per_b, targets_i32.data_ptr(), ldt, input_lens_i32.data_ptr(),
              target_lens_i32.data_ptr(), _ptr(vocab_sizes_i32), B, T, V, blank, _TOPOLOGY[topology], ws.data_ptr(),
              frame_token.data_ptr(), spans.data_ptr(), score.data_ptr(), _ptr(token_score), _stream())
    return frame_token, spans, score, token_score


CTC_VITERBI_WIDE_MAX_LABELS = _C["APTAI_CTC_VITERBI_WIDE_MAX_LABELS"]


def ctc_viterbi_wide(logits, ldl, rows_per_b, targets_i32, input_lens_i32, target_lens_i32, B, T, V, *, blank=0, topology="ctc",
                     vocab_sizes_i32=None, want_token_score=True):
    """`ctc_viterbi` for a wide lattice (aptai_ctc_viterbi_wide): label rows of up to CTC_VITERBI_WIDE_MAX_LABELS slots, the CTC
    topology only (any other is refused by the library).  Same four tensors, same fill values, the same bits as `ctc_viterbi` where
    both take the shape.  Nothing here synchronises host and device."""
    _dev(logits, targets_i32, input_lens_i32, target_lens_i32, vocab_sizes_i32)
    dev = logits.device
    if targets_i32.shape[1] == 0:                      # an all-empty batch still needs one (unread) label slot per row
        targets_i32 = torch.zeros((B, 1), device=dev, dtype=torch.int32)
    ldt = targets_i32.shape[1]
    ws = torch.empty(max(_lib.lib().aptai_ctc_viterbi_wide_workspace_bytes(B, T, ldt), 16), device=dev, dtype=torch.uint8)
    frame_token = torch.empty((B, T), device=dev, dtype=torch.int32)
    spans = torch.empty((B, ldt, 2), device=dev, dtype=torch.int32)
    score = torch.empty(B, device=dev, dtype=torch.float32)
    token_score = torch.empty((B, ldt), device=dev, dtype=torch.float32) if want_token_score else None
    _lib.call("aptai_ctc_viterbi_wide", logits.data_ptr(), ldl, rows_per_b, targets_i32.data_ptr(), ldt, input_lens_i32.data_ptr(),
              target_lens_i32.data_ptr(), _ptr(vocab_sizes_i32), B, T, V, blank, _TOPOLOGY[topology], ws.data_ptr(),
              frame_token.data_ptr(), spans.data_ptr(), score.data_ptr(), _ptr(token_score), _stream())
    return frame_token, spans, score, token_score


# ----------------------------------------------------------------------------- evaluation metrics (csrc/eval.hip)
EVAL_EDIT_MAX_LANE_SIDE = _C["APTAI_EVAL_EDIT_MAX_LANE_SIDE"]


def _eval_lens(lens, B, name):
    if lens.dtype != torch.int32 or lens.numel() != B or not lens.is_contiguous():
        raise _lib.AptaiHipError(f"{name}: lengths must be a contiguous int32 device vector of {B} entries")


def eval_tv_scores(gt, ldg, rows_g, pred, ldp, rows_p, lens_i32, B, max_len, C):
    """(rmse, pcc) fp64 [B][C] of fp32 trajectories at (b*rows + t)*ld + c - see aptai_eval_tv_scores.  No synchronisation."""
    _dev(gt, pred, lens_i32)
    if gt.dtype != torch.float32 or pred.dtype != torch.float32:
        raise _lib.AptaiHipError("eval_tv_scores: fp32 trajectories expected")
    _eval_lens(lens_i32, B, "eval_tv_scores")
    rmse = torch.empty((B, C), device=gt.device, dtype=torch.float64)
    pcc = torch.empty((B, C), device=gt.device, dtype=torch.float64)
    _lib.call("aptai_eval_tv_scores", gt.data_ptr(), ldg, rows_g, pred.data_ptr(), ldp, rows_p, lens_i32.data_ptr(), B, max_len, C,
              rmse.data_ptr(), pcc.data_ptr(), _stream())
    return rmse, pcc


def eval_frame_scores(gt_i64, ldg, pred_i64, ldp, lens_i32, B, max_len):
    """int32 [B][2] = {frames, frames with gt == pred} - see aptai_eval_frame_scores."""
    _dev(gt_i64, pred_i64, lens_i32)
    if gt_i64.dtype != torch.int64 or pred_i64.dtype != torch.int64:
        raise _lib.AptaiHipError("eval_frame_scores: int64 frame labels expected")
    _eval_lens(lens_i32, B, "eval_frame_scores")
    out = torch.empty((B, 2), device=gt_i64.device, dtype=torch.int32)
    _lib.call("aptai_eval_frame_scores", gt_i64.data_ptr(), ldg, pred_i64.data_ptr(), ldp, lens_i32.data_ptr(), B, max_len,
              out.data_ptr(), _stream())
    return out


def eval_boundary_counts(y_f64, ldy, ny_i32, yhat_f64, ldh, nh_i32, B, tolerance):
    """int32 [B][2] = {precision_counter, recall_counter} of get_stats - see aptai_eval_boundary_counts."""
    _dev(y_f64, yhat_f64, ny_i32, nh_i32)
    if y_f64.dtype != torch.float64 or yhat_f64.dtype != torch.float64:
        raise _lib.AptaiHipError("eval_boundary_counts: fp64 boundary values expected")
    _eval_lens(ny_i32, B, "eval_boundary_counts")
    _eval_lens(nh_i32, B, "eval_boundary_counts")
    out = torch.empty((B, 2), device=y_f64.device, dtype=torch.int32)
    _lib.call("aptai_eval_boundary_counts", y_f64.data_ptr(), ldy, ny_i32.data_ptr(), yhat_f64.data_ptr(), ldh, nh_i32.data_ptr(),
              float(tolerance), B, out.data_ptr(), _stream())
    return out


def eval_collapse_runs(x_i64, ld, lens_i32, B, ldo=None):
    """(out int32 [B][ldo] zero-padded, n int32 [B]): runs of equal labels collapsed - see aptai_eval_collapse_runs."""
    _dev(x_i64, lens_i32)
    if x_i64.dtype != torch.int64:
        raise _lib.AptaiHipError("eval_collapse_runs: int64 frame labels expected")
    _eval_lens(lens_i32, B, "eval_collapse_runs")
    ldo = int(ld if ldo is None else ldo)
    out = torch.empty((B, ldo), device=x_i64.device, dtype=torch.int32)
    n = torch.empty(B, device=x_i64.device, dtype=torch.int32)
    _lib.call("aptai_eval_collapse_runs", x_i64.data_ptr(), ld, lens_i32.data_ptr(), B, out.data_ptr(), ldo, n.data_ptr(), _stream())
    return out, n


def eval_edit_distance(a_i32, lda, a_lens_i32, b_i32, ldb, b_lens_i32, B):
    """Levenshtein distance int32 [B] of B pairs of int32 rows - see aptai_eval_edit_distance.  The kernel keeps `a` in registers
    (at most EVAL_EDIT_MAX_LANE_SIDE symbols per row): the narrower side goes there, the distance is symmetric.  Two rows both
    wider than that are refused by the library, with both widths in the message."""
    _dev(a_i32, b_i32, a_lens_i32, b_lens_i32)
    if a_i32.dtype != torch.int32 or b_i32.dtype != torch.int32:
        raise _lib.AptaiHipError("eval_edit_distance: int32 symbols expected")
    _eval_lens(a_lens_i32, B, "eval_edit_distance")
    _eval_lens(b_lens_i32, B, "eval_edit_distance")
    if ldb < lda:
        a_i32, lda, a_lens_i32, b_i32, ldb, b_lens_i32 = b_i32, ldb, b_lens_i32, a_i32, lda, a_lens_i32
    dist = torch.empty(B, device=a_i32.device, dtype=torch.int32)
    _lib.call("aptai_eval_edit_distance", a_i32.data_ptr(), lda, a_lens_i32.data_ptr(), b_i32.data_ptr(), ldb, b_lens_i32.data_ptr(), B,
              dist.data_ptr(), _stream())
    return dist


# ----------------------------------------------------------------------------- audio front end (csrc/frontend.hip)
RESAMPLE_MAX_TABLE = _C["APTAI_RESAMPLE_MAX_TABLE"]


def _i64_vec(t, n, name, what):
    if t.dtype != torch.int64 or t.numel() != n or not t.is_contiguous():
        raise _lib.AptaiHipError(f"{name}: {what} must be a contiguous int64 device vector of {n} entries")


def resample_batch(packed, offsets_i64, B, taps_f32, first_i32, orig, new, Kc, width, out, ncols, out_start_i64=None):
    """Resamples the B utterances packed back to back in `packed` (1-D float32 or int16) into the first `ncols` columns of
    `out` fp32 [B][ld] - see aptai_resample_batch.  `taps_f32` [new][Kc] / `first_i32` [new] from hostlogic.resample_taps (both may
    be None when orig == new).  No synchronisation."""
    _dev(packed, offsets_i64, taps_f32, first_i32, out, out_start_i64)
    if packed.dtype not in (torch.float32, torch.int16) or packed.dim() != 1 or not packed.is_contiguous():
        raise _lib.AptaiHipError("resample_batch: the packed source must be a contiguous 1-D float32 or int16 tensor")
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1 or ncols > out.shape[1]:
        raise _lib.AptaiHipError(f"resample_batch: the output must be fp32 [{B}][>= {ncols}] with unit column stride")
    _i64_vec(offsets_i64, B + 1, "resample_batch", "offsets")
    if out_start_i64 is not None:
        _i64_vec(out_start_i64, B, "resample_batch", "out_start")
    if orig != new:
        if (taps_f32 is None or first_i32 is None or taps_f32.dtype != torch.float32 or first_i32.dtype != torch.int32
                or taps_f32.numel() != new * Kc or first_i32.numel() != new or not taps_f32.is_contiguous() or not first_i32.is_contiguous()):
            raise _lib.AptaiHipError(f"resample_batch: taps fp32 [{new}][{Kc}] and first int32 [{new}] expected")
    _lib.call("aptai_resample_batch", packed.data_ptr(), int(packed.dtype == torch.int16), offsets_i64.data_ptr(), B, _ptr(taps_f32),
              _ptr(first_i32), orig, new, Kc, width, _ptr(out_start_i64), out.data_ptr(), out.stride(0), ncols, _stream())
    return out


RESAMPLE_MAX_RATIOS = _C["APTAI_RESAMPLE_MAX_RATIOS"]
RESAMPLE_ENTRY = 8                      # int32 words per ratio: orig, new, Kc, width, taps_off, first_off, 0, 0


def resample_batch_multi(packed, offsets_i64, B, taps_f32, first_i32, table_i32, table_host, ratio_i32, ratio_host, out, ncols,
                         out_start_i64=None):
    """`resample_batch` with a ratio per row - see aptai_resample_batch_multi.  `table_i32` [n][8] / `ratio_i32` [B] are the device
    copies of the int32 numpy arrays `table_host` / `ratio_host`, which the library checks before the launch; `taps_f32` /
    `first_i32` are the banks back to back (None when every entry is 1:1).  No synchronisation."""
    _dev(packed, offsets_i64, taps_f32, first_i32, table_i32, ratio_i32, out, out_start_i64)
    if packed.dtype not in (torch.float32, torch.int16) or packed.dim() != 1 or not packed.is_contiguous():
        raise _lib.AptaiHipError("resample_batch_multi: the packed source must be a contiguous 1-D float32 or int16 tensor")
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] != B or out.stride(1) != 1 or ncols > out.shape[1]:
        raise _lib.AptaiHipError(f"resample_batch_multi: the output must be fp32 [{B}][>= {ncols}] with unit column stride")
    _i64_vec(offsets_i64, B + 1, "resample_batch_multi", "offsets")
    if out_start_i64 is not None:
        _i64_vec(out_start_i64, B, "resample_batch_multi", "out_start")
    table_host = np.ascontiguousarray(table_host, dtype=np.int32)
    ratio_host = np.ascontiguousarray(ratio_host, dtype=np.int32).reshape(-1)
    n = table_host.shape[0] if table_host.ndim == 2 else 0
    if table_host.ndim != 2 or table_host.shape[1] != RESAMPLE_ENTRY or not 1 <= n <= RESAMPLE_MAX_RATIOS:
        raise _lib.AptaiHipError(f"resample_batch_multi: a table of 1 .. {RESAMPLE_MAX_RATIOS} entries of {RESAMPLE_ENTRY} int32 words expected")
    if (table_i32.dtype != torch.int32 or table_i32.numel() != n * RESAMPLE_ENTRY or not table_i32.is_contiguous()
            or ratio_i32.dtype != torch.int32 or ratio_i32.numel() != B or not ratio_i32.is_contiguous() or ratio_host.size != B):
        raise _lib.AptaiHipError(f"resample_batch_multi: table int32 [{n}][{RESAMPLE_ENTRY}] and ratio int32 [{B}] expected, on the device and on the host")
    for t, dt, what in ((taps_f32, torch.float32, "taps fp32"), (first_i32, torch.int32, "first int32")):
        if t is not None and (t.dtype != dt or not t.is_contiguous()):
            raise _lib.AptaiHipError(f"resample_batch_multi: contiguous {what} expected")
    _lib.call("aptai_resample_batch_multi", packed.data_ptr(), int(packed.dtype == torch.int16), offsets_i64.data_ptr(), B, _ptr(taps_f32),
              0 if taps_f32 is None else taps_f32.numel(), _ptr(first_i32), 0 if first_i32 is None else first_i32.numel(),
              table_i32.data_ptr(), table_host.ctypes.data, n, ratio_i32.data_ptr(), ratio_host.ctypes.data, _ptr(out_start_i64),
              out.data_ptr(), out.stride(0), ncols, _stream())
    return out


def warp_targets(tracks_f64, labels_i64, n_in_i64, n_out_i64, T_out):
    """Frame-level targets stretched from n_in to n_out frames per row - see aptai_warp_targets.  `tracks_f64` fp64 [R_trk][T_in] and
    `labels_i64` int64 [R_lab][T_in] (either may be None), `n_in_i64` / `n_out_i64` int64 device vectors of R_trk + R_lab entries
    (tracks first).  Returns (tracks fp64 [R_trk][T_out] or None, labels int64 [R_lab][T_out] or None).  No synchronisation."""
    _dev(tracks_f64, labels_i64, n_in_i64, n_out_i64)
    if tracks_f64 is None and labels_i64 is None:
        raise _lib.AptaiHipError("warp_targets: neither tracks nor labels")
    for t, dt, what in ((tracks_f64, torch.float64, "tracks fp64"), (labels_i64, torch.int64, "labels int64")):
        if t is not None and (t.dtype != dt or t.dim() != 2 or not t.is_contiguous()):
            raise _lib.AptaiHipError(f"warp_targets: contiguous {what} [rows][T_in] expected")
    if tracks_f64 is not None and labels_i64 is not None and tracks_f64.shape[1] != labels_i64.shape[1]:
        raise _lib.AptaiHipError("warp_targets: tracks and labels must have the same width")
    some = tracks_f64 if tracks_f64 is not None else labels_i64
    R_trk = 0 if tracks_f64 is None else tracks_f64.shape[0]
    R_lab = 0 if labels_i64 is None else labels_i64.shape[0]
    T_in, T_out = some.shape[1], int(T_out)
    _i64_vec(n_in_i64, R_trk + R_lab, "warp_targets", "n_in")
    _i64_vec(n_out_i64, R_trk + R_lab, "warp_targets", "n_out")
    ld_out = max(T_out, 1)
    trk_out = None if tracks_f64 is None else torch.empty((R_trk, ld_out), device=some.device, dtype=torch.float64)[:, :T_out]
    lab_out = None if labels_i64 is None else torch.empty((R_lab, ld_out), device=some.device, dtype=torch.int64)[:, :T_out]
    _lib.call("aptai_warp_targets", _ptr(tracks_f64), R_trk, _ptr(labels_i64), R_lab, T_in, T_in,
              n_in_i64.data_ptr(), n_out_i64.data_ptr(), _ptr(trk_out), _ptr(lab_out), ld_out, T_out, _stream())
    return trk_out, lab_out


def wave_normalize(x, lens_i64, ncols=None):
    """zero_mean_unit_var_norm in place over the first lens[b] samples of every row of x fp32 [B][ld] - see aptai_wave_normalize."""
    _dev(x, lens_i64)
    if x.dtype != torch.float32 or x.dim() != 2 or x.stride(1) != 1:
        raise _lib.AptaiHipError("wave_normalize: fp32 [B][ld] with unit column stride expected")
    B = x.shape[0]
    ncols = x.shape[1] if ncols is None else int(ncols)
    _i64_vec(lens_i64, B, "wave_normalize", "lengths")
    ws = _ws(max(_lib.lib().aptai_wave_normalize_workspace_bytes(B, ncols), 8), x.device)
    _lib.call("aptai_wave_normalize", x.data_ptr(), x.stride(0), lens_i64.data_ptr(), B, ncols, ws.data_ptr(), _stream())
    return x


# ----------------------------------------------------------------------------- long recordings (csrc/longform.hip)
def window_gather(packed, table_i64, first, rows, S):
    """Windows first .. first + rows - 1 of `table_i64` (int64 [n_windows][3] on the device: recording offset, sample start, sample
    count) cut out of `packed` (1-D fp32: the recordings back to back) - see aptai_window_gather.  Returns (audio fp32 [rows][S]
    zero-padded, lens int64 [rows]).  No synchronisation."""
    _dev(packed, table_i64)
    if packed.dtype != torch.float32 or packed.dim() != 1 or not packed.is_contiguous():
        raise _lib.AptaiHipError("window_gather: the packed source must be a contiguous 1-D float32 tensor")
    if table_i64.dtype != torch.int64 or table_i64.dim() != 2 or table_i64.shape[1] != 3 or not table_i64.is_contiguous():
        raise _lib.AptaiHipError("window_gather: the window table must be a contiguous int64 [n_windows][3] device tensor")
    first, rows, S = int(first), int(rows), int(S)
    out = torch.empty((max(rows, 0), max(S, 0)), device=packed.device, dtype=torch.float32)
    lens = torch.empty(max(rows, 0), device=packed.device, dtype=torch.int64)
    _lib.call("aptai_window_gather", packed.data_ptr(), packed.numel(), table_i64.data_ptr(), table_i64.shape[0], first, rows,
              out.data_ptr(), S, S, lens.data_ptr(), _stream())
    return out, lens


def stitch_windows(x, ldx, rows_per_window, n_windows, rec_i64, max_frames, window_frames, hop_frames, ramp_f32, C, *, out=None,
                   out_rows=None, ldo=None, want_argmax=True):
    """Per-window fp32 rows `x` (window w at rows w rows_per_window .., pitch ldx) stitched into the rows of their recordings -
    see aptai_stitch_windows.  `rec_i64`: int64 [n_rec][3] on the device (first window, frame count, first output row);
    `max_frames` >= every frame count; `ramp_f32`: fp32 [window_frames - hop_frames] on the device (hostlogic.long_form_ramp), None
    when no recording has a second window.  `out` fp32 [out_rows][ldo] is made here (zeros) unless given.  Returns (out, argmax
    int64 [out_rows] or None): the argmax rows that no recording owns stay 0.  No synchronisation, no host read-back."""
    _dev(x, rec_i64, ramp_f32, out)
    ldx, rows_per_window, n_windows, C = int(ldx), int(rows_per_window), int(n_windows), int(C)
    if x.dtype != torch.float32 or not x.is_contiguous() or n_windows < 1 or x.numel() < (n_windows * rows_per_window - 1) * ldx + C:
        raise _lib.AptaiHipError(f"stitch_windows: contiguous fp32 results of {n_windows} windows x {rows_per_window} rows of pitch {ldx} expected")
    if rec_i64.dtype != torch.int64 or rec_i64.dim() != 2 or rec_i64.shape[1] != 3 or not rec_i64.is_contiguous():
        raise _lib.AptaiHipError("stitch_windows: the recording table must be a contiguous int64 [n_rec][3] device tensor")
    overlap = int(window_frames) - int(hop_frames)
    if ramp_f32 is not None and (ramp_f32.dtype != torch.float32 or not ramp_f32.is_contiguous() or ramp_f32.numel() < overlap):
        raise _lib.AptaiHipError(f"stitch_windows: a contiguous fp32 ramp of {overlap} entries expected")
    if out is None:
        if out_rows is None:
            raise _lib.AptaiHipError("stitch_windows: out or out_rows expected")
        ldo = C if ldo is None else int(ldo)
        out = torch.zeros((int(out_rows), ldo), device=x.device, dtype=torch.float32)
    if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[1] < C:
        raise _lib.AptaiHipError(f"stitch_windows: the output must be fp32 [rows][>= {C}] with unit column stride")
    argmax = torch.zeros(out.shape[0], device=x.device, dtype=torch.int64) if want_argmax else None
    _lib.call("aptai_stitch_windows", x.data_ptr(), ldx, rows_per_window, n_windows, rec_i64.data_ptr(), rec_i64.shape[0], int(max_frames),
              int(window_frames), int(hop_frames), _ptr(ramp_f32), C, out.data_ptr(), out.stride(0), out.shape[0], _ptr(argmax), _stream())
    return out, argmax


# ----------------------------------------------------------------------------- Force_APTAI heads (fp32)
def sgemm(a, sam, sak, b, sbk, sbn, M, N, K, *, out=None, ldc=None, bias=None, alpha=1.0, accumulate=False, batch=1, bsa=0, bsb=0,
          bsc=0, split_k=None):
    """C[m][n] (+)= alpha * sum_k A(m,k) B(k,n) + bias[n] with explicit element strides (see aptai_sgemm_f32).
    split_k=None picks the K split that fills the chip for gradient-shaped problems (small M x N, long K)."""
    _dev(a, b, out, bias)
    if out is None:
        out = torch.empty((batch * M, N) if batch > 1 else (M, N), device=a.device, dtype=torch.float32)
        if batch > 1 and bsc == 0:
            bsc = M * N
    if split_k is None:
        tiles = ((M + 63) // 64) * ((N + 63) // 64) * batch
        split_k = 1 if (tiles >= 256 or K < 256) else max(1, min(K // 128, 512 // tiles))
    ws = None
    if split_k > 1:
        ws = SCRATCH.get("sgemm", batch * split_k * M * N, a.device, _stream())
    _lib.call("aptai_sgemm_f32", a.data_ptr(), int(a.dtype == torch.bfloat16), sam, sak, b.data_ptr(), sbk, sbn, out.data_ptr(),
              ldc if ldc else N, _ptr(bias), alpha, int(accumulate), M, N, K, batch, bsa, bsb, bsc, split_k, _ptr(ws), _stream())
    return out


def linear_f32(x, w, bias=None, *, rows=None, out=None, ldc=None, ldx=None):
    """y = x W^T + b, x [rows][in] (fp32 or bf16, row stride ldx), W [out][in] fp32."""
    N, K = w.shape
    M = rows if rows is not None else x.shape[0]
    return sgemm(x, ldx if ldx else x.stride(0), 1, w, 1, K, M, N, K, out=out, ldc=ldc, bias=bias)


def linear_f32_dx(dy, w, M):
    """dx [M][K] = dy [M][N] W [N][K] of linear_f32."""
    N, K = w.shape
    return sgemm(dy, N, 1, w, K, 1, M, K, N)


def linear_f32_dwdb(dy, x, M, bias=True):
    """(dW [N][K], db [N] | None) of linear_f32 from dense fp32 dy [M][N], x [M][K]."""
    N, K = dy.shape[1], x.shape[1]
    return sgemm(dy, 1, N, x, K, 1, N, K, M), colsum_f32(dy, M, N) if bias else None


def embed_pe_fwd(ids_i32, emb, pe, N, p, seed):
    rows, D = ids_i32.numel(), emb.shape[1]
    out = torch.empty((rows, D), device=emb.device, dtype=torch.float32)
    _lib.call("aptai_embed_pe_fwd", ids_i32.data_ptr(), emb.data_ptr(), pe.data_ptr(), out.data_ptr(), rows, N, D, p, seed, _stream())
    return out


def embed_bwd(ids_i32, dout, vocab, p, seed):
    rows, D = dout.shape
    demb = torch.zeros((vocab, D), device=dout.device, dtype=torch.float32)
    _lib.call("aptai_embed_bwd", ids_i32.data_ptr(), dout.data_ptr(), demb.data_ptr(), rows, D, p, seed, _stream())
    return demb


XATTN_MAX_SLOTS = 255                  # the wide softmax pair and the CTC kernels behind the forward-sum loss (MAXV = 256 classes)


def fs_row_pitch(N: int) -> int:
    """Floats per forward-sum row [-1 | att_log[0..N) | zeros]: round_up(N + 1, 64)."""
    return (int(N) + 64) // 64 * 64


def xattn_softmax_fwd(raw, ids_i32, B, T, N, fs_rows=None):
    """fs_rows (optional [B*T][fs_row_pitch(N)] fp32, or True to have it allocated and returned as a fifth value): also writes the
    forward-sum CTC input rows [-1 | att_log | 0].  Up to 63 slots (64 without rows) run the one-slot-per-lane kernel, up to 255
    the wide one."""
    dev = raw.device
    if not 0 < N <= XATTN_MAX_SLOTS:
        raise _lib.AptaiHipError(f"xattn_softmax_fwd: 1..{XATTN_MAX_SLOTS} phoneme slots, got {N}")
    ld = fs_row_pitch(N)
    made = fs_rows is True
    if made:
        fs_rows = torch.empty((B * T, ld), device=dev, dtype=torch.float32)
    elif fs_rows is not None and (fs_rows.dtype != torch.float32 or not fs_rows.is_contiguous() or fs_rows.dim() != 2
                                  or fs_rows.shape[0] < B * T or fs_rows.shape[1] != ld):
        raise _lib.AptaiHipError(f"xattn_softmax_fwd: fs_rows must be contiguous fp32 [{B * T}][{ld}] for {N} slots, "
                                 f"got {tuple(fs_rows.shape)} {fs_rows.dtype}")
    energy, att, att_log = (torch.empty((B * T, N), device=dev, dtype=torch.float32) for _ in range(3))
    align = torch.empty((B, T), device=dev, dtype=torch.int64)
    if N <= 63 or (N == 64 and fs_rows is None):
        _lib.call("aptai_xattn_softmax_fwd", raw.data_ptr(), ids_i32.data_ptr(), energy.data_ptr(), att.data_ptr(), att_log.data_ptr(),
                  align.data_ptr(), _ptr(fs_rows), B, T, N, _stream())
    else:
        _lib.call("aptai_xattn_softmax_fwd_wide", raw.data_ptr(), ids_i32.data_ptr(), energy.data_ptr(), att.data_ptr(),
                  att_log.data_ptr(), align.data_ptr(), _ptr(fs_rows), ld, B, T, N, _stream())
    return (energy, att, att_log, align, fs_rows) if made else (energy, att, att_log, align)


def xattn_softmax_bwd(att, att_log, d_att, d_attlog, ld_dattlog=0):
    """d_attlog may be a strided view (e.g. columns 1..N of the forward-sum gradient rows: pass their pitch as ld_dattlog)."""
    rows, N = att.shape
    d_raw = torch.empty_like(att)
    _lib.call("aptai_xattn_softmax_bwd" if N <= 64 else "aptai_xattn_softmax_bwd_wide", att.data_ptr(), att_log.data_ptr(), _ptr(d_att),
              _ptr(d_attlog), ld_dattlog, d_raw.data_ptr(), rows, N, _stream())
    return d_raw


def layernorm_f32_fwd(x, gamma, beta, eps=1e-5):
    rows, cols = x.shape
    y = torch.empty_like(x)
    mean = torch.empty(rows, device=x.device, dtype=torch.float32)
    rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    _lib.call("aptai_layernorm_f32_fwd", x.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), mean.data_ptr(),
              rstd.data_ptr(), rows, cols, eps, _stream())
    return y, mean, rstd


def layernorm_f32_bwd(dy, x, mean, rstd, gamma):
    rows, cols = x.shape
    dx = torch.empty_like(x)
    dg = torch.empty(cols, device=x.device, dtype=torch.float32)
    db = torch.empty(cols, device=x.device, dtype=torch.float32)
    ws = SCRATCH.get("ln32_bwd", 256 * 2 * cols, x.device, _stream())
    _lib.call("aptai_layernorm_f32_bwd", dy.data_ptr(), x.data_ptr(), mean.data_ptr(), rstd.data_ptr(), gamma.data_ptr(),
              dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), rows, cols, _stream())
    return dx, dg, db


def lstm_status_words(device):
    """int32 device tensor with the status word of every LSTM workspace of this device (None if no LSTM has run): lets a caller
    fold the check into a device->host read it makes anyway (Force_APTAI._lists)."""
    words = [ws[:4].view(torch.int32) for _, ws in SCRATCH.buffers("lstm", device)]
    if not words:
        return None
    return words[0] if len(words) == 1 else torch.cat(words)


def lstm_check(status_host, device) -> None:
    """Raises when a bounded wait of the cooperating LSTM kernels timed out (their output is then incomplete); clears the
    status words so that the next step is judged on its own."""
    if status_host is not None and any(int(v) != 0 for v in status_host):
        for _, ws in SCRATCH.buffers("lstm", device):
            ws[:4].zero_()
        raise _lib.AptaiHipError("aptai_lstm: a cross-workgroup wait of the cooperative BiLSTM kernels timed out "
                                 "(not all 16 workgroups of a cluster were resident together?): hout / dgates are incomplete")


def lstm_status(device) -> int:
    """Non-zero if a bounded wait of the cooperating LSTM kernels ever timed out on this device (synchronises)."""
    w = lstm_status_words(torch.device(device) if not isinstance(device, torch.device) else device)
    return 0 if w is None else int(w.abs().max().item())


_GATE_PERM = {}


def lstm_gate_perm(device):
    """(perm, inv) int64 [2048]: the gate-INTERLEAVED column order of aptai_lstm_fwd / _bwd (xproj, gates, dgates: column
    dir * 1024 + unit * 4 + gate) against torch's gate-major order (dir * 1024 + gate * 256 + unit).  `w[perm]` puts the rows of
    cat(weight_ih_l0, weight_ih_l0_reverse) (or a gate-major vector) into the kernels' order; `t[..., inv]` (or `g[inv]` on rows) brings a
    tensor in the kernels' order back to torch's."""
    key = str(device)
    if key not in _GATE_PERM:
        d, u, g = torch.meshgrid(torch.arange(2), torch.arange(256), torch.arange(4), indexing="ij")
        perm = (d * 1024 + g * 256 + u).reshape(-1)                  # position dir*1024 + unit*4 + gate <- gate-major index
        inv = torch.empty_like(perm)
        inv[perm] = torch.arange(2048)
        _GATE_PERM[key] = (perm.to(device), inv.to(device))
    return _GATE_PERM[key]


def lstm_fwd(xproj, whh, lens_i32, B, Tp, T, save=True):
    """xproj in the gate-interleaved column order (lstm_gate_perm); whh [2][1024][256] (weight_hh_l0 | weight_hh_l0_reverse, as stored).
    Returns (hout [B*Tp][512], gates, cstate); gates in the interleaved order."""
    _dev(xproj, whh, lens_i32)
    dev = xproj.device
    hout = torch.empty((B * Tp, 512), device=dev, dtype=torch.float32)
    gates = torch.empty((B * Tp, 2048), device=dev, dtype=torch.float32) if save else None
    cst = torch.empty((B * Tp, 512), device=dev, dtype=torch.float32) if save else None
    # exchange area of the cooperating LSTM workgroups + status word, per (device, STREAM): two Force_APTAI models, or one model driven
    # from two streams, never share one (zeroed once, at creation; every launch re-zeroes what it uses)
    ws = SCRATCH.get("lstm", _lib.lib().aptai_lstm_workspace_bytes(B), dev, _stream(), torch.uint8, zero=True)
    _lib.call("aptai_lstm_fwd", xproj.data_ptr(), whh.data_ptr(), lens_i32.data_ptr(), hout.data_ptr(), _ptr(gates), _ptr(cst),
              ws.data_ptr(), B, Tp, T, 256, _stream())
    return hout, gates, cst


def lstm_bwd(dhout, whh, lens_i32, gates, cst, B, Tp, T):
    _dev(dhout, whh, lens_i32, gates, cst)
    dgates = torch.empty_like(gates)
    ws = SCRATCH.get("lstm", _lib.lib().aptai_lstm_workspace_bytes(B), dhout.device, _stream(), torch.uint8, zero=True)   # as lstm_fwd
    _lib.call("aptai_lstm_bwd", dhout.data_ptr(), whh.data_ptr(), lens_i32.data_ptr(), gates.data_ptr(), cst.data_ptr(),
              dgates.data_ptr(), ws.data_ptr(), B, Tp, T, 256, _stream())
    return dgates


def lstm_fwd_serial(xproj, whhT, lens_i32, B, Tp, T, save=True):
    """One block per (utterance, direction): cross-check of lstm_fwd (aptai_lstm_fwd_serial); whhT [2][256][1024]."""
    dev = xproj.device
    hout = torch.empty((B * Tp, 512), device=dev, dtype=torch.float32)
    gates = torch.zeros((B * Tp, 2048), device=dev, dtype=torch.float32) if save else None
    cst = torch.zeros((B * Tp, 512), device=dev, dtype=torch.float32) if save else None
    _lib.call("aptai_lstm_fwd_serial", xproj.data_ptr(), whhT.data_ptr(), lens_i32.data_ptr(), hout.data_ptr(), _ptr(gates), _ptr(cst),
              B, Tp, T, 256, _stream())
    return hout, gates, cst


def lstm_bwd_serial(dhout, whh, lens_i32, gates, cst, B, Tp, T):
    dgates = torch.empty_like(gates)
    _lib.call("aptai_lstm_bwd_serial", dhout.data_ptr(), whh.data_ptr(), lens_i32.data_ptr(), gates.data_ptr(), cst.data_ptr(),
              dgates.data_ptr(), B, Tp, T, 256, _stream())
    return dgates


def gather_alignment(ids_i32, align, lens_i32, B, T, N):
    out = torch.empty((B, T), device=align.device, dtype=torch.int64)
    _lib.call("aptai_gather_alignment", ids_i32.data_ptr(), align.data_ptr(), lens_i32.data_ptr(), out.data_ptr(), B, T, N, _stream())
    return out


def tanh_dropout_fwd(x, p, seed):
    y = torch.empty_like(x)
    _lib.call("aptai_tanh_dropout_f32", x.data_ptr(), None, None, y.data_ptr(), x.numel(), p, seed, _stream())
    return y


def tanh_dropout_bwd(y, dy, p, seed):
    dx = torch.empty_like(y)
    _lib.call("aptai_tanh_dropout_f32", None, y.data_ptr(), dy.data_ptr(), dx.data_ptr(), y.numel(), p, seed, _stream())
    return dx


def dropout_f32(x, p, seed):
    if p <= 0:
        return x
    y = torch.empty_like(x)
    _lib.call("aptai_dropout_f32", x.data_ptr(), y.data_ptr(), x.numel(), p, seed, _stream())
    return y


def colsum_f32(x, rows, N, ld=None):
    out = torch.empty(N, device=x.device, dtype=torch.float32)
    ws = SCRATCH.get("colsum", 64 * N, x.device, _stream())
    _lib.call("aptai_colsum_f32", x.data_ptr(), ld if ld else x.stride(0), out.data_ptr(), ws.data_ptr(), rows, N, _stream())
    return out
