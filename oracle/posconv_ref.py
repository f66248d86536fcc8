"""fp64 reference of the positional-convolution block (HF:326-379: weight_norm(dim=2) + grouped Conv1d k = 128 + SamePad + GELU)
and of the operand layouts the kernels of csrc/posconv.hip and csrc/elementwise.hip work on.  TEST INFRASTRUCTURE ONLY.

Two routes to the same numbers:
  * the HF form - `conv_same` (F.conv1d with padding = Kw // 2, last frame removed) and torch autograd through it;
  * the layout form the kernels implement - `pack` to the zero-gapped group-major copy, `toeplitz_matmul` on `wf_layout` (forward)
    or on `wd_layout` one row later (data gradient), `wgrad_frames` (frame-axis contraction, weight gradient in the forward layout).
tests/test_cpu_posconv_ref.py proves the second route equal to the first in fp64; the GPU tests then use the second one, because it
also yields the magnitude sums  mag = sum |a| |b|  that the derived error bounds need.

Layouts (G groups, Cg = H / G channels per group, Kw taps, pad = Kw // 2, rows_p = Tp + 2 pad):
  x   [B*Tp][H]                        row-major activations
  Xg  [G][B][pad | Tp | pad][Cg]       packed copy: frame t of utterance b at row pad + t, zero rows in between
  w   [H][Cg][Kw]                      torch Conv1d weight (out channel, in channel of the group, tap)
  Wf  [G][Cg][kk*Cg + c]      =  w[g*Cg + n][c][kk]                 forward
  Wd  [G][c][(Kw-1-kk)*Cg + n] = w[g*Cg + n][c][kk]                 data gradient: flipped taps, in and out channels swapped
"""
import math

import torch
import torch.nn.functional as F

F64 = torch.float64


# ----------------------------------------------------------------------------------------------------------------- layouts
def pack(x, B, Tp, G, pad):
    """x [B*Tp][H] -> Xg [G][B][pad | Tp | pad][Cg] with zero gap rows (dtype kept)."""
    H = x.shape[1]
    Cg = H // G
    xg = torch.zeros((G, B, Tp + 2 * pad, Cg), dtype=x.dtype)
    xg[:, :, pad:pad + Tp] = x.reshape(B, Tp, G, Cg).permute(2, 0, 1, 3)
    return xg


def unpack(xg, pad):
    """Inverse of `pack` on the interior rows: Xg -> x [B*Tp][H]."""
    G, B, rows_p, Cg = xg.shape
    Tp = rows_p - 2 * pad
    return xg[:, :, pad:pad + Tp].permute(1, 2, 0, 3).reshape(B * Tp, G * Cg)


def wf_layout(w, G):
    """w [H][Cg][Kw] -> Wf [G][Cg][Kw*Cg]."""
    H, Cg, Kw = w.shape
    return w.reshape(G, Cg, Cg, Kw).permute(0, 1, 3, 2).reshape(G, Cg, Kw * Cg).contiguous()


def wf_layout_inv(wf, Kw):
    """Wf [G][Cg][Kw*Cg] -> w [H][Cg][Kw] (reads a weight gradient back from the forward layout)."""
    G, Cg, _ = wf.shape
    return wf.reshape(G, Cg, Kw, Cg).permute(0, 1, 3, 2).reshape(G * Cg, Cg, Kw).contiguous()


def wd_layout(w, G):
    """w [H][Cg][Kw] -> Wd [G][c][(Kw-1-kk)*Cg + n]."""
    H, Cg, Kw = w.shape
    return w.reshape(G, Cg, Cg, Kw).flip(3).permute(0, 2, 3, 1).reshape(G, Cg, Kw * Cg).contiguous()


def wd_layout_inv(wd, Kw):
    G, Cg, _ = wd.shape
    return wd.reshape(G, Cg, Kw, Cg).permute(0, 3, 1, 2).flip(3).reshape(G * Cg, Cg, Kw).contiguous()


# ----------------------------------------------------------------------------------------------------- the layout route
def toeplitz_matmul(xg, w, first_row, Tp, with_mag=False):
    """out[b*Tp + t][g*Cg + n] = sum_k Xg[g][b].flat[(first_row + t)*Cg + k] * W[g][n][k],  k = kk*Cg + c < Kw*Cg.
    first_row = 0 with Wf is the forward, first_row = 1 with Wd on the packed dU is the data gradient.
    with_mag: also returns sum_k |Xg| |W| (the scale of the fp32 accumulation error)."""
    G, B, rows_p, Cg = xg.shape
    Kw = w.shape[2] // Cg
    xg, w = xg.to(F64), w.to(F64)
    out = torch.empty((B * Tp, G * Cg), dtype=F64)
    mag = torch.empty_like(out) if with_mag else None
    for g in range(G):
        # windows [B][Tp][Kw][Cg]: frame first_row + t + kk, channel c
        a = xg[g].unfold(1, Kw, 1)[:, first_row:first_row + Tp].permute(0, 1, 3, 2).reshape(B * Tp, Kw * Cg)
        out[:, g * Cg:(g + 1) * Cg] = a @ w[g].t()
        if with_mag:
            mag[:, g * Cg:(g + 1) * Cg] = a.abs() @ w[g].abs().t()
    return (out, mag) if with_mag else out


def wgrad_frames(dug, xg, pad, with_mag=False):
    """dWf[g][n][kk*Cg + c] = sum_f dUg[g].flat[pad + f][n] * Xg[g].flat[f + kk][c] over the B*rows_p - 2 pad frames of the group's
    one long frame axis (the zero gap rows between utterances take part)."""
    G, B, rows_p, Cg = xg.shape
    Kw = 2 * pad
    frames = B * rows_p - Kw
    dug, xg = dug.to(F64).reshape(G, B * rows_p, Cg), xg.to(F64).reshape(G, B * rows_p, Cg)
    out = torch.empty((G, Cg, Kw * Cg), dtype=F64)
    mag = torch.empty_like(out) if with_mag else None
    for g in range(G):
        win = xg[g].unfold(0, Kw, 1)[:frames].permute(0, 2, 1).reshape(frames, Kw * Cg)
        du = dug[g, pad:pad + frames]
        out[g] = du.t() @ win
        if with_mag:
            mag[g] = du.abs().t() @ win.abs()
    return (out, mag) if with_mag else out


# --------------------------------------------------------------------------------------------------------- the HF route
def conv_same(x, w, bias, B, Tp, G):
    """HF Wav2Vec2PositionalConvEmbedding without the activation: grouped Conv1d, padding = Kw // 2, Wav2Vec2SamePadLayer removes
    the last frame (Kw even).  x [B*Tp][H] -> [B*Tp][H]."""
    H, _, Kw = w.shape
    assert Kw % 2 == 0
    y = F.conv1d(x.reshape(B, Tp, H).transpose(1, 2), w, bias, padding=Kw // 2, groups=G)[:, :, :-1]
    return y.transpose(1, 2).reshape(B * Tp, H)


def weight_norm(v, gain):
    """torch weight_norm(dim=2): one norm per tap over dims (0, 1).  Returns (w, norm [Kw])."""
    norm = v.pow(2).sum((0, 1)).sqrt()
    return v * (gain.reshape(-1) / norm), norm


def gelu_erf(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def gelu_erf_grad(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


# ------------------------------------------------------------------------------------------------------------- numerics
def bf16_round(x):
    """Round to bf16 (nearest even) and return in the input's dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def bf16_ulp(x):
    """Spacing of bf16 numbers at |x| (8 significand bits): 2^(floor(log2 |x|) - 7); the smallest normal's for zero."""
    a = x.abs().to(F64).clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)
