"""GPU, operator level: the small bf16 kernels of csrc/elementwise.hip that feed and drain the positional-conv block - frame masking
forward / backward (with the dembed reduction), the bias-gradient column sums, the standalone GELU backward, elementwise dropout and
the conv-stack weight re-layout - against exact or fp64 references.  fp32 sums are bounded by n 2^-24 sum |x| (any order)."""
import numpy as np
import pytest
import torch

from oracle import posconv_ref as R

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS24 = 2.0 ** -24
DGELU_FIT = 1.3e-4                                       # csrc/common.h: |gelu_fast_grad - exact derivative| over all x


def _bits(x):
    return x.contiguous().view(torch.int16)


# ------------------------------------------------------------------------------------------------ frame masking
@pytest.mark.parametrize("with_spec", [True, False], ids=["spec", "nospec"])
@pytest.mark.parametrize("H", [768, 1024])
def test_frame_mask_forward_and_backward(H, with_spec):
    from aptai_amd import ops
    B, Tp, T = 5, 256, 199
    lens = [0, 1, T, 230, 120]                                            # empty, one frame, full, above T (clamped to T), ragged
    g = torch.Generator().manual_seed(H + with_spec)
    spec = (torch.rand(B, T, generator=g) < 0.3).to(torch.uint8)
    spec[4, 120:] = 1                                                     # set on padded frames: must contribute nothing
    spec[2, 0] = spec[2, T - 1] = spec[1, 0] = 1
    embed = torch.randn(H, generator=g)
    t = torch.arange(Tp)
    valid = t[None, :] < torch.tensor(lens).clamp(max=T)[:, None]         # [B][Tp]
    masked = torch.zeros(B, Tp, dtype=torch.bool)
    if with_spec:
        masked[:, :T] = spec.bool()
    masked &= valid
    lens_d = torch.tensor(lens, dtype=torch.int32).cuda()
    spec_d = spec.cuda() if with_spec else None
    # ---- forward (in place): zeros beyond min(len, T), bf16(embed) on masked valid frames, untouched elsewhere
    h = torch.randn(B * Tp, H, generator=g).to(BF16)
    want = h.clone().view(B, Tp, H)
    want[masked] = embed.to(BF16)
    want[~valid] = 0
    h_d = h.cuda()
    ops.frame_mask_fwd(h_d, lens_d, spec_d, embed.cuda() if with_spec else None, B, Tp, T, H)
    torch.cuda.synchronize()
    assert torch.equal(_bits(h_d.cpu()), _bits(want.view(B * Tp, H)))
    # ---- backward (in place): dy zeroed on padded and masked rows, bit-unchanged elsewhere; dembed = sum over masked valid rows
    dy = torch.randn(B * Tp, H, generator=g).to(BF16)
    want = dy.clone().view(B, Tp, H)
    want[masked | ~valid] = 0
    rows = dy.view(B, Tp, H)[masked].to(F64)                              # [n][H]: what dembed sums
    dy_d = dy.cuda()
    dembed = ops.frame_mask_bwd(dy_d, lens_d, spec_d, B, Tp, T, H, want_dembed=True)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dy_d.cpu()), _bits(want.view(B * Tp, H)))
    if not with_spec:
        assert dembed is None
        return
    n = rows.shape[0]
    assert n > 100
    err = (dembed.cpu().to(F64) - rows.sum(0)).abs()
    bound = n * EPS24 * rows.abs().sum(0)
    r = (err / bound).max().item()
    print(f"[elementwise] frame_mask_bwd H={H}: dembed over {n} rows, max |err| / bound = {r:.4f}")
    assert r <= 1.0, r                                  # measured: 0.0008 (H = 768 and 1024)


# ------------------------------------------------------------------------------------------------ column sums
@pytest.mark.parametrize("N", [4, 48, 768, 1000, 3072])
@pytest.mark.parametrize("rows", [1, 3, 17, 1000, 7984, 8192])
def test_colsum_against_fp64(rows, N):
    """fp32 column sums of `rows` bf16 values: |got - ref| <= rows 2^-24 sum |x| per column, in any summation order.  With
    accumulate=True the pre-filled output is one more term of the same sum."""
    from aptai_amd import ops
    g = torch.Generator().manual_seed(rows * 7 + N)
    wide = (rows, N) == (1000, 1000)                                      # one case with ld > N: NaN in the columns beyond N
    ld = N + 24 if wide else N
    x = torch.randn(rows, ld, generator=g).to(BF16)
    if wide:
        x[:, N:] = float("nan")
    ref, mag = x[:, :N].to(F64).sum(0), x[:, :N].to(F64).abs().sum(0)
    x_d = x.cuda()
    got = ops.colsum(x_d, rows, N, ld=ld)
    pre = torch.randn(N, generator=g) * 10
    acc = ops.colsum(x_d, rows, N, ld=ld, out=pre.clone().cuda(), accumulate=True)
    torch.cuda.synchronize()
    r1 = ((got.cpu().to(F64) - ref).abs() / (rows * EPS24 * mag).clamp_min(1e-300)).max().item()
    r2 = ((acc.cpu().to(F64) - (ref + pre.to(F64))).abs() / ((rows + 1) * EPS24 * (mag + pre.to(F64).abs()))).max().item()
    print(f"[elementwise] colsum rows={rows} N={N}: max |err| / bound = {r1:.4f}, accumulate {r2:.4f}")
    assert r1 <= 1.0 and r2 <= 1.0, (r1, r2)            # measured max over the grid: 0.041, accumulate 0.500 (rows = 1)


def test_colsum_integer_data_is_exact():
    from aptai_amd import ops
    rows, N = 7984, 768
    x = torch.randint(-3, 4, (rows, N), generator=torch.Generator().manual_seed(2)).to(BF16)
    got = ops.colsum(x.cuda(), rows, N).cpu()
    assert torch.equal(got.to(F64), x.to(F64).sum(0))


# ------------------------------------------------------------------------------------------------ GELU backward
def test_dgelu_over_every_bf16_in_range():
    """out = bf16(dy * gelu'(u)) for EVERY bf16 u with |u| <= 9 (+-0, +-7, the clamp's neighbours and the subnormals among them)
    against the exact derivative: one bf16 ulp + 1.3e-4 |dy|, the stated fit error of gelu_fast_grad."""
    from aptai_amd import ops
    allbf = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    u = allbf[allbf.float().abs() <= 9.0]
    for special in (0.0, 7.0, -7.0, 7.03125, -7.03125, 6.96875, -6.96875, 9.0, -9.0):
        assert (u.float() == special).any()
    assert (_bits(u) == 0).any() and (_bits(u) == -32768).any()           # +0 and -0
    dys = torch.tensor([1.0, -0.3701171875, 3.0, -123.0], dtype=BF16)
    uu = u.repeat(len(dys))
    dd = dys.repeat_interleave(len(u))
    pad = (-len(uu)) % 8
    uu, dd = torch.cat([uu, uu[:pad]]), torch.cat([dd, dd[:pad]])
    out = ops.dgelu(dd.cuda(), uu.cuda()).cpu()
    ref = dd.to(F64) * R.gelu_erf_grad(uu.to(F64))
    err = (out.to(F64) - ref).abs()
    bound = R.bf16_ulp(ref) + DGELU_FIT * dd.to(F64).abs()
    r = (err / bound).max().item()
    print(f"[elementwise] dgelu over {len(u)} bf16 inputs x {len(dys)} dy: max |err| / bound = {r:.3f}")
    assert r <= 1.0, (r, uu[(err / bound).argmax()].item())           # measured: 0.677


# ------------------------------------------------------------------------------------------------ dropout
def test_dropout_mask_scale_and_tail():
    from aptai_amd import ops
    n, p, seed = 1 << 20, 0.1, 1234
    thr = round(p * 65536)
    scale = np.float32(65536.0) / np.float32(65536 - thr)                 # the scale rule tests/test_gpu_norm_attn.py states, in fp32
    ones = torch.ones(n, dtype=BF16).cuda()
    y1 = ops.dropout(ones, p, seed).cpu()
    drop = y1.float() == 0
    assert torch.equal(y1[~drop].float(), torch.full((int((~drop).sum()),), float(scale)).to(BF16).float())
    frac = drop.float().mean().item()
    sigma = (p * (1 - p) / n) ** 0.5
    print(f"[elementwise] dropout: dropped fraction {frac:.6f} (p = {p}, 3 sigma = {3 * sigma:.6f})")
    assert abs(frac - p) <= 3 * sigma, frac
    x = torch.randn(n, generator=torch.Generator().manual_seed(9)).to(BF16)
    x[x == 0] = 1.0
    y = ops.dropout(x.cuda(), p, seed).cpu()
    want = (x.float() * torch.tensor(scale)).to(BF16)
    want[drop] = 0
    # zero exactly where the mask is (the 8-wide path leaves x * 0 = -0 for negative x: compared by value), bf16(x * scale) elsewhere
    bad = (y.float() != want.float()).nonzero()
    assert len(bad) == 0, f"{len(bad)} of {n} elements differ, first at {bad[0].item()}: {y[bad[0]].item()} vs {want[bad[0]].item()}"
    assert (y.float()[drop] == 0).all() and (y.float()[~drop] != 0).all()
    drop2 = ops.dropout(ones, p, seed + 1).cpu().float() == 0
    differ = (drop ^ drop2).float().mean().item()
    assert abs(differ - 2 * p * (1 - p)) < 0.01, differ                   # another seed: an independent mask
    # the vector path (8 elements per thread) and the scalar tail define the same mask by logical index
    k8 = 8 * 1000
    xs = x[:k8 + 8].cuda()
    y_full, y_tail, y_head = ops.dropout(xs, p, seed).cpu(), ops.dropout(xs[:k8 + 5], p, seed).cpu(), ops.dropout(xs[:k8], p, seed).cpu()
    assert torch.equal(_bits(y_tail[:k8]), _bits(y_head))                 # bit for bit
    assert torch.equal(y_tail.float(), y_full[:k8 + 5].float())           # the scalar tail writes +0 where the 8-wide path has x * 0
    assert torch.equal(_bits(y_full), _bits(y[:k8 + 8]))


# ------------------------------------------------------------------------------------------------ conv weight re-layout
@pytest.mark.parametrize("N,C,Kw", [(512, 512, 3), (512, 1, 10)])
def test_conv_weight_bf16_layout(N, C, Kw):
    """conv_weight_kernel: dst[n][kw*C + c] = bf16(src[n][c][kw]) (K index kw*C + c matches channels-last frames)."""
    from aptai_amd import ops
    w = torch.randn(N, C, Kw, generator=torch.Generator().manual_seed(C))
    got = ops.conv_weight_bf16(w.cuda()).cpu()
    assert got.shape == (N, Kw * C)
    assert torch.equal(_bits(got), _bits(w.permute(0, 2, 1).reshape(N, Kw * C).to(BF16)))
