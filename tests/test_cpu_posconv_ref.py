"""CPU: the reference helper of the positional-conv tests (oracle/posconv_ref.py) checked where it can be checked - the layout
route the kernels implement (pack -> Toeplitz matmul on Wf; Wd one row later; frame-axis contraction for dW) against
F.conv1d(groups=G) + torch autograd in fp64, at the real constants (Kw = 128, pad = 64, Cg in {48, 64})."""
import pytest
import torch
import torch.nn.functional as F

from oracle import posconv_ref as R

KW, PAD, G, B, TP = 128, 64, 2, 2, 128


def _rel(got, ref):
    return ((got - ref).abs().max() / ref.abs().max()).item()


@pytest.mark.parametrize("Cg", [48, 64])
def test_layout_route_equals_grouped_conv1d_and_autograd(Cg):
    H = G * Cg
    g = torch.Generator().manual_seed(Cg)
    x = torch.randn(B * TP, H, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(H, Cg, KW, generator=g, dtype=torch.float64, requires_grad=True)
    bias = torch.randn(H, generator=g, dtype=torch.float64)
    du = torch.randn(B * TP, H, generator=g, dtype=torch.float64)
    y = R.conv_same(x, w, bias, B, TP, G)
    assert y.shape == (B * TP, H)
    # SamePad semantics written out: y[t] = sum_kk w[:, :, kk] x[t + kk - 64], one utterance never sees the other
    t, o = 5, Cg + 3
    xs = x.detach().reshape(B, TP, H)[1, :, Cg:2 * Cg]
    direct = sum((w.detach()[o, :, kk] * xs[t + kk - PAD]).sum() for kk in range(KW) if 0 <= t + kk - PAD < TP) + bias[o]
    assert abs(direct.item() - y[TP + t, o].item()) <= 1e-12 * abs(direct.item())
    y.backward(du)
    xg, dug = R.pack(x.detach(), B, TP, G, PAD), R.pack(du, B, TP, G, PAD)
    wf, wd = R.wf_layout(w.detach(), G), R.wd_layout(w.detach(), G)
    assert _rel(R.toeplitz_matmul(xg, wf, 0, TP) + bias, y.detach()) <= 1e-12
    assert _rel(R.toeplitz_matmul(dug, wd, 1, TP), x.grad) <= 1e-12
    assert _rel(R.wf_layout_inv(R.wgrad_frames(dug, xg, PAD), KW), w.grad) <= 1e-12
    # mag is the same contraction on absolute values
    _, mag = R.toeplitz_matmul(xg, wf, 0, TP, with_mag=True)
    assert _rel(mag, R.conv_same(x.detach().abs(), w.detach().abs(), None, B, TP, G)) <= 1e-12
    _, magw = R.wgrad_frames(dug, xg, PAD, with_mag=True)
    assert (magw >= R.wgrad_frames(dug, xg, PAD).abs() * (1 - 1e-12)).all()


def test_layouts_are_permutations_with_the_documented_indices():
    Cg = 48
    H = G * Cg
    w = torch.arange(H * Cg * KW, dtype=torch.float64).reshape(H, Cg, KW)
    wf, wd = R.wf_layout(w, G), R.wd_layout(w, G)
    for (grp, n, c, kk) in [(0, 0, 0, 0), (1, 47, 5, 127), (1, 3, 46, 64), (0, 17, 1, 1)]:
        assert wf[grp, n, kk * Cg + c] == w[grp * Cg + n, c, kk]
        assert wd[grp, c, (KW - 1 - kk) * Cg + n] == w[grp * Cg + n, c, kk]
    assert torch.equal(R.wf_layout_inv(wf, KW), w) and torch.equal(R.wd_layout_inv(wd, KW), w)
    x = torch.arange(B * TP * H, dtype=torch.float64).reshape(B * TP, H) + 1
    xg = R.pack(x, B, TP, G, PAD)
    assert xg.shape == (G, B, TP + 2 * PAD, Cg)
    assert xg[1, 1, PAD + 7, 5] == x[TP + 7, Cg + 5]
    assert xg[:, :, :PAD].abs().sum() == 0 and xg[:, :, PAD + TP:].abs().sum() == 0
    assert torch.equal(R.unpack(xg, PAD), x)


def test_weight_norm_and_gelu_against_torch():
    g = torch.Generator().manual_seed(3)
    v = torch.randn(96, 48, KW, generator=g, dtype=torch.float64)
    gain = torch.rand(1, 1, KW, generator=g, dtype=torch.float64) + 0.5
    w, norm = R.weight_norm(v, gain)
    assert _rel(w, torch._weight_norm(v, gain, 2)) <= 1e-14
    assert _rel(norm, torch.norm_except_dim(v, 2, 2).reshape(-1)) <= 1e-14
    x = torch.linspace(-9, 9, 3601, dtype=torch.float64, requires_grad=True)
    y = F.gelu(x)
    assert (R.gelu_erf(x.detach()) - y.detach()).abs().max().item() <= 1e-15
    y.sum().backward()
    assert (R.gelu_erf_grad(x.detach()) - x.grad).abs().max().item() <= 1e-15


def test_bf16_helpers():
    x = torch.tensor([1.0, 1.00390625, 1.5, 255.0, 256.0, -3.0, 0.0], dtype=torch.float64)
    assert R.bf16_ulp(x).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 1.0, 2.0, 2.0 ** -6, 2.0 ** -133]
    assert R.bf16_round(torch.tensor([1.00390625 + 1e-6, 257.0], dtype=torch.float64)).tolist() == [1.0078125, 256.0]
