"""GPU, operator level: the positional-convolution block (csrc/posconv.hip: posconv_kernel, posconv64_kernel, posconv_wgrad_kernel;
csrc/elementwise.hip: pack, weight norm forward / backward) against the fp64 reference of oracle/posconv_ref.py, which
tests/test_cpu_posconv_ref.py proves equal to F.conv1d(groups) + autograd.

Inputs are rounded to bf16 on the host, so reference and kernel see the same numbers.  Tolerances are derived, not measured:
  fp32 accumulation of n products, any order:   |err| <= n 2^-24 mag,  mag = sum |a| |b|  (computed in fp64 beside every reference)
  one bf16 output rounding:                      |err| <= 2^-8 |ref|
Exact cases use small integers, for which every partial sum is exact in fp32 and every output exact in bf16: torch.equal.
The largest observed error-to-bound ratios are recorded beside the assertions ("# measured ...")."""
import pytest
import torch

from oracle import posconv_ref as R

pytestmark = pytest.mark.gpu

KW, PAD, G = 128, 64, 16
BASE, LARGE = 48, 64                                     # channels per group: H = 768 / 1024
SHAPES = [(BASE, 1, 128), (BASE, 2, 256), (BASE, 3, 384), (BASE, 2, 1536), (LARGE, 1, 128), (LARGE, 2, 512)]
SHAPES_B2 = [s for s in SHAPES if s[1] >= 2]
BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
EPS24, EPS8 = 2.0 ** -24, 2.0 ** -8
GELU_FIT, DGELU_FIT = 3.3e-5, 1.3e-4                     # csrc/common.h: |gelu_fast - erf form|, |gelu_fast_grad - exact| over all x
NAN_BITS, SENT_BITS = 0x7FC0, 0x7B7B                     # bf16 quiet NaN; bf16 sentinel 1.30e36 (both fit a positive int16)
SENT_F32 = -12345.0


def _id(s):
    return f"Cg{s[0]}-B{s[1]}-Tp{s[2]}"


def _lens(B, Tp):
    return [Tp - 61 * b - (29 if B == 1 else 0) for b in range(B)]           # first utterance full (B > 1), the others ragged


def _zero_beyond(x, lens, Tp):
    x = x.view(len(lens), Tp, -1)
    for b, L in enumerate(lens):
        x[b, L:] = 0
    return x.view(len(lens) * Tp, -1)


def _packed_dev(xg_cpu):
    """The packed copy as the model allocates it: flat, zero-initialised, Cg*8 elements of slack behind it."""
    Cg = xg_cpu.shape[-1]
    buf = torch.zeros(xg_cpu.numel() + Cg * 8, dtype=xg_cpu.dtype, device="cuda")
    buf[:xg_cpu.numel()] = xg_cpu.reshape(-1).cuda()
    return buf


def _batch(Cg, B, Tp):
    """The batch strides of the implicit-GEMM path, as aptai_amd/wav2vec2.py::_EmbedStage._posconv_batch builds them."""
    H, rows_p, K = G * Cg, Tp + 2 * PAD, KW * Cg
    return dict(outer=B, inner=G, a=(rows_p * Cg, B * rows_p * Cg), b=(0, Cg * K), c=(Tp * H, Cg),
                bias=(0, Cg), res=(Tp * H, Cg), aux=(Tp * H, Cg))


def _fwd_gemm_path(xg, wf, out, B, Tp, Cg, **kw):
    """Forward / data gradient through the batched implicit GEMM, the call wav2vec2.py makes when posconv_kernel_fits is false."""
    from aptai_amd import ops
    H, K = G * Cg, KW * Cg
    if kw.get("residual") is not None:
        kw["ldr"] = H
    return ops.gemm(xg, wf, Tp, Cg, K, lda=Cg, ldb=K, out=out, ldc=H, batch=_batch(Cg, B, Tp), **kw)


def _wgrad_gemm_path(dug, xg, dwf, B, Tp, Cg):
    """Weight gradient as the TN GEMM over the group's one long frame axis (wav2vec2-large's path on every step)."""
    from aptai_amd import ops
    rows_p, K = Tp + 2 * PAD, KW * Cg
    kred = B * rows_p - 2 * PAD
    return ops.gemm(dug[PAD * Cg:], xg, Cg, K, kred, a_kmajor=True, b_kmajor=True, out_f32=True, lda=Cg, ldb=Cg, out=dwf, ldc=K,
                    batch=dict(outer=1, inner=G, a=(0, B * rows_p * Cg), b=(0, B * rows_p * Cg), c=(0, Cg * K)))


def _ratio(got, ref, bound):
    """Largest |got - ref| / bound; entries with a zero bound must be exact."""
    err = (got.to(F64) - ref).abs()
    assert torch.isfinite(err).all()
    zero = bound == 0
    assert (err[zero] == 0).all(), "error where the bound is zero"
    return (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0


# ------------------------------------------------------------------------------------------------ random data, one per shape
@pytest.fixture(scope="module")
def cases():
    """Random bf16 data + fp64 references per shape, computed once and reused by (c), (d), (e) and (h)."""
    cache = {}

    def get(shape):
        if shape in cache:
            return cache[shape]
        Cg, B, Tp = shape
        H = G * Cg
        g = torch.Generator().manual_seed(1000 * Cg + 10 * Tp + B)
        c = dict(Cg=Cg, B=B, Tp=Tp, H=H, lens=_lens(B, Tp))
        c["x"] = _zero_beyond(torch.randn(B * Tp, H, generator=g), c["lens"], Tp).to(BF16)
        c["du"] = _zero_beyond(torch.randn(B * Tp, H, generator=g), c["lens"], Tp).to(BF16)
        c["res"] = torch.randn(B * Tp, H, generator=g).to(BF16)
        c["w"] = (torch.randn(H, Cg, KW, generator=g) * 0.05).to(BF16)
        c["bias"] = torch.randn(H, generator=g) * 0.5
        c["xg"], c["dug"] = R.pack(c["x"], B, Tp, G, PAD), R.pack(c["du"], B, Tp, G, PAD)
        c["wf"], c["wd"] = R.wf_layout(c["w"], G), R.wd_layout(c["w"], G)
        c["fwd"], c["fwd_mag"] = R.toeplitz_matmul(c["xg"], c["wf"], 0, Tp, with_mag=True)
        c["dx"], c["dx_mag"] = R.toeplitz_matmul(c["dug"], c["wd"], 1, Tp, with_mag=True)
        if B >= 2:
            c["dw"], c["dw_mag"] = R.wgrad_frames(c["dug"], c["xg"], PAD, with_mag=True)
        cache[shape] = c
        return c
    return get


def _run_fwd(c, path="kernel"):
    """bias + GELU + residual + out_pre, the forward exactly as the model runs it.  Returns (out, out_pre) on the host."""
    from aptai_amd import ops
    Cg, B, Tp, H = c["Cg"], c["B"], c["Tp"], c["H"]
    xg, wf = _packed_dev(c["xg"]), c["wf"].cuda()
    out = torch.empty((B * Tp, H), dtype=BF16, device="cuda")
    pre = torch.empty_like(out)
    if path == "kernel":
        ops.posconv_gemm(xg, wf, out, B, Tp, H, G, KW, PAD, bias=c["bias"].cuda(), gelu=True, residual=c["x"].cuda(), out_pre=pre)
    else:
        _fwd_gemm_path(xg, wf, out, B, Tp, Cg, bias=c["bias"].cuda(), gelu=True, residual=c["x"].cuda(), out_pre=pre)
    torch.cuda.synchronize()
    return out.cpu(), pre.cpu()


def _run_dgrad(c, path="kernel", out_pre=True):
    """residual only (the model's call); out_pre is added by the test to see the convolution before the epilogue."""
    from aptai_amd import ops
    Cg, B, Tp, H = c["Cg"], c["B"], c["Tp"], c["H"]
    dug, wd = _packed_dev(c["dug"]), c["wd"].cuda()
    out = torch.empty((B * Tp, H), dtype=BF16, device="cuda")
    pre = torch.empty_like(out) if out_pre else None
    if path == "kernel":
        ops.posconv_gemm(dug, wd, out, B, Tp, H, G, KW, PAD, first_row=1, residual=c["res"].cuda(), out_pre=pre)
    else:
        _fwd_gemm_path(dug[Cg:], wd, out, B, Tp, Cg, residual=c["res"].cuda(), out_pre=pre)
    torch.cuda.synchronize()
    return out.cpu(), (pre.cpu() if out_pre else None)


def _run_wgrad(c, path="kernel"):
    from aptai_amd import ops
    Cg, B, Tp, H = c["Cg"], c["B"], c["Tp"], c["H"]
    dug, xg = _packed_dev(c["dug"]), _packed_dev(c["xg"])
    dwf = torch.full((G, Cg, KW * Cg), SENT_F32, dtype=F32, device="cuda")
    if path == "kernel":
        ops.posconv_wgrad(dug, xg, dwf, B, Tp, H, G, KW, PAD)
    else:
        _wgrad_gemm_path(dug, xg, dwf, B, Tp, Cg)
    torch.cuda.synchronize()
    return dwf.cpu()


# ------------------------------------------------------------------------------------------------ (a) exact: forward, dgrad
def _one_hot_frames(B, Tp, Cg, g):
    """Exactly one nonzero channel (+-1) per frame per group."""
    idx = torch.randint(0, Cg, (B * Tp, G, 1), generator=g)
    sign = torch.randint(0, 2, (B * Tp, G, 1), generator=g).to(F32) * 2 - 1
    return torch.zeros(B * Tp, G, Cg).scatter_(2, idx, sign).reshape(B * Tp, G * Cg).to(BF16)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_integer_data_forward_and_dgrad_are_exact(shape):
    """w in {-2..2}, one +-1 per frame per group: every output is an integer, |y| <= 2 * 128 = 256, exact in fp32 accumulation in
    any order and exactly representable in bf16.  A dropped, doubled or misplaced term changes an integer: no tolerance hides it.
    Every frame carries data, so every blockIdx.x and every K-tile (96 of 64 k at Cg = 48, 128 taps at Cg = 64) matters."""
    from aptai_amd import ops
    Cg, B, Tp = shape
    H = G * Cg
    g = torch.Generator().manual_seed(7 * Cg + Tp + B)
    w = torch.randint(-2, 3, (H, Cg, KW), generator=g).to(BF16)
    x, du = _one_hot_frames(B, Tp, Cg, g), _one_hot_frames(B, Tp, Cg, g)
    xg, dug = R.pack(x, B, Tp, G, PAD), R.pack(du, B, Tp, G, PAD)
    wf, wd = R.wf_layout(w, G), R.wd_layout(w, G)
    ref_y, ref_dx = R.toeplitz_matmul(xg, wf, 0, Tp), R.toeplitz_matmul(dug, wd, 1, Tp)
    assert ref_y.abs().max() <= 256 and ref_dx.abs().max() <= 256 and ref_y.abs().max() > 16
    y = torch.empty((B * Tp, H), dtype=BF16, device="cuda")
    dx = torch.empty_like(y)
    ops.posconv_gemm(_packed_dev(xg), wf.cuda(), y, B, Tp, H, G, KW, PAD, first_row=0)
    ops.posconv_gemm(_packed_dev(dug), wd.cuda(), dx, B, Tp, H, G, KW, PAD, first_row=1)
    for name, got, ref in (("forward", y, ref_y), ("dgrad", dx, ref_dx)):
        got = got.cpu().to(F64)
        bad = (got != ref).nonzero()
        assert torch.equal(got, ref), f"{name}: {len(bad)} of {ref.numel()} outputs differ, first at (row, col) {bad[0].tolist()}"


# ------------------------------------------------------------------------------------------------ (b) exact: weight gradient
@pytest.mark.parametrize("shape", SHAPES_B2, ids=_id)
def test_integer_data_wgrad_is_exact(shape):
    """dU in {-1, 0, 1}, x in {-2..2}, B >= 2 so the zero gap rows between utterances lie inside the frame axis: every one of the
    G x Cg x 128 Cg fp32 outputs is an integer below 2^24, exact in any summation order.  Cg = 48: the dedicated kernel and the TN GEMM
    path; Cg = 64: the TN GEMM path (lda = Cg < K), which is what wav2vec2-large runs."""
    Cg, B, Tp = shape
    H = G * Cg
    g = torch.Generator().manual_seed(11 * Cg + Tp + B)
    c = dict(Cg=Cg, B=B, Tp=Tp, H=H)
    du = torch.randint(-1, 2, (B * Tp, H), generator=g).to(BF16)
    x = torch.randint(-2, 3, (B * Tp, H), generator=g).to(BF16)
    c["dug"], c["xg"] = R.pack(du, B, Tp, G, PAD), R.pack(x, B, Tp, G, PAD)
    ref = R.wgrad_frames(c["dug"], c["xg"], PAD)
    assert ref.abs().max() < 2 ** 24 and ref.abs().max() > 16
    for path in (("kernel", "gemm") if Cg == BASE else ("gemm",)):
        got = _run_wgrad(c, path).to(F64)
        bad = (got != ref).nonzero()
        assert torch.equal(got, ref), f"{path}: {len(bad)} of {ref.numel()} entries differ, first at (grp, n, k) {bad[0].tolist()}"


# ------------------------------------------------------------------------------------------------ (c) random data, derived bound
def _check_conv_bound(name, pre, ref, mag, Cg):
    """|got - ref| <= 2^-8 |ref| + n 2^-24 mag, n = 128 Cg products per output: fp32 accumulation in any order + one bf16 rounding."""
    bound = EPS8 * ref.abs() + KW * Cg * EPS24 * mag
    r = _ratio(pre, ref, bound)
    print(f"[posconv] {name}: max |err| / bound = {r:.3f}")
    assert r <= 1.0, (name, r)
    return r


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_random_data_forward_and_dgrad_within_the_accumulation_bound(cases, shape):
    c = cases(shape)
    _, pre = _run_fwd(c)
    _check_conv_bound(f"{_id(shape)} forward out_pre", pre, c["fwd"] + c["bias"].to(F64), c["fwd_mag"], c["Cg"])
    _, dpre = _run_dgrad(c)
    _check_conv_bound(f"{_id(shape)} dgrad out_pre", dpre, c["dx"], c["dx_mag"], c["Cg"])
    # measured max |err| / bound over the six shapes: forward 0.994 (Cg48-B3-Tp384; the bf16 rounding term alone reaches ~1: 2^-8 is
    # the unit roundoff), dgrad 0.754.  The accumulation term stays far from its worst case, as the fp32-output wgrad below shows.


@pytest.mark.parametrize("shape", SHAPES_B2, ids=_id)
def test_random_data_wgrad_within_the_accumulation_bound(cases, shape):
    """fp32 output, no rounding term: |got - ref| <= n 2^-24 mag with n = B (Tp + 128) - 128 frames."""
    c = cases(shape)
    n = c["B"] * (c["Tp"] + 2 * PAD) - 2 * PAD
    for path in (("kernel", "gemm") if c["Cg"] == BASE else ("gemm",)):
        r = _ratio(_run_wgrad(c, path), c["dw"], n * EPS24 * c["dw_mag"])
        print(f"[posconv] {_id(shape)} wgrad ({path}): max |err| / bound = {r:.3f}")
        assert r <= 1.0, (path, r)                      # measured max over the shapes: kernel 0.003, TN GEMM 0.003


# ------------------------------------------------------------------------------------------------ (d) epilogue
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_epilogues_the_model_uses(cases, shape):
    """forward: bias + GELU + residual + out_pre; data gradient: residual only.  out = bf16(gelu_fast(pre_fp32) + residual) with
    pre_fp32 within n 2^-24 mag of the reference, |gelu'| <= 1.13, |gelu_fast - gelu_erf| <= 3.3e-5 (common.h), one bf16 rounding."""
    c = cases(shape)
    Cg, n = c["Cg"], KW * c["Cg"]
    out, pre = _run_fwd(c)
    ref_pre = c["fwd"] + c["bias"].to(F64)
    ref_out = R.gelu_erf(ref_pre) + c["x"].to(F64)
    r = _ratio(out, ref_out, 1.13 * n * EPS24 * c["fwd_mag"] + GELU_FIT + EPS8 * ref_out.abs())
    print(f"[posconv] {_id(shape)} forward out (gelu + residual): max |err| / bound = {r:.3f}")
    assert r <= 1.0, r                                  # measured max over the shapes: 0.933
    # out_pre = conv + bias: no GELU, no residual (the bound of (c); a GELU or the residual leaking in is O(1) off)
    _check_conv_bound(f"{_id(shape)} out_pre beside gelu + residual", pre, ref_pre, c["fwd_mag"], Cg)
    # data gradient: conv + residual, one rounding
    dout, _ = _run_dgrad(c, out_pre=False)
    ref_dout = c["dx"] + c["res"].to(F64)
    r = _ratio(dout, ref_dout, n * EPS24 * c["dx_mag"] + EPS8 * ref_dout.abs())
    print(f"[posconv] {_id(shape)} dgrad out (residual): max |err| / bound = {r:.3f}")
    assert r <= 1.0, r                                  # measured max over the shapes: 0.857
    # without out_pre the output is the same bits as with it
    assert torch.equal(dout, _run_dgrad(c)[0])


# ------------------------------------------------------------------------------------------------ (e) guard bands
def _guarded(t, before, after, bits=None, value=None):
    """`t` as an interior slice of a larger device buffer whose slack holds a bf16 bit pattern (or an fp32 value).
    before / after in elements (multiples of 8: the operand keeps its 16-byte alignment).  Returns (buffer, view)."""
    flat = t.reshape(-1)
    if t.dtype == BF16:
        buf = torch.full((before + flat.numel() + after,), bits, dtype=torch.int16).view(BF16).cuda()
    else:
        buf = torch.full((before + flat.numel() + after,), value, dtype=t.dtype, device="cuda")
    view = buf[before:before + flat.numel()]
    view.copy_(flat.cuda())
    return buf, view.view(t.shape)


def _slack_intact(buf, before, n, bits=None, value=None):
    if buf.dtype == BF16:
        raw = buf.view(torch.int16).cpu()
        return bool((raw[:before] == bits).all() and (raw[before + n:] == bits).all())
    return bool((buf[:before] == value).all() and (buf[before + n:] == value).all())


GUARD = 4096                                            # elements of slack around every operand but the packed copy's tail


@pytest.mark.parametrize("shape", [(BASE, 2, 1536), (LARGE, 2, 512)], ids=_id)
def test_guard_bands_no_read_or_write_outside_the_operands(cases, shape):
    """Every operand is an interior slice of a larger allocation: NaN around the inputs (behind the packed copies exactly the Cg*8
    elements the model allocates), a sentinel around the outputs.  A read outside an operand that reaches an accumulator turns
    outputs into NaN, a write outside the output changes a sentinel.  Only allocated memory is touched."""
    from aptai_amd import ops
    c = cases(shape)
    Cg, B, Tp, H = c["Cg"], c["B"], c["Tp"], c["H"]
    M = B * Tp
    _, xg = _guarded(c["xg"], GUARD, Cg * 8, bits=NAN_BITS)
    _, dug = _guarded(c["dug"], GUARD, Cg * 8, bits=NAN_BITS)
    _, wf = _guarded(c["wf"], GUARD, GUARD, bits=NAN_BITS)
    _, wd = _guarded(c["wd"], GUARD, GUARD, bits=NAN_BITS)
    _, x = _guarded(c["x"], GUARD, GUARD, bits=NAN_BITS)
    _, res = _guarded(c["res"], GUARD, GUARD, bits=NAN_BITS)
    _, bias = _guarded(c["bias"], GUARD, GUARD, value=float("nan"))
    sent = torch.zeros((M, H), dtype=BF16)
    bufs = {k: _guarded(sent, GUARD, GUARD, bits=SENT_BITS) for k in ("out", "pre", "dout")}
    ops.posconv_gemm(xg.view(-1), wf, bufs["out"][1], B, Tp, H, G, KW, PAD, bias=bias, gelu=True, residual=x, out_pre=bufs["pre"][1])
    ops.posconv_gemm(dug.view(-1), wd, bufs["dout"][1], B, Tp, H, G, KW, PAD, first_row=1, residual=res)
    torch.cuda.synchronize()
    ref_out, ref_pre = _run_fwd(c)
    ref_dout, _ = _run_dgrad(c, out_pre=False)
    for k, ref in (("out", ref_out), ("pre", ref_pre), ("dout", ref_dout)):
        buf, view = bufs[k]
        got = view.cpu()
        assert not torch.isnan(got.float()).any(), f"{k}: NaN from outside an operand reached the output"
        assert torch.equal(got, ref), f"{k}: differs from the run on plain buffers"
        assert _slack_intact(buf, GUARD, M * H, bits=SENT_BITS), f"{k}: a write outside the output"
    if Cg != BASE:
        return
    dw_buf, dw = _guarded(torch.zeros((G, Cg, KW * Cg), dtype=F32), GUARD, GUARD, value=SENT_F32)
    ops.posconv_wgrad(dug.view(-1), xg.view(-1), dw, B, Tp, H, G, KW, PAD)
    torch.cuda.synchronize()
    got = dw.cpu()
    assert not torch.isnan(got).any(), "wgrad: NaN from outside an operand reached the output"
    assert torch.equal(got, _run_wgrad(c)), "wgrad: differs from the run on plain buffers"
    assert _slack_intact(dw_buf, GUARD, dw.numel(), value=SENT_F32), "wgrad: a write outside the output"


# ------------------------------------------------------------------------------------------------ (f) pack
@pytest.mark.parametrize("shape", [(BASE, 3, 384), (LARGE, 2, 512)], ids=_id)
def test_pack_writes_the_interior_and_never_the_gap_rows(cases, shape):
    from aptai_amd import ops
    c = cases(shape)
    Cg, B, Tp, H = c["Cg"], c["B"], c["Tp"], c["H"]
    rows_p = Tp + 2 * PAD
    n = G * B * rows_p * Cg
    buf, xg = _guarded(torch.zeros(n, dtype=BF16), GUARD, Cg * 8, bits=SENT_BITS)
    xg.view(torch.int16).fill_(SENT_BITS)
    ops.posconv_pack(c["x"].cuda(), xg, B, Tp, H, G, PAD)
    torch.cuda.synchronize()
    got = xg.cpu().view(torch.int16).view(G, B, rows_p, Cg)
    want = R.pack(c["x"], B, Tp, G, PAD).view(torch.int16)
    assert torch.equal(got[:, :, PAD:PAD + Tp], want[:, :, PAD:PAD + Tp])                      # interior: the source, bit for bit
    assert (got[:, :, :PAD] == SENT_BITS).all() and (got[:, :, PAD + Tp:] == SENT_BITS).all()            # gap rows: never written
    assert _slack_intact(buf, GUARD, n, bits=SENT_BITS)
    # ---- with u and rowmajor_out: du = bf16(dy * gelu'(u)), the packed and the row-major copy bit-equal
    g = torch.Generator().manual_seed(Tp + Cg)
    u = (torch.randn(B * Tp, H, generator=g) * 2.5).to(BF16)
    u.view(-1)[:8] = torch.tensor([0.0, -0.0, 7.0, -7.0, 7.03125, -7.03125, 6.96875, -6.96875]).to(BF16)
    dy = c["du"]
    dug = torch.zeros(n + Cg * 8, dtype=BF16, device="cuda")
    rm = torch.empty((B * Tp, H), dtype=BF16, device="cuda")
    ops.posconv_pack(dy.cuda(), dug, B, Tp, H, G, PAD, u=u.cuda(), rowmajor_out=rm)
    torch.cuda.synchronize()
    dug_c, rm = dug.cpu(), rm.cpu()
    packed = dug_c[:n].view(G, B, rows_p, Cg)
    assert torch.equal(R.unpack(packed, PAD).view(torch.int16), rm.view(torch.int16))
    assert packed[:, :, :PAD].abs().sum() == 0 and packed[:, :, PAD + Tp:].abs().sum() == 0 and dug_c[n:].abs().sum() == 0
    ref = dy.to(F64) * R.gelu_erf_grad(u.to(F64))
    r = _ratio(rm, ref, R.bf16_ulp(ref) + DGELU_FIT * dy.to(F64).abs())    # one bf16 ulp + the stated fit error of gelu_fast_grad
    print(f"[posconv] {_id(shape)} pack(u): max |err| / bound = {r:.3f}")
    assert r <= 1.0, r                                  # measured: 0.861 at both shapes


# ------------------------------------------------------------------------------------------------ (g) weight norm
@pytest.mark.parametrize("Cg", [BASE, LARGE])
def test_weight_norm_forward_and_backward(Cg):
    from aptai_amd import ops
    H = G * Cg
    g = torch.Generator().manual_seed(Cg)
    v = torch.randn(H, Cg, KW, generator=g) * 0.1
    gain = torch.rand(KW, generator=g) + 0.5
    wf, wd, norm = ops.posconv_weight(v.cuda(), gain.cuda(), G)
    torch.cuda.synchronize()
    w_ref, norm_ref = R.weight_norm(v.to(F64), gain.to(F64))
    assert ((norm.cpu().to(F64) - norm_ref).abs() / norm_ref).max().item() <= 1e-6
    wf, wd = wf.cpu(), wd.cpu()
    for name, got, ref in (("Wf", wf, R.wf_layout(w_ref, G)), ("Wd", wd, R.wd_layout(w_ref, G))):
        err = (got.to(F64) - R.bf16_round(ref)).abs()
        assert (err <= R.bf16_ulp(ref)).all(), name       # within one bf16 ulp of bf16(ref)
        assert (err != 0).float().mean().item() < 0.01, name     # ... and almost always the same bf16 number
    assert torch.equal(wd.view(torch.int16), R.wd_layout(R.wf_layout_inv(wf, KW), G).view(torch.int16))     # the two layouts agree
    # ---- backward: dv, dgain from a random weight gradient in the forward layout, against fp64 autograd of g v / ||v||
    dwf = torch.randn(G, Cg, KW * Cg, generator=g)
    dv, dgain = ops.posconv_weight_bwd(dwf.cuda(), v.cuda(), gain.cuda(), norm, G)
    torch.cuda.synchronize()
    v64, g64 = v.to(F64).requires_grad_(True), gain.to(F64).requires_grad_(True)
    dW = R.wf_layout_inv(dwf.to(F64), KW)
    R.weight_norm(v64, g64)[0].backward(dW)
    # dot[kk] = sum_{o,c} dW v is an fp32 sum of n = H Cg products: |err| <= n 2^-24 mag_dot, as in (c).  It enters dgain = dot / norm
    # and dv = gain / norm (dW - v dot / norm^2).  On top: the norm is within eps_n = 1e-6 (asserted above; it enters dgain once and
    # dv's two terms up to three times) and each of the <= 6 elementwise fp32 operations rounds once (2^-24 each).
    n, eps_n = H * Cg, 1e-6
    mag_dot = (dW.abs() * v.to(F64).abs()).sum((0, 1))
    gn = (gain.to(F64) / norm_ref)
    b_gain = n * EPS24 * mag_dot / norm_ref + (eps_n + 2 * EPS24) * g64.grad.abs()
    dot = (dW * v.to(F64)).sum((0, 1))
    b_v = gn * v.to(F64).abs() * (n * EPS24 * mag_dot) / norm_ref ** 2 \
        + (3 * eps_n + 6 * EPS24) * gn * (dW.abs() + v.to(F64).abs() * dot.abs() / norm_ref ** 2)
    r_g, r_v = _ratio(dgain.cpu(), g64.grad, b_gain), _ratio(dv.cpu(), v64.grad, b_v)
    print(f"[posconv] Cg{Cg} weight-norm backward: max |err| / bound = dgain {r_g:.2e}, dv {r_v:.4f}")
    assert r_g <= 1.0 and r_v <= 1.0, (r_g, r_v)        # measured: dgain < 1e-4, dv 0.046 (both widths)


# ------------------------------------------------------------------------------------------------ (h) the two paths agree
@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_dedicated_kernels_equal_the_implicit_gemm_path(cases, shape):
    """DESIGN.md section kernels: the dedicated kernels give the bits of the batched implicit-GEMM calls they replaced (the calls
    wav2vec2.py still makes when posconv_kernel_fits is false).  Both operators are called directly on the random data of (c)."""
    c = cases(shape)
    for name, run in (("forward", _run_fwd), ("dgrad", _run_dgrad)):
        k, gm = run(c, "kernel"), run(c, "gemm")
        for what, a, b in (("out", k[0], gm[0]), ("out_pre", k[1], gm[1])):
            nd = (a.view(torch.int16) != b.view(torch.int16)).sum().item()
            d = (a.float() - b.float()).abs().max().item()
            assert torch.equal(a, b), f"{name} {what}: {nd} of {a.numel()} elements differ, max |diff| {d:.3e}"
    if c["Cg"] == BASE and c["B"] >= 2:
        a, b = _run_wgrad(c, "kernel"), _run_wgrad(c, "gemm")
        nd, d = (a != b).sum().item(), (a - b).abs().max().item()
        assert torch.equal(a, b), f"wgrad: {nd} of {a.numel()} entries differ, max |diff| {d:.3e}"


# ------------------------------------------------------------------------------------------------ (i) the whole block
def _rel_l2(a, b):
    return ((a.to(F64) - b).norm() / b.norm()).item()


def test_whole_block_forward_and_backward_against_fp64_autograd():
    """pack, weight, gemm, pack(u), colsum, data gradient, weight gradient, weight_bwd chained as _EmbedStage.fwd / .bwd chain them
    (B = 3, Tp = 512, ragged, base) against weight_norm(dim=2) + grouped conv + SamePad + GELU + residual in fp64.
    Tolerance: the same chain in fp64 on the CPU with bf16 rounding at exactly the tensors the product stores in bf16 (Wf / Wd, u,
    s, dU, dh0); its relative L2 distance from pure fp64 is the storage-rounding floor of each output, and the kernels must stay
    within 2x that floor (the factor covers accumulation order and the GELU fit, which the emulation leaves out)."""
    from aptai_amd import ops
    Cg, B, Tp = BASE, 3, 512
    H, M, rows_p = G * Cg, B * Tp, Tp + 2 * PAD
    lens = [512, 451, 200]
    g = torch.Generator().manual_seed(5)
    h0 = _zero_beyond(torch.randn(M, H, generator=g), lens, Tp).to(BF16)
    ds = torch.randn(M, H, generator=g).to(BF16)
    v = torch.randn(H, Cg, KW, generator=g) * 0.1
    gain = (torch.rand(KW, generator=g) + 0.5) * 2.0
    bias = torch.randn(H, generator=g) * 0.5
    # ---- pure fp64
    x64, v64, g64, b64 = (t.to(F64).requires_grad_(True) for t in (h0, v, gain, bias))
    pre = R.conv_same(x64, R.weight_norm(v64, g64)[0], b64, B, Tp, G)
    s_ref = R.gelu_erf(pre) + x64
    s_ref.backward(ds.to(F64))
    ref = dict(s=s_ref.detach(), dh0=x64.grad, dv=v64.grad, dgain=g64.grad, dbias=b64.grad)
    # ---- fp64 with the product's bf16 storage points
    ve, ge = v.to(F64).requires_grad_(True), gain.to(F64).requires_grad_(True)
    w_e = R.weight_norm(ve, ge)[0]
    w_bf = R.bf16_round(w_e.detach())                                            # Wf / Wd hold the same rounded weights
    xg = R.pack(h0.to(F64), B, Tp, G, PAD)
    pre_e = R.toeplitz_matmul(xg, R.wf_layout(w_bf, G), 0, Tp) + bias.to(F64)
    u_e = R.bf16_round(pre_e)
    du_e = R.bf16_round(ds.to(F64) * R.gelu_erf_grad(u_e))
    dug = R.pack(du_e, B, Tp, G, PAD)
    dW_e = R.wf_layout_inv(R.wgrad_frames(dug, xg, PAD), KW)
    dv_e, dgain_e = torch.autograd.grad(w_e, [ve, ge], grad_outputs=dW_e)
    emu = dict(s=R.bf16_round(R.gelu_erf(pre_e) + h0.to(F64)), dbias=du_e.sum(0), dv=dv_e, dgain=dgain_e,
               dh0=R.bf16_round(R.toeplitz_matmul(dug, R.wd_layout(w_bf, G), 1, Tp) + ds.to(F64)))
    # ---- the kernels
    dev = "cuda"
    xg_d = torch.zeros(G * B * rows_p * Cg + Cg * 8, dtype=BF16, device=dev)
    dug_d = torch.zeros_like(xg_d)
    h0_d, ds_d, v_d, gain_d = h0.cuda(), ds.cuda(), v.cuda(), gain.cuda()
    ops.posconv_pack(h0_d, xg_d, B, Tp, H, G, PAD)
    wf, wd, norm = ops.posconv_weight(v_d, gain_d, G)
    u = torch.empty((M, H), dtype=BF16, device=dev)
    s = torch.empty_like(u)
    ops.posconv_gemm(xg_d, wf, s, B, Tp, H, G, KW, PAD, bias=bias.cuda(), gelu=True, residual=h0_d, out_pre=u)
    du_rm = torch.empty_like(u)
    ops.posconv_pack(ds_d, dug_d, B, Tp, H, G, PAD, u=u, rowmajor_out=du_rm)
    dbias = ops.colsum(du_rm, M, H)
    dh0 = torch.empty_like(u)
    ops.posconv_gemm(dug_d, wd, dh0, B, Tp, H, G, KW, PAD, first_row=1, residual=ds_d)
    dwf = torch.empty((G, Cg, KW * Cg), dtype=F32, device=dev)
    ops.posconv_wgrad(dug_d, xg_d, dwf, B, Tp, H, G, KW, PAD)
    dv, dgain = ops.posconv_weight_bwd(dwf, v_d, gain_d, norm, G)
    torch.cuda.synchronize()
    got = dict(s=s.cpu(), dh0=dh0.cpu(), dv=dv.cpu(), dgain=dgain.cpu(), dbias=dbias.cpu())
    report = {}
    for k in ("s", "dh0", "dv", "dgain", "dbias"):
        report[k] = (_rel_l2(emu[k], ref[k]), _rel_l2(got[k], ref[k]))
        print(f"[posconv] whole block {k}: storage-rounding floor {report[k][0]:.3e}, kernels {report[k][1]:.3e}")
    # floor / kernels, measured:  s 1.833e-3 / 1.833e-3, dh0 2.056e-3 / 2.057e-3, dv 2.047e-3 / 2.049e-3, dgain 2.044e-3 / 2.091e-3,
    # dbias 2.062e-3 / 2.073e-3
    for k, (floor, meas) in report.items():
        assert meas <= 2.0 * floor, (k, floor, meas)


# ------------------------------------------------------------------------------------------------ (j) argument checks
def test_argument_checks_raise_and_launch_nothing():
    from aptai_amd import ops
    from aptai_amd._lib import AptaiHipError
    B, Tp, H, Cg = 1, 128, G * BASE, BASE
    n = G * B * (Tp + 2 * PAD) * Cg + Cg * 8
    xg = torch.zeros(n, dtype=BF16, device="cuda")       # every buffer has the size of the largest legal call below
    w = torch.zeros((G, Cg, KW * Cg), dtype=BF16, device="cuda")
    out = torch.full((B * Tp, H), SENT_BITS, dtype=torch.int16, device="cuda").view(BF16)
    dw = torch.full((G, Cg, KW * Cg), SENT_F32, dtype=F32, device="cuda")
    bad_gemm = [dict(Tp=100), dict(Tp=0), dict(Kw=64, pad=32), dict(H=G * 32), dict(first_row=2), dict(first_row=-1), dict(pad=32)]
    for kw in bad_gemm:
        a = dict(B=B, Tp=Tp, H=H, Kw=KW, pad=PAD, first_row=0)
        a.update(kw)
        with pytest.raises(AptaiHipError):
            ops.posconv_gemm(xg, w, out, a["B"], a["Tp"], a["H"], G, a["Kw"], a["pad"], first_row=a["first_row"])
    bad_wgrad = [dict(Tp=96), dict(Tp=32, B=3), dict(Kw=64, pad=32), dict(H=G * 64), dict(H=G * 32)]
    for kw in bad_wgrad:
        a = dict(B=B, Tp=Tp, H=H, Kw=KW, pad=PAD)
        a.update(kw)
        with pytest.raises(AptaiHipError):
            ops.posconv_wgrad(xg, xg, dw, a["B"], a["Tp"], a["H"], G, a["Kw"], a["pad"])
    torch.cuda.synchronize()
    assert (out.view(torch.int16) == SENT_BITS).all(), "a rejected posconv_gemm call wrote its output"
    assert (dw == SENT_F32).all(), "a rejected posconv_wgrad call wrote its output"
    # the legal neighbours of the rejected calls run
    ops.posconv_gemm(xg, w, out, B, Tp, H, G, KW, PAD, first_row=1)
    ops.posconv_wgrad(xg, xg, dw, B, Tp, H, G, KW, PAD)
    torch.cuda.synchronize()
    assert out.float().abs().sum().item() == 0 and dw.abs().sum().item() == 0
