"""GPU: row sums of the grouped weight-gradient launch (aptai_gemm_bf16_grouped_rowsum).

A problem dW = dY^T X of the grouped launch may also write rowsum[m] = sum_k dY[k][m], the bias gradient: the tiles of its first tile
column form it from the dY fragments they hold, one more MFMA per fragment against a register of ones.  Checked here: exact integer sums
over ragged and multi-tile shapes, the flagship reduction length against float64 and against the ones[K][8] problem it replaces, mixed
groups with guard regions, the refusals, determinism, and a whole train step through the four-problem path against the eight-problem
form it replaces.

Bound of the float comparison: the sum of one column is a chain of K fp32 additions of exact products 1 * dY (bf16 values are fp32
values), each rounding at most 2^-24 relative to a partial sum that never exceeds sum|dY| of the column, so
|rowsum - exact| <= K * 2^-24 * sum|dY| per column."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

TN = dict(a_kmajor=True, b_kmajor=True, out_f32=True)
SENTINEL = -12345.5


def _rand(shape, g):
    return torch.randn(shape, generator=g).to(torch.bfloat16)


def _ints(shape, g):
    return torch.randint(-4, 5, shape, generator=g).to(torch.bfloat16)


def _guarded(M, dev):
    """fp32 buffer of M + 64 sentinels; the row sums go to its first M elements"""
    return torch.full((M + 64,), SENTINEL, device=dev, dtype=torch.float32)


@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("M", [128, 136, 264])
def test_integer_column_sums_are_exact_and_dw_is_unchanged(M, N):
    """K = 192 (three K-tiles); output rows: one tile, a ragged second tile, three tiles with a ragged last; N = 384 has tiles with
    tile_n > 0, which must not write.  The sums are the integer column sums; dW keeps the bits of the problem without the pointer."""
    from aptai_amd import ops
    g = torch.Generator().manual_seed(1000 * M + N)
    K = 192
    dy, x = _ints((K, M), g).cuda(), _rand((K, N), g).cuda()
    buf = _guarded(M, dy.device)
    dw, rs = ops.gemm_grouped([(dy, x, M, N, K, dict(TN, rowsum=buf[:M]))])
    plain, = ops.gemm_grouped([(dy, x, M, N, K, TN)])
    torch.cuda.synchronize()
    assert rs.data_ptr() == buf.data_ptr()
    assert torch.equal(rs.cpu(), dy.cpu().double().sum(0).float())
    assert torch.equal(buf[M:].cpu(), torch.full((64,), SENTINEL))
    assert torch.equal(dw, plain)
    ref = dy.float().cpu().t() @ x.float().cpu()
    assert (dw.cpu() - ref).abs().max().item() <= 2e-3 * ref.abs().max().item()


def test_flagship_reduction_length_against_float64_and_the_ones_problem():
    """K = 8192 (the flagship's frames per batch), 136 output rows (ragged second tile), random bf16 dY: within K * 2^-24 * sum|dY| of
    the float64 column sum, and the very bits of row 0 of the ones[K][8]^T . dY problem through aptai_gemm_bf16_grouped."""
    from aptai_amd import ops
    g = torch.Generator().manual_seed(8192)
    K, M, N = 8192, 136, 128
    dy, x = _rand((K, M), g).cuda(), _rand((K, N), g).cuda()
    dw, rs = ops.gemm_grouped([(dy, x, M, N, K, dict(TN, rowsum=True))])
    old, = ops.gemm_grouped([(ops.ones_kmajor(K, dy.device), dy, 8, M, K, TN)])
    plain, = ops.gemm_grouped([(dy, x, M, N, K, TN)])
    torch.cuda.synchronize()
    d64 = dy.cpu().double()
    err = (rs.cpu().double() - d64.sum(0)).abs()
    bound = K * 2.0 ** -24 * d64.abs().sum(0)
    print(f"row sums vs float64: max err {err.max().item():.3e}, min bound {bound.min().item():.3e}, "
          f"max |new - ones problem| {(rs - old[0]).abs().max().item():.3e}")
    assert (err <= bound).all()
    assert torch.equal(rs, old[0])
    assert torch.equal(dw, plain)


def test_mixed_group_matches_single_launches_and_respects_guards():
    """Four problems in one launch, two with row sums (264 and 136 rows) and two without (128 and 8 rows: the latter a ones problem);
    every output equals the problem launched alone, and the 64 sentinels behind each row-sum vector survive."""
    from aptai_amd import ops
    g = torch.Generator().manual_seed(77)
    K = 192
    shapes = [(264, 384, True), (128, 256, False), (136, 128, True), (8, 264, False)]
    probs, bufs = [], []
    for M, N, want in shapes:
        a = ops.ones_kmajor(K, "cuda:0") if M == 8 else _rand((K, M), g).cuda()
        b = _rand((K, N), g).cuda()
        buf = _guarded(M, a.device) if want else None
        bufs.append(buf)
        probs.append((a, b, M, N, K, dict(TN, rowsum=buf[:M]) if want else TN))
    outs = ops.gemm_grouped(probs)
    torch.cuda.synchronize()
    assert len(outs) == 6
    sums = iter(outs[4:])
    for (a, b, M, N, K_, kw), buf, got in zip(probs, bufs, outs[:4]):
        if buf is None:
            alone, = ops.gemm_grouped([(a, b, M, N, K_, TN)])
        else:
            alone, rs_alone = ops.gemm_grouped([(a, b, M, N, K_, dict(TN, rowsum=True))])
            rs = next(sums)
            assert torch.equal(rs, rs_alone)
            assert torch.equal(buf[M:].cpu(), torch.full((64,), SENTINEL))
            err = (rs.cpu().double() - a.cpu().double().sum(0)).abs()
            assert (err <= K_ * 2.0 ** -24 * a.cpu().double().abs().sum(0)).all()
        assert torch.equal(got, alone)


def test_refused_combinations_do_not_launch():
    """A row-sum pointer on a layout other than both-K-major, on a bf16 output, or with split-K slabs: APTAI_ERR_INVALID with a text
    of its own, and neither the vector nor its guard is written."""
    from aptai_amd import ops, _lib
    g = torch.Generator().manual_seed(5)
    K, M, N = 128, 128, 128
    a, b = _rand((K, M), g).cuda(), _rand((K, N), g).cuda()
    cases = [(dict(a_kmajor=False, b_kmajor=True, out_f32=True), "K-major"),
             (dict(a_kmajor=False, b_kmajor=False, out_f32=True), "K-major"),
             (dict(a_kmajor=True, b_kmajor=True, out_f32=False), "fp32 output"),
             (dict(TN, split_k=2), "partial sum")]
    for kw, text in cases:
        buf = _guarded(M, a.device)
        with pytest.raises(_lib.AptaiHipError) as e:
            ops.gemm_grouped([(a, b, M, N, K, dict(kw, rowsum=buf[:M]))])
        assert "status -1" in str(e.value) and text in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert torch.equal(buf.cpu(), torch.full((M + 64,), SENTINEL))
    # the same descriptors without the pointer are what they were: split-K stays refused by the grouped entry, the layouts run
    ops.gemm_grouped([(a, b, M, N, K, dict(a_kmajor=False, b_kmajor=True, out_f32=True))])
    with pytest.raises(_lib.AptaiHipError):
        ops.gemm_grouped([(a, b, M, N, K, dict(TN, split_k=2))])


def test_two_calls_give_equal_bits():
    from aptai_amd import ops
    g = torch.Generator().manual_seed(21)
    K = 1024
    dy1, x1, dy2, x2 = _rand((K, 264), g).cuda(), _rand((K, 384), g).cuda(), _rand((K, 768), g).cuda(), _rand((K, 136), g).cuda()
    kw = dict(TN, rowsum=True)
    first = ops.gemm_grouped([(dy1, x1, 264, 384, K, kw), (dy2, x2, 768, 136, K, kw)])
    second = ops.gemm_grouped([(dy1, x1, 264, 384, K, kw), (dy2, x2, 768, 136, K, kw)])
    torch.cuda.synchronize()
    assert len(first) == 4
    for p, q in zip(first, second):
        assert torch.equal(p, q)


def test_train_step_equals_the_eight_problem_form(monkeypatch):
    """Two-layer wav2vec2-base phoneme recogniser, 2 x 1 s, the reference's regularisers on, fixed seeds: every gradient of the step
    through the layer backward's four problems with row sums equals the step in which each grouped call runs as the eight problems it
    replaces (four weight gradients + four ones[M][8]^T . dY) on the same tensors, through aptai_gemm_bf16_grouped."""
    from aptai_amd import ops
    from aptai_amd.config import W2V2Config
    from oracle import synth
    from test_gpu_ctc_pr import _build_pr
    cfg = W2V2Config.base(num_hidden_layers=2, vocab_size=40, ctc_loss_reduction="mean", ctc_zero_infinity=True)
    sd = synth.make_state_dict(synth.pr_param_shapes(cfg), 0)
    model = _build_pr(cfg, sd)
    model.train()
    g = torch.Generator().manual_seed(4)
    sb = synth.synth_aptai_batch(cfg, 2, 16000, seed=3)
    lab = torch.full((2, 12), -100, dtype=torch.int64)
    for b, n in enumerate((12, 7)):
        lab[b, :n] = torch.randint(1, 40, (n,), generator=g)
    batch = {"input_values": sb["audio_inputs"].cuda(), "input_lengths": sb["audio_lengths"].reshape(-1).cuda(), "phoneme_labels": lab.cuda()}

    def step():
        model.wav2vec2._step = 11
        model.wav2vec2._layerdrop_gen.manual_seed(0x1A7E)
        np.random.seed(5)
        model.zero_grad(set_to_none=True)
        out = model(**batch)
        out["loss"].backward()
        torch.cuda.synchronize()
        return out["loss"].detach().clone(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}

    grouped = ops.gemm_grouped
    calls = {"four": 0, "eight": 0}

    def counting(problems):
        problems = list(problems)
        calls["four"] += sum(1 for p in problems if p[5].get("rowsum"))
        return grouped(problems)

    def eight_problem_form(problems):
        problems = list(problems)
        plain = [(a, b, M, N, K, {k: v for k, v in kw.items() if k != "rowsum"}) for a, b, M, N, K, kw in problems]
        sums = [(ops.ones_kmajor(K, a.device), a, 8, M, K, TN) for a, b, M, N, K, kw in problems if kw.get("rowsum")]
        calls["eight"] += len(sums)
        outs = grouped(plain + sums)
        return outs[:len(plain)] + [o[0] for o in outs[len(plain):]]

    monkeypatch.setattr(ops, "gemm_grouped", counting)
    loss4, grads4 = step()
    monkeypatch.setattr(ops, "gemm_grouped", eight_problem_form)
    loss8, grads8 = step()
    assert calls["four"] >= 4 and calls["eight"] == calls["four"], calls
    assert torch.equal(loss4, loss8)
    assert set(grads4) == set(grads8) and any(n.endswith("attention.q_proj.bias") for n in grads4)
    bad = [n for n in grads4 if not torch.equal(grads4[n], grads8[n])]
    assert not bad, bad
