"""GPU, operator level: the CTC kernels of csrc/ctc.hip - log-softmax + per-state gather, the alpha / beta recursions at every
register width (NS = 2, 4, 8 states per lane) and at the dispatch edges, the gradient kernel in every form the product calls it
(fp32 / bf16 output, padded rows and columns, grad_out and extra_scale, per-utterance vocabulary) and the best-path decode - against
torch.nn.functional.ctc_loss on float64 CPU tensors (the call the reference project makes) and heads_ref.ctc_best_path.

Labels come from a small alphabet, so equal neighbours are dense and the `skip` rule is exercised across lane boundaries in every
case.  Bounds: the floors are the project's own (tests/test_gpu_ctc_pr.py); where fp32 itself cannot hold them (a handful of feasible
paths, nll near 900) the yardstick is torch's OWN fp32 CPU result against float64, times 4 (fast exp / log instead of libm, another
summation order) - never the kernel's figure."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F32, F64, BF16 = torch.float32, torch.float64, torch.bfloat16
LOSS_FLOOR = 2e-4              # x |ref|             test_ctc_long_targets_and_oracle
GRAD_FLOOR = 1e-4              # x max |ref grad|    test_ctc_long_targets_and_oracle
LP_FLOOR = 1e-5                # absolute            test_ctc_against_torch_golden
YARD = 4.0                     # x (torch fp32 CPU - float64)
REDUCTIONS = ("mean", "sum", "none")


# ------------------------------------------------------------------------------------------------ inputs and float64 references (CPU)
def make_problem(seed, T, V, ldt, target_lens, input_lens, blank=0, alphabet=None):
    """logits 2 randn (T,B,V); labels of the first `alphabet` non-blank classes; the row beyond target_lens[b] holds garbage inside
    [0, V).  Every utterance is feasible: input_len >= L + equal neighbours (asserted)."""
    g = torch.Generator().manual_seed(seed)
    B = len(target_lens)
    logits = 2.0 * torch.randn(T, B, V, generator=g)
    classes = torch.tensor([v for v in range(V) if v != blank][:alphabet or V])
    targets = classes[torch.randint(0, len(classes), (B, ldt), generator=g)].to(torch.int32)
    repeats = []
    for b, L in enumerate(target_lens):
        targets[b, L:] = torch.randint(0, V, (ldt - L,), generator=g, dtype=torch.int32)
        repeats.append(int((targets[b, 1:L] == targets[b, :L - 1]).sum()) if L > 1 else 0)
        assert L <= ldt and input_lens[b] <= T
        assert input_lens[b] >= L + repeats[b], (b, input_lens[b], L, repeats[b])
    return SimpleNamespace(T=T, B=B, V=V, ldt=ldt, blank=blank, logits=logits, targets=targets, tl=tuple(target_lens),
                           il=tuple(input_lens), repeats=repeats)


def torch_ctc(p, reduction, dtype):
    """F.ctc_loss on log_softmax in `dtype` on the CPU: nll per utterance (inf when infeasible), the loss under zero_infinity, its
    gradient with respect to the logits (T,B,V) ('none': of the sum over the batch, what grad_out = 1 means) and log_probs."""
    x = p.logits.to(dtype).clone().requires_grad_(True)
    lp = F.log_softmax(x, -1)
    tg = p.targets.long()
    nll = F.ctc_loss(lp, tg, p.il, p.tl, blank=p.blank, reduction="none", zero_infinity=False).detach()
    loss = F.ctc_loss(lp, tg, p.il, p.tl, blank=p.blank, reduction=reduction, zero_infinity=True)
    loss.sum().backward()
    return SimpleNamespace(nll=nll, loss=loss.detach(), grad=x.grad, lp=lp.detach())


def references(p):
    """{reduction: (float64, fp32 yardstick)}"""
    return {r: (torch_ctc(p, r, F64), torch_ctc(p, r, F32)) for r in REDUCTIONS}


CASES_A = [(63, 5, 120), (64, 5, 130), (127, 5, 230), (128, 7, 230), (255, 9, 300), (127, 256, 140)]
NS_OF = {63: 2, 64: 4, 127: 4, 128: 8, 255: 8}


@functools.lru_cache(maxsize=None)
def case_a(ldt, V, T):
    B = 2 if ldt == 255 else 3
    p = make_problem(1000 * ldt + V, T, V, ldt, [ldt, ldt // 2, 1][:B], [T, T - 17, 5][:B])
    assert min(ns for ns in (2, 4, 8) if ns >= (2 * ldt + 1 + 63) // 64) == NS_OF[ldt]          # launch_recur_ns
    p.refs = references(p)
    return p


@functools.lru_cache(maxsize=None)
def case_pr():
    """The phoneme recogniser's shape: T = 37 of Tp = 64 rows, V = 40 of Np = 64 columns."""
    p = make_problem(7, 37, 40, 12, [12, 7, 3], [37, 30, 9], alphabet=4)
    p.refs = references(p)
    return p


@functools.lru_cache(maxsize=None)
def case_options(blank):
    V = 6
    p = make_problem(11 + blank, 120, V, 70, [70, 33, 1], [120, 101, 4], blank=blank)      # NS = 4
    p.refs = references(p)
    return p


@functools.lru_cache(maxsize=None)
def case_mixed():
    """feasible | L > input_len | infeasible by one equal pair only | L = 0"""
    g = torch.Generator().manual_seed(5)
    T, V, ldt = 30, 5, 10
    targets = torch.randint(1, V, (4, ldt), generator=g, dtype=torch.int32)
    targets[0, :8] = torch.tensor([1, 2, 2, 3, 4, 4, 1, 3])
    targets[2, :6] = torch.tensor([1, 2, 2, 3, 4, 1])
    p = SimpleNamespace(T=T, B=4, V=V, ldt=ldt, blank=0, logits=2.0 * torch.randn(T, 4, V, generator=g), targets=targets,
                        tl=(8, 10, 6, 0), il=(30, 6, 6, 12))
    p.refs = {"mean": (torch_ctc(p, "mean", F64), torch_ctc(p, "mean", F32))}
    return p


def fs_problem(N):
    """Forward-sum rows [-1 | att_log | zeros] (B,T,ld) at pitch ld = round_up(N + 1, 64), as modules._FwdSumFn builds them."""
    g = torch.Generator().manual_seed(300 + N)
    B, T = 2, N + 20
    text, mel = (N, N // 3), (T, T - 9)
    x = 2.0 * torch.randn(B, T, N, generator=g)
    for b in range(B):
        x[b, :, text[b]:] -= 2000.0                                  # masked slots, as the cross-attention leaves them
    ld = (N + 64) // 64 * 64
    rows = torch.zeros(B, T, ld)
    rows[:, :, 0] = -1.0
    rows[:, :, 1:1 + N] = torch.log_softmax(x, -1)
    for b in range(B):
        assert mel[b] >= text[b]                                     # targets 1..n never repeat
    return SimpleNamespace(N=N, B=B, T=T, ld=ld, text=text, mel=mel, rows=rows)


def fs_reference(q, dtype):
    """Per utterance: log_softmax over its own n + 1 classes, F.ctc_loss 'mean' with targets 1..n, mean over the batch - the loop of
    heads_ref.forward_sum_loss.  Gradient with respect to the whole rows (B,T,ld)."""
    x = q.rows.to(dtype).clone().requires_grad_(True)
    total, nll = 0.0, []
    for b in range(q.B):
        n, t = q.text[b], q.mel[b]
        cur = F.log_softmax(x[b, :t, :n + 1], -1).unsqueeze(1)
        l = F.ctc_loss(cur, torch.arange(1, n + 1)[None], [t], [n], blank=0, reduction="mean", zero_infinity=True)
        total = total + l
        nll.append(l.detach() * n)
    loss = total / q.B
    loss.backward()
    return SimpleNamespace(loss=loss.detach(), nll=torch.stack(nll), grad=x.grad)


@functools.lru_cache(maxsize=None)
def case_fs(N):
    q = fs_problem(N)
    q.refs = (fs_reference(q, F64), fs_reference(q, F32))
    return q


def decode_rows(T, V, blank, seed):
    """Integer-valued logits [rows][T][V] (ties in most frames of the random rows) and the name of each row."""
    g = torch.Generator().manual_seed(seed)
    nb = 1 if blank == 0 else 0                                      # a label that is not the blank
    rows, names = [], []
    for lo, hi in ((0, 2), (0, 3), (-1, 2), (0, 5)):
        rows.append(torch.randint(lo, hi, (T, V), generator=g).float())
        names.append(f"ties{lo}:{hi}")

    def from_path(seq, name):
        x = torch.randint(-2, 1, (T, V), generator=g).float()        # <= 0 everywhere, 1 at the chosen class
        x[torch.arange(T), seq] = 1.0
        rows.append(x)
        names.append(name)

    for edge in (64, 128):                                           # frame `edge` opens a new round of 64 frames
        if T <= edge:
            continue
        for name, a, b in (("same", nb, nb), ("blank|label", blank, nb), ("label|blank", nb, blank)):
            seq = torch.randint(0, V, (T,), generator=g)
            seq[edge - 1], seq[edge] = a, b
            if edge >= 2:
                seq[edge - 2] = blank if a != blank else nb          # frame edge-1 differs from its own predecessor
            from_path(seq, f"{name}@{edge}")
    from_path(torch.full((T,), blank), "all-blank")
    from_path(torch.arange(T) % V, "no-repeats")
    return torch.stack(rows), names


# ------------------------------------------------------------------------------------------------ device side
def dev_rows(p, ldl=None, rows_per_b=None, fill=float("nan")):
    """[B * rows_per_b][ldl] fp32 on the device: the logits in rows t < T and columns v < V, `fill` everywhere else."""
    ldl, rows_per_b = ldl or p.V, rows_per_b or p.T
    full = torch.full((p.B, rows_per_b, ldl), fill, dtype=F32)
    full[:, :p.T, :p.V] = p.logits.permute(1, 0, 2)
    return full.view(p.B * rows_per_b, ldl).cuda()


def dev_args(p):
    return (p.targets.cuda(), torch.tensor(p.il, dtype=torch.int32).cuda(), torch.tensor(p.tl, dtype=torch.int32).cuda())


def tbv(d, p, rows_per_b=None):
    """kernel gradient [B * rows_per_b][ldd] -> (T,B,V) on the CPU"""
    return d.view(p.B, rows_per_b or p.T, -1)[:, :p.T, :p.V].permute(1, 0, 2).float().cpu()


def check(tag, got, r64, r32, floor, *, absolute=False, elementwise=False):
    """|got - float64| <= max(floor x scale, 4 x |torch fp32 - float64|); scale = max |ref| (elementwise: |ref|; absolute: 1)."""
    got, r64, r32 = (v.detach().double().reshape(-1) for v in (got, r64, r32))
    err, yard = (got - r64).abs(), (r32 - r64).abs()
    scale = torch.ones_like(r64) if absolute else r64.abs()
    if not elementwise:
        err, yard, scale = err.max().reshape(1), yard.max().reshape(1), scale.max().reshape(1)
    bound = torch.maximum(floor * scale, YARD * yard)
    i = int((err / bound.clamp_min(1e-300)).argmax())
    print(f"[bands] {tag}: kernel |err| {err[i]:.3e} ({err[i] / scale[i].clamp_min(1e-300):.3e} of scale), "
          f"torch-fp32 yardstick {yard[i]:.3e}, bound {bound[i]:.3e}")
    assert bool((err <= bound).all()), (tag, float(err[i]), float(bound[i]))


# ------------------------------------------------------------------------------------------------ the reference itself
def test_reference_torch_float64_agrees_with_the_oracle_recursion():
    """F.ctc_loss in float64 and heads_ref.ctc_loss_ref in float64: one loss, one gradient (<= 1e-11 of its maximum)."""
    from oracle.heads_ref import ctc_loss_ref
    p = case_pr()
    r = p.refs["mean"][0]
    x = p.logits.double().clone().requires_grad_(True)
    loss = ctc_loss_ref(torch.log_softmax(x, -1), p.targets, p.il, p.tl, 0, "mean", True)
    loss.backward()
    assert abs(loss.item() - r.loss.item()) <= 1e-12 * abs(r.loss.item())
    assert (x.grad - r.grad).abs().max().item() <= 1e-11 * r.grad.abs().max().item()


# ------------------------------------------------------------------------------------------------ (a) widths and dispatch edges
@pytest.mark.parametrize("ldt,V,T", CASES_A, ids=[f"ldt{c[0]}-V{c[1]}-T{c[2]}" for c in CASES_A])
def test_recursion_widths_and_dispatch_edges(ldt, V, T):
    """S_max = 2 ldt + 1 picks ctc_recur_kernel<2 | 4 | 8>: both sides of 63|64 and 127|128, the widest row, and NS = 4 at
    MAXV = 256 classes.  Gradient error as a fraction of max |ref grad|, kernel on MI355X / torch's fp32 CPU yardstick, in the
    order of CASES_A:  'mean' 1.2e-6 / 2.5e-6, 1.4e-6 / 1.2e-6, 1.7e-6 / 1.6e-6, 2.3e-6 / 1.9e-6, 2.6e-4 / 3.0e-4, 2.5e-6 / 3.5e-6;
    'sum' and 'none' (the long utterances are not divided by L B) 2.8e-5 / 1.8e-5, 7.9e-5 / 6.7e-5, 9.5e-5 / 9.2e-5,
    1.6e-4 / 1.2e-4, 5.0e-4 / 5.7e-4, 3.1e-4 / 4.3e-4: fp32 itself misses the 1e-4 floor from ldt = 128 on, the kernel stays
    within 1.3 x the yardstick everywhere.  nll and loss: <= 5e-7 relative (floor 2e-4); log_probs: <= 1.1e-6 (floor 1e-5)."""
    from aptai_amd import ops
    p = case_a(ldt, V, T)
    rows, (tg, il, tl) = dev_rows(p), dev_args(p)
    for red in REDUCTIONS:
        r64, r32 = p.refs[red]
        loss, nll, lp, ws = ops.ctc_fwd(rows, V, T, tg, il, tl, p.B, T, V, reduction=red, zero_infinity=True)
        d = ops.ctc_bwd(rows, V, T, tg, il, tl, p.B, T, V, ws, nll, None, reduction=red, zero_infinity=True, ldd=V, out_dtype=F32)
        tag = f"ldt={ldt} V={V} NS={NS_OF[ldt]} {red}"
        check(f"{tag} nll", nll.cpu(), r64.nll, r32.nll, LOSS_FLOOR, elementwise=True)
        if red != "none":                                            # 'none': the loss IS nll, the scalar is not written
            check(f"{tag} loss", loss.cpu(), r64.loss, r32.loss, LOSS_FLOOR)
        check(f"{tag} log_probs", lp.cpu(), r64.lp, r32.lp, LP_FLOOR, absolute=True)
        check(f"{tag} grad", tbv(d, p), r64.grad, r32.grad, GRAD_FLOOR)


# ------------------------------------------------------------------------------------------------ (b) the recogniser's call form
def test_phoneme_recogniser_call_form():
    """pr_head_bwd's call: bf16 output, ldl = ldd = Np = 64 > V = 40, rows_per_b = Tp = 64 > T = 37, a grad_out tensor."""
    from aptai_amd import ops
    p = case_pr()
    r64, r32 = p.refs["mean"]
    Tp, Np, T, V, B = 64, 64, p.T, p.V, p.B
    rows, (tg, il, tl) = dev_rows(p, Np, Tp), dev_args(p)            # NaN in the padding columns and rows
    one = torch.ones(1, device="cuda")
    loss, nll, lp, ws = ops.ctc_fwd(rows, Np, Tp, tg, il, tl, B, T, V)
    check("pr-form loss", loss.cpu(), r64.loss, r32.loss, LOSS_FLOOR)
    check("pr-form log_probs", lp.cpu(), r64.lp, r32.lp, LP_FLOOR, absolute=True)
    d32 = ops.ctc_bwd(rows, Np, Tp, tg, il, tl, B, T, V, ws, nll, one, ldd=Np, out_dtype=F32)
    d16 = ops.ctc_bwd(rows, Np, Tp, tg, il, tl, B, T, V, ws, nll, one, ldd=Np)
    assert d16.dtype == BF16 and d16.shape == (B * Tp, Np) and d32.shape == (B * Tp, Np)
    check("pr-form grad", tbv(d32, p, Tp), r64.grad, r32.grad, GRAD_FLOOR)       # measured 1.0e-5 of max; yardstick 6.9e-6
    assert torch.equal(d16.cpu().view(torch.int16), d32.cpu().to(BF16).view(torch.int16))       # one round-to-nearest-even
    for d in (d32.cpu().view(B, Tp, Np), d16.cpu().view(B, Tp, Np)):
        assert (d[:, :, V:] == 0).all()
        assert (d[:, T:] == 0).all()
        for b in range(B):
            assert (d[b, p.il[b]:] == 0).all()
        assert bool(torch.isfinite(d.float()).all())
    g06 = torch.full((1,), 0.6, device="cuda")
    ds = ops.ctc_bwd(rows, Np, Tp, tg, il, tl, B, T, V, ws, nll, g06, ldd=Np, out_dtype=F32, extra_scale=0.25)
    check("pr-form grad x 0.6 x 0.25", tbv(ds, p, Tp), 0.15 * r64.grad, 0.15 * r32.grad, GRAD_FLOOR)


# ------------------------------------------------------------------------------------------------ (c) options
def test_blank_is_the_last_class():
    from aptai_amd import ops
    p = case_options(5)
    assert p.blank == p.V - 1 and not bool((p.targets[0, :p.tl[0]] == p.blank).any())
    rows, (tg, il, tl) = dev_rows(p), dev_args(p)
    r64, r32 = p.refs["mean"]
    loss, nll, lp, ws = ops.ctc_fwd(rows, p.V, p.T, tg, il, tl, p.B, p.T, p.V, blank=p.blank)
    d = ops.ctc_bwd(rows, p.V, p.T, tg, il, tl, p.B, p.T, p.V, ws, nll, None, blank=p.blank, ldd=p.V, out_dtype=F32)
    check("blank=V-1 nll", nll.cpu(), r64.nll, r32.nll, LOSS_FLOOR, elementwise=True)
    check("blank=V-1 loss", loss.cpu(), r64.loss, r32.loss, LOSS_FLOOR)
    check("blank=V-1 grad", tbv(d, p), r64.grad, r32.grad, GRAD_FLOOR)           # measured 1.6e-6 of max; yardstick 1.1e-6


def test_beta_launched_by_the_backward_and_log_probs_left_out():
    """want_beta=False, then ctc_bwd runs the beta recursion on its own (NS = 4): the bits of the side-by-side launch.
    want_log_probs=False changes nothing else."""
    from aptai_amd import ops
    p = case_options(0)
    rows, (tg, il, tl) = dev_rows(p), dev_args(p)
    a = (rows, p.V, p.T, tg, il, tl, p.B, p.T, p.V)
    loss1, nll1, lp1, ws1 = ops.ctc_fwd(*a, want_beta=True)
    d1 = ops.ctc_bwd(*a, ws1, nll1, None, ldd=p.V, out_dtype=F32)
    loss2, nll2, lp2, ws2 = ops.ctc_fwd(*a, want_beta=False, want_log_probs=False)
    assert ws1._beta_ready and not ws2._beta_ready and lp2 is None and lp1 is not None
    d2 = ops.ctc_bwd(*a, ws2, nll2, None, ldd=p.V, out_dtype=F32)
    assert torch.equal(loss1, loss2) and torch.equal(nll1, nll2)
    assert torch.equal(d1, d2)
    r64, r32 = p.refs["mean"]
    check("beta-by-backward grad", tbv(d2, p), r64.grad, r32.grad, GRAD_FLOOR)


# ------------------------------------------------------------------------------------------------ (d) mixed feasibility
def test_mixed_feasibility_under_zero_infinity():
    from aptai_amd import ops
    p = case_mixed()
    r64, r32 = p.refs["mean"]
    assert torch.isinf(r64.nll).tolist() == [False, True, True, False]
    rows, (tg, il, tl) = dev_rows(p), dev_args(p)
    loss, nll, lp, ws = ops.ctc_fwd(rows, p.V, p.T, tg, il, tl, p.B, p.T, p.V, reduction="mean", zero_infinity=True)
    d = ops.ctc_bwd(rows, p.V, p.T, tg, il, tl, p.B, p.T, p.V, ws, nll, None, reduction="mean", zero_infinity=True, ldd=p.V,
                    out_dtype=F32)
    nll, g = nll.cpu(), tbv(d, p)
    assert nll[1].item() == float("inf") and nll[2].item() == float("inf")
    ok = torch.tensor([0, 3])
    check("mixed nll", nll[ok], r64.nll[ok], r32.nll[ok], LOSS_FLOOR, elementwise=True)
    check("mixed loss", loss.cpu(), r64.loss, r32.loss, LOSS_FLOOR)
    assert (g[:, 1] == 0).all() and (g[:, 2] == 0).all()
    assert (r64.grad[:, 1] == 0).all() and (r64.grad[:, 2] == 0).all()
    check("mixed grad", g[:, ok], r64.grad[:, ok], r32.grad[:, ok], GRAD_FLOOR)    # measured 2.3e-7 of max; yardstick 3.8e-6


# ------------------------------------------------------------------------------------------------ (e) per-utterance vocabulary
@pytest.mark.parametrize("N", [64, 100, 127])
def test_forward_sum_form_at_ns4(N):
    """ForwardSumLoss' call: vocab_sizes = text_lens + 1, targets 1..N, rows at pitch fs_row_pitch(N), fp32 output at ldd = ld."""
    from aptai_amd import ops
    q = case_fs(N)
    r64, r32 = q.refs
    B, T, ld = q.B, q.T, q.ld
    assert ld == ops.fs_row_pitch(N) and 2 < (2 * N + 1 + 63) // 64 <= 4
    rows = q.rows.view(B * T, ld).cuda()
    tg = torch.arange(1, N + 1, dtype=torch.int32)[None, :].repeat(B, 1).contiguous().cuda()
    mel, txt = torch.tensor(q.mel, dtype=torch.int32).cuda(), torch.tensor(q.text, dtype=torch.int32).cuda()
    vs = (txt + 1).contiguous()
    loss, nll, lp, ws = ops.ctc_fwd(rows, ld, T, tg, mel, txt, B, T, N + 1, vocab_sizes_i32=vs, want_log_probs=False)
    d = ops.ctc_bwd(rows, ld, T, tg, mel, txt, B, T, N + 1, ws, nll, torch.ones(1, device="cuda"), vocab_sizes_i32=vs, ldd=ld,
                    out_dtype=F32).cpu().view(B, T, ld)
    check(f"forward-sum N={N} nll", nll.cpu(), r64.nll, r32.nll, LOSS_FLOOR, elementwise=True)
    check(f"forward-sum N={N} loss", loss.cpu(), r64.loss, r32.loss, LOSS_FLOOR)
    # measured, fraction of max |ref grad|, kernel / yardstick: N=64 5.5e-5 / 4.9e-5, N=100 5.4e-5 / 7.4e-5, N=127 1.5e-4 / 1.6e-4
    check(f"forward-sum N={N} grad", d, r64.grad, r32.grad, GRAD_FLOOR)
    for b in range(B):
        assert (d[b, :, q.text[b] + 1:] == 0).all()
        assert (d[b, q.mel[b]:] == 0).all()


# ------------------------------------------------------------------------------------------------ (f) best-path decode
@pytest.mark.parametrize("V", [2, 40, 256])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 130])
def test_greedy_decode_against_best_path(T, V):
    from aptai_amd import ops
    from oracle.heads_ref import ctc_best_path
    ldl, Tp = (V + 3 if V < 256 else V), T + 5
    for blank in (0, V - 1):
        x, names = decode_rows(T, V, blank, seed=100 * T + V + blank)
        B = x.shape[0]
        nb = 1 if blank == 0 else 0
        full = torch.full((B, Tp, ldl), 1e9)                         # padding columns would win every argmax if they were read
        full[:, T:, :V] = -1.0
        full[:, T:, nb] = 5.0                                        # padding rows would decode to a label if they were read
        full[:, :T, :V] = x
        dev = full.view(B * Tp, ldl).cuda()
        want = [ctc_best_path(x[b].numpy(), blank) for b in range(B)]
        assert len(want[names.index("all-blank")]) == 0
        if T > 64:
            assert want[names.index("same@64")].tolist().count(nb) >= 1
        ids, n = ops.ctc_greedy_decode(dev, ldl, Tp, B, T, V, blank, T)
        ids, n = ids.cpu(), n.cpu()
        for b in range(B):
            w = want[b]
            assert n[b].item() == len(w), (names[b], blank, n[b].item(), len(w))
            assert ids[b, :len(w)].tolist() == w.tolist(), (names[b], blank)
            assert (ids[b, len(w):] == 0).all(), (names[b], blank)
        longest = max(len(w) for w in want)
        m = max(1, longest // 2)                                     # shorter than the longest decoded row (T >= 2)
        assert T == 1 or longest > m
        ids, n = ops.ctc_greedy_decode(dev, ldl, Tp, B, T, V, blank, m)
        ids, n = ids.cpu(), n.cpu()
        assert ids.shape == (B, m)
        for b in range(B):
            w = want[b]
            k = min(len(w), m)
            assert n[b].item() == len(w), (names[b], blank, "max_n", m)
            assert ids[b, :k].tolist() == w[:k].tolist() and (ids[b, k:] == 0).all(), (names[b], blank, "max_n", m)


@functools.lru_cache(maxsize=None)
def _greedy_device_batch(blank):
    import greedy_cases
    return torch.from_numpy(greedy_cases.padded(blank)).cuda()


@pytest.mark.parametrize("max_n", [132, 5])
@pytest.mark.parametrize("own_lens", [True, False])
@pytest.mark.parametrize("blank", [0, 2])
@pytest.mark.parametrize("sil", [None, 1])
def test_greedy_decode_contract_lengths_framing_timesteps(sil, blank, own_lens, max_n):
    """aptai_ctc_greedy_decode = hostlogic.ctc_bracketed_best_path row by row on the batch of tests/greedy_cases.py: tokens,
    timesteps and the full length, with and without the silence framing, per-row lengths (None = all T frames, where the frames
    past a row's length are decoded too), max_n = T + 2 and a max_n that cuts rows.  Integers: equality, no tolerance."""
    import greedy_cases as gc
    from aptai_amd import ops
    gc.assert_situations(blank)
    dev = _greedy_device_batch(blank)
    lens = torch.tensor(gc.LENS, dtype=torch.int32).cuda() if own_lens else None
    want = gc.oracle(blank, sil, own_lens)

    def run():
        return [x.cpu().numpy() for x in ops.ctc_greedy_decode(dev, gc.LDL, gc.ROWS_PER_B, gc.B, gc.T, gc.V, blank, max_n,
                                                               input_lens_i32=lens, sil=sil, want_timesteps=True)]
    ids, ts, n = run()
    assert ids.shape == ts.shape == (gc.B, max_n) and ids.dtype == ts.dtype == n.dtype == np.int32
    for b, (tok, pos) in enumerate(want):
        k = min(len(tok), max_n)
        assert n[b] == len(tok), (b, n[b], len(tok))
        assert ids[b, :k].tolist() == tok[:k].tolist() and ts[b, :k].tolist() == pos[:k].tolist(), b
        assert not ids[b, k:].any() and not ts[b, k:].any(), b
    assert [x.tobytes() for x in run()] == [x.tobytes() for x in (ids, ts, n)]
    if not own_lens:                                             # None is all-T lengths, and the two-value form is the same decode
        full = torch.full((gc.B,), gc.T, dtype=torch.int32).cuda()
        same = ops.ctc_greedy_decode(dev, gc.LDL, gc.ROWS_PER_B, gc.B, gc.T, gc.V, blank, max_n, input_lens_i32=full, sil=sil)
        assert len(same) == 2 and np.array_equal(same[0].cpu().numpy(), ids) and np.array_equal(same[1].cpu().numpy(), n)
    with pytest.raises(ValueError, match="input_lens_i32"):
        ops.ctc_greedy_decode(dev, gc.LDL, gc.ROWS_PER_B, gc.B, gc.T, gc.V, blank, max_n, input_lens_i32=torch.zeros(gc.B).cuda())


def test_decode_rows_cover_the_round_boundary():
    """The constructed rows are what they claim (CPU only): frames 63 | 64 hold label | label, blank | label, label | blank."""
    from oracle.heads_ref import ctc_best_path
    for blank, nb in ((0, 1), (39, 0)):
        x, names = decode_rows(130, 40, blank, seed=1)
        am = x.argmax(-1)
        for edge in (64, 128):
            assert am[names.index(f"same@{edge}"), edge - 1:edge + 1].tolist() == [nb, nb]
            assert am[names.index(f"blank|label@{edge}"), edge - 1:edge + 1].tolist() == [blank, nb]
            assert am[names.index(f"label|blank@{edge}"), edge - 1:edge + 1].tolist() == [nb, blank]
            assert am[names.index(f"same@{edge}"), edge - 2].item() != nb
        r = am[names.index("no-repeats")]
        assert bool((r[1:] != r[:-1]).all())
        assert len(ctc_best_path(x[names.index("no-repeats")].numpy(), blank)) == 130 - int((r == blank).sum())
        ties = (x[0] == x[0].max(-1, keepdim=True).values).sum(-1)
        assert (ties > 1).float().mean().item() > 0.5


# ------------------------------------------------------------------------------------------------ (g) host-side refusals
def test_host_side_refusals():
    from aptai_amd import ops
    from aptai_amd._lib import AptaiHipError
    B, T, V = 2, 8, 6
    il, tl = torch.full((B,), T, dtype=torch.int32).cuda(), torch.ones(B, dtype=torch.int32).cuda()
    rows = torch.zeros(B * T, V, device="cuda")
    with pytest.raises(AptaiHipError, match="at most 255 labels"):
        ops.ctc_fwd(rows, V, T, torch.ones(B, 256, dtype=torch.int32).cuda(), il, tl, B, T, V)
    with pytest.raises(AptaiHipError, match="bad sizes"):
        ops.ctc_fwd(torch.zeros(B * T, 257, device="cuda"), 257, T, torch.ones(B, 4, dtype=torch.int32).cuda(), il, tl, B, T, 257)
    tg = torch.ones(B, 4, dtype=torch.int32).cuda()
    loss, nll, lp, ws = ops.ctc_fwd(rows, V, T, tg, il, tl, B, T, V)
    for ldd in (V - 1, 257):
        with pytest.raises(AptaiHipError, match="bad dlogits"):
            ops.ctc_bwd(rows, V, T, tg, il, tl, B, T, V, ws, nll, None, ldd=ldd, out_dtype=F32)
    d = ops.ctc_bwd(rows, V, T, tg, il, tl, B, T, V, ws, nll, None, ldd=256, out_dtype=F32)    # the widest row is accepted
    assert bool(torch.isfinite(d).all()) and (d[:, V:] == 0).all()
