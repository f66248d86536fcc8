"""CPU: the host-side contract of global-norm gradient clipping (aptai_amd.optim.Adam(max_grad_norm=...), clip_grad_norm_): argument
checks that need no device, and the three C-ABI entries being declared (tests/test_cpu_host.py then checks every declared symbol
against the built library)."""
import pytest
import torch


def _cpu_param(n=8):
    p = torch.nn.Parameter(torch.randn(n))
    p.grad = torch.randn(n)
    return p


def test_constructor_rejects_a_negative_or_nan_max_grad_norm():
    from aptai_amd.optim import Adam
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            Adam([_cpu_param()], max_grad_norm=bad)
    opt = Adam([_cpu_param()], max_grad_norm=None)
    assert opt.max_grad_norm is None and opt.last_grad_norm is None and opt.last_clip_coef is None
    opt.max_grad_norm = 1                               # reassignable between steps; inf = measure only
    assert opt.max_grad_norm == 1.0
    opt.max_grad_norm = float("inf")
    with pytest.raises(ValueError):
        opt.max_grad_norm = -0.5
    assert "max_grad_norm" not in opt.param_groups[0] and "max_grad_norm" not in opt.state_dict()["param_groups"][0]


def test_clip_grad_norm_refuses_cpu_and_non_fp32_gradients():
    from aptai_amd import _lib
    from aptai_amd.optim import clip_grad_norm_
    with pytest.raises(_lib.AptaiHipError):
        clip_grad_norm_([_cpu_param()], 1.0)
    with pytest.raises(_lib.AptaiHipError):
        clip_grad_norm_(_cpu_param(), 1.0)              # a single tensor, as torch accepts
    p = torch.nn.Parameter(torch.randn(8, dtype=torch.float64))
    p.grad = torch.randn(8, dtype=torch.float64)
    with pytest.raises(_lib.AptaiHipError):
        clip_grad_norm_([p], 1.0)


def test_clip_grad_norm_computes_the_two_norm_only():
    from aptai_amd.optim import clip_grad_norm_
    for norm_type in (1, 1.0, float("inf")):
        with pytest.raises(ValueError):
            clip_grad_norm_([_cpu_param()], 1.0, norm_type=norm_type)
    with pytest.raises(ValueError):
        clip_grad_norm_([_cpu_param()], -1.0)
    assert float(clip_grad_norm_([torch.nn.Parameter(torch.randn(3))], 1.0)) == 0.0         # nothing has a gradient


def test_the_three_entries_are_declared():
    from aptai_amd import _lib
    declared = set(_lib.declared_symbols())
    for name in ("aptai_grad_sqnorm_multi", "aptai_adam_multi_scaled", "aptai_scale_multi"):
        assert name in declared and name in _lib.ARGTYPES
    assert len(_lib.ARGTYPES["aptai_adam_multi_scaled"]) == len(_lib.ARGTYPES["aptai_adam_multi"]) + 1


def test_workspace_words_follow_the_chunking():
    from aptai_amd import ops
    assert ops.grad_norm_chunks([1, 4096, 4097, 8197, 768 * 768]) == 1 + 1 + 2 + 3 + 144


def test_bad_arguments_are_refused_before_any_launch():
    from aptai_amd import _lib
    with pytest.raises(_lib.AptaiHipError, match="aptai_grad_sqnorm_multi: bad arguments"):
        _lib.call("aptai_grad_sqnorm_multi", None, None, 1, 1, None, None, 1.0, None)
    with pytest.raises(_lib.AptaiHipError, match="max_norm"):
        _lib.call("aptai_grad_sqnorm_multi", 16, 16, 1, 1, 16, 16, -1.0, None)
    with pytest.raises(_lib.AptaiHipError, match="max_norm"):
        _lib.call("aptai_grad_sqnorm_multi", 16, 16, 1, 1, 16, 16, float("nan"), None)
    with pytest.raises(_lib.AptaiHipError, match="grad_scale_dev"):
        _lib.call("aptai_adam_multi_scaled", 16, 16, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None, None)
    with pytest.raises(_lib.AptaiHipError, match="aptai_adam_multi_scaled: betas"):
        _lib.call("aptai_adam_multi_scaled", 16, 16, 1, 1, 1e-3, 1.0, 0.999, 1e-8, 0.0, 16, None)
    with pytest.raises(_lib.AptaiHipError, match="aptai_adam_multi: bad arguments"):
        _lib.call("aptai_adam_multi", 16, 16, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, None)
    with pytest.raises(_lib.AptaiHipError, match="aptai_scale_multi: bad arguments"):
        _lib.call("aptai_scale_multi", 16, 16, 70000, 1, 16, None)
