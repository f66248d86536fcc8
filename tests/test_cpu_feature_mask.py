"""CPU: the host side of SpecAugment along the feature axis (mask_feature_prob; HF `_mask_hidden_states`, second half): the new entry
points are declared, exported and typed; the loop flags reach the W2V2Config; W2V2Config.validate() raises HF's ValueErrors early; the
span-count refusal; and the numpy sampler path keeps HF's RNG order (time mask, then feature mask).  The device side is
tests/test_gpu_feature_mask.py."""
import argparse

import numpy as np
import pytest
import torch

from aptai_amd import hostlogic
from aptai_amd.config import W2V2Config

NEW = ("aptai_frame_feature_mask_fwd", "aptai_frame_feature_mask_bwd")


def test_new_entry_points_are_declared_exported_and_typed():
    from aptai_amd import _lib, ops
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n in NEW:
        assert n in names and n in _lib.ARGTYPES and hasattr(L, n), n
        assert getattr(L, n).argtypes == _lib.ARGTYPES[n]
    # the arguments of aptai_frame_mask_fwd / _bwd plus one pointer (the feature mask)
    assert len(_lib.ARGTYPES["aptai_frame_feature_mask_fwd"]) == len(_lib.ARGTYPES["aptai_frame_mask_fwd"]) + 1
    assert len(_lib.ARGTYPES["aptai_frame_feature_mask_bwd"]) == len(_lib.ARGTYPES["aptai_frame_mask_bwd"]) + 1
    import inspect
    for w in ("frame_mask_fwd", "frame_mask_bwd"):                     # one wrapper pair: the feature mask is an optional argument
        assert inspect.signature(getattr(ops, w)).parameters["feat_mask_u8"].default is None


def test_wrappers_refuse_host_tensors():
    from aptai_amd import _lib, ops
    h = torch.zeros(8, 8, dtype=torch.bfloat16)
    lens = torch.ones(1, dtype=torch.int32)
    feat = torch.zeros(1, 8, dtype=torch.uint8)
    with pytest.raises(_lib.AptaiHipError):
        ops.frame_mask_fwd(h, lens, None, None, 1, 8, 8, 8, feat_mask_u8=feat)
    with pytest.raises(_lib.AptaiHipError):
        ops.frame_mask_bwd(h, lens, None, 1, 8, 8, 8, want_dembed=False, feat_mask_u8=feat)


def _parse(argv):
    from aptai_amd import loops
    ap = argparse.ArgumentParser()
    loops.add_shared_arguments(ap)
    return ap.parse_args(argv)


def test_flags_absent_leave_the_config_untouched():
    from aptai_amd import loops
    a = _parse([])
    assert a.mask_feature_prob is None and a.mask_feature_length is None
    sh = loops.shared_arguments(a)
    assert sh["mask_feature_prob"] is None and sh["mask_feature_length"] is None
    cfg = W2V2Config.base(mask_feature_prob=0.04, mask_feature_length=32)
    before = cfg.to_dict()
    assert loops.apply_mask_feature_arguments(cfg, a) is cfg
    assert cfg.to_dict() == before
    d = loops.default_cfg({})                                          # a loop cfg built without the flags carries "not given"
    assert d.mask_feature_prob is None and d.mask_feature_length is None


def test_flags_given_are_applied_and_validated():
    from aptai_amd import loops
    a = _parse(["--mask_feature_prob", "0.1", "--mask_feature_length", "64"])
    sh = loops.shared_arguments(a)
    assert sh["mask_feature_prob"] == 0.1 and sh["mask_feature_length"] == 64
    cfg = W2V2Config.base()
    before = cfg.to_dict()
    loops.apply_mask_feature_arguments(cfg, a)
    assert (cfg.mask_feature_prob, cfg.mask_feature_length) == (0.1, 64)
    after = cfg.to_dict()
    assert {k for k in after if after[k] != before[k]} == {"mask_feature_prob", "mask_feature_length"}
    # one flag alone: the other field keeps the checkpoint's value
    cfg = W2V2Config.large(mask_feature_length=7)
    loops.apply_mask_feature_arguments(cfg, _parse(["--mask_feature_prob", "0.2"]))
    assert (cfg.mask_feature_prob, cfg.mask_feature_length) == (0.2, 7)
    # a loop cfg (loops.default_cfg) carries them the same way
    cfg = W2V2Config.base()
    loops.apply_mask_feature_arguments(cfg, loops.default_cfg(sh))
    assert (cfg.mask_feature_prob, cfg.mask_feature_length) == (0.1, 64)
    with pytest.raises(ValueError):                                    # longer than the hidden axis: refused before a model is built
        loops.apply_mask_feature_arguments(W2V2Config.base(), _parse(["--mask_feature_prob", "0.1", "--mask_feature_length", "769"]))


def test_validate_raises_only_when_the_feature_mask_is_on():
    W2V2Config().validate()
    W2V2Config.large().validate()
    # off: the length fields are not looked at
    W2V2Config.base(mask_feature_prob=0.0, mask_feature_length=0).validate()
    W2V2Config.base(mask_feature_prob=0.0, mask_feature_length=5000).validate()
    W2V2Config.from_any({"mask_feature_prob": 0.0, "mask_feature_length": 0})
    # on: HF's own errors, early
    with pytest.raises(ValueError, match="bigger than 0"):
        W2V2Config.base(mask_feature_prob=0.1, mask_feature_length=0).validate()
    with pytest.raises(ValueError, match="smaller than `sequence_length`"):
        W2V2Config.base(mask_feature_prob=0.1, mask_feature_length=769).validate()
    W2V2Config.base(mask_feature_prob=0.1, mask_feature_length=768).validate()
    W2V2Config.large(mask_feature_prob=0.1, mask_feature_length=1024).validate()
    with pytest.raises(ValueError, match="mask_feature_prob"):
        W2V2Config.base(mask_feature_prob=1.5).validate()
    W2V2Config.base(mask_feature_prob=1.0).validate()
    with pytest.raises(ValueError):
        W2V2Config.from_any({"mask_feature_prob": 0.1, "mask_feature_length": 0})


def test_span_count_above_the_sampler_cap_is_refused_on_the_host():
    from aptai_amd import ops
    assert ops.SPEC_MAX_SPANS == 256
    ops.feature_mask_span_check(768, 0.25, 10, 0)                      # 20 spans at the most
    ops.feature_mask_span_check(1024, 0.01, 512, 1)
    ops.feature_mask_span_check(768, 0.33, 1, 256)                     # int(253.44 + 1) = 254, min_masks at the cap
    with pytest.raises(ValueError, match="256"):
        ops.feature_mask_span_check(768, 0.5, 1, 0)                    # int(384 + 1) spans
    with pytest.raises(ValueError, match="256"):
        ops.feature_mask_span_check(768, 0.01, 2, 257)                 # min_masks alone


@pytest.mark.parametrize("ragged", [False, True])
def test_host_path_draws_the_time_mask_then_the_feature_mask(ragged):
    """One np.random.seed, HF's order: `_compute_mask_indices` over (B, T) with the attention mask, then over (B, H) without one."""
    from aptai_amd import wav2vec2
    cfg = W2V2Config.base(mask_time_prob=0.05, mask_time_length=10, mask_time_min_masks=2, mask_feature_prob=0.1,
                          mask_feature_length=16, mask_feature_min_masks=1)
    B, T, H = 3, 49, cfg.hidden_size
    fl = torch.tensor([49, 30, 41]) if ragged else None
    np.random.seed(11)
    got_t, got_f = wav2vec2._host_spec_masks(cfg, B, T, fl, True, True)
    np.random.seed(11)
    am = None if fl is None else torch.arange(T)[None, :] < fl[:, None]
    want_t = hostlogic.compute_mask_indices((B, T), 0.05, 10, attention_mask=am, min_masks=2)
    want_f = hostlogic.compute_mask_indices((B, H), 0.1, 16, min_masks=1)
    assert got_t.shape == (B, T) and got_f.shape == (B, H)
    assert np.array_equal(got_t, want_t) and np.array_equal(got_f, want_f)
    assert want_f.any() and not np.array_equal(want_f[0], want_f[1])
    # the order matters: drawn the other way round, the same seed gives other masks
    np.random.seed(11)
    swapped_f = hostlogic.compute_mask_indices((B, H), 0.1, 16, min_masks=1)
    assert not np.array_equal(swapped_f, want_f)
    # the feature mask alone (mask_time_prob = 0 or an explicit mask_time_indices): the first draw of the stream
    np.random.seed(11)
    none_t, only_f = wav2vec2._host_spec_masks(cfg, B, T, fl, False, True)
    assert none_t is None and np.array_equal(only_f, swapped_f)
    # and the time mask alone is what the path drew before the feature axis existed
    np.random.seed(11)
    only_t, none_f = wav2vec2._host_spec_masks(cfg, B, T, fl, True, False)
    assert none_f is None and np.array_equal(only_t, want_t)
