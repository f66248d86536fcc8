"""CPU: the host side of batch-invariant inference - the first-layer frame count, the loops' flag, the two C-ABI entries."""
import argparse

import pytest
import torch

from aptai_amd import hostlogic

KERNEL = (10, 3, 3, 3, 3, 2, 2)
STRIDE = (5, 2, 2, 2, 2, 2, 2)


def test_conv0_frame_lengths_is_the_first_entry_of_conv_layer_lengths():
    lens = [16000, 5125, 5130, 4321, 10, 14, 15, 160000]
    got = hostlogic.conv0_frame_lengths(torch.tensor(lens))
    assert got.dtype == torch.int32 and got.is_contiguous() and got.shape == (len(lens),)
    assert got.tolist() == [hostlogic.conv_layer_lengths(n, KERNEL, STRIDE)[0] for n in lens]
    assert got.tolist()[:7] == [3199, 1024, 1025, 863, 1, 1, 2]
    # the (B, 1) length tensors the models pass, int32 or int64, give the same vector; every frame's window ends inside the utterance
    assert torch.equal(hostlogic.conv0_frame_lengths(torch.tensor(lens, dtype=torch.int32)[:, None]), got)
    assert all(5 * (t - 1) + 10 <= n for t, n in zip(got.tolist(), lens))
    assert hostlogic.conv0_frame_lengths(torch.tensor([9])).tolist() == [0]          # shorter than one window: refused by the model


def test_batch_invariant_eval_flag_and_default():
    from aptai_amd import loops, train_aptai, train_force_aptai, train_phoneme_recognizer
    ap = argparse.ArgumentParser()
    loops.add_shared_arguments(ap)
    assert loops.shared_arguments(ap.parse_args([]))["batch_invariant_eval"] is False
    assert loops.shared_arguments(ap.parse_args(["--batch_invariant_eval"]))["batch_invariant_eval"] is True
    for mod in (train_aptai, train_force_aptai, train_phoneme_recognizer):
        assert mod.default_cfg().batch_invariant_eval is False
        assert mod.default_cfg(batch_invariant_eval=True).batch_invariant_eval is True


def test_validate_sets_the_attribute_for_the_pass_and_restores_it():
    from aptai_amd import loops

    class Model:
        batch_invariant = False
    seen = []

    @loops.batch_invariant_eval
    def validate(model, fail=False):
        seen.append(model.batch_invariant)
        if fail:
            raise RuntimeError("boom")
        return {"ok": 1}
    m = Model()
    assert validate(m) == {"ok": 1} and validate(m, batch_invariant=True) == {"ok": 1}
    with pytest.raises(RuntimeError):
        validate(m, fail=True, batch_invariant=True)
    assert seen == [False, True, True] and m.batch_invariant is False


def test_models_carry_the_switch_off_by_default():
    from aptai_amd.aptai import APTAI
    from aptai_amd.force_aptai import Force_APTAI
    from aptai_amd.w2v2_pr import Wav2Vec2_PR
    from aptai_amd.wav2vec2 import Wav2Vec2Model
    for cls in (Wav2Vec2Model, APTAI, Wav2Vec2_PR, Force_APTAI):
        assert cls.batch_invariant is False
    assert callable(APTAI.get_aptai_outputs)


def test_exports():
    from aptai_amd import _lib, ops
    names = _lib.declared_symbols()
    L = _lib.lib()
    for n, plain in (("aptai_conv0_fwd_lens", "aptai_conv0_fwd"), ("aptai_lowpass_fir_lens", "aptai_lowpass_fir")):
        assert n in names and n in _lib.ARGTYPES and hasattr(L, n), n
        assert getattr(L, n).argtypes == _lib.ARGTYPES[n]
        # the operands of the plain entry, the length vector, the stream
        assert _lib.ARGTYPES[n] == _lib.ARGTYPES[plain][:-1] + [_lib._P, _lib._P]


def test_null_length_vectors_are_refused_before_any_launch():
    from aptai_amd import _lib
    with pytest.raises(_lib.AptaiHipError, match="aptai_conv0_fwd_lens: null frame_lens0"):
        _lib.call("aptai_conv0_fwd_lens", 16, 1, 16000, 16, None, 16, 16, 0, 1e-5, 16, 3199, 3200, 512, 10, 5, 16, None, None, None)
    with pytest.raises(_lib.AptaiHipError, match="aptai_lowpass_fir_lens: null frame_lens"):
        _lib.call("aptai_lowpass_fir_lens", 16, 9, 64, 16, 51, 16, 9, 49, 0, 1, 49, 49, 9, 9, None, None)
