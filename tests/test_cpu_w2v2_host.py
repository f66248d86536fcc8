"""CPU: the host side of Wav2Vec2Model that needs no device - the seed-stream table and `_seed`, the declared state of a fresh model,
the parameter lists the front end and the layers are driven with, and the one rule that decides when a compute copy is rebuilt."""
import itertools

import pytest

from aptai_amd import wav2vec2
from aptai_amd.config import W2V2Config
from aptai_amd.wav2vec2 import Wav2Vec2Model, _copies_stale, _seed


@pytest.fixture(scope="module", params=["base", "large"])
def model(request):
    return Wav2Vec2Model(getattr(W2V2Config, request.param)(num_hidden_layers=2))


def test_seed_stream_table():
    want = dict(_ATTN_DROPOUT_STREAM=1, _OUT_PROJ_DROPOUT_STREAM=2, _ACT_DROPOUT_STREAM=3, _FFN2_DROPOUT_STREAM=4,
                _PROJ_DROPOUT_STREAM=11, _FRONT_DROPOUT_STREAM=12, _TIME_MASK_STREAM=77, _FEATURE_MASK_STREAM=78,
                _LAYER_STREAM_BASE=100, _PR_HEAD_STREAM=777, _APTAI_HEADS_STREAM=999, _FORCE_HEADS_STREAM=4242)
    got = {n: v for n, v in vars(wav2vec2).items() if n.endswith("_STREAM") or n.endswith("_STREAM_BASE")}
    assert got == want
    assert all(type(v) is int for v in got.values())


def test_seed_of_fixed_inputs_is_pinned():
    # computed with _seed as it stood before the streams had names
    assert _seed(0x5EED, 7) == 0x0A57A006A97EDDA0
    assert _seed(0x5EED, 7, 100) == 0xE90EFC510BB1A697
    assert _seed(0xFFFFFFFFFFFFFF, 4242) == 0xEABDF601BFFAFB57       # the base is cut to 48 bits
    assert _seed(0) == 0
    assert _seed(0x5EED, 7, wav2vec2._LAYER_STREAM_BASE) == 0xE90EFC510BB1A697


def test_fresh_model_declares_its_state(model):
    assert model.encoder_precision == "bf16" and model._encoder_precision == "bf16"
    assert model._cache_mode is None and model._train_marker == 0
    assert model._lplan is None and model._feat_lens is None
    with pytest.raises(AttributeError):
        model.encoder_precision = "mxfp8"                             # read-only: set_encoder_precision checks the name


def test_set_encoder_precision_rejects_an_unknown_name(model):
    with pytest.raises(ValueError, match="encoder precision"):
        model.set_encoder_precision("fp8_e5m2")
    assert model.encoder_precision == "bf16"
    for name in ("mxfp8", "bf16_f32res", "f32x3", "f32x6", "bf16"):
        assert model.set_encoder_precision(name) is model and model.encoder_precision == name


def test_front_params_are_the_ten_entries_front_impl_reads(model):
    fp, pc, enc = model.feature_projection, model.encoder.pos_conv_embed.conv, model.encoder
    want = [fp.layer_norm.weight, fp.layer_norm.bias, fp.projection.weight, fp.projection.bias, model.masked_spec_embed,
            pc.parametrizations.weight.original0, pc.parametrizations.weight.original1, pc.bias, enc.layer_norm.weight,
            enc.layer_norm.bias]
    got = model._front_params(with_embed=True)
    assert len(got) == 10 and all(a is b for a, b in zip(got, want))
    assert got._fields == ("fp_ln_w", "fp_ln_b", "proj_w", "proj_b", "embed", "pc_gain", "pc_v", "pc_bias", "enc_ln_w", "enc_ln_b")
    assert wav2vec2._FrontParams(*list(got)) == got                   # what _FrontImpl.fwd does with the list it is handed
    none = model._front_params(with_embed=False)
    assert none.embed is None and [i for i, t in enumerate(none) if t is None] == [4]
    assert all(a is b for i, (a, b) in enumerate(zip(none, want)) if i != 4)


def test_front_params_of_a_model_without_a_mask_embedding():
    m = Wav2Vec2Model(W2V2Config.base(num_hidden_layers=1, mask_time_prob=0.0, mask_feature_prob=0.0))
    assert not hasattr(m, "masked_spec_embed")
    assert m._front_params(with_embed=True).embed is None


def test_layer_parameter_order_is_the_gradient_order_of_the_layer_backward(model):
    for i, l in enumerate(model.encoder.layers):
        at, ff = l.attention, l.feed_forward
        # _LayerImpl.bwd: dg1 db1 dg2 db2, dW q k v, db q k v, out-proj W b, FFN1 W b, FFN2 W b
        want = [l.layer_norm.weight, l.layer_norm.bias, l.final_layer_norm.weight, l.final_layer_norm.bias,
                at.q_proj.weight, at.k_proj.weight, at.v_proj.weight, at.q_proj.bias, at.k_proj.bias, at.v_proj.bias,
                at.out_proj.weight, at.out_proj.bias, ff.intermediate_dense.weight, ff.intermediate_dense.bias,
                ff.output_dense.weight, ff.output_dense.bias]
        got = model._layer_ln_params(i) + model._layer_params(i)
        assert len(got) == 16 and all(a is b for a, b in zip(got, want))


# (training, any parameter trainable, version key equal, optimiser publishes the copies, last cast came from a training forward) -> rebuild
# with no cache mode set: the decisions of _refresh_layer_copies as it stood with its own copy of the rule
_LAYER_COPIES = [
    (0, 0, 0, 0, 0, 1), (0, 0, 0, 0, 1, 1), (0, 0, 0, 1, 0, 1), (0, 0, 0, 1, 1, 1),
    (0, 0, 1, 0, 0, 0), (0, 0, 1, 0, 1, 1), (0, 0, 1, 1, 0, 0), (0, 0, 1, 1, 1, 0),
    (0, 1, 0, 0, 0, 1), (0, 1, 0, 0, 1, 1), (0, 1, 0, 1, 0, 1), (0, 1, 0, 1, 1, 1),
    (0, 1, 1, 0, 0, 0), (0, 1, 1, 0, 1, 1), (0, 1, 1, 1, 0, 0), (0, 1, 1, 1, 1, 0),
    (1, 0, 0, 0, 0, 1), (1, 0, 0, 0, 1, 1), (1, 0, 0, 1, 0, 1), (1, 0, 0, 1, 1, 1),
    (1, 0, 1, 0, 0, 0), (1, 0, 1, 0, 1, 1), (1, 0, 1, 1, 0, 0), (1, 0, 1, 1, 1, 0),
    (1, 1, 0, 0, 0, 1), (1, 1, 0, 0, 1, 1), (1, 1, 0, 1, 0, 1), (1, 1, 0, 1, 1, 1),
    (1, 1, 1, 0, 0, 1), (1, 1, 1, 0, 1, 1), (1, 1, 1, 1, 0, 0), (1, 1, 1, 1, 1, 0),
]
# (training, any parameter trainable, cache hit with an equal version key) -> rebuild: the decisions of _cached as it stood
_CACHED = [(0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 1), (0, 1, 1, 0), (1, 0, 0, 1), (1, 0, 1, 0), (1, 1, 0, 1), (1, 1, 1, 1)]


def test_staleness_rule_truth_table():
    assert len(set(r[:5] for r in _LAYER_COPIES)) == 32 and len(set(r[:3] for r in _CACHED)) == 8
    for tr, tb, ve, sy, af, want in _LAYER_COPIES:
        assert _copies_stale(None, bool(tr), bool(tb), bool(ve), bool(sy), bool(af)) is bool(want), (tr, tb, ve, sy, af)
    for tr, tb, ve, want in _CACHED:
        assert _copies_stale(None, bool(tr), bool(tb), bool(ve)) is bool(want), (tr, tb, ve)
    # the two capture modes outrank every other input: "build" always rebuilds, "frozen" never does
    for flags in itertools.product((False, True), repeat=5):
        assert _copies_stale("build", *flags) is True
        assert _copies_stale("frozen", *flags) is False


def test_cached_follows_the_rule_without_a_device():
    """_cached on host tensors (the builder is plain torch here): hit, miss, the two capture modes, and weights_moved()."""
    model = Wav2Vec2Model(W2V2Config.base(num_hidden_layers=1))
    w = model.feature_projection.projection.weight
    built = []

    def build():
        built.append(1)
        return w.detach().clone()
    model.eval()
    a = model._cached(("t",), [w], build)
    assert model._cached(("t",), [w], build) is a and len(built) == 1          # eval: the version key is trusted
    model.weights_moved()                                                        # moves the marker: eval copies miss once
    b = model._cached(("t",), [w], build)
    assert b is not a and len(built) == 2 and model._cached(("t",), [w], build) is b
    model.train()
    model._cached(("t",), [w], build)
    assert len(built) == 3                                                       # training, trainable: every time
    w.requires_grad_(False)
    try:
        c = model._cached(("t",), [w], build)
        assert model._cached(("t",), [w], build) is c and len(built) == 3       # training, frozen parameter: trusted again
        model._cache_mode = "build"
        model._cached(("t",), [w], build)
        assert len(built) == 4
        model._cache_mode = "frozen"
        assert model._cached(("t",), [w], build) is model._cache[("t",)][1] and len(built) == 4
        with pytest.raises(KeyError):
            model._cached(("never built",), [w], build)
        model.weights_moved()                                                    # un-freezes and clears, as suspend() does
        assert model._cache_mode is None and model._cache == {}
    finally:
        model._cache_mode = None
