"""CPU leg of the text encoders (opendwm_amd/text_encoders.py, csrc/text.hip): the fixtures produced by the transformers classes
(tests/golden/make_text_encoder_fixtures.py) against the plain restatement tests/text_ref.py, the proof that those fixtures BITE
(every semantic mutation moves the output by at least 10 x the GPU test's model-level bound), the host-side pieces (T5 buckets and
bias, EOS pooling, dedupe, state-dict keys, argument checks, the C ABI mirror) and the attention checker against an emulation."""
import ctypes
import os
import re

import pytest
import torch

from tests import text_attn_check as T
from tests import text_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CLIP_FIELDS = ("last_hidden_state", "penultimate", "pooler_output", "text_embeds")


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def t5fx():
    fx = torch.load(os.path.join(GOLDEN, "text_encoders_t5.pt"))
    sd = R.make_t5_state_dict(fx["config"], fx["seed"])
    assert R.state_dict_digest(sd) == fx["digest"], "the rebuilt weights are not those the fixture's reference ran on"
    fx["sd"] = {k: v.float() for k, v in sd.items()}
    fx["ref"] = R.t5(fx["sd"], fx["config"], fx["ids"])
    return fx


@pytest.fixture(scope="module")
def clipfx():
    fxs = torch.load(os.path.join(GOLDEN, "text_encoders_clip.pt"))
    for fx in fxs.values():
        sd = R.make_clip_state_dict(fx["config"], fx["seed"])
        assert R.state_dict_digest(sd) == fx["digest"], "the rebuilt weights are not those the fixture's reference ran on"
        fx["sd"] = {k: v.float() for k, v in sd.items()}
        fx["ref"] = R.clip(fx["sd"], fx["config"], fx["ids"])
    return fxs


# ------------------------------------------------------------------------------------------------ restatement vs fixtures
def test_restatement_reproduces_the_t5_fixture(t5fx):
    for k in ("last_hidden_state", "penultimate"):
        assert rel(t5fx["ref"][k], t5fx[k]) <= 1e-5, k
    assert len(t5fx["ref"]["hidden_states"]) == t5fx["n_hidden_states"] == t5fx["config"]["num_layers"] + 1


def test_restatement_reproduces_the_clip_fixtures(clipfx):
    assert set(clipfx) == {"l", "g"}
    assert clipfx["l"]["config"]["eos_token_id"] == 2 and clipfx["g"]["config"]["eos_token_id"] != 2
    for name, fx in clipfx.items():
        for k in CLIP_FIELDS:
            assert rel(fx["ref"][k], fx[k]) <= 1e-5, (name, k)
        assert len(fx["ref"]["hidden_states"]) == fx["n_hidden_states"] == fx["config"]["num_hidden_layers"] + 1
        assert fx["eos_at"] == [10, 40, 76]


def test_t5_buckets_and_bias_equal_the_fixture_for_every_length(t5fx):
    from opendwm_amd import text_encoders as E
    want_b, want_bias = t5fx["buckets128"].long(), t5fx["bias128"]
    table = t5fx["sd"]["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    for L in range(1, 129):
        b = E.t5_relative_buckets(L, 32, 128)
        assert torch.equal(b, want_b[:L, :L]), L
        assert torch.equal(E.t5_relative_bias(table, L, 32, 128), want_bias[:, :L, :L]), L
    assert torch.equal(R.t5_buckets(128), want_b)
    assert int(want_b.max()) == 31 and int(want_b.min()) == 0
    assert not torch.equal(want_bias, want_bias.transpose(-1, -2))                # transposing the bias is not a no-op


# ------------------------------------------------------------------------------------------------------------ sensitivity
def test_the_fixtures_bite(t5fx, clipfx):
    """a condition on the committed fixtures: each mutation moves the restatement by >= 10 x the model-level bound of the GPU test
    (2 x bf16_ref_err) on the outputs it concerns"""
    cfg, sd, ids = t5fx["config"], t5fx["sd"], t5fx["ids"]
    floor = {k: 20 * v for k, v in t5fx["bf16_ref_err"].items()}
    for name, mut in (("1/8 scale", R.Mut(t5_scale=0.125)), ("bias zeroed", R.Mut(bias="zero")), ("bias transposed", R.Mut(bias="transposed"))):
        o = R.t5(sd, cfg, ids, mut)
        for k in ("last_hidden_state", "penultimate"):
            assert rel(o[k], t5fx[k]) >= floor[k], (name, k, rel(o[k], t5fx[k]), floor[k])
    assert rel(R.t5(sd, cfg, ids, R.Mut(hidden=-1))["penultimate"], t5fx["penultimate"]) >= floor["penultimate"]
    for fname, fx in clipfx.items():
        cfg, sd, ids = fx["config"], fx["sd"], fx["ids"]
        floor = {k: 20 * v for k, v in fx["bf16_ref_err"].items()}
        for name, mut in (("no scale", R.Mut(clip_scale=1.0)), ("non-causal", R.Mut(causal=False))):
            o = R.clip(sd, cfg, ids, mut)
            for k in CLIP_FIELDS:
                assert rel(o[k], fx[k]) >= floor[k], (fname, name, k, rel(o[k], fx[k]), floor[k])
        assert rel(R.clip(sd, cfg, ids, R.Mut(hidden=-1))["penultimate"], fx["penultimate"]) >= floor["penultimate"]
        o = R.clip(sd, cfg, ids, R.Mut(pool_shift=-1))
        for k in ("pooler_output", "text_embeds"):
            assert rel(o[k], fx[k]) >= floor[k], (fname, "pooled row off by one", k)
    # the GELU variants differ by less than that end to end - they are told apart at kernel level (tests/test_text_kernels_gpu.py)
    fx = clipfx["l"]
    other = R.clip(fx["sd"], dict(fx["config"], hidden_act="gelu"), fx["ids"])
    assert rel(other["last_hidden_state"], fx["last_hidden_state"]) < 20 * fx["bf16_ref_err"]["last_hidden_state"]


# ------------------------------------------------------------------------------------------------------------ the classes
def test_state_dict_keys_equal_the_checkpoints(t5fx, clipfx):
    from opendwm_amd import text_encoders as E
    m = E.T5EncoderModel(t5fx["config"])
    assert sorted(m.state_dict()) == t5fx["keys"]
    m.load_state_dict({k: v for k, v in t5fx["sd"].items() if k != "encoder.embed_tokens.weight"})     # the tied table under one name
    assert torch.equal(m.encoder.embed_tokens.weight, t5fx["sd"]["shared.weight"])
    for name, fx in clipfx.items():
        m = E.CLIPTextModelWithProjection(fx["config"])
        assert sorted(m.state_dict()) == fx["keys"]
        m.load_state_dict(fx["sd"])
        plain = E.CLIPTextModel(**fx["config"])
        assert sorted(plain.state_dict()) == [k for k in fx["keys"] if k != "text_projection.weight"]
        unprefixed = {k[len("text_model."):]: v for k, v in fx["sd"].items() if k.startswith("text_model.")}
        plain.load_state_dict(dict(unprefixed, **{"embeddings.position_ids": torch.arange(77)[None]}))
        assert torch.equal(plain.text_model.final_layer_norm.bias, fx["sd"]["text_model.final_layer_norm.bias"])
        assert plain.requires_grad_(False) is plain and plain.dtype == torch.float32 and plain.device.type == "cpu"
        with pytest.raises(RuntimeError):
            plain(fx["ids"])                                        # no CPU / fp32 fallback
    with pytest.raises(NotImplementedError):
        E.CLIPTextModel(hidden_size=128, num_attention_heads=4)
    with pytest.raises(NotImplementedError):
        E.T5EncoderModel(dict(t5fx["config"], d_kv=32))
    with pytest.raises(NotImplementedError):
        E.T5EncoderModel(dict(t5fx["config"], feed_forward_proj="relu"))


def test_eos_pooling_rule(clipfx):
    from opendwm_amd import text_encoders as E
    for fx in clipfx.values():
        assert E.eos_positions(fx["ids"], fx["config"]["eos_token_id"]).tolist() == fx["eos_at"]
    ids = clipfx["g"]["ids"]
    assert E.eos_positions(ids, 2).tolist() != clipfx["g"]["eos_at"]              # the legacy rule would pool another row there


def test_output_object_indexing():
    from opendwm_amd.text_encoders import CLIPTextModel, CLIPTextModelWithProjection, T5EncoderModel, TextEncoderOutput
    a, b, c = torch.zeros(1), torch.ones(1), (torch.zeros(1),)
    o = TextEncoderOutput(CLIPTextModelWithProjection.OUTPUT_ORDER, text_embeds=a, last_hidden_state=b, pooler_output=a)
    assert o[0] is a and o[1] is b and o.hidden_states is None and len(o.to_tuple()) == 2
    o = TextEncoderOutput(CLIPTextModel.OUTPUT_ORDER, last_hidden_state=b, pooler_output=a, hidden_states=c)
    assert o[0] is b and o[1] is a and o[2] is c and o["pooler_output"] is a
    assert TextEncoderOutput(T5EncoderModel.OUTPUT_ORDER, last_hidden_state=b)[0] is b


def test_dedupe_index_logic():
    from opendwm_amd.text_encoders import SD3TextEncoders, dedupe_rows
    ids = torch.tensor([[5, 1, 1], [0, 0, 0], [5, 1, 1], [7, 7, 2], [0, 0, 0], [0, 0, 0]])
    distinct, index = dedupe_rows(ids)
    assert distinct.shape == (3, 3) and torch.equal(distinct[index], ids)
    calls = []

    def fn(x):
        calls.append(x.shape[0])
        return x.float() * 2, x.sum(1, keepdim=True)

    a, b = SD3TextEncoders._run(fn, ids, True)
    a2, b2 = SD3TextEncoders._run(fn, ids, False)
    assert calls == [3, 6] and torch.equal(a, a2) and torch.equal(b, b2)


# ------------------------------------------------------------------------------------------------------------- the C ABI
def test_ctypes_mirror_header_and_sources():
    from opendwm_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
    assert _lib.ABI_VERSION == 18 and re.search(r"#define DWM_ABI_VERSION 18\b", hdr)          # additions only
    body = hdr[hdr.index("typedef struct dwm_text_attn_args"):hdr.index("} dwm_text_attn_args;")]
    names = re.findall(r"[\s\*,]([A-Za-z_0-9]+)\s*[,;]", body)
    assert names == [f for f, _ in _lib.TextAttnArgs._fields_]
    kinds = dict(_lib.TextAttnArgs._fields_)
    assert kinds["heads"] is _lib._i32 and kinds["scale"] is _lib._f32 and kinds["L"] is _lib._i64 and kinds["bias"] is _lib._vp
    for name, arity in (("dwm_text_attention", 2), ("dwm_rmsnorm_rows", 9), ("dwm_text_embed", 10), ("dwm_text_act", 9)):
        m = re.search(rf"^int {name}\(([^;]*)\);", hdr, flags=re.M)
        assert m and len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
    assert "text.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "text.hip"))


def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    from opendwm_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    fake = 1 << 20
    for name in ("dwm_text_attention", "dwm_rmsnorm_rows", "dwm_text_embed", "dwm_text_act"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]

    def attn(**kw):
        a = _lib.TextAttnArgs()
        a.q = a.k = a.v = a.out = fake
        a.ld, a.ldo, a.n_seq, a.L, a.heads, a.scale, a.causal = 192, 64, 2, 77, 1, 1.0, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.dwm_text_attention(ctypes.byref(a), None)

    assert attn(L=0) == -3 and attn(L=129) == -3 and attn(L=129, q=None) == -1
    assert attn(ld=63) == -1 and attn(ld=196) == -2 and attn(q=fake + 2) == -2 and attn(causal=2) == -1 and attn(n_seq=0) == -1
    assert lib.dwm_rmsnorm_rows(fake, 64, 1, 60, fake, 1e-6, fake, 64, None) == -3
    assert lib.dwm_rmsnorm_rows(fake, 8200, 1, 8200, fake, 1e-6, fake, 8200, None) == -3
    assert lib.dwm_rmsnorm_rows(fake, 32, 1, 64, fake, 1e-6, fake, 64, None) == -1
    assert lib.dwm_text_embed(fake, 4, fake, 0, 64, None, 0, fake, 64, None) == -1
    assert lib.dwm_text_embed(fake, 4, fake, 10, 60, None, 0, fake, 64, None) == -3
    assert lib.dwm_text_act(fake, 64, 1, 64, 3, 0, fake, 64, None) == -1
    assert lib.dwm_text_act(fake, 64, 1, 64, 0, 1, fake, 64, None) == -1             # gated needs 2 F columns


def test_wrapper_argument_checks():
    from opendwm_amd import ops
    x = torch.zeros(77, 64, dtype=torch.bfloat16)
    for L in (0, 129):
        with pytest.raises(NotImplementedError):
            ops.text_attention(x, x, x, x, 1, L, 1, 1.0)
    with pytest.raises(NotImplementedError):
        ops.text_attention(x, x, x, x, 1, 77, 2, 1.0)                                # head width 32
    table = torch.zeros(10, 64, dtype=torch.bfloat16)
    for bad in (torch.tensor([[0, 10]]), torch.tensor([[-1, 3]])):
        with pytest.raises(ValueError):
            ops.text_embed(bad, table)
    with pytest.raises(RuntimeError):
        ops.text_embed(torch.tensor([[0, 9]]), table)                                # in range: goes on to "expected a device tensor"
    with pytest.raises(NotImplementedError):
        ops.text_act(x, "relu")


# ------------------------------------------------------------------------------------------- the attention checker bites
@pytest.mark.parametrize("mode", T.MODES)
def test_attention_checker_admits_a_correct_kernel_and_catches_faults(mode):
    L, H, n_seq, scale, causal = 77, 2, 2, 0.125, "causal" in mode
    q, k, v, bias = T.make_inputs(n_seq, L, H, mode, scale, 5, "cpu")
    W = T.Weights(q, k, bias, n_seq, L, H, scale, causal)
    o, bound = T.o_reference(W, v, n_seq, H)
    assert T.worst(T.element_ratios(T.emulate(q, k, v, bias, n_seq, L, H, scale, causal), o, bound, n_seq, L, H))[0] <= 0.7
    for c in range(2):
        got = T.emulate(q, k, T.v_onehot(n_seq, L, H, c, "cpu"), bias, n_seq, L, H, scale, causal)
        assert T.worst(T.census_ratios(got, W, c, n_seq, H))[0] <= 0.8
    faults = ["no_scale"] + (["one_key_more", "addend"] if causal else []) + (["bias_transposed"] if bias is not None else [])
    for fault in faults:
        bad = T.emulate(q, k, v, bias, n_seq, L, H, scale, causal, fault=fault)
        assert T.worst(T.element_ratios(bad, o, bound, n_seq, L, H))[0] > 10, fault
    if causal:                                                   # a hidden key with a nonzero weight is an infinite census ratio
        got = T.emulate(q, k, T.v_onehot(n_seq, L, H, 0, "cpu"), bias, n_seq, L, H, scale, causal, fault="addend")
        assert T.worst(T.census_ratios(got, W, 0, n_seq, H))[0] == float("inf")


def test_generator_reproduces_the_committed_fixtures(t5fx, clipfx):
    pytest.importorskip("transformers")
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_text_encoder_fixtures", os.path.join(GOLDEN, "make_text_encoder_fixtures.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    t5, clip = mod.build()
    for k in ("last_hidden_state", "penultimate", "bias128"):
        assert float((t5[k] - t5fx[k]).abs().max()) == 0, k
    assert torch.equal(t5["buckets128"], t5fx["buckets128"]) and torch.equal(t5["ids"], t5fx["ids"])
    for name in clip:
        for k in CLIP_FIELDS:
            assert float((clip[name][k] - clipfx[name][k]).abs().max()) == 0, (name, k)
