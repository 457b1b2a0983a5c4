"""GPU leg of the text encoders (opendwm_amd/text_encoders.py): the three small models against the fixtures the transformers classes
produced (tests/golden/make_text_encoder_fixtures.py).

Bound: relative Frobenius error <= 2 x bf16_ref_err, the error of the SAME transformers model run in bf16 on the CPU against its
fp32 run, recorded in the fixture.  The HIP path stores what that run stores (bf16 weights and activations), sums in another order
and keeps an fp32 residual stream in its favour; the factor 2 is margin for the reordering and nothing else.  tests/
test_text_encoders_cpu.py shows that every semantic mutation is at least 10 x this bound away.

Measured on an MI355X (this file, printed by each test): see DESIGN.md §23."""
import os

import pytest
import torch

from tests import text_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
bf16 = torch.bfloat16


def rel(a, b):
    return float((a.double().cpu() - b.double()).norm() / b.double().norm())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models(dev):
    """fixtures + the three models (and the plain CLIPTextModel of "g"), loaded once"""
    from opendwm_amd import text_encoders as E
    t5fx = torch.load(os.path.join(GOLDEN, "text_encoders_t5.pt"))
    clipfx = torch.load(os.path.join(GOLDEN, "text_encoders_clip.pt"))
    t5 = E.T5EncoderModel(t5fx["config"])
    t5.load_state_dict(R.make_t5_state_dict(t5fx["config"], t5fx["seed"]))
    out = dict(t5fx=t5fx, clipfx=clipfx, t5=t5.to(dev).to(bf16).requires_grad_(False))
    for name, fx in clipfx.items():
        sd = R.make_clip_state_dict(fx["config"], fx["seed"])
        assert R.state_dict_digest(sd) == fx["digest"]
        m = E.CLIPTextModelWithProjection(fx["config"])
        m.load_state_dict(sd)
        out[name] = m.to(dev).to(bf16).requires_grad_(False)
    plain = E.CLIPTextModel(clipfx["g"]["config"])
    plain.load_state_dict({k: v for k, v in R.make_clip_state_dict(clipfx["g"]["config"], clipfx["g"]["seed"]).items()
                           if k != "text_projection.weight"})
    out["plain"] = plain.to(dev).to(bf16)
    return out


def _check(name, got, fx, key):
    e, bound = rel(got, fx[key]), 2 * fx["bf16_ref_err"][key]
    print(f"{name} {key}: rel err {e:.3e}  bound {bound:.3e} (bf16_ref_err {fx['bf16_ref_err'][key]:.3e})")
    assert e <= bound, (name, key, e, bound)


def test_t5_against_the_transformers_fixture(models):
    fx, m = models["t5fx"], models["t5"]
    assert m.dtype == bf16 and m.device.type == "cuda"
    o = m(fx["ids"], output_hidden_states=True)
    assert len(o.hidden_states) == fx["n_hidden_states"] and o[0] is o.last_hidden_state and o.last_hidden_state.dtype == bf16
    _check("t5", o.last_hidden_state, fx, "last_hidden_state")
    _check("t5", o.hidden_states[-2], fx, "penultimate")
    again = m(fx["ids"])
    assert again.hidden_states is None and torch.equal(again[0], o[0])                       # two runs are bit-equal
    assert torch.equal(m.relative_bias(77).cpu(), fx["bias128"][:, :77, :77])
    # after packing, the parameters are views of the packed operands: the state dict still reads back the checkpoint
    sd = R.make_t5_state_dict(fx["config"], fx["seed"])
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items())


@pytest.mark.parametrize("name", ["l", "g"])
def test_clip_against_the_transformers_fixture(models, name):
    fx, m = models["clipfx"][name], models[name]
    o = m(fx["ids"], output_hidden_states=True)
    assert len(o.hidden_states) == fx["n_hidden_states"] and o[0] is o.text_embeds
    _check(name, o.last_hidden_state, fx, "last_hidden_state")
    _check(name, o.hidden_states[-2], fx, "penultimate")
    _check(name, o.text_embeds, fx, "text_embeds")
    _check(name, o.pooler_output, fx, "pooler_output")
    again = m(fx["ids"].to(m.device))                                                        # ids already on the device
    assert again.hidden_states is None and torch.equal(again[0], o[0]) and torch.equal(again.last_hidden_state, o.last_hidden_state)
    sd = R.make_clip_state_dict(fx["config"], fx["seed"])
    assert all(torch.equal(v.cpu(), sd[k]) for k, v in m.state_dict().items())


def test_clip_text_model_without_projection(models):
    fx, m = models["clipfx"]["g"], models["plain"]
    o = m(fx["ids"])
    assert o[0] is o.last_hidden_state and o[1] is o.pooler_output and o.text_embeds is None
    _check("plain", o.last_hidden_state, fx, "last_hidden_state")
    _check("plain", o.pooler_output, fx, "pooler_output")
    from opendwm_amd import conditions
    e = conditions.encode_clip_text(m, fx["ids"], [3], 2, 4)
    assert e.shape == (3, 2, 4, 77, 192) and torch.equal(e[:, 1, 3], o[0])


def test_sd3_triple_dedupe_bit_equal_and_assembly(models):
    from opendwm_amd import conditions
    from opendwm_amd.text_encoders import SD3TextEncoders
    enc = SD3TextEncoders(models["l"], models["g"], models["t5"])
    pick = torch.tensor([0, 1, 0, 2, 1, 0, 0, 2])                         # a flat prompt list with repeats, as under CFG / shared prompts
    ids = [models["clipfx"]["l"]["ids"][pick], models["clipfx"]["g"]["ids"][pick], models["t5fx"]["ids"][pick]]
    h, p, t5 = enc.encode(*ids, dedupe=True)
    h2, p2, t52 = enc.encode(*ids, dedupe=False)
    for a, b in zip(h + p + [t5], h2 + p2 + [t52]):
        assert a.shape[0] == 8 and torch.equal(a, b)                      # rows are independent: bit-equal
    text, pooled = conditions.encode_sd3_text(enc, *ids, [2, 2, 2], 2, 2, bf16)
    assert text.shape == (2, 2, 2, 154, 128) and pooled.shape == (2, 2, 2, 192)
    # the CPU assembly of the fixture tensors
    fl, fg, ft = models["clipfx"]["l"], models["clipfx"]["g"], models["t5fx"]
    want_text, want_pooled = conditions.assemble_sd3_text(
        [fl["penultimate"][pick], fg["penultimate"][pick]], [fl["text_embeds"][pick], fg["text_embeds"][pick]],
        ft["last_hidden_state"][pick], [2, 2, 2], 2, 2, torch.float32)
    # (the toy T5 is narrower than the two CLIP widths together, so the "padding" of the assembly crops the CLIP block to its first 128
    # features - on both sides alike; CLIP-G's hidden state is checked in test_clip_against_the_transformers_fixture)
    assert want_text.shape == text.shape and want_pooled.shape == pooled.shape
    assert rel(text[..., :77, :], want_text[..., :77, :]) <= 2 * fl["bf16_ref_err"]["penultimate"]
    assert rel(text[..., 77:, :], want_text[..., 77:, :]) <= 2 * ft["bf16_ref_err"]["last_hidden_state"]
    assert rel(pooled, want_pooled) <= 2 * max(fl["bf16_ref_err"]["text_embeds"], fg["bf16_ref_err"]["text_embeds"])
