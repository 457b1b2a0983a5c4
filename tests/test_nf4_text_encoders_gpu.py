"""GPU leg of the 4-bit text encoders (`quantization_config` of opendwm_amd/text_encoders.py) on the small fixture models of
tests/golden/text_encoders_*.pt, weights from tests/text_ref.make_*_state_dict.

  * route "dequant" is BIT-EQUAL to the existing bf16 model loaded with W' (tests/nf4_ref.py): same GEMM, same operands - the exact
    check of the format end to end;
  * route "fused" against tests/text_ref run in fp32 on W': relative Frobenius error <= 2 x bf16_ref_err of the fixture, the bound
    of tests/test_text_encoders_gpu.py.  On the CPU the plain bf16 text_ref run on W' measures 1.0 - 1.07 x
    bf16_ref_err on every tensor, so the reference alone is inside the bound;
  * both routes are at least 4 x that bound away from the UNQUANTISED fixture outputs: quantisation is in effect;
  * dedupe stays bit-equal, the bytes held are exactly those of the format, `.to()` / `load_state_dict` return to pending.

Measured on an MI355X (printed by the tests): see DESIGN.md §24."""
import os

import pytest
import torch

from tests import nf4_ref as Q
from tests import text_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
bf16 = torch.bfloat16
ROUTES = ("fused", "dequant")
NAMES = ("t5", "l", "g")


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


def config(route):
    return dict(load_in_4bit=True, bnb_4bit_quant_type="nf4", bnb_4bit_compute_dtype="bfloat16", route=route)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def world(dev):
    """per model name: fixture, checkpoint state dict, its W' twin, the fp32 reference on W', the bf16 model on W' and the two
    quantised models - everything built and (the references) computed once"""
    from opendwm_amd import text_encoders as E
    t5fx = torch.load(os.path.join(GOLDEN, "text_encoders_t5.pt"))
    clipfx = torch.load(os.path.join(GOLDEN, "text_encoders_clip.pt"))
    out = {}
    for name in NAMES:
        fx = t5fx if name == "t5" else clipfx[name]
        cls = E.T5EncoderModel if name == "t5" else E.CLIPTextModelWithProjection
        sd = (R.make_t5_state_dict if name == "t5" else R.make_clip_state_dict)(fx["config"], fx["seed"])
        assert R.state_dict_digest(sd) == fx["digest"]
        models = {}
        for route in ROUTES:
            m = cls(fx["config"], quantization_config=config(route))
            m.load_state_dict(sd)
            models[route] = m.to(dev).to(bf16).requires_grad_(False)
        sd_w = Q.requantized_state_dict(sd, models["fused"].quantised_modules())
        plain = cls(fx["config"])
        plain.load_state_dict(sd_w)
        ref = (R.t5 if name == "t5" else R.clip)({k: v.float() for k, v in sd_w.items()}, fx["config"], fx["ids"])
        out[name] = dict(fx=fx, sd=sd, sd_w=sd_w, ref=ref, plain=plain.to(dev).to(bf16).requires_grad_(False), **models)
    return out


def fields(o):
    """every output field of a forward(output_hidden_states=True), flat"""
    named = [(k, getattr(o, k)) for k in ("last_hidden_state", "pooler_output", "text_embeds") if getattr(o, k) is not None]
    return named + [(f"hidden_states[{i}]", h) for i, h in enumerate(o.hidden_states)]


@pytest.mark.parametrize("name", NAMES)
def test_dequant_route_is_bit_equal_to_the_bf16_model_on_the_dequantised_weights(world, name):
    w = world[name]
    got = fields(w["dequant"](w["fx"]["ids"], output_hidden_states=True))
    want = fields(w["plain"](w["fx"]["ids"], output_hidden_states=True))
    assert [k for k, _ in got] == [k for k, _ in want] and len(got) >= w["fx"]["n_hidden_states"] + 1
    for (k, a), (_, b) in zip(got, want):
        assert a.dtype == bf16 and torch.equal(a, b), (name, k)


@pytest.mark.parametrize("name", NAMES)
def test_fused_route_against_the_fp32_reference_on_the_dequantised_weights(world, name):
    w = world[name]
    o = w["fused"](w["fx"]["ids"], output_hidden_states=True)
    for key, base in w["fx"]["bf16_ref_err"].items():
        got = o.hidden_states[-2] if key == "penultimate" else getattr(o, key)
        e, bound = rel(got, w["ref"][key]), 2 * base
        print(f"nf4 fused {name} {key}: rel err {e:.3e}  bound {bound:.3e} (bf16_ref_err {base:.3e})")
        assert e <= bound, (name, key, e, bound)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_quantisation_is_in_effect(world, name, route):
    w = world[name]
    o = w[route](w["fx"]["ids"], output_hidden_states=True)
    for key, base in w["fx"]["bf16_ref_err"].items():
        got = o.hidden_states[-2] if key == "penultimate" else getattr(o, key)
        away, floor = rel(got, w["fx"][key]), 4 * 2 * base
        print(f"nf4 {route} {name} {key}: {away:.3e} from the unquantised fixture (floor {floor:.3e})")
        assert away >= floor, (name, route, key, away, floor)


@pytest.mark.parametrize("route", ROUTES)
def test_dedupe_is_bit_equal_with_all_three_models_quantised(world, route):
    from opendwm_amd.text_encoders import SD3TextEncoders
    enc = SD3TextEncoders(world["l"][route], world["g"][route], world["t5"][route])
    pick = torch.tensor([0, 1, 0, 2, 1, 0, 0, 2])
    ids = [world[n]["fx"]["ids"][pick] for n in ("l", "g", "t5")]
    h, p, t5 = enc.encode(*ids, dedupe=True)
    h2, p2, t52 = enc.encode(*ids, dedupe=False)
    for a, b in zip(h + p + [t5], h2 + p2 + [t52]):
        assert a.shape[0] == 8 and torch.equal(a, b)


def held_bytes(m):
    return sum(t.numel() * t.element_size() for t in list(m.parameters()) + list(m.buffers()))


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", NAMES)
def test_bytes_held_are_those_of_the_format(world, name, route):
    w, m = world[name], world[name][route]
    m(w["fx"]["ids"])
    quantised = m.quantised_modules()
    skipped = ("wo",) if name == "t5" else ("text_projection",)
    distinct = {v.data_ptr(): v for v in w["sd"].values()}                        # T5's tied table appears under two names
    want = sum(2 * v.numel() for v in distinct.values())
    for n in quantised:
        N, K = w["sd"][n + ".weight"].shape
        want += N * K // 2 + N * K // 16 - 2 * N * K
        mod = m.get_submodule(n)
        assert mod.weight is None
        assert mod.weight_nf4.dtype == torch.uint8 and tuple(mod.weight_nf4.shape) == (N, K // 2)
        assert mod.weight_absmax.dtype == torch.float32 and tuple(mod.weight_absmax.shape) == (N, K // 64)
    assert quantised and held_bytes(m) == want, (held_bytes(m), want)
    assert held_bytes(w["plain"]) == sum(2 * v.numel() for v in distinct.values())
    keys = set(m.state_dict())
    for n, mod in m.named_modules():
        if isinstance(mod, torch.nn.Linear):
            if n in quantised:
                assert n + ".weight" not in keys and {n + ".weight_nf4", n + ".weight_absmax"} <= keys
            else:
                assert n.endswith(skipped) and mod.weight.dtype == bf16 and n + ".weight" in keys


@pytest.mark.parametrize("name", NAMES)
def test_to_and_load_state_dict_return_to_pending(world, name, dev):
    w, m = world[name], world[name]["fused"]
    ids = w["fx"]["ids"]
    first = fields(m(ids, output_hidden_states=True))
    packed = m.state_dict()
    assert any(k.endswith(".weight_nf4") for k in packed)
    with pytest.raises(RuntimeError, match="weight_nf4"):
        m.load_state_dict(packed)

    def pending():
        return all(m.get_submodule(n).weight is not None and m.get_submodule(n).weight.dtype == bf16 for n in m.quantised_modules()) \
            and not any(k.endswith((".weight_nf4", ".weight_absmax")) for k in m.state_dict())

    assert not pending()
    m.to(dev)
    assert pending()
    for n in m.quantised_modules():                                               # .to() left W' behind: the same codes come back
        assert torch.equal(m.get_submodule(n).weight.cpu(), w["sd_w"][n + ".weight"]), n
    for (k, a), (_, b) in zip(fields(m(ids, output_hidden_states=True)), first):
        assert torch.equal(a, b), (name, ".to()", k)
    assert not pending()
    m.load_state_dict(w["sd"])
    assert pending()
    for (k, a), (_, b) in zip(fields(m(ids, output_hidden_states=True)), first):
        assert torch.equal(a, b), (name, "load_state_dict", k)
    assert not pending()
