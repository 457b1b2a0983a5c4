"""GPU leg of the text encoders' fp32 accuracy path (opendwm_amd/text_encoders.py, `model.to(device).to(torch.float32)`): the three
small models against the fp32 outputs of the transformers classes (tests/golden/text_encoders_{t5,clip}.pt), each tensor within
TOL_F32 = 1e-3 relative Frobenius error - the fp32 tolerance of tests/test_fp32_gpu.py; the dedupe guarantee and the SD 3 assembly
in fp32; the mode switch on one object; and the claim the path exists for: a small fp32 MMDiT conditioned by the fp32 HIP encoders
FROM TOKEN IDS stays within TOL_F32 of the oracle forward conditioned by the fp32 restatement's embeddings.

Measured on an MI355X (printed by each test): see DESIGN.md §23."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import text_ref as R          # noqa: E402

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
GOLDEN = os.path.join(ROOT, "tests", "golden")
bf16, f32 = torch.bfloat16, torch.float32
TOL_F32 = 1e-3                             # tests/test_fp32_gpu.py
PICK = [0, 1, 0, 2, 1, 0, 0, 2]            # the flat prompt list with repeats of tests/test_text_encoders_gpu.py


def rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _load(cls, cfg, sd, dev, dtype):
    m = cls(cfg)
    m.load_state_dict(sd)
    return m.to(dev).to(dtype).requires_grad_(False)


@pytest.fixture(scope="module")
def models(dev):
    """fixtures, state dicts and the fp32 models (T5, CLIP "l" and "g" with projection, the plain CLIPTextModel of "g"), loaded once"""
    from opendwm_amd import text_encoders as E
    t5fx = torch.load(os.path.join(GOLDEN, "text_encoders_t5.pt"))
    clipfx = torch.load(os.path.join(GOLDEN, "text_encoders_clip.pt"))
    sds = dict(t5=R.make_t5_state_dict(t5fx["config"], t5fx["seed"]))
    out = dict(t5fx=t5fx, clipfx=clipfx, sds=sds, t5=_load(E.T5EncoderModel, t5fx["config"], sds["t5"], dev, f32))
    for name, fx in clipfx.items():
        sds[name] = R.make_clip_state_dict(fx["config"], fx["seed"])
        assert R.state_dict_digest(sds[name]) == fx["digest"]
        out[name] = _load(E.CLIPTextModelWithProjection, fx["config"], sds[name], dev, f32)
    sds["plain"] = {k: v for k, v in sds["g"].items() if k != "text_projection.weight"}
    out["plain"] = _load(E.CLIPTextModel, clipfx["g"]["config"], sds["plain"], dev, f32)
    return out


def _check(name, got, fx, key):
    e = rel(got, fx[key])
    print(f"{name} fp32 {key}: rel err {e:.3e}  bound {TOL_F32:.0e}")
    assert got.dtype == f32 and e < TOL_F32, (name, key, e)
    return e


def _reads_back(m, sd):
    have = m.state_dict()
    return set(have) <= set(sd) and all(v.dtype == f32 and torch.equal(v.cpu(), sd[k].float()) for k, v in have.items())


def _mode_switch(name, m, cls, cfg, sd, ids, fx, keys, e32, dev):
    """fp32 -> bf16 on the same object: bit-equal to a freshly loaded bf16 model, and visibly less accurate than the fp32 run"""
    fresh = _load(cls, cfg, sd, dev, bf16)(ids, output_hidden_states=True)
    same = m.to(bf16)(ids, output_hidden_states=True)
    try:
        for key, field in keys:
            a, b = field(same), field(fresh)
            assert a.dtype == bf16 and torch.equal(a, b), (name, key)
            e16 = rel(a, fx[key])
            print(f"{name} bf16 on the same object {key}: rel err {e16:.3e} (fp32 {e32[key]:.3e})")
            assert e16 > 10 * e32[key], (name, key, e16, e32[key])
    finally:
        m.to(f32)
    again = m(ids, output_hidden_states=True)                                # and back: the fp32 result again, bit for bit
    return again


LAST = ("last_hidden_state", lambda o: o.last_hidden_state)
PEN = ("penultimate", lambda o: o.hidden_states[-2])
EMB = ("text_embeds", lambda o: o.text_embeds)
POOL = ("pooler_output", lambda o: o.pooler_output)


def test_t5_fp32_against_the_transformers_fixture(models, dev):
    from opendwm_amd import text_encoders as E
    fx, m = models["t5fx"], models["t5"]
    assert m.dtype == f32 and m.device.type == "cuda"
    o = m(fx["ids"], output_hidden_states=True)
    assert len(o.hidden_states) == fx["n_hidden_states"] and o[0] is o.last_hidden_state
    assert all(h.dtype == f32 for h in o.hidden_states)
    e32 = {key: _check("t5", field(o), fx, key) for key, field in (LAST, PEN)}
    again = m(fx["ids"].to(dev))                                              # two runs are bit-equal; ids already on the device
    assert again.hidden_states is None and torch.equal(again[0], o[0])
    assert _reads_back(m, models["sds"]["t5"])
    back = _mode_switch("t5", m, E.T5EncoderModel, fx["config"], models["sds"]["t5"], fx["ids"], fx, (LAST, PEN), e32, dev)
    assert m.dtype == f32 and torch.equal(back[0], o[0]) and _reads_back(m, models["sds"]["t5"])


@pytest.mark.parametrize("name", ["l", "g"])
def test_clip_fp32_against_the_transformers_fixture(models, dev, name):
    from opendwm_amd import text_encoders as E
    fx, m = models["clipfx"][name], models[name]
    o = m(fx["ids"], output_hidden_states=True)
    assert len(o.hidden_states) == fx["n_hidden_states"] and o[0] is o.text_embeds
    e32 = {key: _check(name, field(o), fx, key) for key, field in (LAST, PEN, EMB, POOL)}
    again = m(fx["ids"].to(m.device))                                         # ids already on the device
    assert again.hidden_states is None and torch.equal(again[0], o[0]) and torch.equal(again.last_hidden_state, o.last_hidden_state)
    assert _reads_back(m, models["sds"][name])
    back = _mode_switch(name, m, E.CLIPTextModelWithProjection, fx["config"], models["sds"][name], fx["ids"], fx,
                        (LAST, PEN, EMB, POOL), e32, dev)
    assert torch.equal(back[0], o[0]) and torch.equal(back.last_hidden_state, o.last_hidden_state)


def test_clip_text_model_without_projection_fp32(models):
    fx, m = models["clipfx"]["g"], models["plain"]
    o = m(fx["ids"])
    assert o[0] is o.last_hidden_state and o[1] is o.pooler_output and o.text_embeds is None
    _check("plain", o.last_hidden_state, fx, "last_hidden_state")
    _check("plain", o.pooler_output, fx, "pooler_output")
    assert torch.equal(m(fx["ids"])[0], o[0]) and _reads_back(m, models["sds"]["plain"])
    from opendwm_amd import conditions
    e = conditions.encode_clip_text(m, fx["ids"], [3], 2, 4)
    assert e.dtype == f32 and e.shape == (3, 2, 4, 77, 192) and torch.equal(e[:, 1, 3], o[0])


def test_operand_planes_live_and_die_with_the_packed_entry(models):
    """the planes of split_weight are the model's: none in the process-wide cache, gone with `_packed`"""
    from opendwm_amd import ops
    m, fx = models["l"], models["clipfx"]["l"]
    ops.clear_split_weights()
    m(fx["ids"])
    assert len(ops._SPLIT_WEIGHTS) == 0 and m._packed is not None
    weights = sum(p.numel() * 4 for p in m.parameters())
    gemm = sum(mod.weight.numel() for mod in m.modules() if isinstance(mod, torch.nn.Linear))
    assert m.held_bytes() == weights + 6 * gemm                  # [hi | lo | hi] in bf16: 6 bytes of planes per GEMM weight
    m.to(f32)                                                    # any .to() releases the packed operands and their planes
    assert m._packed is None and m.held_bytes() == weights


def test_quantisation_with_fp32_is_refused(models, dev):
    from opendwm_amd import text_encoders as E
    fx = models["clipfx"]["l"]
    for route in E.NF4_ROUTES:
        q = E.CLIPTextModelWithProjection(fx["config"], quantization_config=dict(load_in_4bit=True, bnb_4bit_quant_type="nf4", route=route))
        q.load_state_dict(models["sds"]["l"])
        with pytest.raises(NotImplementedError, match=r"(?s)quantization_config.*float32"):
            q.to(dev).to(f32)(fx["ids"])
    t5fx = models["t5fx"]
    q = E.T5EncoderModel(t5fx["config"], quantization_config=dict(load_in_4bit=True, bnb_4bit_quant_type="nf4"))
    q.load_state_dict(models["sds"]["t5"])
    with pytest.raises(NotImplementedError, match=r"(?s)quantization_config.*float32"):
        q.to(dev).to(f32)(t5fx["ids"])
    half = _load(E.CLIPTextModelWithProjection, fx["config"], models["sds"]["l"], dev, torch.float16)
    with pytest.raises(RuntimeError):
        half(fx["ids"])                                          # bf16 and fp32 are the two dtypes there are


def _sd3_ids(models):
    pick = torch.tensor(PICK)
    return pick, [models["clipfx"]["l"]["ids"][pick], models["clipfx"]["g"]["ids"][pick], models["t5fx"]["ids"][pick]]


def test_sd3_triple_dedupe_bit_equal_and_assembly_fp32(models):
    from opendwm_amd import conditions
    from opendwm_amd.text_encoders import SD3TextEncoders
    enc = SD3TextEncoders(models["l"], models["g"], models["t5"])
    pick, ids = _sd3_ids(models)
    h, p, t5 = enc.encode(*ids, dedupe=True)
    h2, p2, t52 = enc.encode(*ids, dedupe=False)
    for a, b in zip(h + p + [t5], h2 + p2 + [t52]):
        assert a.dtype == f32 and a.shape[0] == 8 and torch.equal(a, b)      # rows are independent: bit-equal
    text, pooled = conditions.encode_sd3_text(enc, *ids, [2, 2, 2], 2, 2, f32)
    assert text.dtype == f32 and text.shape == (2, 2, 2, 154, 128) and pooled.shape == (2, 2, 2, 192)
    fl, fg, ft = models["clipfx"]["l"], models["clipfx"]["g"], models["t5fx"]
    want_text, want_pooled = conditions.assemble_sd3_text(
        [fl["penultimate"][pick], fg["penultimate"][pick]], [fl["text_embeds"][pick], fg["text_embeds"][pick]],
        ft["last_hidden_state"][pick], [2, 2, 2], 2, 2, f32)
    assert want_text.shape == text.shape and want_pooled.shape == pooled.shape
    e = (rel(text[..., :77, :], want_text[..., :77, :]), rel(text[..., 77:, :], want_text[..., 77:, :]), rel(pooled, want_pooled))
    print(f"sd3 assembly fp32: clip rows {e[0]:.3e}  t5 rows {e[1]:.3e}  pooled {e[2]:.3e}  bound {TOL_F32:.0e}")
    assert max(e) < TOL_F32, e
    # without a T5 encoder the zeros that stand in for it follow the CLIP dtype
    _, _, z = SD3TextEncoders(models["l"], models["g"], None).encode(ids[0], ids[1], None, joint_attention_dim=128)
    assert z.dtype == f32 and z.shape == (8, 77, 128) and not bool(z.any())


def test_fp32_mmdit_conditioned_from_token_ids_vs_oracle(models, dev):
    """END TO END: token ids -> fp32 HIP encoders -> SD 3 assembly -> fp32 MMDiT forward (the small full-graph configuration of
    tests/test_fp32_gpu.py, pooled width 192 = the two toy CLIP projections) against the CPU oracle forward conditioned by the fp32
    restatement (tests/text_ref.py) of the same encoders.  The same run with the bf16 encoders feeding the fp32 model is printed,
    not asserted: what the conditioning error of the bf16 encoders does to the model output."""
    from oracle import ctsd_oracle as O
    from opendwm_amd import conditions
    from opendwm_amd import text_encoders as E
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.text_encoders import SD3TextEncoders
    from tests.common import rel_err, small_config, small_inputs, to_dev
    pick, ids = _sd3_ids(models)
    fl, fg, ft = models["clipfx"]["l"], models["clipfx"]["g"], models["t5fx"]
    refs = [R.clip({k: v.float() for k, v in models["sds"]["l"].items()}, fl["config"], fl["ids"]),
            R.clip({k: v.float() for k, v in models["sds"]["g"].items()}, fg["config"], fg["ids"]),
            R.t5({k: v.float() for k, v in models["sds"]["t5"].items()}, ft["config"], ft["ids"])]
    ref_text, ref_pooled = conditions.assemble_sd3_text(
        [refs[0]["penultimate"][pick], refs[1]["penultimate"][pick]], [refs[0]["text_embeds"][pick], refs[1]["text_embeds"][pick]],
        refs[2]["last_hidden_state"][pick], [2, 2, 2], 2, 2, f32)
    cfg = small_config(pooled_projection_dim=192)
    assert cfg["joint_attention_dim"] == ref_text.shape[-1]
    sd = O.make_state_dict(cfg, 0)
    inp = small_inputs(cfg, 0, T=2, V=2, text_len=154)
    assert inp["encoder_hidden_states"].shape == ref_text.shape and inp["pooled_projections"].shape == ref_pooled.shape
    ref = O.dit_forward(sd, cfg, **dict(inp, encoder_hidden_states=ref_text, pooled_projections=ref_pooled))
    m = DiTCrossviewTemporalConditionModel(**cfg)
    m.load_state_dict(sd)
    m = m.to(dev).eval()
    m.compute_dtype = f32

    def run(text, pooled):
        di = to_dev(dict(inp, encoder_hidden_states=text, pooled_projections=pooled), dev)
        out, _, _ = m(di.pop("sample"), di.pop("timestep"), **di)
        assert out[0].dtype == f32
        return rel_err(out[0], ref)

    enc32 = SD3TextEncoders(models["l"], models["g"], models["t5"])
    text, pooled = conditions.encode_sd3_text(enc32, *ids, [2, 2, 2], 2, 2, f32)
    assert text.dtype == f32
    e_cond = (rel(text, ref_text), rel(pooled, ref_pooled))
    e32 = run(text, pooled)
    e_oracle_text = run(ref_text.to(dev), ref_pooled.to(dev))               # the model's own error, conditioning exact
    enc16 = SD3TextEncoders(_load(E.CLIPTextModelWithProjection, fl["config"], models["sds"]["l"], dev, bf16),
                            _load(E.CLIPTextModelWithProjection, fg["config"], models["sds"]["g"], dev, bf16),
                            _load(E.T5EncoderModel, ft["config"], models["sds"]["t5"], dev, bf16))
    text16, pooled16 = conditions.encode_sd3_text(enc16, *ids, [2, 2, 2], 2, 2, f32)
    e_cond16 = (rel(text16, ref_text), rel(pooled16, ref_pooled))
    e16 = run(text16, pooled16)
    print(f"fp32 MMDiT from token ids: fp32 encoders rel {e32:.3e} (conditioning text {e_cond[0]:.3e} pooled {e_cond[1]:.3e}); "
          f"reference conditioning rel {e_oracle_text:.3e}; bf16 encoders rel {e16:.3e} (conditioning text {e_cond16[0]:.3e} "
          f"pooled {e_cond16[1]:.3e}); bound {TOL_F32:.0e}")
    assert e32 < TOL_F32, e32
