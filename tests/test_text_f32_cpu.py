"""CPU leg of the text encoders' fp32 accuracy path: the fp32 attention checker (tests/text_attn_f32_check.py) admits a correct
fp32 kernel, catches the four faults tests/text_attn_check.py is shown AND an emulation of the bf16 kernel's arithmetic (the bound
separates fp32 from bf16); the C ABI mirror of the four `_f32` entries; their argument refusals; the models' refusals off the
device."""
import ctypes
import os
import re

import pytest
import torch

from tests import text_attn_f32_check as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = (("dwm_text_attention_f32", 2, "dwm_text_attention"), ("dwm_rmsnorm_rows_f32", 9, "dwm_rmsnorm_rows"),
           ("dwm_text_embed_f32", 10, "dwm_text_embed"), ("dwm_text_act_f32", 9, "dwm_text_act"))


@pytest.mark.parametrize("mode", F.MODES)
def test_fp32_attention_checker_admits_fp32_and_catches_faults_and_bf16(mode):
    L, H, n_seq, scale, causal = 77, 2, 2, 0.125, "causal" in mode
    q, k, v, bias = F.make_inputs(n_seq, L, H, mode, scale, 5, "cpu")
    W = F.Weights(q, k, bias, n_seq, L, H, scale, causal)
    o, bound = F.o_reference(W, v, n_seq, H)
    good = F.emulate(q, k, v, bias, n_seq, L, H, scale, causal)
    r = F.worst(F.element_ratios(good, o, bound, n_seq, L, H))[0]
    print(f"{mode}: correct fp32 emulation, worst element ratio {r:.3f}, frobenius {F.frobenius(good, o, n_seq, L, H):.2e}")
    assert r <= 0.7
    for c in range(2):
        got = F.emulate(q, k, F.v_onehot(n_seq, L, H, c, "cpu"), bias, n_seq, L, H, scale, causal)
        assert F.worst(F.census_ratios(got, W, c, n_seq, H))[0] <= 0.8
    faults = ["no_scale", "bf16_operands"] + (["one_key_more", "addend"] if causal else []) + (["bias_transposed"] if bias is not None else [])
    for fault in faults:
        bad = F.emulate(q, k, v, bias, n_seq, L, H, scale, causal, fault=fault)
        r = F.worst(F.element_ratios(bad, o, bound, n_seq, L, H))[0]
        print(f"{mode}: {fault} worst element ratio {r:.1f}")
        assert r > 10, fault
    # the census sees the bf16 rounding of P alone, and a hidden key with a nonzero weight is an infinite ratio
    got = F.emulate(q, k, F.v_onehot(n_seq, L, H, 0, "cpu"), bias, n_seq, L, H, scale, causal, fault="bf16_operands")
    assert F.worst(F.census_ratios(got, W, 0, n_seq, H))[0] > 10
    if causal:
        got = F.emulate(q, k, F.v_onehot(n_seq, L, H, 0, "cpu"), bias, n_seq, L, H, scale, causal, fault="addend")
        assert F.worst(F.census_ratios(got, W, 0, n_seq, H))[0] == float("inf")


def test_header_ctypes_and_wrappers_agree_on_the_fp32_entries():
    from opendwm_amd import _lib, ops
    import inspect
    hdr = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
    assert _lib.ABI_VERSION == 18 and re.search(r"#define DWM_ABI_VERSION 18\b", hdr)          # additions only
    assert "bf16 path only" not in hdr
    src = open(os.path.join(ROOT, "opendwm_amd", "csrc", "text.hip")).read()
    for name, arity, twin in ENTRIES:
        m = re.search(rf"^int {name}\(([^;]*)\);", hdr, flags=re.M)
        assert m and len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
        assert len(_lib.SIGNATURES[name][1]) == len(_lib.SIGNATURES[twin][1]) and _lib.SIGNATURES[name][0] is _lib.SIGNATURES[twin][0]
        assert re.search(rf'extern "C" int {name}\(', src), name
    for fn, name in ((ops.text_attention, "dwm_text_attention_f32"), (ops.rmsnorm_rows, "dwm_rmsnorm_rows_f32"),
                     (ops.text_embed, "dwm_text_embed_f32"), (ops.text_act, "dwm_text_act_f32")):
        assert f'"{name}"' in inspect.getsource(fn), name


def test_fp32_entry_points_refuse_bad_arguments_before_touching_the_device():
    from opendwm_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    fake = 1 << 20
    for name, _, _ in ENTRIES:
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]

    def attn(**kw):
        a = _lib.TextAttnArgs()
        a.q = a.k = a.v = a.out = fake
        a.ld, a.ldo, a.n_seq, a.L, a.heads, a.scale, a.causal = 192, 64, 2, 77, 1, 1.0, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.dwm_text_attention_f32(ctypes.byref(a), None)

    assert attn(L=0) == -3 and attn(L=129) == -3 and attn(L=129, q=None) == -1
    assert attn(ld=63) == -1 and attn(ld=194) == -2 and attn(q=fake + 4) == -2 and attn(causal=2) == -1 and attn(n_seq=0) == -1
    assert attn(heads=0) == -1 and attn(bias=fake + 2) == -2 and attn(ldo=60) == -1
    assert lib.dwm_rmsnorm_rows_f32(fake, 64, 1, 60, fake, 1e-6, fake, 64, None) == -3
    assert lib.dwm_rmsnorm_rows_f32(fake, 8200, 1, 8200, fake, 1e-6, fake, 8200, None) == -3
    assert lib.dwm_rmsnorm_rows_f32(fake, 32, 1, 64, fake, 1e-6, fake, 64, None) == -1
    assert lib.dwm_rmsnorm_rows_f32(fake, 64, 1, 64, fake, 1e-6, fake, 66, None) == -2
    assert lib.dwm_text_embed_f32(fake, 4, fake, 0, 64, None, 0, fake, 64, None) == -1
    assert lib.dwm_text_embed_f32(fake, 4, fake, 10, 60, None, 0, fake, 64, None) == -3
    assert lib.dwm_text_embed_f32(fake, 4, fake + 4, 10, 64, None, 0, fake, 64, None) == -2
    assert lib.dwm_text_act_f32(fake, 64, 1, 64, 3, 0, fake, 64, None) == -1
    assert lib.dwm_text_act_f32(fake, 64, 1, 64, 0, 1, fake, 64, None) == -1             # gated needs 2 F columns
    assert lib.dwm_text_act_f32(fake, 66, 1, 64, 0, 0, fake, 64, None) == -2


def test_wrapper_refusals_come_before_the_dtype_dispatch():
    from opendwm_amd import ops
    x = torch.zeros(77, 64)
    for L in (0, 129):
        with pytest.raises(NotImplementedError):
            ops.text_attention(x, x, x, x, 1, L, 1, 1.0)
    with pytest.raises(NotImplementedError):
        ops.text_attention(x, x, x, x, 1, 77, 2, 1.0)                                # head width 32
    with pytest.raises(NotImplementedError):
        ops.text_act(x, "relu")
    with pytest.raises(RuntimeError):
        ops.text_attention(x, x, x, x, 1, 77, 1, 1.0)                                # fp32, but not on the device
    with pytest.raises(RuntimeError):
        ops.gemm(torch.zeros(8, 64, dtype=torch.bfloat16), torch.zeros(8, 64, dtype=torch.bfloat16), w_planes=torch.zeros(8, 192))


def test_models_off_the_device_raise_in_every_dtype():
    from opendwm_amd import text_encoders as E
    ids = torch.zeros(2, 7, dtype=torch.int64)
    clip = E.CLIPTextModel(hidden_size=64, num_attention_heads=1, intermediate_size=128, num_hidden_layers=1, vocab_size=50)
    t5 = E.T5EncoderModel(dict(d_model=64, num_heads=1, d_ff=128, num_layers=1, vocab_size=50, feed_forward_proj="gated-gelu"))
    for m in (clip, t5):
        for dt in (torch.float32, torch.bfloat16, torch.float16, torch.float64):
            assert m.to(dt).dtype == dt and m.device.type == "cpu"
            with pytest.raises(RuntimeError):
                m(ids)
    q = E.CLIPTextModel(dict(hidden_size=64, num_attention_heads=1, intermediate_size=128, num_hidden_layers=1, vocab_size=50),
                        quantization_config=dict(load_in_4bit=True, bnb_4bit_quant_type="nf4"))
    with pytest.raises(RuntimeError):
        q(ids)                                                   # on the CPU the device refusal comes first, quantised or not
