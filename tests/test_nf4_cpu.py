"""CPU leg of the NF4 4-bit weights (opendwm_amd/nf4.py, csrc/gemm_nf4.hip, the `quantization_config` of the text encoders): the
properties of the format on the plain restatement tests/nf4_ref.py, the proof that the element bound of tests/gemm_check.py BITES
on the faults a fused dequantising GEMM can have, the C surface and the constructors' configuration handling."""
import ctypes
import os
import re

import pytest
import torch

from tests import gemm_check as G
from tests import nf4_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf16 = torch.bfloat16
NF4 = dict(load_in_4bit=True, bnb_4bit_quant_type="nf4")


def gaussian(n, k, std, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, k, generator=g) * std).to(bf16)


# ----------------------------------------------------------------------------------------------------- table and round trip
def test_table_is_the_nf4_data_type():
    from opendwm_amd import nf4
    lit = [-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635, -0.18477343022823334,
           -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
           0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0]
    assert R.CODE.dtype == torch.float32 and R.CODE.tolist() == torch.tensor(lit, dtype=torch.float32).tolist()
    assert bool((R.CODE[1:] > R.CODE[:-1]).all())                                     # sorted and distinct
    assert nf4.CODE.dtype == torch.float32 and torch.equal(nf4.CODE, R.CODE)
    assert nf4.BLOCK == R.BLOCK == 64 and float(nf4.CODE[nf4.ZERO_CODE]) == 0.0
    assert nf4.packed_bytes(24, 192) == 24 * 192 // 2 + 24 * 192 // 16


@pytest.mark.parametrize("std", [1e-3, 0.02, 1.0, 37.0])
def test_round_trip_is_idempotent(std):
    w = gaussian(96, 512, std, 3)
    q, absmax = R.quantize(w)
    assert q.dtype == torch.uint8 and q.shape == (96, 256) and absmax.shape == (96, 8)
    assert torch.equal(R.unpack(q), R.codes(w)[0]) and torch.equal(R.pack(R.unpack(q)), q)
    q2, absmax2 = R.quantize(R.dequantize(q, absmax))
    assert torch.equal(q2, q) and torch.equal(absmax2, absmax)


def test_zero_block_and_one_signed_block():
    w = gaussian(4, 192, 1.0, 5)
    w[1, 64:128] = 0
    w[2, 0:64] = -w[2, 0:64].abs() - 0.01                                             # every element negative: the extreme is code 0
    c, absmax = R.codes(w)
    assert bool((c[1, 64:128] == 7).all()) and float(absmax[1, 1]) == 0
    d = R.dequantize(*R.quantize(w))
    assert bool((d[1, 64:128] == 0).all())
    assert int(c[2, 0:64].min()) == 0 and int(c[2, 0:64].max()) <= 7
    at = int(w[2, 0:64].float().argmin())
    assert int(c[2, at]) == 0 and float(d[2, at]) == float(w[2, at])                  # the extreme itself is exact
    assert int(c.max()) == 15 and float(d.float().abs().max()) == float(w.float().abs().max())


@pytest.mark.parametrize("shape", [(512, 1024), (192, 256)])
def test_relative_error_is_the_tables(shape):
    """a property of the table (measured: 0.0919 - 0.0921); it catches a wrong table, it bounds no kernel"""
    w = gaussian(*shape, 0.02, 11)
    d = R.dequantize(*R.quantize(w))
    e = float((d.double() - w.double()).norm() / w.double().norm())
    print(f"{shape}: relative Frobenius error {e:.4f}")
    assert 0.085 <= e <= 0.10


# --------------------------------------------------------------------------------------------------------- the checker bites
def stepped_weight(n, k, seed):
    """Gaussian weight whose neighbouring blocks and neighbouring rows differ 100 times in scale"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g)
    scale = torch.tensor([1.0, 100.0])[(torch.arange(n)[:, None] + torch.arange(k // 64)[None, :]) % 2]
    return (w.view(n, k // 64, 64) * scale[:, :, None] * 0.02).view(n, k).to(bf16)


def emulate(a, q, absmax, code=R.CODE, fault=None):
    """a torch emulation of the fused kernel: W' in bf16, fp32 accumulation; `fault`: one way of getting it wrong"""
    c = R.unpack(q)
    if fault == "nibbles":
        c = c.view(c.shape[0], -1, 2).flip(-1).reshape(c.shape)
    if fault == "next_block":
        absmax = absmax.roll(-1, 1)
    if fault == "next_row":
        absmax = absmax.roll(-1, 0)
    if fault == "table":
        code = code.clone()
        code[9] = code[10]
    N, K = c.shape
    if fault == "scale_acc":             # unscaled bf16 code values into the product, the block's partial sum scaled afterwards
        v = code[c].to(bf16).float().view(N, K // 64, 64)
        part = torch.einsum("mbk,nbk->mnb", a.float().view(a.shape[0], K // 64, 64), v)
        return (part * absmax[None]).sum(-1)
    return a.float() @ R.dequantize(R.pack(c), absmax, code).float().T


@pytest.fixture(scope="module")
def bite():
    M, N, K = 48, 64, 256
    g = torch.Generator().manual_seed(17)
    a = torch.randn(M, K, generator=g).to(bf16)
    q, absmax = R.quantize(stepped_weight(N, K, 19))
    ref, mag = G.product(a, R.dequantize(q, absmax))
    return a, q, absmax, ref, mag, K


def test_checker_admits_a_correct_kernel(bite):
    a, q, absmax, ref, mag, K = bite
    acc = emulate(a, q, absmax)
    r16, r32 = G.element_ratio(acc.to(bf16), ref, mag, K), G.element_ratio(acc, ref, mag, K)
    print(f"emulation: bf16 ratio {r16:.3f}, fp32 ratio {r32:.3f}")
    assert r16 < 1 and r32 < 1


@pytest.mark.parametrize("fault", ["nibbles", "next_block", "next_row", "table"])
def test_checker_catches_an_indexing_fault(bite, fault):
    a, q, absmax, ref, mag, K = bite
    acc = emulate(a, q, absmax, fault=fault)
    r16, r32 = G.element_ratio(acc.to(bf16), ref, mag, K), G.element_ratio(acc, ref, mag, K)
    print(f"{fault}: bf16 ratio {r16:.3g}, fp32 ratio {r32:.3g}")
    assert r16 > 1 and r32 > 1


def test_checker_catches_scaled_accumulators():
    """scaling the accumulators of unscaled codes rounds code[q] to bf16 where the format rounds code[q] * absmax: the two differ
    by up to 2^-9 per weight unless absmax is a power of two.  Where a row of A is orthogonal to a weight row the products cancel,
    |ref| is far below the sum of the absolute terms and the 2^-8 |ref| term of the bound has nothing to hide the difference in."""
    M, N, K = 48, 64, 256
    g = torch.Generator().manual_seed(23)
    q, absmax = R.quantize((torch.randn(N, K, generator=g) * 0.02).to(bf16))
    wd = R.dequantize(q, absmax).double()
    a = torch.randn(M, K, generator=g).double()
    a = a - (a @ wd[:M].T).diagonal()[:, None] * wd[:M] / wd[:M].pow(2).sum(1, keepdim=True)     # row i orthogonal to weight row i
    a = a.to(bf16)
    ref, mag = G.product(a, wd)
    assert float((ref.diagonal().abs() / mag.diagonal()).max()) < 2e-3                           # the cancellation is there
    good, bad = emulate(a, q, absmax), emulate(a, q, absmax, fault="scale_acc")
    assert G.element_ratio(good.to(bf16), ref, mag, K) < 1 and G.element_ratio(good, ref, mag, K) < 1
    r16, r32 = G.element_ratio(bad.to(bf16), ref, mag, K), G.element_ratio(bad, ref, mag, K)
    print(f"scale_acc: bf16 ratio {r16:.3g}, fp32 ratio {r32:.3g}")
    assert r16 > 1 and r32 > 1


# ---------------------------------------------------------------------------------------------------------------- surface
def test_header_binding_and_sources_agree():
    from opendwm_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
    assert re.search(rf"#define DWM_ABI_VERSION {_lib.ABI_VERSION}\b", hdr)                      # additions only: the version stays
    for name, arity in (("dwm_nf4_quantize", 8), ("dwm_nf4_dequantize", 8), ("dwm_gemm_nf4", 2)):
        m = re.search(rf"^int {name}\(([^;]*)\);", hdr, flags=re.M)
        assert m and len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
    body = hdr[hdr.index("typedef struct dwm_gemm_nf4_args"):hdr.index("} dwm_gemm_nf4_args;")]
    names = re.findall(r"[\s\*,]([A-Za-z_0-9]+)\s*[,;]", body)
    assert names == [f for f, _ in _lib.GemmNf4Args._fields_]
    kinds = dict(_lib.GemmNf4Args._fields_)
    assert all(kinds[k] is _lib._i64 for k in ("lda", "ldc", "ldc32", "M", "N", "K"))
    assert "gemm_nf4.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gemm_nf4.hip"))


def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    from opendwm_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name in ("dwm_nf4_quantize", "dwm_nf4_dequantize", "dwm_gemm_nf4"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = _lib.SIGNATURES[name]
    fake = 1 << 20

    def gemm(**kw):
        a = _lib.GemmNf4Args()
        a.A = a.q = a.absmax = a.code = a.C = fake
        a.lda, a.ldc, a.ldc32, a.M, a.N, a.K = 128, 64, 64, 77, 64, 128
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.dwm_gemm_nf4(ctypes.byref(a), None)

    assert gemm(K=96, lda=96) == -1 and gemm(K=0) == -1                                           # K % 64
    assert gemm(C32=fake) == -1 and gemm(C=None) == -1                                            # both outputs, neither
    assert gemm(code=None) == -1 and gemm(q=None) == -1 and gemm(absmax=None) == -1 and gemm(A=None) == -1
    assert gemm(M=0) == -1 and gemm(lda=64) == -1 and gemm(ldc=56) == -1
    assert gemm(N=60, ldc=64) == -3                                                               # N % 8
    assert gemm(A=fake + 2) == -2 and gemm(lda=132) == -2 and gemm(bias=fake + 8) == -2 and gemm(C=None, C32=fake + 4) == -2
    assert lib.dwm_nf4_quantize(fake, 96, 8, 96, fake, fake, fake, None) == -1
    assert lib.dwm_nf4_quantize(fake, 64, 8, 64, None, fake, fake, None) == -1
    assert lib.dwm_nf4_quantize(fake, 32, 8, 64, fake, fake, fake, None) == -1
    assert lib.dwm_nf4_quantize(fake, 68, 8, 64, fake, fake, fake, None) == -2
    assert lib.dwm_nf4_dequantize(fake, fake, 8, 96, fake, fake, 96, None) == -1
    assert lib.dwm_nf4_dequantize(fake, fake, 8, 64, None, fake, 64, None) == -1
    assert lib.dwm_nf4_dequantize(fake, fake, 0, 64, fake, fake, 64, None) == -1


def test_wrapper_argument_checks():
    from opendwm_amd import ops
    w = torch.zeros(8, 64, dtype=bf16)
    with pytest.raises(RuntimeError):
        ops.nf4_quantize(w)                                                                       # not on the device: no fallback
    with pytest.raises(RuntimeError):
        ops.nf4_dequantize(torch.zeros(8, 32, dtype=torch.uint8), torch.zeros(8, 1))
    with pytest.raises(RuntimeError):
        ops.gemm_nf4(w, torch.zeros(8, 32, dtype=torch.uint8), torch.zeros(8, 1))


# ------------------------------------------------------------------------------------------------------------ constructors
def test_constructors_refuse_what_is_not_built():
    from opendwm_amd import text_encoders as E
    t5 = dict(feed_forward_proj="gated-gelu", num_layers=1)
    for cls, cfg in ((E.T5EncoderModel, t5), (E.CLIPTextModel, dict(num_hidden_layers=1)),
                     (E.CLIPTextModelWithProjection, dict(num_hidden_layers=1))):
        for bad in (dict(load_in_4bit=True, bnb_4bit_quant_type="fp4"), dict(load_in_4bit=True),
                    dict(NF4, bnb_4bit_use_double_quant=True), dict(load_in_8bit=True)):
            with pytest.raises(NotImplementedError):
                cls(cfg, quantization_config=bad)
        with pytest.raises(ValueError):
            cls(cfg, quantization_config=dict(NF4, route="auto"))
        m = cls(cfg, quantization_config=dict(NF4, bnb_4bit_compute_dtype="float16"))           # accepted and ignored
        assert m.quantization["route"] == E.NF4_DEFAULT_ROUTE and E.NF4_DEFAULT_ROUTE in E.NF4_ROUTES
        assert cls(cfg, quantization_config=dict(NF4, route="dequant")).quantization["route"] == "dequant"
        assert cls(cfg).quantization is None and cls(cfg).quantised_modules() == []


def test_default_skip_lists_and_their_replacement():
    from opendwm_amd import text_encoders as E
    t5cfg = dict(feed_forward_proj="gated-gelu", num_layers=2)
    t5 = E.T5EncoderModel(t5cfg, quantization_config=NF4)
    assert t5.quantization["skip"] == ["wo"]
    names = t5.quantised_modules()
    linear = [n for n, m in t5.named_modules() if isinstance(m, torch.nn.Linear)]
    assert sorted(names) == sorted(n for n in linear if not n.endswith(".wo")) and len(names) == 12
    assert sorted(E.T5EncoderModel(t5cfg, quantization_config=dict(NF4, llm_int8_skip_modules=[])).quantised_modules()) == sorted(linear)
    only_attn = E.T5EncoderModel(t5cfg, quantization_config=dict(NF4, llm_int8_skip_modules=["DenseReluDense"])).quantised_modules()
    assert sorted(only_attn) == sorted(n for n in linear if "SelfAttention" in n)                 # replaced: the list no longer names wo
    clip = E.CLIPTextModelWithProjection(dict(num_hidden_layers=2), quantization_config=NF4)
    assert clip.quantization["skip"] == ["text_projection"]
    linear = [n for n, m in clip.named_modules() if isinstance(m, torch.nn.Linear)]
    assert sorted(clip.quantised_modules()) == sorted(n for n in linear if n != "text_projection") and len(linear) == 13
    every = E.CLIPTextModelWithProjection(dict(num_hidden_layers=2), quantization_config=dict(NF4, llm_int8_skip_modules=[]))
    assert sorted(every.quantised_modules()) == sorted(linear)
    with pytest.raises(NotImplementedError):                                                      # Q | K | V is one operand
        E.CLIPTextModel(dict(num_hidden_layers=1), quantization_config=dict(NF4, llm_int8_skip_modules=["k_proj"]))
    with pytest.raises(RuntimeError, match="weight_nf4"):
        t5.load_state_dict({"encoder.block.0.layer.0.SelfAttention.q.weight_nf4": torch.zeros(1, dtype=torch.uint8)})
