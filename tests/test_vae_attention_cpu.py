"""CPU leg of the fused VAE mid-block attention: the ctypes mirror of dwm_vae_attn_args, the route selection of
AutoencoderKL.mid_attention (a pure function) and the argument checks of ops.vae_attention that need no device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf16, f32 = torch.bfloat16, torch.float32


def test_abi_mirror_matches_header():
    """dwm_vae_attn_args: the header's fields in the header's order (4 pointers, 6 int64, int32 + float: 88 bytes); both entry points
    are bound; additions do not move the ABI version"""
    from opendwm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
    body = hdr[hdr.index("typedef struct dwm_vae_attn_args"):hdr.index("} dwm_vae_attn_args;")]
    names = re.findall(r"[\s\*,]([A-Za-z_0-9]+)\s*[,;]", body)
    assert names == [f for f, _ in _lib.VaeAttnArgs._fields_] == ["q", "k", "v", "out", "ldq", "ldk", "ldv", "ldo", "I", "P", "C", "scale"]
    assert ctypes.sizeof(_lib.VaeAttnArgs) == 4 * 8 + 6 * 8 + 4 + 4
    assert _lib.VaeAttnArgs.C.offset == 80 and _lib.VaeAttnArgs.scale.offset == 84
    for name in ("dwm_vae_attention", "dwm_vae_attention_f32"):
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int32 and args == [ctypes.POINTER(_lib.VaeAttnArgs), ctypes.c_void_p]
    assert _lib.ABI_VERSION == 18 and re.search(r"#define DWM_ABI_VERSION 18\b", hdr)


def test_source_is_in_the_build():
    from opendwm_amd import build
    assert "vae_attention.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "vae_attention.hip"))


@pytest.mark.parametrize("dt", [bf16, f32])
def test_route_selection_auto(dt):
    from opendwm_amd.vae import mid_attention_route
    for C in (128, 512):
        assert [mid_attention_route(P, C, dt, "auto") for P in (64, 4096)] == ["gemm", "gemm"]
        assert [mid_attention_route(P, C, dt, "auto") for P in (60, 836, 4160)] == ["fused"] * 3
    assert mid_attention_route(836, 512, dt) == "fused"                  # "auto" is the default


def test_route_selection_forced_modes():
    from opendwm_amd.vae import mid_attention_route
    for P in (64, 4096, 60, 836, 4160):
        assert mid_attention_route(P, 512, bf16, "fused") == "fused"
    assert mid_attention_route(64, 512, bf16, "gemm") == "gemm" and mid_attention_route(4096, 128, f32, "gemm") == "gemm"
    for P in (60, 836, 4160):
        with pytest.raises(NotImplementedError, match="mid_attention"):
            mid_attention_route(P, 512, bf16, "gemm")
    with pytest.raises(ValueError):
        mid_attention_route(64, 512, bf16, "flash")


def test_route_selection_uncovered_channels():
    """C = 192: no instantiation of the kernel.  "fused" falls back to the GEMM route where that applies; elsewhere the error names
    both limits"""
    from opendwm_amd.vae import mid_attention_route
    assert mid_attention_route(64, 192, bf16, "fused") == "gemm" and mid_attention_route(4096, 192, bf16, "auto") == "gemm"
    for mode in ("auto", "fused"):
        with pytest.raises(NotImplementedError) as ei:
            mid_attention_route(836, 192, bf16, mode)
        assert "192" in str(ei.value) and "% 64" in str(ei.value) and "4096" in str(ei.value)


def test_default_mode_and_packed_weight():
    from opendwm_amd.vae import AutoencoderKL
    vae = AutoencoderKL(block_out_channels=(64, 64, 128, 128), norm_num_groups=16)
    assert vae.mid_attention == "auto"
    attn = vae.decoder.mid_block.attentions[0]
    pk = attn.packed()
    assert pk["w"].shape == (384, 128) and pk["b"].shape == (384,) and attn.packed() is pk
    assert torch.equal(pk["w"][128:256].float(), attn.to_k.weight.detach().to(pk["w"].dtype).float())


def test_wrapper_rejects_bad_arguments():
    from opendwm_amd import ops
    I, P, C = 2, 20, 128
    t = lambda rows=I * P, dt=bf16: torch.zeros(rows, C, dtype=dt)
    with pytest.raises(RuntimeError, match="device tensor"):
        ops.vae_attention(t(), t(), t(), t(), I, P, 1.0)                 # CPU tensors
    with pytest.raises(RuntimeError, match="all be bf16 or all fp32"):
        ops.vae_attention(t(), t(dt=f32), t(), t(), I, P, 1.0)
    with pytest.raises(RuntimeError, match="all be bf16 or all fp32"):
        ops.vae_attention(t(dt=f32), t(dt=f32), t(dt=f32), t(), I, P, 1.0)
    with pytest.raises(RuntimeError, match=r"k must be \[I\*P, C\]"):
        ops.vae_attention(t(), t(rows=I * P - 1), t(), t(), I, P, 1.0)
    with pytest.raises(RuntimeError, match=r"out must be \[I\*P, C\]"):
        ops.vae_attention(t(), t(), t(), t(rows=P), I, P, 1.0)
    with pytest.raises(RuntimeError, match="positive"):
        ops.vae_attention(t(), t(), t(), t(), 0, P, 1.0)


def test_launcher_argument_codes():
    """dwm_vae_attention* validate before they touch the device, so the codes can be read without one: null pointers and
    non-positive sizes DWM_EINVAL (-1), a pointer off 16 bytes or a stride off the 16-byte grid DWM_EALIGN (-2), a head dimension
    without an instantiation DWM_EUNSUPPORTED (-3)"""
    from opendwm_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for name, gran in (("dwm_vae_attention", 8), ("dwm_vae_attention_f32", 4)):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]

        def rc(**over):
            a = _lib.VaeAttnArgs()
            a.q, a.k, a.v, a.out = 0x10000, 0x20000, 0x30000, 0x40000
            a.ldq = a.ldk = a.ldv = 3 * 512
            a.ldo, a.I, a.P, a.C, a.scale = 512, 2, 836, 512, 512 ** -0.5
            for k, v in over.items():
                setattr(a, k, v)
            return fn(ctypes.byref(a), None)
        assert fn(None, None) == -1
        assert [rc(q=None), rc(out=None), rc(I=0), rc(P=0), rc(P=-5), rc(C=0), rc(ldo=256)] == [-1] * 7
        assert [rc(C=192, ldo=192), rc(C=64), rc(C=1024, ldq=3072, ldk=3072, ldv=3072, ldo=1024)] == [-3] * 3
        assert [rc(k=0x20008), rc(out=0x40002), rc(ldq=3 * 512 + gran // 2), rc(ldo=512 + 1)] == [-2] * 4
