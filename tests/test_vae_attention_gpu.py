"""GPU leg of the fused VAE mid-block attention (csrc/vae_attention.hip, ops.vae_attention, AutoencoderKL.mid_attention).

Kernel level: fp64 softmax attention ON THE DEVICE from the same (bf16-rounded / fp32) inputs; bf16 against TOL_KERNEL = 6e-3, the
bound of the project's other bf16 kernel tests (a CPU emulation of a bf16 flash kernel - key tiles of 32, fp32 statistics and
accumulators, probabilities rounded to bf16 before P.V, bf16 output - gives 2.0-2.2e-3 on unit-normal inputs at these shapes, 1.6e-3
on the large-score inputs, 0 at P = 1: a margin of about 2.7); fp32 against test_fp32_gpu's TOL_KERNEL_F32 = 1e-4.
Model level: oracle.ctsd_oracle.vae_decode / vae_encode_moments on bf16-rounded weights, TOL_MODEL = 2e-2 (fp32 path: TOL_F32)."""
import pytest
import torch

from oracle import ctsd_oracle as O
from tests.common import rel_err
from tests.test_fp32_gpu import TOL_F32, TOL_KERNEL_F32
from tests.test_train_gpu import _log         # one JSON line per measurement into the suite's gpu_parity.log

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16, f32 = torch.bfloat16, torch.float32
TOL_KERNEL = 6e-3
TOL_MODEL = 2e-2
SMALL = dict(block_out_channels=(64, 64, 128, 128), layers_per_block=2, norm_num_groups=16, latent_channels=16)
FULL = dict(block_out_channels=(128, 256, 512, 512), layers_per_block=2, norm_num_groups=32, latent_channels=16)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _qkv(I, P, C, dev, seed, dt=bf16, large=False):
    """q, k, v as the three column blocks of one [I*P, 3C] buffer.  large: q x 3 and key row j x (0.25 + 2.75 j / (P - 1)), so
    the largest score grows along the keys: the running maximum moves at every key tile"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    buf = torch.randn(I * P, 3 * C, generator=g)
    if large:
        buf[:, :C] *= 3.0
        ramp = 0.25 + 2.75 * torch.arange(P, dtype=torch.float32) / (P - 1)
        buf[:, C:2 * C] *= ramp.repeat(I)[:, None]
    buf = buf.to(dt).to(dev)
    return buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:]


def _ref64(q, k, v, I, P, scale):
    C = q.shape[1]
    q, k, v = (t.double().reshape(I, P, C) for t in (q, k, v))
    logits = torch.matmul(q, k.transpose(1, 2)) * scale
    return torch.matmul(torch.softmax(logits, -1), v).reshape(I * P, C), logits.abs().max().item()


def _run(q, k, v, I, P):
    from opendwm_amd import ops
    out = torch.empty((I * P, q.shape[1]), dtype=q.dtype, device=q.device)
    return ops.vae_attention(q, k, v, out, I, P, q.shape[1] ** -0.5)


@pytest.mark.parametrize("I", [1, 3])
@pytest.mark.parametrize("P", [1, 31, 64, 65, 209, 836])
@pytest.mark.parametrize("C", [128, 512])
def test_kernel_bf16_vs_fp64(dev, C, P, I):
    """P below one key tile, not a multiple of 8, across query / key tile boundaries, the interactive config's 22 x 38; more than
    one image; operands strided (column blocks of one buffer)"""
    q, k, v = _qkv(I, P, C, dev, 100 + P)
    out = _run(q, k, v, I, P)
    ref, _ = _ref64(q, k, v, I, P, C ** -0.5)
    e = rel_err(out, ref)
    _log("vae_attention_bf16", C=C, P=P, I=I, rel=e)
    assert out.dtype == bf16 and e < TOL_KERNEL, e


def test_kernel_bf16_beyond_softmax_ceiling(dev):
    C, P = 512, 4100
    q, k, v = _qkv(1, P, C, dev, 7)
    e = rel_err(_run(q, k, v, 1, P), _ref64(q, k, v, 1, P, C ** -0.5)[0])
    _log("vae_attention_bf16", C=C, P=P, I=1, rel=e)
    assert e < TOL_KERNEL, e


@pytest.mark.parametrize("P", [209, 836])
@pytest.mark.parametrize("C", [128, 512])
def test_kernel_bf16_large_scores(dev, C, P):
    """the running maximum moves at every key tile, so the rescaling of O is exercised; the fp64 reference stays finite"""
    q, k, v = _qkv(1, P, C, dev, 11, large=True)
    ref, top = _ref64(q, k, v, 1, P, C ** -0.5)
    assert torch.isfinite(ref).all() and 15.0 < top < 80.0, top
    e = rel_err(_run(q, k, v, 1, P), ref)
    _log("vae_attention_bf16_large_scores", C=C, P=P, largest_logit=top, rel=e)
    assert e < TOL_KERNEL, e


@pytest.mark.parametrize("dt", [bf16, f32])
@pytest.mark.parametrize("C", [128, 512])
def test_kernel_isolation_and_bounds(dev, C, dt):
    """image 1 all NaN, the rows before and after the [I*P] rows NaN (q, k, v) / a sentinel (out): image 0 is finite and bit-equal
    to the I = 1 launch, the sentinel rows are untouched (a masked key that reached a product would show as NaN)"""
    from opendwm_amd import ops
    P, pad = 209, 40
    q, k, v = _qkv(1, P, C, dev, 21, dt)
    buf = torch.full((pad + 2 * P + pad, 3 * C), float("nan"), dtype=dt, device=dev)
    buf[pad:pad + P, :C], buf[pad:pad + P, C:2 * C], buf[pad:pad + P, 2 * C:] = q, k, v
    out = torch.full((pad + 2 * P + pad, C), 123.0, dtype=dt, device=dev)
    rows = slice(pad, pad + 2 * P)
    ops.vae_attention(buf[rows, :C], buf[rows, C:2 * C], buf[rows, 2 * C:], out[rows], 2, P, C ** -0.5)
    one = _run(q, k, v, 1, P)
    assert torch.isfinite(out[pad:pad + P].float()).all() and torch.equal(out[pad:pad + P], one)
    assert (out[:pad] == 123.0).all() and (out[pad + 2 * P:] == 123.0).all()
    assert rel_err(one, _ref64(q, k, v, 1, P, C ** -0.5)[0]) < (TOL_KERNEL if dt == bf16 else TOL_KERNEL_F32)


@pytest.mark.parametrize("dt", [bf16, f32])
def test_kernel_same_launch_twice_bit_equal(dev, dt):
    q, k, v = _qkv(3, 209, 512, dev, 5, dt)
    assert torch.equal(_run(q, k, v, 3, 209), _run(q, k, v, 3, 209))


@pytest.mark.parametrize("P", [31, 65, 836])
@pytest.mark.parametrize("C", [128, 512])
def test_kernel_fp32_vs_fp64(dev, C, P):
    q, k, v = _qkv(2, P, C, dev, 200 + P, f32)
    out = _run(q, k, v, 2, P)
    e = rel_err(out, _ref64(q, k, v, 2, P, C ** -0.5)[0])
    _log("vae_attention_f32", C=C, P=P, I=2, rel=e)
    assert out.dtype == f32 and e < TOL_KERNEL_F32, e


@pytest.mark.parametrize("C", [128, 512])
def test_kernel_fp32_large_scores(dev, C):
    q, k, v = _qkv(1, 209, C, dev, 11, f32, large=True)
    ref, top = _ref64(q, k, v, 1, 209, C ** -0.5)
    assert torch.isfinite(ref).all() and 15.0 < top < 80.0, top
    e = rel_err(_run(q, k, v, 1, 209), ref)
    _log("vae_attention_f32_large_scores", C=C, largest_logit=top, rel=e)
    assert e < TOL_KERNEL_F32, e


def test_wrapper_rejects_uncovered_channels(dev):
    q, k, v = _qkv(1, 64, 192, dev, 1)
    with pytest.raises(RuntimeError, match="head dimension"):
        _run(q, k, v, 1, 64)


# --------------------------------------------------------------------------------- model level
def _bf16_round_sd(sd):
    return {k: v.to(bf16).float() for k, v in sd.items()}


@pytest.fixture(scope="module")
def small_vae(dev):
    from opendwm_amd.vae import AutoencoderKL
    sd = _bf16_round_sd(O.make_vae_state_dict(SMALL, 0))
    vae = AutoencoderKL(**SMALL)
    vae.load_state_dict(sd)
    return vae.to(dev).to(bf16).eval(), sd


def _latents(n, h, w, seed=3):
    return torch.randn(n, 16, h, w, generator=torch.Generator().manual_seed(seed)).to(bf16).float()


@pytest.mark.parametrize("h,w", [(6, 10), (11, 19)])
def test_vae_decode_any_size_vs_oracle(dev, small_vae, h, w):
    """P = 60 and P = 209 pixels per latent: no multiple of 64, so these decodes raise NotImplementedError without the fused route"""
    vae, sd = small_vae
    z = _latents(3, h, w)
    ref = O.vae_decode(sd, SMALL, z)
    out = vae.decode(z.to(dev), return_dict=False, chunk=2)[0]
    e = rel_err(out, ref)
    _log("vae_decode_any_size", h=h, w=w, rel=e)
    assert vae.mid_attention == "auto" and out.shape == (3, 3, 8 * h, 8 * w) and e < TOL_MODEL, e


def test_vae_encode_any_size_vs_oracle(dev, small_vae):
    vae, sd = small_vae
    x = (torch.rand(3, 3, 48, 80, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(bf16).float()
    ref = O.vae_encode_moments(sd, SMALL, x)
    mom = vae.encode(x.to(dev), chunk=2).latent_dist.parameters
    e = rel_err(mom, ref)
    _log("vae_encode_any_size", rel=e, shape=list(mom.shape))
    assert mom.shape == (3, 32, 6, 10) and e < TOL_MODEL, e


def test_vae_decode_any_size_fp32(dev):
    from opendwm_amd.vae import AutoencoderKL
    sd = O.make_vae_state_dict(SMALL, 0)
    vae = AutoencoderKL(**SMALL)
    vae.load_state_dict(sd)
    vae = vae.to(dev).eval()
    vae.compute_dtype = f32
    z = torch.randn(3, 16, 6, 10, generator=torch.Generator().manual_seed(3))
    out = vae.decode(z.to(dev), return_dict=False)[0]
    e = rel_err(out, O.vae_decode(sd, SMALL, z))
    _log("vae_decode_any_size_fp32", rel=e)
    assert out.dtype == f32 and e < TOL_F32, e


def test_vae_full_width_interactive_geometry_on_device(dev):
    """the released widths (one head of 512) on one 22 x 38 latent -> 176 x 304 px, the interactive-generation config's geometry
    (P = 836 = 13 * 64 + 4), against the fp32 oracle evaluated on the device"""
    from opendwm_amd.vae import AutoencoderKL
    sd = _bf16_round_sd(O.make_vae_state_dict(FULL, 0))
    vae = AutoencoderKL(**FULL)
    vae.load_state_dict(sd)
    vae = vae.to(dev).to(bf16).eval()
    z = _latents(1, 22, 38, seed=0).to(dev)
    ref = O.vae_decode({k: v.to(dev) for k, v in sd.items()}, FULL, z)
    out = vae.decode(z, return_dict=False)[0]
    e = rel_err(out, ref)
    _log("vae_decode_full_width_22x38", rel=e, shape=list(out.shape))
    assert out.shape == (1, 3, 176, 304) and e < TOL_MODEL, e


def test_vae_decode_beyond_softmax_ceiling_on_device(dev, small_vae):
    """66 x 64 = 4224 pixels: a multiple of 64, only the softmax kernel's 4096 ceiling stood in the way"""
    vae, sd = small_vae
    z = _latents(1, 66, 64, seed=1).to(dev)
    ref = O.vae_decode({k: v.to(dev) for k, v in sd.items()}, SMALL, z)
    out = vae.decode(z, return_dict=False)[0]
    e = rel_err(out, ref)
    _log("vae_decode_66x64", rel=e)
    assert out.shape == (1, 3, 528, 512) and e < TOL_MODEL, e


def test_vae_routes_where_both_apply(dev, small_vae):
    """3 latents of 8 x 8 (P = 64): both routes meet the oracle, and "auto" IS the GEMM route there, bit for bit"""
    vae, sd = small_vae
    z = _latents(3, 8, 8)
    ref = O.vae_decode(sd, SMALL, z)
    outs = {}
    try:
        for mode in ("auto", "gemm", "fused"):
            vae.mid_attention = mode
            outs[mode] = vae.decode(z.to(dev), return_dict=False, chunk=2)[0]
    finally:
        vae.mid_attention = "auto"
    errs = {m: rel_err(o, ref) for m, o in outs.items()}
    _log("vae_decode_routes", **errs)
    assert errs["fused"] < TOL_MODEL and errs["gemm"] < TOL_MODEL, errs
    assert torch.equal(outs["auto"], outs["gemm"])
    vae.mid_attention = "gemm"
    try:
        with pytest.raises(NotImplementedError, match="mid_attention"):
            vae.decode(_latents(1, 6, 10).to(dev))
    finally:
        vae.mid_attention = "auto"
