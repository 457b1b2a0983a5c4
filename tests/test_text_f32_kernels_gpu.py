"""GPU leg of the fp32 text-encoder kernels (csrc/text.hip: dwm_text_attention_f32, dwm_rmsnorm_rows_f32, dwm_text_embed_f32,
dwm_text_act_f32, reached through the dtype dispatch of ops.text_attention / rmsnorm_rows / text_embed / text_act).  The ladder of
tests/test_text_kernels_gpu.py with fp32 operands that are NOT bf16 values, so that a kernel rounding anything to bf16 fails.
Every launch: relative Frobenius error < TOL_KERNEL_F32 = 1e-4 (the kernel tolerance of tests/test_fp32_gpu.py) against fp64, and
the per-element bounds below, which are several orders tighter.

Attention: the element bound and the one-hot-V key census of tests/text_attn_f32_check.py (its docstring holds the derivation),
NaN-fenced strided fused-QKV inputs and a sentinel-fenced output.

RMSNorm: per element 32 u |ref|, u = 2^-24 - tests/test_text_kernels_gpu.py's allowance for the fp32 statistics (41 roundings of a
sum of positive terms, halved by the square root, + 7 for mean / eps / sqrt / reciprocal, + 2 for the products x r w = 30.5 u),
WITHOUT its bf16 term: the output is stored in fp32.

Embed: bit-equal (a copy, or one fp32 add of two fp32 values, which torch rounds the same way).

Activations: a dense fp32 grid in [-12, 12] against the fp64 formula, per element (6 |z| + 40) u |ref| + 2^-126 (x max(1, |gate|)
when gated), z = the argument of the activation's exponential: 1.702 x (quick-GELU), a^2 with a = max(-x, 0) / sqrt 2 (erf-GELU in
its erfc form: erfc(a) ~ e^-a^2), t = 2 sqrt(2 / pi) (x + 0.044715 x^3) (tanh-GELU).  Derivation: each result is x f(z) with
|d ln f / dz| <= 1, so an ABSOLUTE error dz of the computed z is a relative error dz of the result.  z is formed from x by at most
four rounded operations with rounded constants, each off by <= u |z|, and the deep-tail branch of kind 2 adds ln |x| (rounded once)
to it: dz <= 6 u |z|.  On top: the library function (exp within 3 ulp, erfc within 16 ulp = 32 u - the accuracy OpenCL demands
of them), 1 + e, the division and the products by x, 0.5 and the gate, one rounding each: <= 40 u.  A result below the smallest
normal number may be flushed: 2^-126, times the gate it is multiplied by.  At |z| = 100 this is 3.8e-5 relative; a bf16 kernel (one
rounding to 8 bits, 3.9e-3) or the hardware exp2 / log2 approximations on a large argument do not pass it."""
import pytest
import torch

from tests import text_attn_check as T
from tests import text_attn_f32_check as F

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
TOL_KERNEL_F32 = 1e-4                     # tests/test_fp32_gpu.py
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _launch(q, k, v, bias, n_seq, L, H, scale, causal, dev):
    """one fenced launch: q | k | v as column blocks of ONE NaN-fenced fp32 buffer (row stride 3 D + 32), out inside a sentinel buffer"""
    from opendwm_amd import ops
    D = H * 64
    iview, ibuf = F.fenced((n_seq * L, 3 * D), f32, dev, col_off=8, pad_cols=24)
    for i, t in enumerate((q, k, v)):
        iview[:, i * D:(i + 1) * D] = t
    before = ibuf.clone()
    oview, obuf = F.fenced((n_seq * L, D), f32, dev, col_off=4, pad_cols=4, fill="sentinel")
    ops.text_attention(iview[:, :D], iview[:, D:2 * D], iview[:, 2 * D:], oview, n_seq, L, H, scale, causal=causal, bias=bias)
    assert torch.equal(ibuf.view(torch.int32), before.view(torch.int32)), "the inputs or their fences were written"
    assert F.untouched(obuf, oview), "output fence touched"
    assert bool(torch.isfinite(oview).all()), "NaN / Inf / unwritten output elements (a fenced row reached a product, or a row was skipped)"
    return oview


@pytest.mark.parametrize("L", [1, 15, 16, 17, 32, 33, 64, 77, 127, 128])
def test_text_attention_f32_element_bound_and_key_census(dev, L):
    n, worst_frob, worst_ratio = 0, 0.0, 0.0
    for H in (1, 5):
        for n_seq in (1, 3):
            for mi, mode in enumerate(F.MODES):
                causal, scale = "causal" in mode, (1.0, 0.125)[(mi + H + n_seq + L) % 2]
                q, k, v, bias = F.make_inputs(n_seq, L, H, mode, scale, 100 * L + 10 * H + n_seq + mi, dev)
                W = F.Weights(q, k, bias, n_seq, L, H, scale, causal)
                o, bound = F.o_reference(W, v, n_seq, H)
                got = _launch(q, k, v, bias, n_seq, L, H, scale, causal, dev)
                what = f"L={L} H={H} n_seq={n_seq} {mode} scale={scale}"
                fro = F.frobenius(got, o, n_seq, L, H)
                r, at = F.worst(F.element_ratios(got, o, bound, n_seq, L, H))
                worst_frob, worst_ratio = max(worst_frob, fro), max(worst_ratio, r)
                assert fro < TOL_KERNEL_F32, f"relative Frobenius error {fro:.3e}; {what}"
                assert r <= 1.0, f"element bound: ratio {r:.3f} at (seq, head, query, channel) {at}; {what}"
                for c in range((L + 63) // 64):
                    got = _launch(q, k, F.v_onehot(n_seq, L, H, c, dev), bias, n_seq, L, H, scale, causal, dev)
                    r, at = F.worst(F.census_ratios(got, W, c, n_seq, H))
                    assert r <= 1.0, f"key census chunk {c}: ratio {r:.3f} at (seq, head, query, key - {64 * c}) {at}; {what}"
                n += 1
    print(f"text_attention_f32 L={L}: worst relative Frobenius error {worst_frob:.3e}, worst element ratio {worst_ratio:.3f}")
    assert n == 16


def test_text_attention_f32_both_scales_in_every_mode_and_twice_bit_equal(dev):
    L, H, n_seq = 77, 3, 2
    for mi, mode in enumerate(F.MODES):
        for scale in (1.0, 0.125):
            causal = "causal" in mode
            q, k, v, bias = F.make_inputs(n_seq, L, H, mode, scale, 7 + mi, dev)
            W = F.Weights(q, k, bias, n_seq, L, H, scale, causal)
            o, bound = F.o_reference(W, v, n_seq, H)
            got = _launch(q, k, v, bias, n_seq, L, H, scale, causal, dev).clone()
            r, at = F.worst(F.element_ratios(got, o, bound, n_seq, L, H))
            assert r <= 1.0, (mode, scale, r, at)
            assert F.frobenius(got, o, n_seq, L, H) < TOL_KERNEL_F32
            assert torch.equal(got, _launch(q, k, v, bias, n_seq, L, H, scale, causal, dev))


def test_text_attention_f32_is_not_the_bf16_kernel(dev):
    """the same fp32 values through the bf16 kernel miss the fp32 element bound: the bound tells the two paths apart on the device"""
    from opendwm_amd import ops
    L, H, n_seq, scale = 77, 2, 2, 0.125
    q, k, v, bias = F.make_inputs(n_seq, L, H, "causal_bias", scale, 3, dev)
    W = F.Weights(q, k, bias, n_seq, L, H, scale, True)
    o, bound = F.o_reference(W, v, n_seq, H)
    out16 = torch.empty(n_seq * L, H * 64, dtype=bf16, device=dev)
    ops.text_attention(q.to(bf16), k.to(bf16), v.to(bf16), out16, n_seq, L, H, scale, causal=True, bias=bias)
    assert F.worst(F.element_ratios(out16.float(), o, bound, n_seq, L, H))[0] > 10


def test_text_f32_refusals(dev):
    from opendwm_amd import ops
    for L in (0, 129):
        x = torch.zeros(max(L, 1), 64, dtype=f32, device=dev)
        with pytest.raises(NotImplementedError):
            ops.text_attention(x, x, x, torch.empty_like(x), 1, L, 1, 1.0)
    x = torch.zeros(77, 64, dtype=f32, device=dev)
    with pytest.raises(NotImplementedError):
        ops.text_attention(x, x, x, torch.empty_like(x), 1, 77, 2, 1.0)              # head width 32
    # mixed dtypes: every operand follows the first
    xb = x.to(bf16)
    for args in ((x, x, xb, torch.empty_like(x)), (x, xb, x, torch.empty_like(x)), (x, x, x, torch.empty_like(xb)),
                 (xb, xb, x, torch.empty_like(xb)), (xb, xb, xb, torch.empty_like(x))):
        with pytest.raises(RuntimeError):
            ops.text_attention(*args, 1, 77, 1, 1.0)
    w32, w16 = torch.ones(64, device=dev), torch.ones(64, dtype=bf16, device=dev)
    with pytest.raises(RuntimeError):
        ops.rmsnorm_rows(x, w32, 1e-6, out=torch.empty_like(xb))
    with pytest.raises(RuntimeError):
        ops.rmsnorm_rows(x, w16, 1e-6, out=torch.empty_like(x))
    with pytest.raises(RuntimeError):
        ops.rmsnorm_rows(xb, w32, 1e-6)                                              # the stream is fp32 on both paths
    ids = torch.zeros(1, 77, dtype=torch.int64)
    with pytest.raises(RuntimeError):
        ops.text_embed(ids, x, xb)
    with pytest.raises(RuntimeError):
        ops.text_embed(ids, xb, x)
    with pytest.raises(RuntimeError):
        ops.text_act(x, "gelu", out=torch.empty_like(xb))
    with pytest.raises(RuntimeError):
        ops.text_act(xb, "gelu", out=torch.empty_like(x))
    with pytest.raises(RuntimeError):
        ops.gemm(x, torch.zeros(64, 64, device=dev), split_k=1, w_planes=torch.zeros(64, 128, dtype=bf16, device=dev))


@pytest.mark.parametrize("D", [64, 128, 4096, 8192])
@pytest.mark.parametrize("rows", [1, 77, 231])
def test_rmsnorm_rows_f32(dev, D, rows):
    from opendwm_amd import ops
    g = torch.Generator(device="cpu").manual_seed(D + rows)
    x = torch.randn(rows, D, generator=g) * 3
    x[rows // 2] = 0                                             # a row of zeros
    x[rows - 1, D // 3] = 1e4                                    # an outlier channel
    w = (1 + 0.2 * torch.randn(D, generator=g)).to(dev)
    xv, xbuf = F.fenced((rows, D), f32, dev, col_off=4, pad_cols=12)
    xv.copy_(x)
    before = xbuf.clone()
    yv, ybuf = F.fenced((rows, D), f32, dev, col_off=8, pad_cols=4, fill="sentinel")
    eps = 1e-6
    ops.rmsnorm_rows(xv, w, eps, out=yv)
    assert F.untouched(ybuf, yv), "output fence touched"
    assert torch.equal(xbuf.view(torch.int32), before.view(torch.int32))
    x64 = xv.double()
    ref = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps) * w.double()
    r, at = T.worst(T._ratios(yv, ref, 32 * U24 * ref.abs()))
    assert r <= 1.0, f"ratio {r:.3f} at (row, column) {at}"
    assert float((yv.double() - ref).norm() / ref.norm()) < TOL_KERNEL_F32
    if rows > 1:
        assert bool((yv[rows // 2] == 0).all())
    assert ops.rmsnorm_rows(xv, w, eps).dtype == f32


def test_text_embed_f32_bit_equal(dev):
    from opendwm_amd import ops
    g = torch.Generator(device="cpu").manual_seed(3)
    vocab, D, n_seq, L = 301, 72, 3, 77
    table = torch.randn(vocab, D, generator=g).to(dev)
    pos = torch.randn(L + 3, D, generator=g).to(dev)
    assert not torch.equal(table, table.to(bf16).float())
    ids = torch.randint(0, vocab, (n_seq, L), generator=g)
    ids[0, 0], ids[0, 1], ids[2, L - 1] = 0, vocab - 1, vocab - 1                 # the first and the last vocabulary row
    for p in (None, pos):
        ov, obuf = F.fenced((n_seq * L, D), f32, dev, col_off=4, pad_cols=4, fill="sentinel")
        ops.text_embed(ids, table, p, out=ov)
        want = table[ids.to(dev).reshape(-1)]
        if p is not None:
            want = want + p[:L].repeat(n_seq, 1)
        assert F.untouched(obuf, ov) and torch.equal(ov, want)
    # ids already on the device are clamped by the kernel, never turned into an address outside the table
    bad = ids.clone()
    bad[1, 5], bad[1, 6] = -7, vocab + 1000
    ov, obuf = F.fenced((n_seq * L, D), f32, dev, col_off=4, pad_cols=4, fill="sentinel")
    ops.text_embed(bad.to(dev), table, out=ov)
    assert F.untouched(obuf, ov) and torch.equal(ov, table[bad.clamp(0, vocab - 1).to(dev).reshape(-1)])
    with pytest.raises(ValueError):
        ops.text_embed(bad, table)                                # on the host they are rejected


@pytest.mark.parametrize("kind", ["quick_gelu", "gelu", "gelu_new"])
def test_text_act_f32_dense_grid(dev, kind):
    from opendwm_amd import ops
    n = 1 << 17
    x = torch.cat([torch.linspace(-12.0, 12.0, n - 64, dtype=f64).float(),
                   torch.tensor([0.0, -0.0, 12.0, -12.0, 1e-30, -1e-30, 1e-6, -1e-6]), torch.linspace(-11.99, -5.0, 56)])
    x = x.reshape(-1, 64).to(dev)                                # fp32 values; all but a handful are not bf16 values
    ref = T.act_reference(x.double(), kind)
    yv, ybuf = F.fenced(tuple(x.shape), f32, dev, col_off=8, pad_cols=4, fill="sentinel")
    ops.text_act(x, kind, out=yv)
    assert F.untouched(ybuf, yv)
    r, at = T.worst(T._ratios(yv, ref, F.act_bound(x.double(), kind, ref)))
    print(f"text_act_f32 {kind}: worst ratio {r:.3f} at x = {float(x[at])}")
    assert r <= 1.0, f"{kind}: ratio {r:.3f} at {at}: x = {float(x[at])}, got {float(yv[at])}, fp64 {float(ref[at])}"
    assert float((yv.double() - ref).norm() / ref.norm()) < TOL_KERNEL_F32
    # gated: act(x[:, :F]) * x[:, F:] from one [rows, 2F] matrix
    g = torch.Generator(device="cpu").manual_seed(11)
    gate = (torch.randn(x.shape, generator=g) * 2).to(dev)
    xg_v, xg_buf = F.fenced((x.shape[0], 128), f32, dev, col_off=8, pad_cols=12)
    xg_v[:, :64], xg_v[:, 64:] = x, gate
    before = xg_buf.clone()
    refg = ref * gate.double()
    yv, ybuf = F.fenced(tuple(x.shape), f32, dev, col_off=8, pad_cols=4, fill="sentinel")
    ops.text_act(xg_v, kind, gated=True, out=yv)
    assert F.untouched(ybuf, yv) and torch.equal(xg_buf.view(torch.int32), before.view(torch.int32))
    r, at = T.worst(T._ratios(yv, refg, F.act_bound(x.double(), kind, refg, gate.double())))
    assert r <= 1.0, f"{kind} gated: ratio {r:.3f} at {at}"
    # the three kinds are told apart: the other two formulas are far outside the bound somewhere on the grid
    for other in ("quick_gelu", "gelu", "gelu_new"):
        if other != kind:
            o = T.act_reference(x.double(), other) * gate.double()
            assert T.worst(T._ratios(yv, o, F.act_bound(x.double(), other, o, gate.double())))[0] > 100.0, (kind, other)
