"""GPU leg of the text-encoder kernels (csrc/text.hip; ops.text_attention, rmsnorm_rows, text_embed, text_act).

Attention: fp64 from the same bf16 inputs, the derived element bound and the one-hot-V key census of tests/text_attn_check.py
(its docstring holds the derivation), NaN-fenced strided fused-QKV inputs and a sentinel-fenced output.
RMSNorm: per element 1.01 2^-8 |ref| (one bf16 rounding, acting on the computed value) + 32 2^-24 |ref| for the fp32 statistics:
the sum of squares is a chain of at most 32 fused multiply-adds per thread, 6 shuffle adds and 3 adds across the waves (41
roundings of a sum of positive terms: 41 u relative, u = 2^-24); mean, + eps, square root and reciprocal add 1 + 1 + 2 + 5 u on
the way to r = rsqrt(.), which halves the error of its argument: 0.5 (41 + 2) + 7 = 28.5 u; the two multiplications x r w add 2 u.
Embed: bit-equal (one fp32 add of two bf16 values).  Activations: every bf16 value in [-12, 12], within one bf16 ulp of the fp64
formula - at that resolution quick-GELU, erf-GELU and tanh-GELU are three different functions."""
import pytest
import torch

from tests import text_attn_check as T

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _launch(q, k, v, bias, n_seq, L, H, scale, causal, dev):
    """one fenced launch: q | k | v as column blocks of ONE NaN-fenced buffer (row stride 3 D + 64), out inside a sentinel buffer"""
    from opendwm_amd import ops
    D = H * 64
    iview, ibuf = T.fenced((n_seq * L, 3 * D), bf16, dev, col_off=16, pad_cols=48)
    for i, t in enumerate((q, k, v)):
        iview[:, i * D:(i + 1) * D] = t
    before = ibuf.clone()
    oview, obuf = T.fenced((n_seq * L, D), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
    ops.text_attention(iview[:, :D], iview[:, D:2 * D], iview[:, 2 * D:], oview, n_seq, L, H, scale, causal=causal, bias=bias)
    assert torch.equal(ibuf.view(torch.int16), before.view(torch.int16)), "the inputs or their fences were written"
    assert T.untouched(obuf, oview), "output fence touched"
    assert bool(torch.isfinite(oview).all()), "NaN / Inf / unwritten output elements (a fenced row reached a product, or a row was skipped)"
    return oview


@pytest.mark.parametrize("L", [1, 15, 16, 17, 32, 33, 64, 77, 127, 128])
def test_text_attention_element_bound_and_key_census(dev, L):
    n = 0
    for H in (1, 5):
        for n_seq in (1, 3):
            for mi, mode in enumerate(T.MODES):
                causal, scale = "causal" in mode, (1.0, 0.125)[(mi + H + n_seq + L) % 2]
                q, k, v, bias = T.make_inputs(n_seq, L, H, mode, scale, 100 * L + 10 * H + n_seq + mi, dev)
                W = T.Weights(q, k, bias, n_seq, L, H, scale, causal)
                o, bound = T.o_reference(W, v, n_seq, H)
                got = _launch(q, k, v, bias, n_seq, L, H, scale, causal, dev)
                r, at = T.worst(T.element_ratios(got, o, bound, n_seq, L, H))
                assert r <= 1.0, f"element bound: ratio {r:.3f} at (seq, head, query, channel) {at}; L={L} H={H} n_seq={n_seq} {mode} scale={scale}"
                for c in range((L + 63) // 64):
                    got = _launch(q, k, T.v_onehot(n_seq, L, H, c, dev), bias, n_seq, L, H, scale, causal, dev)
                    r, at = T.worst(T.census_ratios(got, W, c, n_seq, H))
                    assert r <= 1.0, f"key census chunk {c}: ratio {r:.3f} at (seq, head, query, key - {64 * c}) {at}; L={L} H={H} n_seq={n_seq} {mode} scale={scale}"
                n += 1
    assert n == 16


def test_text_attention_both_scales_in_every_mode_and_twice_bit_equal(dev):
    """the parity rule above gives each (L, mode) one scale; here every mode gets both at L = 77, and a second launch is bit-equal"""
    L, H, n_seq = 77, 3, 2
    for mi, mode in enumerate(T.MODES):
        for scale in (1.0, 0.125):
            causal = "causal" in mode
            q, k, v, bias = T.make_inputs(n_seq, L, H, mode, scale, 7 + mi, dev)
            W = T.Weights(q, k, bias, n_seq, L, H, scale, causal)
            o, bound = T.o_reference(W, v, n_seq, H)
            got = _launch(q, k, v, bias, n_seq, L, H, scale, causal, dev).clone()
            r, at = T.worst(T.element_ratios(got, o, bound, n_seq, L, H))
            assert r <= 1.0, (mode, scale, r, at)
            assert torch.equal(got, _launch(q, k, v, bias, n_seq, L, H, scale, causal, dev))


def test_text_attention_refuses_long_sequences(dev):
    from opendwm_amd import ops
    for L in (0, 129):
        x = torch.zeros(max(L, 1), 64, dtype=bf16, device=dev)
        with pytest.raises(NotImplementedError):
            ops.text_attention(x, x, x, torch.empty_like(x), 1, L, 1, 1.0)


@pytest.mark.parametrize("D", [64, 128, 4096, 8192])
@pytest.mark.parametrize("rows", [1, 77, 231])
def test_rmsnorm_rows(dev, D, rows):
    from opendwm_amd import ops
    g = torch.Generator(device="cpu").manual_seed(D + rows)
    x = torch.randn(rows, D, generator=g) * 3
    x[rows // 2] = 0                                             # a row of zeros
    x[rows - 1, D // 3] = 1e4                                    # an outlier channel
    w = (1 + 0.2 * torch.randn(D, generator=g)).to(bf16)
    xv, xbuf = T.fenced((rows, D), f32, dev, col_off=4, pad_cols=12)
    xv.copy_(x)
    yv, ybuf = T.fenced((rows, D), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
    for eps in (1e-6,):
        ops.rmsnorm_rows(xv, w.to(dev), eps, out=yv)
        assert T.untouched(ybuf, yv), "output fence touched"
        x64 = xv.double()
        ref = x64 * torch.rsqrt(x64.pow(2).mean(-1, keepdim=True) + eps) * w.to(dev).double()
        bound = (1.01 * 2.0 ** -8 + 32 * 2.0 ** -24) * ref.abs()
        r, at = T.worst(T._ratios(yv, ref, bound))
        assert r <= 1.0, f"ratio {r:.3f} at (row, column) {at}"
        if rows > 1:
            assert bool((yv[rows // 2] == 0).all())


def test_text_embed_bit_equal(dev):
    from opendwm_amd import ops
    g = torch.Generator(device="cpu").manual_seed(3)
    vocab, D, n_seq, L = 301, 72, 3, 77
    table = torch.randn(vocab, D, generator=g).to(bf16).to(dev)
    pos = torch.randn(L + 3, D, generator=g).to(bf16).to(dev)
    ids = torch.randint(0, vocab, (n_seq, L), generator=g)
    ids[0, 0], ids[0, 1], ids[2, L - 1] = 0, vocab - 1, vocab - 1                 # the first and the last vocabulary row
    for p in (None, pos):
        ov, obuf = T.fenced((n_seq * L, D), f32, dev, col_off=4, pad_cols=4, fill="sentinel")
        ops.text_embed(ids, table, p, out=ov)
        want = table[ids.to(dev).reshape(-1)].float()
        if p is not None:
            want = want + p[:L].float().repeat(n_seq, 1)
        assert T.untouched(obuf, ov) and torch.equal(ov, want)
    # ids already on the device are clamped by the kernel, never turned into an address outside the table
    bad = ids.clone()
    bad[1, 5], bad[1, 6] = -7, vocab + 1000
    got = ops.text_embed(bad.to(dev), table)
    assert torch.equal(got, table[bad.clamp(0, vocab - 1).to(dev).reshape(-1)].float())
    with pytest.raises(ValueError):
        ops.text_embed(bad, table)                                # on the host they are rejected


@pytest.mark.parametrize("kind", ["quick_gelu", "gelu", "gelu_new"])
def test_text_act_every_bf16_value_within_one_ulp(dev, kind):
    from opendwm_amd import ops
    top = int(torch.tensor(12.0).to(bf16).view(torch.int16))                      # bit pattern of 12.0
    bits = torch.arange(0, top + 1, dtype=torch.int32)
    bits = torch.cat([bits, bits + 0x8000 - 0x10000, torch.zeros((-2 * (top + 1)) % 64, dtype=torch.int32)])      # sign bit set: as int16
    x = bits.to(torch.int16).view(bf16).reshape(-1, 64).to(dev)                               # every bf16 in [-12, 12]
    assert float(x.float().max()) == 12.0 and float(x.float().min()) == -12.0
    ref = T.act_reference(x.double(), kind)
    yv, ybuf = T.fenced(tuple(x.shape), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
    ops.text_act(x, kind, out=yv)
    assert T.untouched(ybuf, yv)
    r, at = T.worst(T._ratios(yv, ref, T.ulp_bf16(ref)))
    assert r <= 1.0, f"{kind}: {r:.3f} ulp at {at}: x = {float(x[at])}, got {float(yv[at])}, fp64 {float(ref[at])}"
    # gated: act(x[:, :F]) * x[:, F:] from one [rows, 2F] matrix
    g = torch.Generator(device="cpu").manual_seed(11)
    gate = (torch.randn(x.shape, generator=g) * 2).to(bf16).to(dev)
    xg_v, _ = T.fenced((x.shape[0], 128), bf16, dev, col_off=8, pad_cols=24)
    xg_v[:, :64], xg_v[:, 64:] = x, gate
    ref = ref * gate.double()
    yv, ybuf = T.fenced(tuple(x.shape), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
    ops.text_act(xg_v, kind, gated=True, out=yv)
    assert T.untouched(ybuf, yv)
    floor = T.TINY * gate.double().abs().clamp_min(1.0)
    r, at = T.worst(T._ratios(yv, ref, T.ulp_bf16(ref, floor)))
    assert r <= 1.0, f"{kind} gated: {r:.3f} ulp at {at}"
    # the three kinds are told apart: the other two formulas are many ulps away somewhere on the grid
    for other in ("quick_gelu", "gelu", "gelu_new"):
        if other != kind:
            o = T.act_reference(x.double(), other) * gate.double()
            assert T.worst(T._ratios(yv, o, T.ulp_bf16(o)))[0] > 4.0, (kind, other)
