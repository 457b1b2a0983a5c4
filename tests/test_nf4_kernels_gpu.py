"""GPU leg of the NF4 kernels (csrc/gemm_nf4.hip): dwm_nf4_quantize and dwm_nf4_dequantize bit for bit against the plain restatement
tests/nf4_ref.py, dwm_gemm_nf4 element by element inside the fp64 bounds tests/gemm_check.py derives (tests/test_nf4_cpu.py shows
that those bounds catch swapped nibbles, an absmax one block or one row off, a wrong table entry and scaled accumulators).

Every operand sits behind fences: A and the bf16 weights in NaN, q in 0xFF bytes (code 15 = 1.0), absmax and bias in NaN, every
output - the fp32 stream that is updated in place included - in the sentinel NaN pattern, compared bit for bit afterwards.
Neighbouring blocks and neighbouring rows of every weight differ 100 times in scale, so an index one block or one row off moves a
result far outside its bound."""
import pytest
import torch

from tests import gemm_check as G
from tests import nf4_ref as R

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16, f32 = torch.bfloat16, torch.float32

MS, NS, KS = (1, 15, 16, 17, 77, 129, 231), (8, 24, 64, 200), (64, 128, 192, 448)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def stepped_weight(n, k, seed):
    """bf16 [n, k] on the CPU: Gaussian, neighbouring blocks and rows 100 times apart in scale; where there is room, block 1 of
    row 1 all zero and block 0 of row 2 all negative"""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g)
    scale = torch.tensor([1.0, 100.0])[(torch.arange(n)[:, None] + torch.arange(k // 64)[None, :]) % 2]
    w = (w.view(n, k // 64, 64) * scale[:, :, None] * 0.02).view(n, k).to(bf16)
    if k >= 128:
        w[1, 64:128] = 0
    w[2, 0:64] = -w[2, 0:64].abs() - 0.001
    return w


def fenced_bytes(shape, dev):
    """(uint8 view [n, k2], the bf16 buffer around it, the bf16 interior): a q OUTPUT behind sentinel fences"""
    n, k2 = shape
    inner, buf = G.fenced_vec(n * k2 // 2, bf16, dev, off=8, fill="sentinel")
    return inner.view(torch.uint8).view(n, k2), buf, inner


def fenced_q(q, dev):
    """q as an OPERAND: a contiguous slice of a buffer of 0xFF bytes"""
    buf = torch.full((q.numel() + 128,), 0xFF, dtype=torch.uint8, device=dev)
    view = buf[64:64 + q.numel()].view(q.shape)
    view.copy_(q)
    return view


def fenced_absmax(absmax, dev, fill=G.NAN):
    inner, buf = G.fenced_vec(absmax.numel(), f32, dev, off=8, fill=fill)
    view = inner.view(absmax.shape)
    if fill != "sentinel":
        view.copy_(absmax)
    return view, buf, inner


# ------------------------------------------------------------------------------------------------- quantise / dequantise
@pytest.mark.parametrize("N", [8, 24, 200])
@pytest.mark.parametrize("K", [64, 192, 4096])
def test_quantize_bit_equal_to_the_reference(dev, N, K):
    from opendwm_amd import _lib, nf4, ops
    w_cpu = stepped_weight(N, K, 100 + N + K)
    w, _ = G.fenced((N, K), bf16, dev, col_off=8, pad_cols=24)                       # strided source, NaN all around
    G.put(w, w_cpu)
    want_q, want_absmax = R.quantize(w_cpu)
    q, absmax = ops.nf4_quantize(w)
    assert q.dtype == torch.uint8 and tuple(q.shape) == (N, K // 2) and absmax.dtype == f32 and tuple(absmax.shape) == (N, K // 64)
    assert torch.equal(q.cpu(), want_q) and torch.equal(absmax.cpu().view(torch.int32), want_absmax.view(torch.int32))
    # the same launch into fenced outputs
    qv, qbuf, qinner = fenced_bytes((N, K // 2), dev)
    av, abuf, ainner = fenced_absmax(want_absmax, dev, fill="sentinel")
    rc = _lib.load().dwm_nf4_quantize(w.data_ptr(), w.stride(0), N, K, nf4.device_code(dev).data_ptr(), qv.data_ptr(), av.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert G.untouched(qbuf, qinner) and G.untouched(abuf, ainner)
    assert torch.equal(qv.cpu(), want_q) and torch.equal(av.cpu().view(torch.int32), want_absmax.view(torch.int32))
    if K >= 128:
        assert bool((R.unpack(want_q)[1, 64:128] == 7).all()) and float(want_absmax[1, 1]) == 0      # the zero block is in the data
    assert int(R.unpack(want_q)[2, 0:64].min()) == 0 and int(R.unpack(want_q)[2, 0:64].max()) <= 7  # and the one-signed block


@pytest.mark.parametrize("N", [8, 24, 200])
@pytest.mark.parametrize("K", [64, 192, 4096])
def test_dequantize_bit_equal_to_the_reference(dev, N, K):
    from opendwm_amd import ops
    q_cpu, absmax_cpu = R.quantize(stepped_weight(N, K, 200 + N + K))
    want = R.dequantize(q_cpu, absmax_cpu)
    q = fenced_q(q_cpu, dev)
    absmax, _, _ = fenced_absmax(absmax_cpu, dev)
    out, buf = G.fenced((N, K), bf16, dev, col_off=8, pad_cols=24, fill="sentinel")
    assert ops.nf4_dequantize(q, absmax, out=out) is out
    assert G.untouched(buf, out)
    assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))
    assert torch.equal(ops.nf4_dequantize(q, absmax).cpu().view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------ GEMM
@pytest.fixture(scope="module")
def weights(dev):
    """(N, K) -> dict(q, absmax, bias: fenced operands on the device; wd: W' bf16 on the device; size), built once"""
    out = {}
    for N in NS:
        for K in KS:
            q_cpu, absmax_cpu = R.quantize(stepped_weight(N, K, 300 + N + K))
            bias, _ = G.fenced_vec(N, bf16, dev)
            G.put(bias, (torch.randn(N, generator=torch.Generator().manual_seed(N + K)) * 3).to(bf16))
            wd = R.dequantize(q_cpu, absmax_cpu)
            out[(N, K)] = dict(q=fenced_q(q_cpu, dev), absmax=fenced_absmax(absmax_cpu, dev)[0], bias=bias, wd=wd.to(dev),
                               size=float(wd.float().norm(dim=1).mean()))          # of a product element, A being unit Gaussian
    return out


def a_operand(dev, M, K, seed=7):
    a, _ = G.fenced((M, K), bf16, dev, col_off=16, pad_cols=48)
    G.put(a, torch.randn(M, K, generator=torch.Generator().manual_seed(seed + K)).to(bf16))
    return a


def launch(dev, a, w, with_bias, kind, seed=0):
    """one fenced launch -> (view, buffer, Ref)"""
    from opendwm_amd import ops
    M, N = a.shape[0], w["q"].shape[0]
    bias = w["bias"] if with_bias else None
    prod = G.product(a, w["wd"])
    if kind == "bf16":
        out, buf = G.fenced((M, N), bf16, dev, col_off=8, pad_cols=8, fill="sentinel")
        assert ops.gemm_nf4(a, w["q"], w["absmax"], bias, out=out) is out
        return out, buf, G.plain(prod, bias)
    stream, buf = G.fenced((M, N), f32, dev, col_off=4, pad_cols=4, fill="sentinel")
    before = torch.randn(MS[-1], N, generator=torch.Generator().manual_seed(seed + 5))[:M].to(dev) * w["size"]     # row r the same for every M
    G.put(stream, before)
    assert ops.gemm_nf4(a, w["q"], w["absmax"], bias, out32=stream) is stream
    return stream, buf, G.resid(prod, bias, res=before)


@pytest.mark.parametrize("kind", ["bf16", "f32_stream"])
@pytest.mark.parametrize("M", MS)
def test_gemm_inside_the_element_bound(dev, weights, M, kind):
    worst = (0.0, None)
    for K in KS:
        a = a_operand(dev, M, K)
        for N in NS:
            for with_bias in (False, True):
                tag = (M, N, K, with_bias, kind)
                view, buf, ref = launch(dev, a, weights[(N, K)], with_bias, kind)
                assert G.untouched(buf, view), ("output fence touched", tag)
                assert bool(torch.isfinite(view).all()), ("NaN / Inf in the result", tag)
                ratio = G.check(view, ref, K)
                if not ratio <= 1:
                    print("over the bound", tag, "(row, column, got, ref, ratio):", *G.worst(view, ref, K, 8), sep="\n    ")
                assert ratio <= 1, (ratio, tag)
                if ratio >= worst[0]:
                    worst = (ratio, tag)
    print(f"gemm_nf4 M = {M} {kind}: worst element ratio {worst[0]:.3f} at {worst[1]}")


@pytest.mark.parametrize("kind", ["bf16", "f32_stream"])
def test_rows_do_not_depend_on_the_row_count_and_launches_repeat(dev, weights, kind):
    for N, K in ((200, 448), (64, 192), (8, 64)):
        w = weights[(N, K)]
        a = a_operand(dev, 231, K)
        full, _, _ = launch(dev, a, w, True, kind)
        again, _, _ = launch(dev, a, w, True, kind)
        assert torch.equal(full.view(torch.int32 if kind != "bf16" else torch.int16), again.view(torch.int32 if kind != "bf16" else torch.int16))
        for rows in (77, 1):
            part, _, _ = launch(dev, a[:rows], w, True, kind)                        # the same rows and, for the stream, the same prefill
            assert torch.equal(part, full[:rows]), (N, K, rows, kind)
