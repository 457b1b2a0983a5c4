"""dwm_fifo_slide_multi on the GPU: the in-place slide of a list of [outer][T][inner] buffers against torch.cat([x[:, 1:], fresh], 1),
bit for bit.  Every buffer is carved from a larger allocation whose bytes on both sides must come back unchanged (the fence idea of
tests/gemm_check.py).  Sizes: the smallest rows of each piece width (2, 4, 16 bytes), rows that are no multiple of 16 (6, 132: the
added_time_ids rows), a ragged last block (4112 = 257 pieces) and a row that spans two blocks (one block's chunk + 16 bytes)."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
GUARD, FILL = 256, 0xA5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


class Carved:
    """a tensor of `shape` inside an arena of FILL bytes, GUARD (+ misalign) bytes from its start"""
    def __init__(self, shape, dtype, dev, misalign=0):
        n = torch.empty(shape, dtype=dtype).numel() * torch.empty((), dtype=dtype).element_size()
        self.arena = torch.full((GUARD + misalign + n + GUARD,), FILL, dtype=torch.uint8, device=dev)
        self.lo, self.hi = GUARD + misalign, GUARD + misalign + n
        self.t = self.arena[self.lo:self.hi].view(dtype).view(shape)

    def fences_intact(self):
        return bool((self.arena[:self.lo] == FILL).all()) and bool((self.arena[self.hi:] == FILL).all())


def _ints(shape, dtype, dev, seed):
    g = torch.Generator().manual_seed(seed)
    info = torch.iinfo(dtype)
    return torch.randint(max(info.min, -2 ** 40), min(info.max, 2 ** 40), shape, generator=g, dtype=torch.int64).to(dtype).to(dev)


def _tie_floats(shape, dev, seed):
    """fp32 values whose low 16 bits sit on and next to the bf16 rounding tie: ...8000 (tie: to even), 7fff, 8001, 0000"""
    g = torch.Generator().manual_seed(seed)
    hi = (torch.randn(shape, generator=g) * 3).to(bf16).view(torch.int16).to(torch.int32) << 16
    low = torch.tensor([0x8000, 0x7FFF, 0x8001, 0x0000, 0x8000], dtype=torch.int32)[torch.randint(0, 5, shape, generator=g)]
    return (hi | low).view(torch.float32).to(dev)


CASES = [(T, outer, fo) for T in (1, 2, 3, 7) for outer, fo in ((1, 1), (2, 2), (2, 1), (4, 4), (4, 2))]


def _inner_bytes():
    from opendwm_amd import ops
    return [2, 6, 16, 48, 132, 4112, ops.FIFO_CHUNK * 16 + 16]


@pytest.mark.parametrize("convert", [0, 1])
@pytest.mark.parametrize("k", range(7))
def test_slide_equals_cat(dev, k, convert):
    from opendwm_amd import ops
    nbytes = _inner_bytes()[k]
    inner = nbytes // 2                                          # 2-byte elements: int16 bytes, or bf16 converted from fp32
    for seed, (T, outer, fo) in enumerate(CASES):
        if convert:
            x = Carved((outer, T, inner), bf16, dev)
            x.t.copy_(_tie_floats((outer, T, inner), dev, seed).to(bf16))
            fresh = Carved((fo, 1, inner), torch.float32, dev)
            fresh.t.copy_(_tie_floats((fo, 1, inner), dev, 100 + seed))
            new = fresh.t.to(bf16)
            assert new.numel() < 64 or not torch.equal(new.float(), fresh.t)      # the values do round
        else:
            x = Carved((outer, T, inner), torch.int16, dev)
            x.t.copy_(_ints((outer, T, inner), torch.int16, dev, seed))
            fresh = Carved((fo, 1, inner), torch.int16, dev)
            fresh.t.copy_(_ints((fo, 1, inner), torch.int16, dev, 100 + seed))
            new = fresh.t
        want = torch.cat([x.t[:, 1:], new.repeat(outer // fo, 1, 1)], 1)      # buf[o][T - 1] = fresh[o % fresh_outer]
        keep = fresh.t.clone()
        ops.fifo_slide([x.t], [fresh.t])
        torch.cuda.synchronize()
        assert torch.equal(x.t, want), (nbytes, T, outer, fo)
        assert x.fences_intact() and fresh.fences_intact() and torch.equal(fresh.t, keep), (nbytes, T, outer, fo)


@pytest.mark.parametrize("convert", [0, 1])
def test_misaligned_buffer_takes_the_narrow_path(dev, convert):
    """buf two bytes off a 16-byte boundary, rows a multiple of 16 bytes: 2-byte pieces, still exact and inside its bytes"""
    from opendwm_amd import ops
    for T, outer, fo, inner in ((3, 2, 1, 24), (7, 4, 2, 520), (1, 2, 2, 8)):
        x = Carved((outer, T, inner), bf16 if convert else torch.int16, dev, misalign=2)
        assert x.t.data_ptr() % 16 == 2
        if convert:
            x.t.copy_(_tie_floats((outer, T, inner), dev, 5).to(bf16))
            fresh = _tie_floats((fo, 1, inner), dev, 6)
            new = fresh.to(bf16)
        else:
            x.t.copy_(_ints((outer, T, inner), torch.int16, dev, 5))
            fresh = new = _ints((fo, 1, inner), torch.int16, dev, 6)
        want = torch.cat([x.t[:, 1:], new.repeat(outer // fo, 1, 1)], 1)
        plan = ops.FifoSlide([(x.t, fresh, outer, T)])
        assert plan.host_items[0].n == outer * inner              # one column per 2-byte piece
        plan.run()
        torch.cuda.synchronize()
        assert torch.equal(x.t, want) and x.fences_intact()


def test_one_launch_slides_a_mixed_list(dev, monkeypatch):
    """five buffers of four dtypes, different T, rows of 132 / 48 / 40 / 6 / 2064 bytes, one of them converted: ONE launch"""
    from opendwm_amd import ops
    g = torch.Generator().manual_seed(11)
    a = Carved((2, 3, 33), torch.float32, dev)
    a.t.copy_(torch.randn(2, 3, 33, generator=g))
    fa = torch.randn(2, 1, 33, generator=g).to(dev)
    b = Carved((4, 7, 24), bf16, dev)
    b.t.copy_(_tie_floats((4, 7, 24), dev, 1).to(bf16))
    fb = _tie_floats((2, 1, 24), dev, 2)                          # fp32 -> bf16, both CFG halves take it
    c = Carved((1, 2, 5), torch.int64, dev)
    c.t.copy_(_ints((1, 2, 5), torch.int64, dev, 3))
    fc = _ints((1, 1, 5), torch.int64, dev, 4)
    d = Carved((2, 1, 6), torch.bool, dev)
    d.t.copy_(torch.rand(2, 1, 6, generator=g) < 0.5)
    fd = (torch.rand(2, 1, 6, generator=g) < 0.5).to(dev)
    e = Carved((2, 3, 1032), bf16, dev)
    e.t.copy_(torch.randn(2, 3, 1032, generator=g))
    fe = torch.randn(2, 1, 1032, generator=g).to(bf16).to(dev)
    bufs, fresh = [a, b, c, d, e], [fa, fb, fc, fd, fe]
    want = [torch.cat([x.t[:, 1:], (f.to(x.t.dtype)).repeat(x.t.shape[0] // f.shape[0], 1, 1)], 1) for x, f in zip(bufs, fresh)]
    launches = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *args: (launches.append(name), real(name, *args))[1])
    ops.fifo_slide([x.t for x in bufs], fresh)
    torch.cuda.synchronize()
    assert launches == ["dwm_fifo_slide_multi"]
    for x, w in zip(bufs, want):
        assert torch.equal(x.t, w) and x.fences_intact(), x.t.dtype
    # a kept plan slides again: three more frames of the fp32 buffer walk through it in order
    plan = ops.FifoSlide([(a.t, fa, 2, 3)])
    for i in range(3):
        fa.fill_(float(i))
        plan.run()
    torch.cuda.synchronize()
    assert torch.equal(a.t, torch.arange(3.0, device=dev).view(1, 3, 1).expand(2, 3, 33)) and a.fences_intact()


def test_raw_entry_point_returns_status_codes_and_writes_nothing(dev):
    from opendwm_amd import _lib, ops
    lib = _lib.load()
    x = Carved((2, 3, 8), torch.float32, dev)
    x.t.copy_(torch.arange(48.0).view(2, 3, 8))
    keep = x.t.clone()
    fresh = torch.ones(2, 1, 8, device=dev)
    plan = ops.FifoSlide([(x.t, fresh, 2, 3)])
    stream = torch.cuda.current_stream().cuda_stream

    def call(host=True, n_items=1, items=True, bi=True, bs=True, n_blocks=None, chunk=plan.chunk, **kw):
        it = _lib.FifoItem.from_buffer_copy(plan.host_items[0])
        for k, v in kw.items():
            setattr(it, k, v)
        arr = (_lib.FifoItem * 1)(it)
        return lib.dwm_fifo_slide_multi(arr if host else None, n_items, plan.items.data_ptr() if items else None,
                                        plan.block_item.data_ptr() if bi else None, plan.block_start.data_ptr() if bs else None,
                                        plan.block_item.numel() if n_blocks is None else n_blocks, chunk, stream)
    for bad in (dict(host=False), dict(items=False), dict(bi=False), dict(bs=False), dict(buf=None), dict(fresh=None),
                dict(n_items=0), dict(n_items=-3), dict(n_blocks=0), dict(n_blocks=-1), dict(chunk=0), dict(chunk=-256), dict(chunk=100),
                dict(outer=-2), dict(T=-3), dict(T=0), dict(inner_bytes=-32), dict(inner_bytes=31), dict(fresh_outer=-2),
                dict(fresh_outer=0), dict(outer=3), dict(convert=2), dict(convert=-1), dict(n=5), dict(n_blocks=2),
                dict(fresh=x.t.data_ptr() + 64)):
        assert call(**bad) == -1, bad                             # DWM_EINVAL
    assert call(buf=x.t.data_ptr() + 1) == -2 and call(fresh=fresh.data_ptr() + 1) == -2      # DWM_EALIGN
    assert call(outer=1 << 31, fresh_outer=1 << 31) == -3         # DWM_EUNSUPPORTED
    torch.cuda.synchronize()
    assert torch.equal(x.t, keep) and x.fences_intact()
    assert call() == 0                                            # ... and the list as planned goes through
    torch.cuda.synchronize()
    assert torch.equal(x.t, torch.cat([keep[:, 1:], fresh], 1)) and x.fences_intact()
