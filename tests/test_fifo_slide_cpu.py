"""dwm_fifo_slide_multi / ops.FifoSlide / StreamingDriver(persistent=True) without a GPU: the C ABI declaration against its ctypes
mirror, the argument checks of the entry point (they run on the host, before any HIP call) and of the wrapper (before any launch)."""
import ctypes
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HDR = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3


def test_header_prototype_equals_the_signature_entry():
    from opendwm_amd import _lib, build
    assert _lib.ABI_VERSION == 18 and re.search(r"#define\s+DWM_ABI_VERSION\s+18\b", HDR)
    m = re.search(r"^int\s+dwm_fifo_slide_multi\s*\(([^)]*)\)\s*;", HDR, flags=re.M)
    assert m, "dwm_fifo_slide_multi is not declared in include/dwm_hip.h"
    ctype = {"const dwm_fifo_item*": ctypes.POINTER(_lib.FifoItem), "int64_t": ctypes.c_int64, "const int32_t*": ctypes.c_void_p,
             "const int64_t*": ctypes.c_void_p, "void*": ctypes.c_void_p}
    params = [" ".join(p.split()).rsplit(" ", 1) for p in m.group(1).split(",")]
    assert [n for _, n in params] == ["host_items", "n_items", "items", "block_item", "block_start", "n_blocks", "chunk", "stream"]
    res, args = _lib.SIGNATURES["dwm_fifo_slide_multi"]
    want = [ctype[t] for t, _ in params]
    want[2] = ctypes.c_void_p                                  # the DEVICE copy of the items travels as an address
    assert res is ctypes.c_int32 and args == want
    assert "fifo.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "fifo.hip"))


def test_ctypes_item_matches_the_header_struct():
    from opendwm_amd import _lib
    body = HDR[HDR.index("typedef struct dwm_fifo_item"):HDR.index("} dwm_fifo_item;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decl = re.findall(r"(const void\*|void\*|int64_t)\s+(\w+)\s*;", body)
    assert [n for _, n in decl] == [n for n, _ in _lib.FifoItem._fields_]
    for (ct, name), (_, field) in zip(decl, _lib.FifoItem._fields_):
        assert field is (ctypes.c_int64 if ct == "int64_t" else ctypes.c_void_p), name
    assert ctypes.sizeof(_lib.FifoItem) == 8 * len(decl) == 64


def test_entry_point_refuses_bad_lists_before_touching_the_device():
    """fake addresses, never dereferenced: every call returns its status code from the host-side checks, nothing is launched"""
    from opendwm_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    fn = lib.dwm_fifo_slide_multi
    fn.restype, fn.argtypes = _lib.SIGNATURES["dwm_fifo_slide_multi"]
    buf, fresh, tab, chunk = 1 << 24, 1 << 20, 1 << 28, 1024

    def call(n_blocks=None, chunk=chunk, items_dev=tab, bi=tab + 4096, bs=tab + 8192, host=True, n_items=1, **kw):
        it = dict(buf=buf, fresh=fresh, outer=2, T=3, inner_bytes=64, fresh_outer=2, convert=0, n=None)
        it.update(kw)
        a = (it["buf"] or 0) | (it["fresh"] or 0) | it["inner_bytes"]
        piece = 16 if a % 16 == 0 else 4 if a % 4 == 0 else 2
        if it["n"] is None:
            it["n"] = it["outer"] * (it["inner_bytes"] // piece)
        arr = (_lib.FifoItem * 1)(_lib.FifoItem(*[it[k] for k, _ in _lib.FifoItem._fields_]))
        nb = (max(it["n"], 1) + chunk - 1) // chunk if n_blocks is None and chunk > 0 else (n_blocks or 1)
        return fn(arr if host else None, n_items, items_dev, bi, bs, nb, chunk, None)

    for bad in (dict(host=False), dict(items_dev=None), dict(bi=None), dict(bs=None), dict(buf=None), dict(fresh=None)):
        assert call(**bad) == EINVAL, bad                                          # null pointers
    for bad in (dict(n_items=0), dict(n_items=-1), dict(n_blocks=-1), dict(chunk=0), dict(chunk=-1024), dict(chunk=1000),
                dict(outer=0), dict(outer=-2), dict(T=0), dict(T=-1), dict(inner_bytes=0), dict(inner_bytes=-16), dict(fresh_outer=0),
                dict(fresh_outer=-1)):
        assert call(**bad) == EINVAL, bad                                          # sizes that are not positive
    assert call(inner_bytes=63) == EINVAL and call(inner_bytes=31, convert=1) == EINVAL      # rows are multiples of 2 bytes
    assert call(outer=3, fresh_outer=2) == EINVAL and call(outer=2, fresh_outer=4) == EINVAL
    assert call(convert=2) == EINVAL and call(convert=-1) == EINVAL
    assert call(n=7) == EINVAL                                                     # not outer * inner_bytes / piece
    assert call(n_blocks=2) == EINVAL                                              # not the blocks the item needs
    assert call(fresh=buf) == EINVAL and call(fresh=buf + 2 * 3 * 64 - 16) == EINVAL and call(fresh=buf - 64) == EINVAL      # overlap
    assert call(fresh=buf - 2 * 64 * 2 + 16, convert=1) == EINVAL                   # an fp32 fresh frame is twice as long
    assert call(buf=buf + 1) == EALIGN and call(fresh=fresh + 1) == EALIGN and call(fresh=fresh + 2, convert=1) == EALIGN
    assert call(outer=1 << 31, fresh_outer=1 << 31, n_blocks=1) == EUNSUPPORTED
    assert call(outer=1 << 20, fresh_outer=1, inner_bytes=1 << 30, n_blocks=1) == EUNSUPPORTED       # 2^50 bytes, 2^46 columns


class _Device(torch.Tensor):
    """a host tensor that says it lives on the device: what the wrapper's checks look at, without a GPU"""
    @property
    def is_cuda(self):
        return True


def _dev(t):
    return t.as_subclass(_Device)


def test_wrapper_refuses_before_any_launch(monkeypatch):
    from opendwm_amd import ops
    calls = []
    monkeypatch.setattr(ops, "_call", lambda *a: calls.append(a))
    x, f = torch.zeros(2, 3, 8), torch.zeros(2, 1, 8)
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.fifo_slide([x], [f])                                                   # CPU tensors
    with pytest.raises(RuntimeError, match="device tensors"):
        ops.fifo_slide([_dev(x)], [f])
    big = _dev(torch.zeros(2, 4, 8))
    with pytest.raises(RuntimeError, match="overlaps"):
        ops.fifo_slide([big.view(-1)[:48].view(2, 3, 8)], [big.view(-1)[40:56].view(2, 1, 8)])
    with pytest.raises(RuntimeError, match="divides outer"):
        ops.fifo_slide([_dev(torch.zeros(3, 2, 8))], [_dev(torch.zeros(2, 1, 8))])  # outer % fresh_outer != 0
    with pytest.raises(RuntimeError, match="divides outer"):
        ops.fifo_slide([_dev(x)], [_dev(torch.zeros(2, 1, 7))])                    # not whole rows
    with pytest.raises(RuntimeError, match="only fp32 -> bf16"):
        ops.fifo_slide([_dev(x)], [_dev(f.to(torch.bfloat16))])                    # mismatched dtypes
    with pytest.raises(RuntimeError, match="only fp32 -> bf16"):
        ops.fifo_slide([_dev(x.to(torch.int64))], [_dev(f)])
    with pytest.raises(RuntimeError, match="multiple of 2"):
        ops.fifo_slide([_dev(torch.zeros(2, 3, 7, dtype=torch.uint8))], [_dev(torch.zeros(2, 1, 7, dtype=torch.uint8))])
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.fifo_slide([_dev(torch.zeros(2, 8, 3)).transpose(1, 2)], [_dev(f)])
    with pytest.raises(RuntimeError, match="one fresh tensor per buffer"):
        ops.fifo_slide([_dev(x)], [])
    assert calls == []
    # a good list: one launch, the item rows and the block tables of the header's rules
    b16 = _dev(torch.zeros(4, 3, 1032, dtype=torch.bfloat16))                      # 2064-byte rows: 129 pieces of 16 bytes
    ops.fifo_slide([_dev(x), b16], [_dev(f), _dev(torch.zeros(2, 1032))])
    (name, host, n, items, bi, bs, nb, chunk), = calls
    assert name == "dwm_fifo_slide_multi" and n == 2 and chunk == ops.FIFO_CHUNK and chunk % 256 == 0
    assert (host[0].outer, host[0].T, host[0].inner_bytes, host[0].fresh_outer, host[0].convert) == (2, 3, 32, 2, 0)
    assert (host[1].outer, host[1].T, host[1].inner_bytes, host[1].fresh_outer, host[1].convert) == (4, 3, 2064, 2, 1)
    piece0 = 16 if (x.data_ptr() | f.data_ptr()) % 16 == 0 else 4
    assert host[0].n == 2 * 32 // piece0 and host[1].n in (4 * 129, 4 * 516)
    assert nb == sum((h.n + chunk - 1) // chunk for h in host)


def test_persistent_driver_needs_a_stream_session():
    from opendwm_amd.drivers import StreamingDriver
    from opendwm_amd.pipeline import CTSDDenoiser, UNetDenoiser
    cfg = dict(inference_steps=6, sequence_length_per_iteration=3)

    class RunOnly:
        def run(self, *a, **kw):
            raise AssertionError("not reached")
    for den in (RunOnly(), UNetDenoiser.__new__(UNetDenoiser)):
        StreamingDriver(den, cfg)                                                  # the default driver takes any denoiser
        with pytest.raises(ValueError, match="stream session"):
            StreamingDriver(den, cfg, persistent=True)
    assert StreamingDriver(CTSDDenoiser(None, inference_steps=6), cfg, persistent=True).persistent
    assert not StreamingDriver(RunOnly(), cfg).persistent


def test_stream_session_refuses_sharded_denoisers():
    """the construction only: no collective runs"""
    from opendwm_amd.pipeline import CTSDDenoiser
    den = CTSDDenoiser(None, inference_steps=6)
    den.frame_shard = object()                                                     # what CTSDDenoiser(frame_group=...) leaves
    with pytest.raises(ValueError, match="frame_group / cfg_group"):
        den.begin_stream(torch.zeros(1, 3, 3, 16, 8, 12), {})
    den = CTSDDenoiser(None, inference_steps=6)
    den.cfg_group = object()
    with pytest.raises(ValueError, match="frame_group / cfg_group"):
        den.begin_stream(torch.zeros(1, 3, 3, 16, 8, 12), {})
    with pytest.raises(RuntimeError, match="begin_stream"):
        CTSDDenoiser(None, inference_steps=6).advance_stream(torch.zeros(1, 1, 3, 16, 8, 12), {})
