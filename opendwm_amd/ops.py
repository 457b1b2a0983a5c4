"""Tensor-level wrappers around the C ABI (include/dwm_hip.h).  PyTorch supplies device
memory and the current HIP stream; all arithmetic happens in libdwm_hip.so.  Every
function raises if its tensors are not bf16 CUDA(HIP) tensors — there is no fallback."""
from __future__ import annotations

import contextlib
import ctypes as C
import functools
import os
import threading
from dataclasses import dataclass
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import (ACT_GELU_TANH, ACT_NONE, ACT_RELU, ACT_SILU, EPI_GEGLU, EPI_PLAIN, EPI_RESID,
                   EPI_RMSHEAD)

BIG = 1 << 30
bf16 = torch.bfloat16
f32 = torch.float32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _call(name: str, *args) -> None:
    """run entry point `name` (a key of _lib.SIGNATURES) on the current stream; a failure is reported under that name"""
    _lib.check(getattr(_lib.load(), name)(*args, _stream()), name)


def _dt(t: torch.Tensor):
    """dtype a wrapper expects of its tensors, chosen by its first one: fp32 = the accuracy path, anything else must be bf16"""
    return f32 if t.dtype == f32 else bf16


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _chk2d(t: torch.Tensor, name: str, dtype=bf16):
    if not t.is_cuda:
        raise RuntimeError(f"{name}: expected a device tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise RuntimeError(f"{name}: expected {dtype}, got {t.dtype}")
    if t.dim() != 2 or t.stride(1) != 1:
        raise RuntimeError(f"{name}: expected a 2-D tensor with contiguous rows, got {tuple(t.shape)} strides {t.stride()}")


def _chkvec(t: Optional[torch.Tensor], name: str, dtype=bf16):
    if t is None:
        return
    if not t.is_cuda or t.dtype != dtype or not t.is_contiguous():
        raise RuntimeError(f"{name}: expected a contiguous {dtype} device tensor")


# --------------------------------------------------------------------------------- GEMM
@dataclass
class PaddedGrid:
    """Zero-padded token grid [I, h+2, w+2] used by the implicit-GEMM 3x3 convolutions: compact pixel
    index m = (i*h + y)*w + x lives at row i*(h+2)(w+2) + (y+1)(w+2) + (x+1) of the padded matrix."""
    I: int
    h: int
    w: int

    @property
    def rows(self) -> int:
        return self.I * (self.h + 2) * (self.w + 2)

    @property
    def pixels(self) -> int:
        return self.I * self.h * self.w

    def fill(self, m: "_lib.RowMap2D") -> None:
        m.rw, m.rh = self.w, self.h
        m.rpitch, m.ipitch = self.w + 2, (self.h + 2) * (self.w + 2)
        m.origin = self.w + 2 + 1

    def tap_shifts(self):
        """row shift of tap (dy, dx), dy/dx in {-1,0,1}, in the order of a [N, 3, 3, C] weight"""
        return [(dy - 1) * (self.w + 2) + (dx - 1) for dy in range(3) for dx in range(3)]

    def fill_stride2(self, m: "_lib.RowMap2D") -> None:
        """map of the (h/2 x w/2) OUTPUT pixels of a stride-2 3x3 conv with diffusers' (0,1,0,1) padding onto
        this grid: output (y, x) reads input rows (2y + dy, 2x + dx), dy, dx in 0..2, i.e. padded rows
        (2y + 1 + dy, 2x + 1 + dx): origin = first interior row, taps shift by dy*(w+2) + dx."""
        m.rw, m.rh = self.w // 2, self.h // 2
        m.rpitch, m.ipitch = 2 * (self.w + 2), (self.h + 2) * (self.w + 2)
        m.origin = self.w + 2 + 1
        m.xstep = 2

    def tap_shifts_stride2(self):
        return [dy * (self.w + 2) + dx for dy in range(3) for dx in range(3)]

    def fill_stride2_sym(self, m: "_lib.RowMap2D") -> None:
        """stride-2 3x3 conv with symmetric padding 1 (diffusers Downsample2D(padding=1), SD 2.1 UNet): output (y, x)
        reads input rows (2y - 1 + dy, 2x - 1 + dx) = padded rows (2y + dy, 2x + dx): origin 0, same tap shifts."""
        self.fill_stride2(m)
        m.origin = 0

    def interior_index(self, device=None) -> torch.Tensor:
        """[pixels] int64 padded-row index of every compact pixel (host reference of the kernel's map).  device: where the index is
        made - the training backwards make it on the GPU, so that they hold no host-to-device copy (a captured train step)"""
        i = torch.arange(self.I, device=device)[:, None, None]
        y = torch.arange(self.h, device=device)[None, :, None]
        x = torch.arange(self.w, device=device)[None, None, :]
        return (i * (self.h + 2) * (self.w + 2) + (y + 1) * (self.w + 2) + x + 1).reshape(-1)


@dataclass
class TimeGrid:
    """Token rows [(b t v), (h w)] with one zero frame before and after every sequence:
    [B, T + 2, V*N, C] - the input layout of a Conv3d with kernel (3, 1, 1) / padding (1, 0, 0) run as a
    3-tap implicit GEMM (diffusers TemporalResnetBlock).  `vn` = V * h * w rows per frame."""
    B: int
    T: int
    vn: int

    @property
    def rows(self) -> int:
        return self.B * (self.T + 2) * self.vn

    @property
    def pixels(self) -> int:
        return self.B * self.T * self.vn

    def fill(self, m: "_lib.RowMap2D") -> None:
        m.rw, m.rh = self.vn, self.T
        m.rpitch, m.ipitch = self.vn, (self.T + 2) * self.vn
        m.origin = self.vn

    def tap_shifts(self):
        return [-self.vn, 0, self.vn]


@dataclass
class Grid3D:
    """Input layout of a causal 3x3x3 convolution (CogVideoXCausalConv3d) run as a 27-tap implicit GEMM: token rows
    ordered (frame t, video b, y, x) - a frame of all videos is one contiguous slab - with two context frames in
    front of the clip and a zero spatial border: [T + 2, B, h + 2, w + 2, C].  Compact pixel m = ((t*B + b)*h + y)*w + x
    lives at row ((t + 2)*B + b)*(h+2)(w+2) + (y+1)(w+2) + x + 1.  The context frames hold the previous chunk's last
    two input frames (or the first frame twice); there is no trailing padding (causal)."""
    T: int
    B: int
    h: int
    w: int

    @property
    def frame_rows(self) -> int:          # rows of one padded frame slab (all videos)
        return self.B * (self.h + 2) * (self.w + 2)

    @property
    def rows(self) -> int:
        return (self.T + 2) * self.frame_rows

    @property
    def pixels(self) -> int:
        return self.T * self.B * self.h * self.w

    def fill(self, m: "_lib.RowMap2D") -> None:
        m.rw, m.rh = self.w, self.h
        m.rpitch, m.ipitch = self.w + 2, (self.h + 2) * (self.w + 2)
        m.origin = 2 * self.frame_rows + self.w + 2 + 1

    def tap_shifts(self):
        """row shift of tap (dt, dy, dx) in the order of a [N, 3, 3, 3, C] weight; dt = 2 is the current frame"""
        return [(dt - 2) * self.frame_rows + (dy - 1) * (self.w + 2) + (dx - 1)
                for dt in range(3) for dy in range(3) for dx in range(3)]


def _overlaps(a: torch.Tensor, b: torch.Tensor) -> bool:
    """do the byte ranges spanned by two 2-D row-strided tensors intersect?"""
    def span(t):
        lo = t.data_ptr()
        return lo, lo + ((t.shape[0] - 1) * t.stride(0) + t.shape[1]) * t.element_size() if t.numel() else lo
    (a0, a1), (b0, b1) = span(a), span(b)
    return a0 < b1 and b0 < a1


def _gemm_dims(a, w, dt, rows, epilogue, a_grid, conv3x3, stride2, conv_taps, c_grid, fp32_checks):
    """operand checks and the (M, N, K, taps, nout, orow) of a dwm_gemm_args: M output pixels, `taps` K-axis taps, out [orow, nout]"""
    _chk2d(a, "a", dt)
    _chk2d(w, "w", dt)
    if not w.is_contiguous():
        raise RuntimeError("w must be contiguous [N, K]")
    N, K = w.shape
    taps = 9 if conv3x3 else len(conv_taps) if conv_taps is not None else 1
    # known asymmetry: dwm_gemm_f32's wrapper makes three checks (fp32_checks) that dwm_gemm_bf16's never made; kept as they were
    if fp32_checks and taps > 27:
        raise NotImplementedError("gemm (fp32): at most 27 taps (three groups of 9, each tap walked as three plane products)")
    if a_grid is not None:
        if a.shape[0] != a_grid.rows or a.shape[1] * taps != K or (fp32_checks and not a.is_contiguous()):
            raise RuntimeError(f"gemm: padded A {tuple(a.shape)} does not match grid / weight {tuple(w.shape)}")
        if stride2 and (not conv3x3 or a_grid.h % 2 or a_grid.w % 2):
            raise RuntimeError("gemm: stride2 needs conv3x3 on an even-sized grid")
        M = a_grid.pixels // 4 if stride2 else a_grid.pixels
    else:
        if fp32_checks and (conv3x3 or conv_taps is not None or stride2):
            raise RuntimeError("gemm: convolution taps need a_grid")
        M = a.shape[0] if rows is None else rows
        if a.shape[1] != K:
            raise RuntimeError(f"gemm: K mismatch {a.shape} x {w.shape}")
    if c_grid is not None and c_grid.pixels != M:
        raise RuntimeError("gemm: c_grid pixel count != M")
    return M, N, K, taps, N // 2 if epilogue == EPI_GEGLU else N, c_grid.rows if c_grid is not None else M


def _gemm_out(out, shape, dt, device, padded):
    """the [orow, nout] result matrix: allocated (zeroed when it is a padded grid, whose border the kernel leaves alone) or checked"""
    if out is None:
        out = (torch.zeros if padded else torch.empty)(shape, dtype=dt, device=device)
    _chk2d(out, "out", dt)
    if out.shape != shape:
        raise RuntimeError(f"gemm: out shape {tuple(out.shape)} != {shape}")
    return out


def _gemm_operands(g, dt, stream_dt, gate, rows_per_gate, res, res_mod, blend, alpha, rows_per_alpha, rms_w, rms_ncols, rms_eps):
    """the epilogue operands of a dwm_gemm_args.  dt: dtype of gate / rms_w; stream_dt: dtype of res / blend (fp32 where the bf16
    GEMM updates the fp32 residual stream)"""
    if gate is not None:
        _chk2d(gate, "gate", dt)
        g.gate, g.ld_gate, g.rows_per_gate = gate.data_ptr(), gate.stride(0), rows_per_gate
    if res is not None:
        _chk2d(res, "res", stream_dt)
        g.res, g.ld_res, g.res_mod = res.data_ptr(), res.stride(0), res_mod
    if blend is not None:
        _chk2d(blend, "blend", stream_dt)
        _chkvec(alpha, "alpha", f32)
        g.blend, g.ld_blend, g.alpha, g.rows_per_alpha = blend.data_ptr(), blend.stride(0), alpha.data_ptr(), rows_per_alpha
    if rms_w is not None:
        _chkvec(rms_w, "rms_w", dt)
        g.rms_w, g.rms_ncols, g.rms_eps = rms_w.data_ptr(), rms_ncols, rms_eps


def _gemm_maps(g, a, a_grid, conv3x3, stride2, conv_taps, c_grid, res, blend):
    """a_map, the taps and c_map of a dwm_gemm_args whose A / out (with res, blend) are padded token grids"""
    if a_grid is not None:
        if stride2:
            (a_grid.fill_stride2_sym if stride2 == "sym" else a_grid.fill_stride2)(g.a_map)
        else:
            a_grid.fill(g.a_map)
        shifts = conv_taps
        if conv3x3:
            shifts = a_grid.tap_shifts_stride2() if stride2 else a_grid.tap_shifts()
        if shifts is not None:
            g.ntaps, g.k_per_tap = len(shifts), a.shape[1]
            for t, sh in enumerate(shifts):
                g.tap_shift[t] = sh
    if c_grid is not None:
        c_grid.fill(g.c_map)
        for name, t in (("res", res), ("blend", blend)):
            if t is not None and t.shape[0] != c_grid.rows:
                raise RuntimeError(f"gemm: {name} must be a padded grid when c_grid is given")


def gemm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
         out: Optional[torch.Tensor] = None, epilogue: int = EPI_PLAIN, act: int = ACT_NONE,
         gate: Optional[torch.Tensor] = None, rows_per_gate: int = 1,
         res: Optional[torch.Tensor] = None, res_mod: int = 0,
         blend: Optional[torch.Tensor] = None, alpha: Optional[torch.Tensor] = None,
         rows_per_alpha: int = 1,
         rms_w: Optional[torch.Tensor] = None, rms_ncols: int = 0, rms_eps: float = 1e-6,
         a_grid=None, conv3x3: bool = False, stride2=False, conv_taps: Optional[list] = None,
         c_grid=None, out32: Optional[torch.Tensor] = None, mirror: bool = True, w_is_activation: bool = False,
         rows: Optional[int] = None, split_k: int = 0, tile: int = 0, _debug: int = 0,
         w_planes: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[M, Nout] = epilogue(a[M, K] @ w[N, K]^T).  See dwm_gemm_bf16.
    tile: 0 = the kernel's choice, 1 = 256 x 256 tiles, 2 = 256 x 128 tiles (two workgroups per CU).
    a_grid: A is a padded token grid (PaddedGrid.rows x C); M = its pixel count; with conv3x3 the K
    axis is 9 taps x C (w is [N, 9*C], tap-major).  c_grid: out / res / blend are padded grids.
    split_k: 0 = the kernel's rule (small tile grid + long K -> K ranges, fp32 partials, ordered reduction),
    1 = never, n > 1 = exactly n ranges.  _debug: ablation knobs, honoured only by -DDWM_DEV_HOOKS builds of the library.
    out32 (RESID): fp32 residual stream - `res` and `blend` are then fp32 matrices shaped like the output, the result goes to
    out32 in fp32 (out32 may be `res` or `blend` itself) and, rounded, to the bf16 `out`; mirror=False: no bf16 copy at all
    (`out` must be None; the call returns out32) - the hidden / context streams of the bf16 MMDiT forward.
    w_is_activation: `w` is a per-call tensor, not a parameter (fp32 path: its operand planes are not cached).
    fp32 `a`: the accuracy path (dwm_gemm_f32), all operands fp32; out32, mirror, tile and _debug are not looked at, and of split_k
    only the value 1: it forbids the kernel's own split-K rule, so that a row's sum does not depend on M (the text encoders);
    w_planes: split_weight(w, cache=False) where the caller holds the planes itself (they are then not looked up in, or added
    to, the process-wide cache of split_weight)."""
    if w_planes is not None and a.dtype != f32:
        raise RuntimeError("gemm: w_planes belongs to the fp32 path")
    if a.dtype == f32:
        return _gemm_f32(a, w, bias, out, rows, epilogue, act, gate, rows_per_gate, res, res_mod, blend, alpha, rows_per_alpha, rms_w,
                         rms_ncols, rms_eps, a_grid, conv3x3, stride2, conv_taps, c_grid, not w_is_activation, split_k == 1, w_planes)
    M, N, K, _, nout, orow = _gemm_dims(a, w, bf16, rows, epilogue, a_grid, conv3x3, stride2, conv_taps, c_grid, False)
    if not mirror:
        if out32 is None or out is not None:
            raise RuntimeError("gemm: mirror=False needs out32 and no `out`")
    else:
        out = _gemm_out(out, (orow, nout), bf16, a.device, c_grid is not None)
        if _overlaps(a, out):       # bf16 only (like the three checks of _gemm_dims, an asymmetry kept as it was)
            raise RuntimeError("gemm: `out` overlaps the A operand (a tile's output would overwrite rows other tiles still read)")
    _chkvec(bias, "bias")
    g = _lib.GemmArgs()
    g.A, g.lda, g.W, g.bias = a.data_ptr(), a.stride(0), w.data_ptr(), _p(bias)
    if out is not None:
        g.C, g.ldc = out.data_ptr(), out.stride(0)
    g.M, g.N, g.K, g.epilogue, g.act = M, N, K, epilogue, act
    if out32 is not None:           # the fp32-stream form: res / blend are fp32 and shaped like out32, no split-K
        if epilogue != EPI_RESID or res_mod != 0:
            raise RuntimeError("gemm: out32 needs the RESID epilogue (res_mod = 0; `res`, if any, in fp32)")
        _chk2d(out32, "out32", f32)
        if out32.shape != (orow, nout):
            raise RuntimeError("gemm: out32 must have the shape of the output")
        if res is not None and res.shape != out32.shape:
            raise RuntimeError("gemm: the fp32 res must have the shape of the output")
        g.C32, g.ldc32 = out32.data_ptr(), out32.stride(0)
        split_k = 1
    _gemm_operands(g, bf16, f32 if out32 is not None else bf16, gate, rows_per_gate, res, res_mod, blend, alpha, rows_per_alpha,
                   rms_w, rms_ncols, rms_eps)
    _gemm_maps(g, a, a_grid, conv3x3, stride2, conv_taps, c_grid, res, blend)
    g.reserved = _debug
    g.split_k = split_k
    g.tile = _gemm_tile_request(tile)
    # split-K scratch (fp32 partial tiles, a fixed 1 GiB): only handed over when the kernel's own rule can take it
    if split_k != 1 and epilogue in (EPI_PLAIN, EPI_RESID) and ((M + 255) // 256) * ((N + 255) // 256) <= 128 and K >= 1024:
        ws = _gemm_workspace(a.device)
        g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    _call("dwm_gemm_bf16", C.byref(g))
    return out if mirror else out32


# 4-wave GEMM kernels (gemm_bf16_4w.hip) for the calling thread's launches: the MMDiT inference forward and the MMDiT train step open a
# `gemm_4wave_scope` around their own launches (`model.gemm_4wave`); inside it `ops.gemm(..., tile=0)` asks for dwm_gemm_args.tile = 3
# ("automatic, and the 4-wave kernels may serve the launch").  Everything else - UNet, VAEs, direct ops.gemm calls - keeps the 8-wave
# kernels.  The switch is per thread (no module global to race on between models / streams driven from different threads); autograd
# runs backward on its own thread, so the training Functions re-open the scope there (`scope_of` / `capture_scope`).
# Environment DWM_GEMM4W (read HERE, on the host side - the library takes its kernel selection from dwm_gemm_args only): 0 = never,
# 1 = every automatic-tile launch, f = as the scope asks but the fast form only (dwm_gemm_args.tile = 4).
_G4W = threading.local()
_G4W_ENV = os.environ.get("DWM_GEMM4W", "")


def block_permute(src: torch.Tensor, dst: torch.Tensor, dims, src_strides, block_elems: int) -> torch.Tensor:
    """dst (dense, blocks in the order dims = (n0, n1, n2, n3)) <- src block at sum(i_k * src_strides[k]) (strides in blocks); blocks of
    `block_elems` contiguous elements.  dwm_block_permute: the pack / unpack of the frame-shard all-to-all (sharding.py)."""
    if not (src.is_cuda and dst.is_cuda and src.is_contiguous() and dst.is_contiguous() and src.dtype == dst.dtype):
        raise RuntimeError("block_permute: contiguous device tensors of one dtype expected")
    a = _lib.BlockPermuteArgs()
    a.src, a.dst = src.data_ptr(), dst.data_ptr()
    a.block_bytes = block_elems * src.element_size()
    n = 1
    for i in range(4):
        a.n[i], a.sstride[i] = dims[i], src_strides[i]
        n *= dims[i]
    if n * block_elems != src.numel() or dst.numel() != src.numel():
        raise RuntimeError("block_permute: dims x block size do not cover the tensors")
    _call("dwm_block_permute", C.byref(a))
    return dst


def head_exchange(src: torch.Tensor, dst: torch.Tensor, rows: int, S: int, R: int, Dr: int, merge: bool = False) -> torch.Tensor:
    """split (merge=False): src [rows, S * R * Dr] with contiguous rows (a column slice of a wider buffer is fine) -> dst dense
    [R, rows, S, Dr]; merge: src dense [R, rows, S, Dr] -> dst [rows, S * R * Dr].  dwm_head_exchange: the pack / unpack of the frame
    shard's head exchange (sharding.py), bf16 or fp32."""
    wide, dense = (dst, src) if merge else (src, dst)
    if not (src.is_cuda and dst.is_cuda and src.dtype == dst.dtype and src.element_size() in (2, 4)):
        raise RuntimeError("head_exchange: device tensors of one 2- or 4-byte dtype expected")
    if min(rows, S, R, Dr) <= 0:
        raise RuntimeError("head_exchange: rows, S, R and Dr must be positive")
    if wide.dim() != 2 or wide.stride(1) != 1 or tuple(wide.shape) != (rows, S * R * Dr) or (rows > 1 and wide.stride(0) < S * R * Dr):
        raise RuntimeError(f"head_exchange: the row-major side must be [rows, S * R * Dr] = [{rows}, {S * R * Dr}] with contiguous rows, "
                           f"got {tuple(wide.shape)} strides {wide.stride()}")
    if not dense.is_contiguous() or dense.numel() != rows * S * R * Dr:
        raise RuntimeError("head_exchange: the dense side must be contiguous with rows * S * R * Dr elements")
    ld = wide.stride(0) if rows > 1 else max(wide.stride(0), S * R * Dr)
    _call("dwm_head_exchange", src.data_ptr(), dst.data_ptr(), rows, S, R, Dr, src.element_size(), ld, 1 if merge else 0)
    return dst


FIFO_CHUNK = 1024               # columns (pieces of 16 / 4 / 2 bytes) per workgroup of dwm_fifo_slide_multi: 4 per thread, 16 KiB per frame


class FifoSlide:
    """A list of buffers that slide by one frame in ONE launch (dwm_fifo_slide_multi), planned once for buffers that stay where they are.

    pairs: (buf, fresh, outer, T) per entry.  buf: a contiguous device tensor read as [outer][T][inner], updated in place:
    buf[o][t] = buf[o][t + 1], buf[o][T - 1] = fresh[o % fresh_outer].  fresh: a contiguous device tensor of fresh_outer rows of the
    same inner size (fresh_outer = its element count / the inner element count, a divisor of outer), of buf's dtype - or fp32 for a
    bf16 buf, rounded as ops.cast_bf16 rounds.  It must not overlap buf.  The plan holds the tensors (their addresses are in its
    device tables) and is valid as long as nobody reallocates them; `run()` launches on the current stream and can be captured."""

    def __init__(self, pairs, chunk: int = FIFO_CHUNK):
        pairs = list(pairs)
        if not pairs:
            raise RuntimeError("fifo_slide: an empty list")
        self.chunk, self.tensors, rows = chunk, pairs, []
        dev = pairs[0][0].device
        for buf, fresh, outer, T in pairs:
            if not (torch.is_tensor(buf) and torch.is_tensor(fresh) and buf.is_cuda and fresh.is_cuda):
                raise RuntimeError("fifo_slide: expected device tensors (the HIP path has no CPU fallback)")
            if buf.device != dev or fresh.device != dev or not buf.is_contiguous() or not fresh.is_contiguous():
                raise RuntimeError("fifo_slide: contiguous tensors on one device expected")
            convert = buf.dtype == bf16 and fresh.dtype == f32
            if fresh.dtype != buf.dtype and not convert:
                raise RuntimeError(f"fifo_slide: fresh is {fresh.dtype}, the buffer {buf.dtype} (only fp32 -> bf16 is converted)")
            if outer <= 0 or T <= 0 or buf.numel() == 0 or buf.numel() % (outer * T) != 0:
                raise RuntimeError(f"fifo_slide: a buffer of {buf.numel()} elements is not [outer = {outer}][T = {T}][inner]")
            inner = buf.numel() // (outer * T)
            inner_bytes = inner * buf.element_size()
            if inner_bytes % 2 != 0:
                raise RuntimeError(f"fifo_slide: rows of {inner_bytes} bytes (a multiple of 2 is needed)")
            if fresh.numel() == 0 or fresh.numel() % inner != 0 or outer % (fresh.numel() // inner) != 0:
                raise RuntimeError(f"fifo_slide: fresh has {fresh.numel()} elements: not a number of rows of {inner} that divides outer = {outer}")
            b0, f0 = buf.data_ptr(), fresh.data_ptr()
            if f0 < b0 + buf.numel() * buf.element_size() and b0 < f0 + fresh.numel() * fresh.element_size():
                raise RuntimeError("fifo_slide: fresh overlaps the buffer it is shifted into")
            a = b0 | f0 | inner_bytes
            piece = 16 if a % 16 == 0 else 4 if a % 4 == 0 else 2          # fifo_piece_bytes of csrc/fifo.hip
            rows.append((b0, f0, outer, T, inner_bytes, fresh.numel() // inner, int(convert), outer * (inner_bytes // piece)))
        self.bytes_moved = sum((2 * r[3] - 1) * r[2] * r[4] for r in rows)        # read T - 1 frames + fresh, write T (fresh as buf bytes)
        self.host_items = (_lib.FifoItem * len(rows))(*[_lib.FifoItem(*r) for r in rows])
        self.items = torch.tensor(rows, dtype=torch.int64).to(dev)                   # [n, 8] = dwm_fifo_item[n]
        bi, bs = [], []
        for i, r in enumerate(rows):
            nb = (r[-1] + chunk - 1) // chunk
            bi.append(torch.full((nb,), i, dtype=torch.int32))
            bs.append(torch.arange(nb, dtype=torch.int64) * chunk)
        self.block_item, self.block_start = torch.cat(bi).to(dev), torch.cat(bs).to(dev)

    def run(self) -> None:
        _call("dwm_fifo_slide_multi", self.host_items, len(self.host_items), _p(self.items), _p(self.block_item), _p(self.block_start),
              self.block_item.numel(), self.chunk)


def fifo_slide(bufs: Sequence[torch.Tensor], freshes: Sequence[torch.Tensor]) -> None:
    """slide every bufs[i] [outer, T, ...] by one frame along dim 1 in place and put freshes[i] ([fresh_outer, 1, ...] or
    [fresh_outer, ...]) into its last frame: torch.cat([buf[:, 1:], fresh], 1) without the allocation, all buffers in one launch.
    A one-off form of FifoSlide (which see); callers that slide the same buffers again and again keep a FifoSlide."""
    if len(bufs) != len(freshes):
        raise RuntimeError("fifo_slide: one fresh tensor per buffer")
    for b in bufs:
        if not torch.is_tensor(b) or b.dim() < 2:
            raise RuntimeError("fifo_slide: buffers are tensors [outer, T, ...]")
    FifoSlide([(b, f, b.shape[0], b.shape[1]) for b, f in zip(bufs, freshes)]).run()


ATTN_Q_PRESCALED = 1 << 15     # dwm_attn_args.variant: q arrives with scale * log2(e) folded in by its producer
ATTN_STREAM = 1 << 12           # ... the one-wave-per-SIMD streaming form of the resident kernel (attention_stream.hip): the library's default where it covers the launch
ATTN_RES12 = 1 << 13            # ... keep the 12-wave resident kernel there (A/B measurements)

# Environment DWM_ATTN_VARIANT (an integer, e.g. 0x1000): bits OR-ed into dwm_attn_args.variant of every ops.attention call (A/B
# measurements of the attention kernels; the library reads no environment).  DWM_ATTN_RES4=1 / 2 = bits 12 / 12 + 13 (round 5's name).
_ATTN_ENV_VARIANT = int(os.environ.get("DWM_ATTN_VARIANT", "0") or "0", 0) | \
    {"1": 1 << 12, "2": (1 << 12) | (1 << 13)}.get(os.environ.get("DWM_ATTN_RES4", "")[:1], 0)


def _gemm_tile_request(tile: int) -> int:
    """dwm_gemm_args.tile of one launch: the caller's explicit configuration (1 / 2), else 3 / 4 ("automatic, and the 4-wave kernels may
    serve the launch" / "... their fast form only") inside a gemm_4wave_scope or under DWM_GEMM4W=1"""
    if tile != 0:
        return tile
    env = _G4W_ENV[:1]
    on = getattr(_G4W, "on", False)
    if env == "0":
        return 0
    if env == "f":
        return 4 if on else 0
    if env not in ("", "0"):
        return 3
    return 3 if on else 0


def gemm_4wave_enabled() -> bool:
    return bool(getattr(_G4W, "on", False))


@contextlib.contextmanager
def gemm_4wave_scope(on: bool):
    prev = gemm_4wave_enabled()
    _G4W.on = bool(on)
    try:
        yield
    finally:
        _G4W.on = prev


# Ordered gradient reductions: inside `ordered_reductions(True)` the five reducing wrappers of opendwm_amd.train_ops
# launch the dwm_*_ordered entry points.  Per thread and carried into the backward exactly like the GEMM scope above.
_ORD = threading.local()


def ordered_reductions_enabled() -> bool:
    return bool(getattr(_ORD, "on", False))


@contextlib.contextmanager
def ordered_reductions(on: bool):
    prev = ordered_reductions_enabled()
    _ORD.on = bool(on)
    try:
        yield
    finally:
        _ORD.on = prev


def opens_ordered_scope(fn):
    """decorator for a training forward fn(model, ...): it runs inside ordered_reductions(model.ordered_reductions) - a plain
    attribute, False where it is absent (CTSDTrainer(deterministic=...) sets it)"""
    @functools.wraps(fn)
    def wrapped(model, *args, **kwargs):
        with ordered_reductions(getattr(model, "ordered_reductions", False)):
            return fn(model, *args, **kwargs)
    return wrapped


def carries_ordered_scope(cls):
    """class decorator for torch.autograd.Function subclasses: the backward (autograd's own thread) runs inside the
    ordered_reductions scope its forward ran in"""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *args, **kwargs):
        ctx._ordered_reductions = ordered_reductions_enabled()
        return fwd(ctx, *args, **kwargs)

    def backward(ctx, *grads):
        with ordered_reductions(getattr(ctx, "_ordered_reductions", False)):
            return bwd(ctx, *grads)

    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return cls


def carries_gemm_scope(cls):
    """class decorator for torch.autograd.Function subclasses: the backward (autograd's own thread) runs inside the
    gemm_4wave_scope and the ordered_reductions scope its forward ran in"""
    fwd, bwd = cls.forward, cls.backward

    def forward(ctx, *args, **kwargs):
        ctx._gemm_4wave = gemm_4wave_enabled()
        return fwd(ctx, *args, **kwargs)

    def backward(ctx, *grads):
        with gemm_4wave_scope(getattr(ctx, "_gemm_4wave", False)):
            return bwd(ctx, *grads)

    cls.forward, cls.backward = staticmethod(forward), staticmethod(backward)
    return carries_ordered_scope(cls)


_SPLIT_WEIGHTS: dict = {}
SPLIT_WEIGHT_CACHE_MAX = 2048        # > the ~1300 weight matrices of the largest model on the path


def split_weight(w: torch.Tensor, taps: int = 1, cache: bool = True) -> torch.Tensor:
    """fp32 [N, K] -> the pre-split bf16 operand [N, 3K] of dwm_gemm_f32 (hi = bf16(w), lo = bf16(w - hi)): [hi | lo | hi], or -
    `taps` > 1, K = taps x C tap-major (implicit convolution) - [hi_t | lo_t | hi_t] per tap t; more than 9 taps (the 27 of a causal
    3x3x3 convolution) are laid out as groups of 9, group g = [N, 9 * 3C] contiguous, one after the other (dwm_gemm_f32 walks a
    group per main-loop launch).
    Cached on the tensor's storage / version (weights and packed weights are long-lived), at most SPLIT_WEIGHT_CACHE_MAX entries
    (least recently used first out: per-call temporaries must not pile up); `clear_split_weights()` drops everything."""
    key = (w.data_ptr(), w._version, tuple(w.shape), taps)
    hit = _SPLIT_WEIGHTS.pop(key, None) if cache else None
    if hit is None:
        hi = w.to(bf16)
        lo = (w - hi.float()).to(bf16)
        if taps > 1:
            N, K = w.shape
            h3, l3 = hi.view(N, taps, K // taps), lo.view(N, taps, K // taps)
            ws = torch.stack([h3, l3, h3], 2)                                  # [N, taps, 3, C]
            if taps > 9:
                ws = torch.cat([ws[:, t0:t0 + 9].reshape(-1) for t0 in range(0, taps, 9)]).view(N, 3 * K)
            else:
                ws = ws.reshape(N, 3 * K).contiguous()
        else:
            ws = torch.cat([hi, lo, hi], 1).contiguous()
        hit = (ws, w)                                               # keeps `w` alive: its address is the key
    if not cache:
        return hit[0]
    _SPLIT_WEIGHTS[key] = hit                                       # (re-)inserted last: dict order = recency
    while len(_SPLIT_WEIGHTS) > SPLIT_WEIGHT_CACHE_MAX:
        _SPLIT_WEIGHTS.pop(next(iter(_SPLIT_WEIGHTS)))
    return hit[0]


def clear_split_weights() -> None:
    _SPLIT_WEIGHTS.clear()


def _gemm_f32(a, w, bias, out, rows, epilogue, act, gate, rows_per_gate, res, res_mod, blend, alpha, rows_per_alpha, rms_w, rms_ncols,
              rms_eps, a_grid, conv3x3, stride2, conv_taps, c_grid, cache_w, no_split=False, w_planes=None):
    """gemm() for fp32 operands (dwm_gemm_f32).  no_split: one K range whatever the tile grid (dwm_gemm_args.split_k = 1);
    w_planes: split_weight(w) held by the caller, used as it is"""
    M, N, K, taps, nout, orow = _gemm_dims(a, w, f32, rows, epilogue, a_grid, conv3x3, stride2, conv_taps, c_grid, True)
    out = _gemm_out(out, (orow, nout), f32, a.device, c_grid is not None)
    _chkvec(bias, "bias", f32)
    # the W operand is the pre-split bf16 planes of w (an activation in the W position - attention scores of the VAE - is not kept)
    if w_planes is None:
        ws = split_weight(w, taps, cache=cache_w)
    else:
        ws = w_planes
        _chk2d(ws, "w_planes", bf16)
        if taps != 1 or tuple(ws.shape) != (N, 3 * K) or not ws.is_contiguous():
            raise RuntimeError(f"gemm: w_planes must be the contiguous [N, 3K] = [{N}, {3 * K}] planes of a plain GEMM's weight")
    g = _lib.GemmArgs()
    g.A, g.lda, g.W, g.bias, g.C, g.ldc = a.data_ptr(), a.stride(0), ws.data_ptr(), _p(bias), out.data_ptr(), out.stride(0)
    g.M, g.N, g.K, g.epilogue, g.act = M, N, K, epilogue, act
    g.split_k = 1 if no_split else 0
    _gemm_operands(g, f32, f32, gate, rows_per_gate, res, res_mod, blend, alpha, rows_per_alpha, rms_w, rms_ncols, rms_eps)
    _gemm_maps(g, a, a_grid, conv3x3, stride2, conv_taps, c_grid, res, blend)
    # scratch, grown on demand: the operand planes of A + one set of fp32 partial slices per group of 9 taps
    a_rows = a_grid.rows if a_grid is not None else M
    groups = (taps + 8) // 9
    need = 4 * a_rows * (K // taps) + 256 + 4 * M * N * groups
    tiles = ((M + 255) // 256) * ((N + 255) // 256)
    if tiles * groups <= 128 and not no_split:
        need += 4 * M * N * min(32, 256 // tiles)          # room for the kernel's own split-K rule
    wsb = _f32_workspace(a.device, need)
    g.workspace, g.workspace_bytes = wsb.data_ptr(), wsb.numel() * 4
    _call("dwm_gemm_f32", C.byref(g))
    return out


_WORKSPACES: dict = {}
_F32_WORKSPACES: dict = {}
GEMM_WORKSPACE_BYTES = 1 << 30          # 1 GiB per (device, stream): up to ~8 K ranges of the largest weight gradient (12288 x 1536 fp32)


def _workspace(cache: dict, device: torch.device, nbytes: int, slack: int = 0) -> torch.Tensor:
    """fp32 scratch of at least `nbytes`, one per (device, stream) in `cache`; a new one is allocated with `slack` bytes to spare"""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = cache.get(key)
    if ws is None or ws.numel() * 4 < nbytes:
        ws = cache[key] = torch.empty((nbytes + slack) // 4, dtype=f32, device=device)
    return ws


def _f32_workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """scratch of dwm_gemm_f32 (operand planes + fp32 partial sums), grown on demand to the need + 64 MiB"""
    return _workspace(_F32_WORKSPACES, device, nbytes, 64 << 20)


def _gemm_workspace(device: torch.device) -> torch.Tensor:
    """fp32 scratch of the split-K GEMM path, a fixed size: partial tiles live there only between the
    two kernels of one dwm_gemm_bf16 call, so calls on one stream share it."""
    return _workspace(_WORKSPACES, device, GEMM_WORKSPACE_BYTES)


# ---------------------------------------------------------------------------- attention
@dataclass
class RowMap:
    """row(p, l) of include/dwm_hip.h; see the constructors below for the reference
    rearranges (crossview_temporal_dit.py:300-361) they encode."""
    L0: int
    n_problems: int
    pdiv: Sequence[int] = (1, 1, 1)
    pmod: Sequence[int] = (BIG, 1, 1)
    pstride: Sequence[int] = (0, 0, 0)
    ldiv: Sequence[int] = (BIG, BIG)
    lstride: Sequence[int] = (1, 0, 0)
    # group mask geometry (cross-view): mask index = p // p_per_mask, group(l) = (l // group_size) % G
    p_per_mask: int = 1
    group_size: int = 1

    def rows(self) -> torch.Tensor:
        """[n_problems, L0] int64 row indices (host reference of the kernel's addressing)."""
        p = torch.arange(self.n_problems)[:, None]
        l = torch.arange(self.L0)[None, :]
        r = torch.zeros(self.n_problems, self.L0, dtype=torch.int64)
        for d, m, s in zip(self.pdiv, self.pmod, self.pstride):
            r = r + ((p // d) % m) * s
        r = r + (l % self.ldiv[0]) * self.lstride[0] + ((l // self.ldiv[0]) % self.ldiv[1]) * self.lstride[1] \
            + (l // (self.ldiv[0] * self.ldiv[1])) * self.lstride[2]
        return r


def rowmap_identity(n_problems: int, L0: int) -> RowMap:
    """(b) n c: problem p owns rows p*L0 .. p*L0+L0-1 (joint / dual attention)."""
    return RowMap(L0=L0, n_problems=n_problems, pstride=(L0, 0, 0))


def rowmap_crossview_rowwise(B: int, T: int, V: int, h: int, w: int) -> RowMap:
    """(bt v) (h w) c -> (bt h) (v w) c   (crossview_temporal_dit.py:307-309)."""
    return RowMap(L0=V * w, n_problems=B * T * h,
                  pdiv=(h, 1, 1), pmod=(BIG, h, 1), pstride=(V * h * w, w, 0),
                  ldiv=(w, BIG), lstride=(1, h * w, 0), p_per_mask=T * h, group_size=w)


def rowmap_crossview_full(B: int, T: int, V: int, h: int, w: int) -> RowMap:
    """(bt v) (h w) c -> bt (h v w) c   (crossview_temporal_dit.py:290-292)."""
    return RowMap(L0=h * V * w, n_problems=B * T,
                  pstride=(V * h * w, 0, 0),
                  ldiv=(w, V), lstride=(1, h * w, w), p_per_mask=T, group_size=w)


def rowmap_crossview_pointwise(B: int, T: int, V: int, h: int, w: int) -> RowMap:
    """btv hw c -> (bt hw) v c: TemporalBasicTransformerBlock(num_frames=V) of the SD 2.1 UNet without row-wise
    cross-view attention (crossview_temporal.py:358-361, :228-229)."""
    hw = h * w
    return RowMap(L0=V, n_problems=B * T * hw,
                  pdiv=(hw, 1, 1), pmod=(BIG, hw, 1), pstride=(V * hw, 1, 0),
                  ldiv=(BIG, BIG), lstride=(hw, 0, 0), p_per_mask=T * hw, group_size=1)


def rowmap_temporal_rowwise(B: int, T: int, V: int, h: int, w: int) -> RowMap:
    """(b t v) (h w) c -> (b v h) (t w) c   (crossview_temporal_dit.py:345-347)."""
    return RowMap(L0=T * w, n_problems=B * V * h,
                  pdiv=(V * h, h, 1), pmod=(BIG, V, h), pstride=(T * V * h * w, h * w, w),
                  ldiv=(w, BIG), lstride=(1, V * h * w, 0))


def rowmap_temporal_full(B: int, T: int, V: int, h: int, w: int) -> RowMap:
    """(b t v) hw c -> (b v) (t hw) c   (crossview_temporal_dit.py:336-338)."""
    return RowMap(L0=T * h * w, n_problems=B * V,
                  pdiv=(V, 1, 1), pmod=(BIG, V, 1), pstride=(T * V * h * w, h * w, 0),
                  ldiv=(h * w, BIG), lstride=(1, V * h * w, 0))


# The temporal maps over the RECEIVED layout of the frame shard's head exchange (sharding.FrameShard.heads_gather): rows ordered
# (i, b, tl, v, n) with i the source rank, Tl = T / R frames per rank, frame t = i * Tl + tl, n = token of the h x w grid.  Problems and
# tokens are enumerated exactly as by the unsharded maps above, so the attention reads q / k / v from the receive buffer as it
# arrived and writes the send buffer of the way back: no rearranged copy on either side.
def rowmap_temporal_full_exchanged(B: int, Tl: int, R: int, V: int, h: int, w: int) -> RowMap:
    """rowmap_temporal_full(B, R * Tl, V, h, w) on rows ordered (i, b, tl, v, n)."""
    N = h * w
    return RowMap(L0=R * Tl * N, n_problems=B * V,
                  pdiv=(V, 1, 1), pmod=(BIG, V, 1), pstride=(Tl * V * N, N, 0),
                  ldiv=(N, Tl), lstride=(1, V * N, B * Tl * V * N))


def rowmap_temporal_rowwise_exchanged(B: int, Tl: int, R: int, V: int, h: int, w: int) -> RowMap:
    """rowmap_temporal_rowwise(B, R * Tl, V, h, w) on rows ordered (i, b, tl, v, n)."""
    N = h * w
    return RowMap(L0=R * Tl * w, n_problems=B * V * h,
                  pdiv=(V * h, h, 1), pmod=(BIG, V, h), pstride=(Tl * V * N, N, w),
                  ldiv=(w, Tl), lstride=(1, V * N, B * Tl * V * N))


def rowmap_temporal_pointwise(B: int, T: int, V: int, h: int, w: int) -> RowMap:
    """(b t v) hw c -> (b v hw) t c   (crossview_temporal_dit.py:354-356)."""
    hw = h * w
    return RowMap(L0=T, n_problems=B * V * hw,
                  pdiv=(V * hw, hw, 1), pmod=(BIG, V, hw), pstride=(T * V * hw, hw, 1),
                  ldiv=(BIG, BIG), lstride=(V * hw, 0, 0))


def _attn_problem(a, q, heads, scale, rowmap):
    """the part of a dwm_attn_args every form shares: heads (64 wide), the softmax scale and the row map"""
    a.heads, a.head_dim = heads, 64
    if q.shape[1] != heads * 64:
        raise RuntimeError("attention: head_dim must be 64")
    a.scale = float(scale) if scale is not None else 64 ** -0.5
    for i in range(3):
        a.pdiv[i], a.pmod[i], a.pstride[i] = rowmap.pdiv[i], rowmap.pmod[i], rowmap.pstride[i]
        a.lstride[i] = rowmap.lstride[i]
    a.ldiv[0], a.ldiv[1] = rowmap.ldiv


def _attn_lse(a, lse):
    """hand the optional log-sum-exp output to a filled dwm_attn_args"""
    if lse is not None:
        if lse.dtype != f32 or not lse.is_contiguous() or lse.numel() != a.n_problems * a.heads * (a.L0 + a.L1):
            raise RuntimeError("lse: fp32 contiguous [n_problems, heads, L0+L1] expected")
        a.lse = lse.data_ptr()


def _attn_bwd_launch(b, lse):
    """dwm_attention_bwd on a filled dwm_attn_bwd_args, with the forward's lse and a `delta` scratch of its size"""
    b.fwd.lse = lse.data_ptr()
    delta = torch.empty(lse.numel(), dtype=f32, device=lse.device)
    b.delta = delta.data_ptr()
    _call("dwm_attention_bwd", C.byref(b))
    delta.record_stream(torch.cuda.current_stream())


def _attn_args(a, q, k, v, out, rowmap, heads, q1, k1, v1, out1, scale, group_mask, dense_mask):
    """fill a dwm_attn_args; returns the uint8 mask tensor that must outlive the launch (or None)"""
    dt = _dt(q)                                                    # fp32: the accuracy path (dwm_attention_f32)
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _chk2d(t, name, dt)
    if not (q.stride(0) == k.stride(0) == v.stride(0)):
        raise RuntimeError("q, k, v must share a row stride")
    a.q0, a.k0, a.v0, a.ld0 = q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0)
    a.o0, a.ldo0 = out.data_ptr(), out.stride(0)
    a.L0, a.L1, a.n_problems = rowmap.L0, 0, rowmap.n_problems
    if q1 is not None:
        for name, t in (("q1", q1), ("k1", k1), ("v1", v1), ("out1", out1)):
            _chk2d(t, name, dt)
        if q1.shape[0] % rowmap.n_problems != 0:
            raise RuntimeError("segment 1 rows must be n_problems * L1")
        a.q1, a.k1, a.v1, a.ld1 = q1.data_ptr(), k1.data_ptr(), v1.data_ptr(), q1.stride(0)
        a.o1, a.ldo1 = out1.data_ptr(), out1.stride(0)
        a.L1 = q1.shape[0] // rowmap.n_problems
    _attn_problem(a, q, heads, scale, rowmap)
    a.mask_mode = 0
    keep = None
    if group_mask is not None:
        keep = group_mask.to(torch.uint8).contiguous()
        a.mask_mode, a.mask = 1, keep.data_ptr()
        a.mask_G, a.group_size, a.p_per_mask = keep.shape[-1], rowmap.group_size, rowmap.p_per_mask
    elif dense_mask is not None:
        keep = dense_mask.to(torch.uint8).contiguous()
        a.mask_mode, a.mask = 2, keep.data_ptr()
    return keep


def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor,
              rowmap: RowMap, heads: int, *,
              q1: Optional[torch.Tensor] = None, k1: Optional[torch.Tensor] = None,
              v1: Optional[torch.Tensor] = None, out1: Optional[torch.Tensor] = None,
              scale: Optional[float] = None,
              group_mask: Optional[torch.Tensor] = None, dense_mask: Optional[torch.Tensor] = None,
              variant: int = 0, lse: Optional[torch.Tensor] = None) -> None:
    """softmax(QK^T * scale [+mask]) V per (problem, head); q/k/v/out are 2-D [rows, heads*64]
    views sharing a row stride (e.g. column slices of a fused qkv buffer).  Segment 1
    (q1/k1/v1/out1: [n_problems*L1, heads*64]) is appended to every problem's key/query
    sequence (text context of the joint attention).  group_mask: bool/uint8 [Bm, G, G];
    dense_mask: bool/uint8 [n_problems, L, L].  lse (optional, fp32 [n_problems, heads, L0+L1])
    receives the negative log2-domain log-sum-exp the backward needs."""
    a = _lib.AttnArgs()
    keep = _attn_args(a, q, k, v, out, rowmap, heads, q1, k1, v1, out1, scale, group_mask, dense_mask)
    a.variant = variant | _ATTN_ENV_VARIANT
    _attn_lse(a, lse)
    _call("dwm_attention_f32" if q.dtype == f32 else "dwm_attention_fwd", C.byref(a))
    if keep is not None:
        keep.record_stream(torch.cuda.current_stream())


def attention_bwd(q, k, v, out, dout, dq, dk, dv, rowmap: RowMap, heads: int, lse: torch.Tensor, *,
                  q1=None, k1=None, v1=None, out1=None, dout1=None, dq1=None, dk1=None, dv1=None,
                  scale: Optional[float] = None, group_mask=None, dense_mask=None) -> None:
    """Backward of `attention` (same arguments plus the forward outputs, their gradients and lse);
    writes dq/dk/dv (and dq1/dk1/dv1), which share a row stride per segment."""
    b = _lib.AttnBwdArgs()
    keep = _attn_args(b.fwd, q, k, v, out, rowmap, heads, q1, k1, v1, out1, scale, group_mask, dense_mask)
    for name, t in (("dout", dout), ("dq", dq), ("dk", dk), ("dv", dv)):
        _chk2d(t, name)
    if dout.stride(0) != out.stride(0) or not (dq.stride(0) == dk.stride(0) == dv.stride(0)):
        raise RuntimeError("dout must be laid out like out; dq, dk, dv must share a row stride")
    b.do0, b.dq0, b.dk0, b.dv0, b.ld_d0 = dout.data_ptr(), dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), dq.stride(0)
    if q1 is not None:
        for name, t in (("dout1", dout1), ("dq1", dq1), ("dk1", dk1), ("dv1", dv1)):
            _chk2d(t, name)
        if dout1.stride(0) != out1.stride(0):
            raise RuntimeError("dout1 must be laid out like out1")
        b.do1, b.dq1, b.dk1, b.dv1, b.ld_d1 = dout1.data_ptr(), dq1.data_ptr(), dk1.data_ptr(), dv1.data_ptr(), dq1.stride(0)
    _attn_bwd_launch(b, lse)
    if keep is not None:
        keep.record_stream(torch.cuda.current_stream())


def _cross_args(a, q, k, v, out, n_problems, heads, scale):
    """fill a dwm_attn_args in `cross` mode: queries = segment 0, keys / values = segment 1, each addressed from one base"""
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _chk2d(t, name, _dt(q))
    if k.stride(0) != v.stride(0) or q.shape[0] % n_problems or k.shape[0] % n_problems:
        raise RuntimeError("cross_attention: k, v must share a row stride; rows must be n_problems * L")
    a.q0 = a.q1 = q.data_ptr()
    a.k0 = a.k1 = k.data_ptr()
    a.v0 = a.v1 = v.data_ptr()
    a.ld0, a.ld1 = q.stride(0), k.stride(0)
    a.o0, a.ldo0 = out.data_ptr(), out.stride(0)
    a.L0, a.L1, a.n_problems = q.shape[0] // n_problems, k.shape[0] // n_problems, n_problems
    _attn_problem(a, q, heads, scale, rowmap_identity(n_problems, a.L0))
    a.cross = 1


def cross_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, n_problems: int, heads: int,
                    scale: Optional[float] = None, lse: Optional[torch.Tensor] = None) -> None:
    """Cross-attention (diffusers BasicTransformerBlock.attn2): q/out [n_problems*Lq, heads*64], k/v
    [n_problems*Lk, heads*64] (column slices of one buffer sharing a row stride); every query attends to all Lk keys of
    its problem.  Runs dwm_attention_fwd in `cross` mode: queries = segment 0, keys / values = segment 1.
    lse (optional, fp32 [n_problems, heads, Lq + Lk], the query entries are written): for cross_attention_bwd."""
    a = _lib.AttnArgs()
    _cross_args(a, q, k, v, out, n_problems, heads, scale)
    _attn_lse(a, lse)
    if q.dtype == f32 and lse is not None:       # the fp32 accuracy path (UNet text cross-attention)
        raise NotImplementedError("cross_attention: no LSE output on the fp32 path (inference only)")
    _call("dwm_attention_f32" if q.dtype == f32 else "dwm_attention_fwd", C.byref(a))


def cross_attention_bwd(q, k, v, out, dout, dq, dk, dv, n_problems: int, heads: int, lse: torch.Tensor,
                        scale: Optional[float] = None) -> None:
    """Backward of `cross_attention`: dq like q (row stride of its own), dk / dv like k / v (sharing a row stride)."""
    b = _lib.AttnBwdArgs()
    _cross_args(b.fwd, q, k, v, out, n_problems, heads, scale)
    for name, t in (("dout", dout), ("dq", dq), ("dk", dk), ("dv", dv)):
        _chk2d(t, name)
    if dout.stride(0) != out.stride(0) or dk.stride(0) != dv.stride(0) or dq.shape != q.shape or dk.shape != k.shape:
        raise RuntimeError("cross_attention_bwd: dout like out, dq like q, dk / dv like k / v (one row stride)")
    # one gradient base per tensor for both segments (the kernels address segment 1 relative to segment 0, cf. the forward)
    b.do0 = b.do1 = dout.data_ptr()
    b.dq0 = b.dq1 = dq.data_ptr()
    b.dk0 = b.dk1 = dk.data_ptr()
    b.dv0 = b.dv1 = dv.data_ptr()
    b.ld_d0, b.ld_d1 = dq.stride(0), dk.stride(0)
    _attn_bwd_launch(b, lse)


# -------------------------------------------------------------------------------- norms
# entry point -> dtype of (x, xsum, everything else: out / out2, weight / bias, the modulation matrices, addvec)
_LAYERNORM_FORMS = {"dwm_layernorm": (bf16, bf16, bf16), "dwm_layernorm_f32": (f32, f32, f32), "dwm_layernorm_x32": (f32, f32, bf16)}


def layernorm(x: torch.Tensor, *, eps: float, out: Optional[torch.Tensor] = None,
              weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
              scale: Optional[torch.Tensor] = None, shift: Optional[torch.Tensor] = None,
              rows_per_mod: int = 0,
              scale2: Optional[torch.Tensor] = None, shift2: Optional[torch.Tensor] = None,
              out2: Optional[torch.Tensor] = None,
              addvec: Optional[torch.Tensor] = None, rows_per_add: int = 0,
              xsum: Optional[torch.Tensor] = None, x32: bool = False):
    """See dwm_layernorm.  scale/shift (and scale2/shift2) are 2-D views sharing one row
    stride (column slices of the AdaLN modulation matrix).  x32: x (and xsum) are the fp32 residual stream of the bf16
    forward, everything else bf16 (dwm_layernorm_x32); otherwise fp32 x: the accuracy path (dwm_layernorm_f32)."""
    fn = "dwm_layernorm_x32" if x32 else "dwm_layernorm_f32" if x.dtype == f32 else "dwm_layernorm"
    xdt, sumdt, dt = _LAYERNORM_FORMS[fn]
    _chk2d(x, "x", xdt)
    rows, D = x.shape
    if out is None:
        out = torch.empty((rows, D), dtype=dt, device=x.device)
    _chk2d(out, "out", dt)
    a = _lib.LayerNormArgs()
    a.x, a.ldx, a.y, a.ldy = x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0)
    a.rows, a.D, a.eps = rows, D, eps
    _chkvec(weight, "weight", dt)
    _chkvec(bias, "bias", dt)
    a.weight, a.bias = _p(weight), _p(bias)
    if scale is not None:
        _chk2d(scale, "scale", dt)
        _chk2d(shift, "shift", dt)
        if scale.stride(0) != shift.stride(0):
            raise RuntimeError("scale/shift must share a row stride")
        a.scale, a.shift, a.ld_mod, a.rows_per_mod = scale.data_ptr(), shift.data_ptr(), scale.stride(0), rows_per_mod
    if out2 is not None:
        _chk2d(out2, "out2", dt)
        _chk2d(scale2, "scale2", dt)
        _chk2d(shift2, "shift2", dt)
        if scale2.stride(0) != a.ld_mod or shift2.stride(0) != a.ld_mod:
            raise RuntimeError("scale2/shift2 must share the row stride of scale/shift")
        a.y2, a.ldy2, a.scale2, a.shift2 = out2.data_ptr(), out2.stride(0), scale2.data_ptr(), shift2.data_ptr()
    if addvec is not None:
        _chk2d(addvec, "addvec", dt)
        a.addvec, a.ld_add, a.rows_per_add = addvec.data_ptr(), addvec.stride(0), rows_per_add
        if xsum is not None:
            _chk2d(xsum, "xsum", sumdt)
            a.xsum, a.ldxsum = xsum.data_ptr(), xsum.stride(0)
    _call(fn, C.byref(a))
    return out


def rmsnorm_heads_(x: torch.Tensor, w_expanded: torch.Tensor, eps: float) -> torch.Tensor:
    """In-place per-64-wide-head RMSNorm of x[rows, ncols]; w_expanded [ncols]."""
    _chk2d(x, "x")
    _chkvec(w_expanded, "w")
    _call("dwm_rmsnorm_heads", x.data_ptr(), x.stride(0), x.shape[0], x.shape[1], w_expanded.data_ptr(), eps)
    return x


# -------------------------------------------------------------------------- elementwise
def silu(x: torch.Tensor) -> torch.Tensor:
    _chkvec(x, "x", _dt(x))
    y = torch.empty_like(x)
    _call("dwm_silu_f32" if x.dtype == f32 else "dwm_silu", x.data_ptr(), y.data_ptr(), x.numel())
    return y


def timestep_sinusoid(t: torch.Tensor, channels: int, dtype: torch.dtype = bf16) -> torch.Tensor:
    """diffusers Timesteps(channels, flip_sin_to_cos=True, downscale_freq_shift=0) -> [n, channels] bf16 (or fp32: the accuracy path)."""
    t = t.reshape(-1).to(f32).contiguous()
    if not t.is_cuda:
        raise RuntimeError("timestep_sinusoid: expected a device tensor")
    out = torch.empty((t.numel(), channels), dtype=f32 if dtype == f32 else bf16, device=t.device)
    _call("dwm_timestep_sinusoid_f32" if dtype == f32 else "dwm_timestep_sinusoid", t.data_ptr(), t.numel(), channels, out.data_ptr())
    return out


def _image_token_rows(what: str, x: torch.Tensor, p: int, ldo: Optional[int], dtype: torch.dtype):
    """patchify / unshuffle_tokens: check the [I, C, H, W] image, allocate the [I*(H/p)*(W/p), ldo] token rows -> (out, ldo)"""
    if not x.is_cuda or x.dim() != 4 or not x.is_contiguous() or x.dtype not in (f32, bf16):
        raise RuntimeError(f"{what}: expected a contiguous fp32/bf16 [I,C,H,W] device tensor")
    I, Cc, H, W = x.shape
    ldo = ldo or (Cc * p * p + 63) // 64 * 64
    if dtype == f32 and x.dtype != f32:
        raise RuntimeError(f"{what}: the fp32 form takes fp32 images")
    return torch.empty((I * (H // p) * (W // p), ldo), dtype=f32 if dtype == f32 else bf16, device=x.device), ldo


def patchify(x: torch.Tensor, p: int, ldo: Optional[int] = None, dtype: torch.dtype = bf16) -> torch.Tensor:
    """[I, C, H, W] (fp32 / bf16) -> [I*(H/p)*(W/p), ldo] im2col rows (zero padded to ldo), bf16 (or fp32: the accuracy path)."""
    out, ldo = _image_token_rows("patchify", x, p, ldo, dtype)
    if dtype == f32:
        _call("dwm_patchify_f32", x.data_ptr(), *x.shape, p, out.data_ptr(), ldo)
    else:                                   # the bf16 entry point takes either image dtype, as a flag
        _call("dwm_patchify", x.data_ptr(), int(x.dtype == f32), *x.shape, p, out.data_ptr(), ldo)
    return out


def unpatchify(x: torch.Tensor, I: int, Cc: int, h: int, w: int, p: int) -> torch.Tensor:
    dt = _dt(x)
    _chk2d(x, "x", dt)
    out = torch.empty((I, Cc, h * p, w * p), dtype=dt, device=x.device)
    _call("dwm_unpatchify_f32" if dt == f32 else "dwm_unpatchify", x.data_ptr(), x.stride(0), I, Cc, h, w, p, out.data_ptr())
    return out


def cfg_euler_step(pred: torch.Tensor, latents: torch.Tensor, guidance: float, dsigma,
                   model_in: Optional[torch.Tensor] = None, group_elems: int = 0) -> None:
    """latents(fp32, in place) += dsigma * (u + g (c - u)) with pred = [uncond; cond] bf16 (fp32 pred + fp32 model_in: the
    accuracy path).  dsigma: a number, or per-frame steps [n / group_elems] fp32 (diffusion forcing)."""
    n = latents.numel()
    dt = _dt(pred)
    if pred.dtype != dt or pred.numel() != 2 * n or not pred.is_contiguous() or not pred.is_cuda:
        raise RuntimeError("cfg_euler_step: pred must be contiguous bf16 (fp32: the accuracy path) with 2x the latent elements")
    # known asymmetry, kept as it was: the fp32 form never checked that latents is a device tensor
    if latents.dtype != f32 or not latents.is_contiguous() or (dt == bf16 and not latents.is_cuda):
        raise RuntimeError("cfg_euler_step: latents must be contiguous fp32")
    if model_in is not None and (model_in.dtype != dt or model_in.numel() != 2 * n or not model_in.is_contiguous()):
        raise RuntimeError("cfg_euler_step: model_in must be contiguous [2, n] of pred's dtype")
    grouped = torch.is_tensor(dsigma)
    if grouped and (dsigma.dtype != f32 or not dsigma.is_cuda or not dsigma.is_contiguous() or dsigma.numel() * group_elems != n):
        raise RuntimeError("cfg_euler_step: dsigma must be a contiguous fp32 device tensor with n / group_elems entries")
    head = (pred.data_ptr(), latents.data_ptr(), _p(model_in), n, float(guidance))
    if dt == f32:                           # one entry point for both kinds of step: the scalar, then the (nullable) table
        _call("dwm_cfg_euler_step_f32", *head, 0.0 if grouped else float(dsigma), dsigma.data_ptr() if grouped else None, group_elems)
    elif grouped:
        _call("dwm_cfg_euler_step_grouped", *head, dsigma.data_ptr(), group_elems)
    else:
        _call("dwm_cfg_euler_step", *head, float(dsigma))


def cfg_multistep(pred: torch.Tensor, latents: torch.Tensor, x0_prev: torch.Tensor, guidance: float, kx: float, ko: float,
                  A: float, B: float, Cc: float, model_in: Optional[torch.Tensor] = None) -> None:
    """CFG combine + linear multistep scheduler update (see dwm_cfg_multistep); latents / x0_prev fp32 in place."""
    n = latents.numel()
    if pred.dtype not in (bf16, f32) or pred.numel() != 2 * n or not pred.is_contiguous() or not pred.is_cuda:
        raise RuntimeError("cfg_multistep: pred must be contiguous bf16 (fp32: the accuracy path) with 2x the latent elements")
    for t in (latents, x0_prev):
        if t.dtype != f32 or not t.is_contiguous() or t.numel() != n:
            raise RuntimeError("cfg_multistep: latents / x0_prev must be contiguous fp32 of the same size")
    if model_in is not None and (model_in.dtype != pred.dtype or model_in.numel() != 2 * n or not model_in.is_contiguous()):
        raise RuntimeError("cfg_multistep: model_in must be contiguous, of pred's dtype and size")
    _call("dwm_cfg_multistep_f32" if pred.dtype == f32 else "dwm_cfg_multistep", pred.data_ptr(), latents.data_ptr(),
          x0_prev.data_ptr(), _p(model_in), n, float(guidance), float(kx), float(ko), float(A), float(B), float(Cc))


def cfg_multistep_grouped(pred: torch.Tensor, latents: torch.Tensor, x0_prev: torch.Tensor, guidance: float, coef: torch.Tensor,
                          group_elems: int, keep_model_in: Optional[torch.Tensor] = None,
                          model_in: Optional[torch.Tensor] = None) -> None:
    """cfg_multistep with the (kx, ko, A, B, C) rows in device memory: coef fp32 [n / group_elems, 5], or [1, 5] for every
    group; keep_model_in int32 [n / group_elems]: groups (reference frames) whose model_in entries stay as they are.  See
    dwm_cfg_multistep_grouped."""
    n = latents.numel()
    if pred.dtype not in (bf16, f32) or pred.numel() != 2 * n or not pred.is_contiguous() or not pred.is_cuda:
        raise RuntimeError("cfg_multistep_grouped: pred must be contiguous bf16 (fp32: the accuracy path) with 2x the latent elements")
    for t in (latents, x0_prev):
        if t.dtype != f32 or not t.is_contiguous() or t.numel() != n or not t.is_cuda:
            raise RuntimeError("cfg_multistep_grouped: latents / x0_prev must be contiguous fp32 device tensors of the same size")
    if group_elems <= 0 or group_elems % 4 != 0 or n % group_elems != 0:
        raise RuntimeError(f"cfg_multistep_grouped: group_elems {group_elems} must be a multiple of 4 that divides the {n} latent elements")
    groups = n // group_elems
    if coef.dtype != f32 or not coef.is_contiguous() or not coef.is_cuda or coef.numel() not in (5, 5 * groups):
        raise RuntimeError("cfg_multistep_grouped: coef must be a contiguous fp32 device tensor [n / group_elems, 5] or [1, 5]")
    if keep_model_in is not None and (keep_model_in.dtype != torch.int32 or not keep_model_in.is_contiguous() or
                                      not keep_model_in.is_cuda or keep_model_in.numel() != groups):
        raise RuntimeError("cfg_multistep_grouped: keep_model_in must be a contiguous int32 device tensor [n / group_elems]")
    if model_in is not None and (model_in.dtype != pred.dtype or model_in.numel() != 2 * n or not model_in.is_contiguous()):
        raise RuntimeError("cfg_multistep_grouped: model_in must be contiguous, of pred's dtype and size")
    _call("dwm_cfg_multistep_grouped_f32" if pred.dtype == f32 else "dwm_cfg_multistep_grouped", pred.data_ptr(), latents.data_ptr(),
          x0_prev.data_ptr(), _p(model_in), n, float(guidance), coef.data_ptr(), coef.numel() // 5, _p(keep_model_in), group_elems)


def ray_features(cam: torch.Tensor, h: int, w: int, ldo: int = 128, dtype: torch.dtype = bf16) -> torch.Tensor:
    """cam fp32 [I, 21] (see dwm_ray_features) -> bf16 (or, the fp32 accuracy path, fp32) [I*h*w, ldo]: RayEncoder's 72
    positional-encoding inputs per token."""
    if cam.dtype != f32 or cam.dim() != 2 or cam.shape[1] != 21 or not cam.is_contiguous() or not cam.is_cuda:
        raise RuntimeError("ray_features: cam must be a contiguous fp32 device tensor [I, 21]")
    if dtype not in (bf16, f32):
        raise RuntimeError("ray_features: bf16 or fp32 output")
    out = torch.empty((cam.shape[0] * h * w, ldo), dtype=dtype, device=cam.device)
    _call("dwm_ray_features_f32" if dtype == f32 else "dwm_ray_features", cam.data_ptr(), cam.shape[0], h, w, out.data_ptr(), ldo)
    return out


def frame_affine(x: torch.Tensor, y: torch.Tensor, coef: torch.Tensor, group_elems: int, out: Optional[torch.Tensor] = None,
                 out_bf16: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = coef[g, 0] * x + coef[g, 1] * y (fp32), g = element // group_elems; see dwm_frame_affine."""
    n = x.numel()
    for t in (x, y):
        if t.dtype != f32 or not t.is_contiguous() or not t.is_cuda or t.numel() != n:
            raise RuntimeError("frame_affine: x / y must be contiguous fp32 device tensors of one size")
    if coef.dtype != f32 or not coef.is_contiguous() or not coef.is_cuda or coef.numel() * group_elems != 2 * n:
        raise RuntimeError("frame_affine: coef must be a contiguous fp32 device tensor [n / group_elems, 2]")
    if out is None and out_bf16 is None:
        out = torch.empty_like(x)
    _call("dwm_frame_affine", x.data_ptr(), y.data_ptr(), coef.data_ptr(), _p(out), _p(out_bf16), n, group_elems)
    return out if out is not None else out_bf16


def cfg_ddim_step(pred: torch.Tensor, latents: torch.Tensor, coef: torch.Tensor, group_elems: int, prediction_type: int,
                  guidance: Optional[float] = None, clip_range: float = 0.0, use_clipped_model_output: bool = False,
                  noise: Optional[torch.Tensor] = None, x0_out: Optional[torch.Tensor] = None,
                  model_in: Optional[torch.Tensor] = None, skip: Optional[torch.Tensor] = None) -> None:
    """[CFG combine +] tensor-timestep DDIM update of `latents` (fp32, in place); see dwm_cfg_ddim_step.
    guidance None: pred holds n elements; otherwise pred = [uncond; cond] with 2n.
    skip: int32 [n / group_elems] - groups with a flag != 0 keep latents / x0_out / model_in bit-unchanged
    (dwm_cfg_ddim_step_masked); None: every group is updated, through the entry point this wrapper always called."""
    n = latents.numel()
    cfg = guidance is not None
    if pred.dtype not in (bf16, f32) or pred.numel() != (2 * n if cfg else n) or not pred.is_contiguous() or not pred.is_cuda:
        raise RuntimeError("cfg_ddim_step: pred must be a contiguous bf16 / fp32 device tensor with n (2n with guidance) elements")
    for t in (latents, noise, x0_out):
        if t is not None and (t.dtype != f32 or not t.is_contiguous() or t.numel() != n or not t.is_cuda):
            raise RuntimeError("cfg_ddim_step: latents / noise / x0_out must be contiguous fp32 device tensors of one size")
    if coef.dtype != f32 or not coef.is_contiguous() or not coef.is_cuda or coef.numel() * group_elems != 6 * n:
        raise RuntimeError("cfg_ddim_step: coef must be a contiguous fp32 device tensor [n / group_elems, 6]")
    if model_in is not None and (model_in.dtype != bf16 or model_in.numel() != (2 * n if cfg else n) or not model_in.is_contiguous()):
        raise RuntimeError("cfg_ddim_step: model_in must be contiguous bf16")
    args = (pred.data_ptr(), int(pred.dtype == f32), int(cfg), latents.data_ptr(), _p(model_in), _p(x0_out), _p(noise), coef.data_ptr(),
            n, group_elems, float(guidance or 0.0), int(prediction_type), float(clip_range), int(bool(use_clipped_model_output)))
    if skip is None:
        _call("dwm_cfg_ddim_step", *args)
        return
    if skip.dtype != torch.int32 or not skip.is_contiguous() or not skip.is_cuda or skip.numel() * group_elems != n:
        raise RuntimeError("cfg_ddim_step: skip must be a contiguous int32 device tensor [n / group_elems]")
    _call("dwm_cfg_ddim_step_masked", *args, skip.data_ptr())


def unshuffle_tokens(x: torch.Tensor, r: int, ldo: Optional[int] = None, dtype: torch.dtype = bf16) -> torch.Tensor:
    """PixelUnshuffle(r): [I, C, H, W] (fp32 / bf16) -> token-major [I*(H/r)*(W/r), ldo], bf16 or (dtype=torch.float32, fp32
    input: the accuracy path) fp32; columns past C r r are zero."""
    out, ldo = _image_token_rows("unshuffle_tokens", x, r, ldo, dtype)
    if dtype == f32:
        _call("dwm_unshuffle_tokens_f32", x.data_ptr(), *x.shape, r, out.data_ptr(), ldo)
    else:                                   # the bf16 entry point takes either image dtype, as a flag
        _call("dwm_unshuffle_tokens", x.data_ptr(), int(x.dtype == f32), *x.shape, r, out.data_ptr(), ldo)
    return out


def avgpool2_tokens(x: torch.Tensor, I: int, h: int, w: int) -> torch.Tensor:
    """AvgPool2d(2) on token-major [I*h*w, C] -> [I*(h/2)*(w/2), C]."""
    dt = _dt(x)
    _chk2d(x, "x", dt)
    if not x.is_contiguous() or x.shape[0] != I * h * w:
        raise RuntimeError("avgpool2_tokens: x must be contiguous [I*h*w, C]")
    out = torch.empty((I * (h // 2) * (w // 2), x.shape[1]), dtype=dt, device=x.device)
    _call("dwm_avgpool2_tokens_f32" if dt == f32 else "dwm_avgpool2_tokens", x.data_ptr(), I, h, w, x.shape[1], out.data_ptr())
    return out


def add_(y: torch.Tensor, x: torch.Tensor) -> torch.Tensor:
    """y += x (contiguous device tensors of one shape).  y bf16: x bf16, or fp32 (the fp32 sum is rounded once).  y fp32 (the
    fp32 residual stream): x fp32 or bf16."""
    if y.shape != x.shape or y.dtype not in (bf16, f32) or x.dtype not in (bf16, f32) \
            or not y.is_contiguous() or not x.is_contiguous() or not y.is_cuda:
        raise RuntimeError("add_: expected contiguous device tensors of one shape (bf16 / fp32)")
    if y.dtype == f32 and x.dtype == bf16:
        cast_f32(x, out=y, accumulate=True)
    elif y.dtype == f32:
        _call("dwm_add_f32_f32_inplace", y.data_ptr(), x.data_ptr(), y.numel())
    else:
        _call("dwm_add_f32_inplace" if x.dtype == f32 else "dwm_add_inplace", y.data_ptr(), x.data_ptr(), y.numel())
    return y


def _gn_maps(grid, img_map: Optional[tuple]):
    """the (dwm_rowmap2d, dwm_gn_imgmap) pair of the group-norm entry points, forward and backward: the padded grid of the
    normalised-side matrix (or none) and the image / pixel -> token row map (iv, pn, s_ihi, s_ilo, s_phi) (or none)"""
    m = _lib.RowMap2D()
    if grid is not None:
        grid.fill(m)
    im = _lib.GnImgMap()
    if img_map is not None:
        im.iv, im.pn, im.s_ihi, im.s_ilo, im.s_phi = img_map
    return m, im


def groupnorm_silu(x: torch.Tensor, I: int, P: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                   eps: float, silu: bool = True, out: Optional[torch.Tensor] = None,
                   out_grid=None, img_map: Optional[tuple] = None, zmap: Optional[dict] = None) -> torch.Tensor:
    """GroupNorm(groups) [+ SiLU] of token-major x [I*P, C]; with out_grid the result lands in the
    interior of a padded grid `out` [out_grid.rows, C] whose border must already be zero.  img_map =
    (iv, pn, s_ihi, s_ilo, s_phi): image i / pixel p -> token row (see dwm_groupnorm_silu_mapped).
    zmap = dict(mod [z rows, 2C], frames, videos, h, w, shift, zt): CogVideoXSpatialNorm3D (dwm_groupnorm_spatial)."""
    dt = _dt(x)                                                        # fp32: the accuracy path (dwm_groupnorm_silu_f32)
    _chk2d(x, "x", dt)
    if not x.is_contiguous() or x.shape[0] != I * P:
        raise RuntimeError("groupnorm_silu: x must be contiguous [I*P, C]")
    Cc = x.shape[1]
    _chkvec(gamma, "gamma", dt)
    _chkvec(beta, "beta", dt)
    rows = out_grid.rows if out_grid is not None else I * P
    if out is None:
        out = (torch.zeros if out_grid is not None else torch.empty)((rows, Cc), dtype=dt, device=x.device)
    if out.shape != (rows, Cc) or not out.is_contiguous() or out.dtype != dt:
        raise RuntimeError("groupnorm_silu: bad out")
    stats = torch.empty(_lib.load().dwm_groupnorm_stats_floats(I, P, groups), dtype=f32, device=x.device)
    m, im = _gn_maps(out_grid, img_map)
    head = (x.data_ptr(), out.data_ptr(), I, P, Cc, groups, eps, gamma.data_ptr(), beta.data_ptr(), int(silu), stats.data_ptr(),
            C.byref(m), C.byref(im))
    if zmap is None:
        _call("dwm_groupnorm_silu_f32" if dt == f32 else "dwm_groupnorm_silu_mapped", *head)
        return out
    mod = zmap["mod"]
    _chk2d(mod, "zmap.mod", dt)
    zm = _lib.GnZMap()
    zm.mod, zm.ld_mod = mod.data_ptr(), mod.stride(0)
    zm.frames, zm.videos, zm.h, zm.w, zm.shift = zmap["frames"], zmap["videos"], zmap["h"], zmap["w"], zmap["shift"]
    for t, z in enumerate(zmap["zt"]):
        zm.zt[t] = z
    need = ((max(zmap["zt"]) + 1) * zmap["videos"]) * (zmap["h"] >> zmap["shift"]) * (zmap["w"] >> zmap["shift"])
    if mod.shape[0] < need or mod.shape[1] < 2 * Cc:
        raise RuntimeError("groupnorm_silu: zmap.mod is smaller than the latent grid it is indexed with")
    _call("dwm_groupnorm_spatial_f32" if dt == f32 else "dwm_groupnorm_spatial", *head, C.byref(zm))
    return out


def frame_mix(x: torch.Tensor, frame_elems: int, f0, f1, w0, w1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out frame j = w0[j] * x[f0[j]] + w1[j] * x[f1[j]] over frames of `frame_elems` contiguous bf16 elements of the
    flat tensor x (temporal average pooling / temporal nearest upsampling of the CogVideoX VAE)."""
    n = len(f0)
    dt = x.dtype
    if dt not in (bf16, f32) or not x.is_cuda or not x.is_contiguous() or x.numel() % frame_elems != 0:
        raise RuntimeError("frame_mix: x must be a contiguous bf16 (or, the fp32 accuracy path, fp32) device tensor of whole frames")
    nin = x.numel() // frame_elems
    if not (len(f1) == len(w0) == len(w1) == n) or n == 0 or n > 64 or max(max(f0), max(f1)) >= nin:
        raise RuntimeError("frame_mix: bad frame tables")
    if out is None:
        out = torch.empty(n * frame_elems, dtype=dt, device=x.device)
    if out.numel() != n * frame_elems or out.dtype != dt or not out.is_contiguous():
        raise RuntimeError("frame_mix: bad out")
    fm = _lib.FrameMix()
    fm.n_out = n
    for j in range(n):
        fm.f0[j], fm.f1[j], fm.w0[j], fm.w1[j] = f0[j], f1[j], w0[j], w1[j]
    _call("dwm_frame_mix_f32" if dt == f32 else "dwm_frame_mix_bf16", x.data_ptr(), out.data_ptr(), frame_elems, C.byref(fm))
    return out


def upsample2_padded(x: torch.Tensor, I: int, h: int, w: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """nearest 2x upsample of token-major [I*h*w, C] into the padded grid of the [I, 2h, 2w] image."""
    dt = _dt(x)
    _chk2d(x, "x", dt)
    if not x.is_contiguous() or x.shape[0] != I * h * w:
        raise RuntimeError("upsample2_padded: x must be contiguous [I*h*w, C]")
    g = PaddedGrid(I, 2 * h, 2 * w)
    if out is None:
        out = torch.zeros((g.rows, x.shape[1]), dtype=dt, device=x.device)
    _chk2d(out, "out", dt)
    _call("dwm_upsample2_padded_f32" if dt == f32 else "dwm_upsample2_padded", x.data_ptr(), out.data_ptr(), I, h, w, x.shape[1])
    return out


def pad_tokens(x: torch.Tensor, grid: PaddedGrid, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """compact token rows [grid.pixels, C] -> interior of a zero-bordered padded grid [grid.rows, C]."""
    dt = _dt(x)
    _chk2d(x, "x", dt)
    if not x.is_contiguous() or x.shape[0] != grid.pixels:
        raise RuntimeError("pad_tokens: x must be contiguous [grid.pixels, C]")
    if out is None:
        out = torch.zeros((grid.rows, x.shape[1]), dtype=dt, device=x.device)
    _chk2d(out, "out", dt)
    m = _lib.RowMap2D()
    grid.fill(m)
    _call("dwm_pad_tokens_f32" if dt == f32 else "dwm_pad_tokens", x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], C.byref(m))
    return out


def softmax_rows(x: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dt = _dt(x)
    _chk2d(x, "x", dt)
    out = torch.empty_like(x) if out is None else out
    _chk2d(out, "out", dt)
    _call("dwm_softmax_rows_f32" if dt == f32 else "dwm_softmax_rows", x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], x.stride(0),
          float(scale))
    return out


VAE_ATTENTION_CHANNELS = (128, 256, 512)       # head dimensions dwm_vae_attention is instantiated for


def vae_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, I: int, P: int, scale: float) -> torch.Tensor:
    """Single-head attention over I images of P pixels (the VAE mid block): out[i] = softmax(scale * q[i] k[i]^T) v[i], one launch,
    no P x P matrix in memory, any P >= 1.  q, k, v, out: 2-D [I*P, C] with contiguous rows, all bf16 or all fp32 (the accuracy
    path); q, k, v may be column blocks of one [I*P, 3C] buffer.  C in VAE_ATTENTION_CHANNELS."""
    dt = _dt(q)
    if any(t.dtype != dt for t in (q, k, v, out)):
        raise RuntimeError(f"vae_attention: q, k, v, out must all be bf16 or all fp32, got {[str(t.dtype) for t in (q, k, v, out)]}")
    if I <= 0 or P <= 0:
        raise RuntimeError(f"vae_attention: I and P must be positive, got I={I} P={P}")
    Cc = q.shape[-1]
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        if tuple(t.shape) != (I * P, Cc):
            raise RuntimeError(f"vae_attention: {name} must be [I*P, C] = [{I * P}, {Cc}], got {tuple(t.shape)}")
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _chk2d(t, name, dt)
    if Cc not in VAE_ATTENTION_CHANNELS:
        raise RuntimeError(f"vae_attention: head dimension {Cc} is not one of {VAE_ATTENTION_CHANNELS}")
    if any(_overlaps(out, t) for t in (q, k, v)):
        raise RuntimeError("vae_attention: out must not overlap q, k or v")
    a = _lib.VaeAttnArgs()
    a.q, a.k, a.v, a.out = q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr()
    a.ldq, a.ldk, a.ldv, a.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    a.I, a.P, a.C, a.scale = I, P, Cc, float(scale)
    _call("dwm_vae_attention_f32" if dt == f32 else "dwm_vae_attention", C.byref(a))
    return out


# ------------------------------------------------------------------------ text encoders
TEXT_ATTENTION_MAX_L = 128                       # a row's scores stay in registers (dwm_text_attention)
TEXT_ACT_KINDS = {"quick_gelu": 0, "gelu": 1, "gelu_new": 2, "gelu_pytorch_tanh": 2}


def text_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, n_seq: int, L: int, heads: int, scale: float,
                   causal: bool = False, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = softmax(scale q k^T [+ bias] [causal]) v for n_seq sequences of L tokens, `heads` heads of width 64 (dwm_text_attention).
    q, k, v: bf16 [n_seq*L, heads*64] with contiguous rows and ONE row stride (column blocks of a fused QKV buffer); bias: fp32
    [heads, L, L] or None.  L outside 1..TEXT_ATTENTION_MAX_L or another head width: NotImplementedError.
    fp32 q: the accuracy path (dwm_text_attention_f32) - k, v and out fp32 too, exact fp32 contractions."""
    dt = _dt(q)
    if not 1 <= L <= TEXT_ATTENTION_MAX_L:
        raise NotImplementedError(f"text_attention: L = {L} is outside 1..{TEXT_ATTENTION_MAX_L}")
    if heads <= 0 or q.shape[-1] != heads * 64:
        raise NotImplementedError(f"text_attention: head width {q.shape[-1]} / {heads} is not 64")
    if n_seq <= 0:
        raise RuntimeError(f"text_attention: n_seq must be positive, got {n_seq}")
    for name, t in (("q", q), ("k", k), ("v", v), ("out", out)):
        _chk2d(t, name, dt)
        if tuple(t.shape) != (n_seq * L, heads * 64):
            raise RuntimeError(f"text_attention: {name} must be [n_seq*L, heads*64] = [{n_seq * L}, {heads * 64}], got {tuple(t.shape)}")
    if not (q.stride(0) == k.stride(0) == v.stride(0)):
        raise RuntimeError("text_attention: q, k, v must share a row stride")
    if any(_overlaps(out, t) for t in (q, k, v)):
        raise RuntimeError("text_attention: out must not overlap q, k or v")
    _chkvec(bias, "bias", f32)
    if bias is not None and tuple(bias.shape) != (heads, L, L):
        raise RuntimeError(f"text_attention: bias must be [heads, L, L] = [{heads}, {L}, {L}], got {tuple(bias.shape)}")
    a = _lib.TextAttnArgs()
    a.q, a.k, a.v, a.ld, a.out, a.ldo = q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), out.data_ptr(), out.stride(0)
    a.n_seq, a.L, a.heads, a.scale, a.causal, a.bias = n_seq, L, heads, float(scale), int(bool(causal)), _p(bias)
    _call("dwm_text_attention_f32" if dt == f32 else "dwm_text_attention", C.byref(a))
    return out


def rmsnorm_rows(x: torch.Tensor, weight: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """T5LayerNorm of the fp32 residual stream x [rows, D] -> bf16 (dwm_rmsnorm_rows): x rsqrt(mean(x^2) + eps) weight.
    fp32 weight: the accuracy path (dwm_rmsnorm_rows_f32), fp32 out"""
    dt = _dt(weight)
    _chk2d(x, "x", f32)
    _chkvec(weight, "weight", dt)
    rows, D = x.shape
    if weight.numel() != D:
        raise RuntimeError(f"rmsnorm_rows: weight must have {D} elements, got {weight.numel()}")
    if D % 8 != 0 or D > 8192:
        raise NotImplementedError(f"rmsnorm_rows: D = {D} must be a multiple of 8, at most 8192")
    if out is None:
        out = torch.empty((rows, D), dtype=dt, device=x.device)
    _chk2d(out, "out", dt)
    if out.shape != x.shape:
        raise RuntimeError("rmsnorm_rows: out must have the shape of x")
    _call("dwm_rmsnorm_rows_f32" if dt == f32 else "dwm_rmsnorm_rows", x.data_ptr(), x.stride(0), rows, D, weight.data_ptr(), float(eps),
          out.data_ptr(), out.stride(0))
    return out


def text_embed(ids: torch.Tensor, table: torch.Tensor, pos: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 stream [n_seq*L, D] = table[ids] (+ pos[position]) for ids [n_seq, L] int64 (dwm_text_embed).  Ids that arrive on the
    host - the normal case: the tokenizer runs there - are checked against the vocabulary here; ids already on the device are
    clamped by the kernel instead (checking them would cost a synchronisation).  fp32 table (and pos): dwm_text_embed_f32."""
    if ids.dim() != 2 or ids.dtype != torch.int64:
        raise RuntimeError(f"text_embed: ids must be a 2-D int64 tensor, got {tuple(ids.shape)} {ids.dtype}")
    if table.dim() != 2 or ids.numel() == 0:
        raise RuntimeError(f"text_embed: expected a 2-D table and at least one id, got {tuple(table.shape)}, {tuple(ids.shape)}")
    vocab, D = table.shape
    n_seq, L = ids.shape
    if not ids.is_cuda and (int(ids.min()) < 0 or int(ids.max()) >= vocab):
        raise ValueError(f"text_embed: token ids outside [0, {vocab}): min {int(ids.min())}, max {int(ids.max())}")
    dt = _dt(table)
    _chk2d(table, "table", dt)
    ids = ids.to(table.device)
    if not table.is_contiguous() or D % 8 != 0:
        raise RuntimeError("text_embed: the table must be contiguous with D % 8 == 0")
    if pos is not None:
        _chk2d(pos, "pos", dt)
        if not pos.is_contiguous() or pos.shape[1] != D or pos.shape[0] < L:
            raise RuntimeError(f"text_embed: pos must be a contiguous [>= {L}, {D}] table, got {tuple(pos.shape)}")
    ids = ids.contiguous()
    if out is None:
        out = torch.empty((n_seq * L, D), dtype=f32, device=table.device)
    _chk2d(out, "out", f32)
    if tuple(out.shape) != (n_seq * L, D):
        raise RuntimeError("text_embed: out must be [n_seq*L, D]")
    _call("dwm_text_embed_f32" if dt == f32 else "dwm_text_embed", ids.data_ptr(), n_seq * L, table.data_ptr(), vocab, D, _p(pos), L, out.data_ptr(), out.stride(0))
    return out


def text_act(x: torch.Tensor, kind: str, gated: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """act(x) (x [rows, F]) or act(x[:, :F]) * x[:, F:] (gated, x [rows, 2F]) on bf16, computed in fp32 (dwm_text_act);
    kind: a key of TEXT_ACT_KINDS (the transformers activation names).  fp32 x: the accuracy path (dwm_text_act_f32), fp32 out,
    the library's exp / erfc instead of the hardware approximations"""
    if kind not in TEXT_ACT_KINDS:
        raise NotImplementedError(f"text_act: activation {kind!r} is not one of {sorted(TEXT_ACT_KINDS)}")
    dt = _dt(x)
    _chk2d(x, "x", dt)
    rows, cols = x.shape
    F = cols // 2 if gated else cols
    if (gated and cols % 2) or F % 8 != 0:
        raise RuntimeError(f"text_act: {cols} columns do not make {'2 x ' if gated else ''}F with F % 8 == 0")
    if out is None:
        out = torch.empty((rows, F), dtype=dt, device=x.device)
    _chk2d(out, "out", dt)
    if tuple(out.shape) != (rows, F):
        raise RuntimeError("text_act: out must be [rows, F]")
    _call("dwm_text_act_f32" if dt == f32 else "dwm_text_act", x.data_ptr(), x.stride(0), rows, F, TEXT_ACT_KINDS[kind], int(bool(gated)), out.data_ptr(), out.stride(0))
    return out


# -------------------------------------------------------------------- NF4 4-bit weights
def _nf4_operands(q: torch.Tensor, absmax: torch.Tensor, what: str):
    """checks of a packed weight (nf4.py): q uint8 [N, K/2], absmax fp32 [N, K/64], both contiguous on one device -> (N, K)"""
    from . import nf4
    for name, t, dt in (("q", q, torch.uint8), ("absmax", absmax, f32)):
        if not t.is_cuda or t.dtype != dt or t.dim() != 2 or not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be a contiguous 2-D {dt} device tensor")
    N, K = q.shape[0], 2 * q.shape[1]
    if N == 0 or K == 0 or K % nf4.BLOCK != 0 or tuple(absmax.shape) != (N, K // nf4.BLOCK) or absmax.device != q.device:
        raise RuntimeError(f"{what}: q {tuple(q.shape)} and absmax {tuple(absmax.shape)} are not [N, K/2] and [N, K/{nf4.BLOCK}] of one weight")
    if q.data_ptr() % 16 != 0 or absmax.data_ptr() % 4 != 0:
        raise RuntimeError(f"{what}: q must be 16-byte aligned, absmax 4-byte aligned")
    return N, K


def _chk_aligned(t: torch.Tensor, name: str):
    es = t.element_size()
    if t.data_ptr() % 16 != 0 or (t.stride(0) * es) % 16 != 0:
        raise RuntimeError(f"{name}: data pointer and row stride must be multiples of 16 bytes")


def nf4_quantize(w: torch.Tensor):
    """bf16 [N, K] (contiguous rows, K % 64 == 0) -> (q uint8 [N, K/2], absmax fp32 [N, K/64]) by dwm_nf4_quantize"""
    from . import nf4
    _chk2d(w, "w")
    _chk_aligned(w, "w")
    N, K = w.shape
    if N == 0 or K == 0 or K % nf4.BLOCK != 0:
        raise RuntimeError(f"nf4_quantize: K = {K} must be a positive multiple of {nf4.BLOCK} (and N = {N} positive)")
    q = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device)
    absmax = torch.empty((N, K // nf4.BLOCK), dtype=f32, device=w.device)
    _call("dwm_nf4_quantize", w.data_ptr(), w.stride(0), N, K, nf4.device_code(w.device).data_ptr(), q.data_ptr(), absmax.data_ptr())
    return q, absmax


def nf4_dequantize(q: torch.Tensor, absmax: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """W' = bf16(code[q] * absmax), bf16 [N, K] (dwm_nf4_dequantize); out: contiguous rows, any 16-byte-aligned row stride"""
    from . import nf4
    N, K = _nf4_operands(q, absmax, "nf4_dequantize")
    if out is None:
        out = torch.empty((N, K), dtype=bf16, device=q.device)
    _chk2d(out, "out")
    _chk_aligned(out, "out")
    if tuple(out.shape) != (N, K) or out.device != q.device:
        raise RuntimeError(f"nf4_dequantize: out must be [{N}, {K}] on the device of q, got {tuple(out.shape)}")
    _call("dwm_nf4_dequantize", q.data_ptr(), absmax.data_ptr(), N, K, nf4.device_code(q.device).data_ptr(), out.data_ptr(), out.stride(0))
    return out


def gemm_nf4(a: torch.Tensor, q: torch.Tensor, absmax: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
             out: Optional[torch.Tensor] = None, out32: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a [M, K] bf16 times the NF4 weight (q, absmax) [N, K] transposed, plus bias (dwm_gemm_nf4): the bf16 linear layer on the
    dequantised weight W', the weight dequantised on the way into the matrix pipes.  Returns bf16 [M, N] (`out`, allocated if
    neither output is given) or, with `out32` (fp32 [M, N], the residual stream), adds the result into it in place and returns
    it.  N % 8 == 0.  A row's result does not depend on M."""
    from . import nf4
    _chk2d(a, "a")
    _chk_aligned(a, "a")
    N, K = _nf4_operands(q, absmax, "gemm_nf4")
    M = a.shape[0]
    if M == 0 or a.shape[1] != K or a.device != q.device:
        raise RuntimeError(f"gemm_nf4: a must be [M >= 1, {K}] on the device of q, got {tuple(a.shape)}")
    if N % 8 != 0:
        raise NotImplementedError(f"gemm_nf4: N = {N} must be a multiple of 8")
    _chkvec(bias, "bias")
    if bias is not None and (bias.numel() != N or bias.device != a.device or bias.data_ptr() % 16 != 0):
        raise RuntimeError(f"gemm_nf4: bias must be a 16-byte-aligned vector of {N} elements on the device of a")
    if out is not None and out32 is not None:
        raise RuntimeError("gemm_nf4: give out or out32, not both")
    if out32 is None and out is None:
        out = torch.empty((M, N), dtype=bf16, device=a.device)
    res = out if out32 is None else out32
    _chk2d(res, "out" if out32 is None else "out32", bf16 if out32 is None else f32)
    _chk_aligned(res, "out" if out32 is None else "out32")
    if tuple(res.shape) != (M, N) or res.device != a.device:
        raise RuntimeError(f"gemm_nf4: the output must be [{M}, {N}] on the device of a, got {tuple(res.shape)}")
    if _overlaps(res, a):
        raise RuntimeError("gemm_nf4: the output must not overlap a")
    g = _lib.GemmNf4Args()
    g.A, g.lda, g.q, g.absmax, g.code, g.bias = a.data_ptr(), a.stride(0), q.data_ptr(), absmax.data_ptr(), nf4.device_code(a.device).data_ptr(), _p(bias)
    g.C, g.ldc, g.C32, g.ldc32 = _p(out), (out.stride(0) if out is not None else 0), _p(out32), (out32.stride(0) if out32 is not None else 0)
    g.M, g.N, g.K = M, N, K
    _call("dwm_gemm_nf4", C.byref(g))
    return res


def cast_bf16(x: torch.Tensor) -> torch.Tensor:
    if x.dtype == bf16:
        return x
    if x.dtype != f32 or not x.is_cuda:
        raise RuntimeError("cast_bf16: expected an fp32 device tensor")
    x = x.contiguous()
    out = torch.empty(x.shape, dtype=bf16, device=x.device)
    _call("dwm_cast_f32_to_bf16", x.data_ptr(), out.data_ptr(), x.numel())
    return out


def cast_f32(x: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False) -> torch.Tensor:
    """fp32 (+)= bf16, 2-D row-strided or contiguous (dwm_cast_bf16_to_f32): the entry of the fp32 residual stream, and the
    fp32 gradient accumulation of training (train_ops.cast_f32 is this function)"""
    if x.dtype != bf16 or not x.is_cuda:
        raise RuntimeError("cast_f32: expected a bf16 device tensor")
    x2 = x if x.dim() == 2 else x.reshape(1, -1)
    _chk2d(x2, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=f32, device=x.device)
        accumulate = False
    o2 = out if out.dim() == 2 else out.reshape(1, -1)
    _chk2d(o2, "out", f32)
    if o2.shape != x2.shape:
        raise RuntimeError("cast_f32: shape mismatch")
    _call("dwm_cast_bf16_to_f32", x2.data_ptr(), x2.stride(0), o2.data_ptr(), o2.stride(0), x2.shape[0], x2.shape[1], int(accumulate))
    return out


def tr_probe(offsets: torch.Tensor) -> torch.Tensor:
    """Diagnostic: semantics probe of ds_read_b64_tr_b16 (tests only)."""
    offsets = offsets.to(torch.int32).contiguous()
    out = torch.empty((64, 4), dtype=torch.int16, device=offsets.device)
    _call("dwm_debug_tr_probe", offsets.data_ptr(), out.data_ptr())
    return out
