"""Thin wrappers over the training entry points of libdwm_hip.so (include/dwm_hip.h, "Training"
section) plus the two GEMM-shaped composites every linear layer's backward needs.  Same
conventions as opendwm_amd.ops: bf16 CUDA tensors, current stream, no fallback."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence, Tuple

import torch

from . import _lib, ops, quant8
from .ops import _call, _chk2d, _p, cast_f32, ACT_GELU_TANH, ACT_SILU  # noqa: F401  (cast_f32: fp32 (+)= bf16, used as train_ops.cast_f32)
from .ops import ordered_reductions, ordered_reductions_enabled, carries_ordered_scope  # noqa: F401  (the scope lives beside the GEMM scope)

bf16 = torch.bfloat16
# weight gradients by dwm_gemm_tn (operands as they are); "0": the transposes + NT GEMM path (A/B measurements)
WGRAD_TN = os.environ.get("DWM_WGRAD_TN", "1") != "0"


def transpose(x: torch.Tensor, rows_pad: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x [rows, cols] -> out [cols, rows_pad] (zero-filled beyond `rows`; default: rows rounded up to 64)."""
    _chk2d(x, "x")
    rows, cols = x.shape
    if rows_pad is None:
        rows_pad = (rows + 63) // 64 * 64
    if out is None:
        out = torch.empty((cols, rows_pad), dtype=bf16, device=x.device)
    _call("dwm_transpose_bf16", _p(x), x.stride(0), rows, cols, _p(out), out.stride(0), rows_pad)
    return out


# ---- ordered reductions (include/dwm_hip.h, "Ordered reductions").  Inside `ordered_reductions(True)` the five reducing
# wrappers below launch dwm_<op>_ordered with a workspace from the caching allocator (uninitialised: stage 1 writes every slot stage 2
# reads).  `return_partials=True` (tests) makes a wrapper return (result, partials): the workspace viewed as [chunks..., cols] with
# the op's documented layout, None outside the scope.
def _ordered_workspace(query: str, dev: torch.device, *args) -> torch.Tensor:
    return torch.empty(max(int(getattr(_lib.load(), query)(*args)), 1), dtype=torch.float32, device=dev)


def segsum(a: torch.Tensor, b: Optional[torch.Tensor] = None, rows_per_group: Optional[int] = None,
           out: Optional[torch.Tensor] = None, return_partials: bool = False):
    """fp32 [groups, ncols]: per-group column sums of a (* b); `out` (if given) is accumulated into.
    return_partials: (out, partials [groups, chunks, ncols]) inside ordered_reductions, (out, None) outside."""
    _chk2d(a, "a")
    rows, ncols = a.shape
    rpg = rows if rows_per_group is None else rows_per_group
    groups = (rows + rpg - 1) // rpg
    if out is None:
        out = torch.zeros((groups, ncols), dtype=torch.float32, device=a.device)
    if b is not None:
        _chk2d(b, "b")
    ws = None
    if ordered_reductions_enabled():
        ws = _ordered_workspace("dwm_segsum_ordered_floats", a.device, rows, ncols, rpg)
        _call("dwm_segsum_ordered", _p(a), a.stride(0), _p(b), 0 if b is None else b.stride(0), rows, ncols, rpg, _p(out),
              out.stride(0), _p(ws), ws.numel())
        ws = ws.view(groups, -1, ncols)
    else:
        _call("dwm_segsum", _p(a), a.stride(0), _p(b), 0 if b is None else b.stride(0), rows, ncols, rpg, _p(out), out.stride(0))
    return (out, ws) if return_partials else out


def segsum_diff(a: torch.Tensor, b: torch.Tensor, b2: torch.Tensor, rows_per_group: Optional[int] = None,
                out: Optional[torch.Tensor] = None, return_partials: bool = False):
    """fp32 [groups, ncols]: per-group column sums of a * (b - b2), the difference taken in fp32 before the product; `out` (if given)
    is accumulated into.  return_partials: as segsum."""
    for t, n in ((a, "a"), (b, "b"), (b2, "b2")):
        _chk2d(t, n)
    if b.shape != a.shape or b2.shape != a.shape:
        raise RuntimeError("segsum_diff: shape mismatch")
    rows, ncols = a.shape
    rpg = rows if rows_per_group is None else rows_per_group
    groups = (rows + rpg - 1) // rpg
    if out is None:
        out = torch.zeros((groups, ncols), dtype=torch.float32, device=a.device)
    ws = None
    if ordered_reductions_enabled():
        ws = _ordered_workspace("dwm_segsum_diff_ordered_floats", a.device, rows, ncols, rpg)
        _call("dwm_segsum_diff_ordered", _p(a), a.stride(0), _p(b), b.stride(0), _p(b2), b2.stride(0), rows, ncols, rpg,
              _p(out), out.stride(0), _p(ws), ws.numel())
        ws = ws.view(groups, -1, ncols)
    else:
        _call("dwm_segsum_diff", _p(a), a.stride(0), _p(b), b.stride(0), _p(b2), b2.stride(0), rows, ncols, rpg,
              _p(out), out.stride(0))
    return (out, ws) if return_partials else out


def act_fwd(x: torch.Tensor, act: int) -> torch.Tensor:
    y = torch.empty_like(x)
    _call("dwm_act_fwd", _p(x), _p(y), x.numel(), act)
    return y


def act_bwd(x: torch.Tensor, dy: torch.Tensor, act: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    dx = torch.empty_like(x) if out is None else out
    _call("dwm_act_bwd", _p(x), _p(dy), _p(dx), x.numel(), act)
    return dx


def geglu_fwd(u: torch.Tensor) -> torch.Tensor:
    _chk2d(u, "u")
    rows, two = u.shape
    g = torch.empty((rows, two // 2), dtype=bf16, device=u.device)
    _call("dwm_geglu_fwd", _p(u), u.stride(0), rows, two // 2, _p(g), g.stride(0))
    return g


def geglu_bwd(u: torch.Tensor, dg: torch.Tensor) -> torch.Tensor:
    _chk2d(u, "u"); _chk2d(dg, "dg")
    rows, two = u.shape
    du = torch.empty_like(u)
    _call("dwm_geglu_bwd", _p(u), u.stride(0), _p(dg), dg.stride(0), rows, two // 2, _p(du), du.stride(0))
    return du


def act_bwd_recompute(x: torch.Tensor, dy: torch.Tensor, act: int, y_out: Optional[torch.Tensor] = None,
                      dx: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(act(x), dy * act'(x)) from one read of x: act_fwd and act_bwd in one launch, bit-equal to both"""
    y_out = torch.empty_like(x) if y_out is None else y_out
    dx = torch.empty_like(x) if dx is None else dx
    if dy.numel() != x.numel() or y_out.numel() != x.numel() or dx.numel() != x.numel():
        raise RuntimeError("act_bwd_recompute: x, dy, y_out and dx must have one element count")
    _call("dwm_act_bwd_recompute", _p(x), _p(dy), _p(y_out), _p(dx), x.numel(), act)
    return y_out, dx


def geglu_bwd_recompute(u: torch.Tensor, dg: torch.Tensor, g_out: Optional[torch.Tensor] = None,
                        du: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(geglu_fwd(u), geglu_bwd(u, dg)) from one read of u"""
    _chk2d(u, "u"); _chk2d(dg, "dg")
    rows, two = u.shape
    g_out = torch.empty((rows, two // 2), dtype=bf16, device=u.device) if g_out is None else g_out
    du = torch.empty_like(u) if du is None else du
    _chk2d(g_out, "g_out"); _chk2d(du, "du")
    if dg.shape != (rows, two // 2) or g_out.shape != dg.shape or du.shape != u.shape:
        raise RuntimeError("geglu_bwd_recompute: u and du [rows, 2 * inner], dg and g_out [rows, inner] expected")
    _call("dwm_geglu_bwd_recompute", _p(u), u.stride(0), _p(dg), dg.stride(0), rows, two // 2, _p(g_out), g_out.stride(0),
          _p(du), du.stride(0))
    return g_out, du


def rowcombine(a: torch.Tensor, *, gate_a: Optional[torch.Tensor] = None, rows_per_gate_a: int = 1,
               coef_a: Optional[torch.Tensor] = None, rows_per_coef_a: int = 1,
               b: Optional[torch.Tensor] = None, coef_b: Optional[torch.Tensor] = None, rows_per_coef_b: int = 1,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = a * gate_a[row // rpg] * coef_a[row // rpc] + b * coef_b[row // rpc] (see dwm_rowcombine)."""
    _chk2d(a, "a")
    if out is None:
        out = torch.empty((a.shape[0], a.shape[1]), dtype=bf16, device=a.device)
    r = _lib.RowCombineArgs()
    r.a, r.lda = _p(a), a.stride(0)
    if gate_a is not None:
        _chk2d(gate_a, "gate_a")
        r.gate_a, r.ld_gate_a, r.rows_per_gate_a = _p(gate_a), gate_a.stride(0), rows_per_gate_a
    if coef_a is not None:
        r.coef_a, r.rows_per_coef_a = _p(coef_a), rows_per_coef_a
    if b is not None:
        _chk2d(b, "b")
        r.b, r.ldb = _p(b), b.stride(0)
        if coef_b is not None:
            r.coef_b, r.rows_per_coef_b = _p(coef_b), rows_per_coef_b
    r.out, r.ldo, r.rows, r.ncols = _p(out), out.stride(0), a.shape[0], a.shape[1]
    _call("dwm_rowcombine", C.byref(r))
    return out


def layernorm_bwd(x: torch.Tensor, dy: torch.Tensor, *, eps: float, dx: Optional[torch.Tensor] = None,
                  accumulate: bool = False, addvec: Optional[torch.Tensor] = None, rows_per_add: int = 1,
                  weight: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None,
                  scale2: Optional[torch.Tensor] = None, rows_per_mod: int = 0, dy2: Optional[torch.Tensor] = None,
                  dgamma: Optional[torch.Tensor] = None, dbeta: Optional[torch.Tensor] = None,
                  dgamma2: Optional[torch.Tensor] = None, dbeta2: Optional[torch.Tensor] = None,
                  grad_per_group: bool = False, return_partials: bool = False):
    """Backward of ops.layernorm; dgamma/dbeta[/2] are fp32 [G or 1, D] accumulators (see dwm_layernorm_bwd).
    return_partials: (dx, partials [slots, groups, chunks, D]) inside ordered_reductions - slots = the accumulators given, in the
    order dgamma, dbeta, dgamma2, dbeta2 - and (dx, None) outside or without accumulators."""
    _chk2d(x, "x"); _chk2d(dy, "dy")
    rows, D = x.shape
    if dx is None:
        dx = torch.empty((rows, D), dtype=bf16, device=x.device)
        accumulate = False
    a = _lib.LayerNormBwdArgs()
    a.x, a.ldx, a.dy, a.lddy, a.dx, a.lddx = _p(x), x.stride(0), _p(dy), dy.stride(0), _p(dx), dx.stride(0)
    a.accumulate, a.rows, a.D, a.eps = int(accumulate), rows, D, eps
    if addvec is not None:
        a.addvec, a.ld_add, a.rows_per_add = _p(addvec), addvec.stride(0), rows_per_add
    if dy2 is not None:
        a.dy2, a.lddy2 = _p(dy2), dy2.stride(0)
    a.weight = _p(weight)
    mod = scale if scale is not None else scale2
    if mod is not None:
        a.scale, a.scale2, a.ld_mod, a.rows_per_mod = _p(scale), _p(scale2), mod.stride(0), rows_per_mod
    elif grad_per_group:
        a.rows_per_mod = rows_per_mod
    g0 = next((g for g in (dgamma, dbeta, dgamma2, dbeta2) if g is not None), None)
    if g0 is not None:
        a.dgamma, a.dbeta, a.dgamma2, a.dbeta2 = _p(dgamma), _p(dbeta), _p(dgamma2), _p(dbeta2)
        a.ld_grad, a.grad_per_group = g0.stride(0), int(grad_per_group)
    ws = None
    if ordered_reductions_enabled():
        ws = _ordered_workspace("dwm_layernorm_bwd_ordered_floats", x.device, C.byref(a))
        _call("dwm_layernorm_bwd_ordered", C.byref(a), _p(ws), ws.numel())
        slots = sum(g is not None for g in (dgamma, dbeta, dgamma2, dbeta2))
        rpg = rows_per_mod if rows_per_mod > 0 else rows
        groups = (rows + rpg - 1) // rpg
        ws = ws.view(slots, groups, -1, D) if slots else None
    else:
        _call("dwm_layernorm_bwd", C.byref(a))
    return (dx, ws) if return_partials else dx


def rmsnorm_heads_train_(x: torch.Tensor, w_expanded: torch.Tensor, eps: float) -> torch.Tensor:
    """In-place per-head RMSNorm of x [rows, ncols]; returns rinv fp32 [rows, ncols // 64]."""
    _chk2d(x, "x")
    rows, ncols = x.shape
    rinv = torch.empty((rows, ncols // 64), dtype=torch.float32, device=x.device)
    _call("dwm_rmsnorm_heads_train", _p(x), x.stride(0), rows, ncols, _p(w_expanded), eps, _p(rinv))
    return rinv


def rmsnorm_heads_bwd_(y: torch.Tensor, rinv: torch.Tensor, w_expanded: torch.Tensor, dy: torch.Tensor,
                       dw: torch.Tensor, return_partials: bool = False):
    """dy -> dx in place; dw fp32 [ncols] accumulated.
    return_partials: (dx, partials [chunks of 32 rows, ncols]) inside ordered_reductions, (dx, None) outside."""
    _chk2d(y, "y"); _chk2d(dy, "dy")
    rows, ncols = y.shape
    ws = None
    if ordered_reductions_enabled():
        ws = _ordered_workspace("dwm_rmsnorm_heads_bwd_ordered_floats", y.device, rows, ncols)
        _call("dwm_rmsnorm_heads_bwd_ordered", _p(y), y.stride(0), _p(rinv), _p(w_expanded), _p(dy), dy.stride(0), rows, ncols, _p(dw),
              _p(ws), ws.numel())
        ws = ws.view(-1, ncols)
    else:
        _call("dwm_rmsnorm_heads_bwd", _p(y), y.stride(0), _p(rinv), _p(w_expanded), _p(dy), dy.stride(0), rows, ncols, _p(dw))
    return (dy, ws) if return_partials else dy


# ---- tensor lists: AdamW, 8-bit AdamW and the gradient norm share one scheme.  A list of tensors is cut into chunks of `chunk` elements,
# one workgroup per chunk; the kernels get an item array (one struct of pointers and the element count per tensor) and two block tables.
ADAMW_CHUNK = 1 << 16            # elements per workgroup of the multi-tensor AdamW (a multiple of the 8-bit block of 256)
GRAD_CHUNK = 1 << 16             # elements per workgroup of dwm_grad_sumsq_multi / dwm_grad_scale_multi
GRAD_SUMSQ_E = GRAD_CHUNK // 1024        # squares one fp32 accumulator of grad_sumsq_multi_kernel receives per chunk, at most


class _BlockTables:
    """(block_item int32, block_start int64) of a tensor list on its device: ceil(n / chunk) workgroups per tensor, in order"""
    def __init__(self, dev: torch.device, chunk: int, numels: tuple):
        bi, bs = [], []
        for i, n in enumerate(numels):
            nb = (n + chunk - 1) // chunk
            bi.append(torch.full((nb,), i, dtype=torch.int32))
            bs.append(torch.arange(nb, dtype=torch.int64) * chunk)
        self.block_item, self.block_start, self._scratch = torch.cat(bi).to(dev), torch.cat(bs).to(dev), None

    def grad_scratch(self):
        """(partials fp64, flags int32), one per block, for dwm_grad_sumsq_multi: allocated on first use and reused by every call on
        this list, so calls on one list belong on one stream"""
        if self._scratch is None:
            self._scratch = (torch.empty_like(self.block_item, dtype=torch.float64), torch.empty_like(self.block_item))
        return self._scratch


# (device index, chunk, tuple of numels) -> _BlockTables, least recently used first.  Six entries: the fp32 list of an optimizer, its
# 8-bit list, the gradient list (one entry with either where the numels are the same), the two lists of an EMA (the shadows without a
# gradient in the step, the exchange) and one spare.
_BLOCK_TABLES: dict = {}


def _block_tables(dev: torch.device, chunk: int, numels: tuple) -> _BlockTables:
    key = (dev.index, chunk, numels)
    tab = _BLOCK_TABLES.pop(key, None)                # a hit goes back in as the most recent
    if tab is None:
        while len(_BLOCK_TABLES) >= 6:
            _BLOCK_TABLES.pop(next(iter(_BLOCK_TABLES)))
        tab = _BlockTables(dev, chunk, numels)
    _BLOCK_TABLES[key] = tab
    return tab


# (device index, rows) -> item array, least recently used first: the lists of a sync-free optimizer step (gradients, fp32 batch, 8-bit
# batch) hold the same pointers step after step, and a copy from pageable host memory would make the host wait for the stream
_ITEMS: dict = {}


def _items(rows, dev: torch.device, reuse: bool = False) -> torch.Tensor:
    """equal-length rows of integers (the pointers of one tensor's item struct, its element count last) -> the item array on `dev`.
    reuse: the array of an earlier call with the same rows, where there is one (eight are kept)"""
    if not reuse:
        return torch.tensor(rows, dtype=torch.int64).to(dev, non_blocking=True)
    key = (dev.index, tuple(rows))
    hit = _ITEMS.pop(key, None)
    if hit is None:
        while len(_ITEMS) >= 8:
            _ITEMS.pop(next(iter(_ITEMS)))
        hit = torch.tensor(rows, dtype=torch.int64).to(dev)
    _ITEMS[key] = hit
    return hit


def _adamw_scalars(lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float) -> tuple:
    """the eight trailing float arguments of dwm_adamw / dwm_adamw_multi / dwm_adamw8_multi (bias corrections from `step`)"""
    return lr, beta1, beta2, eps, weight_decay, 1.0 - beta1 ** step, 1.0 - beta2 ** step, grad_scale


def adamw_(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, p_bf16: Optional[torch.Tensor], *,
           lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int, grad_scale: float = 1.0) -> None:
    for t in (p, g, m, v):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError("adamw_: fp32 contiguous tensors expected")
    _call("dwm_adamw", _p(p), _p(g), _p(m), _p(v), _p(p_bf16), p.numel(),
          *_adamw_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale))


def _dev_operands(device_operands, dev: torch.device, what: str, hyper_floats: int = 3) -> tuple:
    """(hyper, cond) of the *_dev entry points checked: hyper fp32 [>= 3] = (lr, bias_corr1, bias_corr2) - [>= 4] with
    one_minus_decay behind them for the EMA forms (hyper_floats) -, cond None or fp32 [>= 3] = the out of grad_sumsq_multi, both
    contiguous on `dev`"""
    hyper, cond = device_operands
    for t, name, need in ((hyper, "hyper", hyper_floats), (cond, "cond", 3)):
        if t is None and name == "cond":
            continue
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < need or t.device != dev:
            raise RuntimeError(f"{what}: device_operands {name} must be a contiguous fp32 tensor of at least {need} elements on the "
                               "tensors' device")
    return hyper, cond


def adamw_hyper(lr: float, beta1: float, beta2: float, step: int, out: Optional[torch.Tensor] = None,
                one_minus_decay: float = 0.0) -> torch.Tensor:
    """host tensor [4] = (lr, bias_corr1, bias_corr2, one_minus_decay) of one optimizer step: the `hyper` array of the *_dev entry
    points, from the scalars `_adamw_scalars` hands the by-value ones (so a float32 of either holds the same bits).  The fourth
    float is read by the EMA forms only."""
    sc = _adamw_scalars(lr, beta1, beta2, 0.0, 0.0, step, 1.0)
    out = torch.empty(4, dtype=torch.float32) if out is None else out
    out[0], out[1], out[2], out[3] = sc[0], sc[5], sc[6], one_minus_decay
    return out


def adamw_multi_(ps, gs, ms, vs, shadows, *, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float, step: int,
                 grad_scale: float = 1.0, device_operands: Optional[tuple] = None) -> None:
    """dwm_adamw_multi: one launch for the whole list (fp32 contiguous p / g / m / v of equal numel per entry; shadows: bf16 copy or
    None).  All entries share the hyper-parameters and `step`.
    device_operands = (hyper, cond): dwm_adamw_multi_dev - lr and the bias corrections are read from `hyper`, the gradient
    coefficient and the non-finite flag from `cond` (None: 1 and 0); `lr`, `step` and `grad_scale` are then not used."""
    if not ps:
        return
    dev = ps[0].device
    rows = []
    for p, g, m, v, sh in zip(ps, gs, ms, vs, shadows):
        for t in (p, g, m, v):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.device != dev:
                raise RuntimeError("adamw_multi_: fp32 contiguous tensors of one shape on one device expected")
        rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if sh is None else sh.data_ptr(), p.numel()))
    items = _items(rows, dev, reuse=device_operands is not None)                      # [n, 6] = dwm_adamw_item[n]
    tab = _block_tables(dev, ADAMW_CHUNK, tuple(r[-1] for r in rows))
    if device_operands is not None:
        hyper, cond = _dev_operands(device_operands, dev, "adamw_multi_")
        _call("dwm_adamw_multi_dev", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK,
              _p(hyper), _p(cond), beta1, beta2, eps, weight_decay)
        return
    _call("dwm_adamw_multi", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK,
          *_adamw_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale))


# ---- block-wise 8-bit optimizer state (opendwm_amd.quant8: value = code[q] * absmax[block of 256])
def _chk_q8(q: torch.Tensor, absmax: torch.Tensor, n: int, dev, what: str) -> None:
    if (q.dtype != torch.uint8 or not q.is_contiguous() or q.numel() != n or q.device != dev or absmax.dtype != torch.float32
            or not absmax.is_contiguous() or absmax.numel() != quant8.n_blocks(n) or absmax.device != dev):
        raise RuntimeError(f"{what}: contiguous uint8 codes [n] and fp32 scales [ceil(n / 256)] on the tensor's device expected")


def _chk_code(code: torch.Tensor, dev, what: str) -> None:
    if code.dtype != torch.float32 or not code.is_contiguous() or code.numel() != 256 or code.device != dev:
        raise RuntimeError(f"{what}: the code table must be 256 contiguous fp32 values on the tensor's device")


def quantize_blockwise8(x: torch.Tensor, code: torch.Tensor, floor_positive: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """x (fp32, contiguous) -> (codes uint8 of x's shape, absmax fp32 [ceil(n / 256)]); floor_positive: a strictly positive value
    never gets the zero code (see dwm_quantize_blockwise8)"""
    if x.dtype != torch.float32 or not x.is_contiguous() or not x.is_cuda or x.numel() == 0:
        raise RuntimeError("quantize_blockwise8: a non-empty fp32 contiguous device tensor expected")
    _chk_code(code, x.device, "quantize_blockwise8")
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    absmax = torch.empty(quant8.n_blocks(x.numel()), dtype=torch.float32, device=x.device)
    _call("dwm_quantize_blockwise8", _p(x), x.numel(), _p(code), int(floor_positive), _p(q), _p(absmax))
    return q, absmax


def dequantize_blockwise8(q: torch.Tensor, absmax: torch.Tensor, code: torch.Tensor) -> torch.Tensor:
    """fp32 tensor of q's shape: code[q] * absmax[block]"""
    if not q.is_cuda or q.numel() == 0:
        raise RuntimeError("dequantize_blockwise8: a non-empty device tensor expected")
    _chk_q8(q, absmax, q.numel(), q.device, "dequantize_blockwise8")
    _chk_code(code, q.device, "dequantize_blockwise8")
    x = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    _call("dwm_dequantize_blockwise8", _p(q), _p(absmax), q.numel(), _p(code), _p(x))
    return x


def adamw8_multi_(ps, gs, mqs, mas, vqs, vas, shadows, *, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                  step: int, grad_scale: float = 1.0, device_operands: Optional[tuple] = None) -> None:
    """dwm_adamw8_multi: adamw_multi_ with the moments of every entry in the 8-bit format (mq / vq: uint8 codes, ma / va: fp32
    block scales); the signed table encodes m, the unsigned one v.  device_operands: as for adamw_multi_ (dwm_adamw8_multi_dev)."""
    if not ps:
        return
    dev = ps[0].device
    rows = []
    for p, g, mq, ma, vq, va, sh in zip(ps, gs, mqs, mas, vqs, vas, shadows):
        for t in (p, g):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.device != dev:
                raise RuntimeError("adamw8_multi_: fp32 contiguous tensors of one shape on one device expected")
        _chk_q8(mq, ma, p.numel(), dev, "adamw8_multi_")
        _chk_q8(vq, va, p.numel(), dev, "adamw8_multi_")
        rows.append((p.data_ptr(), g.data_ptr(), mq.data_ptr(), ma.data_ptr(), vq.data_ptr(), va.data_ptr(),
                     0 if sh is None else sh.data_ptr(), p.numel()))
    items = _items(rows, dev, reuse=device_operands is not None)                      # [n, 8] = dwm_adamw8_item[n]
    tab = _block_tables(dev, ADAMW_CHUNK, tuple(r[-1] for r in rows))
    code_m, code_v = quant8.device_codes(dev)
    if device_operands is not None:
        hyper, cond = _dev_operands(device_operands, dev, "adamw8_multi_")
        _call("dwm_adamw8_multi_dev", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK,
              _p(code_m), _p(code_v), _p(hyper), _p(cond), beta1, beta2, eps, weight_decay)
        return
    _call("dwm_adamw8_multi", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK, _p(code_m),
          _p(code_v), *_adamw_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale))


# ---- EMA weights (include/dwm_hip.h "EMA weights"): e' = e + one_minus_decay * (p' - e), one fp32 shadow per tensor
def _chk_ema(e: Optional[torch.Tensor], p: torch.Tensor, what: str) -> int:
    """the pointer of the shadow `e` of `p` (0 for None: the tensor has none)"""
    if e is None:
        return 0
    if e.dtype != torch.float32 or not e.is_contiguous() or e.numel() != p.numel() or e.device != p.device or e.data_ptr() == p.data_ptr():
        raise RuntimeError(f"{what}: a shadow must be an fp32 contiguous tensor of its parameter's size on its device, and not the "
                           "parameter itself")
    return e.data_ptr()


def _chk_omd(one_minus_decay: float, what: str) -> float:
    if not 0.0 <= one_minus_decay <= 1.0:               # a nan fails both comparisons
        raise ValueError(f"{what}: one_minus_decay must be in [0, 1], got {one_minus_decay!r}")
    return float(one_minus_decay)


def adamw_ema_multi_(ps, gs, ms, vs, shadows, emas, *, lr: float, beta1: float, beta2: float, eps: float, weight_decay: float,
                     step: int, one_minus_decay: float, grad_scale: float = 1.0, device_operands: Optional[tuple] = None) -> None:
    """dwm_adamw_ema_multi: adamw_multi_ with the EMA shadow of every entry (emas: fp32 tensor or None = no shadow, updated as by
    adamw_multi_) moved in the same pass.  p / m / v / the bf16 copies come out bit-equal to adamw_multi_.
    device_operands = (hyper, cond): dwm_adamw_ema_multi_dev - as for adamw_multi_, and one_minus_decay is read from hyper[3]
    (`adamw_hyper(..., one_minus_decay=)`); the keyword is then not used."""
    if not ps:
        return
    dev = ps[0].device
    rows = []
    for p, g, m, v, sh, e in zip(ps, gs, ms, vs, shadows, emas):
        for t in (p, g, m, v):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.device != dev:
                raise RuntimeError("adamw_ema_multi_: fp32 contiguous tensors of one shape on one device expected")
        rows.append((p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if sh is None else sh.data_ptr(),
                     _chk_ema(e, p, "adamw_ema_multi_"), p.numel()))
    items = _items(rows, dev, reuse=device_operands is not None)                      # [n, 7] = dwm_adamw_ema_item[n]
    tab = _block_tables(dev, ADAMW_CHUNK, tuple(r[-1] for r in rows))
    if device_operands is not None:
        hyper, cond = _dev_operands(device_operands, dev, "adamw_ema_multi_", hyper_floats=4)
        _call("dwm_adamw_ema_multi_dev", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK,
              _p(hyper), _p(cond), beta1, beta2, eps, weight_decay)
        return
    _call("dwm_adamw_ema_multi", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK,
          *_adamw_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale), _chk_omd(one_minus_decay, "adamw_ema_multi_"))


def adamw8_ema_multi_(ps, gs, mqs, mas, vqs, vas, shadows, emas, *, lr: float, beta1: float, beta2: float, eps: float,
                      weight_decay: float, step: int, one_minus_decay: float, grad_scale: float = 1.0,
                      device_operands: Optional[tuple] = None) -> None:
    """dwm_adamw8_ema_multi: adamw8_multi_ with the EMA shadows (fp32; None = no shadow) moved in the same pass; everything else as
    adamw_ema_multi_"""
    if not ps:
        return
    dev = ps[0].device
    rows = []
    for p, g, mq, ma, vq, va, sh, e in zip(ps, gs, mqs, mas, vqs, vas, shadows, emas):
        for t in (p, g):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != p.numel() or t.device != dev:
                raise RuntimeError("adamw8_ema_multi_: fp32 contiguous tensors of one shape on one device expected")
        _chk_q8(mq, ma, p.numel(), dev, "adamw8_ema_multi_")
        _chk_q8(vq, va, p.numel(), dev, "adamw8_ema_multi_")
        rows.append((p.data_ptr(), g.data_ptr(), mq.data_ptr(), ma.data_ptr(), vq.data_ptr(), va.data_ptr(),
                     0 if sh is None else sh.data_ptr(), _chk_ema(e, p, "adamw8_ema_multi_"), p.numel()))
    items = _items(rows, dev, reuse=device_operands is not None)                      # [n, 9] = dwm_adamw8_ema_item[n]
    tab = _block_tables(dev, ADAMW_CHUNK, tuple(r[-1] for r in rows))
    code_m, code_v = quant8.device_codes(dev)
    if device_operands is not None:
        hyper, cond = _dev_operands(device_operands, dev, "adamw8_ema_multi_", hyper_floats=4)
        _call("dwm_adamw8_ema_multi_dev", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK,
              _p(code_m), _p(code_v), _p(hyper), _p(cond), beta1, beta2, eps, weight_decay)
        return
    _call("dwm_adamw8_ema_multi", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK, _p(code_m),
          _p(code_v), *_adamw_scalars(lr, beta1, beta2, eps, weight_decay, step, grad_scale),
          _chk_omd(one_minus_decay, "adamw8_ema_multi_"))


def ema_multi_(emas, ps, *, one_minus_decay: float = 0.0, device_operands: Optional[tuple] = None) -> None:
    """dwm_ema_multi: emas[i] += one_minus_decay * (ps[i] - emas[i]) for the whole list in one launch; ps are read only.
    device_operands = (hyper, cond), either may be None: hyper (device fp32 [>= 4]) - one_minus_decay is read from hyper[3] and the
    keyword is not used; cond (device fp32 [>= 3], the out of grad_sumsq_multi) - nothing changes when cond[2] is set."""
    if not ps:
        return
    dev = ps[0].device
    rows = []
    for e, p in zip(emas, ps):
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev or not p.is_cuda or e is None:
            raise RuntimeError("ema_multi_: fp32 contiguous parameters with a shadow each on one HIP device expected (there is no "
                               "CPU fallback)")
        if p.numel() > 0:
            rows.append((_chk_ema(e, p, "ema_multi_"), p.data_ptr(), p.numel()))
    if not rows:
        return
    hyper = cond = None
    if device_operands is not None:
        hyper, cond = device_operands
        for t, name, need in ((hyper, "hyper", 4), (cond, "cond", 3)):
            if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < need
                                  or t.device != dev):
                raise RuntimeError(f"ema_multi_: device_operands {name} must be None or a contiguous fp32 tensor of at least {need} "
                                   "elements on the tensors' device")
    items = _items(rows, dev, reuse=device_operands is not None)                      # [n, 3] = dwm_ema_item[n]
    tab = _block_tables(dev, ADAMW_CHUNK, tuple(r[-1] for r in rows))
    omd = 0.0 if hyper is not None else _chk_omd(one_minus_decay, "ema_multi_")
    _call("dwm_ema_multi", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK, omd, _p(hyper),
          _p(cond))


def ema_swap_multi_(ps, emas, shadows) -> None:
    """dwm_ema_swap_multi: ps[i] <-> emas[i] in place for the whole list in one launch; shadows[i] (bf16 compute copy or None)
    receives the bf16 of the new ps[i].  A second call restores every byte."""
    if not ps:
        return
    dev = ps[0].device
    rows = []
    for p, e, sh in zip(ps, emas, shadows):
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev or not p.is_cuda or e is None:
            raise RuntimeError("ema_swap_multi_: fp32 contiguous parameters with a shadow each on one HIP device expected (there is "
                               "no CPU fallback)")
        if sh is not None and (sh.dtype != bf16 or not sh.is_contiguous() or sh.numel() != p.numel() or sh.device != dev):
            raise RuntimeError("ema_swap_multi_: a compute copy must be a contiguous bf16 tensor of its parameter's size")
        if p.numel() > 0:
            rows.append((p.data_ptr(), _chk_ema(e, p, "ema_swap_multi_"), 0 if sh is None else sh.data_ptr(), p.numel()))
    if not rows:
        return
    items = _items(rows, dev, reuse=True)                                             # [n, 4] = dwm_ema_swap_item[n]
    tab = _block_tables(dev, ADAMW_CHUNK, tuple(r[-1] for r in rows))
    _call("dwm_ema_swap_multi", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), ADAMW_CHUNK)


# ---- gradient norm / clip coefficient / non-finite check in one read (gradnorm.hip)
def _grad_items(gs, what: str, reuse: bool = False):
    """(non-empty entries, their dwm_grad_item rows on the device, block tables) of a gradient list"""
    gs = [g for g in gs if g.numel() > 0]
    if not gs:
        return gs, None, None
    dev = gs[0].device
    for g in gs:
        if g.dtype != torch.float32 or not g.is_contiguous() or g.device != dev or not g.is_cuda or g.data_ptr() % 4:
            raise RuntimeError(f"{what}: fp32 contiguous tensors on one HIP device expected (there is no CPU fallback)")
    rows = [(g.data_ptr(), g.numel()) for g in gs]
    return gs, _items(rows, dev, reuse), _block_tables(dev, GRAD_CHUNK, tuple(r[-1] for r in rows))


def grad_sumsq_multi(gs, pre_scale: float = 1.0, max_norm: Optional[float] = None, reuse_items: bool = False) -> torch.Tensor:
    """dwm_grad_sumsq_multi over a list of fp32 tensors (any 4-byte aligned views): device tensor [4] = (|| pre_scale * g ||_2,
    coef = pre_scale * min(1, max_norm / (norm + 1e-6)), 1.0 if any element is inf / nan else 0.0, 0).  max_norm None or <= 0: no
    clip, coef = pre_scale.  Empty tensors are dropped; an empty list gives (0, pre_scale, 0, 0) without a launch.
    reuse_items: the item array of an earlier call on the same tensors is used again (no host-to-device copy in a steady step)."""
    gs, items, tab = _grad_items(gs, "grad_sumsq_multi", reuse_items)
    if not gs:
        return torch.tensor([0.0, pre_scale, 0.0, 0.0], dtype=torch.float32)
    partials, flags = tab.grad_scratch()
    out = torch.empty(4, dtype=torch.float32, device=items.device)
    _call("dwm_grad_sumsq_multi", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), GRAD_CHUNK, pre_scale,
          0.0 if max_norm is None else max_norm, _p(partials), _p(flags), _p(out))
    return out


def grad_scale_multi_(gs, coef: float) -> None:
    """dwm_grad_scale_multi: g *= coef in place for every tensor of the list, one launch"""
    gs, items, tab = _grad_items(gs, "grad_scale_multi_")
    if not gs:
        return
    _call("dwm_grad_scale_multi", _p(items), _p(tab.block_item), _p(tab.block_start), tab.block_item.numel(), GRAD_CHUNK, coef)


# ---- low-rank adapters (lora.hip; include/dwm_hip.h "Low-rank adapters"): W + scale * B A over a list of weights
LORA_TILE_ROWS, LORA_TILE_COLS, LORA_DA_ROWS = 32, 128, 512      # the tile of the kernels and the rows behind one dA partial
LORA_FIN_CHUNK = 1 << 14                                         # elements of dA per workgroup of the finishing launch


class LoraTables:
    """the block tables of a list of (N, K, r) shapes on its device: .merge (32 x 128 tiles), .da (512-row chunk x 128 columns),
    .fin (runs of LORA_FIN_CHUNK of r * K) and .db (32 rows).  They depend on the shapes only: a caller with a fixed list keeps them."""
    def __init__(self, dev: torch.device, shapes):
        cd = lambda a, b: (a + b - 1) // b
        self.shapes, self.device = tuple(tuple(s) for s in shapes), dev
        self.merge = _BlockTables(dev, 1, tuple(cd(N, LORA_TILE_ROWS) * cd(K, LORA_TILE_COLS) for N, K, r in self.shapes))
        self.da = _BlockTables(dev, 1, tuple(cd(N, LORA_DA_ROWS) * cd(K, LORA_TILE_COLS) for N, K, r in self.shapes))
        self.fin = _BlockTables(dev, LORA_FIN_CHUNK, tuple(r * K for N, K, r in self.shapes))
        self.db = _BlockTables(dev, 1, tuple(cd(N, LORA_TILE_ROWS) for N, K, r in self.shapes))


def _lora_items(ws, as_, bs, outs, out2s, scratch, scales, what: str, out_dtypes: tuple):
    """(host item array, its device copy, shapes) of dwm_lora_item rows.  The dtypes, devices, contiguity and the agreement of the
    shapes are checked here; the limits on r and K are the library's (DWM_EUNSUPPORTED)."""
    import struct
    dev = ws[0].device
    rows, shapes = [], []
    for i, (w, a, b, out, scale) in enumerate(zip(ws, as_, bs, outs, scales)):
        for t, dts, name in ((w, (torch.float32, bf16), "the weight / gradient"), (a, (torch.float32,), "A"), (b, (torch.float32,), "B"),
                             (out, out_dtypes, "the output")):
            if not t.is_cuda or t.device != dev or t.dtype not in dts or not t.is_contiguous():
                raise RuntimeError(f"{what}: {name} of entry {i} must be a contiguous {' / '.join(str(d) for d in dts)} tensor on "
                                   "one HIP device (there is no CPU fallback)")
        if w.dim() != 2 or a.dim() != 2 or b.dim() != 2 or a.shape[1] != w.shape[1] or b.shape != (w.shape[0], a.shape[0]):
            raise RuntimeError(f"{what}: entry {i}: W [N, K], A [r, K] and B [N, r] expected, got {tuple(w.shape)}, {tuple(a.shape)}, "
                               f"{tuple(b.shape)}")
        N, K = w.shape
        r = a.shape[0]
        if out2s is None:
            if out.shape != w.shape:
                raise RuntimeError(f"{what}: entry {i}: out must have W's shape")
            out2, sc = 0, 0
        else:
            d2 = out2s[i]
            if out.shape != a.shape or d2.shape != b.shape or d2.dtype != torch.float32 or not d2.is_contiguous() or d2.device != dev:
                raise RuntimeError(f"{what}: entry {i}: dA and dB must be contiguous fp32 tensors of A's and B's shapes")
            out2, sc = d2.data_ptr(), scratch[i].data_ptr()
        flags = int(w.dtype == bf16) | (int(out.dtype == bf16) << 1)
        rows.append((w.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), out2, sc, N, K, r | (flags << 32),
                     struct.unpack("<I", struct.pack("<f", float(scale)))[0], r * K))
        shapes.append((N, K, r))
    host = torch.tensor(rows, dtype=torch.int64)                  # [n, 11] = dwm_lora_item[n]
    return host, host.to(dev, non_blocking=True), tuple(shapes)


def lora_merge_multi(ws, as_, bs, outs, scales, tables: Optional[LoraTables] = None) -> None:
    """dwm_lora_merge_multi: outs[i] = ws[i] + scales[i] * bs[i] @ as_[i] for the whole list in one launch.  ws / outs fp32 or bf16
    [N, K] (out may be w itself: the in-place fold), as_ fp32 [r, K], bs fp32 [N, r].  bf16 out = the merge (a compute copy),
    fp32 out = the fold; the arithmetic is stated at the prototype."""
    if not ws:
        return
    host, items, shapes = _lora_items(ws, as_, bs, outs, None, None, scales, "lora_merge_multi", (torch.float32, bf16))
    tab = tables if tables is not None and tables.shapes == shapes and tables.device == items.device else LoraTables(items.device, shapes)
    _call("dwm_lora_merge_multi", host.data_ptr(), len(shapes), _p(items), _p(tab.merge.block_item), _p(tab.merge.block_start),
          tab.merge.block_item.numel())


def lora_project_multi(gs, as_, bs, das, dbs, scales, accumulate: bool = False, tables: Optional[LoraTables] = None,
                       return_partials: bool = False):
    """dwm_lora_project_multi: das[i] (+)= scales[i] * bs[i]^T @ gs[i], dbs[i] (+)= scales[i] * gs[i] @ as_[i]^T for the whole list
    (three launches).  gs fp32 or bf16 [N, K]; das / dbs fp32, overwritten unless `accumulate`.  No atomics: equal bits every time.
    return_partials (tests): the dA partials of every entry, [row chunks, r, K]."""
    if not gs:
        return [] if return_partials else None
    dev = gs[0].device
    query = _lib.load().dwm_lora_project_ws_floats
    sizes = [max(int(query(g.shape[0], g.shape[1], a.shape[0])), 4) if g.dim() == 2 and a.dim() == 2 else 4 for g, a in zip(gs, as_)]
    offs = [0]
    for s in sizes:
        offs.append(offs[-1] + (s + 3) // 4 * 4)
    scratch = torch.empty(offs[-1], dtype=torch.float32, device=dev)
    parts = [scratch[o:o + s] for o, s in zip(offs, sizes)]
    host, items, shapes = _lora_items(gs, as_, bs, das, dbs, parts, scales, "lora_project_multi", (torch.float32,))
    tab = tables if tables is not None and tables.shapes == shapes and tables.device == items.device else LoraTables(items.device, shapes)
    _call("dwm_lora_project_multi", host.data_ptr(), len(shapes), _p(items), _p(tab.da.block_item), _p(tab.da.block_start),
          tab.da.block_item.numel(), _p(tab.fin.block_item), _p(tab.fin.block_start), tab.fin.block_item.numel(), LORA_FIN_CHUNK,
          _p(tab.db.block_item), _p(tab.db.block_start), tab.db.block_item.numel(), int(accumulate))
    if return_partials:
        return [p.view(-1, r, K) for p, (N, K, r) in zip(parts, shapes)]
    return None


# ------------------------------------------------------------------------------------------ composites
def linear_dgrad(dy: torch.Tensor, w_t: torch.Tensor, out: Optional[torch.Tensor] = None, **epi) -> torch.Tensor:
    """dX [M, K] = dY [M, N] @ W [N, K], with W^T [K, N] given (the GEMM contracts over the columns of
    both operands).  Extra keyword arguments are GEMM epilogue options (e.g. a fused residual add)."""
    return ops.gemm(dy, w_t, None, out=out, **epi)


def gemm_tn(dy: torch.Tensor, x: torch.Tensor, tap_shifts: Optional[Sequence[int]] = None, split_k: int = 0,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [N, taps*C] (bf16) = sum over rows m of dy[m, n] * x[clamp(m + shift_t, 0, rows(x) - 1), c] (dwm_gemm_tn): the weight
    gradient of a linear layer (no taps) or - dy and x on the same padded token grid, dy zero on its border rows - of a
    convolution with those taps, from the row-major operands as they are (no transposes, no per-tap gathers).
    dy [M, N], M % 64 == 0; x [rows, C]."""
    _chk2d(dy, "dy")
    _chk2d(x, "x")
    M, N = dy.shape
    Cc = x.shape[1]
    ntaps = len(tap_shifts) if tap_shifts is not None else 0
    if ntaps > 27:
        raise RuntimeError("gemm_tn: at most 27 taps")
    if tap_shifts is None and x.shape[0] < M:
        raise RuntimeError("gemm_tn: x has fewer rows than dy")
    cols = max(ntaps, 1) * Cc
    if out is None:
        out = torch.empty((N, cols), dtype=bf16, device=dy.device)
    _chk2d(out, "out")
    if out.shape != (N, cols):
        raise RuntimeError(f"gemm_tn: out must be [{N}, {cols}]")
    ws = ops._gemm_workspace(dy.device)
    g = _lib.GemmTnArgs()
    g.A, g.lda, g.B, g.ldb, g.b_rows = _p(dy), dy.stride(0), _p(x), x.stride(0), x.shape[0]
    g.out, g.ldo, g.M, g.N, g.C = _p(out), out.stride(0), M, N, Cc
    g.ntaps, g.split_k = ntaps, split_k
    for t in range(ntaps):
        g.tap_shift[t] = int(tap_shifts[t])
    g.workspace, g.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    _call("dwm_gemm_tn", C.byref(g))
    return out


def _tn_fits(n: int, cols: int) -> bool:
    """one fp32 partial tile set [n, cols] of dwm_gemm_tn must fit the shared GEMM workspace"""
    return n * cols * 4 <= ops.GEMM_WORKSPACE_BYTES


def linear_wgrad(dy: torch.Tensor, x: torch.Tensor, want_bias: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """dW [N, K] (bf16) = dY^T X and db [N] (fp32) = column sums of dY; dY [M, N], X [M, K].
    Both operands are transposed so the contraction (over the M tokens) runs along rows."""
    if WGRAD_TN and dy.shape[0] % 64 == 0 and dy.shape[1] % 8 == 0 and x.shape[1] % 8 == 0 and _tn_fits(dy.shape[1], x.shape[1]):
        dw = gemm_tn(dy, x)                # both operands as they are (gemm_tn.hip)
    else:
        dyt = transpose(dy)                # [N, Mp]
        xt = transpose(x)                  # [K, Mp]
        dw = ops.gemm(dyt, xt, None)       # [N, K]
    db = segsum(dy)[0] if want_bias else None
    return dw, db


def conv_wgrad(dy: torch.Tensor, x_pad: torch.Tensor, idx: torch.Tensor, shifts) -> torch.Tensor:
    """dW [N, taps*C] (tap-major, bf16): dW[n, t, c] = sum_pixels dy[pixel, n] * x_pad[idx[pixel] + shift_t, c].
    dy is scattered onto x_pad's row space (zeros elsewhere) and ALL taps are one dwm_gemm_tn launch over those rows; where
    that does not pay (an output grid much sparser than the input grid: stride-2 convolutions) or does not apply, one
    weight-gradient GEMM per tap on the transposed operands (gather of the tap-shifted rows + transpose, per tap)."""
    N, Cc = dy.shape[1], x_pad.shape[1]
    rows = x_pad.shape[0]
    if WGRAD_TN and N % 8 == 0 and Cc % 8 == 0 and 2 * dy.shape[0] >= rows and _tn_fits(N, len(shifts) * Cc):
        dyp = torch.zeros(((rows + 63) // 64 * 64, N), dtype=bf16, device=dy.device)
        dyp.index_copy_(0, idx, dy)
        return gemm_tn(dyp, x_pad, tap_shifts=[int(s) for s in shifts])
    dw = torch.empty((N, len(shifts) * Cc), dtype=bf16, device=dy.device)
    dyt = transpose(dy)
    for t, sh in enumerate(shifts):
        xt = transpose(x_pad[idx + sh])
        ops.gemm(dyt, xt, None, out=dw[:, t * Cc:(t + 1) * Cc])
    return dw


def groupnorm_bwd(x: torch.Tensor, dz: torch.Tensor, I: int, P: int, gamma: torch.Tensor, beta: torch.Tensor, groups: int,
                  eps: float, dgamma: torch.Tensor, dbeta: torch.Tensor, *, silu: bool = True, dx: Optional[torch.Tensor] = None,
                  accumulate: bool = False, dz_grid=None, img_map: Optional[tuple] = None, return_partials: bool = False):
    """Backward of ops.groupnorm_silu: x [I*P, C] = the forward input, dz = gradient of the forward output - compact
    rows, or (dz_grid) the padded grid the forward wrote into; returns dx [I*P, C] bf16 (accumulate: added to the given dx);
    dgamma / dbeta: fp32 [C] accumulators (see dwm_groupnorm_bwd).
    return_partials: (dx, partials [I, chunks, 2, C]; [..., 0, :] dgamma, [..., 1, :] dbeta) inside ordered_reductions, else (dx, None)."""
    _chk2d(x, "x")
    _chk2d(dz, "dz")
    Cc = x.shape[1]
    rows = dz_grid.rows if dz_grid is not None else I * P
    if not x.is_contiguous() or x.shape[0] != I * P or not dz.is_contiguous() or dz.shape != (rows, Cc):
        raise RuntimeError("groupnorm_bwd: x must be contiguous [I*P, C], dz [rows, C] (rows of the padded grid if dz_grid)")
    for name, t in (("dgamma", dgamma), ("dbeta", dbeta)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != Cc or not t.is_cuda:
            raise RuntimeError(f"groupnorm_bwd: {name} must be a contiguous fp32 CUDA vector of C elements")
    if dx is None:
        if accumulate:
            raise RuntimeError("groupnorm_bwd: accumulate needs dx")
        dx = torch.empty_like(x)
    _chk2d(dx, "dx")
    if dx.shape != x.shape or not dx.is_contiguous():
        raise RuntimeError("groupnorm_bwd: bad dx")
    stats = torch.empty(2 * _lib.load().dwm_groupnorm_stats_floats(I, P, groups), dtype=torch.float32, device=x.device)
    m, im = ops._gn_maps(dz_grid, img_map)
    ws = None
    if ordered_reductions_enabled():
        ws = _ordered_workspace("dwm_groupnorm_bwd_ordered_floats", x.device, I, P, Cc)
        _call("dwm_groupnorm_bwd_ordered", _p(x), _p(dz), _p(dx), I, P, Cc, groups, eps, _p(gamma), _p(beta), int(silu),
              int(accumulate), _p(stats), _p(dgamma), _p(dbeta), C.byref(m), C.byref(im), _p(ws), ws.numel())
        ws = ws.view(I, -1, 2, Cc)
    else:
        _call("dwm_groupnorm_bwd", _p(x), _p(dz), _p(dx), I, P, Cc, groups, eps, _p(gamma), _p(beta), int(silu), int(accumulate),
              _p(stats), _p(dgamma), _p(dbeta), C.byref(m), C.byref(im))
    return (dx, ws) if return_partials else dx
