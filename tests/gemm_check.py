"""Shared checker of the GEMM tests (tests/test_gemm_check_cpu.py proves that it bites, tests/test_gemm_fence_gpu.py points it at the
kernels).  Plain torch, any device; nothing here touches the library.

Fences
------
`fenced` hands out an interior view of a larger buffer whose every other element holds a fill:
  * operand fences hold NaN: a fenced value that reaches a stored product (a K loop one step too far, a gate / alpha lookup one
    group too far, a row past M) shows up as a NaN in the result;
  * output fences hold SENTINEL, a fixed NON-canonical NaN bit pattern that no arithmetic produces (hardware and torch emit the
    canonical quiet NaN), compared bit for bit through an integer view by `untouched`: a store past column nout of a partial
    column tile, past row M of a partial row tile or into the gap between nout and ldc changes those bits.  The pattern is a
    NaN as well, so one fence serves both roles where the output is an operand (the in-place forms).

Element bound
-------------
`element_ratio` returns max |got - ref| / bound over the matrix, ref in fp64 from the same (bf16) inputs,

    bound = 2^-8 |ref| + 1.01 L (K + 8) 2^-23 mag + extra        (bf16 outputs)
    bound = 4 * 2^-24 |ref| + L (K + 8) 2^-23 mag                  (fp32 outputs: the fp32 residual stream)

derived, not tuned:
  * round-to-nearest to bf16 (8 significand bits) is off by at most half an ulp, 2^-8 relative at the start of a binade; the
    rounding acts on the computed value, not on ref, hence the factor 1.01 on the other terms;
  * a K-term fp32 accumulation is off by at most one ulp (2^-23) of the sum of the ABSOLUTE terms per addition, whatever the
    order - MFMA's internal truncation and split-K included; `mag` is that absolute sum carried through the epilogue (the
    epilogue formula with every operand replaced by its absolute value, e.g. |res| + |gate| (|A| |W|^T + |bias|)); the 8 are
    the epilogue's own fp32 operations (bias, gate, residual, blend: one rounding each, each of a value below mag);
  * L is the Lipschitz constant of the activation, which scales the error of its argument: 1 for none / relu, 1.1 for silu
    (max |silu'| = 1.0998), 1.13 for both gelus (max |gelu'| = 1.129);
  * extra is what csrc/common.h states about its own approximations: erf by Abramowitz-Stegun 7.1.26, 1.5e-7 absolute, i.e.
    0.75e-7 |x| on gelu = 0.5 x (1 + erf); the hardware v_rcp_f32 and v_exp_f32 behind every sigmoid, one ulp each with a few
    roundings of their arguments: 8 * 2^-23 (|x| + |ref|);
  * GEGLU, out = h gelu(g): the product rule, |gelu(g)| acc_h + 1.13 |h| acc_g with acc = (K + 8) 2^-23 mag of each factor -
    `geglu` returns that sum as its `mag` (L = 1) and |h| times gelu's extra;
  * RMSHEAD: the normalised q / k columns have no element bound (every element depends on its head's 64 sums); `rmshead_check`
    holds each (row, 64-column head) block's relative norm to the suite's kernel tolerance - every block, not the matrix - and
    the v columns to the element bound.
"""
from dataclasses import dataclass

import torch

bf16 = torch.bfloat16
f32 = torch.float32
NAN = float("nan")
# non-canonical NaNs (the canonical quiet NaNs are 0x7fc0 / 0x7fc00000)
SENTINEL = {bf16: 0x7FA5, f32: 0x7FA5A5A5}
_INT_VIEW = {bf16: torch.int16, f32: torch.int32}
LIPSCHITZ = {"none": 1.0, "relu": 1.0, "silu": 1.1, "gelu_tanh": 1.13, "gelu_erf": 1.13}
U23 = 2.0 ** -23


# ------------------------------------------------------------------------------------------------------------------ fences
def _fill(buf, fill):
    if fill == "sentinel":
        buf.view(_INT_VIEW[buf.dtype]).fill_(SENTINEL[buf.dtype])
    else:
        buf.fill_(fill)
    return buf


def fenced(shape, dtype, dev, *, col_off, pad_cols, guard_rows=3, fill=NAN):
    """(view, buffer): `view` is buffer[guard_rows : guard_rows + rows, col_off : col_off + cols] - stride(1) == 1, leading
    dimension col_off + cols + pad_cols - and EVERY element of the buffer, the view's included, holds `fill` (NaN, or "sentinel" =
    SENTINEL as a bit pattern); operands are copied into the view afterwards.  col_off and the leading dimension must be
    multiples of 16 bytes (8 bf16 / 4 fp32 elements), which keeps the view's data pointer 16-byte aligned; a leading dimension
    that has to meet more (the 4-wave kernels want lda % 64 == 0) is the caller's choice of col_off + pad_cols."""
    rows, cols = shape
    q = 16 // torch.empty((), dtype=dtype).element_size()
    ld = col_off + cols + pad_cols
    assert col_off % q == 0 and ld % q == 0, (col_off, ld, q)
    buf = _fill(torch.empty((rows + 2 * guard_rows, ld), dtype=dtype, device=dev), fill)
    view = buf[guard_rows:guard_rows + rows, col_off:col_off + cols]
    assert view.stride(1) == 1 and view.data_ptr() % 16 == 0
    return view, buf


def fenced_vec(n, dtype, dev, *, off=8, fill=NAN):
    """(view, buffer) for a vector operand (bias, alpha, norm weights): a contiguous slice with `off` fill elements on each side"""
    buf = _fill(torch.empty((n + 2 * off,), dtype=dtype, device=dev), fill)
    return buf[off:off + n], buf


def put(view, values):
    view.copy_(values)
    return view


def _fill_bits(dtype, fill):
    if fill == "sentinel":
        return torch.tensor(SENTINEL[dtype], dtype=torch.int64).to(_INT_VIEW[dtype]).item()
    return torch.tensor([fill], dtype=dtype).view(_INT_VIEW[dtype]).item()


def untouched(buffer, view, fill="sentinel"):
    """True if every element of `buffer` outside `view` still holds the fill's exact bits"""
    es = buffer.element_size()
    off = (view.data_ptr() - buffer.data_ptr()) // es
    if buffer.dim() == 1:
        ld, r0, c0, rows, cols = buffer.numel(), 0, off, 1, view.numel()
    else:
        ld = buffer.stride(0)
        r0, c0, (rows, cols) = off // ld, off % ld, view.shape
    ints = buffer.view(_INT_VIEW[buffer.dtype]).reshape(-1, ld)
    want = _fill_bits(buffer.dtype, fill)
    outside = torch.ones(ints.shape, dtype=torch.bool, device=buffer.device)
    outside[r0:r0 + rows, c0:c0 + cols] = False
    return bool((ints[outside] == want).all().item())


def holds_fill(t, fill="sentinel"):
    """True if every element of `t` (e.g. the border rows of a padded output grid) still holds the fill's exact bits"""
    return bool((t.contiguous().view(_INT_VIEW[t.dtype]) == _fill_bits(t.dtype, fill)).all().item())


# ------------------------------------------------------------------------------------------------- fp64 references + mag
@dataclass
class Ref:
    ref: torch.Tensor       # fp64 value of the epilogue
    mag: torch.Tensor       # the same epilogue on absolute values (pre-activation where there is an activation)
    L: float = 1.0          # Lipschitz constant of the activation
    extra: object = 0.0     # absolute allowance for common.h's approximations


def product(a, w):
    """(A W^T, |A| |W|^T) in fp64"""
    a, w = a.double(), w.double()
    return a @ w.T, a.abs() @ w.abs().T


def activate(x, act):
    if act == "none":
        return x
    if act == "relu":
        return torch.relu(x)
    if act == "silu":
        return x * torch.sigmoid(x)
    if act == "gelu_tanh":
        return torch.nn.functional.gelu(x, approximate="tanh")
    if act == "gelu_erf":
        return torch.nn.functional.gelu(x)
    raise ValueError(act)


def act_extra(x, y, act):
    """allowance for the approximations behind y = act(x) (see the module docstring)"""
    if act in ("none", "relu"):
        return torch.zeros_like(x)
    e = 8 * U23 * (x.abs() + y.abs())
    if act == "gelu_erf":
        e = e + 0.75e-7 * x.abs()
    return e


def _pre(prod, bias):
    p, pa = prod
    if bias is not None:
        p, pa = p + bias.double(), pa + bias.double().abs()
    return p, pa


def plain(prod, bias=None, act="none"):
    """act(A W^T + bias); prod = product(a, w)"""
    x, mag = _pre(prod, bias)
    y = activate(x, act)
    return Ref(y, mag, LIPSCHITZ[act], act_extra(x, y, act))


def resid(prod, bias=None, act="none", *, gate=None, rows_per_gate=1, res=None, res_mod=0, blend=None, alpha=None, rows_per_alpha=1):
    """v = act(A W^T + bias); v *= gate[row / rows_per_gate]; v += res[row % res_mod | row / -res_mod | row];
    v = alpha blend + (1 - alpha) v with alpha[row / rows_per_alpha]"""
    x, mag = _pre(prod, bias)
    v = activate(x, act)
    extra = act_extra(x, v, act)
    rows = torch.arange(x.shape[0], device=x.device)
    if gate is not None:
        g = gate.double()[rows // rows_per_gate]
        v, mag, extra = v * g, mag * g.abs(), extra * g.abs()
    if res is not None:
        r = res.double()[rows % res_mod if res_mod > 0 else rows // -res_mod if res_mod < 0 else rows]
        v, mag = v + r, mag + r.abs()
    if blend is not None:
        al = alpha.double()[rows // rows_per_alpha][:, None]
        v = al * blend.double() + (1 - al) * v
        mag = al.abs() * blend.double().abs() + (1 - al).abs() * mag
        extra = extra * (1 - al).abs()
    return Ref(v, mag, LIPSCHITZ[act], extra)


def geglu(prod, bias=None):
    """out[:, j] = h_j gelu_erf(g_j), [h | g] = the two halves of A W^T + bias (W / bias UNPACKED: value rows, then gate rows)"""
    x, mag = _pre(prod, bias)
    n2 = x.shape[1] // 2
    h, g, mh, mg = x[:, :n2], x[:, n2:], mag[:, :n2], mag[:, n2:]
    y = activate(g, "gelu_erf")
    return Ref(h * y, y.abs() * mh + LIPSCHITZ["gelu_erf"] * h.abs() * mg, 1.0, h.abs() * act_extra(g, y, "gelu_erf"))


def rmshead(prod, bias, rms_w, rms_ncols, eps):
    """columns < rms_ncols: per 64-column head x rsqrt(mean(x^2) + eps) w; the others x.  mag is meaningful for the others only."""
    x, mag = _pre(prod, bias)
    M = x.shape[0]
    qk = x[:, :rms_ncols].reshape(M, -1, 64)
    qk = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + eps) * rms_w.double().view(-1, 64)
    return Ref(torch.cat([qk.reshape(M, rms_ncols), x[:, rms_ncols:]], 1), mag)


# ------------------------------------------------------------------------------------------------------------- the bound
def element_ratios(got, ref, mag, K, L=1.0, extra=0):
    """|got - ref| / bound per element (fp64); a non-finite `got` gives inf"""
    ref, mag = ref.double(), mag.double()
    acc = L * (K + 8) * U23 * mag
    if got.dtype == f32:
        # the fp32 stream carries no activation (RESID on C32 is launched without one): there is no allowance to add, and one
        # that is asked for must not be dropped silently
        assert not torch.is_tensor(extra) or not bool(extra.any()), "the fp32 bound has no `extra` term"
        assert torch.is_tensor(extra) or extra == 0, "the fp32 bound has no `extra` term"
        bound = 4 * 2.0 ** -24 * ref.abs() + acc
    else:
        bound = 2.0 ** -8 * ref.abs() + 1.01 * acc + extra
    g = got.double()
    r = (g - ref).abs() / bound.clamp_min(1e-300)
    r = torch.where((g - ref) == 0, torch.zeros_like(r), r)
    return torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))


def element_ratio(got, ref, mag, K, L=1.0, extra=0):
    """max |got - ref| / bound (see the module docstring); <= 1 passes"""
    r = element_ratios(got, ref, mag, K, L, extra)
    return r.max().item() if r.numel() else 0.0


def check(got, r: Ref, K):
    return element_ratio(got, r.ref, r.mag, K, r.L, r.extra)


def worst(got, r: Ref, K, n=20):
    """the n worst elements as (row, column, got, ref, bound ratio) - what a failing test prints"""
    ratios = element_ratios(got, r.ref, r.mag, K, r.L, r.extra)
    flat = ratios.reshape(-1)
    idx = torch.topk(flat, min(n, flat.numel())).indices
    cols = ratios.shape[1]
    return [(int(i) // cols, int(i) % cols, got.reshape(-1)[i].item(), r.ref.reshape(-1)[i].item(), flat[i].item()) for i in idx]


def rmshead_check(got, r: Ref, K, rms_ncols):
    """(worst relative norm error of a (row, 64-column head) block of the normalised columns, element ratio of the others)"""
    M = got.shape[0]
    g = got[:, :rms_ncols].double().reshape(M, -1, 64)
    w = r.ref[:, :rms_ncols].reshape(M, -1, 64)
    blocks = (g - w).norm(dim=-1) / w.norm(dim=-1).clamp_min(1e-30)
    blocks = torch.where(torch.isfinite(blocks), blocks, torch.full_like(blocks, float("inf")))
    worst_block = blocks.max().item() if blocks.numel() else 0.0
    v = got[:, rms_ncols:]
    ratio = element_ratio(v, r.ref[:, rms_ncols:], r.mag[:, rms_ncols:], K) if v.shape[1] else 0.0
    return worst_block, ratio
