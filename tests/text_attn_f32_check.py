"""Checker of the fp32 text-encoder attention tests (tests/test_text_f32_kernels_gpu.py; tests/test_text_f32_cpu.py runs it against
plain fp32 emulations).  Plain torch, any device; nothing here touches the library.  It is tests/text_attn_check.py's element bound
and one-hot-V key census restated for dwm_text_attention_f32: fp32 operands (NOT bf16-representable ones - a kernel that rounds
Q, K, P, V or O to bf16 must fail), unit roundoff u = 2^-24, no bf16 rounding anywhere.

Reference
---------
fp64 from the same fp32 q / k / v and the same fp32 bias, per (sequence, head):
    x_ij = c <q_i, k_j> + b_ij          c = float32(scale), b = 0 without a bias
    w    = softmax_j(x_ij) over the allowed keys (j < L, and j <= i when causal), 0 elsewhere
    o = w V,  absv = w |V|,  A_ij = <|q_i|, |k_j|>

Element bound on O (derived, not tuned)
---------------------------------------
    rho_ij = u (74 c A_ij + |b_ij|) + u (|x_ij| + max_j |x_ij| + 6)
    e_ij   = expm1(rho_ij + max_j rho_ij)
    bound  = 1.01 ((w o e) |V| + (sum_j w e) |o|) + (L + 12) u absv + 2 2^-126 sum_j |V_j|
  * rho, first term - the error of the computed x in its own (natural) unit, which IS the relative error of exp(x): a 64-term fp32
    accumulation, in any order and with or without fused multiply-adds, is off by at most (K + 8) u = 72 u of the sum of its
    absolute terms c A (the count of tests/gemm_check.py, at fp32's unit roundoff); the multiplication by c rounds once (u c A);
    the bias add rounds once more, by at most u |x| <= u (c A + |b|) - the bias itself is an exact fp32 input.  72 + 1 + 1 = 74 on
    c A, 1 on |b|.  This is text_attn_check's rho with 2^-23 (a bf16-input kernel's fp32 ACCUMULATOR, kept generous there)
    replaced by u: here it is the whole budget, nothing else is coarser;
  * rho, second term: x - m rounds once (u (|x| + |m|), |m| <= max_j |x|); the exponential is the library's, within 3 ulp = 6 u of
    the exact function (the accuracy OpenCL demands of exp; the implementation is nearer 1 ulp);
  * e: numerator and denominator are perturbed independently, so a weight is off by at most expm1(rho + max rho) of itself; the
    1.01 covers the second-order terms;
  * (L + 12) u absv - the arithmetic AFTER the exponentials, all of it fp32: the L-term accumulation of p V (L u absv, any order),
    the sum of the p (a tree of 6 + 1 adds of positive terms: 7 u of the sum, i.e. 7 u |o| <= 7 u absv), the normalisation (one
    division, or a reciprocal and a product: 2 u |o|), and 3 u to spare for a kernel that rounds the normalised weight once more.
    THERE IS NO 2^-8 TERM: P is not rounded to bf16 in front of the product and O is stored in fp32.  A kernel that rounds P or O
    to bf16 misses this bound by a factor of about 2^-9 / (L u) = 2^15 / L >= 256;
  * 2 2^-126 per key: an exponential below the smallest normal number may be flushed to zero; the row sum is >= 1 (the maximum
    contributes exp(0)), so each flush costs at most 2^-126 |V_j|.  Only the peaked rows (+-80 through the bias) get near it.

Key census
----------
One-hot V as in text_attn_check: out[i, d] IS the weight of key 64 c + d.  Every weight within 1.01 w_ij e_ij + (L + 12) u w_ij +
2 2^-126; excluded keys (past L, causally hidden) and the channels past the last key EXACTLY 0."""
import torch

from tests import text_attn_check as T
from tests.text_attn_check import MODES, TINY, heads_view, worst  # noqa: F401  (re-exported)
from tests.gemm_check import fenced, untouched  # noqa: F401  (re-exported)

f32 = torch.float32
f64 = torch.float64
U24 = 2.0 ** -24


def make_inputs(n_seq, L, H, mode, scale, seed, dev):
    """text_attn_check.make_inputs without its rounding to bf16: (q, k, v, bias or None) in fp32 on `dev`.  Score standard deviation
    ~2; row min(3, L - 1) of every head PEAKED through the bias (-80 on every key, +80 on one), row L // 2 ALL-EQUAL."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    D = H * 64
    q = torch.randn(n_seq * L, D, generator=g) * (0.25 / scale)
    k = torch.randn(n_seq * L, D, generator=g)
    gv = torch.randn(n_seq * L, H, 64, generator=g)
    q.view(n_seq, L, D)[:, L // 2] = 0
    d = torch.arange(64).view(1, 1, 64)
    h = torch.arange(H).view(1, H, 1)
    s = (torch.arange(n_seq * L) // L).view(-1, 1, 1)
    v = ((0.5 + 1.5 * d / 63) * (1 + 0.5 * h + 0.25 * s) * (1 + 0.25 * gv)).reshape(n_seq * L, D)
    bias = None
    if "bias" in mode:
        bias = torch.randn(H, L, L, generator=g) * 2.0
        r = min(3, L - 1)
        bias[:, r, :] = -80.0
        for hh in range(H):
            bias[hh, r, (5 * hh + 1) % (r + 1 if "causal" in mode else L)] = 80.0
        if L // 2 != r:
            bias[:, L // 2, :] = 0.5
        bias = bias.to(dev)
    assert not torch.equal(q, q.bfloat16().float()) or L == 1              # the operands are not bf16 values
    return q.to(dev), k.to(dev), v.to(dev), bias


def v_onehot(n_seq, L, H, c, dev):
    return T.v_onehot(n_seq, L, H, c, dev).float()


class Weights:
    """w, e [n_seq, H, L, L] fp64 and the allowed-key mask [L, L]"""

    def __init__(self, q, k, bias, n_seq, L, H, scale, causal):
        Q, K = heads_view(q, n_seq, L, H).double(), heads_view(k, n_seq, L, H).double()
        c = float(torch.tensor(scale, dtype=f32))
        b = torch.zeros(1, H, L, L, dtype=f64, device=q.device) if bias is None else bias.double()[None]
        A = Q.abs() @ K.abs().transpose(-1, -2)
        x = c * (Q @ K.transpose(-1, -2)) + b
        i = torch.arange(L, device=q.device)
        self.allowed = (i[None, :] <= i[:, None]) if causal else torch.ones(L, L, dtype=torch.bool, device=q.device)
        zero = torch.zeros_like(x)
        xmax = torch.where(self.allowed, x.abs(), zero).amax(-1, keepdim=True)
        rho = U24 * (74 * abs(c) * A + b.abs()) + U24 * (x.abs() + xmax + 6)
        rho_max = torch.where(self.allowed, rho, zero).amax(-1, keepdim=True)
        self.e = torch.expm1(rho + rho_max)
        self.w = torch.softmax(torch.where(self.allowed, x, torch.full_like(x, float("-inf"))), -1)
        self.L = L


def o_reference(W: Weights, v, n_seq, H):
    """(o, bound) [n_seq, H, L, 64] fp64"""
    V = heads_view(v, n_seq, W.L, H).double()
    o = W.w @ V
    absv = W.w @ V.abs()
    we = W.w * W.e
    bound = 1.01 * (we @ V.abs() + we.sum(-1, keepdim=True) * o.abs()) + (W.L + 12) * U24 * absv + 2 * TINY * V.abs().sum(-2, keepdim=True)
    return o, bound


def element_ratios(got, o, bound, n_seq, L, H):
    return T._ratios(heads_view(got, n_seq, L, H), o, bound)


def frobenius(got, o, n_seq, L, H):
    """relative Frobenius error of the launch against the fp64 reference"""
    g = heads_view(got, n_seq, L, H).double()
    return float((g - o).norm() / o.norm())


def census_ratios(got, W: Weights, c, n_seq, H):
    g = heads_view(got, n_seq, W.L, H).double()
    w, e = W.w[..., 64 * c:64 * c + 64], W.e[..., 64 * c:64 * c + 64]
    pad = 64 - w.shape[-1]
    if pad:
        w, e = torch.nn.functional.pad(w, (0, pad)), torch.nn.functional.pad(e, (0, pad))
    r = T._ratios(g, w, 1.01 * w * e + (W.L + 12) * U24 * w + 2 * TINY)
    return torch.where((w == 0) & (g != 0), torch.full_like(r, float("inf")), r)


def emulate(q, k, v, bias, n_seq, L, H, scale, causal, fault=None):
    """what a correct fp32 kernel computes, in plain fp32 torch - the CPU proof that the bounds admit a correct kernel.  fault: a
    defect the checks must catch - text_attn_check's four ("one_key_more", "bias_transposed", "no_scale", "addend") and
    "bf16_operands": Q, K and P rounded to bf16 in front of their products, the arithmetic of the bf16 kernel"""
    Q, K, V = (heads_view(t, n_seq, L, H).float() for t in (q, k, v))
    if fault == "bf16_operands":
        Q, K = Q.bfloat16().float(), K.bfloat16().float()
    x = (1.0 if fault == "no_scale" else torch.tensor(scale, dtype=f32)) * (Q @ K.transpose(-1, -2))
    if bias is not None:
        x = x + (bias.transpose(-1, -2) if fault == "bias_transposed" else bias)[None].float()
    i = torch.arange(L, device=q.device)
    allowed = (i[None, :] <= i[:, None] + (fault == "one_key_more")) if causal else torch.ones(L, L, dtype=torch.bool, device=q.device)
    xm = x - 8.0 * (~allowed) if fault == "addend" else torch.where(allowed, x, torch.full_like(x, float("-inf")))
    p = torch.exp(xm - xm.amax(-1, keepdim=True))
    pp = p.bfloat16().float() if fault == "bf16_operands" else p
    o = (pp @ V) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(n_seq * L, H * 64)


# ---- activations
def act_exponent(x64, kind):
    """|z|: the size of the argument the activation's exponential (or erfc's e^-a^2) is taken of"""
    if kind == "quick_gelu":
        return (1.702 * x64).abs()
    if kind == "gelu":
        return (-x64).clamp_min(0) ** 2 / 2
    return (1.5957691216057308 * (x64 + 0.044715 * x64 ** 3)).abs()


def act_bound(x64, kind, ref, gate64=None):
    """(6 |z| + 40) u |ref| + 2^-126 max(1, |gate|) - see tests/test_text_f32_kernels_gpu.py"""
    floor = TINY * (gate64.abs().clamp_min(1.0) if gate64 is not None else 1.0)
    return (6 * act_exponent(x64, kind) + 40) * U24 * ref.abs() + floor
