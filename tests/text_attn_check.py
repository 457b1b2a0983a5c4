"""Checker of the text-encoder attention tests (tests/test_text_kernels_gpu.py; tests/test_text_encoders_cpu.py runs it against a
plain fp32 emulation).  Plain torch, any device; nothing here touches the library.  It is tests/attn_check.py's element bound and
one-hot-V key census restated for dwm_text_attention, whose scores live in the NATURAL-log domain and carry an additive fp32 bias;
the fences are tests/gemm_check.py's.

Reference
---------
fp64 from the same bf16 q / k / v and the same fp32 bias, per (sequence, head):
    x_ij = c <q_i, k_j> + b_ij          c = float32(scale), b = 0 without a bias
    w    = softmax_j(x_ij) over the allowed keys (j < L, and j <= i when causal), 0 elsewhere
    o = w V,  absv = w |V|,  A_ij = <|q_i|, |k_j|>

Element bound on O (derived, not tuned)
---------------------------------------
    rho_ij = 2^-23 (74 c A_ij + |b_ij|) + 4 2^-23 (|x_ij| + max_j |x_ij| + 1)
    e_ij   = expm1(rho_ij + max_j rho_ij)
    bound  = 1.01 (2 2^-8 |o| + 2^-8 absv + (w o e) |V| + (sum_j w e) |o|) + 2 L 2^-23 absv + 2 2^-126 sum_j |V_j|
  * rho, first term - the error of the computed x in its own (natural) unit, which IS the relative error of exp(x): a 64-term fp32
    accumulation is off by at most (K + 8) 2^-23 = 72 2^-23 of the sum of its absolute terms c A (as in gemm_check); the
    multiplication by c rounds once (2^-23 c A at most); THE BIAS ADD rounds once more, by at most 2^-23 |x| <= 2^-23 (c A + |b|) -
    the bias itself is an exact fp32 input.  72 + 1 + 1 = 74 on c A, 1 on |b|: this is the extension of attn_check's rho by the
    fp32 bias add;
  * rho, second term: x - m rounds once (2^-23 (|x| + |m|), |m| <= max_j |x|), the conversion to the exp2 domain multiplies by a
    rounded constant and rounds (1.5 2^-23 of the same), the hardware exp2 is off by about an ulp: 4 2^-23 (|x| + max |x| + 1) in all;
  * e, the 2^-8 terms, the 1.01 and 2 L 2^-23 absv: as in attn_check (numerator and denominator perturbed independently; one bf16
    rounding of the output plus one allowance for a rounded-P denominator; one bf16 rounding of every P entry; fp32 accumulation
    and normalisation of the PV sum);
  * 2 2^-126 per key: an exp2 result and its bf16 rounding below the smallest normal number may be flushed to zero; the row sum is
    >= 1 (the maximum contributes exp(0)), so each flush costs at most 2^-126 |V_j| of the output.  Only the peaked rows (scores
    +-80 through the bias: weights down to e^-160) get anywhere near it.

Key census
----------
One-hot V: V[s L + j, h 64 + (j - 64 c)] = 1 for the keys 64 c <= j < 64 c + 64, everything else 0.  Then out[i, d] IS the weight of
key 64 c + d: every weight within 1.01 w_ij (3 2^-8 + e_ij) + 2 2^-126, excluded keys (past L, causally hidden) and the channels
past the last key EXACTLY 0 - which is what removal by selection gives and a large negative addend does not."""
import math

import torch

from tests.attn_check import _ratios, worst  # noqa: F401  (worst is re-exported)
from tests.gemm_check import U23, fenced, holds_fill, untouched  # noqa: F401  (re-exported)

bf16 = torch.bfloat16
f32 = torch.float32
f64 = torch.float64
U8 = 2.0 ** -8
TINY = 2.0 ** -126
MODES = ("plain", "causal", "bias", "causal_bias")


def heads_view(x, n_seq, L, H):
    """row tensor [n_seq * L, H * 64] -> [n_seq, H, L, 64]"""
    return x.reshape(n_seq, L, H, 64).transpose(1, 2)


def make_inputs(n_seq, L, H, mode, scale, seed, dev):
    """(q, k, v_signature, bias or None) on `dev`.  Score standard deviation ~2.  Row min(3, L - 1) of every head is PEAKED through the
    bias (-80 on every key, +80 on one), row L // 2 is ALL-EQUAL (q = 0, a constant bias row)."""
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
    return q.to(bf16).to(dev), k.to(bf16).to(dev), v.to(bf16).to(dev), bias


def v_onehot(n_seq, L, H, c, dev):
    """the census launch c: V[key j, j - 64 c] = 1 for 64 c <= j < 64 c + 64, in every head of every sequence"""
    v = torch.zeros(n_seq, L, H, 64)
    j = torch.arange(L)
    sel = (j >= 64 * c) & (j < 64 * c + 64)
    v[:, j[sel], :, j[sel] - 64 * c] = 1.0
    return v.reshape(n_seq * L, H * 64).to(bf16).to(dev)


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
        rho = U23 * (74 * abs(c) * A + b.abs()) + 4 * U23 * (x.abs() + xmax + 1)
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
    bound = 1.01 * (2 * U8 * o.abs() + U8 * absv + we @ V.abs() + we.sum(-1, keepdim=True) * o.abs()) + 2 * W.L * U23 * absv \
        + 2 * TINY * V.abs().sum(-2, keepdim=True)
    return o, bound


def element_ratios(got, o, bound, n_seq, L, H):
    return _ratios(heads_view(got, n_seq, L, H), o, bound)


def census_ratios(got, W: Weights, c, n_seq, H):
    """the census launch c against the weights of keys 64 c .. 64 c + 63; where the weight is 0 (excluded keys, channels past the
    last key) anything but an exact 0 gives inf"""
    g = heads_view(got, n_seq, W.L, H).double()
    w, e = W.w[..., 64 * c:64 * c + 64], W.e[..., 64 * c:64 * c + 64]
    pad = 64 - w.shape[-1]
    if pad:
        w, e = torch.nn.functional.pad(w, (0, pad)), torch.nn.functional.pad(e, (0, pad))
    r = _ratios(g, w, 1.01 * w * (3 * U8 + e) + 2 * TINY)
    return torch.where((w == 0) & (g != 0), torch.full_like(r, float("inf")), r)


def emulate(q, k, v, bias, n_seq, L, H, scale, causal, fault=None):
    """what a correct bf16 kernel computes, in plain fp32 torch (P rounded to bf16 in front of PV, fp32 sum of the unrounded p, bf16
    out) - the CPU proof that the bounds admit a correct kernel.  fault: a defect the checks must catch - "one_key_more" (causal: key
    i + 1 visible), "bias_transposed", "no_scale", "addend" (hidden keys get -8 added instead of being removed)."""
    Q, K, V = (heads_view(t, n_seq, L, H).float() for t in (q, k, v))
    x = (1.0 if fault == "no_scale" else torch.tensor(scale, dtype=f32)) * (Q @ K.transpose(-1, -2))
    if bias is not None:
        x = x + (bias.transpose(-1, -2) if fault == "bias_transposed" else bias)[None].float()
    i = torch.arange(L, device=q.device)
    allowed = (i[None, :] <= i[:, None] + (fault == "one_key_more")) if causal else torch.ones(L, L, dtype=torch.bool, device=q.device)
    xm = x - 8.0 * (~allowed) if fault == "addend" else torch.where(allowed, x, torch.full_like(x, float("-inf")))
    p = torch.exp(xm - xm.amax(-1, keepdim=True))
    o = (p.to(bf16).float() @ V) / p.sum(-1, keepdim=True)
    return o.transpose(1, 2).reshape(n_seq * L, H * 64).to(bf16)


def ulp_bf16(x, floor=None):
    """spacing of bf16 at |x| (fp64 tensor), not below `floor` = 2^-126: an fp32 value under the smallest normal number may be
    flushed to zero.  A gated activation passes floor = 2^-126 max(1, |gate|): act(x) is itself such an fp32 value, and what its
    flush loses is multiplied by the gate."""
    e = torch.floor(torch.log2(x.abs().clamp_min(TINY)))
    return torch.maximum(torch.exp2(e - 7), torch.full_like(x, TINY) if floor is None else floor)


def act_reference(x64, kind):
    """fp64 activation in its cancellation-free form: x sigmoid(1.702 x); 0.5 x erfc(-x / sqrt 2) (= x Phi(x)); x sigmoid(2 u),
    u = sqrt(2 / pi) (x + 0.044715 x^3) (= 0.5 x (1 + tanh u))"""
    if kind == "quick_gelu":
        return x64 * torch.sigmoid(1.702 * x64)
    if kind == "gelu":
        return 0.5 * x64 * torch.special.erfc(-x64 / math.sqrt(2.0))
    if kind == "gelu_new":
        return x64 * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x64 + 0.044715 * x64 ** 3))
    raise ValueError(kind)
