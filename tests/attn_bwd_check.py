"""Shared checker of the attention-backward tests (tests/test_attn_bwd_check_cpu.py proves that it bites,
tests/test_attention_bwd_fence_gpu.py points it at the kernels).  Plain torch, any device; nothing here touches the library.  Cases,
problems, row-map gathering, masks, `fold` and the forward's `scores` are tests/attn_check.py's, the fences tests/gemm_check.py's.

The operation under test (csrc/attention_bwd.hip as it stands)
---------------------------------------------------------------
A launch is a function of (q, k, v, O, lse, dO, masks) - NOT the derivative of an ideal attention:
  * c = float32(scale) * float32(log2 e) (attn_check.fold_constant); `lse` is the forward's saved NEGATIVE log2-domain log-sum-exp,
    fp32 [P, H, L0 + L1] (cross: only the L0 query entries are defined); O is the forward's bf16 output;
  * D_i = sum_d dO_id O_id from the given bf16 O (delta_kernel), fp32;
  * attn_dq_kernel:   s = Q'' k^T with Q'' = bf16_rne(fp32(q) c) = fold(q),  P = 2^(s + lse),  dS = P (dO V^T - D),
                      dQ = scale (bf16(dS) k)               (raw k, fp32 sum, fp32 * scale, one bf16 rounding)
  * attn_dkv_kernel:  s = q K''^T with K'' = fold(k),  the same P and dS formulas on THAT s,
                      dK = scale (bf16(dS)^T q),  dV = bf16(P)^T dO     (raw q)
  * a pair the mask forbids has P = 0 exactly; no row sum is taken anywhere: P rests on the given lse alone.
So dQ comes from one P matrix and dK / dV from a slightly different one.  `reference` evaluates exactly these formulas in fp64, per
(problem, head), gathered through the row map - each output with the folded operand of its own kernel.
`ideal_gradients` is the same formula without any folding or rounding: tests/test_attn_bwd_check_cpu.py holds it to fp64 autograd
through a plain softmax attention (~1e-12), which proves that the formula is the right operation.

Element bounds (derived, not tuned)
-----------------------------------
u23 = 2^-23 (fp32), u8 = 2^-8 (one round-to-nearest to bf16, relative).  For the pair (i, j) of one kernel, with A = |operand||operand|^T
of the scores, B = |dO| |V|^T, absD_i = sum_d |dO_id O_id|:
    rho_ij = ln2 (72 u23 (A_ij + |lse_i|) + 4 u23 (|s_ij| + |lse_i| + 1))        e_ij = expm1(rho_ij)
    x_ij   = 72 u23 (B_ij + |D_i|) + 12 u23 absD_i
    eP_ij  = P_ij (e_ij (1 + u8) + u8) + TINY
    eS_ij  = (|dS_ij| (e_ij + 2 u23) + P_ij (1 + e_ij) x_ij) (1 + u8) + u8 |dS_ij| + TINY
  * rho: the 64-term fp32 score accumulation starts from the C-init lse, so it is off by at most (64 + 8) u23 of the sum of its
    absolute terms, A_ij + |lse_i| (as gemm_check counts an accumulation); the hardware exp2 is good to an ulp on an argument of
    size |s - lse| (4 u23 (|s| + |lse| + 1), as the forward's); ln 2 turns a log2-domain error into a relative one of P.  lse is an
    INPUT here: unlike the forward there is no denominator term.  A large |lse| costs 76 u23 ln2 |lse| of P and no more.
  * x: the error of dP - D: a 64-term fp32 accumulation with C-init -D, (64 + 8) u23 (B_ij + |D_i|), plus the fp32 error of D
    itself: delta_kernel sums 8 products in sequence and combines 8 lanes with three shuffles - at most 11 roundings on the way of
    any term, 12 u23 absD_i taken.
  * eP: P (1 + e) rounded once to bf16 (the dV MFMA's operand).  eS: dS = P (dP - D) in fp32 (two roundings: the product, and one
    spare), then once to bf16 (the dQ / dK MFMAs' operand).  TINY = 2^-120 lets a P below the fp32 normal range flush to zero.
    dS sums to ~0 along a row, so nothing here is relative to a RESULT: everything is relative to the entries.
With n = 64 (tiles walked) + 8 terms per fp32 accumulation of the second MFMA (the 8: the final fp32 * scale and spares) and one
bf16 rounding of the stored gradient:
    bound_dQ = scale (eS_q |k| + n u23 (|dS_q| + eS_q) |k|) (1 + u8) + u8 |dQ|       [walks the key tiles]
    bound_dK = scale (eS_k^T |q| + n u23 (|dS_k| + eS_k)^T |q|) (1 + u8) + u8 |dK|   [walks the query tiles]
    bound_dV = (eP_k^T |dO| + n u23 (P_k + eP_k)^T |dO|) (1 + u8) + u8 |dV|
How large these come out against the gradients is MEASURED (tests/test_attn_bwd_check_cpu.py::test_bounds_against_the_gradients
prints it): with the inputs below the median bound is 0.8 % of the row's root mean square for dV and 3.5 / 2.4 / 1.3 % for dQ and dK
at qs = 0.25 / 1 / 3 (dS cancels along a row, the more the flatter the softmax); the emulation of the rounding points reaches
0.58 - 0.85 of the element bounds and 0.47 - 0.49 of the census bounds.

Inputs
------
q, k Gaussian (q times qs in attn_check.QS); V = Problem.v_signature (positive, a signature per column, head and problem);
dO = the same kind of signature with other constants and a fixed sign per column (-1 where d % 4 == 3): no cancellation inside
dV = P^T dO, and a wrong row, column, head or problem of V or dO is many bounds off.
Isolated mode (primary): O and lse come from the fp64 forward reference of the very inputs (attn_check.scores on fold(q) and k),
O rounded once to bf16, lse once to fp32, so the backward is tested on exactly known inputs.  Chained mode: O and lse come from the
library's forward (which tests/test_attention_fence_gpu.py holds to its own bounds) and are GIVEN inputs of the same reference.

Three census probes
-------------------
Each reads one matrix entry per output element and demands EXACT zeros where the kernel must select rather than add:
  * dV census, launch c: dO[i, i - 64 c] = 1 for the queries 64 c .. 64 c + 63 in every head, 0 elsewhere.  Then
    dV[j, d] = bf16(P_k[64 c + d, j]): ceil(Lq / 64) launches read out all of P^T as the key side sees it; bound eP (1 + u8) + u8 P.
  * dQ census, launch c: K[j, j - 64 c] = 1 for the keys 64 c .. 64 c + 63, the other keys zero rows.  Then
    dQ[i, d] = scale bf16(dS_q[i, 64 c + d]); bound scale eS_q (1 + u8) + u8 |dQ|.
  * dK census, launch c: Q one-hot over the query chunk c.  Then dK[j, d] = scale bf16(dS_k[64 c + d, j]); the same bound on eS_k.
(The u8 of the output rounding is kept although a bf16 value times a power-of-two scale stores exactly: the scale is an argument.)
Masked pairs and the channels past the last query / key must be exactly 0.  A dropped pair is 100 % off on its own entry, a
duplicated one 2 x, a counted pad query or pad key is a nonzero where 0 is demanded.  O and lse of a census launch are the forward
reference of THAT launch's inputs.

Fences: `BwdFenced`, below."""
from dataclasses import dataclass

import torch

from tests import attn_check as A
from tests.attn_check import (GAP, LN2, NAN, QS, SENTINEL, U8, U23, Problem, fenced, fenced_vec, fold, fold_constant,  # noqa: F401
                              holds_fill, scores, untouched, worst)

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
TINY = 2.0 ** -120
LADDER_T = (-120, -12, 0, 19, 90)
NEVER_ATTENDED_KEY = 9


# ------------------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class BCase(A.Case):
    """attn_check.Case plus: below (the segment-1 gradients lie BELOW segment 0 in their allocation: a negative dq1 - dq0), chained
    (O and lse from the library's forward), census (False: the three element checks only)"""
    below: bool = False
    chained: bool = False
    census: bool = True


def _cases():
    c = []
    ident = lambda P, L: ("identity", (P, L))
    # lengths; (problems, heads) chosen for the workgroup counts P * H * ceil(L / 128): 4 8 9 10 6 21 4 12 15 8 30 27
    for L, P, H in ((1, 2, 2), (31, 4, 2), (32, 3, 3), (33, 5, 2), (63, 2, 3), (64, 7, 3), (65, 2, 2), (127, 4, 3), (128, 5, 3), (129, 2, 2),
                    (193, 5, 3), (257, 3, 3)):
        c.append(BCase("lengths", f"L{L}", ident(P, L), H, twice=(L == 257)))
    # two segments: the seam inside a tile, at a tile edge, in the second block; segment-1 gradients above and below segment 0
    for i, (L0, L1) in enumerate(((33, 32), (64, 1), (100, 10), (127, 2), (130, 65))):
        c.append(BCase("two_segments", f"L{L0}+{L1}", ident(2 + i % 2, L0), 3 - i % 2, L1=L1, below=bool(i % 2)))
    # cross-attention: dq blocks over Lq, dk / dv blocks over Lk, kbeg = L0
    for i, (Lq, Lk) in enumerate(((1, 1), (33, 77), (130, 65), (65, 130))):
        c.append(BCase("cross", f"Lq{Lq}_Lk{Lk}", ident(3 - i % 2, Lq), 2 + i % 2, L1=Lk, cross=True))
    # row maps
    c.append(BCase("rowmaps", "rowwise_Tw65", ("temporal_rowwise", (1, 5, 1, 3, 13)), 2))
    c.append(BCase("rowmaps", "pointwise_T5", ("temporal_pointwise", (1, 5, 2, 1, 3)), 3))
    c.append(BCase("rowmaps", "pointwise_T17", ("temporal_pointwise", (1, 17, 1, 1, 5)), 2))
    for i, V in enumerate((3, 4, 6, 8)):
        for j, w in enumerate((8, 11)):
            c.append(BCase("group_mask", f"V{V}_w{w}", ("crossview_rowwise", (2, 1, V, 2 if V == 6 else 1, w)), 2 + (i + j) % 2, mask="group"))
    c.append(BCase("group_mask", "full_V3", ("crossview_full", (2, 1, 3, 2, 7)), 2, mask="group"))
    # dense masks: a row -> key 0 only, a row -> one key of the ragged last tile only, one key that NO query attends
    c.append(BCase("dense_mask", "L65", ident(2, 65), 2, mask="dense"))
    c.append(BCase("dense_mask", "L129", ident(2, 129), 3, mask="dense"))
    c.append(BCase("dense_mask", "L100+10", ident(2, 100), 2, L1=10, mask="dense", below=True))
    # score offsets: rows at t in LADDER_T
    c.append(BCase("score_offsets", "L129", ident(2, 129), 2, ladder=32))
    # chained: O and lse from the library's forward
    c.append(BCase("chained", "L129", ident(2, 129), 2, chained=True, census=False))
    c.append(BCase("chained", "L100+10", ident(2, 100), 3, L1=10, chained=True, census=False))
    c.append(BCase("chained", "group_full_V3", ("crossview_full", (2, 1, 3, 2, 7)), 2, mask="group", chained=True, census=False))
    c.append(BCase("chained", "dense_L65", ident(2, 65), 2, mask="dense", chained=True, census=False))
    c.append(BCase("chained", "cross_Lq33_Lk77", ident(2, 33), 3, L1=77, cross=True, chained=True, census=False))
    return c


CASES = _cases()


def workgroups(case: BCase, n_problems: int, L0: int):
    """(dq, dkv) workgroup counts of a launch, as launch_bwd computes them"""
    qend = L0 if case.cross else L0 + case.L1
    nkeys = case.L1 if case.cross else L0 + case.L1
    return n_problems * case.heads * ((qend + 127) // 128), n_problems * case.heads * ((nkeys + 127) // 128)


# ------------------------------------------------------------------------------------------------------------------ inputs
class BwdProblem(Problem):
    """attn_check.Problem plus the backward's inputs.  The dense mask gets one key that no query attends; the ladder puts the rows
    of every (problem, head) at the offsets LADDER_T in turn."""

    def __init__(self, case, rowmap, dev, scale: float = 0.125):
        super().__init__(case, rowmap, dev, scale)
        seed = 5000 + 11 * CASES.index(case) if case in CASES else 4999
        self.gd0, self.gd1 = A._gauss((self.R0, self.D), seed), A._gauss((self.P * self.L1, self.D), seed + 1)

    def _dense_mask(self, seed):
        super()._dense_mask(seed)
        j = NEVER_ATTENDED_KEY
        m = self.dense_mask.clone()
        m[:, :, j] = False
        m[:, j, 0] = True                                    # its own query still attends something
        self.dense_mask = self.allowed = m

    def ladder_t(self, qs):
        if qs not in self._t:
            t = torch.tensor([LADDER_T[i % len(LADDER_T)] for i in range(self.L0)])
            self._t[qs] = t.view(1, 1, self.L0).expand(self.P, self.H, self.L0).contiguous()
        return self._t[qs]

    def do_signature(self):
        """sign(d) (1.5 - d / 63) (1 + 0.25 h + 0.5 p) (1 + 0.25 gauss), sign = -1 where d % 4 == 3"""
        d = torch.arange(64).view(1, 1, 64)
        h = torch.arange(self.H).view(1, self.H, 1)
        sign = torch.where(d % 4 == 3, -1.0, 1.0)
        out = []
        for g, p in ((self.gd0, self.p0), (self.gd1, self.p1)):
            sig = sign * (1.5 - d / 63) * (1 + 0.25 * h + 0.5 * p.view(-1, 1, 1)) * (1 + 0.25 * g.view(-1, self.H, 64))
            out.append(sig.reshape(-1, self.D).to(bf16).to(self.dev))
        return tuple(out)

    def chunks(self, part):
        return ((self.Lq if part == "q" else self.Lk) + 63) // 64

    def onehot(self, c, part):
        """row tensors (segment 0, segment 1) that hold x[token l, l - 64 c] = 1 for 64 c <= l < 64 c + 64 in every head; part "q":
        l = the query position, "k": the key position (cross: the rows of the other side stay zero)"""
        out = []
        for l, n, has in ((self.l0, self.R0, not (self.cross and part == "k")), (self.l1, self.P * self.L1, not (self.cross and part == "q"))):
            x = torch.zeros(n, self.H, 64)
            if has and n:
                sel = (l >= 64 * c) & (l < 64 * c + 64)
                x[sel, :, (l[sel] - 64 * c)] = 1.0
            out.append(x.reshape(n, self.D).to(bf16).to(self.dev))
        return tuple(out)

    def scatter(self, x, out0, out1, part):
        """x [P, H, L, 64] -> the row tensors (part "q": query rows, "k": key rows)"""
        x = x.transpose(1, 2)
        if self.cross:
            if part == "q":
                out0[self.rows.reshape(-1)] = x.reshape(-1, self.D).to(out0.dtype)
            else:
                out1.copy_(x.reshape(-1, self.D))
            return
        out0[self.rows.reshape(-1)] = x[:, :self.L0].reshape(-1, self.D).to(out0.dtype)
        if self.L1:
            out1.copy_(x[:, self.L0:].reshape(-1, self.D))

    def allowed4(self):
        """[P, 1, Lq, Lk] bool"""
        if self.allowed is None:
            return torch.ones(self.P, 1, self.Lq, self.Lk, dtype=torch.bool, device=self.dev)
        return self.allowed[:, None]

    def forward_reference(self, q, k, v):
        """(O row tensors bf16, lse [P, H, L0 + L1] fp32 with NaN in the undefined key entries of a cross launch) from the fp64
        forward of the inputs as launched: scores of fold(q) and k, lse = -log2 sum 2^s"""
        Qg = self.gather(fold(q[0], self.scale), fold(q[1], self.scale), "q")
        S = scores(self, Qg, self.gather(*k, "k"))
        o = S.w @ self.gather(*v, "k").double()
        O0 = torch.zeros(self.R0, self.D, dtype=bf16, device=self.dev)
        O1 = torch.zeros(self.P * self.L1, self.D, dtype=bf16, device=self.dev)
        self.scatter(o, O0, O1, "q")
        lse = torch.full((self.P, self.H, self.L0 + self.L1), NAN, dtype=f32, device=self.dev)
        lse[:, :, :self.Lq] = S.lse.float()
        return (O0, O1), lse


# --------------------------------------------------------------------------------------------------------------- reference
@dataclass
class Side:
    """one kernel's view of the pairs: [P, H, Lq, Lk] fp64"""
    P: torch.Tensor
    dS: torch.Tensor
    eP: torch.Tensor
    eS: torch.Tensor


@dataclass
class Ref:
    q: Side                    # attn_dq_kernel: scores of fold(q) and raw k
    k: Side                    # attn_dkv_kernel: scores of raw q and fold(k)
    dq: torch.Tensor           # [P, H, Lq, 64]
    dk: torch.Tensor           # [P, H, Lk, 64]
    dv: torch.Tensor
    bound: dict                # name -> bound, shaped like the gradient
    allowed: torch.Tensor      # [P, 1, Lq, Lk]
    scale: float


def _side(Qs, Ks, lse, allowed, X, x_err):
    """P, dS and their entry errors from the score operands of one kernel (see the module docstring)"""
    s = Qs @ Ks.transpose(-1, -2)
    Aabs = Qs.abs() @ Ks.abs().transpose(-1, -2)
    la = lse.abs()[..., None]
    rho = LN2 * (72 * U23 * (Aabs + la) + 4 * U23 * (s.abs() + la + 1))
    e = torch.expm1(rho)
    P = torch.where(allowed, torch.exp2(s + lse[..., None]), torch.zeros_like(s))
    dS = P * X
    eP = P * (e * (1 + U8) + U8) + TINY
    eS = (dS.abs() * (e + 2 * U23) + P * (1 + e) * x_err) * (1 + U8) + U8 * dS.abs() + TINY
    zero = torch.zeros_like(P)
    return Side(P, dS, torch.where(allowed, eP, zero), torch.where(allowed, eS, zero))


def reference(prob: BwdProblem, Qg, Kg, Vg, Og, dOg, lse_q) -> Ref:
    """the operation of the module docstring in fp64.  Qg, Og, dOg [P, H, Lq, 64], Kg, Vg [P, H, Lk, 64] gathered bf16 inputs,
    lse_q [P, H, Lq] fp32 (the NEGATIVE log2-domain log-sum-exp as given to the launch)"""
    sc = prob.scale
    c = fold_constant(sc).to(Qg.device)
    Q, K, V, O, dO, lse = Qg.double(), Kg.double(), Vg.double(), Og.double(), dOg.double(), lse_q.double()
    Qf, Kf = (Qg.float() * c).to(bf16).double(), (Kg.float() * c).to(bf16).double()
    allowed = prob.allowed4().to(Qg.device)
    D = (dO * O).sum(-1)
    absD = (dO * O).abs().sum(-1)
    X = dO @ V.transpose(-1, -2) - D[..., None]
    B = dO.abs() @ V.abs().transpose(-1, -2)
    x_err = 72 * U23 * (B + D.abs()[..., None]) + 12 * U23 * absD[..., None]
    sq = _side(Qf, K, lse, allowed, X, x_err)
    sk = _side(Q, Kf, lse, allowed, X, x_err)
    nk = 64 * ((K.shape[-2] + 63) // 64) + 8           # dq walks the key tiles
    nq = 64 * ((Q.shape[-2] + 63) // 64) + 8           # dk / dv walk the query tiles
    dq = sc * (sq.dS @ K)
    dk = sc * (sk.dS.transpose(-1, -2) @ Q)
    dv = sk.P.transpose(-1, -2) @ dO
    T = lambda t: t.transpose(-1, -2)
    bound = dict(
        dq=sc * (sq.eS @ K.abs() + nk * U23 * ((sq.dS.abs() + sq.eS) @ K.abs())) * (1 + U8) + U8 * dq.abs(),
        dk=sc * (T(sk.eS) @ Q.abs() + nq * U23 * (T(sk.dS.abs() + sk.eS) @ Q.abs())) * (1 + U8) + U8 * dk.abs(),
        dv=(T(sk.eP) @ dO.abs() + nq * U23 * (T(sk.P + sk.eP) @ dO.abs())) * (1 + U8) + U8 * dv.abs())
    return Ref(sq, sk, dq, dk, dv, bound, allowed, sc)


def ideal_gradients(Q, K, V, O, dO, lse, allowed, scale):
    """the same formula on exact fp64 operands without folding: s = c Q K^T in the log2 domain, P = 2^(s + lse); (dQ, dK, dV)"""
    c = scale / LN2
    s = c * (Q @ K.transpose(-1, -2))
    P = torch.where(allowed, torch.exp2(s + lse[..., None]), torch.zeros_like(s))
    D = (dO * O).sum(-1, keepdim=True)
    dS = P * (dO @ V.transpose(-1, -2) - D)
    return scale * (dS @ K), scale * (dS.transpose(-1, -2) @ Q), P.transpose(-1, -2) @ dO


def _pad64(t):
    """the last dimension filled up to 64 with zeros (False)"""
    pad = 64 - t.shape[-1]
    return t if not pad else torch.cat([t, torch.zeros(t.shape[:-1] + (pad,), dtype=t.dtype, device=t.device)], -1)


def census_ratios(got_g, R: Ref, which: str, c: int):
    """the census launch c of `which` in ("dv", "dq", "dk") (module docstring): got_g = that gradient gathered [P, H, L, 64]; channel d
    against the matrix entry it must hold; where 0 is demanded (masked pairs, channels past the end) any other value gives inf"""
    sl = slice(64 * c, 64 * c + 64)
    if which == "dq":                                   # dQ[i, d] = scale dS_q[i, 64 c + d]
        val, err, ok = R.scale * R.q.dS[..., sl], R.scale * R.q.eS[..., sl], R.allowed[..., sl]
    else:                                               # d*[j, d] = entry [64 c + d, j]: transpose the query chunk
        src, e = (R.k.P, R.k.eP) if which == "dv" else (R.scale * R.k.dS, R.scale * R.k.eS)
        val, err, ok = src[..., sl, :].transpose(-1, -2), e[..., sl, :].transpose(-1, -2), R.allowed[..., sl, :].transpose(-1, -2)
    ok = ok.expand(val.shape)
    val, err, ok = _pad64(val), _pad64(err), _pad64(ok)
    r = A._ratios(got_g, val, err * (1 + U8) + U8 * val.abs())
    return torch.where(~ok & (got_g.double() != 0), torch.full_like(r, float("inf")), r)


# ---------------------------------------------------------------------------------------------------------------- fences
class BwdFenced:
    """the buffers of one backward launch:
      * q / k / v as column slices of ONE NaN-fenced [R0 + GAP + P L1, 3 D + 64] buffer (segment 0, GAP NaN rows, segment 1), NaN in
        the guards and pad columns; cross: the key / value columns of segment 0 and the query columns of segment 1 stay NaN;
      * O and dO each as views of a NaN-fenced buffer at column offset 8 with ldo = D + 16 (cross: segment 0 only);
      * lse [P, H, L0 + L1] fp32 as a slice of a NaN-fenced vector (cross: the key entries stay NaN);
      * dq / dk / dv as column slices of ONE sentinel-filled [rows + guards, 3 D + 40] buffer at column offset 16, the views included;
        segment 1 shares the allocation, ABOVE segment 0 (below=False) or BELOW it (a negative dq1 - dq0), GAP rows between them;
        cross: dq is the query rows' first D columns, dk / dv the key rows' other columns, the rest must keep the sentinel.
    Fill the forward's results with `set_forward`, or let a forward write O0 / O1 / lse, then `freeze`; `violations` lists what the
    backward launch broke: a changed input or fence, an unwritten or non-finite gradient, a write anywhere else."""

    def __init__(self, prob: BwdProblem, q, k, v, dO, below=False):
        self.prob = prob
        D, R0, R1 = prob.D, prob.R0, prob.P * prob.L1
        dev = prob.dev
        self.iview, self.ibuf = fenced((R0 + GAP + R1, 3 * D), bf16, dev, col_off=16, pad_cols=48)
        seg0, seg1 = self.iview[:R0], self.iview[R0 + GAP:]
        for i, (x0, x1) in enumerate((q, k, v)):
            if not (prob.cross and i > 0):
                seg0[:, i * D:(i + 1) * D] = x0
            if R1 and not (prob.cross and i == 0):
                seg1[:, i * D:(i + 1) * D] = x1
        self.q0, self.k0, self.v0 = (seg0[:, i * D:(i + 1) * D] for i in range(3))
        self.q1, self.k1, self.v1 = (seg1[:, i * D:(i + 1) * D] for i in range(3)) if R1 else (None, None, None)
        R1o = 0 if prob.cross else R1
        self.R1o = R1o
        orows = R0 + (GAP + R1o if R1o else 0)
        self.oview, self.obuf = fenced((orows, D), bf16, dev, col_off=8, pad_cols=8)
        self.dview, self.dbuf = fenced((orows, D), bf16, dev, col_off=8, pad_cols=8)
        self.O0, self.dO0 = self.oview[:R0], self.dview[:R0]
        self.O1, self.dO1 = (self.oview[R0 + GAP:], self.dview[R0 + GAP:]) if R1o else (None, None)
        self.dO0.copy_(dO[0])
        if R1o:
            self.dO1.copy_(dO[1])
        self.lse, self.lbuf = fenced_vec(prob.lse_len(), f32, dev, off=8)
        # gradients
        self.below = below and R1 > 0
        self.gview, self.gbuf = fenced((R0 + (GAP + R1 if R1 else 0), 3 * D), bf16, dev, col_off=16, pad_cols=24, fill="sentinel")
        if self.below:
            g1, self.ggap, g0 = self.gview[:R1], self.gview[R1:R1 + GAP], self.gview[R1 + GAP:]
        else:
            g0 = self.gview[:R0]
            g1, self.ggap = (self.gview[R0 + GAP:], self.gview[R0:R0 + GAP]) if R1 else (None, None)
        self.g0, self.g1 = g0, g1
        self.dq0, self.dk0, self.dv0 = (g0[:, i * D:(i + 1) * D] for i in range(3))
        self.dq1, self.dk1, self.dv1 = (g1[:, i * D:(i + 1) * D] for i in range(3)) if R1 else (None, None, None)
        self.frozen = None

    def set_forward(self, O, lse):
        self.O0.copy_(O[0])
        if self.R1o:
            self.O1.copy_(O[1])
        self.lse.copy_(lse.reshape(-1))
        return self.freeze()

    def freeze(self):
        self.frozen = [b.clone() for b in (self.ibuf, self.obuf, self.dbuf, self.lbuf)]
        return self

    def grads(self):
        """((dq0, dq1), (dk0, dk1), (dv0, dv1)) as Problem.gather takes them (cross: dq1 / dk0 / dv0 are not outputs)"""
        return (self.dq0, self.dq1), (self.dk0, self.dk1), (self.dv0, self.dv1)

    def written(self):
        """name -> the views the launch must have written"""
        if self.prob.cross:
            return dict(dq=self.dq0, dk=self.dk1, dv=self.dv1)
        w = dict(dq=self.dq0, dk=self.dk0, dv=self.dv0)
        if self.g1 is not None:
            w.update(dq1=self.dq1, dk1=self.dk1, dv1=self.dv1)
        return w

    def violations(self):
        bad = []
        assert self.frozen is not None
        for name, b, was in zip(("q / k / v", "O", "dO", "lse"), (self.ibuf, self.obuf, self.dbuf, self.lbuf), self.frozen):
            iv = torch.int16 if b.dtype == bf16 else torch.int32
            if not torch.equal(b.view(iv), was.view(iv)):
                bad.append(f"the input {name} or its fence was written")
        if not untouched(self.gbuf, self.gview):
            bad.append("gradient fence touched")
        if self.ggap is not None and not holds_fill(self.ggap):
            bad.append("rows between the two segments' gradients written")
        if self.prob.cross:
            D = self.prob.D
            if not holds_fill(self.g0[:, D:]):
                bad.append("cross: dk / dv columns of the query rows written")
            if not holds_fill(self.g1[:, :D]):
                bad.append("cross: dq columns of the key rows written")
        for name, t in self.written().items():
            if not bool(torch.isfinite(t).all()):
                bad.append(f"NaN / Inf / unwritten elements in {name}: rows {torch.nonzero(~torch.isfinite(t).all(1)).flatten()[:8].tolist()}")
        return bad


# ---------------------------------------------------------------------------------------------------------------- the run
def run_case(prob: BwdProblem, harness):
    """every check of one case.  harness.backward(F) runs the kernels (or the emulation) on a frozen BwdFenced and does its own fence
    checks; harness.forward(F) (chained cases) lets the forward write F.O0 / F.O1 / F.lse.  Returns {check: (worst ratio, where)};
    "repeat_bit_equal" is 0.0 / inf."""
    case = prob.case
    res = {}

    def note(name, ratios, **kw):
        r, at = worst(ratios)
        if name not in res or r > res[name][0]:
            res[name] = (r, dict(at=at, **kw))

    def launch(q, k, v, dO):
        F = BwdFenced(prob, q, k, v, dO, below=case.below)
        if case.chained:
            harness.forward(F)
            F.freeze()
        else:
            F.set_forward(*prob.forward_reference(q, k, v))
        harness.backward(F)
        R = reference(prob, prob.gather(F.q0, F.q1, "q"), prob.gather(F.k0, F.k1, "k"), prob.gather(F.v0, F.v1, "k"),
                      prob.gather(F.O0, F.O1, "q"), prob.gather(F.dO0, F.dO1, "q"), prob.lse_queries(F.lse))
        return F, R

    def gathered(F):
        gq, gk, gv = F.grads()
        return dict(dq=prob.gather(*gq, "q"), dk=prob.gather(*gk, "k"), dv=prob.gather(*gv, "k"))

    k = (prob.k0, prob.k1)
    v = prob.v_signature()
    dO = prob.do_signature()
    for qs in case.qs:
        q = prob.q_plain(qs)
        F, R = launch(q, k, v, dO)
        got = gathered(F)
        for name in ("dq", "dk", "dv"):
            note(name, A._ratios(got[name], getattr(R, name), R.bound[name]), qs=qs)
        if case.twice:
            F2, _ = launch(q, k, v, dO)
            same = torch.equal(F.gbuf.view(torch.int16), F2.gbuf.view(torch.int16))
            res["repeat_bit_equal"] = (max(res.get("repeat_bit_equal", (0.0,))[0], 0.0 if same else float("inf")), dict(qs=qs))
    if case.census:
        q = prob.q_plain(1.0)
        for ch in range(prob.chunks("q")):
            F, R = launch(q, k, v, prob.onehot(ch, "q"))
            note("census_dv", census_ratios(gathered(F)["dv"], R, "dv", ch), chunk=ch)
            F, R = launch(prob.onehot(ch, "q"), k, v, dO)
            note("census_dk", census_ratios(gathered(F)["dk"], R, "dk", ch), chunk=ch)
        for ch in range(prob.chunks("k")):
            F, R = launch(q, prob.onehot(ch, "k"), v, dO)
            note("census_dq", census_ratios(gathered(F)["dq"], R, "dq", ch), chunk=ch)
    return res
