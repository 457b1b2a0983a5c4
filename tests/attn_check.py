"""Shared checker of the attention-forward tests (tests/test_attn_check_cpu.py proves that it bites, tests/test_attention_fence_gpu.py
points it at the kernels).  Plain torch, any device; nothing here touches the library - a row map is any object with `rows()`, `L0`,
`n_problems`, `p_per_mask` and `group_size` (ops.RowMap), handed in by the caller.  Fences are tests/gemm_check.py's.

Reference
---------
fp64, from the same bf16 inputs, per (problem, head), gathered through the row map's rows().  With variant bit 15
(ops.ATTN_Q_PRESCALED) Q' carries scale * log2(e), so the scores are exactly s = Q' k in the log2 domain, w = softmax(s ln 2) over the
allowed keys, o = w V; beside them absv = w |V|, A = |Q'| |k|^T and lse_ref = -log2 sum_j 2^s_ij.

Element bound on O (derived, not tuned)
---------------------------------------
    rho_ij = ln2 (72 2^-23 A_ij + 4 2^-23 (|s_ij| + 1))
    e_ij   = expm1(rho_ij + max_j rho_ij)
    bound  = 1.01 (2 2^-8 |o| + 2^-8 absv + (w o e) |V| + (sum_j w e) |o|) + 2 L 2^-23 absv
  * rho: a 64-term fp32 score accumulation is off by at most (K + 8) 2^-23 = 72 2^-23 of the sum of its absolute terms (as in
    gemm_check), the hardware exp2 by an ulp on a few roundings of its argument (s - m: 4 2^-23 (|s| + 1)); ln 2 turns the log2-domain
    error of a score into the relative error of its weight;
  * e: numerator and denominator of a weight are perturbed independently, each entry by at most its own rho, the denominator by at most
    the row's largest;
  * 2 2^-8 |o|: one bf16 rounding of the output (2^-8 relative at most) and one allowance for kernels that sum the ROUNDED P in the
    denominator; 2^-8 absv: one bf16 rounding of every P entry in front of the PV MFMA; the 1.01 because the roundings act on the
    computed values; 2 L 2^-23 absv: fp32 accumulation and rescaling of the PV sum.
With the positive, per-column / head / problem signed V of `Problem.v_signature` the bound is ~1.2 % of |o| and a wrong column, head or
problem is tens of bounds off.  (Zero-mean V cancels o to ~L^-1/2 of absv: the same bound is then 20 % of |o|.)  The CPU emulation of
these rounding points (tests/test_attn_check_cpu.py) reaches 0.37-0.45 of this bound over the cases of the table, 0.62-0.66 of the
census bound below.

Key census
----------
One-hot V: for the keys 64 c .. 64 c + 63, V[j, j - 64 c] = 1 in every head, everything else 0.  Then out[i, d] IS the softmax weight
of key 64 c + d and ceil(L / 64) launches read out the whole P matrix: every weight within 1.01 w_ij (3 2^-8 + e_ij) (rounding of P,
of the output, the rounded-P denominator), masked keys and the channels past the last key EXACTLY 0.  A dropped key is 100 % off on
its entry, a duplicated one 2 x, a counted pad key lowers the whole row.

LSE bound
---------
    |lse - lse_ref| <= max_j rho_ij / ln2 + 2^-22 (|lse_ref| + max_j |s_ij| + 8)
(the row's largest score error shifts the log of the sum by at most itself; the second term is the fp32 log2, the running-maximum
additions and the final subtraction).

Default path (Q scaled inside the kernel)
-----------------------------------------
Spec bound: the same formulas around s = c (q k), c = float32(scale) * float32(log2 e) as the library's fill_params computes it, with
rho_ij enlarged by 1.01 2^-8 scale (|q| |k|^T)_ij for the bf16 rounding of c q - loose (~10 % of |o|), for gross errors of the scale
path.  The sharp statement is `fold`: the kernels form Q'' = bf16_rne(fp32(q) * fp32(c)), one IEEE multiply and one round-to-nearest
conversion, so a default launch must be BIT-EQUAL to the prescaled launch on Q''.

Score-offset ladder
-------------------
k[:, 63] = 1 for every key and q'[i, 63] = t_i, an integer (exact in bf16 up to 256): every score of row i moves by t_i, the softmax
does not, the maximum-free fast path of the resident kernels does (row sums leave [2^-64, 2^64], or fall below 2^-6 with pad keys).
`ladder` lays every integer of [-140, 90] out so that the first `fast_rows` queries of every (problem, head) hold t in [-12, 19] -
inside every acceptance range - and the others walk ascending through the rest, so that 32-query tiles straddle each threshold; at
t = -140 the row sum 2^t sum_j 2^s' underflows to 0.  That serves a kernel whose unit of acceptance is one 32-query tile (the 12-wave
resident kernel).  The streaming kernel accepts or redoes the 2..3 adjacent tiles of a wave together, so a tile-wise ladder leaves
no accepted unit near an edge there: `edge_ladder` places t per row from the row's own sum (t_i + sigma_i = log2 of it) and per unit
of that kernel - whole units within 3 binades inside each edge, units that are redone for a single row less than a binade outside
it, the rest walking through every integer of [-140, 90]."""
import math
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

from tests.gemm_check import NAN, SENTINEL, U23, fenced, fenced_vec, holds_fill, put, untouched  # noqa: F401  (re-exported)

bf16 = torch.bfloat16
f32 = torch.float32
f64 = torch.float64
LN2 = math.log(2.0)
U8 = 2.0 ** -8
LOG2E_F32 = torch.tensor(1.4426950408889634, dtype=f32)
QS = (0.25, 1.0, 3.0)
LADDER_MIN, LADDER_MAX = -140, 90
LADDER_FAST = list(range(-12, 20))                       # 32 values inside every acceptance range
LADDER_REST = [t for t in range(LADDER_MIN, LADDER_MAX + 1) if t not in LADDER_FAST]


def fold_constant(scale: float) -> torch.Tensor:
    """c = float32(scale) * float32(log2 e), an fp32 scalar, as fill_params computes it"""
    return torch.tensor(scale, dtype=f32) * LOG2E_F32


def fold(q: torch.Tensor, scale: float) -> torch.Tensor:
    """Q'' = bf16_rne(fp32(q) * fp32(c)): what the kernels' scale_frag makes of a bf16 q"""
    return (q.float() * fold_constant(scale).to(q.device)).to(bf16)


# ------------------------------------------------------------------------------------------------------------ the case table
@dataclass(frozen=True)
class Case:
    """one row of the GPU file's table.  rowmap: (constructor name without `rowmap_`, arguments); mask: None, "group" (random per batch
    entry, one view attending only itself), "dense" (50 % random, diagonal forced, one row -> key 0 only, one row -> one key of the
    ragged last tile only); hpi: heads per item (variant bits 8-11; 0 = the library's choice); kernel: the family the launch must be
    served by ("stream": asserted through the launch counter)"""
    family: str
    name: str
    rowmap: Tuple[str, tuple]
    heads: int
    L1: int = 0
    mask: Optional[str] = None
    variant: int = 0
    hpi: int = 0
    cross: bool = False
    lse: bool = False
    ladder: int = 0                 # 0: no ladder; else the number of leading fast rows per (problem, head) of `ladder`
    units: Tuple[int, ...] = ()     # the edge ladder (`edge_ladder`): the query rows of each wave unit of the streaming kernel
    edges: Tuple[int, int] = (-64, 64)          # ... and the log2 of the row sums its fast path accepts (-6 with pad keys)
    qs: Tuple[float, ...] = QS
    kernel: str = ""
    twice: bool = False             # two launches must be bit-identical

    @property
    def id(self):
        return f"{self.family}-{self.name}"

    def launch_variant(self):
        return self.variant | (self.hpi << 8)


def _cases():
    c = []
    # packed short: every slot size and its ragged fill; 5 / 13 problems leave the last tile and the last workgroup partly empty
    for L in (1, 8, 9, 16, 17, 32):
        for P in (5, 13):
            c.append(Case("packed_short", f"L{L}_P{P}", ("identity", (P, L)), 2 if P == 5 else 3))
    c.append(Case("packed_short", "pointwise_T9_P5", ("temporal_pointwise", (1, 9, 1, 1, 5)), 3))
    c.append(Case("packed_short", "pointwise_T17_P13", ("temporal_pointwise", (1, 17, 13, 1, 1)), 2))
    # group-masked: shared (LDS) form for V = 4 / 6 / 8, per-wave form (bit 7) for those and V = 3; every (V, w) pair
    ws = (8, 11, 32)
    for i, V in enumerate((4, 6, 8)):
        for j, w in enumerate(ws):
            h = 2 if V == 6 else 1
            c.append(Case("group_shared", f"V{V}_w{w}", ("crossview_rowwise", (2, 1, V, h, w)), 2 + (i + j) % 2, mask="group"))
            c.append(Case("group_per_wave", f"V{V}_w{w}", ("crossview_rowwise", (2, 1, V, h, w)), 3 - (i + j) % 2, mask="group", variant=1 << 7))
    for w in ws:
        c.append(Case("group_per_wave", f"V3_w{w}", ("crossview_rowwise", (2, 1, 3, 1, w)), 2, mask="group", variant=1 << 7))
    # resident 12-wave kernel (bit 13) and its 8-compute-wave geometry at every length, one head and all heads per item
    for i, L in enumerate((64, 65, 96, 97, 224)):
        for j, v in enumerate((1 << 13, 8)):
            heads = 2 + (i + j) % 2
            c.append(Case("resident", f"L{L}_v{v}", ("identity", (2 + j, L)), heads, variant=v, hpi=1 if (i + j) % 2 else heads))
    c.append(Case("resident", "L33+32_v8192", ("identity", (2, 33)), 3, L1=32, variant=1 << 13, hpi=1))
    c.append(Case("resident", "L33+32_v8", ("identity", (3, 33)), 2, L1=32, variant=8, hpi=2))
    c.append(Case("resident", "rowwise_Tw65", ("temporal_rowwise", (1, 5, 1, 3, 13)), 2, variant=1 << 13, hpi=2))
    c.append(Case("resident", "rowwise_Tw65_v8", ("temporal_rowwise", (1, 5, 1, 3, 13)), 2, variant=8, hpi=1))
    c.append(Case("resident", "ladder_L224", ("identity", (2, 224)), 2, variant=1 << 13, hpi=1, ladder=32))
    # streaming (the library's choice at 225 <= L <= 608)
    for i, L in enumerate((225, 256, 257, 575, 608)):
        heads = 2 + i % 2
        c.append(Case("streaming", f"L{L}", ("identity", (2, L)), heads, hpi=1 if i % 2 else heads, kernel="stream"))
    c.append(Case("streaming", "L448+154", ("identity", (2, 448)), 2, L1=154, hpi=1, kernel="stream"))
    c.append(Case("streaming", "rowwise_Tw232", ("temporal_rowwise", (1, 8, 1, 3, 29)), 2, hpi=2, kernel="stream"))
    c.append(Case("streaming", "ladder_L256", ("identity", (2, 256)), 2, hpi=1, units=(64, 64, 64, 64), edges=(-64, 64), kernel="stream"))
    c.append(Case("streaming", "ladder_L257_31pads", ("identity", (2, 257)), 2, hpi=2, units=(96, 64, 64, 33), edges=(-6, 64),
                  kernel="stream"))
    c.append(Case("streaming", "L257_online_forced", ("identity", (2, 257)), 3, variant=1 << 4, hpi=1, kernel="stream"))
    # persistent seams: 260 items on 256 CUs, every problem checked
    c.append(Case("persistent_seams", "I130_N225_stream", ("identity", (130, 225)), 2, hpi=1, kernel="stream", twice=True))
    c.append(Case("persistent_seams", "I130_N225_res12", ("identity", (130, 225)), 2, variant=1 << 13, hpi=1, twice=True))
    # tiled (bit 5), 32 and 64 queries per wave at every length, the three mask modes
    for i, L in enumerate((63, 64, 65, 129, 300)):
        for qt in (1, 2):
            c.append(Case("tiled", f"L{L}_q{qt}", ("identity", (2 + (i + qt) % 2, L)), 3 - (i + qt) % 2, variant=32 | qt))
    c.append(Case("tiled", "L100+10_q1", ("identity", (2, 100)), 3, L1=10, variant=32 | 1))
    c.append(Case("tiled", "L100+10_q2", ("identity", (3, 100)), 2, L1=10, variant=32 | 2))
    c.append(Case("tiled", "group_full_q1", ("crossview_full", (2, 1, 3, 2, 7)), 2, mask="group", variant=32 | 1))
    c.append(Case("tiled", "group_full_q2", ("crossview_full", (2, 1, 4, 3, 9)), 3, mask="group", variant=32 | 2))
    c.append(Case("tiled", "dense_L65_q1", ("identity", (2, 65)), 2, mask="dense", variant=32 | 1))
    c.append(Case("tiled", "dense_L129_q2", ("identity", (2, 129)), 3, mask="dense", variant=32 | 2))
    c.append(Case("tiled", "dense_L100+10_q1", ("identity", (2, 100)), 2, L1=10, mask="dense", variant=32 | 1))
    c.append(Case("tiled", "ladder_L129_q1", ("identity", (2, 129)), 2, variant=32 | 1, ladder=32))
    c.append(Case("tiled", "ladder_L129_q2", ("identity", (2, 129)), 2, variant=32 | 2, ladder=32))
    # tiled with lse (the training forward)
    c.append(Case("tiled_lse", "L65", ("identity", (2, 65)), 2, lse=True))
    c.append(Case("tiled_lse", "L129_q2", ("identity", (2, 129)), 3, lse=True, variant=2))
    c.append(Case("tiled_lse", "L100+10", ("identity", (2, 100)), 3, L1=10, lse=True))
    c.append(Case("tiled_lse", "dense_L65", ("identity", (3, 65)), 2, mask="dense", lse=True))
    c.append(Case("tiled_lse", "group_full", ("crossview_full", (2, 1, 3, 2, 7)), 2, mask="group", lse=True))
    # cross-attention: queries = segment 0, keys / values = segment 1
    for Lq, Lk in ((33, 77), (1, 1), (130, 65)):
        for lse in (False, True):
            c.append(Case("cross", f"Lq{Lq}_Lk{Lk}" + ("_lse" if lse else ""), ("identity", (2 if lse else 3, Lq)), 3 if lse else 2, L1=Lk,
                          cross=True, lse=lse))
    return c


CASES = _cases()


def make_rowmap(ops, case: Case):
    """the case's row map from the library's constructors (the caller passes opendwm_amd.ops)"""
    kind, args = case.rowmap
    return getattr(ops, "rowmap_" + kind)(*args)


def ladder(n_blocks: int, L: int, fast_rows: int) -> torch.Tensor:
    """[n_blocks, L] integer offsets t (see the module docstring); block b = problem * heads + head"""
    assert fast_rows % 32 == 0 and fast_rows < L
    rest = L - fast_rows
    t = torch.empty(n_blocks, L, dtype=torch.int64)
    for b in range(n_blocks):
        t[b, :fast_rows] = torch.tensor([LADDER_FAST[i % 32] for i in range(fast_rows)])
        vals = sorted(LADDER_REST[(b * rest + i) % len(LADDER_REST)] for i in range(rest))
        t[b, fast_rows:] = torch.tensor(vals)
    return t


EDGE_ROLES = ("fast", "inside_lo", "inside_hi", "one_below", "one_above")


def edge_ladder(sigma: torch.Tensor, units, edges) -> torch.Tensor:
    """[n_blocks, L] integer offsets for a kernel that accepts or redoes a whole UNIT of query rows (the streaming kernel: the adjacent
    tiles of one wave, one __all over their row sums).  sigma [n_blocks, L] = log2 sum_j 2^s' of every row WITHOUT its offset, so
    row i's sum is 2^(t_i + sigma_i) and t_i can place it; units = the row counts of the units of one (problem, head), edges = (lo, hi)
    = log2 of the accepted range.  The first five units (block-major) get one role each:
      fast       t in [-12, 19], as in `ladder`
      inside_lo  every row sum in [2^lo, 2^(lo + 3)): the whole unit is normalised by the fast path right at its lower edge
      inside_hi  every row sum in (2^(hi - 3), 2^hi]
      one_below  every row sum in [2^(lo + 4), 2^(lo + 10)) but the middle row's, which lies in [2^(lo - 1), 2^lo): the unit is redone
                 because of that row alone
      one_above  the same at the upper edge
    and the others walk ascending through every integer of [-140, 90]."""
    lo, hi = edges
    B, L = sigma.shape
    assert sum(units) == L
    up = torch.ceil(lo - sigma).long()            # the smallest t with t + sigma >= lo
    dn = torch.floor(hi - sigma).long()           # the largest t with t + sigma <= hi
    t = torch.zeros(B, L, dtype=torch.int64)
    every = list(range(LADDER_MIN, LADDER_MAX + 1))
    n = k = 0
    for b in range(B):
        r0 = 0
        for size in units:
            rows, i = slice(r0, r0 + size), torch.arange(size)
            role = EDGE_ROLES[n] if n < len(EDGE_ROLES) else "walk"
            if role == "fast":
                t[b, rows] = torch.tensor([LADDER_FAST[j % 32] for j in range(size)])
            elif role == "inside_lo":
                t[b, rows] = up[b, rows] + i % 3
            elif role == "inside_hi":
                t[b, rows] = dn[b, rows] - i % 3
            elif role == "one_below":
                t[b, rows] = up[b, rows] + 4 + i % 6
                t[b, r0 + size // 2] = up[b, r0 + size // 2] - 1
            elif role == "one_above":
                t[b, rows] = dn[b, rows] - 4 - i % 6
                t[b, r0 + size // 2] = dn[b, r0 + size // 2] + 1
            else:
                t[b, rows] = torch.tensor(sorted(every[(k + j) % len(every)] for j in range(size)))
                k += size
            n += 1
            r0 += size
    assert n > len(EDGE_ROLES) and k >= len(every)
    return t


# ------------------------------------------------------------------------------------------------------------------ inputs
def _gauss(shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


class Problem:
    """the inputs of one case as ROW tensors - segment 0 [R0, D] addressed through the row map, segment 1 [P * L1, D] dense - and what
    the reference needs to gather them.  cross: queries live in segment 0 only, keys / values in segment 1 only."""

    def __init__(self, case: Case, rowmap, dev, scale: float = 0.125):
        self.case, self.dev, self.scale = case, torch.device(dev), scale
        self.P, self.H, self.L0, self.L1, self.cross = rowmap.n_problems, case.heads, rowmap.L0, case.L1, case.cross
        self.D = self.H * 64
        self.Lq = self.L0 if self.cross else self.L0 + self.L1
        self.Lk = self.L1 if self.cross else self.L0 + self.L1
        rows = rowmap.rows()
        self.R0 = int(rows.max()) + 1
        flat = rows.reshape(-1)
        assert flat.unique().numel() == flat.numel() == self.R0, "the row map must be a bijection onto the rows of segment 0"
        self.rows = rows.to(self.dev)
        # (problem, position in the sequence) of every row of either segment
        p0 = torch.empty(self.R0, dtype=torch.int64)
        l0 = torch.empty(self.R0, dtype=torch.int64)
        p0[flat] = torch.arange(self.P).repeat_interleave(self.L0)
        l0[flat] = torch.arange(self.L0).repeat(self.P)
        self.p0, self.l0 = p0, l0
        r1 = torch.arange(self.P * self.L1)
        self.p1, self.l1 = (r1 // max(self.L1, 1)), (r1 % max(self.L1, 1)) + (0 if self.cross else self.L0)
        seed = 1000 + 7 * CASES.index(case) if case in CASES else 999
        self.gq0, self.gq1 = _gauss((self.R0, self.D), seed), _gauss((self.P * self.L1, self.D), seed + 1)
        k0, k1 = _gauss((self.R0, self.D), seed + 2), _gauss((self.P * self.L1, self.D), seed + 3)
        self.gv0, self.gv1 = _gauss((self.R0, self.D), seed + 4), _gauss((self.P * self.L1, self.D), seed + 5)
        self.has_ladder, self._t, self._memo = bool(case.ladder or case.units), {}, {}
        if self.has_ladder:
            assert self.L1 == 0 and not self.cross
            k0.view(self.R0, self.H, 64)[:, :, 63] = 1.0
        self.k0, self.k1 = k0.to(bf16).to(self.dev), k1.to(bf16).to(self.dev)
        self.group_mask = self.dense_mask = self.allowed = None
        if case.mask == "group":
            self._group_mask(rowmap, seed + 6)
        elif case.mask == "dense":
            self._dense_mask(seed + 6)

    # ---- masks
    def _group_mask(self, rowmap, seed):
        L = self.L0
        gs, ppm = rowmap.group_size, rowmap.p_per_mask
        l = torch.arange(L)
        kind, args = self.case.rowmap
        assert kind.startswith("crossview")
        G = args[2]                                          # group(l) = (l // group_size) % G: the view count of the constructor
        B = (self.P + ppm - 1) // ppm
        gm = torch.rand(B, G, G, generator=torch.Generator().manual_seed(seed)) < 0.5
        gm |= torch.eye(G, dtype=torch.bool)
        gm[0, 1, :] = False
        gm[0, 1, 1] = True                                   # one view attends only itself
        if B > 1:
            gm[1, 0, G - 1] = not bool(gm[0, 0, G - 1])      # the batch entries differ
        g = (l // gs) % G
        p = torch.arange(self.P)
        self.group_mask = gm.to(self.dev)
        self.allowed = gm[(p // ppm)[:, None, None], g[None, :, None], g[None, None, :]].to(self.dev)

    def _dense_mask(self, seed):
        L = self.Lq
        m = torch.rand(self.P, L, L, generator=torch.Generator().manual_seed(seed)) < 0.5
        m |= torch.eye(L, dtype=torch.bool)
        m[:, 5, :] = False
        m[:, 5, 0] = True                                    # a row that allows only key 0
        m[:, L - 2, :] = False
        m[:, L - 2, L - 1] = True                            # a row that allows only the last key (the ragged last tile)
        self.dense_mask = m.to(self.dev)
        self.allowed = self.dense_mask

    def memo(self, key, make):
        """a reference is computed once per problem, shared by the runs that need it and left unchanged"""
        if key not in self._memo:
            self._memo[key] = make()
        return self._memo[key]

    # ---- operands
    def ladder_t(self, qs):
        """[P, H, L0] integer score offsets of a ladder case (the edge ladder depends on the row sums, hence on qs)"""
        if qs not in self._t:
            if self.case.units:
                rows = self.rows.reshape(-1).cpu()
                per_head = lambda x: x[rows].view(self.P, self.L0, self.H, 64).transpose(1, 2).double()
                Q = per_head(fold((self.gq0 * qs).to(bf16), self.scale)).clone()
                Q[..., 63] = 0
                sigma = torch.logsumexp(Q @ per_head(self.k0.cpu()).transpose(-1, -2) * LN2, -1) / LN2
                t = edge_ladder(sigma.view(self.P * self.H, self.L0), self.case.units, self.case.edges)
            else:
                t = ladder(self.P * self.H, self.L0, self.case.ladder)
            self._t[qs] = t.view(self.P, self.H, self.L0)
        return self._t[qs]

    def _ladder_column(self, q0, values):
        """column 63 of every head of q0 <- values [P, H, L0], through the row map"""
        q0.view(self.R0, self.H, 64)[self.rows.reshape(-1).cpu(), :, 63] = values.permute(0, 2, 1).reshape(-1, self.H).to(q0.dtype)

    def q_plain(self, qs):
        """(q0, q1) bf16 for the default path: gauss * qs (ladder: column 63 = bf16(t / c))"""
        q0, q1 = (self.gq0 * qs).to(bf16), (self.gq1 * qs).to(bf16)
        if self.has_ladder:
            self._ladder_column(q0, (self.ladder_t(qs).double() / float(fold_constant(self.scale))).to(bf16))
        return q0.to(self.dev), q1.to(self.dev)

    def q_prescaled(self, qs):
        """(Q0', Q1') = fold(q_plain) (ladder: column 63 = t exactly)"""
        q0, q1 = (fold(x.cpu(), self.scale) for x in self.q_plain(qs))
        if self.has_ladder:
            t = self.ladder_t(qs)
            assert int(t.abs().max()) <= 256                     # integers up to 256 are exact in bf16
            self._ladder_column(q0, t.to(bf16))
        return q0.to(self.dev), q1.to(self.dev)

    def v_signature(self):
        """(0.5 + 1.5 d / 63) (1 + 0.5 h + 0.25 p) (1 + 0.25 gauss): positive, a signature per column, head and problem"""
        d = torch.arange(64).view(1, 1, 64)
        h = torch.arange(self.H).view(1, self.H, 1)
        out = []
        for g, p in ((self.gv0, self.p0), (self.gv1, self.p1)):
            sig = (0.5 + 1.5 * d / 63) * (1 + 0.5 * h + 0.25 * p.view(-1, 1, 1)) * (1 + 0.25 * g.view(-1, self.H, 64))
            out.append(sig.reshape(-1, self.D).to(bf16).to(self.dev))
        return tuple(out)

    def n_chunks(self):
        return (self.Lk + 63) // 64

    def v_onehot(self, c):
        """the census launch c: V[key j, j - 64 c] = 1 for 64 c <= j < 64 c + 64, in every head"""
        out = []
        for l, n, is_key in ((self.l0, self.R0, not self.cross), (self.l1, self.P * self.L1, True)):
            v = torch.zeros(n, self.H, 64)
            if is_key and n:
                sel = (l >= 64 * c) & (l < 64 * c + 64)
                v[sel, :, (l[sel] - 64 * c)] = 1.0
            out.append(v.reshape(n, self.D).to(bf16).to(self.dev))
        return tuple(out)

    # ---- gather / scatter between row tensors and [P, H, L, 64]
    def gather(self, x0, x1, part):
        """part "q" (queries, outputs) or "k" (keys, values)"""
        segs = []
        if not (self.cross and part == "k"):
            segs.append(x0[self.rows.reshape(-1)].view(self.P, self.L0, self.H, 64))
        if self.L1 and not (self.cross and part == "q"):
            segs.append(x1.reshape(self.P, self.L1, self.H, 64))
        return torch.cat(segs, 1).transpose(1, 2)

    def scatter_out(self, o, out0, out1):
        """o [P, H, Lq, 64] -> the row tensors out0 [R0, D] (and out1)"""
        o = o.transpose(1, 2)
        out0[self.rows.reshape(-1)] = o[:, :self.L0].reshape(-1, self.D).to(out0.dtype)
        if self.L1 and not self.cross:
            out1.copy_(o[:, self.L0:].reshape(-1, self.D))

    def lse_len(self):
        return self.P * self.H * (self.L0 + self.L1)

    def lse_queries(self, lse):
        """the query entries [P, H, Lq] of an lse buffer [P, H, L0 + L1] (cross: the key entries are not written)"""
        return lse.view(self.P, self.H, self.L0 + self.L1)[:, :, :self.Lq]


# --------------------------------------------------------------------------------------------------------------- reference
@dataclass
class Scores:
    s: torch.Tensor            # [P, H, Lq, Lk] fp64 log2-domain scores (masked entries: their raw value)
    w: torch.Tensor            # softmax weights, 0 at masked keys
    e: torch.Tensor            # relative allowance per weight
    lse: torch.Tensor          # [P, H, Lq] -log2 sum 2^s
    lse_bound: torch.Tensor
    allowed: Optional[torch.Tensor]
    Lk: int = 0
    we_sum: torch.Tensor = field(default=None)


def scores(prob: Problem, Qg, Kg, c: float = 1.0, extra_scale: float = 0.0) -> Scores:
    """Qg, Kg gathered [P, H, L, 64].  Prescaled: c = 1.  Default path: Qg = the plain q, c = float(fold_constant(scale)),
    extra_scale = scale (the spec bound's allowance for the rounding of c q)."""
    Q, K = Qg.double(), Kg.double()
    qk = Q @ K.transpose(-1, -2)
    A = Q.abs() @ K.abs().transpose(-1, -2)
    s = c * qk
    rho = LN2 * (72 * U23 * (abs(c) * A) + 4 * U23 * (s.abs() + 1)) + 1.01 * U8 * extra_scale * A
    allowed = None if prob.allowed is None else prob.allowed[:, None]
    neg = torch.full_like(s, float("-inf"))
    sm = s if allowed is None else torch.where(allowed, s, neg)
    lse = -torch.logsumexp(sm * LN2, -1) / LN2
    w = torch.exp2(sm + lse[..., None])
    rho_max = (rho if allowed is None else torch.where(allowed, rho, torch.zeros_like(rho))).amax(-1)
    s_max = (s.abs() if allowed is None else torch.where(allowed, s.abs(), torch.zeros_like(s))).amax(-1)
    e = torch.expm1(rho + rho_max[..., None])
    lse_bound = rho_max / LN2 + 2.0 ** -22 * (lse.abs() + s_max + 8)
    return Scores(s, w, e, lse, lse_bound, allowed, K.shape[-2], (w * e).sum(-1))


def o_reference(S: Scores, Vg):
    """(o, bound) [P, H, Lq, 64] fp64 for the element runs"""
    V = Vg.double()
    o = S.w @ V
    absv = S.w @ V.abs()
    bound = 1.01 * (2 * U8 * o.abs() + U8 * absv + (S.w * S.e) @ V.abs() + S.we_sum[..., None] * o.abs()) + 2 * S.Lk * U23 * absv
    return o, bound


def _ratios(got, ref, bound):
    g = got.double()
    d = (g - ref).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))


def element_ratios(got_g, o, bound):
    """|got - o| / bound per element; got_g = the output gathered [P, H, Lq, 64]; a non-finite element gives inf"""
    return _ratios(got_g, o, bound)


def census_ratios(got_g, S: Scores, c: int):
    """the census launch c: channel d of the output against the weight of key 64 c + d; 0 is demanded exactly (masked keys, channels
    past the last key): any other value there gives inf"""
    w = S.w[..., 64 * c:64 * c + 64]
    e = S.e[..., 64 * c:64 * c + 64]
    pad = 64 - w.shape[-1]
    if pad:
        w = torch.nn.functional.pad(w, (0, pad))
        e = torch.nn.functional.pad(e, (0, pad))
    r = _ratios(got_g, w, 1.01 * w * (3 * U8 + e))
    return torch.where((w == 0) & (got_g.double() != 0), torch.full_like(r, float("inf")), r)


def lse_ratios(lse_q, S: Scores):
    """lse_q [P, H, Lq] (Problem.lse_queries) against the LSE bound"""
    return _ratios(lse_q, S.lse, S.lse_bound)


def worst(ratios):
    """(max ratio, its index as a tuple)"""
    if ratios.numel() == 0:
        return 0.0, ()
    flat = ratios.reshape(-1)
    flat = torch.where(torch.isnan(flat), torch.full_like(flat, float("inf")), flat)
    i = int(flat.argmax())
    return float(flat[i]), tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratios.shape))


# ---------------------------------------------------------------------------------------------------------------- the run
class Launch:
    """what a launcher hands back: out0 [R0, D], out1 [P * L1, D] or None, lse [P, H, L0 + L1] fp32 or None"""

    def __init__(self, out0, out1=None, lse=None):
        self.out0, self.out1, self.lse = out0, out1, lse


def run_case(prob: Problem, launch, census=True, default_path=True):
    """every check of one case.  launch(q, k, v, prescaled, want_lse) -> Launch with q / k / v pairs of row tensors (segment 0,
    segment 1); it runs the kernel (or the emulation) and does its own fence checks.  Returns {check name: (worst ratio, where)};
    "default_bit_equal" is 0.0 / inf."""
    case = prob.case
    res = {}

    def note(name, ratios, **kw):
        r, at = worst(ratios)
        if name not in res or r > res[name][0]:
            res[name] = (r, dict(at=at, **kw))

    k = (prob.k0, prob.k1)
    Kg = prob.gather(*k, "k")
    v = prob.v_signature()
    Vg = prob.gather(*v, "k")
    c = float(fold_constant(prob.scale))
    for qs in case.qs:
        qp = prob.q_prescaled(qs)
        S = prob.memo(("S", qs), lambda: scores(prob, prob.gather(*qp, "q"), Kg))
        o, bound = prob.memo(("o", qs), lambda: o_reference(S, Vg))
        pre = launch(qp, k, v, True, case.lse)
        note("element", element_ratios(prob.gather(pre.out0, pre.out1, "q"), o, bound), qs=qs)
        if case.lse:
            note("lse", lse_ratios(prob.lse_queries(pre.lse), S), qs=qs)
        if case.twice:
            again = launch(qp, k, v, True, case.lse)
            rep = torch.equal(pre.out0, again.out0) and (pre.out1 is None or torch.equal(pre.out1, again.out1))
            if case.lse:
                rep = rep and torch.equal(prob.lse_queries(pre.lse), prob.lse_queries(again.lse))
            res["repeat_bit_equal"] = (max(res.get("repeat_bit_equal", (0.0,))[0], 0.0 if rep else float("inf")), dict(qs=qs))
        if not default_path:
            continue
        # the default path: the spec bound, and bit-equality with the prescaled launch on Q'' = fold(q)
        qd = prob.q_plain(qs)
        Sd = prob.memo(("Sd", qs), lambda: scores(prob, prob.gather(*qd, "q"), Kg, c, prob.scale))
        od, bound_d = prob.memo(("od", qs), lambda: o_reference(Sd, Vg))
        dflt = launch(qd, k, v, False, case.lse)
        note("default_spec", element_ratios(prob.gather(dflt.out0, dflt.out1, "q"), od, bound_d), qs=qs)
        if case.lse:
            note("default_spec_lse", lse_ratios(prob.lse_queries(dflt.lse), Sd), qs=qs)
        twin = pre
        if prob.has_ladder:                     # the ladder's prescaled Q holds t exactly, fold(q) does not: its own twin launch
            twin = launch(tuple(fold(x, prob.scale) for x in qd), k, v, True, case.lse)
        same = torch.equal(dflt.out0, twin.out0) and (dflt.out1 is None or torch.equal(dflt.out1, twin.out1))
        if case.lse:
            same = same and torch.equal(prob.lse_queries(dflt.lse), prob.lse_queries(twin.lse))
        res["default_bit_equal"] = (max(res.get("default_bit_equal", (0.0,))[0], 0.0 if same else float("inf")), dict(qs=qs))
    if census:
        qs = 0.25
        qp = prob.q_prescaled(qs)
        S = prob.memo(("S", qs), lambda: scores(prob, prob.gather(*qp, "q"), Kg))
        for ch in range(prob.n_chunks()):
            out = launch(qp, k, prob.v_onehot(ch), True, False)
            note("census", census_ratios(prob.gather(out.out0, out.out1, "q"), S, ch), chunk=ch)
    return res


# ------------------------------------------------------------------------------------------------------- fenced launches
GAP = 3                     # fence rows between the two segments of a buffer


class Fenced:
    """the buffers of one launch:
      * q / k / v as column slices of ONE NaN-fenced [R0 + GAP + P * L1, 3 D + 64] buffer (segment 0 in front, GAP NaN rows, segment
        1), NaN guards around it; cross: the key / value columns of segment 0 and the query columns of segment 1 stay NaN;
      * out (and out1) as views of one buffer at column offset 8 with ldo = D + 16, the whole buffer - the views included - holding
        the sentinel pattern;
      * lse [P, H, L0 + L1] fp32 as a sentinel-filled slice of a longer vector.
    `violations` lists what a launch broke: a touched fence, an unwritten or non-finite result."""

    def __init__(self, prob: Problem, q, k, v, want_lse):
        self.prob = prob
        D, R0, R1 = prob.D, prob.R0, prob.P * prob.L1
        self.iview, self.ibuf = fenced((R0 + GAP + R1, 3 * D), bf16, prob.dev, col_off=16, pad_cols=48)
        seg0, seg1 = self.iview[:R0], self.iview[R0 + GAP:]
        for i, (x0, x1) in enumerate((q, k, v)):
            if not (prob.cross and i > 0):
                seg0[:, i * D:(i + 1) * D] = x0
            if R1 and not (prob.cross and i == 0):
                seg1[:, i * D:(i + 1) * D] = x1
        self.q0, self.k0, self.v0 = (seg0[:, i * D:(i + 1) * D] for i in range(3))
        self.q1, self.k1, self.v1 = (seg1[:, i * D:(i + 1) * D] for i in range(3)) if R1 else (None, None, None)
        self.inputs = self.ibuf.clone()
        self.R1o = 0 if prob.cross else R1
        self.oview, self.obuf = fenced((R0 + (GAP + self.R1o if self.R1o else 0), D), bf16, prob.dev, col_off=8, pad_cols=8, fill="sentinel")
        self.out0 = self.oview[:R0]
        self.out1 = self.oview[R0 + GAP:] if self.R1o else None
        self.lse = self.lbuf = None
        if want_lse:
            self.lse, self.lbuf = fenced_vec(prob.lse_len(), f32, prob.dev, off=8, fill="sentinel")

    def violations(self):
        p, bad = self.prob, []
        if not torch.equal(self.ibuf.view(torch.int16), self.inputs.view(torch.int16)):
            bad.append("the inputs or their fences were written")
        if not untouched(self.obuf, self.oview):
            bad.append("output fence touched")
        if self.R1o and not holds_fill(self.oview[p.R0:p.R0 + GAP]):
            bad.append("rows between the two segments' outputs written")
        for name, t in (("out", self.out0), ("out1", self.out1)):
            if t is not None and not bool(torch.isfinite(t).all()):
                bad.append(f"NaN / Inf / unwritten elements in {name}: rows {torch.nonzero(~torch.isfinite(t).all(1)).flatten()[:8].tolist()}")
        if self.lse is not None:
            if not untouched(self.lbuf, self.lse):
                bad.append("lse fence touched")
            both = self.lse.view(p.P, p.H, p.L0 + p.L1)
            if not bool(torch.isfinite(both[:, :, :p.Lq]).all()):
                bad.append("NaN / Inf / unwritten lse entries")
            if p.cross and not holds_fill(both[:, :, p.Lq:]):
                bad.append("key entries of the lse buffer written")
        return bad

    def result(self) -> Launch:
        return Launch(self.out0, self.out1, self.lse)
