"""The attention-backward checker (tests/attn_bwd_check.py) has to bite - on the CPU, no library involved (the row maps are the
plain-Python constructors of opendwm_amd.ops).

(a) `emulate` repeats the rounding points of csrc/attention_bwd.hip in torch - per kernel its own folded operand (fold(q) and raw k for
    dQ, raw q and fold(k) for dK / dV), fp32 scores on top of the given lse, fp32 exp2, fp32 D from the given bf16 O, fp32 dP - D,
    bf16 P and bf16 dS in front of the second products, fp32 sums, fp32 * scale, one bf16 rounding of each stored gradient - and must
    stay inside EVERY element and census bound on every case of the GPU file's table, behind the same fences.  The worst ratio per
    family and check is printed (and recorded in DESIGN.md).
(b) mutants of the emulation, or of what it stored, each exceed a bound, break a demanded zero or trip a fence; the ratios are printed.
(c) the reference formula agrees with fp64 autograd through a plain softmax attention, and the table has the properties claimed for it."""
import dataclasses
import json

import pytest
import torch

from opendwm_amd import ops
from tests import attn_bwd_check as B
from tests import attn_check as A

bf16, f32 = torch.bfloat16, torch.float32
FAMILY_WORST = {}
INF = float("inf")


def emulate(prob, F, mutate=None, mutate_out=None):
    """the backward launch on the CPU, written into the gradient views of the BwdFenced F.  mutate(kernel, ctx) may change what one
    kernel ("dq" / "dkv") works on, mutate_out(outs) the fp32 results [P, H, L, 64] before they are rounded and stored."""
    sc = prob.scale
    g = lambda x0, x1, part: prob.gather(x0, x1, part).float()
    Q, K, V = g(F.q0, F.q1, "q"), g(F.k0, F.k1, "k"), g(F.v0, F.v1, "k")
    O, dO = g(F.O0, F.O1, "q"), g(F.dO0, F.dO1, "q")
    Qf, Kf = A.fold(Q.to(bf16), sc).float(), A.fold(K.to(bf16), sc).float()
    lse = prob.lse_queries(F.lse).float().clone()
    negD = -(dO * O).sum(-1)
    allowed = prob.allowed4().expand(prob.P, prob.H, prob.Lq, prob.Lk)

    def kernel(name, Qs, Ks):
        ctx = dict(Qs=Qs, Ks=Ks, Kprod=K, Qprod=Q, V=V, dO=dO, lse=lse, negD=negD, allowed=allowed.clone())
        if mutate is not None:
            mutate(name, ctx)
        s = ctx["Qs"] @ ctx["Ks"].transpose(-1, -2) + ctx["lse"][..., None]
        P = torch.where(ctx["allowed"], torch.exp2(s), torch.zeros_like(s))
        X = ctx["dO"] @ ctx["V"].transpose(-1, -2) + ctx["negD"][..., None]
        return ctx, P.to(bf16).float(), (P * X).to(bf16).float()

    ctx, _, dS = kernel("dq", Qf, K)
    dq = (dS @ ctx["Kprod"]) * sc
    ctx, Pb, dS = kernel("dkv", Q, Kf)
    dk = (dS.transpose(-1, -2) @ ctx["Qprod"]) * sc
    dv = Pb.transpose(-1, -2) @ ctx["dO"]
    outs = dict(dq=dq[..., :prob.Lq, :], dk=dk[..., :prob.Lk, :], dv=dv[..., :prob.Lk, :])
    if mutate_out is not None:
        mutate_out(outs)
    (dq0, dq1), (dk0, dk1), (dv0, dv1) = F.grads()
    prob.scatter(outs["dq"].to(bf16), dq0, dq1, "q")
    prob.scatter(outs["dk"].to(bf16), dk0, dk1, "k")
    prob.scatter(outs["dv"].to(bf16), dv0, dv1, "k")


def emulate_forward(prob, F):
    """a forward with the kernels' rounding points (attn_check's emulation) for the chained cases: O bf16, lse fp32"""
    g = lambda x0, x1, part: prob.gather(x0, x1, part).float()
    Qf = A.fold(g(F.q0, F.q1, "q").to(bf16), prob.scale).float()
    s = Qf @ g(F.k0, F.k1, "k").transpose(-1, -2)
    s = torch.where(prob.allowed4(), s, torch.full_like(s, -INF))
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    o = (p.to(bf16).float() @ g(F.v0, F.v1, "k")) / p.sum(-1, keepdim=True)
    prob.scatter(o.to(bf16), F.O0, F.O1, "q")
    prob.lse_queries(F.lse).copy_(-(m + torch.log2(p.sum(-1, keepdim=True))).squeeze(-1))


class Harness:
    def __init__(self, prob, mutate=None, mutate_out=None, after=None):
        self.prob, self.mutate, self.mutate_out, self.after = prob, mutate, mutate_out, after

    def forward(self, F):
        emulate_forward(self.prob, F)

    def backward(self, F):
        emulate(self.prob, F, self.mutate, self.mutate_out)
        if self.after is not None:
            self.after(F)
        bad = F.violations()
        assert not bad, bad


def _problem(case):
    return B.BwdProblem(case, A.make_rowmap(ops, case), "cpu")


def _case(cid):
    return next(c for c in B.CASES if c.id == cid)


# ------------------------------------------------------------------------------------------------- (c) reference and coverage
@pytest.mark.parametrize("L,masked", [(7, False), (37, True)])
def test_reference_formula_is_the_gradient_of_softmax_attention(L, masked):
    """attn_bwd_check.ideal_gradients - P = 2^(s + lse), dS = P (dO V^T - rowsum(dO O)), dQ = scale dS K, dK = scale dS^T Q,
    dV = P^T dO - on exact fp64 O and lse against fp64 autograd through a plain softmax attention"""
    gen = torch.Generator().manual_seed(L)
    Q, K, V, dO = (torch.randn(2, 3, L, 64, generator=gen, dtype=torch.float64) for _ in range(4))
    allowed = torch.ones(2, 1, L, L, dtype=torch.bool)
    if masked:
        allowed = (torch.rand(2, 1, L, L, generator=gen) < 0.5) | torch.eye(L, dtype=torch.bool)
    scale = 0.125
    Q.requires_grad_(True), K.requires_grad_(True), V.requires_grad_(True)
    s = scale * (Q @ K.transpose(-1, -2))
    s = torch.where(allowed, s, torch.full_like(s, -INF))
    O = torch.softmax(s, -1) @ V
    (O * dO).sum().backward()
    lse = -torch.logsumexp(s.detach(), -1) / A.LN2
    got = B.ideal_gradients(Q.detach(), K.detach(), V.detach(), O.detach(), dO, lse, allowed, scale)
    for name, a, b in zip(("dq", "dk", "dv"), got, (Q.grad, K.grad, V.grad)):
        rel = float((a - b).norm() / b.norm())
        worst = float(((a - b).abs() / b.abs().clamp_min(1e-3 * float(b.abs().max()))).max())
        print("attn_bwd_check_autograd", json.dumps(dict(L=L, masked=masked, grad=name, rel=rel, worst_element=worst)))
        assert rel < 1e-12 and worst < 1e-11, (name, rel, worst)


def test_the_table_covers_what_it_promises():
    ids = [c.id for c in B.CASES]
    assert len(set(ids)) == len(ids)
    assert {c.family for c in B.CASES} == {"lengths", "two_segments", "cross", "rowmaps", "group_mask", "dense_mask", "score_offsets", "chained"}
    assert {c.qs for c in B.CASES} == {A.QS}
    ids = set(ids)
    assert all(f"lengths-L{L}" in ids for L in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 193, 257))
    assert all(f"two_segments-L{a}+{b}" in ids for a, b in ((33, 32), (64, 1), (100, 10), (127, 2), (130, 65)))
    assert all(f"cross-Lq{a}_Lk{b}" in ids for a, b in ((1, 1), (33, 77), (130, 65), (65, 130)))
    assert all(f"group_mask-V{V}_w{w}" in ids for V in (3, 4, 6, 8) for w in (8, 11))
    # workgroup counts of the two kernels: below 8, a multiple of 8, several nonzero remainders of the xcd_remap remainder path
    counts = set()
    for c in B.CASES:
        rm = A.make_rowmap(ops, c)
        dq, dkv = B.workgroups(c, rm.n_problems, rm.L0)
        counts |= {dq, dkv}
        if c.cross and c.name in ("Lq130_Lk65", "Lq65_Lk130"):
            assert dq != dkv                                   # the block counts differ between the two kernels
    assert any(n < 8 for n in counts) and any(n >= 8 and n % 8 == 0 for n in counts)
    assert len({n % 8 for n in counts if n > 8 and n % 8}) >= 5, sorted(counts)
    two = [c for c in B.CASES if c.L1 and not c.cross]
    L0 = lambda c: A.make_rowmap(ops, c).L0
    assert any(L0(c) % 64 not in (0,) and L0(c) < 128 for c in two)          # a seam inside a tile
    assert any(L0(c) % 64 == 0 for c in two)                                  # ... at a tile edge
    assert any(L0(c) > 128 for c in two)                                      # ... in the second block
    cross = [c for c in B.CASES if c.cross]
    assert any(L0(c) % 64 for c in cross) and any(c.L1 % 64 for c in cross)   # a ragged last tile of queries, and of keys
    assert {c.below for c in two if not c.chained} == {False, True}           # both signs of dq1 - dq0
    assert any(c.twice and max(B.workgroups(c, 1, L0(c))) > c.heads for c in B.CASES)      # determinism on a multi-block case
    dense = _problem(_case("dense_mask-L65"))
    assert not bool(dense.allowed[:, :, B.NEVER_ATTENDED_KEY].any()) and bool(dense.allowed.any(-1).all())
    assert int(dense.allowed[0, 5].sum()) == 1 and bool(dense.allowed[0, 5, 0]) and bool(dense.allowed[0, 63, 64])
    lad = _problem(_case("score_offsets-L129"))
    assert set(lad.ladder_t(1.0).reshape(-1).tolist()) == set(B.LADDER_T)


def test_gradient_buffer_layout_has_both_delta_signs():
    for cid, sign in (("two_segments-L33+32", 1), ("two_segments-L64+1", -1)):
        prob = _problem(_case(cid))
        q = prob.q_plain(1.0)
        F = B.BwdFenced(prob, q, (prob.k0, prob.k1), prob.v_signature(), prob.do_signature(), below=prob.case.below)
        deltas = {a.data_ptr() - b.data_ptr() for a, b in ((F.dq1, F.dq0), (F.dk1, F.dk0), (F.dv1, F.dv0))}
        assert len(deltas) == 1 and deltas.pop() * sign > 0
        assert F.dq0.data_ptr() != F.gbuf.data_ptr() and F.dq0.stride(0) == 3 * prob.D + 40


# ----------------------------------------------------------------------------------------------------------- (a) emulation
@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.id)
def test_emulation_stays_inside_every_bound(case):
    prob = _problem(case)
    res = B.run_case(prob, Harness(prob))
    for name, (ratio, where) in res.items():
        key = (case.family, name)
        if key not in FAMILY_WORST or ratio > FAMILY_WORST[key][0]:
            FAMILY_WORST[key] = (ratio, case.name)
    assert all(r <= 1 for r, _ in res.values()), (case.id, res)


def test_emulation_worst_ratio_per_family():
    """printed after the cases above (collection order); every family's worst stays <= 1"""
    for (fam, name), (ratio, case) in sorted(FAMILY_WORST.items()):
        print("attn_bwd_check_emulation", json.dumps(dict(family=fam, check=name, worst_ratio=ratio, case=case)))
    assert FAMILY_WORST and all(v[0] <= 1 for v in FAMILY_WORST.values())


def test_bounds_against_the_gradients():
    """how large the element bounds are against gradient entries of typical size (the row's root mean square), printed: the figure
    the module docstring of attn_bwd_check quotes"""
    prob = _problem(_case("two_segments-L100+10"))
    for qs in A.QS:
        q, k, v, dO = prob.q_plain(qs), (prob.k0, prob.k1), prob.v_signature(), prob.do_signature()
        O, lse = prob.forward_reference(q, k, v)
        R = B.reference(prob, prob.gather(*q, "q"), prob.gather(*k, "k"), prob.gather(*v, "k"), prob.gather(*O, "q"), prob.gather(*dO, "q"),
                        prob.lse_queries(lse))
        fig = {n: float((R.bound[n] / getattr(R, n).pow(2).mean(-1, keepdim=True).sqrt()).median()) for n in ("dq", "dk", "dv")}
        print("attn_bwd_check_bound_size", json.dumps(dict(qs=qs, median_bound_over_row_rms=fig)))
        assert all(0 < f < 0.1 for f in fig.values()), fig


# ------------------------------------------------------------------------------------------------------------- (b) mutants
TWO_SEG = "two_segments-L100+10"      # 2 problems x 3 heads, 100 + 10 tokens: key 109 = the last, key 100 = the first of segment 1
BLOCKS = "lengths-L193"               # two key blocks, four query tiles
GROUP = "group_mask-V4_w11"
DENSE = "dense_mask-L65"


def _run_mutant(cid, mutate=None, mutate_out=None, after=None, qs=None, census=True):
    case = _case(cid)
    case = dataclasses.replace(case, census=census and case.census, **({} if qs is None else dict(qs=qs)))
    prob = _problem(case)
    res = B.run_case(prob, Harness(prob, mutate, mutate_out, after))
    print("attn_bwd_check_mutant", json.dumps({k: v[0] for k, v in res.items()}))
    return res


def _flagged(res):
    return {k for k, v in res.items() if v[0] > 1}


def test_unmutated_runs_of_the_mutant_cases_pass():
    for cid in (TWO_SEG, DENSE):
        assert not _flagged(_run_mutant(cid))


def test_mutant_last_key_dropped_from_one_querys_dS():
    def mutate(kernel, ctx):
        if kernel == "dq":
            ctx["allowed"][1, :, 57, 109] = False
    res = _run_mutant(TWO_SEG, mutate)
    assert res["census_dq"][0] > 1 and res["census_dq"][1]["at"][0] == 1 and res["census_dq"][1]["at"][2] == 57, res
    assert res["census_dq"][1]["chunk"] == 1 and res["dq"][0] > 1 and _flagged(res) <= {"census_dq", "dq"}, res


def test_mutant_first_key_of_segment_1_dropped():
    def mutate(kernel, ctx):
        ctx["allowed"][..., 100] = False
    res = _run_mutant(TWO_SEG, mutate)
    assert _flagged(res) == {"dq", "dk", "dv", "census_dq", "census_dk", "census_dv"}, res


def test_mutant_one_query_tile_skipped_in_one_key_block():
    def mutate(kernel, ctx):
        if kernel == "dkv":
            ctx["allowed"][0, 1, 64:128, 128:] = False
    res = _run_mutant(BLOCKS, mutate, census=False)
    assert res["dk"][0] > 1 and res["dv"][0] > 1 and res["dq"][0] <= 1, res
    assert res["dv"][1]["at"][:2] == (0, 1) and res["dv"][1]["at"][2] >= 128, res


def test_mutant_one_pad_query_admitted_with_score_0():
    """the clamp row of a ragged query tile (the last query's lse, D and dO, as the DMA duplicates them) with score 0"""
    def mutate(kernel, ctx):
        if kernel == "dkv":
            ctx["Qs"] = torch.cat([ctx["Qs"], torch.zeros_like(ctx["Qs"][..., :1, :])], -2)
            for name in ("Qprod", "dO"):
                ctx[name] = torch.cat([ctx[name], ctx[name][..., -1:, :]], -2)
            for name in ("lse", "negD"):
                ctx[name] = torch.cat([ctx[name], ctx[name][..., -1:]], -1)
            ctx["allowed"] = torch.cat([ctx["allowed"], torch.ones_like(ctx["allowed"][..., :1, :])], -2)
    res = _run_mutant(TWO_SEG, mutate)
    assert res["census_dv"][0] > 1 and res["census_dk"][0] > 1 and res["dv"][0] > 1, res


def test_mutant_one_pad_key_admitted():
    """the clamp row of the ragged last key tile: the last key once more"""
    def mutate(kernel, ctx):
        if kernel == "dq":
            for name in ("Ks", "Kprod", "V"):
                ctx[name] = torch.cat([ctx[name], ctx[name][..., -1:, :]], -2)
            ctx["allowed"] = torch.cat([ctx["allowed"], ctx["allowed"][..., -1:]], -1)
    res = _run_mutant(TWO_SEG, mutate)
    assert res["census_dq"][0] > 1 and res["dq"][0] > 1 and _flagged(res) == {"census_dq", "dq"}, res


@pytest.mark.parametrize("cid", [GROUP, DENSE])
def test_mutant_one_masked_pair_admitted(cid):
    prob = _problem(_case(cid))
    i = 7
    j = int(torch.nonzero(~prob.allowed[1, i])[0])

    def mutate(kernel, ctx):
        ctx["allowed"][1, :, i, j] = True
    res = _run_mutant(cid, mutate)
    assert res["census_dq"][0] == INF and res["census_dk"][0] == INF and res["census_dv"][0] == INF, res
    assert res["census_dq"][1]["at"][0] == 1 and res["census_dq"][1]["at"][2] == i, res


def test_mutant_never_attended_key_given_weight():
    def mutate(kernel, ctx):
        if kernel == "dkv":
            ctx["allowed"][0, :, 20, B.NEVER_ATTENDED_KEY] = True
    res = _run_mutant(DENSE, mutate)
    assert res["dk"][0] > 1e6 and res["dv"][0] > 1e6 and res["dv"][1]["at"][2] == B.NEVER_ATTENDED_KEY, res
    assert res["census_dv"][0] == INF and res["census_dk"][0] == INF, res


def test_mutant_D_from_the_wrong_head():
    def mutate(kernel, ctx):
        ctx["negD"] = ctx["negD"].roll(1, 1)
    res = _run_mutant(TWO_SEG, mutate, census=False)
    assert res["dq"][0] > 1 and res["dk"][0] > 1 and res["dv"][0] <= 1, res


def test_mutant_D_omitted():
    def mutate(kernel, ctx):
        ctx["negD"] = torch.zeros_like(ctx["negD"])
    res = _run_mutant(TWO_SEG, mutate)
    assert {"dq", "dk", "census_dq", "census_dk"} <= _flagged(res) and res["dv"][0] <= 1, res


def test_mutant_lse_of_the_neighbouring_row():
    def mutate(kernel, ctx):
        ctx["lse"] = ctx["lse"].roll(1, -1)
    res = _run_mutant(TWO_SEG, mutate)
    assert _flagged(res) == {"dq", "dk", "dv", "census_dq", "census_dk", "census_dv"}, res


def test_mutant_folded_operand_swapped_between_the_kernels():
    """dq on (q, fold(k)), dk / dv on (fold(q), k): the sharp reference - each output with its own kernel's folded operand - tells the
    two P matrices apart at qs = 3 in all three element checks (measured: 3.3 / 2.8 / 2.1 bounds), so no common reference with a fold
    term in rho is needed.  At qs = 0.25 and 1 the two P matrices lie within the bounds of each other (printed, not asserted): the
    scores are then too small for the operand's bf16 rounding to matter."""
    def mutate(kernel, ctx):
        if kernel == "dq":
            ctx["Qs"], ctx["Ks"] = ctx["Qprod"], A.fold(ctx["Kprod"].to(bf16), 0.125).float()
        else:
            ctx["Qs"], ctx["Ks"] = A.fold(ctx["Qprod"].to(bf16), 0.125).float(), ctx["Kprod"]
    for qs in (0.25, 1.0):
        _run_mutant(TWO_SEG, mutate, qs=(qs,), census=False)
    res = _run_mutant(TWO_SEG, mutate, qs=(3.0,))
    assert {"dq", "dk", "dv"} <= _flagged(res), res


def test_mutant_scale_dropped_from_dK():
    def out(o):
        o["dk"] = o["dk"] / 0.125
    res = _run_mutant(TWO_SEG, mutate_out=out)
    assert _flagged(res) == {"dk", "census_dk"}, res


def test_mutant_dK_and_dV_swapped():
    def out(o):
        o["dk"], o["dv"] = o["dv"], o["dk"]
    res = _run_mutant(TWO_SEG, mutate_out=out, census=False)
    assert _flagged(res) == {"dk", "dv"}, res


def test_mutant_two_k_rows_swapped_in_the_dQ_product_only():
    def mutate(kernel, ctx):
        if kernel == "dq":
            K = ctx["Kprod"].clone()
            K[..., [40, 41], :] = K[..., [41, 40], :]
            ctx["Kprod"] = K
    res = _run_mutant(TWO_SEG, mutate)
    assert _flagged(res) == {"dq", "census_dq"} and res["census_dq"][1]["at"][-1] in (40, 41), res


def test_mutant_head_reads_the_next_heads_dO():
    def mutate(kernel, ctx):
        dO = ctx["dO"].clone()
        dO[:, 0] = dO[:, 1]
        ctx["dO"] = dO
    res = _run_mutant(TWO_SEG, mutate, census=False)
    assert _flagged(res) == {"dq", "dk", "dv"} and res["dv"][1]["at"][1] == 0, res


def test_mutant_last_gradient_row_stored_one_row_early():
    """the row lands on its neighbour (flagged by the element bound) and its own place keeps the sentinel (flagged as unwritten)"""
    def early(F):
        F.dk1[-2] = F.dk1[-1]
    res = _run_mutant(TWO_SEG, after=early, census=False)
    assert _flagged(res) == {"dk"} and res["dk"][1]["at"][0] == 1 and res["dk"][1]["at"][2] == 108, res

    def early_unwritten(F):
        F.dk1[-2] = F.dk1[-1]
        F.dk1[-1].view(torch.int16).fill_(A.SENTINEL[bf16])
    with pytest.raises(AssertionError, match="unwritten elements in dk1"):
        _run_mutant(TWO_SEG, after=early_unwritten, census=False)


def test_mutant_store_into_the_segment_1_rows_of_the_wrong_problem():
    def stray(F):
        F.dq1[F.prob.L1] = F.dq1[0]             # problem 0's first context row lands on problem 1's
    res = _run_mutant(TWO_SEG, after=stray, census=False)
    assert _flagged(res) == {"dq"} and res["dq"][1]["at"][0] == 1 and res["dq"][1]["at"][2] == 100, res


@pytest.mark.parametrize("where", ["pad_columns", "column_before", "guard_row_below", "guard_row_above", "gap_rows"])
def test_mutant_stores_outside_the_gradients(where):
    def stray(F):
        D, rows = F.prob.D, F.gview.shape[0]
        r, c = {"pad_columns": (3 + 4, 16 + 3 * D), "column_before": (3 + 4, 15), "guard_row_below": (3 + rows, 16 + 5), "guard_row_above": (2, 16),
                "gap_rows": (3 + F.prob.R0 + 1, 16 + D + 3)}[where]
        F.gbuf[r, c] = 1.0
    with pytest.raises(AssertionError, match="fence touched|between the two segments"):
        _run_mutant(TWO_SEG, after=stray, census=False)


def test_mutant_cross_gradients_outside_their_side():
    def stray(F):
        F.g0[0, F.prob.D] = 0.0                 # a dk element on a query row
    with pytest.raises(AssertionError, match="dk / dv columns of the query rows"):
        _run_mutant("cross-Lq33_Lk77", after=stray, census=False)

    def stray2(F):
        F.g1[0, 0] = 0.0                        # a dq element on a key row
    with pytest.raises(AssertionError, match="dq columns of the key rows"):
        _run_mutant("cross-Lq33_Lk77", after=stray2, census=False)


def test_mutant_inputs_written():
    def o_written(F):
        F.O0[3, 5] = 0.0
    with pytest.raises(AssertionError, match="input O"):
        _run_mutant(TWO_SEG, after=o_written, census=False)

    def lse_fence(F):
        F.lbuf[3] = 0.0
    with pytest.raises(AssertionError, match="input lse"):
        _run_mutant(TWO_SEG, after=lse_fence, census=False)
