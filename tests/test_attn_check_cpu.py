"""The attention checker (tests/attn_check.py) has to bite - on the CPU, no library involved (the row maps are the plain-Python
constructors of opendwm_amd.ops).

(a) `emulate` repeats the kernels' rounding points - fp32 scores from the bf16 operands, p = exp2(s - m) in fp32, bf16 P in the
    numerator, the denominator from the rounded or from the unrounded P, fp32 PV sum, one bf16 rounding of the output, the default path
    through Q'' = bf16(fp32(q) * c) - and must pass EVERY check of attn_check.run_case on the inputs of every case of the GPU file's
    table (attn_check.CASES, behind the same fences): the condition that the reference alone stays inside the bounds.  The worst ratio
    per family is printed and must be <= 1.
(b) thirteen mutants of the emulation each exceed a bound or trip a fence."""
import json

import pytest
import torch

from opendwm_amd import ops
from tests import attn_check as A

bf16, f32 = torch.bfloat16, torch.float32
FAMILY_WORST = {}


def emulate(prob, q, k, v, prescaled, want_lse, rounded_den, mutate=None):
    """the launch on the CPU: returns the attn_check.Fenced it wrote its results into"""
    F = A.Fenced(prob, q, k, v, want_lse)
    q0, q1 = F.q0, F.q1
    if not prescaled:
        q0, q1 = A.fold(q0, prob.scale), (None if q1 is None else A.fold(q1, prob.scale))
    Qg, Kg, Vg = prob.gather(q0, q1, "q").float(), prob.gather(F.k0, F.k1, "k").float(), prob.gather(F.v0, F.v1, "k").float()
    allowed = torch.ones(prob.P, 1, prob.Lq, prob.Lk, dtype=torch.bool) if prob.allowed is None else prob.allowed[:, None].clone()
    if mutate is not None:
        Qg, Kg, Vg, allowed = mutate(Qg, Kg, Vg, allowed)
    s = Qg @ Kg.transpose(-1, -2)
    s = torch.where(allowed, s, torch.full_like(s, float("-inf")))
    m = s.amax(-1, keepdim=True)
    p = torch.exp2(s - m)
    pb = p.to(bf16).float()
    den = (pb if rounded_den else p).sum(-1, keepdim=True)
    o = ((pb @ Vg) / den).to(bf16)
    prob.scatter_out(o, F.out0, F.out1)
    if want_lse:
        # the LSE bound carries no bf16 term: lse comes from the fp32 sum of the UNROUNDED p (as attn_fwd_kernel's l_run does);
        # the rounded-P denominator is an allowance of the output bound alone
        prob.lse_queries(F.lse).copy_(-(m + torch.log2(p.sum(-1, keepdim=True))).squeeze(-1))
    return F


def _launcher(prob, rounded_den, mutate=None, after=None):
    def launch(q, k, v, prescaled, want_lse):
        F = emulate(prob, q, k, v, prescaled, want_lse, rounded_den, mutate)
        if after is not None:
            after(F)
        bad = F.violations()
        assert not bad, bad
        return F.result()
    return launch


def _problem(case):
    return A.Problem(case, A.make_rowmap(ops, case), "cpu")


def _case(cid):
    return next(c for c in A.CASES if c.id == cid)


# ----------------------------------------------------------------------------------------------------------- (a) emulation
def test_the_table_covers_what_it_promises():
    ids = [c.id for c in A.CASES]
    assert len(set(ids)) == len(ids)
    for case in A.CASES:
        if case.ladder:
            t = _problem(case).ladder_t(1.0)
            assert set(t.reshape(-1).tolist()) == set(range(A.LADDER_MIN, A.LADDER_MAX + 1)), case.id
            assert bool((t[:, :, :case.ladder].abs() <= 20).all()), case.id
            assert int(t.min()) == -140 and int(t.max()) == 90
    assert {c.qs for c in A.CASES} == {A.QS}
    fams = {c.family for c in A.CASES}
    assert fams == {"packed_short", "group_shared", "group_per_wave", "resident", "streaming", "persistent_seams", "tiled", "tiled_lse",
                    "cross"}
    # the products the table names, in full
    ids = set(ids)
    assert all(f"{f}-V{V}_w{w}" in ids for f in ("group_shared", "group_per_wave") for V in (4, 6, 8) for w in (8, 11, 32))
    assert all(f"group_per_wave-V3_w{w}" in ids for w in (8, 11, 32))
    assert all(f"resident-L{L}_v{v}" in ids for L in (64, 65, 96, 97, 224) for v in (8192, 8))
    assert all(f"tiled-L{L}_q{q}" in ids for L in (63, 64, 65, 129, 300) for q in (1, 2))


EDGE_MARGIN = 2e-3       # binades between a placed row sum and the edge: far more than the fp32 row sum of a kernel is off by


@pytest.mark.parametrize("case", [c for c in A.CASES if c.units], ids=lambda c: c.id)
def test_edge_ladder_places_whole_units_at_the_acceptance_edges(case):
    """from lse_ref of the inputs as launched (every qs of the element runs, which include the census' 0.25): per wave unit of the
    streaming kernel, log2 of the row sums against the accepted range [lo, hi].  There is a unit that lies entirely within 3 binades
    inside each edge (normalised by the fast path AT the edge: with pad keys that is where (sum + n_pad) - n_pad has cancelled most),
    a unit that is redone for ONE row less than a binade outside each edge, a unit well inside, and the offsets still cover every
    integer of [-140, 90]."""
    prob = _problem(case)
    lo, hi = case.edges
    m = EDGE_MARGIN
    Kg = prob.gather(prob.k0, prob.k1, "k")
    for qs in case.qs:
        assert set(prob.ladder_t(qs).reshape(-1).tolist()) >= set(range(A.LADDER_MIN, A.LADDER_MAX + 1))
        lsum = -A.scores(prob, prob.gather(*prob.q_prescaled(qs), "q"), Kg).lse.reshape(prob.P * prob.H, prob.L0)
        found = set()
        for b in range(lsum.shape[0]):
            r0 = 0
            for size in case.units:
                u = lsum[b, r0:r0 + size]
                r0 += size
                below, above = u < lo, u > hi
                if bool(((u >= lo + m) & (u <= lo + 3)).all()):
                    found.add("inside_lo")
                if bool(((u <= hi - m) & (u >= hi - 3)).all()):
                    found.add("inside_hi")
                if bool(((u >= lo + 1) & (u <= hi - 1)).all()):
                    found.add("well_inside")
                if int(below.sum()) == 1 and not bool(above.any()) and lo - 1 <= float(u[below]) <= lo - m and bool((u[~below] >= lo + 4).all()):
                    found.add("one_below")
                if int(above.sum()) == 1 and not bool(below.any()) and hi + m <= float(u[above]) <= hi + 1 and bool((u[~above] <= hi - 4).all()):
                    found.add("one_above")
        assert found == {"inside_lo", "inside_hi", "well_inside", "one_below", "one_above"}, (case.id, qs, found)


@pytest.mark.parametrize("case", [c for c in A.CASES if c.units], ids=lambda c: c.id)
def test_maximum_free_arithmetic_stays_inside_the_bound_at_the_edges(case):
    """the fast path's own arithmetic on the rows its acceptance test lets through: p = 2^s with no maximum, bf16 P in the numerator,
    the row sum in fp32 with the pad keys' 1.0 each added FIRST and subtracted at the end (the order that cancels most:
    ((n_pad + p_0) + p_1 ...) - n_pad, sequential), one reciprocal, one bf16 rounding.  Every accepted row - those of the unit placed
    within 3 binades of the lower edge above all - must stay inside the element bound; the worst ratio of that unit is printed."""
    prob = _problem(case)
    lo, hi = case.edges
    n_pad = -prob.L0 % 32
    Kg, v = prob.gather(prob.k0, prob.k1, "k"), prob.v_signature()
    Vg = prob.gather(*v, "k")
    for qs in case.qs:
        Qg = prob.gather(*prob.q_prescaled(qs), "q")
        S = A.scores(prob, Qg, Kg)
        o, bound = A.o_reference(S, Vg)
        p = torch.exp2(Qg.float() @ Kg.float().transpose(-1, -2))
        pads = torch.ones(p.shape[:-1] + (n_pad,))
        den = torch.cat([pads, p], -1).cumsum(-1)[..., -1:] - float(n_pad)
        got = ((p.to(bf16).float() @ Vg.float()) * (1.0 / den)).to(bf16)
        lsum = -S.lse
        accepted = (lsum >= lo) & (lsum <= hi)
        at_edge = accepted & (lsum <= lo + 3)
        assert int(at_edge.sum()) >= min(case.units)
        r = A.element_ratios(got, o, bound)
        print("attn_check_fast_path", json.dumps(dict(case=case.id, qs=qs, n_pad=n_pad, worst_accepted=float(r[accepted].max()),
                                                       worst_within_3_binades_of_the_lower_edge=float(r[at_edge].max()))))
        assert float(r[accepted].max()) <= 1


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.id)
def test_emulation_stays_inside_every_bound(case):
    prob = _problem(case)
    for rounded_den in (False, True):
        res = A.run_case(prob, _launcher(prob, rounded_den))
        for name, (ratio, where) in res.items():
            key = (case.family, name)
            if key not in FAMILY_WORST or ratio > FAMILY_WORST[key][0]:
                FAMILY_WORST[key] = (ratio, case.name, rounded_den)
        assert all(r <= 1 for r, _ in res.values()), (case.id, rounded_den, res)


def test_emulation_worst_ratio_per_family():
    """printed after the cases above (collection order); every family's worst stays <= 1"""
    for (fam, name), (ratio, case, rounded) in sorted(FAMILY_WORST.items()):
        print("attn_check_emulation", json.dumps(dict(family=fam, check=name, worst_ratio=ratio, case=case, rounded_denominator=rounded)))
    assert FAMILY_WORST and all(v[0] <= 1 for v in FAMILY_WORST.values())


# ------------------------------------------------------------------------------------------------------------- (b) mutants
TWO_SEG = "tiled-L100+10_q1"          # 2 problems x 3 heads, 100 + 10 keys: key 109 = the last, key 100 = the first of segment 1
DENSE = "tiled-dense_L65_q1"
LSE = "tiled_lse-L100+10"


def _run_mutant(cid, mutate=None, after=None, census=True):
    prob = _problem(_case(cid))
    res = A.run_case(prob, _launcher(prob, False, mutate, after), census=census, default_path=False)
    print("attn_check_mutant", json.dumps({k: v[0] for k, v in res.items()}))
    return res


def _drop(j):
    def mutate(Q, K, V, allowed):
        allowed[..., j] = False
        return Q, K, V, allowed
    return mutate


def test_mutant_last_key_dropped():
    res = _run_mutant(TWO_SEG, _drop(109))
    assert res["census"][0] > 1 and res["census"][1]["chunk"] == 1 and res["element"][0] > 1, res


def test_mutant_first_key_of_segment_1_dropped():
    res = _run_mutant(TWO_SEG, _drop(100))
    assert res["census"][0] > 1 and res["element"][0] > 1, res


def test_mutant_one_key_counted_twice():
    def mutate(Q, K, V, allowed):
        return Q, torch.cat([K, K[..., 37:38, :]], -2), torch.cat([V, V[..., 37:38, :]], -2), torch.cat([allowed, allowed[..., 37:38]], -1)
    res = _run_mutant(TWO_SEG, mutate)
    assert res["census"][0] > 1 and res["census"][1]["at"][-1] == 37, res


def test_mutant_one_pad_key_with_score_0_counted():
    def mutate(Q, K, V, allowed):
        z = torch.zeros_like(K[..., :1, :])
        return Q, torch.cat([K, z], -2), torch.cat([V, z], -2), torch.cat([allowed, torch.ones_like(allowed[..., :1])], -1)
    res = _run_mutant(TWO_SEG, mutate)
    assert res["census"][0] > 1 and res["element"][0] > 1, res


def test_mutant_one_masked_key_admitted():
    prob = _problem(_case(DENSE))
    i = 7
    j = int(torch.nonzero(~prob.allowed[1, i])[0])

    def mutate(Q, K, V, allowed):
        allowed[1, :, i, j] = True
        return Q, K, V, allowed
    res = _run_mutant(DENSE, mutate)
    assert res["census"][0] == float("inf") and res["census"][1]["at"][0] == 1 and res["census"][1]["at"][2] == i, res
    assert res["element"][0] > 1, res


def test_mutant_two_k_rows_swapped():
    def mutate(Q, K, V, allowed):
        K = K.clone()
        K[..., [40, 41], :] = K[..., [41, 40], :]
        return Q, K, V, allowed
    res = _run_mutant(TWO_SEG, mutate)
    assert res["census"][0] > 1 and res["census"][1]["at"][-1] in (40, 41), res


def test_mutant_two_v_columns_swapped():
    def mutate(Q, K, V, allowed):
        V = V.clone()
        V[..., [20, 21]] = V[..., [21, 20]]
        return Q, K, V, allowed
    res = _run_mutant(TWO_SEG, mutate)
    assert res["element"][0] > 1 and res["element"][1]["at"][-1] in (20, 21), res


def test_mutant_head_reads_the_next_heads_k():
    def mutate(Q, K, V, allowed):
        K = K.clone()
        K[:, 0] = K[:, 1]
        return Q, K, V, allowed
    res = _run_mutant(TWO_SEG, mutate)
    assert res["census"][0] > 1 and res["census"][1]["at"][1] == 0 and res["element"][0] > 1, res


def test_mutant_last_query_row_stored_one_row_early():
    """the row lands on its neighbour (flagged by the element bound) and its own place keeps the sentinel (flagged as unwritten)"""
    def early(F):
        F.out1[-2] = F.out1[-1]
    res = _run_mutant(TWO_SEG, after=early, census=False)
    assert res["element"][0] > 1 and res["element"][1]["at"][0] == 1 and res["element"][1]["at"][2] == 108, res

    def early_unwritten(F):
        F.out1[-2] = F.out1[-1]
        F.out1[-1].view(torch.int16).fill_(A.SENTINEL[bf16])
    with pytest.raises(AssertionError, match="unwritten"):
        _run_mutant(TWO_SEG, after=early_unwritten, census=False)


@pytest.mark.parametrize("where", ["row_past_out1", "row_past_out0", "gap_to_ldo", "column_before"])
def test_mutant_stores_outside_the_output(where):
    def stray(F):
        R0 = F.prob.R0
        r, c = {"row_past_out1": (3 + F.oview.shape[0], 8), "row_past_out0": (3 + R0, 8 + 5), "gap_to_ldo": (3 + R0 - 1, 8 + F.prob.D),
                "column_before": (3 + 4, 7)}[where]
        F.obuf[r, c] = 1.0
    with pytest.raises(AssertionError, match="fence touched|between the two segments"):
        _run_mutant(TWO_SEG, after=stray, census=False)


def test_mutant_lse_off_by_2_to_minus_10_on_one_row():
    def off(F):
        F.prob.lse_queries(F.lse)[1, 2, 57] += 2.0 ** -10
    res = _run_mutant(LSE, after=off, census=False)
    assert res["lse"][0] > 1 and res["lse"][1]["at"] == (1, 2, 57), res
    assert _run_mutant(LSE, census=False)["lse"][0] <= 1


def test_mutant_unwritten_lse_entry_and_lse_fence():
    def unwritten(F):
        F.prob.lse_queries(F.lse)[0, 1, 109:110].view(torch.int32).fill_(A.SENTINEL[f32])
    with pytest.raises(AssertionError, match="unwritten lse"):
        _run_mutant(LSE, after=unwritten, census=False)

    def past(F):
        F.lbuf[8 + F.prob.lse_len()] = 0.0
    with pytest.raises(AssertionError, match="lse fence"):
        _run_mutant(LSE, after=past, census=False)


def test_cross_lse_key_entries_must_keep_the_sentinel():
    def keys_written(F):
        p = F.prob
        F.lse.view(p.P, p.H, p.L0 + p.L1)[0, 0, p.Lq] = 0.0
    with pytest.raises(AssertionError, match="key entries"):
        _run_mutant("cross-Lq33_Lk77_lse", after=keys_written, census=False)


def test_fold_is_one_multiply_and_one_rne_conversion():
    """Q'' of attn_check.fold against the definition evaluated in fp64 (the fp32 product of two values of 8 and 24 significant bits is
    exact in fp64), including the ties"""
    q = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(bf16)
    q = q[torch.isfinite(q)]
    c = A.fold_constant(0.125)
    exact = q.double() * c.double()
    want = exact.float().to(bf16)                   # fp64 -> fp32 -> bf16: the two roundings of the kernel
    assert torch.equal(A.fold(q, 0.125).view(torch.int16), want.view(torch.int16))
