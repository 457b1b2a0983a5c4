"""GPU leg: the attention backward behind memory fences - every element of dq / dk / dv (and of the segment-1 gradients) and every
entry of the three census probes against an fp64 bound (tests/attn_bwd_check.py; tests/test_attn_bwd_check_cpu.py proves that the
checker bites).

Every launch of this file runs with (attn_bwd_check.BwdFenced)
  * q / k / v as column slices of one fenced [rows + guards, 3 D + 64] buffer, NaN in the guards, the pad columns and the rows between
    the two segments (cross: in the key / value columns of the query rows and the query columns of the key rows as well),
  * O and dO as views (column offset 8, ldo = D + 16) of NaN-fenced buffers, the lse vector NaN-fenced, with NaN in the key entries
    of a cross launch,
  * dq / dk / dv as column slices of one sentinel-filled [rows + guards, 3 D + 40] buffer at column offset 16, the segment-1 gradients
    in the same allocation above or below segment 0 (both signs of dq1 - dq0),
and asserts after it: inputs and their fences bit-identical, every gradient element the row map reaches written and finite, nothing
else changed (cross: dq only on the query rows, dk / dv only on the key rows), and - per case of attn_bwd_check.CASES - every element
at the three query scales and every entry of the dV, dK and dQ censuses within its bound, demanded zeros exact.  In the isolated
cases O and lse are the checker's fp64 forward of the inputs (no forward launch); the chained cases take them from ops.attention /
ops.cross_attention as the trainers do.  One case is launched twice and must repeat bit for bit (no atomics).  The fp64 references
are computed on the device.  One line per family with the worst ratio of every check and its place goes to the suite's parity log
(`_log` of tests/test_hip_gpu.py); the recorded run is profiles/attention_bwd_check_mi355x.log.

Measured on an MI355X: 5.15 s for the file, 45 tests (1.9 s of it the first launch, the slowest case after
it 0.06 s: 18 launches at L = 257); element ratios 0.58-0.85, census ratios 0.47-0.49, nothing exceeded a bound.
The whole gpu suite with this file: 967 passed in 948 s against the 1200 s limit of tests/conftest.py (the parent's total is DERIVED
from that, 948 - 5 = ~943 s: it was not measured on its own)."""
import pytest
import torch

from tests import attn_bwd_check as B
from tests import attn_check as A
from tests.test_hip_gpu import _log

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def worst():
    """(family, check) -> (worst ratio, where); one log line per family when the module is done"""
    d = {}
    yield d
    for fam in sorted({k[0] for k in d}):
        _log("attention_bwd_fence", family=fam, **{chk: dict(worst_ratio=r, **at) for (f, chk), (r, at) in sorted(d.items()) if f == fam})


class Library:
    """attn_bwd_check.run_case's harness on the library"""

    def __init__(self, prob):
        from opendwm_amd import ops
        self.prob, self.ops, self.rm = prob, ops, A.make_rowmap(ops, prob.case)

    def _seg1(self, F, **names):
        return {k: getattr(F, v) for k, v in names.items()} if self.prob.L1 else {}

    def forward(self, F):
        p = self.prob
        if p.cross:
            self.ops.cross_attention(F.q0, F.k1, F.v1, F.O0, p.P, p.H, scale=p.scale, lse=F.lse)
        else:
            self.ops.attention(F.q0, F.k0, F.v0, F.O0, self.rm, p.H, scale=p.scale, group_mask=p.group_mask, dense_mask=p.dense_mask,
                               lse=F.lse, **self._seg1(F, q1="q1", k1="k1", v1="v1", out1="O1"))

    def backward(self, F):
        p = self.prob
        if p.cross:
            self.ops.cross_attention_bwd(F.q0, F.k1, F.v1, F.O0, F.dO0, F.dq0, F.dk1, F.dv1, p.P, p.H, F.lse, scale=p.scale)
        else:
            self.ops.attention_bwd(F.q0, F.k0, F.v0, F.O0, F.dO0, F.dq0, F.dk0, F.dv0, self.rm, p.H, F.lse, scale=p.scale,
                                   group_mask=p.group_mask, dense_mask=p.dense_mask,
                                   **self._seg1(F, q1="q1", k1="k1", v1="v1", out1="O1", dout1="dO1", dq1="dq1", dk1="dk1", dv1="dv1"))
        bad = F.violations()
        assert not bad, (p.case.id, bad)


def _problem(cid, dev):
    from opendwm_amd import ops
    case = next(c for c in B.CASES if c.id == cid)
    return B.BwdProblem(case, A.make_rowmap(ops, case), dev)


@pytest.mark.parametrize("case", B.CASES, ids=lambda c: c.id)
def test_attention_backward_behind_fences(dev, worst, case):
    prob = _problem(case.id, dev)
    res = B.run_case(prob, Library(prob))
    for name, (ratio, where) in res.items():
        print("attention_bwd_fence", case.id, name, ratio, where)
        key = (case.family, name)
        if key not in worst or ratio > worst[key][0]:
            worst[key] = (ratio, dict(case=case.name, **where))
    assert all(r <= 1 for r, _ in res.values()), (case.id, res)


# ------------------------------------------------------------------------------------------------------------- refusals
def _frozen(prob, below=False):
    q, k, v = prob.q_plain(1.0), (prob.k0, prob.k1), prob.v_signature()
    return B.BwdFenced(prob, q, k, v, prob.do_signature(), below=below).set_forward(*prob.forward_reference(q, k, v))


def _nothing_written(F):
    """after a refused launch: the whole gradient buffer still holds the sentinel, inputs and fences are as they were"""
    assert A.holds_fill(F.gbuf)
    assert [b for b in F.violations() if "unwritten" not in b] == []


def test_refused_cross_attention_with_a_mask(dev):
    """ops.cross_attention_bwd takes no mask: the same argument block with a dense mask set (these lines MIRROR its body and must
    follow it when it changes)"""
    from opendwm_amd import _lib, ops
    prob = _problem("cross-Lq33_Lk77", dev)
    F = _frozen(prob)
    mask = torch.ones(prob.P, prob.L0 + prob.L1, prob.L0 + prob.L1, dtype=torch.uint8, device=dev)
    b = _lib.AttnBwdArgs()
    ops._cross_args(b.fwd, F.q0, F.k1, F.v1, F.O0, prob.P, prob.H, prob.scale)
    b.fwd.mask_mode, b.fwd.mask = 2, mask.data_ptr()
    b.do0 = b.do1 = F.dO0.data_ptr()
    b.dq0 = b.dq1 = F.dq0.data_ptr()
    b.dk0 = b.dk1 = F.dk1.data_ptr()
    b.dv0 = b.dv1 = F.dv1.data_ptr()
    b.ld_d0, b.ld_d1 = F.dq0.stride(0), F.dk1.stride(0)
    with pytest.raises(RuntimeError, match="DWM_EUNSUPPORTED"):
        ops._attn_bwd_launch(b, F.lse)
    torch.cuda.synchronize()
    _nothing_written(F)
    b.fwd.mask_mode, b.fwd.mask = 0, None                   # the very same block without the mask is served
    ops._attn_bwd_launch(b, F.lse)
    torch.cuda.synchronize()
    assert F.violations() == []


def test_refused_gradient_row_stride_not_a_multiple_of_8(dev):
    from opendwm_amd import ops
    prob = _problem("lengths-L33", dev)
    F = _frozen(prob)
    D = prob.D
    g = torch.empty(prob.R0, 3 * D + 4, dtype=bf16, device=dev)
    g.view(torch.int16).fill_(A.SENTINEL[bf16])
    rm = A.make_rowmap(ops, prob.case)
    with pytest.raises(RuntimeError, match="DWM_EALIGN"):
        ops.attention_bwd(F.q0, F.k0, F.v0, F.O0, F.dO0, g[:, :D], g[:, D:2 * D], g[:, 2 * D:3 * D], rm, prob.H, F.lse, scale=prob.scale)
    torch.cuda.synchronize()
    assert A.holds_fill(g)
    _nothing_written(F)


def test_refused_unequal_segment_1_gradient_deltas(dev):
    from opendwm_amd import ops
    prob = _problem("two_segments-L33+32", dev)
    F = _frozen(prob)
    rm = A.make_rowmap(ops, prob.case)
    with pytest.raises(RuntimeError, match="DWM_EUNSUPPORTED"):           # dk1 - dk0 = dq1 - dq0 - D
        ops.attention_bwd(F.q0, F.k0, F.v0, F.O0, F.dO0, F.dq0, F.dk0, F.dv0, rm, prob.H, F.lse, scale=prob.scale,
                          q1=F.q1, k1=F.k1, v1=F.v1, out1=F.O1, dout1=F.dO1, dq1=F.dq1, dk1=F.dq1, dv1=F.dv1)
    torch.cuda.synchronize()
    _nothing_written(F)
