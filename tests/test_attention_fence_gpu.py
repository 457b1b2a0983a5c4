"""GPU leg: the attention forward behind memory fences - every output element, every softmax weight (key census) and every lse entry
against an fp64 bound (tests/attn_check.py; tests/test_attn_check_cpu.py proves that the checker bites).

Every launch of this file runs with (attn_check.Fenced)
  * q / k / v as column slices of one fenced [rows + guards, 3 D + 64] buffer, NaN in the guards, the pad columns and the rows between
    the two segments (cross: in the key / value columns of the query rows and the query columns of the key rows as well),
  * the output, and out1 where there is one, as views of a buffer (column offset 8, ldo = D + 16) that holds the sentinel pattern
    everywhere, the views included,
  * the lse buffer fenced and sentinel-filled,
and asserts after it: inputs and fences bit-identical, no NaN / Inf in the result (every element was written, no fenced value
reached a product), and - per case of attn_check.CASES - every element on the prescaled (variant bit 15) and on the default path,
every weight of the census and every lse entry within its bound.  The default path is held to the loose spec bound AND to bit-equality
with the prescaled launch on Q'' = bf16_rne(fp32(q) * fp32(c)).  The streaming kernel is asserted through dwm_attn_stream_launches.
The fp64 references are computed on the device.  One line per family with the worst ratio of every check and its place goes to the
suite's parity log (`_log` of tests/test_hip_gpu.py; the score-offset ladders as families of their own); the recorded run is
profiles/attention_check_mi355x.log.

Which kernel serves a case: only the streaming family can be asserted (its launch counter); the packed, group, resident and tiled
cases rely on the selection rules of plan_attention (attention.hip) as they stand - a change of those rules could re-route a case to
another kernel, e.g. the tiled one, without this file noticing beyond "not the streaming kernel".

Measured on an MI355X with the table's first 78 cases (the diagonal samples of the group, resident and tiled rows, qs = 1 alone on
the ladders and the persistent seams, the tile-wise ladder on the streaming kernel): 5.1 s for the file (2 s of it the first launch),
the slowest case after the first 0.10 s (persistent seams, 130 problems); the whole gpu suite with the file 937 s (838 passed),
against the 1200 s limit of tests/conftest.py.  The parent's suite time is DERIVED from that, 937 - 5 = ~932 s: it was not measured
on its own.  The table has 92 cases since (the full products, every qs everywhere, the per-unit edge ladder of the streaming kernel);
by the per-case times above that is ~6 s.  Those 14 cases and the edge ladder pass the CPU emulation; their MI355X run is not
recorded here.  Default-path bit-equality held in every family of the recorded run."""
import ctypes as C

import pytest
import torch

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
        _log("attention_fence", family=fam, **{chk: dict(worst_ratio=r, **at) for (f, chk), (r, at) in sorted(d.items()) if f == fam})


def _stream_launches():
    from opendwm_amd import _lib
    return int(_lib.load().dwm_attn_stream_launches())


def _launcher(prob, counts):
    """attn_check.run_case's `launch` on the library: ops.attention / ops.cross_attention on fenced buffers"""
    from opendwm_amd import _lib, ops
    case = prob.case
    rm = A.make_rowmap(ops, case)

    def launch(q, k, v, prescaled, want_lse):
        F = A.Fenced(prob, q, k, v, want_lse)
        variant = case.launch_variant() | (ops.ATTN_Q_PRESCALED if prescaled else 0)
        if case.cross:
            if prescaled:                   # ops.cross_attention takes no variant: the same argument block with bit 15 set.  These
                                            # four lines MIRROR the body of ops.cross_attention and must follow it when it changes
                a = _lib.AttnArgs()
                ops._cross_args(a, F.q0, F.k1, F.v1, F.out0, prob.P, prob.H, prob.scale)
                a.variant = variant
                ops._attn_lse(a, F.lse)
                ops._call("dwm_attention_fwd", C.byref(a))
            else:
                ops.cross_attention(F.q0, F.k1, F.v1, F.out0, prob.P, prob.H, scale=prob.scale, lse=F.lse)
        else:
            kw = dict(q1=F.q1, k1=F.k1, v1=F.v1, out1=F.out1) if prob.L1 else {}
            ops.attention(F.q0, F.k0, F.v0, F.out0, rm, prob.H, scale=prob.scale, group_mask=prob.group_mask, dense_mask=prob.dense_mask,
                          variant=variant, lse=F.lse, **kw)
        counts[0] += 1
        bad = F.violations()
        assert not bad, (case.id, dict(prescaled=prescaled, lse=want_lse), bad)
        return F.result()
    return launch


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.id)
def test_attention_behind_fences(dev, worst, case):
    from opendwm_amd import ops
    prob = A.Problem(case, A.make_rowmap(ops, case), dev)
    counts = [0]
    s0 = _stream_launches()
    res = A.run_case(prob, _launcher(prob, counts))
    served = _stream_launches() - s0
    assert served == (counts[0] if case.kernel == "stream" else 0), (case.id, served, counts[0])
    for name, (ratio, where) in res.items():
        print("attention_fence", case.id, name, ratio, where)
        key = (case.family + ("_ladder" if case.ladder or case.units else ""), name)      # the score-offset ladders get lines of their own
        if key not in worst or ratio > worst[key][0]:
            worst[key] = (ratio, dict(case=case.name, **where))
    assert all(r <= 1 for r, _ in res.values()), (case.id, res)
