"""The GEMM checker (tests/gemm_check.py) has to bite - on the CPU, no library involved.

(a) the clean result - the fp32 torch product with the epilogue applied in fp32, rounded to bf16, from the suite's input recipe -
    stays inside the element bound with ZERO elements over it, for every epilogue the helper knows;
(b) six mutants of the clean result are flagged: the last K step dropped in the last row, the bias omitted in the last 8 columns,
    one element moved by two bf16 ulps, the gate of the next group on the last row of a group, one store one column past nout and
    one store one row past M (the last two by `untouched`);
(c) for the first two the whole-matrix Frobenius error - what the 6e-3 check of tests/test_hip_gpu.py looks at - is printed beside
    the verdict.  Measured with the seeds used here: the dropped K step scores 6.9e-3 at 513 x 264 x 1536 and 1.1e-2 at
    300 x 520 x 704 - just over the 6e-3 line, and under it with other draws of the same recipe (5.8e-3 has been seen at the first
    shape) - while the element bound flags 258 of 264 and 514 of 520 elements of those rows.

GEGLU needs N % 64 == 0 and the q / k heads N % 192 == 0, which none of the five shapes has: those two epilogues run at the same
M and K with N rounded up to the next such multiple."""
import json

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_check as G
from tests.common import rel_err

bf16 = torch.bfloat16
SHAPES = [(257, 264, 64), (255, 136, 192), (1, 8, 128), (300, 520, 704), (513, 264, 1536)]
ACTS = ["none", "gelu_tanh", "silu", "relu"]
RPG = 100


def _rand(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(bf16)


def _up(n, q):
    return (n + q - 1) // q * q


_CACHE = {}


def _inputs(M, N, K):
    """the suite's recipe (randn, W scaled by K^-0.5, everything rounded to bf16), the fp32 product and the fp64 products; computed
    once per shape and left unchanged"""
    key = (M, N, K)
    if key not in _CACHE:
        a, w, b = _rand((M, K), 1), _rand((N, K), 2, K ** -0.5), _rand((N,), 3)
        groups = (M + RPG - 1) // RPG
        d = dict(a=a, w=w, b=b, gate=_rand((groups, N), 4), res=_rand((M, N), 5), blend=_rand((M, N), 6),
                 alpha=torch.rand(groups, generator=torch.Generator().manual_seed(7)), pos=_rand((RPG, N), 8),
                 y32=a.float() @ w.float().T + b.float(), prod=G.product(a, w))
        _CACHE[key] = d
    return _CACHE[key]


def _act32(y, act):
    return {"none": lambda t: t, "relu": torch.relu, "silu": F.silu, "gelu_tanh": lambda t: F.gelu(t, approximate="tanh")}[act](y)


def _resid_forms(d, M):
    """name -> (fp32 clean result, fp64 reference) of the six operand sets of test_gemm_resid"""
    rows = torch.arange(M) // RPG
    y, p, b = d["y32"], d["prod"], d["b"]
    gate, res, blend, alpha, pos = d["gate"], d["res"], d["blend"], d["alpha"], d["pos"]
    al = alpha[rows][:, None]
    return {
        "gate_res": (res.float() + gate.float()[rows] * y, G.resid(p, b, gate=gate, rows_per_gate=RPG, res=res)),
        "res_blend": (al * blend.float() + (1 - al) * (res.float() + y),
                      G.resid(p, b, res=res, blend=blend, alpha=alpha, rows_per_alpha=RPG)),
        "res": (res.float() + y, G.resid(p, b, res=res)),
        "res_mod_pos": (y + pos.float()[torch.arange(M) % RPG], G.resid(p, b, res=pos, res_mod=RPG)),
        "res_mod_neg": (y + gate.float()[rows], G.resid(p, b, res=gate, res_mod=-RPG)),
        "res_mod_neg_relu": (torch.relu(y) + gate.float()[rows], G.resid(p, b, "relu", res=gate, res_mod=-RPG)),
    }


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_clean_results_stay_inside_the_bound(M, N, K):
    d = _inputs(M, N, K)
    ratios = {}
    for act in ACTS:
        r = G.plain(d["prod"], d["b"], act)
        got = _act32(d["y32"], act).to(bf16)
        ratios["plain_" + act] = (G.check(got, r, K), int((G.element_ratios(got, r.ref, r.mag, K, r.L, r.extra) > 1).sum()))
    for name, (clean, r) in _resid_forms(d, M).items():
        got = clean.to(bf16)
        ratios[name] = (G.check(got, r, K), int((G.element_ratios(got, r.ref, r.mag, K, r.L, r.extra) > 1).sum()))
    # the fp32 residual stream: fp32 operands, fp32 result, the fp32 bound
    res32 = d["res"].float() * 1.001
    r = G.resid(d["prod"], d["b"], res=res32)
    got = res32 + d["y32"]
    ratios["res_out32"] = (G.check(got, r, K), int((G.element_ratios(got, r.ref, r.mag, K) > 1).sum()))
    # GEGLU and the q / k heads at the next N they accept
    Ng = _up(N, 64)
    a, w, b = d["a"], _rand((Ng, K), 2, K ** -0.5), _rand((Ng,), 3)
    y = a.float() @ w.float().T + b.float()
    r = G.geglu(G.product(a, w), b)
    got = (y[:, :Ng // 2] * F.gelu(y[:, Ng // 2:])).to(bf16)
    ratios["geglu"] = (G.check(got, r, K), int((G.element_ratios(got, r.ref, r.mag, K, r.L, r.extra) > 1).sum()))
    Nr = _up(N, 192)
    D = Nr // 3
    w, b = _rand((Nr, K), 2, K ** -0.5), _rand((Nr,), 3)
    rms = _rand((2 * D,), 9) * 0.2 + 1
    y = a.float() @ w.float().T + b.float()
    qk = y[:, :2 * D].view(M, -1, 64)
    qk = qk * torch.rsqrt(qk.pow(2).mean(-1, keepdim=True) + 1e-6) * rms.float().view(-1, 64)
    got = torch.cat([qk.reshape(M, 2 * D), y[:, 2 * D:]], 1).to(bf16)
    r = G.rmshead(G.product(a, w), b, rms, 2 * D, 1e-6)
    block, ratio = G.rmshead_check(got, r, K, 2 * D)
    rv = G.element_ratios(got[:, 2 * D:], r.ref[:, 2 * D:], r.mag[:, 2 * D:], K)
    ratios["rmshead_v"] = (ratio, int((rv > 1).sum()))
    print("gemm_check_clean", json.dumps(dict(M=M, N=N, K=K, rmshead_block=block, **{k: v[0] for k, v in ratios.items()})))
    assert block < 6e-3, block
    assert all(v[0] <= 1 and v[1] == 0 for v in ratios.values()), ratios


def _clean_plain(d, a=None, b=None):
    a = d["a"] if a is None else a
    b = d["b"] if b is None else b
    return (a.float() @ d["w"].float().T + b.float()).to(bf16)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_dropped_last_k_step_in_the_last_row_is_flagged(M, N, K):
    d = _inputs(M, N, K)
    r = G.plain(d["prod"], d["b"])
    a = d["a"].clone()
    a[-1, K - 64:] = 0
    mutant = _clean_plain(d, a=a)
    over = G.element_ratios(mutant, r.ref, r.mag, K) > 1
    frob = rel_err(mutant, r.ref)
    print("gemm_check_mutant", json.dumps(dict(mutant="dropped_k_step", M=M, N=N, K=K, flagged_in_row=int(over[-1].sum()), row=N,
                                               frobenius=frob, frobenius_check_passes=frob < 6e-3)))
    assert int(over[:-1].sum()) == 0                     # the other rows are the clean result
    assert int(over[-1].sum()) >= 0.95 * N, (int(over[-1].sum()), N)


def _resolvable_bias(N):
    """the recipe's bias from the first seed (3, 4, ...) whose last eight entries are all at least 0.1 in magnitude.  Results
    here reach |ref| ~ 4, where half a bf16 ulp is 2^-8 * 4 = 0.016: an omitted bias entry below that is indistinguishable from
    the output rounding for ANY check at bf16 resolution (seed 3 at N = 264 has b[257] = 0.0145: 4 of 2056 and 18 of 4104
    elements escape there, all in that column, all with |ref| > 1.8).  0.1 clears rounding of mutant and bound together."""
    for seed in range(3, 64):
        b = _rand((N,), seed)
        if float(b[-8:].abs().min()) >= 0.1:
            return b
    raise AssertionError("no seed found")


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_omitted_bias_in_the_last_columns_is_flagged(M, N, K):
    d = _inputs(M, N, K)
    bias = _resolvable_bias(N)
    r = G.plain(d["prod"], bias)
    b = bias.clone()
    b[-8:] = 0
    mutant = _clean_plain(d, b=b)
    over = G.element_ratios(mutant, r.ref, r.mag, K) > 1
    frob = rel_err(mutant, r.ref)
    print("gemm_check_mutant", json.dumps(dict(mutant="omitted_bias", M=M, N=N, K=K, flagged=int(over[:, -8:].sum()), of=M * 8,
                                               frobenius=frob, frobenius_check_passes=frob < 6e-3)))
    assert int(over[:, :-8].sum()) == 0
    assert bool(over[:, -8:].all()), (int(over[:, -8:].sum()), M * 8)


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_two_ulps_on_one_element_are_flagged(M, N, K):
    d = _inputs(M, N, K)
    r = G.plain(d["prod"], d["b"])
    for sign in (1, -1):
        mutant = _clean_plain(d)
        bits = mutant.view(torch.int16)
        bits[M // 2, N // 2] += 2 * sign                 # two ulps up / down in magnitude
        over = G.element_ratios(mutant, r.ref, r.mag, K) > 1
        assert int(over.sum()) == 1 and bool(over[M // 2, N // 2]), (sign, int(over.sum()))


# what the recipe's own bias (seed 3) allows: b[257] = 0.0145 of the N = 264 vector is below half a bf16 ulp (2^-8 |ref|) of every
# result with |ref| > 3.7 and within the rounding of many smaller ones - omitting it there cannot be told from output rounding
RECIPE_BIAS_ESCAPES = {(257, 264, 64): 4, (255, 136, 192): 0, (1, 8, 128): 0, (300, 520, 704): 0, (513, 264, 1536): 18}


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_omitted_bias_of_the_recipe_itself(M, N, K):
    """the same mutant with the recipe's seed-3 bias, unfiltered: the checker's real power.  Every escape lies in a column whose
    bias entry is below 0.1, and there are no more of them than measured (4 of 2056 and 18 of 4104, all in the column of
    b[257] = 0.0145, all at |ref| > 1.8)."""
    d = _inputs(M, N, K)
    r = G.plain(d["prod"], d["b"])
    b = d["b"].clone()
    b[-8:] = 0
    mutant = _clean_plain(d, b=b)
    over = G.element_ratios(mutant, r.ref, r.mag, K) > 1
    escaped = ~over[:, -8:]
    print("gemm_check_mutant", json.dumps(dict(mutant="omitted_bias_recipe", M=M, N=N, K=K, escaped=int(escaped.sum()), of=M * 8)))
    assert int(over[:, :-8].sum()) == 0
    assert int(escaped.sum()) <= RECIPE_BIAS_ESCAPES[(M, N, K)], int(escaped.sum())
    assert bool((d["b"][-8:].abs()[escaped.any(0)] < 0.1).all())
    assert bool((r.ref[:, -8:][escaped].abs() > 1.8).all())


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gate_of_the_next_group_is_flagged(M, N, K):
    """the last row of the first group (row 99, or the last row where M <= 100) reads the gate row behind its own; the gate
    table has one row more than the launch needs, as a kernel that looks one group too far would find"""
    d = _inputs(M, N, K)
    gate = torch.cat([d["gate"], _rand((1, N), 14)])
    rows = torch.arange(M) // RPG
    r = G.resid(d["prod"], d["b"], gate=gate, rows_per_gate=RPG, res=d["res"])
    row = min(RPG, M) - 1
    wrong = rows.clone()
    wrong[row] += 1
    mutant = (d["res"].float() + gate.float()[wrong] * d["y32"]).to(bf16)
    over = G.element_ratios(mutant, r.ref, r.mag, K) > 1
    assert G.check(mutant, r, K) > 1
    assert int(over.sum()) == int(over[row].sum()) and int(over[row].sum()) >= 0.9 * N, int(over[row].sum())


@pytest.mark.parametrize("dtype", [bf16, torch.float32])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_stores_outside_the_result_are_caught(M, N, K, dtype):
    d = _inputs(M, N, K)
    q = 8 if dtype == bf16 else 4
    view, buf = G.fenced((M, N), dtype, "cpu", col_off=q, pad_cols=q, fill="sentinel")
    assert view.data_ptr() % 16 == 0 and view.stride(1) == 1 and view.stride(0) == N + 2 * q
    assert G.holds_fill(view) and G.untouched(buf, view)
    G.put(view, d["y32"].to(dtype))
    assert G.untouched(buf, view) and torch.equal(view, d["y32"].to(dtype))
    for r, c in ((3 + M - 1, q + N), (3 + M, q), (3 + M // 2, q - 1), (2, q + N - 1)):     # past nout, past M, before column 0, before row 0
        saved = buf[r, c].clone()
        buf[r, c] = 1.0
        assert not G.untouched(buf, view), (r, c)
        buf[r, c] = float("nan")                         # a canonical NaN is not the fence's pattern either
        assert not G.untouched(buf, view), (r, c)
        buf.view(torch.int16 if dtype == bf16 else torch.int32)[r, c] = saved.view(torch.int16 if dtype == bf16 else torch.int32)
        assert G.untouched(buf, view)


def test_operand_fences_are_nan_and_reach_the_ratio():
    """a NaN operand fence that reaches the result makes the ratio infinite (never a silent pass: NaN compares false)"""
    view, buf = G.fenced((5, 16), bf16, "cpu", col_off=16, pad_cols=48)
    assert buf.isnan().all() and view.stride(0) == 80 and G.untouched(buf, view, fill=G.NAN)
    vec, vbuf = G.fenced_vec(8, torch.float32, "cpu")
    assert vbuf.isnan().all() and vec.is_contiguous() and vec.data_ptr() % 16 == 0
    d = _inputs(1, 8, 128)
    r = G.plain(d["prod"], d["b"])
    got = _clean_plain(d)
    got[0, 3] = float("nan")
    assert G.check(got, r, 128) == float("inf") and not G.check(got, r, 128) <= 1
