"""Block-wise 8-bit AdamW, the part that needs no GPU: the code tables, a plain-torch restatement of the format and of one
optimizer step (the yardstick tests/test_adam8bit_gpu.py holds the HIP kernels to), and the host contract of
train.AdamW8bit.  The restatement takes nothing from opendwm_amd but the two code tables."""
import math

import pytest
import torch

from opendwm_amd.quant8 import dynamic_code

BLOCK = 256
HYPER = dict(lr=1e-3, b1=0.9, b2=0.975, eps=1e-8, wd=0.01)      # betas of the shipped SD 3.5 training configs
CODE_CAP = 1e-4          # share of elements whose code may differ by ONE adjacent entry between two orders of the same arithmetic


# ------------------------------------------------------------------------------- the restatement (yardstick of the kernels)
def encode(x, code, floor_positive=False):
    """x [n] -> (codes uint8 [n], absmax fp32 [ceil(n / 256)]): code = number of midpoints of adjacent entries strictly below
    x / absmax; floor_positive: a positive x never gets the code of 0.0.  Arithmetic in x's dtype."""
    n, nb = x.numel(), -(-x.numel() // BLOCK)
    xb = torch.zeros(nb * BLOCK, dtype=x.dtype)
    xb[:n] = x
    xb = xb.view(nb, BLOCK)
    absmax = xb.abs().amax(1, keepdim=True)
    y = torch.where(absmax > 0, xb / torch.where(absmax > 0, absmax, torch.ones_like(absmax)), torch.zeros_like(xb))
    code = code.to(x.dtype)
    q = torch.bucketize(y, (code[:-1] + code[1:]) * 0.5)           # right=False: midpoints[q - 1] < y <= midpoints[q]
    if floor_positive:
        zc = int((code == 0).nonzero())
        q = torch.where((xb > 0) & (q == zc), torch.full_like(q, zc + 1), q)
    return q.view(-1)[:n].to(torch.uint8), absmax.view(-1).float()


def decode(q, absmax, code, dtype=torch.float32):
    return code.to(dtype)[q.long()] * absmax.to(dtype).repeat_interleave(BLOCK)[:q.numel()]


def step(p, g, mq, ma, vq, va, t, *, lr, b1, b2, eps, wd, grad_scale=1.0, dtype=torch.float32):
    """one AdamW step from 8-bit state -> (p, mq, ma, vq, va); torch.optim.AdamW's update from the fresh moments, every
    constant rounded to `dtype` first"""
    c = lambda x: torch.tensor(x, dtype=dtype)
    cm, cv = dynamic_code(True), dynamic_code(False)
    g = g.to(dtype) * c(grad_scale)
    m = c(b1) * decode(mq, ma, cm, dtype) + (1 - c(b1)) * g
    v = c(b2) * decode(vq, va, cv, dtype) + (1 - c(b2)) * g * g
    p = p.to(dtype) * (1 - c(lr) * c(wd))
    p = p - c(lr) * (m / c(1 - b1 ** t)) / ((v / c(1 - b2 ** t)).sqrt() + c(eps))
    return (p, *encode(m, cm), *encode(v, cv, floor_positive=True))


def fresh_state(n):
    nb = -(-n // BLOCK)
    zm = int((dynamic_code(True) == 0).nonzero())
    return (torch.full((n,), zm, dtype=torch.uint8), torch.zeros(nb), torch.zeros(n, dtype=torch.uint8), torch.zeros(nb))


def trajectory_inputs(n=65536, steps=50, seed=0):
    """(p0, [g_1 .. g_steps]): gradients with log-normal per-element scales of sigma 2, so that blocks are heavy-tailed"""
    gen = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=gen)
    scale = torch.exp(2.0 * torch.randn(n, generator=gen))
    return p0, [scale * torch.randn(n, generator=gen) for _ in range(steps)]


def trajectory(dtype, p0, grads):
    """the restatement's run -> (final p, [(mq, vq) per step])"""
    p, state, codes = p0.to(dtype), fresh_state(p0.numel()), []
    for t, g in enumerate(grads, 1):
        p, *state = step(p, g, *state, t, dtype=dtype, **HYPER)
        codes.append((state[0], state[2]))
    return p, codes


def code_disagreement(a, b):
    """(share of elements whose codes differ, largest distance in codes)"""
    d = (a.int() - b.int()).abs()
    return (d > 0).float().mean().item(), int(d.max())


def fp32_adamw_trajectory(p0, grads):
    p = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([p], lr=HYPER["lr"], betas=(HYPER["b1"], HYPER["b2"]), eps=HYPER["eps"], weight_decay=HYPER["wd"])
    for g in grads:
        p.grad = g.clone()
        opt.step()
    return p.detach()


# ------------------------------------------------------------------------------- tables
@pytest.mark.parametrize("signed", [True, False])
def test_tables(signed):
    code = dynamic_code(signed)
    assert code.dtype == torch.float32 and code.shape == (256,)
    assert bool((code[1:] > code[:-1]).all())
    assert code[-1] == 1.0 and bool((code == 0).any())
    if signed:
        assert -1.0 <= code[0].item() and abs(code[0].item() + 0.99297) < 1e-5
        assert abs(code[code != 0].abs().min().item() - 5.5e-7) < 1e-12
    else:
        assert code[0] == 0.0
        assert torch.allclose(code[1:3], torch.tensor([3.25e-7, 7.75e-7]), rtol=1e-6, atol=0)
        assert torch.allclose(code[-3:], torch.tensor([0.98945, 0.99648, 1.0]), rtol=0, atol=1e-5)


def test_encode_decode_roundtrip_is_nearest_entry():
    """the restatement itself: every table entry encodes to its own index, a midpoint goes down, decode inverts"""
    for signed in (True, False):
        code = dynamic_code(signed)
        x = code.clone()                                    # absmax = 1 (the table holds 1.0)
        q, a = encode(x, code)
        assert torch.equal(q.long(), torch.arange(256)) and a.item() == 1.0
        assert torch.equal(decode(q, a, code), code)
        mid = (code[:-1] + code[1:]) * 0.5
        q, _ = encode(torch.cat([mid, torch.ones(1)]), code)
        assert torch.equal(q[:255].long(), torch.arange(255))


# ------------------------------------------------------------------------------- the yardstick is sound
def test_restatement_fp32_agrees_with_fp64():
    """50 steps of the heavy-tailed trajectory in fp32; at every step the fp64 restatement takes the same step from the same
    state: what the order / precision of the arithmetic alone can do to the codes.  At most CODE_CAP of the elements may differ
    at any step, never by more than one adjacent code - the cap the GPU comparisons (one step from identical state) reuse.
    Measured while writing: worst share 1.53e-5 (one element of 65 536), distance 1.

    Two free-running trajectories (fp32 and fp64, 50 steps each from their own state) are held to the same share at every step
    (measured: 3.1e-5).  Their distance is reported, not bounded by 1: a one-code disagreement that straddles a decade boundary
    near zero is carried into the next step by the state itself and shows as up to three codes of the finer decade below
    (element 24696 here: codes 134 / 135 after step 1, 131 / 134 after step 2).  That is propagation through the format, not
    arithmetic order, and it dies out within a few steps."""
    p0, grads = trajectory_inputs()
    p, state, worst, dist = p0.clone(), fresh_state(p0.numel()), 0.0, 0
    c32 = []
    for t, g in enumerate(grads, 1):
        out32 = step(p, g, *state, t, dtype=torch.float32, **HYPER)
        out64 = step(p, g, *state, t, dtype=torch.float64, **HYPER)
        for k in (1, 3):
            share, d = code_disagreement(out32[k], out64[k])
            worst, dist = max(worst, share), max(dist, d)
        p, *state = out32
        c32.append((state[0], state[2]))
    print(f"fp32 vs fp64 restatement, step by step: worst share of differing codes {worst:.3e}, largest distance {dist}")
    assert worst <= CODE_CAP and dist <= 1
    p64, c64 = trajectory(torch.float64, p0, grads)
    worst, dist = 0.0, 0
    for (m32, v32), (m64, v64) in zip(c32, c64):
        for a, b in ((m32, m64), (v32, v64)):
            share, d = code_disagreement(a, b)
            worst, dist = max(worst, share), max(dist, d)
    print(f"fp32 vs fp64 restatement, free-running: worst share of differing codes {worst:.3e}, largest distance {dist}")
    assert worst <= CODE_CAP
    assert ((p.double() - p64).norm() / (p64 - p0.double()).norm()).item() < 1e-3


def test_restatement_against_fp32_adamw_is_reported():
    """the figure tests/test_adam8bit_gpu.py::test_trajectory_against_fp32_adamw takes its constant from"""
    p0, grads = trajectory_inputs()
    p8, _ = trajectory(torch.float32, p0, grads)
    p32 = fp32_adamw_trajectory(p0, grads)
    dev = ((p8 - p32).norm() / (p32 - p0).norm()).item()
    print(f"restatement: |p8 - p32| / |p32 - p0| after 50 steps = {dev:.6f}")
    assert 0 < dev < 1          # the 8-bit run moves with the fp32 one; the exact value is the GPU test's constant


# ------------------------------------------------------------------------------- the guard
def test_guard_keeps_positive_second_moments_off_the_zero_code():
    code = dynamic_code(False)
    x = torch.full((256,), 1e-9)
    x[17] = 1.0
    x[200] = 0.0
    q0, _ = encode(x, code)
    q1, _ = encode(x, code, floor_positive=True)
    small = torch.ones(256, dtype=torch.bool)
    small[17] = small[200] = False
    assert bool((q0[small] == 0).all()) and q0[17] == 255
    assert bool((q1[small] == 1).all()) and q1[17] == 255 and q1[200] == 0       # an exact zero stays zero
    assert bool((decode(q1, torch.ones(1), code)[small] > 0).all())


# ------------------------------------------------------------------------------- host contract of AdamW8bit (no kernel call)
def test_adamw8bit_host_contract():
    from opendwm_amd import quant8
    from opendwm_amd.train import AdamW8bit
    big, odd, small = (torch.nn.Parameter(torch.zeros(*s)) for s in ((64, 128), (4097,), (4095,)))
    strided = torch.nn.Parameter(torch.zeros(128, 128).t())               # non-contiguous: fp32 moments
    opt = AdamW8bit([big, odd, small, strided], lr=1.0, betas=(0.9, 0.95))
    assert isinstance(opt, torch.optim.Optimizer) and opt.min_8bit_size == 4096
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 0.5 ** s)
    sched.step()
    assert opt.lr == 0.5 and opt.betas == (0.9, 0.95) and opt.t == 0 and opt.state_dict()["state"] == {}
    for p in (big, odd, small, strided):
        opt._init_state(p)
    for p in (big, odd):
        st, n = opt.state[p], p.numel()
        nb = math.ceil(n / 256)
        assert sorted(st) == ["exp_avg", "exp_avg_absmax", "exp_avg_sq", "exp_avg_sq_absmax", "step"]
        for key, signed in (("exp_avg", True), ("exp_avg_sq", False)):
            q, a = st[key], st[key + "_absmax"]
            assert q.dtype == torch.uint8 and q.shape == p.shape and a.dtype == torch.float32 and a.shape == (nb,)
            assert q.numel() * q.element_size() + a.numel() * a.element_size() == n + 4 * nb
            assert bool((dynamic_code(signed)[q.long()] == 0).all()) and not a.any()          # zero moments
            assert quant8.zero_code(signed) == int(q.flatten()[0])
    for p in (small, strided):
        st = opt.state[p]
        assert sorted(st) == ["exp_avg", "exp_avg_sq", "step"] and st["exp_avg"].dtype == torch.float32
        assert st["exp_avg"].shape == p.shape
    want = sum(2 * (p.numel() + 4 * math.ceil(p.numel() / 256)) for p in (big, odd)) + sum(8 * p.numel() for p in (small, strided))
    assert sum(t.numel() * t.element_size() for st in opt.state.values() for k, t in st.items() if k != "step") == want
    # its own state dict round-trips through torch's loader (which casts state tensors to the parameter's dtype) as bytes
    sd = opt.state_dict()
    opt2 = AdamW8bit([torch.nn.Parameter(torch.zeros_like(p)) for p in (big, odd, small, strided)], lr=3.0)
    opt2.load_state_dict(sd)
    st2 = opt2.state[opt2.param_groups[0]["params"][1]]
    assert st2["exp_avg"].dtype == torch.uint8 and torch.equal(st2["exp_avg"], opt.state[odd]["exp_avg"]) and opt2.lr == 0.5
    assert st2["exp_avg_absmax"].dtype == torch.float32
    with pytest.raises(NotImplementedError):
        bad = AdamW8bit([torch.nn.Parameter(torch.zeros(4))])
        bad.param_groups[0]["amsgrad"] = True
        bad.step()


# ------------------------------------------------------------------------------- what step() hands to the wrappers (no kernel call)
ROUTING_HYPER = dict(lr=0.5, beta1=0.8, beta2=0.95, eps=1e-6, weight_decay=0.125)


def _routing_params():
    """name -> parameter, in the optimizer's order; every gradient a fixed-seed randn"""
    gen = torch.Generator().manual_seed(3)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    ps = {k: torch.nn.Parameter(rnd(*s)) for k, s in (("big", (64, 128)), ("odd", (4097,)), ("small", (4095,)), ("nograd", (16,)),
                                                      ("bf16grad", (8, 16)), ("stridedgrad", (8, 16)), ("resumed", (40,)))}
    for k, p in ps.items():
        if k != "nograd":
            p.grad = rnd(*p.shape)
    ps["bf16grad"].grad.data = ps["bf16grad"].grad.data.to(torch.bfloat16)
    ps["stridedgrad"].grad = rnd(16, 8).t()
    assert ps["bf16grad"].grad.dtype == torch.bfloat16 and not ps["stridedgrad"].grad.is_contiguous()
    return ps


def _record_wrappers(monkeypatch):
    """T.adamw_multi_ / T.adamw8_multi_ / T.adamw_ replaced by recorders -> (multi calls as (kind, args, kwargs), adamw_ calls);
    the adamw_ stand-in refuses what the wrapper refuses (non-contiguous tensors)"""
    from opendwm_amd import train_ops as T
    multi, single = [], []
    monkeypatch.setattr(T, "adamw_multi_", lambda *a, **kw: multi.append((32, a, kw)))
    monkeypatch.setattr(T, "adamw8_multi_", lambda *a, **kw: multi.append((8, a, kw)))

    def adamw_(p, g, m, v, p_bf16, **kw):
        single.append((p, g, m, v))
        if not all(t.is_contiguous() for t in (p, g, m, v)):
            raise RuntimeError("adamw_: fp32 contiguous tensors expected")
    monkeypatch.setattr(T, "adamw_", adamw_)
    return multi, single


@pytest.mark.parametrize("bits", [8, 32])
def test_step_routing(bits, monkeypatch):
    """one step() of AdamW8bit / AdamW over a list that takes every branch of the host loop: which wrapper gets which tensors, in
    which order, with which scalars"""
    from opendwm_amd.train import AdamW, AdamW8bit
    multi, single = _record_wrappers(monkeypatch)
    ps = _routing_params()
    kw = dict(lr=ROUTING_HYPER["lr"], betas=(ROUTING_HYPER["beta1"], ROUTING_HYPER["beta2"]), eps=ROUTING_HYPER["eps"],
              weight_decay=ROUTING_HYPER["weight_decay"])
    opt = AdamW8bit(ps.values(), min_8bit_size=4096, **kw) if bits == 8 else AdamW(ps.values(), **kw)
    resumed = ps["resumed"]
    opt.load_state_dict({"state": {6: {"step": torch.tensor(5.0), "exp_avg": torch.full((40,), 0.5), "exp_avg_sq": torch.ones(40)}},
                         "param_groups": opt.state_dict()["param_groups"]})
    assert list(opt.state) == [resumed]
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in ps.items()}
    assert opt.step(grad_scale=0.25) is None

    eight = ["big", "odd"] if bits == 8 else []
    fresh32 = [k for k in ps if k not in eight + ["nograd", "resumed"]]
    want = ([(8, 1, eight)] if eight else []) + [(32, 1, fresh32), (32, 6, ["resumed"])]
    assert [(kind, c["step"]) for kind, _, c in multi] == [(kind, step) for kind, step, _ in want]        # one call per (kind, step)
    for (kind, args, call), (_, step, names) in zip(multi, want):
        assert call == dict(ROUTING_HYPER, step=step, grad_scale=0.25)
        assert len(args) == (7 if kind == 8 else 5) and all(len(a) == len(names) for a in args)
        states = [opt.state[ps[k]] for k in names]
        keys = ("exp_avg", "exp_avg_absmax", "exp_avg_sq", "exp_avg_sq_absmax") if kind == 8 else ("exp_avg", "exp_avg_sq")
        assert all(a.data_ptr() == ps[k].data_ptr() and a.shape == ps[k].shape for a, k in zip(args[0], names))
        for lst, key in zip(args[2:-1], keys):
            assert all(a is st[key] for a, st in zip(lst, states)), key                                  # moments by identity
        assert all(st["exp_avg"].dtype == (torch.uint8 if kind == 8 else torch.float32) for st in states)
        for g, k in zip(args[1], names):
            assert g.dtype == torch.float32 and g.is_contiguous() and torch.equal(g, grads[k].float())
            assert torch.equal(ps[k].grad, grads[k])                                                      # the gradient itself is left alone
            if k not in ("bf16grad", "stridedgrad"):
                assert g is ps[k].grad                                                                    # no copy where none is needed
        assert all(sh is None for sh in args[-1])                                                         # CPU tensors carry no shadow
    for k, p in ps.items():
        if k == "nograd":
            assert p not in opt.state                               # no state, no step
        else:
            assert float(opt.state[p]["step"]) == (6.0 if k == "resumed" else 1.0)
    assert opt.t == 6 and single == []                              # T.adamw_ is not part of step()

    # a transposed parameter: RuntimeError from step(), raised inside the loop over the group - the parameters before it have
    # counted the step, no launch was made for the group
    multi.clear()
    first = torch.nn.Parameter(torch.zeros(64, 128))
    transposed = torch.nn.Parameter(torch.zeros(128, 128).t())
    last = torch.nn.Parameter(torch.zeros(8))
    for p in (first, transposed, last):
        p.grad = torch.ones_like(p)
    opt = (AdamW8bit if bits == 8 else AdamW)([first, transposed, last])
    with pytest.raises(RuntimeError):
        opt.step()
    assert multi == [] and single == []
    assert float(opt.state[first]["step"]) == 1.0 and last not in opt.state


def test_abi_item_mirror_matches_header():
    """the row train_ops.adamw8_multi_ writes per tensor is dwm_adamw8_item: eight 8-byte fields in the header's order"""
    import ctypes
    import os
    import re
    from opendwm_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dwm_hip.h")).read()
    body = hdr[hdr.index("typedef struct dwm_adamw8_item"):hdr.index("} dwm_adamw8_item;")]
    names = re.findall(r"[\s\*]([a-z_0-9]+);", body)
    assert names == [f for f, _ in _lib.AdamW8Item._fields_] and ctypes.sizeof(_lib.AdamW8Item) == 64
    assert _lib.ABI_VERSION == 18 and {"dwm_quantize_blockwise8", "dwm_dequantize_blockwise8", "dwm_adamw8_multi"} <= set(_lib.SIGNATURES)


def test_trainer_optimizer_bits():
    from opendwm_amd.pipeline import CTSDTrainer
    from opendwm_amd.train import AdamW, AdamW8bit
    from tests.golden.make_reference_checkpoint_fixture import tiny_model
    tr = CTSDTrainer(tiny_model(), lr=3e-4, betas=(0.9, 0.95), optimizer_bits=8)
    assert type(tr.optimizer) is AdamW8bit and tr.optimizer.lr == 3e-4 and tr.optimizer.betas == (0.9, 0.95)
    assert len(tr.optimizer.param_groups[0]["params"]) == 4
    assert type(CTSDTrainer(tiny_model()).optimizer) is AdamW
    assert type(CTSDTrainer(tiny_model(), optimizer_bits=32).optimizer) is AdamW
    with pytest.raises(ValueError):
        CTSDTrainer(tiny_model(), optimizer_bits=16)
