"""Fused gradient clip / unscale / non-finite check, the part that needs no GPU: the C ABI additions, train.LossScaler against a real
torch.amp.GradScaler, a plain-torch restatement of what dwm_grad_sumsq_multi returns (the yardstick tests/test_grad_clip_gpu.py
holds the HIP kernels to; it takes nothing from opendwm_amd), and the host contract of CTSDTrainer(grad_conditioning=...)."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = torch.float32


# ------------------------------------------------------------------------------- the restatement (yardstick of the kernels)
def ref(gs, pre_scale=1.0, max_norm=None):
    """(total_norm fp32, coef fp32, found_inf) of a list of tensors: the norm of pre_scale * g summed in fp64 and rounded to fp32,
    then torch.nn.utils.clip_grad_norm_'s coefficient in fp32 from that fp32 norm (a true fp32 division), times pre_scale;
    max_norm None or <= 0: no clip.  found_inf: any element inf / nan (the elements, not the sum)."""
    pre = torch.tensor(pre_scale, dtype=f32)
    total = torch.zeros((), dtype=torch.float64)
    for g in gs:
        total = total + (g.double() * pre.double()).pow(2).sum()
    norm = total.sqrt().to(f32)
    coef = pre
    if max_norm is not None and max_norm > 0:
        coef = pre * torch.clamp(torch.tensor(max_norm, dtype=f32) / (norm + torch.tensor(1e-6, dtype=f32)), max=1.0)
    return norm, coef, any(not bool(torch.isfinite(g).all()) for g in gs)


def norm_bound(E):
    """relative error allowed to the kernel's fp32 norm: the squares are non-negative, so an fp32 accumulator that receives E of
    them (their own rounding included) is off by at most (E + 1) 2^-24 relative, as is the fp64 sum of such accumulators; the square
    root halves that ((E + 1) 2^-25, + 2^-25 for second order); 2^-24 for the fp32 store of the root"""
    return (E + 2) * 2.0 ** -25 + 2.0 ** -24


def _heavy(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.exp(2.0 * torch.randn(n, generator=g)) * torch.randn(n, generator=g)


# ------------------------------------------------------------------------------- C ABI
def test_abi_additions_are_declared():
    from opendwm_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
    assert re.search(r"typedef struct dwm_grad_item\s*\{\s*float\*\s*g;\s*int64_t\s+n;\s*\}\s*dwm_grad_item;", hdr)
    for name in ("dwm_grad_sumsq_multi", "dwm_grad_scale_multi"):
        assert re.search(rf"^int\s+{name}\s*\(const dwm_grad_item\*", hdr, flags=re.M), name
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["dwm_grad_sumsq_multi"][1]) == 11 and len(_lib.SIGNATURES["dwm_grad_scale_multi"][1]) == 7
    assert _lib.ABI_VERSION == 18 and re.search(r"#define DWM_ABI_VERSION 18\b", hdr)          # additions only
    assert "gradnorm.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "gradnorm.hip"))


def test_wrapper_constants():
    from opendwm_amd import train_ops as T
    assert T.GRAD_CHUNK % 1024 == 0 and T.GRAD_SUMSQ_E == T.GRAD_CHUNK // 1024 and 1 <= T.GRAD_SUMSQ_E <= 256
    assert norm_bound(T.GRAD_SUMSQ_E) <= 8e-6


# ------------------------------------------------------------------------------- LossScaler against GradScaler
POISON = [0, 0, 0, 1, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1, 0]       # growth after steps 3, 9, 13, 16; two poisoned steps in a row


def test_loss_scaler_follows_grad_scaler():
    from opendwm_amd.train import LossScaler
    kw = dict(init_scale=1024.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=3)
    theirs, ours = torch.amp.GradScaler("cpu", **kw), LossScaler(**kw)
    assert LossScaler().state_dict() == {"scale": 65536.0, "growth_factor": 2.0, "backoff_factor": 0.5, "growth_interval": 2000,
                                         "_growth_tracker": 0}
    w = torch.nn.Parameter(torch.tensor([0.5]))
    opt = torch.optim.SGD([w], lr=0.01)
    scales, grew, skipped = [], 0, 0
    for poison in POISON:
        x = torch.tensor([float("inf") if poison else 1.5])
        loss = ((w * x - 1.0) ** 2).sum()
        before = w.detach().clone()
        assert torch.equal(ours.scale(loss), theirs.scale(loss))
        theirs.scale(loss).backward()
        theirs.unscale_(opt)
        found_inf = not bool(torch.isfinite(w.grad).all())
        assert found_inf == bool(poison)
        theirs.step(opt)
        skipped += int(torch.equal(w.detach(), before))
        prev = ours.get_scale()
        theirs.update()
        ours.update(found_inf)
        opt.zero_grad()
        assert ours.get_scale() == theirs.get_scale()
        grew += int(ours.get_scale() > prev)
        scales.append(ours.get_scale())
    assert len(POISON) >= 15 and grew >= 1 and skipped == sum(POISON) and scales[2] == 2048.0 and scales[4] == 512.0, scales
    # each loads the other's state
    a, b = LossScaler(), torch.amp.GradScaler("cpu")
    a.load_state_dict(theirs.state_dict())
    b.load_state_dict(ours.state_dict())
    assert a.state_dict() == theirs.state_dict() == ours.state_dict() == b.state_dict()
    assert a.get_scale() == b.get_scale() == ours.get_scale()
    for found in (False, False, True, False):                    # and they go on in step
        a.update(found)
        ours.update(found)
    assert a.state_dict() == ours.state_dict()


def test_loss_scaler_rejects_bad_arguments():
    from opendwm_amd.train import LossScaler
    for kw in (dict(growth_factor=1.0), dict(backoff_factor=1.0), dict(growth_interval=0)):
        with pytest.raises(ValueError):
            LossScaler(**kw)


# ------------------------------------------------------------------------------- the restatement against torch's own clip
def _params_with(gs):
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    return ps


@pytest.mark.parametrize("case", ["clip", "below", "none", "zero"])
def test_restatement_is_torch_clip_grad_norm(case):
    gs = [_heavy(n, n) for n in (1, 3, 257, 4096, 70001)]
    n64 = torch.sqrt(sum(g.double().pow(2).sum() for g in gs)).item()
    pre = 2.0 ** -7
    max_norm = {"clip": 0.5 * pre * n64, "below": 2.0 * pre * n64, "none": None, "zero": 0.0}[case]
    norm, coef, found = ref(gs, pre, max_norm)
    assert not found and abs(norm.item() - pre * n64) <= 2.0 ** -24 * pre * n64
    if case != "clip":
        assert coef.item() == pre                                  # exactly: min(1, .) = 1, or no clip at all
    if max_norm:
        # torch's clip on the unscaled gradients (a power of two: exact), in fp64 so that its own summation error (4e-6 of the
        # norm for its fp32 CPU sum on these heavy-tailed values) stays out: same norm up to the fp32 rounding, same gradients
        ps = _params_with([g.double() * pre for g in gs])
        tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
        assert abs(tn.item() - norm.item()) <= 2.0 ** -24 * norm.item()
        for p, g in zip(ps, gs):
            assert torch.allclose(p.grad, g.double() * coef.double(), rtol=1e-6, atol=0.0)
        if case == "clip":
            assert 0.49 * pre < coef.item() < 0.51 * pre
    for bad in (float("inf"), float("-inf"), float("nan")):
        gb = [g.clone() for g in gs]
        gb[2][100] = bad
        assert ref(gb, pre, max_norm)[2]


def test_empty_list():
    from opendwm_amd import train
    from opendwm_amd import train_ops as T
    norm, coef, found = ref([], 0.25, 1.0)
    assert (norm.item(), coef.item(), found) == (0.0, 0.25, False)
    empty = [torch.nn.Parameter(torch.zeros(3)), torch.nn.Parameter(torch.zeros(0))]          # no gradient at all / an empty one
    empty[1].grad = torch.zeros(0)
    assert T.grad_sumsq_multi([], 0.25, 1.0).tolist() == [0.0, 0.25, 0.0, 0.0]
    assert train.grad_norm_and_coef(empty, 1.0, 0.25) == (0.0, 0.25, False)
    assert train.grad_norm_and_coef(empty) == (0.0, 1.0, False)
    assert train.clip_grad_norm_(empty, 1.0).item() == 0.0
    T.grad_scale_multi_([], 0.5)


def test_host_tensors_are_refused():
    """no CPU fallback: a gradient that is not on a HIP device is an error, not a torch computation"""
    from opendwm_amd import train
    p = torch.nn.Parameter(torch.zeros(8))
    p.grad = torch.ones(8)
    with pytest.raises(RuntimeError):
        train.grad_norm_and_coef([p], 1.0)


# ------------------------------------------------------------------------------- trainer contract
def test_trainer_grad_conditioning_argument():
    from opendwm_amd.pipeline import CTSDTrainer
    from opendwm_amd.train import LossScaler
    with pytest.raises(ValueError):
        CTSDTrainer(torch.nn.Linear(4, 4), grad_conditioning="nope")
    tc = {"enable_grad_scaler": True, "max_norm_for_grad_clip": 1.0}
    tr = CTSDTrainer(torch.nn.Linear(4, 4), training_config=dict(tc))
    assert tr.grad_conditioning == "torch" and isinstance(tr.grad_scaler, torch.amp.GradScaler)
    fu = CTSDTrainer(torch.nn.Linear(4, 4), training_config=dict(tc), grad_conditioning="fused")
    assert fu.grad_conditioning == "fused" and isinstance(fu.grad_scaler, LossScaler) and fu.grad_scaler.get_scale() == 65536.0
    assert fu.skipped_steps == 0 and fu.last_grad_norm == 0.0 and fu.max_grad_norm == 1.0
    assert CTSDTrainer(torch.nn.Linear(4, 4), grad_conditioning="fused").grad_scaler is None


def test_block_tables_cover_every_element_once():
    """the table builder (host code; the kernels index with it): ceil(n / chunk) consecutive-start blocks per tensor, in order, and a
    cache entry per (device, chunk, numels) that the gradient list and the two lists of an optimizer can hold side by side"""
    from opendwm_amd import train_ops as T
    cpu = torch.device("cpu")
    T._BLOCK_TABLES.clear()
    numels = (1, 3, T.GRAD_CHUNK - 1, T.GRAD_CHUNK, T.GRAD_CHUNK + 1, 3 * T.GRAD_CHUNK + 5)
    tab = T._block_tables(cpu, T.GRAD_CHUNK, numels)
    bi, bs, (partials, flags) = tab.block_item, tab.block_start, tab.grad_scratch()
    assert bi.dtype == torch.int32 and bs.dtype == torch.int64 and partials.dtype == torch.float64 and flags.dtype == torch.int32
    assert bi.numel() == bs.numel() == partials.numel() == flags.numel() == sum(-(-n // T.GRAD_CHUNK) for n in numels)
    covered = [0] * len(numels)
    for i, s in zip(bi.tolist(), bs.tolist()):
        assert s == covered[i] and s < numels[i]                  # consecutive starts, never an empty block
        covered[i] = min(s + T.GRAD_CHUNK, numels[i])
    assert tuple(covered) == numels and bi.tolist() == sorted(bi.tolist())
    assert T._block_tables(cpu, T.GRAD_CHUNK, numels).block_item is bi and tab.grad_scratch()[0] is partials
    # the gradient list and the fp32 / 8-bit lists of an optimizer, asked for in rotation as a training loop does: nothing is evicted
    keys = [(T.GRAD_CHUNK, numels), (T.ADAMW_CHUNK, numels[:3]), (T.ADAMW_CHUNK, numels[3:])]
    first = [T._block_tables(cpu, *k) for k in keys]
    assert first[0] is tab
    for _ in range(3):
        T._block_tables(cpu, T.GRAD_CHUNK, (7,))                  # the spare entry: an occasional fourth list evicts none of them
        for k, t0 in zip(keys, first):
            t = T._block_tables(cpu, *k)
            assert t is t0 and t.block_item is t0.block_item and t.block_start is t0.block_start
    T._BLOCK_TABLES.clear()
