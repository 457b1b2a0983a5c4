"""GPU leg (`-m gpu`) of the sync-free AdamW entry points dwm_adamw_multi_dev / dwm_adamw8_multi_dev (include/dwm_hip.h):
lr, the bias corrections, the gradient coefficient and the non-finite flag come from device memory instead of the argument list.

Given equal scalar values every output is bit-equal to the by-value entry point's (the kernels run one body), and a set flag leaves
every buffer as it was.  One list holds tensors of 1, 255, 256, 257, 4096 and 100 003 elements: partial 8-bit blocks of 1, 255 and 1
(= 257 - 256) and 163 (= 100 003 mod 256) elements, a tensor shorter than a chunk of 65 536 and one of two chunks.  Every buffer sits
between 64-element fences (NaN, 0xA5 for the byte codes) that are compared with the data, as §16 does."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16 = torch.bfloat16
SIZES = (1, 255, 256, 257, 4096, 100003)
FENCE = 64
HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
STEP, COEF = 3, 0.37


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _fenced(t):
    """(the view a kernel gets, the whole buffer): t between two fences of FENCE elements of its dtype"""
    fill = 0xA5 if t.dtype == torch.uint8 else float("nan")
    whole = torch.full((t.numel() + 2 * FENCE,), fill, dtype=t.dtype, device=t.device)
    view = whole[FENCE:FENCE + t.numel()]
    view.copy_(t.reshape(-1))
    return view, whole


def _state(dev, bits):
    """per tensor: the argument lists of adamw_multi_ / adamw8_multi_ as fenced views, and every whole buffer"""
    from opendwm_amd import quant8, train_ops as T
    gen = torch.Generator().manual_seed(17)
    lists, wholes = None, []
    for n in SIZES:
        p = torch.randn(n, generator=gen)
        g = torch.randn(n, generator=gen) * torch.exp2(torch.randint(-6, 7, (n,), generator=gen).float())
        m = 0.1 * torch.randn(n, generator=gen)
        v = 0.01 * torch.rand(n, generator=gen) ** 2
        row = [p.to(dev), g.to(dev)]
        if bits == 8:
            code_m, code_v = quant8.device_codes(dev)
            mq, ma = T.quantize_blockwise8(m.to(dev), code_m)
            vq, va = T.quantize_blockwise8(v.to(dev), code_v, floor_positive=True)
            row += [mq, ma, vq, va]
        else:
            row += [m.to(dev), v.to(dev)]
        row.append(torch.zeros(n, dtype=bf16, device=dev))            # the bf16 compute copy
        pairs = [_fenced(t) for t in row]
        if lists is None:
            lists = [[] for _ in pairs]
        for lst, (view, whole) in zip(lists, pairs):
            lst.append(view)
            wholes.append(whole)
    return lists, wholes


def _same(a, b):
    """bit-equal, NaN fences included"""
    raw = lambda t: t.reshape(-1) if t.dtype == torch.uint8 else t.reshape(-1).view(torch.uint8)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw(a), raw(b))


def _step_fn(bits):
    from opendwm_amd import train_ops as T
    return T.adamw8_multi_ if bits == 8 else T.adamw_multi_


@pytest.mark.parametrize("with_cond", [True, False], ids=["cond", "cond_null"])
@pytest.mark.parametrize("bits", [32, 8])
def test_dev_entry_point_is_bit_equal_to_by_value(dev, bits, with_cond):
    from opendwm_amd import train_ops as T
    by_value, wholes_v = _state(dev, bits)
    by_dev, wholes_d = _state(dev, bits)
    before = [w.clone() for w in wholes_v]
    assert all(_same(a, b) for a, b in zip(wholes_v, wholes_d))
    coef = COEF if with_cond else 1.0
    _step_fn(bits)(*by_value, step=STEP, grad_scale=coef, **HYPER)
    hyper = T.adamw_hyper(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], STEP).to(dev)
    cond = torch.tensor([123.0, COEF, 0.0, 9.0], device=dev) if with_cond else None      # norm and the fourth value are not read
    _step_fn(bits)(*by_dev, step=-1, lr=float("nan"), grad_scale=float("nan"), device_operands=(hyper, cond),
                   **{k: v for k, v in HYPER.items() if k != "lr"})
    torch.cuda.synchronize()
    different = [i for i, (a, b) in enumerate(zip(wholes_v, wholes_d)) if not _same(a, b)]
    assert not different, (bits, different)
    per = len(wholes_v) // len(SIZES)
    moved = {i for i, (a, b) in enumerate(zip(wholes_v, before)) if not _same(a, b)}
    # the step happened: the parameters and the compute copy of every tensor changed, no gradient did (a one-element tensor keeps
    # its moment codes - the largest entry - so the moments are not listed here; they are compared above)
    assert all(i not in moved for i in range(1, len(wholes_v), per)), sorted(moved)
    assert all(i in moved and i + per - 1 in moved for i in range(0, len(wholes_v), per)), sorted(moved)
    for view in by_dev[0]:
        assert bool(torch.isfinite(view).all())
    for p, sh in zip(by_dev[0], by_dev[-1]):
        assert torch.equal(sh, p.to(bf16))


@pytest.mark.parametrize("bits", [32, 8])
def test_set_flag_leaves_every_buffer_alone(dev, bits):
    from opendwm_amd import train_ops as T
    lists, wholes = _state(dev, bits)
    before = [w.clone() for w in wholes]
    hyper = T.adamw_hyper(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], STEP).to(dev)
    for flag in (1.0, float("nan"), -2.0):                              # anything but zero
        cond = torch.tensor([float("inf"), COEF, flag, 0.0], device=dev)
        _step_fn(bits)(*lists, step=STEP, device_operands=(hyper, cond), **HYPER)
    torch.cuda.synchronize()
    changed = [i for i, (a, b) in enumerate(zip(wholes, before)) if not _same(a, b)]
    assert not changed, (bits, changed)
    # and the same launch with the flag clear does step (the skip is the flag's doing)
    _step_fn(bits)(*lists, step=STEP, device_operands=(hyper, torch.tensor([1.0, COEF, 0.0, 0.0], device=dev)), **HYPER)
    torch.cuda.synchronize()
    assert not _same(wholes[0], before[0])


def test_optimizer_step_with_device_operands_equals_by_value_step(dev):
    """AdamW.step(device_operands=(None, cond)): the hyper rows the optimizer stages itself (one pinned copy for both batches of an
    8-bit optimizer) give the parameters, states and compute copies of step(grad_scale=coef); a set flag plus undo_step() is a step
    that did not happen"""
    from opendwm_amd import train
    from opendwm_amd.blocks import STORE
    gen = torch.Generator().manual_seed(3)
    init = [torch.randn(n, generator=gen) for n in (12, 5000, 100003)]
    grads = [[torch.randn(t.shape, generator=gen) for t in init] for _ in range(3)]

    def run(route):
        STORE.bump()
        ps = [torch.nn.Parameter(t.clone().to(dev)) for t in init]
        opt = train.AdamW8bit(ps, lr=2e-4, weight_decay=0.01)
        for k, gs in enumerate(grads):
            for p, g in zip(ps, gs):
                p.grad = g.to(dev)
            [STORE.bf(p) for p in ps]
            if route == "value":
                if k != 1:
                    opt.step(grad_scale=COEF)
            else:
                opt.step(device_operands=(None, torch.tensor([1.0, COEF, float(k == 1), 0.0], device=dev)))
                if k == 1:
                    opt.undo_step()
        torch.cuda.synchronize()
        out = [p.detach().clone() for p in ps] + [STORE.bf(p).clone() for p in ps]
        for p in ps:
            out += [v.clone() for _, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
        return out
    a, b = run("value"), run("dev")
    assert len(a) == len(b) and all(_same(x.contiguous(), y.contiguous()) for x, y in zip(a, b))
