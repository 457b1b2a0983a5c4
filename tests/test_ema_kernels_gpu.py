"""GPU leg (`-m gpu`) of the EMA entry points (include/dwm_hip.h "EMA weights"): dwm_adamw_ema_multi, dwm_adamw8_ema_multi,
their _dev forms, dwm_ema_multi and dwm_ema_swap_multi.

One list holds tensors of 1, 255, 256, 257, 4096, 65 535, 65 537 and 100 003 elements: partial 8-bit blocks, one element either side
of a chunk of 65 536, and two chunks.  Every buffer sits between 64-element fences (NaN, 0xA5 for the byte codes) that are compared
with the data.  The shadows of the odd-numbered tensors start one element late in their buffer, so they are 4-byte aligned and no
more: the 8-bit form takes its element path for them and its vector path for the others.

The shadow bound: |e' - fp64(e + omd * (p' - e))| <= 2^-21 * max(|e|, |p'|) with p' read back from the kernel - five fp32 roundings
of magnitude at most 2^-24 * max, with or without FMA contraction (the rounding of omd to fp32 among them: the reference takes the
caller's double), rounded up to a power of two.  It holds for any correct fp32 implementation."""
import pytest
import torch

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16 = torch.bfloat16
SIZES = (1, 255, 256, 257, 4096, 65535, 65537, 100003)
FENCE = 64
HYPER = dict(lr=2e-4, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.01)
STEP, COEF = 3, 0.37
BOUND = 2.0 ** -21


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _fenced(t, shift=0):
    """(the view a kernel gets, the whole buffer): t between two fences of at least FENCE elements of its dtype, `shift` elements late"""
    fill = 0xA5 if t.dtype == torch.uint8 else float("nan")
    whole = torch.full((t.numel() + 2 * FENCE + shift,), fill, dtype=t.dtype, device=t.device)
    view = whole[FENCE + shift:FENCE + shift + t.numel()]
    view.copy_(t.reshape(-1))
    return view, whole


@pytest.fixture(scope="module")
def host_data():
    """the values of every test, drawn once: per tensor (p, g, m, v, e)"""
    gen = torch.Generator().manual_seed(29)
    rows = []
    for n in SIZES:
        p = torch.randn(n, generator=gen)
        g = torch.randn(n, generator=gen) * torch.exp2(torch.randint(-6, 7, (n,), generator=gen).float())
        m = 0.1 * torch.randn(n, generator=gen)
        v = 0.01 * torch.rand(n, generator=gen) ** 2
        e = p + 0.05 * torch.randn(n, generator=gen) * torch.exp2(torch.randint(-8, 3, (n,), generator=gen).float())
        rows.append((p, g, m, v, e))
    return rows


def _state(dev, host_data, bits):
    """(the argument lists of adamw_multi_ / adamw8_multi_ as fenced views, the fenced shadows, every whole buffer of the former,
    every whole buffer of the latter)"""
    from opendwm_amd import quant8, train_ops as T
    lists, wholes, emas, ema_wholes = None, [], [], []
    for i, (p, g, m, v, e) in enumerate(host_data):
        row = [p.to(dev), g.to(dev)]
        if bits == 8:
            code_m, code_v = quant8.device_codes(dev)
            mq, ma = T.quantize_blockwise8(m.to(dev), code_m)
            vq, va = T.quantize_blockwise8(v.to(dev), code_v, floor_positive=True)
            row += [mq, ma, vq, va]
        else:
            row += [m.to(dev), v.to(dev)]
        row.append(torch.zeros(p.numel(), dtype=bf16, device=dev))            # the bf16 compute copy
        pairs = [_fenced(t) for t in row]
        if lists is None:
            lists = [[] for _ in pairs]
        for lst, (view, whole) in zip(lists, pairs):
            lst.append(view)
            wholes.append(whole)
        view, whole = _fenced(e.to(dev), shift=i % 2)
        emas.append(view)
        ema_wholes.append(whole)
    return lists, emas, wholes, ema_wholes


def _same(a, b):
    """bit-equal, NaN fences included"""
    raw = lambda t: t.reshape(-1) if t.dtype == torch.uint8 else t.reshape(-1).view(torch.uint8)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw(a.contiguous()), raw(b.contiguous()))


def _fences_intact(views, wholes):
    for view, whole in zip(views, wholes):
        start = view.storage_offset() - whole.storage_offset()
        if not (bool(torch.isnan(whole[:start]).all()) and bool(torch.isnan(whole[start + view.numel():]).all())):
            return False
    return True


def _plain(bits):
    from opendwm_amd import train_ops as T
    return T.adamw8_multi_ if bits == 8 else T.adamw_multi_


def _fused(bits):
    from opendwm_amd import train_ops as T
    return T.adamw8_ema_multi_ if bits == 8 else T.adamw_ema_multi_


def _check_bound(e_new, e_old, p_new, omd, what):
    e64, p64 = e_old.double(), p_new.double()
    want = e64 + omd * (p64 - e64)
    err = (e_new.double() - want).abs()
    lim = BOUND * torch.maximum(e64.abs(), p64.abs())
    worst = float((err - lim).max())
    assert bool((err <= lim).all()), (what, worst, float(err.max()))
    assert bool(torch.isfinite(e_new).all()), what


@pytest.mark.parametrize("route", ["value", "dev"])
@pytest.mark.parametrize("bits", [32, 8])
def test_fused_entries_are_bit_equal_to_the_plain_ones(dev, host_data, bits, route):
    from opendwm_amd import train_ops as T
    omd = 0.1
    plain, _, wholes_p, _ = _state(dev, host_data, bits)
    fused, emas, wholes_f, ema_wholes = _state(dev, host_data, bits)
    e_before = [e.clone() for e in emas]
    assert all(_same(a, b) for a, b in zip(wholes_p, wholes_f))
    if route == "value":
        _plain(bits)(*plain, step=STEP, grad_scale=COEF, **HYPER)
        _fused(bits)(*fused, emas, step=STEP, grad_scale=COEF, one_minus_decay=omd, **HYPER)
    else:
        cond = torch.tensor([123.0, COEF, 0.0, 9.0], device=dev)
        hyper3 = T.adamw_hyper(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], STEP).to(dev)
        hyper4 = T.adamw_hyper(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], STEP, one_minus_decay=omd).to(dev)
        rest = {k: v for k, v in HYPER.items() if k != "lr"}
        _plain(bits)(*plain, step=-1, lr=float("nan"), device_operands=(hyper3, cond), **rest)
        _fused(bits)(*fused, emas, step=-1, lr=float("nan"), one_minus_decay=float("nan"), device_operands=(hyper4, cond), **rest)
    torch.cuda.synchronize()
    different = [i for i, (a, b) in enumerate(zip(wholes_p, wholes_f)) if not _same(a, b)]
    assert not different, (bits, route, different)                      # p, g, m, v, the scales, the bf16 copy and all their fences
    assert _fences_intact(emas, ema_wholes)
    for p, sh in zip(fused[0], fused[-1]):
        assert torch.equal(sh, p.to(bf16))
    for i, (e, e0, p) in enumerate(zip(emas, e_before, fused[0])):
        assert not _same(e, e0) or e.numel() == 1
        _check_bound(e, e0, p, omd, (bits, route, SIZES[i]))


@pytest.mark.parametrize("omd", [1e-4, 0.1, 0.5])
@pytest.mark.parametrize("bits", [32, 8])
def test_shadows_are_within_the_fp32_bound(dev, host_data, bits, omd):
    lists, emas, _, ema_wholes = _state(dev, host_data, bits)
    e_before = [e.clone() for e in emas]
    _fused(bits)(*lists, emas, step=STEP, one_minus_decay=omd, **HYPER)
    torch.cuda.synchronize()
    assert _fences_intact(emas, ema_wholes)
    for i, (e, e0, p) in enumerate(zip(emas, e_before, lists[0])):
        _check_bound(e, e0, p, omd, (bits, omd, SIZES[i]))


@pytest.mark.parametrize("bits", [32, 8])
def test_the_two_ends_of_the_decay_range_are_exact(dev, host_data, bits):
    lists, emas, _, ema_wholes = _state(dev, host_data, bits)
    before = [w.clone() for w in ema_wholes]
    p_before = [p.clone() for p in lists[0]]
    _fused(bits)(*lists, emas, step=STEP, one_minus_decay=0.0, **HYPER)               # decay 1: the shadows stay, bit for bit
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(ema_wholes, before))
    assert all(not _same(p, p0) for p, p0 in zip(lists[0], p_before))                 # ... while the step took place
    _fused(bits)(*lists, emas, step=STEP + 1, one_minus_decay=1.0, **HYPER)           # decay 0: the shadows are the new parameters
    torch.cuda.synchronize()
    assert all(_same(e, p) for e, p in zip(emas, lists[0])) and _fences_intact(emas, ema_wholes)


@pytest.mark.parametrize("route", ["value", "dev"])
@pytest.mark.parametrize("bits", [32, 8])
def test_entries_without_a_shadow_are_updated_as_by_the_plain_entry(dev, host_data, bits, route):
    from opendwm_amd import train_ops as T
    omd = 0.25
    plain, _, wholes_p, _ = _state(dev, host_data, bits)
    fused, emas, wholes_f, ema_wholes = _state(dev, host_data, bits)
    before = [w.clone() for w in ema_wholes]
    mixed = [e if i % 3 != 1 else None for i, e in enumerate(emas)]                    # tensors 1, 4, 7 have none
    if route == "value":
        _plain(bits)(*plain, step=STEP, **HYPER)
        _fused(bits)(*fused, mixed, step=STEP, one_minus_decay=omd, **HYPER)
    else:
        hyper = T.adamw_hyper(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], STEP, one_minus_decay=omd).to(dev)
        _plain(bits)(*plain, step=STEP, device_operands=(hyper, None), **HYPER)
        _fused(bits)(*fused, mixed, step=STEP, one_minus_decay=omd, device_operands=(hyper, None), **HYPER)
    torch.cuda.synchronize()
    different = [i for i, (a, b) in enumerate(zip(wholes_p, wholes_f)) if not _same(a, b)]
    assert not different, (bits, route, different)
    for i, (w, w0, e, p) in enumerate(zip(ema_wholes, before, emas, fused[0])):
        if mixed[i] is None:
            assert _same(w, w0), i                                                     # nobody wrote to a buffer that was not handed in
        else:
            _check_bound(e, w0[FENCE + i % 2:FENCE + i % 2 + e.numel()], p, omd, (bits, route, SIZES[i]))
    assert _fences_intact(emas, ema_wholes)


@pytest.mark.parametrize("bits", [32, 8])
def test_set_flag_leaves_every_buffer_alone_shadows_included(dev, host_data, bits):
    from opendwm_amd import train_ops as T
    lists, emas, wholes, ema_wholes = _state(dev, host_data, bits)
    before = [w.clone() for w in wholes + ema_wholes]
    hyper = T.adamw_hyper(HYPER["lr"], HYPER["beta1"], HYPER["beta2"], STEP, one_minus_decay=0.3).to(dev)
    for flag in (1.0, float("nan")):                                     # anything but zero
        cond = torch.tensor([float("inf"), COEF, flag, 0.0], device=dev)
        _fused(bits)(*lists, emas, step=STEP, one_minus_decay=0.3, device_operands=(hyper, cond), **HYPER)
        T.ema_multi_(emas, lists[0], one_minus_decay=0.3, device_operands=(hyper, cond))
        T.ema_multi_(emas, lists[0], one_minus_decay=0.3, device_operands=(None, cond))
    torch.cuda.synchronize()
    changed = [i for i, (a, b) in enumerate(zip(wholes + ema_wholes, before)) if not _same(a, b)]
    assert not changed, (bits, changed)
    # and the same launch with the flag clear does step and average (the skip is the flag's doing)
    _fused(bits)(*lists, emas, step=STEP, one_minus_decay=0.3, device_operands=(hyper, torch.tensor([1.0, COEF, 0.0, 0.0], device=dev)),
                 **HYPER)
    torch.cuda.synchronize()
    assert not _same(wholes[0], before[0]) and not _same(ema_wholes[-1], before[-1])


def test_ema_multi_is_the_element_rule_alone(dev, host_data):
    from opendwm_amd import train_ops as T
    lists, emas, wholes, ema_wholes = _state(dev, host_data, 32)
    before = [w.clone() for w in wholes]
    for omd, operands in ((0.1, None), (1e-4, None), (0.5, "hyper")):
        e0 = [e.clone() for e in emas]
        if operands is None:
            T.ema_multi_(emas, lists[0], one_minus_decay=omd)
        else:                                                            # hyper[3] overrides the by-value scalar; a clear flag lets it run
            hyper = torch.tensor([float("nan"), float("nan"), float("nan"), omd], device=dev)
            T.ema_multi_(emas, lists[0], one_minus_decay=0.0, device_operands=(hyper, torch.zeros(4, device=dev)))
        torch.cuda.synchronize()
        for i, (e, old, p) in enumerate(zip(emas, e0, lists[0])):
            assert not _same(e, old) or e.numel() == 1
            _check_bound(e, old, p, omd, (omd, operands, SIZES[i]))
    assert all(_same(a, b) for a, b in zip(wholes, before))              # p (and everything else) untouched
    assert _fences_intact(emas, ema_wholes)
    e0 = [w.clone() for w in ema_wholes]
    T.ema_multi_(emas, lists[0], one_minus_decay=0.0)                    # decay 1: nothing moves
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(ema_wholes, e0))
    T.ema_multi_(emas, lists[0], one_minus_decay=1.0)                    # decay 0: the shadows are the parameters
    torch.cuda.synchronize()
    assert all(_same(e, p) for e, p in zip(emas, lists[0])) and _fences_intact(emas, ema_wholes)
    with pytest.raises(ValueError):
        T.ema_multi_(emas, lists[0], one_minus_decay=1.5)


@pytest.mark.parametrize("with_copy", [True, False], ids=["bf16_copy", "bf16_null"])
def test_swap_exchanges_in_place_and_two_swaps_restore(dev, host_data, with_copy):
    from opendwm_amd import _lib
    from opendwm_amd import train_ops as T
    lists, emas, wholes, ema_wholes = _state(dev, host_data, 32)
    ps, copies = lists[0], lists[-1]
    per = len(wholes) // len(SIZES)
    p_wholes, c_wholes = wholes[0::per], wholes[per - 1::per]
    # compute copies as they stand before an exchange: the bf16 of p
    for p, c in zip(ps, copies):
        c.copy_(p.to(bf16))
    before = [w.clone() for w in wholes + ema_wholes]
    p0, e0 = [p.clone() for p in ps], [e.clone() for e in emas]
    T.ema_swap_multi_(ps, emas, copies if with_copy else [None] * len(ps))
    torch.cuda.synchronize()
    assert all(_same(p, e) for p, e in zip(ps, e0)) and all(_same(e, p) for e, p in zip(emas, p0))
    assert _fences_intact(emas, ema_wholes) and _fences_intact(ps, p_wholes) and _fences_intact(copies, c_wholes)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    for p, c, old in zip(ps, copies, p0):
        if not with_copy:
            assert _same(c, old.to(bf16))                                # a NULL copy is accepted and nothing is written for it
            continue
        n4 = (p.numel() + 3) // 4 * 4                                    # dwm_cast_f32_to_bf16 wants n % 4 == 0 and aligned buffers
        src, dst = torch.zeros(n4, device=dev), torch.zeros(n4, dtype=bf16, device=dev)
        src[:p.numel()].copy_(p)
        assert lib.dwm_cast_f32_to_bf16(src.data_ptr(), dst.data_ptr(), n4, stream) == 0
        torch.cuda.synchronize()
        assert _same(c, dst[:p.numel()])
    T.ema_swap_multi_(ps, emas, copies if with_copy else [None] * len(ps))
    torch.cuda.synchronize()
    changed = [i for i, (a, b) in enumerate(zip(wholes + ema_wholes, before)) if not _same(a, b)]
    assert not changed, changed
