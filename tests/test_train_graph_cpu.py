"""Whole-step HIP graph of the trainer and the sync-free AdamW step, the part that needs no GPU: the constructor contract
of CTSDTrainer(graph=...), the C ABI additions dwm_adamw_multi_dev / dwm_adamw8_multi_dev (header, binding, the status codes their
argument checks return before any launch) and the host bookkeeping of AdamW.step(device_operands=...) / undo_step()."""
import ctypes as C
import inspect
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2


def _header():
    return open(os.path.join(ROOT, "include", "dwm_hip.h")).read()


# ------------------------------------------------------------------------------- trainer contract
def test_graph_argument_defaults_to_off():
    from opendwm_amd.pipeline import CTSDTrainer
    assert inspect.signature(CTSDTrainer.__init__).parameters["graph"].default is False
    absent, off = CTSDTrainer(torch.nn.Linear(4, 4)), CTSDTrainer(torch.nn.Linear(4, 4), graph=False)
    for tr in (absent, off):
        assert tr.graph is False and tr._graph is None and tr.graph_captures == 0 and tr.graph_replays == 0
    assert {k: v for k, v in vars(absent).items() if isinstance(v, (bool, int, float, str, type(None)))} == \
        {k: v for k, v in vars(off).items() if isinstance(v, (bool, int, float, str, type(None)))}
    off.graph_sync()                                  # a no-op without a graph step behind it
    assert off.skipped_steps == 0


def test_graph_refuses_what_it_does_not_capture():
    from opendwm_amd.pipeline import CTSDTrainer
    lin = lambda: torch.nn.Linear(4, 4)
    with pytest.raises(ValueError, match="ddp=True"):
        CTSDTrainer(lin(), graph=True, ddp=True)
    with pytest.raises(ValueError, match="grad_conditioning='fused'"):
        CTSDTrainer(lin(), graph=True, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="grad_conditioning='fused'"):
        CTSDTrainer(lin(), graph=True, training_config={"max_norm_for_grad_clip": 1.0})
    with pytest.raises(ValueError, match="grad_conditioning='fused'"):
        CTSDTrainer(lin(), graph=True, training_config={"enable_grad_scaler": True})
    with pytest.raises(ValueError, match="not on the device"):
        CTSDTrainer(lin(), graph=True)
    with pytest.raises(ValueError, match="not on the device"):      # the fused route is served; a host model still is not
        CTSDTrainer(lin(), graph=True, grad_conditioning="fused", max_grad_norm=1.0)
    # nothing that worked before raises: the same arguments without graph=True
    CTSDTrainer(lin(), max_grad_norm=1.0)
    CTSDTrainer(lin(), training_config={"enable_grad_scaler": True, "max_norm_for_grad_clip": 1.0})


# ------------------------------------------------------------------------------- C ABI
def test_abi_additions_are_declared():
    from opendwm_amd import _lib
    hdr = _header()
    assert re.search(r"^int dwm_adamw_multi_dev\(const dwm_adamw_item\* items,", hdr, re.M)
    assert re.search(r"^int dwm_adamw8_multi_dev\(const dwm_adamw8_item\* items,", hdr, re.M)
    for name, by_value in (("dwm_adamw_multi_dev", "dwm_adamw_multi"), ("dwm_adamw8_multi_dev", "dwm_adamw8_multi")):
        res, args = _lib.SIGNATURES[name]
        res0, args0 = _lib.SIGNATURES[by_value]
        # the by-value arguments with (lr, bias_corr1, bias_corr2, grad_scale) gone and (hyper, cond) in front of beta1
        n_lead = len(args0) - 9                                        # items .. chunk [, code_m, code_v]
        assert res is res0 and list(args) == list(args0[:n_lead]) + [_lib._vp, _lib._vp] + [_lib._f32] * 4 + [_lib._vp], name
        proto = re.search(rf"^int {name}\((.*?)\);", hdr, re.M | re.S).group(1)
        assert len(proto.split(",")) == len(args), name
        assert "const float* hyper, const float* cond" in " ".join(proto.split())
    assert len(_lib.SIGNATURES["dwm_adamw_multi_dev"][1]) == 12 and len(_lib.SIGNATURES["dwm_adamw8_multi_dev"][1]) == 14
    assert _lib.ABI_VERSION == 18 and re.search(r"^#define DWM_ABI_VERSION 18$", hdr, re.M)      # additions only
    assert len(_lib.SIGNATURES["dwm_adamw_multi"][1]) == 14 and len(_lib.SIGNATURES["dwm_adamw8_multi"][1]) == 16


def test_dev_entry_points_check_their_arguments_on_the_host():
    """every refusal comes before the launch, so the codes can be read without a device; the pointers are never dereferenced"""
    from opendwm_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) // 64 * 64
    items, bi, bs, hyper, cond, cm, cv = (base + 256 * i for i in range(7))
    chunk = 1 << 16

    def call32(items=items, bi=bi, bs=bs, n_blocks=1, chunk=chunk, hyper=hyper, cond=cond):
        return lib.dwm_adamw_multi_dev(items, bi, bs, n_blocks, chunk, hyper, cond, 0.9, 0.999, 1e-8, 0.01, None)

    def call8(items=items, bi=bi, bs=bs, n_blocks=1, chunk=chunk, cm=cm, cv=cv, hyper=hyper, cond=cond):
        return lib.dwm_adamw8_multi_dev(items, bi, bs, n_blocks, chunk, cm, cv, hyper, cond, 0.9, 0.999, 1e-8, 0.01, None)
    for call in (call32, call8):
        for bad in (dict(items=None), dict(bi=None), dict(bs=None), dict(n_blocks=0), dict(n_blocks=-1), dict(chunk=0), dict(hyper=None)):
            assert call(**bad) == EINVAL, (call.__name__, bad)
        for bad in (dict(hyper=hyper + 1), dict(hyper=hyper + 2), dict(cond=cond + 2), dict(cond=cond + 3), dict(hyper=hyper + 2, cond=None)):
            assert call(**bad) == EALIGN, (call.__name__, bad)
        assert call(hyper=None, cond=cond + 1) == EINVAL                 # the null pointer is reported first
    for bad in (dict(cm=None), dict(cv=None), dict(chunk=1000), dict(chunk=chunk + 128)):
        assert call8(**bad) == EINVAL, bad
    # the by-value entry points refuse the same table arguments with the same code
    assert lib.dwm_adamw_multi(None, bi, bs, 1, chunk, 1e-4, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001, 1.0, None) == EINVAL
    assert lib.dwm_adamw8_multi(items, bi, bs, 1, 1000, cm, cv, 1e-4, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001, 1.0, None) == EINVAL


# ------------------------------------------------------------------------------- wrappers and optimizer bookkeeping
def test_hyper_row_holds_the_by_value_bits():
    """the float32 the kernel reads from `hyper` is the float32 ctypes makes of the by-value argument"""
    from opendwm_amd import train_ops as T
    for lr, b1, b2, step in ((2e-4, 0.9, 0.999, 1), (1.234567e-4, 0.9, 0.95, 7), (3e-5, 0.8, 0.9999, 12345)):
        row = T.adamw_hyper(lr, b1, b2, step)
        sc = T._adamw_scalars(lr, b1, b2, 1e-8, 0.01, step, 1.0)
        want = [C.c_float(sc[0]).value, C.c_float(sc[5]).value, C.c_float(sc[6]).value, 0.0]
        assert row.dtype == torch.float32 and row.tolist() == want
    out = torch.full((2, 4), 7.0)
    assert T.adamw_hyper(1e-3, 0.9, 0.999, 3, out=out[1]) is not None and out[0].tolist() == [7.0] * 4 and out[1, 0].item() == C.c_float(1e-3).value


def test_device_operands_are_checked():
    from opendwm_amd import train_ops as T
    cpu = torch.device("cpu")
    ok = torch.zeros(4)
    assert T._dev_operands((ok, None), cpu, "t") == (ok, None)
    for bad in (torch.zeros(2), torch.zeros(4, dtype=torch.float64), torch.zeros(8)[::2], None, 3.0):
        with pytest.raises(RuntimeError, match="device_operands hyper"):
            T._dev_operands((bad, None), cpu, "t")
    with pytest.raises(RuntimeError, match="device_operands cond"):
        T._dev_operands((ok, torch.zeros(2)), cpu, "t")


@pytest.mark.parametrize("bits", [32, 8])
def test_step_with_device_operands_routes_and_undoes(bits, monkeypatch):
    """step(device_operands=...) hands the operands to the same batches in the same order as the by-value step and counts the step;
    undo_step() takes the count back and drops a state the undone step created - the state of an optimizer whose step was skipped"""
    from opendwm_amd import train, train_ops as T
    calls = []
    monkeypatch.setattr(T, "adamw_multi_", lambda *a, **kw: calls.append((32, a, kw)))
    monkeypatch.setattr(T, "adamw8_multi_", lambda *a, **kw: calls.append((8, a, kw)))
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (8, 5000, 12)]
    frozen = torch.nn.Parameter(torch.randn(4), requires_grad=False)
    opt = (train.AdamW8bit if bits == 8 else train.AdamW)(ps + [frozen], lr=2e-4)
    for p in ps:
        p.grad = torch.ones_like(p)
    hyper, cond = torch.zeros(4), torch.zeros(4)
    opt.step(device_operands=(hyper, cond))
    kinds = [k for k, _, _ in calls]
    assert kinds == ([8, 32] if bits == 8 else [32])
    for _, a, kw in calls:
        assert kw["device_operands"][0] is hyper and kw["device_operands"][1] is cond and kw["step"] == 1
    assert all(float(opt.state[p]["step"]) == 1.0 for p in ps) and frozen not in opt.state
    opt.undo_step()
    assert len(opt.state) == 0                          # as if the step had not been called
    opt.undo_step()                                     # nothing left to undo
    calls.clear()
    opt.step()                                          # the by-value route: no device_operands keyword at all
    assert all("device_operands" not in kw and kw["step"] == 1 for _, _, kw in calls) and [k for k, _, _ in calls] == kinds
    opt.step(device_operands=(hyper, None))
    assert all(float(opt.state[p]["step"]) == 2.0 for p in ps)
    opt.undo_step()
    assert all(float(opt.state[p]["step"]) == 1.0 for p in ps) and len(opt.state) == len(ps)
