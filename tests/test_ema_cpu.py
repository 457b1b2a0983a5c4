"""EMA of the weights, the part that needs no GPU: the six C ABI additions (header, binding, item mirrors, the status
codes their argument checks return before any launch), train.EMA's decay schedule against diffusers 0.31 EMAModel.get_decay restated
here, its state dict, and the constructor / context / checkpoint contract of CTSDTrainer(ema=...)."""
import ctypes as C
import inspect
import math
import os
import re
import warnings

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN = -1, -2
NEW = {"dwm_adamw_ema_multi": 15, "dwm_adamw8_ema_multi": 17, "dwm_adamw_ema_multi_dev": 12, "dwm_adamw8_ema_multi_dev": 14,
       "dwm_ema_multi": 9, "dwm_ema_swap_multi": 6}


def _header():
    return open(os.path.join(ROOT, "include", "dwm_hip.h")).read()


# ------------------------------------------------------------------------------- C ABI
def test_abi_additions_are_declared():
    from opendwm_amd import _lib
    hdr = _header()
    for name, arity in NEW.items():
        proto = re.search(rf"^int {name}\((.*?)\);", hdr, re.M | re.S)
        assert proto, name
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._i32 and len(proto.group(1).split(",")) == arity == len(args), name
    # the fused forms: the plain entry's arguments, one float more in front of the stream (by value) / the same list (_dev)
    for plain, fused in (("dwm_adamw_multi", "dwm_adamw_ema_multi"), ("dwm_adamw8_multi", "dwm_adamw8_ema_multi")):
        args0, args = _lib.SIGNATURES[plain][1], _lib.SIGNATURES[fused][1]
        assert list(args) == list(args0[:-1]) + [_lib._f32, _lib._vp]
        assert list(_lib.SIGNATURES[fused + "_dev"][1]) == list(_lib.SIGNATURES[plain + "_dev"][1])
        proto = " ".join(re.search(rf"^int {fused}\((.*?)\);", hdr, re.M | re.S).group(1).split())
        assert proto.endswith("float one_minus_decay, void* stream")
    assert _lib.ABI_VERSION == 18 and re.search(r"^#define DWM_ABI_VERSION 18$", hdr, re.M)      # additions only
    assert len(_lib.SIGNATURES["dwm_adamw_multi"][1]) == 14 and len(_lib.SIGNATURES["dwm_adamw8_multi"][1]) == 16


def test_item_mirrors_have_the_header_field_order():
    from opendwm_amd import _lib
    hdr = _header()
    for struct, mirror in (("dwm_adamw_ema_item", _lib.AdamWEmaItem), ("dwm_adamw8_ema_item", _lib.AdamW8EmaItem),
                           ("dwm_ema_item", _lib.EmaItem), ("dwm_ema_swap_item", _lib.EmaSwapItem)):
        body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", hdr, re.S).group(1)
        fields = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
        assert fields == [f[0] for f in mirror._fields_], struct
        assert C.sizeof(mirror) == 8 * len(fields), struct            # rows of int64 in train_ops._items
    # the existing items with `ema` before n
    plain8 = [f[0] for f in _lib.AdamW8Item._fields_]
    assert [f[0] for f in _lib.AdamW8EmaItem._fields_] == plain8[:-1] + ["ema", "n"]
    assert [f[0] for f in _lib.AdamWEmaItem._fields_] == ["p", "g", "m", "v", "p_bf16", "ema", "n"]


def test_entry_points_check_their_arguments_on_the_host():
    """every refusal comes before the launch, so the codes can be read without a device; the pointers are never dereferenced"""
    from opendwm_amd import _lib
    lib = _lib.load()
    buf = (C.c_char * 4096)()
    base = (C.addressof(buf) + 63) // 64 * 64
    items, bi, bs, hyper, cond, cm, cv = (base + 256 * i for i in range(7))
    chunk = 1 << 16
    sc = (1e-4, 0.9, 0.999, 1e-8, 0.01, 0.1, 0.001, 1.0)

    def val32(items=items, bi=bi, bs=bs, n_blocks=1, chunk=chunk, omd=0.5):
        return lib.dwm_adamw_ema_multi(items, bi, bs, n_blocks, chunk, *sc, omd, None)

    def val8(items=items, bi=bi, bs=bs, n_blocks=1, chunk=chunk, cm=cm, cv=cv, omd=0.5):
        return lib.dwm_adamw8_ema_multi(items, bi, bs, n_blocks, chunk, cm, cv, *sc, omd, None)

    def dev32(items=items, bi=bi, bs=bs, n_blocks=1, chunk=chunk, hyper=hyper, cond=cond):
        return lib.dwm_adamw_ema_multi_dev(items, bi, bs, n_blocks, chunk, hyper, cond, 0.9, 0.999, 1e-8, 0.01, None)

    def dev8(items=items, bi=bi, bs=bs, n_blocks=1, chunk=chunk, cm=cm, cv=cv, hyper=hyper, cond=cond):
        return lib.dwm_adamw8_ema_multi_dev(items, bi, bs, n_blocks, chunk, cm, cv, hyper, cond, 0.9, 0.999, 1e-8, 0.01, None)

    def ema(items=items, bi=bi, bs=bs, n_blocks=1, chunk=chunk, omd=0.5, hyper=None, cond=None):
        return lib.dwm_ema_multi(items, bi, bs, n_blocks, chunk, omd, hyper, cond, None)

    def swap(items=items, bi=bi, bs=bs, n_blocks=1, chunk=chunk):
        return lib.dwm_ema_swap_multi(items, bi, bs, n_blocks, chunk, None)
    tables = (dict(items=None), dict(bi=None), dict(bs=None), dict(n_blocks=0), dict(n_blocks=-1), dict(chunk=0), dict(chunk=-256))
    for call in (val32, val8, dev32, dev8, ema, swap):
        for bad in tables:
            assert call(**bad) == EINVAL, (call.__name__, bad)
    for call in (val32, val8, ema):
        for omd in (-0.1, 1.5, float("nan")):
            assert call(omd=omd) == EINVAL, (call.__name__, omd)
    for call in (dev32, dev8):
        assert call(hyper=None) == EINVAL
        for bad in (dict(hyper=hyper + 1), dict(hyper=hyper + 2), dict(cond=cond + 2), dict(cond=cond + 3), dict(hyper=hyper + 2, cond=None)):
            assert call(**bad) == EALIGN, (call.__name__, bad)
        assert call(hyper=None, cond=cond + 1) == EINVAL                 # the null pointer is reported first
    for bad in (dict(hyper=hyper + 1), dict(hyper=hyper + 2, cond=cond), dict(cond=cond + 2), dict(hyper=hyper, cond=cond + 3)):
        assert ema(**bad) == EALIGN, bad
    assert ema(omd=float("nan"), hyper=hyper + 2) == EALIGN              # with a hyper row the by-value scalar is not looked at
    for call in (val8, dev8):
        for bad in (dict(cm=None), dict(cv=None), dict(chunk=1000), dict(chunk=chunk + 128)):
            assert call(**bad) == EINVAL, (call.__name__, bad)


def test_hyper_row_carries_one_minus_decay_in_the_unused_float():
    from opendwm_amd import train_ops as T
    row = T.adamw_hyper(2e-4, 0.9, 0.999, 3)
    assert row[3].item() == 0.0                                          # today's bits without the keyword
    with_ema = T.adamw_hyper(2e-4, 0.9, 0.999, 3, one_minus_decay=0.125)
    assert with_ema[:3].tolist() == row[:3].tolist() and with_ema[3].item() == 0.125
    cpu, ok3, ok4 = torch.device("cpu"), torch.zeros(3), torch.zeros(4)
    assert T._dev_operands((ok3, None), cpu, "t") == (ok3, None)
    with pytest.raises(RuntimeError, match="device_operands hyper"):
        T._dev_operands((ok3, None), cpu, "t", hyper_floats=4)
    assert T._dev_operands((ok4, ok3), cpu, "t", hyper_floats=4) == (ok4, ok3)


# ------------------------------------------------------------------------------- train.EMA
def _diffusers_get_decay(optimization_step, decay, min_decay, update_after_step, use_ema_warmup, inv_gamma, power):
    """diffusers 0.31 training_utils.EMAModel.get_decay, restated"""
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    if use_ema_warmup:
        cur_decay_value = 1 - (1 + step / inv_gamma) ** -power
    else:
        cur_decay_value = (1 + step) / (10 + step)
    cur_decay_value = min(cur_decay_value, decay)
    cur_decay_value = max(cur_decay_value, min_decay)
    return cur_decay_value


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("after", [0, 5])
def test_get_decay_is_diffusers(warmup, after):
    from opendwm_amd import train
    ps = [torch.nn.Parameter(torch.zeros(3))]
    for decay, min_decay, inv_gamma, power in ((0.9999, 0.0, 1.0, 2 / 3), (0.5, 0.0, 1.0, 2 / 3), (0.9999, 0.4, 2.0, 0.75),
                                               (0.75, 0.75, 1.0, 2 / 3)):
        kw = dict(decay=decay, min_decay=min_decay, update_after_step=after, use_ema_warmup=warmup, inv_gamma=inv_gamma, power=power)
        ema = train.EMA(ps, **kw)
        for step in (0, 1, 2, 10, 1000):
            want = _diffusers_get_decay(step, **kw)
            assert ema.get_decay(step) == want, (kw, step)
            assert want == 0.0 or min_decay <= want <= decay
    # the clamps bite: the top one late, the bottom one early
    ema = train.EMA(ps, decay=0.5, min_decay=0.4, update_after_step=after, use_ema_warmup=warmup)
    assert ema.get_decay(1000) == 0.5 and ema.get_decay(after + 1) == 0.0       # before the first averaged step: 0, not min_decay
    assert ema.get_decay(after + 2) == 0.4                                       # (1 + 1) / (10 + 1) = 0.18 and 1 - 2 ** -(2 / 3) = 0.37
    # advance(): the counter first, then that step's 1 - decay, as EMAModel.step does
    ema = train.EMA(ps, decay=0.9, update_after_step=after, use_ema_warmup=warmup)
    for n in range(1, after + 5):
        assert ema.advance() == 1.0 - _diffusers_get_decay(n, 0.9, 0.0, after, warmup, 1.0, 2 / 3) and ema.optimization_step == n


def test_ema_holds_shadows_of_the_trainable_parameters_only():
    from opendwm_amd import train
    a, b = torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(2, 3))
    frozen = torch.nn.Parameter(torch.randn(4), requires_grad=False)
    ema = train.EMA([("a", a), ("frozen", frozen), ("b", b), ("a_again", a)])
    assert [n for n, _ in ema.named_shadows()] == ["a", "b"]
    assert ema.shadow_of(frozen) is None and torch.equal(ema.shadow_of(a), a.detach()) and ema.shadow_of(a).data_ptr() != a.data_ptr()
    assert ema.shadow_of(b).dtype == torch.float32 and ema.shadow_of(b).shape == b.shape and not ema.swapped
    assert [n for n, _ in train.EMA([a, frozen, b]).named_shadows()] == ["0", "2"]
    with pytest.raises(ValueError):
        train.EMA([a], decay=0.5, min_decay=0.6)
    with pytest.raises(ValueError):
        train.EMA([torch.nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))])
    assert "deliberate difference" in " ".join(train.EMA.__doc__.lower().split())


def test_ema_state_dict_round_trips():
    from opendwm_amd import train
    lin = torch.nn.Linear(4, 3)
    kw = dict(decay=0.99, min_decay=0.1, update_after_step=2, use_ema_warmup=True, inv_gamma=2.0, power=0.75)
    ema = train.EMA(list(lin.named_parameters()), **kw)
    for _ in range(7):
        ema.advance()
    for _, e in ema.named_shadows():
        e.add_(1.5)
    sd = ema.state_dict()
    assert set(sd) == set(kw) | {"optimization_step", "shadows"} and set(sd["shadows"]) == {"weight", "bias"}
    assert {k: sd[k] for k in kw} == kw and sd["optimization_step"] == 7
    other = train.EMA(list(torch.nn.Linear(4, 3).named_parameters()))
    other.load_state_dict({k: (v if k != "shadows" else {n: t.clone() for n, t in v.items()}) for k, v in sd.items()})
    assert other.optimization_step == 7 and {k: getattr(other, k) for k in kw} == kw
    for (n, e), (n2, e2) in zip(ema.named_shadows(), other.named_shadows()):
        assert n == n2 and torch.equal(e, e2) and e.data_ptr() != e2.data_ptr()
    assert other.get_decay(8) == ema.get_decay(8)
    with pytest.raises(RuntimeError, match="missing"):
        other.load_state_dict(dict(sd, shadows={"weight": sd["shadows"]["weight"]}))
    # averaged_state_dict: the model's keys, shadows where there are some, the parameters' own values elsewhere
    lin.bias.requires_grad_(False)
    part = train.EMA(list(lin.named_parameters()))
    part.shadow_of(lin.weight).mul_(2.0)
    avg = part.averaged_state_dict(lin)
    assert list(avg) == ["weight", "bias"] and torch.equal(avg["weight"], 2.0 * lin.weight.detach()) and torch.equal(avg["bias"], lin.bias.detach())


# ------------------------------------------------------------------------------- optimizer routing
@pytest.mark.parametrize("bits", [32, 8])
def test_step_routes_shadowed_parameters_to_the_fused_entries(bits, monkeypatch):
    """AdamW.step(ema=...): the batches with a shadow go to the _ema_ wrappers with this step's 1 - decay, shadows without a gradient to
    one ema_multi_ call, and ema=None makes the calls it always made"""
    from opendwm_amd import train, train_ops as T
    calls = []
    for name in ("adamw_multi_", "adamw8_multi_", "adamw_ema_multi_", "adamw8_ema_multi_", "ema_multi_"):
        monkeypatch.setattr(T, name, lambda *a, _n=name, **kw: calls.append((_n, a, kw)))
    ps = [torch.nn.Parameter(torch.randn(n)) for n in (8, 5000, 12)]
    idle = torch.nn.Parameter(torch.randn(6))                            # trainable, but without a gradient in these steps
    opt = (train.AdamW8bit if bits == 8 else train.AdamW)(ps + [idle], lr=2e-4)
    ema = train.EMA(ps[:2] + [idle], decay=0.9)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.step(ema=ema)                                                    # counter 1: decay 0, 1 - decay = 1
    fused = ["adamw8_ema_multi_", "adamw_ema_multi_"] if bits == 8 else ["adamw_ema_multi_"]
    assert [n for n, _, _ in calls] == fused + ["ema_multi_"] and ema.optimization_step == 1
    for n, a, kw in calls[:-1]:
        assert kw["one_minus_decay"] == 1.0 and kw["step"] == 1 and "device_operands" not in kw
        assert len(a[-1]) == len(a[0])
        for t, e in zip(a[0], a[-1]):                                    # the last list: the shadow of that row's parameter
            assert e is ema.shadow_of(next(q for q in ps if q.data_ptr() == t.data_ptr()))
    assert [e is None for e in calls[-2][1][-1]] == ([False, True] if bits == 8 else [False, False, True])  # ps[2] has no shadow
    n, a, kw = calls[-1]
    assert a[0][0] is ema.shadow_of(idle) and a[1][0].data_ptr() == idle.data_ptr() and kw == {"one_minus_decay": 1.0}
    calls.clear()
    opt.step(ema=ema)                                                    # counter 2: decay (1 + 1) / (10 + 1)
    assert all(kw["one_minus_decay"] == 1.0 - 2 / 11 for _, _, kw in calls) and ema.optimization_step == 2
    calls.clear()
    hyper, cond = torch.zeros(4), torch.zeros(4)
    opt.step(device_operands=(hyper, cond), ema=ema)
    assert [n for n, _, _ in calls] == fused + ["ema_multi_"] and ema.optimization_step == 3
    assert all(kw["device_operands"][0] is hyper and kw["device_operands"][1] is cond for _, _, kw in calls)
    opt.undo_step()
    assert ema.optimization_step == 3                                    # a skipped step still counts
    calls.clear()
    opt.step()                                                           # ema=None: today's calls, today's keywords
    assert [n for n, _, _ in calls] == (["adamw8_multi_", "adamw_multi_"] if bits == 8 else ["adamw_multi_"])
    assert all("one_minus_decay" not in kw and "device_operands" not in kw for _, _, kw in calls) and ema.optimization_step == 3
    # a batch none of whose tensors has a shadow takes the plain entry, without the extra list
    calls.clear()
    lone = train.EMA([idle], decay=0.9)
    lone.advance()
    opt.step(ema=lone)
    plain = [c for c in calls if c[0] in ("adamw_multi_", "adamw8_multi_")]
    assert len(plain) == len(fused) and all(len(a) == (7 if n == "adamw8_multi_" else 5) for n, a, _ in plain)
    assert calls[-1][0] == "ema_multi_"
    ema.swapped = True
    with pytest.raises(RuntimeError, match="exchanged"):
        opt.step(ema=ema)


# ------------------------------------------------------------------------------- trainer contract
def test_ema_argument_defaults_to_none():
    from opendwm_amd.pipeline import CTSDTrainer
    assert inspect.signature(CTSDTrainer.__init__).parameters["ema"].default is None
    absent, off = CTSDTrainer(torch.nn.Linear(4, 4)), CTSDTrainer(torch.nn.Linear(4, 4), ema=None)
    scalars = lambda tr: {k: v for k, v in vars(tr).items() if isinstance(v, (bool, int, float, str, type(None)))}
    assert scalars(absent) == scalars(off) and absent.ema is None and off.ema is None
    with pytest.raises(RuntimeError, match="without ema="):
        with off.ema_weights():
            pass
    with pytest.raises(TypeError):
        CTSDTrainer(torch.nn.Linear(4, 4), ema=0.999)


def test_trainer_builds_the_ema_over_what_it_optimizes():
    from opendwm_amd import train
    from opendwm_amd.pipeline import CTSDTrainer
    model = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
    tr = CTSDTrainer(model, ema=dict(decay=0.99, use_ema_warmup=True), training_config={"freezing_pattern": "^1$"})
    assert isinstance(tr.ema, train.EMA) and tr.ema.decay == 0.99 and tr.ema.use_ema_warmup and tr.ema.optimization_step == 0
    assert [n for n, _ in tr.ema.named_shadows()] == ["0.weight", "0.bias"]           # the frozen module has no shadows
    assert tr.ema.shadow_of(model[1].weight) is None
    given = train.EMA(list(model.named_parameters()))
    assert CTSDTrainer(model, ema=given).ema is given


def test_train_step_inside_ema_weights_raises(monkeypatch):
    from opendwm_amd import train_ops as T
    from opendwm_amd.pipeline import CTSDTrainer
    swaps = []
    monkeypatch.setattr(T, "ema_swap_multi_", lambda ps, emas, shadows: swaps.append(len(ps)))
    tr = CTSDTrainer(torch.nn.Linear(4, 4), ema={})
    with pytest.raises(KeyError):                                        # an exception inside the context still swaps back
        with tr.ema_weights() as model:
            assert model is tr.model and tr.ema.swapped and swaps == [2]
            with pytest.raises(RuntimeError, match="ema_weights"):
                tr.train_step(torch.zeros(1), {})
            with pytest.raises(RuntimeError, match="already inside"):
                with tr.ema_weights():
                    pass
            raise KeyError("x")
    assert not tr.ema.swapped and swaps == [2, 2]


def test_checkpoint_carries_the_ema_and_its_absence_resets(tmp_path):
    from opendwm_amd.pipeline import CTSDTrainer
    torch.manual_seed(0)
    tr = CTSDTrainer(torch.nn.Linear(4, 3), ema=dict(decay=0.9))
    for _ in range(3):
        tr.ema.advance()
    for _, e in tr.ema.named_shadows():
        e.add_(0.25)
    tr.save_checkpoint(str(tmp_path / "with"), 3)
    assert os.path.exists(tmp_path / "with" / "ema" / "3.pth")
    fresh = CTSDTrainer(torch.nn.Linear(4, 3), ema=dict(decay=0.5))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                                   # the file is there: no warning
        fresh.load_checkpoint(str(tmp_path / "with"), 3)
    assert fresh.ema.optimization_step == 3 and fresh.ema.decay == 0.9 and fresh.global_step == 3
    for (n, e), (n2, e2) in zip(tr.ema.named_shadows(), fresh.ema.named_shadows()):
        assert n == n2 and torch.equal(e, e2)
        assert torch.equal(e2 - 0.25, dict(fresh.model.named_parameters())[n].detach())
    # a run that had no EMA: its checkpoint has no ema/ file
    CTSDTrainer(tr.model).save_checkpoint(str(tmp_path / "without"), 5)
    assert not os.path.exists(tmp_path / "without" / "ema")
    fresh.ema.advance()
    with pytest.warns(UserWarning, match="restart from the loaded parameters") as rec:
        fresh.load_checkpoint(str(tmp_path / "without"), 5)
    assert len([w for w in rec if "ema" in str(w.message)]) == 1
    assert fresh.ema.optimization_step == 0
    for n, e in fresh.ema.named_shadows():
        assert torch.equal(e, dict(fresh.model.named_parameters())[n].detach())
