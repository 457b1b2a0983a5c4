"""GPU leg (`-m gpu`) of CTSDTrainer(graph=True): forward, loss, loss scaling and backward replayed as one HIP graph, the
optimizer step queued without a host read.

With deterministic=True a train step is a function of its inputs and the library build, so the graph trainer is held to
the eager trainer BIT FOR BIT: one eager and one graph trainer start from the same state dict on their own models, and after every
step the loss, every parameter, every optimizer state tensor and every step count are torch.equal.  A stale packed operand, a missed
refresh of a compute copy, a wrong coefficient or flag, or a replay that reads memory somebody else rewrote shows as a difference at
these launch-bound sizes.  Shapes: the small MMDiT configuration of the trainer tests (2 samples x 3 frames x 3 views of 8 x 12 latents,
text length 10) and its layout-adapter variant, and the small SD 2.1 UNet at latents (2, 2, 3, 4, 8, 16), text length 10."""
import collections
import types

import pytest
import torch

from tests.common import rel_err, small_config, small_inputs, to_dev
from tests.test_deterministic_train_gpu import _census, _make_trainer, _unet_case
from tests.test_keep_activations_gpu import _trainer_inputs
from tests.test_train_gpu import _log

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16 = torch.bfloat16
STEPS = 4
KINDS = ("mmdit", "unet")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _fresh_param_store():
    from opendwm_amd.blocks import STORE
    STORE.bump()
    yield


_CASES = {}


def _mmdit_case(layout=False):
    """cfg / sd / inp of tests/test_keep_activations_gpu._Case("rowwise") without its oracle gradients; layout: with the ImageAdapter"""
    from oracle import ctsd_oracle as O
    over = {}
    if layout:
        over["condition_image_adapter_config"] = dict(in_channels=6, channels=[128, 128, 128], is_downblocks=[True, False, False],
                                                      num_res_blocks=2, downscale_factor=8, use_zero_convs=True)
    cfg = small_config(temporal_attention_type="rowwise", **over)
    sd = {k: v.to(bf16).float() for k, v in O.make_state_dict(cfg, 0).items()}
    inp = small_inputs(cfg, 0)
    if layout:
        inp["condition_image_tensor"] = torch.rand(2, 3, 3, 6, 64, 96, generator=torch.Generator().manual_seed(5))
    inp = {k: (v.to(bf16).float() if v.is_floating_point() and k not in ("timestep", "added_time_ids") else v) for k, v in inp.items()}
    return types.SimpleNamespace(cfg=cfg, sd=sd, inp=inp)


def _case(kind, dev):
    """(trainer kind, case, (latents, conditions, timestep indices, noise)), built once per module"""
    if kind not in _CASES:
        if kind == "unet":
            case = _unet_case(dev)
            _CASES[kind] = ("unet", case, case[2:])
        else:
            case = _mmdit_case(layout=kind == "mmdit_layout")
            _CASES[kind] = ("mmdit", case, _trainer_inputs(case, dev))
    return _CASES[kind]


def _snapshot(m, tr, loss, sync=False):
    """loss, parameters and optimizer state tensors.  Graph mode reads the flag of a step one step late, so the host-side step
    counts are left out unless sync: then the trainer catches up first (graph_sync) and the counts are compared too"""
    if sync:
        tr.graph_sync()
    out = {"loss": loss.detach().clone()}
    for n, p in m.named_parameters():
        out["p." + n] = p.detach().clone()
    for i, st in tr.optimizer.state_dict()["state"].items():
        for k, v in st.items():
            if sync or k != "step":
                out[f"s.{i}.{k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    return out


def _different(a, b):
    if set(a) != set(b):
        return sorted(set(a) ^ set(b))[:8]
    return [k for k in a if a[k].dtype != b[k].dtype or not torch.equal(a[k].cpu(), b[k].cpu())][:8]


_TRAINERS = []           # the trainer of the `_run` in progress is the last one (for `between` hooks)
_PLAIN = {}


def _plain_runs(kind, dev):
    """the 4-step runs of the eager and the graph trainer with nothing but deterministic=True, shared by the tests that read them"""
    if kind not in _PLAIN:
        _PLAIN[kind] = (_run(kind, dev, False, deterministic=True), _run(kind, dev, True, deterministic=True))
    return _PLAIN[kind]


def _run(kind, dev, graph, steps=STEPS, noises=None, between=None, **kw):
    """snapshots after every step of a fresh trainer, the last one after graph_sync() and with the step counts; noises: per-step
    noise (default: the case's), between(k, model): called after step k (1-based)"""
    tkind, case, (lat, cond, idx, noise) = _case(kind, dev)
    m, tr = _make_trainer(tkind, dev, case, graph=graph, **kw)
    _TRAINERS[:] = [tr]
    tr.initial = {n: p.detach().clone() for n, p in m.named_parameters()}
    snaps = []
    for k in range(steps):
        loss = tr.train_step(lat, cond, timestep_indices=idx, noise=noise if noises is None else noises[k])
        snaps.append(_snapshot(m, tr, loss, sync=k == steps - 1))
        if between is not None:
            between(k + 1, m)
    torch.cuda.synchronize()
    return m, tr, snaps


def _assert_bit_equal(name, eager, graph, first=0):
    for k, (a, b) in enumerate(zip(eager, graph)):
        if k >= first:
            bad = _different(a, b)
            assert not bad, (name, "step", k + 1, bad)
    assert any(not torch.equal(eager[-1][n], eager[0][n]) for n in eager[0] if n.startswith("p."))     # the steps did step


_NORMS = {}


def _first_step_norm(kind, dev):
    """the gradient norm of the first step, as the fused route reads it (no clip is active at this max_norm)"""
    if kind not in _NORMS:
        _, tr, _ = _run(kind, dev, False, steps=1, deterministic=True, grad_conditioning="fused", max_grad_norm=1e30)
        _NORMS[kind] = tr.last_grad_norm
        assert 0.0 < _NORMS[kind] < float("inf")
    return _NORMS[kind]


def _variant(name, kind, dev):
    if name == "plain":
        return {}
    if name == "8bit_clip":
        return dict(optimizer_bits=8, grad_conditioning="fused", max_grad_norm=0.5 * _first_step_norm(kind, dev))
    if name == "accumulate2":
        return dict(training_config={"gradient_accumulation_steps": 2})
    if name == "lr_scheduler":
        return dict(lr_scheduler=lambda opt: torch.optim.lr_scheduler.LambdaLR(opt, lambda s: 1.0 / (1.0 + s)))
    if name == "keep":
        return dict(activations="keep")
    if name == "freeze":
        return dict(training_config={"freezing_pattern": "mid_block" if kind == "unet" else "temporal_transformer_blocks"})
    raise KeyError(name)


VARIANTS = [(k, v) for k in ("mmdit", "mmdit_layout", "unet") for v in ("plain", "8bit_clip", "accumulate2", "lr_scheduler", "keep", "freeze")
            if not (v == "keep" and k != "mmdit") and not (k == "mmdit_layout" and v != "plain")]


@pytest.mark.parametrize("kind,variant", VARIANTS, ids=[f"{k}-{v}" for k, v in VARIANTS])
def test_graph_steps_equal_eager_steps_bitwise(dev, kind, variant):
    kw = dict(deterministic=True, **_variant(variant, kind, dev))
    if variant == "plain":
        (me, te, eager), (mg, tg, graph) = _plain_runs(kind, dev)
    else:
        norms = []                                             # the eager trainer's gradient norm of every step (it does not lag)
        me, te, eager = _run(kind, dev, False, between=lambda k, m: norms.append(_TRAINERS[-1].last_grad_norm), **kw)
        mg, tg, graph = _run(kind, dev, True, **kw)
    _log("train_graph_bitwise", kind=kind, variant=variant, captures=tg.graph_captures, replays=tg.graph_replays,
         capture_seconds=getattr(tg, "graph_capture_seconds", None), losses=[s["loss"].item() for s in graph])
    _assert_bit_equal(f"{kind}-{variant}", eager, graph)
    assert tg.graph_captures == 1 and tg.graph_replays == STEPS - tg.graph_warmup and tg.graph_warmup >= 1
    assert te.graph_captures == 0 and te.graph_replays == 0
    assert tg.skipped_steps == 0 and te.skipped_steps == 0
    if variant == "8bit_clip":
        assert tg.last_grad_norm == te.last_grad_norm == norms[-1]
        assert norms[1] > tg.max_grad_norm and norms[2] > tg.max_grad_norm       # the coefficient of replayed steps was not 1
        assert any(k.endswith("exp_avg_absmax") for k in graph[-1])
    if variant == "accumulate2":                               # steps 1 and 3 are micro-steps: nothing but the gradients moves
        assert all(torch.equal(graph[0]["p." + n], v) for n, v in tg.initial.items())
        assert tg.optimizer.t == STEPS // 2 == te.optimizer.t
    if variant == "lr_scheduler":
        assert tg.optimizer.lr == te.optimizer.lr == 2e-4 / (1.0 + STEPS)
    if variant == "freeze":
        pat = "mid_block" if kind == "unet" else "temporal_transformer_blocks"
        for m, tr in ((me, te), (mg, tg)):
            frozen = [(n, p) for n, p in m.named_parameters() if n.startswith(pat)]
            assert frozen and tr.frozen_modules
            for n, p in frozen:
                assert not p.requires_grad and p not in tr.optimizer.state, n
                assert torch.equal(p.detach(), tr.initial[n]), n


@pytest.mark.parametrize("kind", KINDS)
def test_untouched_parameters_get_no_state(dev, kind):
    """parameters without a gradient in the captured backward have no optimizer state in either trainer and keep their bits (weight
    decay included): the same set, whatever it is for the configuration"""
    (me, te, eager), (mg, tg, graph) = _plain_runs(kind, dev)
    stated = lambda m, tr: {n for n, p in m.named_parameters() if p in tr.optimizer.state}
    assert stated(me, te) == stated(mg, tg) and len(stated(mg, tg)) > 0
    for n, p in mg.named_parameters():
        if n not in stated(mg, tg):
            assert torch.equal(p.detach(), tg.initial[n]), n


@pytest.mark.parametrize("kind", KINDS)
def test_non_finite_step_is_skipped(dev, kind):
    """an inf in the noise of step 2 under enable_grad_scaler + fused: step 2 changes no parameter and no moment, counts as skipped and
    halves the scale; steps 3 - 4 are the eager trainer's bit for bit"""
    _, _, (lat, cond, idx, noise) = _case(kind, dev)
    bad = noise.clone()
    bad[0, 0, 0, 0, 0, 0] = float("inf")
    noises = [noise, bad, noise, noise]
    kw = dict(deterministic=True, grad_conditioning="fused", training_config={"enable_grad_scaler": True})
    _, te, eager = _run(kind, dev, False, noises=noises, **kw)
    _, tg, graph = _run(kind, dev, True, noises=noises, **kw)
    for name, tr, snaps in (("eager", te, eager), ("graph", tg, graph)):
        rest = lambda s: {k: v for k, v in s.items() if k != "loss" and not k.endswith(".step")}
        assert not _different(rest(snaps[0]), rest(snaps[1])), name                 # step 2 changed no parameter and no moment
        assert _different(rest(snaps[1]), rest(snaps[2])), name                     # step 3 did
        assert tr.skipped_steps == 1 and tr.grad_scaler.get_scale() == 32768.0 and tr.optimizer.t == STEPS - 1, name
    _log("train_graph_non_finite", kind=kind, losses=[s["loss"].item() for s in graph], last_grad_norm=tg.last_grad_norm)
    _assert_bit_equal(f"{kind}-non_finite", eager, graph, first=2)                  # steps 3 - 4, the step counts of step 4 included
    for k in (0, 1):                                                                # steps 1 - 2 as well, the nan loss of step 2 aside
        drop = lambda s: {n: v for n, v in s.items() if n != "loss"}
        assert not _different(drop(eager[k]), drop(graph[k])), k
    assert torch.equal(eager[0]["loss"], graph[0]["loss"]) and not bool(torch.isfinite(graph[1]["loss"]))
    assert tg.last_grad_norm == te.last_grad_norm


@pytest.mark.parametrize("kind", KINDS)
def test_foreign_forward_between_steps(dev, kind):
    """an eval() forward of the same model at another frame count between steps 2 and 3 (a preview): steps 3 - 4 still equal an eager
    trainer that did the same.  The graph is not captured again: a replay reads nothing a foreign forward can replace."""
    tkind, case, (lat, cond, idx, noise) = _case(kind, dev)
    if tkind == "unet":
        from oracle import unet_oracle as U
        inp = U.make_unet_inputs(case[0], 2, 1, 3, 8, 16, text_len=10)
        x, ts = inp.pop("sample"), inp.pop("timesteps")
    else:
        inp = small_inputs(case.cfg, 0, T=1)
        x, ts = inp.pop("sample"), inp.pop("timestep")
    pcond = to_dev(inp, dev, bf16)
    if "added_time_ids" in inp:
        pcond["added_time_ids"] = inp["added_time_ids"].to(dev)
    previews = {}

    def preview(which):
        def between(k, m):
            if k == 2:
                m.eval()
                with torch.no_grad():
                    previews[which] = m(x.to(dev).to(bf16), ts.to(dev), **pcond)[0][0].float().clone()
                m.train()
        return between
    _, te, eager = _run(kind, dev, False, between=preview("eager"), deterministic=True)
    _, tg, graph = _run(kind, dev, True, between=preview("graph"), deterministic=True)
    assert torch.equal(previews["eager"], previews["graph"]) and bool(torch.isfinite(previews["graph"]).all())
    _assert_bit_equal(f"{kind}-foreign_forward", eager, graph)
    assert tg.graph_captures == 1 and tg.graph_replays == STEPS - tg.graph_warmup


def test_second_trainer_and_changed_inputs(dev):
    """a second (eager) trainer stepping the same model between two graph steps, then inputs of another shape: the graph trainer
    follows the parameters the other trainer wrote - its replay reads the live compute copies - and captures again for the new shape"""
    tkind, case, (lat, cond, idx, noise) = _case("mmdit", dev)

    def run(graph):
        m, tr = _make_trainer(tkind, dev, case, graph=graph, deterministic=True)
        from opendwm_amd.pipeline import CTSDTrainer
        other = CTSDTrainer(m, lr=1e-3, weight_decay=0.0, deterministic=True)
        out = []
        for k in range(3):
            out.append(_snapshot(m, tr, tr.train_step(lat, cond, timestep_indices=idx, noise=noise)))
            if k == 1:
                other.train_step(lat, cond, timestep_indices=idx, noise=noise)
        small = {k: (v[:1] if torch.is_tensor(v) else v) for k, v in cond.items()}
        out.append(_snapshot(m, tr, tr.train_step(lat[:1], small, timestep_indices=idx[:1], noise=noise[:1]), sync=True))
        torch.cuda.synchronize()
        return tr, out
    te, eager = run(False)
    tg, graph = run(True)
    _assert_bit_equal("mmdit-second_trainer", eager, graph)
    assert tg.graph_captures == 2 and tg.graph_replays == 3


@pytest.mark.parametrize("kind", KINDS)
def test_launch_census_without_graph(dev, kind):
    """graph=False launches exactly the symbols of a trainer built without the argument, none of them *_dev; graph=True queues the
    *_dev optimizer launches and no by-value ones once it replays"""
    tkind, case, (lat, cond, idx, noise) = _case(kind, dev)
    seen = {}
    for name, kw in (("absent", {}), ("off", dict(graph=False)), ("on", dict(graph=True))):
        m, tr = _make_trainer(tkind, dev, case, **kw)
        counts = []
        for _ in range(2):
            with _census() as names:
                tr.train_step(lat, cond, timestep_indices=idx, noise=noise)
            counts.append(collections.Counter(names))
        torch.cuda.synchronize()
        seen[name] = counts
        del tr, m
    assert seen["off"] == seen["absent"]
    assert not any(n.endswith("_dev") for c in seen["off"] for n in c)
    assert seen["on"][0] == seen["off"][0]                                  # the warm-up step is the eager step
    replay = seen["on"][1]                                                   # capture + replay: the capture's launches are counted once
    assert replay["dwm_adamw_multi_dev"] == seen["off"][1]["dwm_adamw_multi"] >= 1 and replay["dwm_adamw_multi"] == 0
    other = lambda c: {n: k for n, k in c.items() if not n.startswith("dwm_adamw")}
    assert other(replay) == other(seen["off"][1])                            # the captured region holds the eager step's launches


@pytest.mark.parametrize("kind", KINDS)
def test_default_mode_graph_against_eager(dev, kind):
    """deterministic=False: the fp32 atomics finish some sums in any order, so graph against eager per parameter after 2 steps is held
    to a relative Frobenius difference of 1e-5 - two orders above the 5e-8 - 1e-7 spread DESIGN §19 records for those atomics"""
    me, _, _ = _run(kind, dev, False, steps=2)
    mg, tg, _ = _run(kind, dev, True, steps=2)
    worst, name = 0.0, None
    pe = dict(me.named_parameters())
    for n, p in mg.named_parameters():
        e = rel_err(p.detach(), pe[n].detach())
        if e > worst:
            worst, name = e, n
    _log("train_graph_default_mode", kind=kind, worst_rel=worst, parameter=name)
    print("train_graph_default_mode", kind, worst, name)
    assert tg.graph_replays == 1 and worst <= 1e-5, (worst, name)
