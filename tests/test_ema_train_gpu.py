"""GPU leg (`-m gpu`) of CTSDTrainer(ema=...) and train.EMA on the smallest MMDiT and SD 2.1 UNet of the trainer tests
(their builders are restated here): 2 samples x 3 frames x 3 views of 8 x 12 latents, text length 10, and latents (2, 2, 3, 4, 8, 16).

With deterministic=True a train step is a function of its inputs and the library build, so "the EMA changes nothing else"
and "the graph trainer averages what the eager one averages" are held BIT FOR BIT over 4 steps.  The shadows themselves are held to the
fp64 recurrence e_k = e_(k-1) + (1 - decay_k) * (p_k - e_(k-1)), seeded every step with the previous shadow as read from the device and
with diffusers' decay of that step restated here, within 2^-21 * max(|e_(k-1)|, |p_k|): five fp32 roundings of at most 2^-24 * max
each, rounded up to a power of two (the bound of tests/test_ema_kernels_gpu.py)."""
import types

import pytest
import torch

from tests.common import small_config, small_inputs, to_dev

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16 = torch.bfloat16
STEPS = 4
DECAY = 0.99
BOUND = 2.0 ** -21


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


# ------------------------------------------------------------------------------- the builders of the trainer tests, restated
_CASES = {}


def _case(kind, dev):
    """(model factory, (latents, conditions, timestep indices, noise)), built once per module"""
    if kind in _CASES:
        return _CASES[kind]
    noise_of = lambda lat: torch.randn(lat.shape, generator=torch.Generator().manual_seed(5))
    if kind == "unet":
        from oracle import unet_oracle as U
        from opendwm_amd.unet import UNetCrossviewTemporalConditionModel
        cfg = U.make_unet_config(block_out_channels=(128, 256, 512, 512), num_attention_heads=(2, 4, 8, 8), cross_attention_dim=128,
                                 projection_class_embeddings_input_dim=11 * 256)
        sd = {k: v.to(bf16).float() for k, v in U.make_unet_state_dict(cfg, 0).items()}
        inp = U.make_unet_inputs(cfg, 2, 2, 3, 8, 16, text_len=10)
        cond = to_dev({k: v for k, v in inp.items() if k not in ("sample", "timesteps")}, dev)
        lat = torch.randn(2, 2, 3, 4, 8, 16, generator=torch.Generator().manual_seed(3)).to(dev)

        def make(state=None):
            m = UNetCrossviewTemporalConditionModel(**cfg)
            m.load_state_dict(sd if state is None else state, strict=True)
            return m.to(dev).train()
    else:
        from oracle import ctsd_oracle as O
        from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
        cfg = small_config(temporal_attention_type="rowwise")
        sd = {k: v.to(bf16).float() for k, v in O.make_state_dict(cfg, 0).items()}
        inp = small_inputs(cfg, 0)
        inp = {k: (v.to(bf16).float() if v.is_floating_point() and k not in ("timestep", "added_time_ids") else v) for k, v in inp.items()}
        lat = inp.pop("sample").to(dev)
        inp.pop("timestep")
        cond = to_dev(inp, dev)

        def make(state=None):
            m = DiTCrossviewTemporalConditionModel(**cfg)
            m.load_state_dict(sd if state is None else state)
            return m.to(dev).train()
    _CASES[kind] = (make, (lat, cond, torch.tensor([250, 800]), noise_of(lat)))
    return _CASES[kind]


def _make_trainer(kind, dev, state=None, **kw):
    from opendwm_amd.blocks import STORE
    from opendwm_amd.pipeline import CTSDTrainer
    STORE.bump()
    m = _case(kind, dev)[0](state)
    return m, CTSDTrainer(m, lr=2e-4, weight_decay=0.01, deterministic=True, **kw)


def _snapshot(m, tr, loss, sync=False):
    """loss, parameters and optimizer state tensors (graph mode reads the flag of a step one step late: the host-side step counts
    are compared after graph_sync only); the shadows go beside it under "e." keys"""
    if sync:
        tr.graph_sync()
    out = {"loss": loss.detach().clone()}
    for n, p in m.named_parameters():
        out["p." + n] = p.detach().clone()
    if tr.lora is not None:
        for n, p in tr.lora.state_dict().items():
            out["p." + n] = p.detach().clone()
    for i, st in tr.optimizer.state_dict()["state"].items():
        for k, v in st.items():
            if sync or k != "step":
                out[f"s.{i}.{k}"] = v.detach().clone() if torch.is_tensor(v) else torch.tensor(v)
    if tr.ema is not None:
        for n, e in tr.ema.named_shadows():
            out["e." + n] = e.detach().clone()
    return out


def _different(a, b, prefixes=("loss", "p.", "s.")):
    ka, kb = ({k for k in d if k.startswith(prefixes)} for d in (a, b))
    if ka != kb:
        return sorted(ka ^ kb)[:8]
    return [k for k in sorted(ka) if a[k].dtype != b[k].dtype or not torch.equal(a[k].cpu(), b[k].cpu())][:8]


_RUNS = {}


def _run(kind, dev, key=None, steps=STEPS, first=0, trainer=None, **kw):
    """(model, trainer, snapshot after every step) of a fresh (or the given) trainer; key: the run is kept for other tests"""
    if key is not None and (kind, key) in _RUNS:
        return _RUNS[(kind, key)]
    lat, cond, idx, noise = _case(kind, dev)[1]
    m, tr = _make_trainer(kind, dev, **kw) if trainer is None else trainer
    snaps = []
    for k in range(first, steps):
        loss = tr.train_step(lat, cond, timestep_indices=idx, noise=noise)
        snaps.append(_snapshot(m, tr, loss, sync=k == steps - 1))
    torch.cuda.synchronize()
    if key is not None:
        _RUNS[(kind, key)] = (m, tr, snaps)
    return m, tr, snaps


def _diffusers_decay(optimization_step, decay=DECAY, min_decay=0.0, update_after_step=0, use_ema_warmup=False, inv_gamma=1.0, power=2 / 3):
    """diffusers 0.31 EMAModel.get_decay, restated"""
    step = max(0, optimization_step - update_after_step - 1)
    if step <= 0:
        return 0.0
    cur = 1 - (1 + step / inv_gamma) ** -power if use_ema_warmup else (1 + step) / (10 + step)
    return max(min(cur, decay), min_decay)


def _check_recurrence(prev, now, n_step, what):
    """every "e." entry of `now` against the fp64 recurrence from the shadows of `prev` and the parameters of `now`"""
    omd = 1.0 - _diffusers_decay(n_step)
    names = [k[2:] for k in now if k.startswith("e.")]
    assert names, what
    for n in names:
        e0, p1, e1 = prev["e." + n].double(), now["p." + n].double(), now["e." + n].double()
        err = (e1 - (e0 + omd * (p1 - e0))).abs()
        lim = BOUND * torch.maximum(e0.abs(), p1.abs())
        assert bool((err <= lim).all()), (what, n_step, n, float(err.max()), float((err - lim).max()))
    return names


# ------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("kind,bits", [("mmdit", 32), ("mmdit", 8), ("unet", 32)])
def test_ema_does_not_disturb_training_and_follows_the_recurrence(dev, kind, bits):
    _, _, plain = _run(kind, dev, key=("plain", bits), optimizer_bits=bits)
    m, tr, averaged = _run(kind, dev, key=("ema", bits), optimizer_bits=bits, ema=dict(decay=DECAY))
    for k, (a, b) in enumerate(zip(plain, averaged)):
        bad = _different(a, b)
        assert not bad, (kind, bits, "step", k + 1, bad)
    assert any(not torch.equal(plain[-1][n], plain[0][n]) for n in plain[0] if n.startswith("p."))     # the steps did step
    assert tr.ema.optimization_step == STEPS and not tr.ema.swapped
    # one shadow per trainable parameter, under the checkpoint's keys
    assert [n for n, _ in tr.ema.named_shadows()] == [n for n, p in m.named_parameters() if p.requires_grad]
    # step 1 has decay 0: the shadows ARE the parameters it wrote; later steps follow the recurrence from the shadow read back
    first = averaged[0]
    assert all(torch.equal(first["e." + n], first["p." + n]) for n, _ in tr.ema.named_shadows())
    for k in range(1, STEPS):
        names = _check_recurrence(averaged[k - 1], averaged[k], k + 1, (kind, bits))
        moved = [n for n in names if not torch.equal(averaged[k]["e." + n], averaged[k - 1]["e." + n])]
        lagging = [n for n in names if not torch.equal(averaged[k]["e." + n], averaged[k]["p." + n])]
        assert len(moved) > len(names) // 2 and len(lagging) > len(names) // 2, (k, len(moved), len(lagging), len(names))


def test_shadows_move_on_optimizing_calls_only(dev):
    m, tr, snaps = _run("mmdit", dev, ema=dict(decay=DECAY), training_config={"gradient_accumulation_steps": 2})
    names = [n for n, _ in tr.ema.named_shadows()]
    start = _case("mmdit", dev)[0]().state_dict()
    assert all(torch.equal(snaps[0]["e." + n], start[n].to(dev)) for n in names)                      # call 1: nothing moved
    assert any(not torch.equal(snaps[1]["e." + n], snaps[0]["e." + n]) for n in names)                # call 2: the optimizer stepped
    assert all(torch.equal(snaps[2]["e." + n], snaps[1]["e." + n]) for n in names)                    # call 3
    assert any(not torch.equal(snaps[3]["e." + n], snaps[2]["e." + n]) for n in names)                # call 4
    assert tr.ema.optimization_step == 2
    assert all(torch.equal(snaps[1]["e." + n], snaps[1]["p." + n]) for n in names)                    # the first optimizing call: decay 0
    _check_recurrence(snaps[2], snaps[3], 2, "accumulate")


def _clip(dev):
    """half the gradient norm of the first step: a clip that is active"""
    if "clip" not in _RUNS:
        _, tr, _ = _run("mmdit", dev, steps=1, grad_conditioning="fused", max_grad_norm=1e30)
        assert 0.0 < tr.last_grad_norm < float("inf")
        _RUNS["clip"] = 0.5 * tr.last_grad_norm
    return _RUNS["clip"]


def _graph_runs(dev):
    kw = dict(grad_conditioning="fused", max_grad_norm=_clip(dev), ema=dict(decay=DECAY))
    return _run("mmdit", dev, key="fused_eager", **kw), _run("mmdit", dev, key="fused_graph", graph=True, **kw)


def test_graph_mode_averages_what_the_eager_trainer_averages(dev):
    (_, tr_e, eager), (_, tr_g, graph) = _graph_runs(dev)
    assert tr_g.graph_captures == 1 and tr_g.graph_replays == STEPS - 1 and tr_e.graph_captures == 0
    for k, (a, b) in enumerate(zip(eager, graph)):
        bad = _different(a, b, prefixes=("loss", "p.", "s.", "e."))
        assert not bad, ("step", k + 1, bad)
    assert tr_g.ema.optimization_step == tr_e.ema.optimization_step == STEPS and tr_g.skipped_steps == 0
    assert any(not torch.equal(graph[-1][n], graph[-1]["p." + n[2:]]) for n in graph[-1] if n.startswith("e."))


def test_a_step_skipped_on_the_device_leaves_the_shadows_and_counts(dev):
    from opendwm_amd import train
    from opendwm_amd.blocks import STORE
    gen = torch.Generator().manual_seed(3)
    ps = [torch.nn.Parameter(torch.randn(n, generator=gen).to(dev)) for n in (12, 5000, 100003)]
    idle = torch.nn.Parameter(torch.randn(300, generator=gen).to(dev))              # a shadow without a gradient
    opt = train.AdamW8bit(ps + [idle], lr=2e-4, weight_decay=0.01)
    ema = train.EMA(ps + [idle], decay=0.9)

    def step(flag):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=gen).to(dev)
        [STORE.bf(p) for p in ps]
        opt.step(device_operands=(None, torch.tensor([1.0, 0.5, flag, 0.0], device=dev)), ema=ema)
        torch.cuda.synchronize()
    step(0.0)
    step(0.0)
    for _, e in ema.named_shadows():                                                   # make every shadow differ from its parameter
        e.add_(0.125)
    before = [t.detach().clone() for t in ps + [idle] + [e for _, e in ema.named_shadows()] + [STORE.bf(p) for p in ps]]
    step(1.0)
    after = [t.detach().clone() for t in ps + [idle] + [e for _, e in ema.named_shadows()] + [STORE.bf(p) for p in ps]]
    assert all(torch.equal(a.view(torch.uint8 if a.dtype == torch.uint8 else torch.int16 if a.dtype == bf16 else torch.int32),
                           b.view(torch.uint8 if b.dtype == torch.uint8 else torch.int16 if b.dtype == bf16 else torch.int32))
               for a, b in zip(before, after))
    assert ema.optimization_step == 3                                                  # the skipped call counts ...
    opt.undo_step()
    assert ema.optimization_step == 3 and opt.t == 2                                   # ... also after the optimizer took its own count back
    step(0.0)                                                                          # the same call with the flag clear does average
    assert ema.optimization_step == 4
    omd = 1.0 - _diffusers_decay(4, decay=0.9)
    for (p, e), e0 in zip(ema.pairs(), before[len(ps) + 1:]):
        assert not torch.equal(e, e0)
        want = e0.double() + omd * (p.detach().double() - e0.double())
        assert bool(((e.double() - want).abs() <= BOUND * torch.maximum(e0.double().abs(), p.detach().double().abs())).all())


def _forward(kind, dev, tr):
    """(the model's prediction, the loss) of the trainer's forward on the case's inputs, without a backward"""
    lat, cond, idx, noise = _case(kind, dev)[1]
    preds = []
    hook = tr.model.register_forward_hook(lambda mod, args, out: preds.append(out[0][0].detach().clone()))
    try:
        with torch.no_grad():
            loss = tr.loss(lat, cond, timestep_indices=idx, noise=noise)
    finally:
        hook.remove()
    torch.cuda.synchronize()
    assert len(preds) == 1
    return preds[0], loss.detach().clone()


def _compute_copies(m):
    from opendwm_amd.blocks import STORE
    return {n: STORE.shadow_of(p).clone() for n, p in m.named_parameters() if STORE.shadow_of(p) is not None}


def test_ema_weights_evaluates_the_average_and_gives_the_run_back(dev):
    """a graph trainer, three steps, an evaluation inside ema_weights(), the fourth step: the evaluation is the forward of a fresh
    model loaded from averaged_state_dict, and the fourth step is the fourth step of the run that never swapped"""
    from opendwm_amd.pipeline import CTSDTrainer
    _, (_, _, reference) = _graph_runs(dev)
    kw = dict(grad_conditioning="fused", max_grad_norm=_clip(dev), ema=dict(decay=DECAY), graph=True)
    m, tr, snaps = _run("mmdit", dev, steps=STEPS - 1, **kw)
    tr.graph_sync()
    assert not _different(snaps[-1], reference[STEPS - 2], prefixes=("loss", "p.", "e."))
    averaged = {k: v.detach().clone() for k, v in tr.ema.averaged_state_dict(m).items()}
    names = [n for n, _ in tr.ema.named_shadows()]
    assert all(torch.equal(averaged[n], snaps[-1]["e." + n]) for n in names) and set(averaged) == set(m.state_dict())
    params0, copies0, captures = {n: p.detach().clone() for n, p in m.named_parameters()}, _compute_copies(m), tr.graph_captures
    addresses = {n: p.data_ptr() for n, p in m.named_parameters()}
    assert len(copies0) > len(params0) // 2
    with tr.ema_weights() as model:
        assert model is m and tr.ema.swapped
        assert all(torch.equal(p.detach(), averaged[n]) for n, p in m.named_parameters())
        assert all(torch.equal(e, params0[n]) for n, e in tr.ema.named_shadows())                      # the trained weights wait there
        pred_in, loss_in = _forward("mmdit", dev, tr)
        with pytest.raises(RuntimeError, match="ema_weights"):
            tr.train_step(*_case("mmdit", dev)[1][:2])
    assert not tr.ema.swapped
    pred_raw, _ = _forward("mmdit", dev, tr)
    assert not torch.equal(pred_raw, pred_in)                                                          # the average is not the raw weights
    # everything is back, where it was
    assert all(torch.equal(p.detach(), params0[n]) and p.data_ptr() == addresses[n] for n, p in m.named_parameters())
    assert all(torch.equal(e, averaged[n]) for n, e in tr.ema.named_shadows())
    copies1 = _compute_copies(m)
    assert set(copies0) <= set(copies1) and all(torch.equal(copies1[n], copies0[n]) for n in copies0)
    assert tr.graph_captures == captures
    _, _, last = _run("mmdit", dev, first=STEPS - 1, trainer=(m, tr))
    assert tr.graph_captures == captures
    bad = _different(last[0], reference[-1], prefixes=("loss", "p.", "s.", "e."))
    assert not bad, bad
    # (last: loading a state dict drops every compute copy of the process, which would make the graph trainer capture again)
    fresh = _case("mmdit", dev)[0](averaged)
    pred_fresh, loss_fresh = _forward("mmdit", dev, CTSDTrainer(fresh, deterministic=True))
    assert torch.equal(pred_in, pred_fresh) and torch.equal(loss_in, loss_fresh)


def test_lora_shadows_are_the_adapters_and_the_context_merges_them(dev):
    from opendwm_amd import train_ops as T
    from opendwm_amd.blocks import STORE
    m, tr, snaps = _run("mmdit", dev, steps=3, ema=dict(decay=DECAY),
                        lora=dict(rank=4, alpha=8.0, generator=torch.Generator().manual_seed(11)))
    lora = tr.lora
    assert sorted(n for n, _ in tr.ema.named_shadows()) == sorted(lora.state_dict())         # (the optimizer's order: every A, then every B)
    assert all(tr.ema.shadow_of(p) is not None for p in lora.parameters()) and all(tr.ema.shadow_of(p) is None for p in m.parameters())
    _check_recurrence(snaps[1], snaps[2], 3, "lora")
    targets = lora.targets()
    before = [STORE.shadow_of(p).clone() for p in targets]
    a_avg = [tr.ema.shadow_of(a).clone() for a in lora.lora_A]
    b_avg = [tr.ema.shadow_of(b).clone() for b in lora.lora_B]
    want = [torch.empty_like(c) for c in before]
    T.lora_merge_multi([p.data for p in targets], a_avg, b_avg, want, [lora.scale] * len(targets))
    torch.cuda.synchronize()
    assert any(not torch.equal(w, c) for w, c in zip(want, before))
    with tr.ema_weights():
        assert lora.merged()
        assert all(torch.equal(a.detach(), s) for a, s in zip(lora.lora_A, a_avg)) and all(torch.equal(b.detach(), s) for b, s in zip(lora.lora_B, b_avg))
        assert all(torch.equal(STORE.shadow_of(p), w) for p, w in zip(targets, want))
    assert lora.merged() and not tr.ema.swapped
    assert all(torch.equal(STORE.shadow_of(p), c) for p, c in zip(targets, before))


def test_checkpoint_resumes_the_average(dev, tmp_path):
    import os
    _, _, whole = _run("mmdit", dev, key=("ema", 32), optimizer_bits=32, ema=dict(decay=DECAY))
    m, tr, _ = _run("mmdit", dev, steps=2, optimizer_bits=32, ema=dict(decay=DECAY))
    tr.save_checkpoint(str(tmp_path), 2)
    assert os.path.exists(tmp_path / "ema" / "2.pth")
    del m, tr
    m2, tr2 = _make_trainer("mmdit", dev, optimizer_bits=32, ema=dict(decay=0.5))
    tr2.load_checkpoint(str(tmp_path), 2)
    assert tr2.ema.optimization_step == 2 and tr2.ema.decay == DECAY and tr2.global_step == 2
    _, _, rest = _run("mmdit", dev, first=2, trainer=(m2, tr2))
    for k, (a, b) in enumerate(zip(whole[2:], rest)):
        bad = _different(a, b, prefixes=("loss", "p.", "e."))
        assert not bad, ("step", k + 3, bad)
