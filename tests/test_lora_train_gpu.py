"""GPU leg of low-rank fine-tuning (opendwm_amd/lora.py, CTSDTrainer(lora=...)) on the small full-graph configuration:
adapter gradients against fp32 autograd through the oracle with A and B as leaves, the zero-initialised adapter as the plain
trainer bit for bit, what a training step may and may not touch, staleness of the merged compute copies, checkpoints and folding."""
import pytest
import torch

from tests.common import rel_err, small_config, small_inputs, to_dev

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
RANK, ALPHA = 4, 8.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _setup(tt="rowwise"):
    """(cfg, state dict, inputs) with every floating tensor a bf16 value held in fp32, as tests/test_train_gpu.py prepares them"""
    from oracle import ctsd_oracle as O
    cfg = small_config(temporal_attention_type=tt)
    sd = {k: v.to(bf16).float() for k, v in O.make_state_dict(cfg, 0).items()}
    inp = small_inputs(cfg, 0)
    inp = {k: (v.to(bf16).float() if v.is_floating_point() and k not in ("timestep", "added_time_ids") else v) for k, v in inp.items()}
    return cfg, sd, inp


@pytest.fixture(scope="module")
def base():
    return _setup()


def _model(cfg, sd, dev):
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    m = DiTCrossviewTemporalConditionModel(**cfg)
    m.load_state_dict(sd)
    return m.to(dev).train()


def _adapters(m, seed=3, b_std=0.0):
    from opendwm_amd.lora import LoraAdapters
    la = LoraAdapters(m, rank=RANK, alpha=ALPHA, generator=torch.Generator().manual_seed(seed))
    if b_std:
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for b in la.lora_B:
                b.copy_(torch.randn(b.shape, generator=g) * b_std)
    return la


def _batch(inp, dev, seed=5):
    """(latents, conditions on the device, timestep indices, noise): one fixed batch"""
    inp = dict(inp)
    lat = inp.pop("sample")
    inp.pop("timestep")
    noise = torch.randn(lat.shape, generator=torch.Generator().manual_seed(seed))
    return lat.to(dev), to_dev(inp, dev), torch.tensor([250, 800]), noise


def _bits(t):
    return t.detach().contiguous().view(torch.int32 if t.dtype == f32 else torch.int16).cpu()


# --------------------------------------------------------------------------------------------------- gradients vs the oracle
@pytest.mark.parametrize("tt", ["rowwise", "pointwise"])
def test_adapter_gradients_vs_oracle(dev, tt):
    """forward_train after merge_() against the oracle on W + s B A formed in fp32, and A.grad / B.grad after project_grads_()
    against fp32 autograd through the oracle with A and B as leaves; thresholds of test_model_gradients_vs_oracle"""
    from oracle import ctsd_oracle as O
    from opendwm_amd import train
    cfg, sd, inp = _setup(tt)
    di = to_dev(inp, dev)
    wgt = torch.randn(inp["sample"].shape, generator=torch.Generator().manual_seed(11)).to(dev)
    m = _model(cfg, sd, dev)
    la = _adapters(m, b_std=0.05)
    adapted = {id(p) for p in la.targets()}
    for p in m.parameters():
        p.requires_grad_(id(p) in adapted)

    # the oracle: every targeted weight replaced by W + s B A, A and B leaves
    sdo = {k: v.to(dev) for k, v in sd.items()}
    leaves = []
    for name, a, b in zip(la.names, la.lora_A, la.lora_B):
        a0, b0 = a.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
        sdo[name] = sdo[name] + la.scale * (b0 @ a0)
        leaves.append((a0, b0))
    moved = max(rel_err(sdo[n].detach(), sd[n]) for n in la.names)
    assert moved > 0.05, moved                      # the adapters are no rounding error of the base weights
    ref = O.dit_forward(sdo, cfg, **di)
    (ref * wgt).sum().backward()

    la.merge_()
    assert la.merged()
    kw = dict(di)
    out = train.forward_train(m, kw.pop("sample"), kw.pop("timestep"), kw.pop("encoder_hidden_states"), kw.pop("pooled_projections"),
                              crossview_attention_mask=kw.get("crossview_attention_mask"), added_time_ids=kw.get("added_time_ids"))
    e_fwd = rel_err(out, ref.detach())
    (out.float() * wgt).sum().backward()
    assert all((p.grad is not None) == (id(p) in adapted) for p in m.parameters())
    la.project_grads_()
    assert all(p.grad is None for p in m.parameters())
    errs, num, den = {}, 0.0, 0.0
    for name, a, b, (a0, b0) in zip(la.names, la.lora_A, la.lora_B, leaves):
        for tag, got, want in (("A", a.grad, a0.grad), ("B", b.grad, b0.grad)):
            assert got is not None and want is not None, (name, tag)
            x, y = got.double().cpu(), want.double().cpu()
            errs[f"{name}:{tag}"] = ((x - y).norm() / y.norm().clamp_min(1e-30)).item()
            num += float((x - y).pow(2).sum())
            den += float(y.pow(2).sum())
    glob = (num / den) ** 0.5
    worst = sorted(errs.items(), key=lambda kv: -kv[1])[:5]
    print(f"lora gradients {tt}: fwd {e_fwd:.3e} global {glob:.3e} worst {worst}")
    assert e_fwd < 2e-2 and glob < 3e-2, (e_fwd, glob, worst)
    assert all(v < 0.15 for v in errs.values()), worst


# ------------------------------------------------------------------------------------------------------------ the trainer
def test_zero_initialised_adapters_give_the_plain_trainers_loss(dev, base):
    from opendwm_amd.pipeline import CTSDTrainer
    cfg, sd, inp = base
    lat, di, idx, noise = _batch(inp, dev)
    plain = CTSDTrainer(_model(cfg, sd, dev), lr=1e-3, weight_decay=0.0)
    l0 = plain.train_step(lat, di, timestep_indices=idx, noise=noise)
    tr = CTSDTrainer(_model(cfg, sd, dev), lr=1e-3, weight_decay=0.0, lora=dict(rank=RANK, alpha=ALPHA))
    l1 = tr.train_step(lat, di, timestep_indices=idx, noise=noise)
    assert torch.equal(_bits(l0.float()), _bits(l1.float())), (l0.item(), l1.item())
    assert tr.lora.merged()


@pytest.mark.parametrize("bits,accum", [(32, None), (8, None), (32, 2)], ids=["adamw", "adamw8", "accumulate2"])
def test_four_steps_touch_the_adapters_only(dev, base, bits, accum):
    from opendwm_amd.pipeline import CTSDTrainer
    cfg, sd, inp = base
    lat, di, idx, noise = _batch(inp, dev)
    m = _model(cfg, sd, dev)
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    tc = {} if accum is None else {"gradient_accumulation_steps": accum}
    tr = CTSDTrainer(m, lr=2e-3, weight_decay=0.0, optimizer_bits=bits, training_config=tc, max_grad_norm=1.0,
                     lora=dict(rank=RANK, alpha=ALPHA, generator=torch.Generator().manual_seed(3)))
    adapted = {id(p) for p in tr.lora.targets()}
    losses = []
    for i in range(4 * (accum or 1)):
        losses.append(tr.train_step(lat, di, timestep_indices=idx, noise=noise).item())
        optimized = accum is None or (i + 1) % accum == 0
        assert all(p.grad is None for p in m.parameters()), i                      # untargeted: never; targeted: projected and dropped
        assert all((p.grad is None) == optimized for p in tr.lora.parameters()), i  # held across the micro-steps of a cycle
        assert tr.lora.merged()
    print(f"lora four steps ({bits} bit, accumulate {accum}): losses {losses}")
    assert losses[-1] < losses[0], losses
    if accum:                                        # the micro-steps of a cycle see the same weights
        assert losses[0] == losses[1] and losses[2] != losses[1]
    for n, p in m.named_parameters():                # every base master, bit for bit
        assert torch.equal(_bits(p), _bits(before[n])), n
    lora_ids = {id(p) for p in tr.lora.parameters()}
    assert len(tr.optimizer.state) == len(lora_ids) and all(id(p) in lora_ids for p in tr.optimizer.state)
    # and the adapters did move (a projection whose output the model drops, the context query of the context-pre-only last block,
    # has a zero gradient and stays)
    still = [n for n, b in zip(tr.lora.names, tr.lora.lora_B) if float(b.detach().abs().max()) == 0]
    print("adapters that did not move:", still)
    assert 10 * len(still) < len(tr.lora.names), still
    assert tr.lora.held_bytes() == sum(p.numel() * 4 for p in tr.lora.parameters())
    if bits == 8:
        assert any(st["exp_avg"].dtype == torch.uint8 for st in tr.optimizer.state.values()) or \
            all(p.numel() < tr.optimizer.min_8bit_size for p in tr.lora.parameters())


def _twin(cfg, sd, dev, seed=3, **kw):
    from opendwm_amd.pipeline import CTSDTrainer
    return CTSDTrainer(_model(cfg, sd, dev), lr=2e-3, weight_decay=0.0, deterministic=True,
                       lora=dict(rank=RANK, alpha=ALPHA, generator=torch.Generator().manual_seed(seed)), **kw)


def test_dropped_compute_copies_are_noticed_and_merged_again(dev, base):
    from opendwm_amd.blocks import STORE
    cfg, sd, inp = base
    lat, di, idx, noise = _batch(inp, dev)
    calm = _twin(cfg, sd, dev)
    want = [calm.train_step(lat, di, timestep_indices=idx, noise=noise) for _ in range(3)]
    tr = _twin(cfg, sd, dev)
    got = [tr.train_step(lat, di, timestep_indices=idx, noise=noise)]
    assert tr.lora.merged()
    STORE.bump()                                     # what a state-dict load or .to() amounts to: every compute copy is dropped
    assert not tr.lora.merged()
    got.append(tr.train_step(lat, di, timestep_indices=idx, noise=noise))
    assert tr.lora.merged()
    w = tr.lora.targets()[0]
    w.data = w.data.clone()                          # the master moved (as .to() moves it): the copy no longer belongs to it
    assert not tr.lora.merged()
    got.append(tr.train_step(lat, di, timestep_indices=idx, noise=noise))
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(_bits(a.float()), _bits(b.float())), (i, a.item(), b.item())
    assert want[2].item() != want[0].item()          # the adapters matter to the loss: a step on the base model would show


def test_checkpoint_round_trip(dev, base, tmp_path):
    import os
    cfg, sd, inp = base
    lat, di, idx, noise = _batch(inp, dev)
    a = _twin(cfg, sd, dev)
    for _ in range(2):
        a.train_step(lat, di, timestep_indices=idx, noise=noise)
    a.save_checkpoint(str(tmp_path), 2)
    assert sorted(os.listdir(tmp_path)) == ["lora", "optimizer"]                  # the base checkpoint is not written again
    f = torch.load(os.path.join(tmp_path, "lora", "2.pth"), weights_only=True)
    assert f["rank"] == RANK and f["alpha"] == ALPHA and set(f["state"]) == set(a.lora.state_dict())
    assert os.path.getsize(os.path.join(tmp_path, "lora", "2.pth")) < 2 * a.lora.held_bytes() + (1 << 16)
    want = [a.train_step(lat, di, timestep_indices=idx, noise=noise) for _ in range(2)]
    b = _twin(cfg, sd, dev, seed=99)                 # other adapters: the load has to replace them
    b.load_checkpoint(str(tmp_path), 2)
    assert b.global_step == 2 and not b.lora.merged()
    got = [b.train_step(lat, di, timestep_indices=idx, noise=noise) for _ in range(2)]
    for i, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(_bits(x.float()), _bits(y.float())), (i, x.item(), y.item())
    for (k, v), w in zip(a.lora.state_dict().items(), b.lora.state_dict().values()):
        assert torch.equal(_bits(v), _bits(w)), k


def test_fold_is_the_merge_and_unfold_takes_it_back(dev, base):
    cfg, sd, inp = base
    lat, di, _, _ = _batch(inp, dev)
    ts = inp["timestep"].to(dev)

    def infer(model):
        model.eval()
        with torch.no_grad():
            return model(lat.to(bf16), ts, **di)[0][0]
    m = _model(cfg, sd, dev)
    plain = infer(m)
    la = _adapters(m, b_std=0.05)
    la.merge_()
    merged = infer(m)
    assert la.merged() and not torch.equal(merged, plain)
    copy = _model(cfg, sd, dev)
    la.fold_into_(copy)
    assert torch.equal(_bits(infer(copy)), _bits(merged))
    params = dict(copy.named_parameters())
    folded = {n: params[n].detach().clone() for n in la.names}
    assert all(not torch.equal(folded[n].cpu(), sd[n]) for n in la.names)
    la.unfold_from_(copy)
    for n in la.names:                               # the same s B A both times: what is left are the two roundings, half an ulp each
        w0, w1, wf = sd[n].double(), params[n].detach().double().cpu(), folded[n].double().cpu()
        assert bool(((w1 - w0).abs() <= 2.0 ** -23 * torch.maximum(w0.abs(), wf.abs()) * (1 + 2.0 ** -6)).all()), n
    for n, p in copy.named_parameters():             # nothing else moved
        if n not in la.names:
            assert torch.equal(p.detach().cpu(), sd[n]), n
    # a bf16 inference model takes the adapter in its own dtype
    half = _model(cfg, sd, dev).to(bf16).eval()
    la.fold_into_(half)
    e = rel_err(infer(half).float(), merged.float())
    assert e < 2e-2, e                               # W + s B A rounded once more to bf16: the same model within the forward's tolerance
