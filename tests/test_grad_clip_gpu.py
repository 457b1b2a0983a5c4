"""GPU leg (`-m gpu`) of the fused gradient clip / unscale / non-finite check: the HIP kernels of gradnorm.hip
(dwm_grad_sumsq_multi, dwm_grad_scale_multi) against the fp64 restatement of tests/test_grad_clip_cpu.py, train.clip_grad_norm_
against torch's, and CTSDTrainer(grad_conditioning="fused") against the default torch route."""
import pytest
import torch

from tests import test_grad_clip_cpu as R          # the restatement ref(), the derived bound, the heavy-tailed recipe
from tests.test_train_gpu import _log, _train_model         # one JSON line per measurement into the suite's gpu_parity.log

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32

# the smallest sizes that reach every path: a tensor smaller than a vector, chunk seams on both sides (chunk = 65 536), partial
# last chunks, and - the last three - views of one buffer that start 1, 2 and 3 elements past a 16-byte boundary
NUMELS = [1, 3, 255, 256, 257, 4095, 4096, 65535, 65536, 65537, 3 * 65536 + 5]
VIEWS = [(1, 1021), (2, 65536), (3, 70001)]                 # (elements past the 16-byte grid, length)
PHASES = [0] * len(NUMELS) + [ph for ph, _ in VIEWS]
ALL_NUMELS = NUMELS + [n for _, n in VIEWS]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def heavy():
    """host values of the list, g = randn * exp(2 * randn), and their fp64 norm; never modified"""
    vals = [R._heavy(n, 1000 + i) for i, n in enumerate(ALL_NUMELS)]
    return vals, torch.sqrt(sum(v.double().pow(2).sum() for v in vals)).item()


def _device_list(vals, dev):
    """the list on the device: own allocations for NUMELS, three views of ONE buffer at the offsets of VIEWS"""
    out = [v.to(dev) for v in vals[:len(NUMELS)]]
    buf, off = torch.zeros(sum(n + 8 for _, n in VIEWS), device=dev), 0
    for (ph, n), v in zip(VIEWS, vals[len(NUMELS):]):
        off = (off + 3) // 4 * 4 + ph
        buf[off:off + n] = v.to(dev)
        out.append(buf[off:off + n])
        off += n
    assert all((t.data_ptr() // 4) % 4 == ph for t, ph in zip(out, PHASES))
    return out


def _guarded_list(vals, dev, guard):
    """every tensor an interior view (at its phase of the 16-byte grid) of a buffer of its own filled with `guard`"""
    out = []
    for v, ph in zip(vals, PHASES):
        buf = torch.full((v.numel() + 12,), guard, device=dev)
        buf[4 + ph:4 + ph + v.numel()] = v.to(dev)
        out.append(buf[4 + ph:4 + ph + v.numel()])
    return out


def _coef_from(norm32: torch.Tensor, pre_scale: float, max_norm: float) -> torch.Tensor:
    """the fp32 formula applied to a given fp32 norm (host, IEEE division)"""
    q = torch.tensor(max_norm, dtype=f32) / (norm32.cpu() + torch.tensor(1e-6, dtype=f32))
    return torch.tensor(pre_scale, dtype=f32) * torch.clamp(q, max=1.0)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.detach().cpu().contiguous().view(torch.int32)


def test_kernel_against_fp64(dev, heavy):
    from opendwm_amd import train_ops as T
    vals, n64 = heavy
    E = T.GRAD_SUMSQ_E
    assert E <= 256
    bound = R.norm_bound(E)
    gs = _device_list(vals, dev)
    res = {}
    for factor in (0.5, 2.0):
        max_norm = factor * n64
        out = T.grad_sumsq_multi(gs, 1.0, max_norm).cpu()
        rel = abs(out[0].double().item() - n64) / n64
        res[factor] = rel
        print("grad_sumsq_multi", dict(max_norm_over_norm=factor, rel=rel, bound=bound, out=out.tolist()))
        assert rel <= bound, (factor, rel, bound)
        assert torch.equal(_bits(out[1]), _bits(_coef_from(out[0], 1.0, max_norm)))             # bit for bit
        assert (out[1].item() == 1.0) == (factor == 2.0) and out[2].item() == 0.0 and out[3].item() == 0.0
        norm_ref, coef_ref, found_ref = R.ref(vals, 1.0, max_norm)
        assert not found_ref and abs(out[1].item() - coef_ref.item()) <= 2 * bound * coef_ref.item()
    none = T.grad_sumsq_multi(gs, 0.25, None).cpu()               # no clip: coef = pre_scale, norm of the scaled list
    assert none[1].item() == 0.25 and torch.equal(_bits(none[0]), _bits(T.grad_sumsq_multi(gs, 0.25, 0.0).cpu()[0]))
    assert abs(none[0].double().item() - 0.25 * n64) / (0.25 * n64) <= bound
    _log("grad_sumsq_multi", E=E, bound=bound, rel_err_of_norm=res)


def test_power_of_two_scale_is_exact(dev):
    from opendwm_amd import train_ops as T
    g = torch.Generator().manual_seed(7)
    vals = [torch.randn(n, generator=g) for n in ALL_NUMELS]       # randn only: nothing over- or underflows
    n64 = torch.sqrt(sum(v.double().pow(2).sum() for v in vals)).item()
    plain = T.grad_sumsq_multi(_device_list(vals, dev), 1.0, 0.5 * n64).cpu()
    scaled = T.grad_sumsq_multi(_device_list([v * 65536.0 for v in vals], dev), 2.0 ** -16, 0.5 * n64).cpu()
    assert torch.equal(_bits(scaled[0]), _bits(plain[0]))
    assert torch.equal(_bits(scaled[1] * 65536.0), _bits(plain[1])) and plain[1].item() < 1.0
    assert scaled[2].item() == 0.0 and plain[2].item() == 0.0


def test_non_finite_detection(dev, heavy):
    from opendwm_amd import train_ops as T
    vals, _ = heavy
    gs = _device_list(vals, dev)
    assert T.grad_sumsq_multi(gs, 1.0, 1.0)[2].item() == 0.0
    big = len(NUMELS) - 1
    places = {"first element of the first tensor = the 1-element tensor": (0, 0),
              "first element of a long tensor": (big, 0),
              "last element of a partial tail": (big, NUMELS[big] - 1),
              "unaligned head of a view": (len(NUMELS), 0),
              "last element of an unaligned view": (len(ALL_NUMELS) - 1, ALL_NUMELS[-1] - 1),
              "middle of a chunk": (8, 30001),
              "middle of a later chunk of a view": (len(ALL_NUMELS) - 1, 65536 + 2222)}
    assert NUMELS[0] == 1 and NUMELS[big] % 65536 == 5
    for what, (i, j) in places.items():
        keep = gs[i][j].item()
        for bad in (float("inf"), float("-inf"), float("nan")):
            gs[i][j] = bad
            assert T.grad_sumsq_multi(gs, 1.0, 1.0)[2].item() == 1.0, (what, bad)
            assert T.grad_sumsq_multi(gs, 2.0 ** -16, None)[2].item() == 1.0, (what, bad)
        gs[i][j] = keep
    assert T.grad_sumsq_multi(gs, 1.0, 1.0)[2].item() == 0.0


def test_isolation(dev, heavy):
    """NaN directly before and after every tensor: never read (it would raise the flag and poison the sum)"""
    from opendwm_amd import train_ops as T
    vals, n64 = heavy
    clean = T.grad_sumsq_multi(_guarded_list(vals, dev, 0.0), 1.0, 0.5 * n64).cpu()
    fenced_list = _guarded_list(vals, dev, float("nan"))
    fenced = T.grad_sumsq_multi(fenced_list, 1.0, 0.5 * n64).cpu()
    assert fenced[2].item() == 0.0 and torch.equal(_bits(fenced), _bits(clean))
    # the in-place scale writes nothing outside either: the guards stay NaN, the values are g * coef
    T.grad_scale_multi_(fenced_list, 0.5)
    for t, v in zip(fenced_list, vals):
        base = t._base
        assert torch.equal(t.cpu(), v * 0.5)
        assert bool(torch.isnan(base[:t.storage_offset()]).all()) and bool(torch.isnan(base[t.storage_offset() + t.numel():]).all())


def test_determinism(dev, heavy):
    from opendwm_amd import train_ops as T
    vals, n64 = heavy
    gs = _device_list(vals, dev)
    a = T.grad_sumsq_multi(gs, 1.0, 0.5 * n64).cpu()
    b = T.grad_sumsq_multi(gs, 1.0, 0.5 * n64).cpu()
    assert torch.equal(_bits(a), _bits(b))


def _params_with(gs):
    ps = [torch.nn.Parameter(torch.empty_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g
    return ps


def test_clip_grad_norm(dev, heavy, monkeypatch):
    from opendwm_amd import train
    from opendwm_amd import train_ops as T
    vals, n64 = heavy
    bound = R.norm_bound(T.GRAD_SUMSQ_E)
    calls, scale0 = [], T.grad_scale_multi_

    def recording(gs, coef):
        calls.append(coef)
        return scale0(gs, coef)
    monkeypatch.setattr(T, "grad_scale_multi_", recording)
    # clipping
    gs = _device_list(vals, dev)
    before = [g.clone() for g in gs]
    norm = train.clip_grad_norm_(_params_with(gs), 0.5 * n64)
    assert torch.is_tensor(norm) and abs(norm.item() - n64) / n64 <= bound and len(calls) == 1
    coef = calls[0]
    assert torch.equal(_bits(torch.tensor(coef, dtype=f32)), _bits(_coef_from(norm.float(), 1.0, 0.5 * n64)))
    for g, g0 in zip(gs, before):
        assert torch.equal(g, g0 * coef)                          # bit-equal to torch's product with the same coefficient
    # not clipping: nothing is launched, nothing changes
    gs = _device_list(vals, dev)
    norm2 = train.clip_grad_norm_(_params_with(gs), 2.0 * n64)
    assert len(calls) == 1 and torch.equal(_bits(norm2), _bits(norm))
    for g, g0 in zip(gs, before):
        assert torch.equal(_bits(g), _bits(g0))
    # against torch's own clip on a copy
    theirs = [g0.clone() for g0 in before]
    tn = torch.nn.utils.clip_grad_norm_(_params_with(theirs), 0.5 * n64)
    rel = abs(norm.item() - tn.item()) / tn.item()
    print("clip_grad_norm_", dict(ours=norm.item(), torch=tn.item(), fp64=n64, rel=rel, bound=bound))
    _log("clip_grad_norm_", ours=norm.item(), torch=tn.item(), fp64=n64, rel_to_torch=rel, bound=bound)
    assert rel <= bound
    # a non-fp32 gradient goes the way AdamW.step reads it (.float()), and gets the scaled values back
    p = torch.nn.Parameter(torch.zeros(1000, dtype=bf16, device=dev))
    p.grad = vals[5][:1000].to(dev).to(bf16)
    g0 = p.grad.clone()
    n16 = train.clip_grad_norm_([p], 0.5 * g0.double().norm().item())
    assert abs(n16.item() - g0.double().norm().item()) <= bound * n16.item()
    assert torch.equal(p.grad, (g0.float() * calls[-1]).to(bf16))


# ------------------------------------------------------------------------------- the trainer
@pytest.fixture(scope="module")
def problem(dev):
    """the small DiT config, state dict and inputs of tests/test_train_gpu.py::test_train_step_grad_scaler_mode, and the gradient
    norm of the first step (read once, from a torch-mode trainer's backward)"""
    from oracle import ctsd_oracle as O
    from opendwm_amd.pipeline import CTSDTrainer
    from tests.common import small_config, small_inputs, to_dev
    cfg = small_config()
    sd = {k: v.to(bf16).float() for k, v in O.make_state_dict(cfg, 0).items()}
    inp = small_inputs(cfg, 0)
    inp = {k: (v.to(bf16).float() if v.is_floating_point() and k not in ("timestep", "added_time_ids") else v) for k, v in inp.items()}
    lat = inp.pop("sample")
    inp.pop("timestep")
    noise = torch.randn(lat.shape, generator=torch.Generator().manual_seed(5))
    idx = torch.tensor([250, 800])
    di = to_dev(inp, dev)
    probe = CTSDTrainer(_train_model(cfg, sd, dev), lr=2e-4, weight_decay=0.0)
    probe.loss(lat.to(dev), di, timestep_indices=idx, noise=noise).backward()
    norm = torch.sqrt(sum(p.grad.double().pow(2).sum() for p in probe.model.parameters() if p.grad is not None)).item()
    assert norm > 0 and norm == norm
    return dict(cfg=cfg, sd=sd, lat=lat, di=di, noise=noise, idx=idx, norm=norm, dev=dev)


def _trainer(pb, tc, mode, **kw):
    from opendwm_amd.pipeline import CTSDTrainer
    return CTSDTrainer(_train_model(pb["cfg"], pb["sd"], pb["dev"]), lr=2e-4, weight_decay=0.0, training_config=dict(tc),
                       grad_conditioning=mode, **kw)


def _step(pb, tr, lat=None):
    return tr.train_step((pb["lat"] if lat is None else lat).to(pb["dev"]), pb["di"], timestep_indices=pb["idx"], noise=pb["noise"]).item()


def _worst(a, b):
    """metric of test_train_step_grad_scaler_mode: max over parameters of max|a - b| / max|b|"""
    return max(((x.detach() - y.detach()).abs().max() / y.detach().abs().max().clamp_min(1e-12)).item()
               for x, y in zip(a.model.parameters(), b.model.parameters()))


def _moved(pb, tr):
    return any(not torch.equal(p.detach().cpu(), pb["sd"][k].to(p.dtype)) for k, p in tr.model.named_parameters() if k in pb["sd"])


def _one_step_pair(pb, tc, name):
    plain, fused = _trainer(pb, tc, "torch"), _trainer(pb, tc, "fused")
    l0, l1 = _step(pb, plain), _step(pb, fused)
    worst = _worst(fused, plain)
    _log("grad_conditioning_" + name, loss_torch=l0, loss_fused=l1, worst_param_rel=worst, last_grad_norm=fused.last_grad_norm,
         first_step_norm=pb["norm"])
    assert abs(l0 - l1) <= 1e-6 * abs(l0) and worst < 1e-5 and _moved(pb, fused), (l0, l1, worst)
    assert fused.optimizer.t == 1 and fused.skipped_steps == 0
    return plain, fused


def test_trainer_fused_matches_torch_and_skips_poisoned_steps(problem):
    from opendwm_amd.train import LossScaler
    pb = problem
    m = 0.5 * pb["norm"]
    plain, fused = _one_step_pair(pb, {"enable_grad_scaler": True, "max_norm_for_grad_clip": m}, "scaler_and_clip")
    assert isinstance(fused.grad_scaler, LossScaler) and isinstance(plain.grad_scaler, torch.amp.GradScaler)
    assert fused.last_grad_norm > m and abs(fused.last_grad_norm - pb["norm"]) < 1e-3 * pb["norm"]        # the clip was active
    assert fused.grad_scaler.get_scale() == 65536.0
    before = [p.detach().clone() for p in fused.model.parameters()]
    t_before = fused.optimizer.t
    bad = pb["lat"].clone()
    bad[0, 0, 0, 0, 0, 0] = float("inf")
    _step(pb, fused, bad)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, fused.model.parameters()))                # bit-identical
    assert fused.optimizer.t == t_before and fused.grad_scaler.get_scale() == 32768.0 and fused.skipped_steps == 1
    assert all(p.grad is None or not p.grad.any() for p in fused.model.parameters())                        # zero_grad ran
    l2 = _step(pb, fused)
    assert l2 == l2 and abs(l2) != float("inf") and fused.optimizer.t == t_before + 1 and fused.skipped_steps == 1


def test_trainer_clip_only(problem):
    m = 0.5 * problem["norm"]
    plain, fused = _one_step_pair(problem, {"max_norm_for_grad_clip": m}, "clip_only")
    assert fused.grad_scaler is None and plain.grad_scaler is None and fused.last_grad_norm > m


def test_trainer_clip_only_skips_a_non_finite_step(problem):
    """the one deliberate deviation (fused mode only): without a scaler the torch route would write nan into every weight"""
    pb = problem
    fused = _trainer(pb, {"max_norm_for_grad_clip": 0.5 * pb["norm"]}, "fused")
    before = [p.detach().clone() for p in fused.model.parameters()]
    bad = pb["lat"].clone()
    bad[0, 0, 0, 0, 0, 0] = float("inf")
    with pytest.warns(UserWarning, match="non-finite gradient"):
        _step(pb, fused, bad)
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, fused.model.parameters()))
    assert fused.optimizer.t == 0 and fused.skipped_steps == 1
    l1 = _step(pb, fused)
    assert l1 == l1 and fused.optimizer.t == 1


def test_trainer_scaler_only(problem):
    plain, fused = _one_step_pair(problem, {"enable_grad_scaler": True}, "scaler_only")
    assert fused.max_grad_norm is None and abs(fused.last_grad_norm - problem["norm"]) < 1e-3 * problem["norm"]


def test_trainer_gradient_accumulation(problem):
    pb = problem
    tc = {"enable_grad_scaler": True, "max_norm_for_grad_clip": 0.5 * pb["norm"], "gradient_accumulation_steps": 2}
    plain, fused = _trainer(pb, tc, "torch"), _trainer(pb, tc, "fused")
    for tr in (plain, fused):
        _step(pb, tr)
        assert not _moved(pb, tr) and tr.optimizer.t == 0            # first call: weights bit-identical
        _step(pb, tr)
        assert _moved(pb, tr) and tr.optimizer.t == 1 and tr.global_step == 2
    worst = _worst(fused, plain)
    _log("grad_conditioning_accumulation", worst_param_rel=worst, last_grad_norm=fused.last_grad_norm)
    assert worst < 1e-5 and fused.last_grad_norm > 1.5 * pb["norm"]     # the norm of the sum of two equal micro-steps


def test_trainer_8bit_optimizer_in_fused_mode(problem):
    pb = problem
    tr = _trainer(pb, {"enable_grad_scaler": True, "max_norm_for_grad_clip": 0.5 * pb["norm"]}, "fused", optimizer_bits=8)
    losses = [_step(pb, tr) for _ in range(6)]
    _log("grad_conditioning_8bit", losses=losses, skipped=tr.skipped_steps)
    assert all(l == l and abs(l) != float("inf") for l in losses) and losses[-1] < losses[0] and tr.optimizer.t == 6


# ------------------------------------------------------------------------------- one table cache for the three tensor-list kernels
def _interleaved_run(dev, clear_cache):
    """four rounds of grad_sumsq_multi -> adamw8_multi_ -> adamw_multi_ on an fp32-moment list, an 8-bit list and the gradient list of
    both, grad_scale taken from the norm call -> (every parameter, moment, code, scale and norm output on the host, the table
    pointers in the cache after each round).  clear_cache: the table cache is emptied before every call."""
    from opendwm_amd import quant8
    from opendwm_amd import train_ops as T
    numels = [5, 256, 4099, T.ADAMW_CHUNK + 1]
    gen = torch.Generator().manual_seed(11)
    rnd = lambda: [torch.randn(n, generator=gen).to(dev) for n in numels]
    zeros = lambda dtype=f32, fill=0: [torch.full((n,), fill, dtype=dtype, device=dev) for n in numels]
    scales = lambda: [torch.zeros(quant8.n_blocks(n), device=dev) for n in numels]
    p32, m32, v32, p8 = rnd(), zeros(), zeros(), rnd()
    mq, ma, vq, va = zeros(torch.uint8, quant8.zero_code(True)), scales(), zeros(torch.uint8, quant8.zero_code(False)), scales()
    hyper = dict(lr=1e-3, beta1=0.9, beta2=0.975, eps=1e-8, weight_decay=0.01)
    none = [None] * len(numels)

    def call(fn, *a, **kw):
        if clear_cache:
            T._BLOCK_TABLES.clear()
        return fn(*a, **kw)

    T._BLOCK_TABLES.clear()
    norms, ptrs = [], []
    for step in range(1, 5):
        g32, g8 = rnd(), rnd()
        out = call(T.grad_sumsq_multi, g32 + g8, 0.5, 1.0)
        norms.append(out.cpu())
        coef = norms[-1][1].item()
        assert 0.0 < coef < 0.5 and norms[-1][2].item() == 0.0                # the clip is active, nothing is non-finite
        call(T.adamw8_multi_, p8, g8, mq, ma, vq, va, none, step=step, grad_scale=coef, **hyper)
        call(T.adamw_multi_, p32, g32, m32, v32, none, step=step, grad_scale=coef, **hyper)
        ptrs.append({k: (t.block_item.data_ptr(), t.block_start.data_ptr()) for k, t in T._BLOCK_TABLES.items()})
    torch.cuda.synchronize()
    keys = {(dev.index, T.GRAD_CHUNK, tuple(numels + numels)), (dev.index, T.ADAMW_CHUNK, tuple(numels))}
    return [t.cpu() for lst in (p32, m32, v32, p8, mq, ma, vq, va) for t in lst] + norms, ptrs, keys


def test_shared_tables_interleaved(dev):
    """the gradient list and the two optimizer lists (equal numels: ONE entry serves the fp32 and the 8-bit launch) live side by
    side in the cache: the kernels get the same table buffers in every round, and every result is bit for bit what freshly built
    tables give"""
    from opendwm_amd import train_ops as T
    cached, ptrs, keys = _interleaved_run(dev, clear_cache=False)
    assert set(ptrs[0]) == keys and all(p == ptrs[0] for p in ptrs), ptrs
    fresh, one_entry, _ = _interleaved_run(dev, clear_cache=True)
    assert all(len(p) == 1 for p in one_entry)                                 # the cache really was empty before each call
    assert len(cached) == len(fresh) == 8 * 4 + 4
    for i, (a, b) in enumerate(zip(cached, fresh)):
        assert a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)), i
    assert all(bool(cached[i].any()) for i in (4, 8, 20, 23))                  # fp32 moments and 8-bit scales have left zero
    T._BLOCK_TABLES.clear()
