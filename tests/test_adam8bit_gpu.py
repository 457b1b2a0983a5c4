"""GPU leg (`-m gpu`) of the block-wise 8-bit AdamW: the HIP kernels (dwm_quantize_blockwise8, dwm_dequantize_blockwise8,
dwm_adamw8_multi) against the plain-torch restatement of tests/test_adam8bit_cpu.py, train.AdamW8bit against fp32 AdamW,
through CTSDTrainer, through checkpoints, and its memory."""
import math
import os

import pytest
import torch

from opendwm_amd.quant8 import dynamic_code
from tests import test_adam8bit_cpu as R          # the restatement: encode / decode / step, the trajectory, CODE_CAP
from tests.common import rel_err
from tests.test_train_gpu import _log         # one JSON line per measurement into the suite's gpu_parity.log

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
bf16 = torch.bfloat16

# |p8 - p32| / |p32 - p0| of the CPU restatement after the 50 steps of R.trajectory_inputs() (seed 0, 65 536 elements, log-normal
# gradient scales of sigma 2, R.HYPER), printed by tests/test_adam8bit_cpu.py::test_restatement_against_fp32_adamw_is_reported:
# 0.312612.  The HIP path agrees with the restatement to R.CODE_CAP per step, so this is its yardstick; 1.25 is the allowance.
TRAJECTORY_DEVIATION_RESTATEMENT = 0.312612
TRAJECTORY_BOUND = 1.25 * TRAJECTORY_DEVIATION_RESTATEMENT


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _heavy(n, seed, positive=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.exp(2.0 * torch.randn(n, generator=g)) * torch.randn(n, generator=g)
    return x * x if positive else x


# ------------------------------------------------------------------------------- quantise / dequantise
@pytest.mark.parametrize("signed", [True, False])
def test_quantize_dequantize_match_restatement(dev, signed):
    from opendwm_amd import train_ops as T
    code = dynamic_code(signed)
    code_d = code.to(dev)
    res = {}
    for n in (1, 255, 256, 257, 100_003, 1 << 20):
        x = _heavy(n, n, positive=not signed)
        if n > 1024:
            x[512:768] = 0.0                                    # one all-zero block
        for floor in ((False, True) if not signed else (False,)):
            q, a = T.quantize_blockwise8(x.to(dev), code_d, floor_positive=floor)
            q_ref, a_ref = R.encode(x, code, floor_positive=floor)
            assert q.dtype == torch.uint8 and q.shape == x.shape and a.shape == (math.ceil(n / 256),)
            assert torch.equal(a.cpu(), a_ref)                                         # scales: bit-equal
            share, dist = R.code_disagreement(q.cpu(), q_ref)
            res[f"{n}{'+floor' if floor else ''}"] = share
            assert share <= R.CODE_CAP and dist <= 1, (n, floor, share, dist)
            assert torch.equal(T.dequantize_blockwise8(q, a, code_d).cpu(), R.decode(q.cpu(), a.cpu(), code))    # bit-equal
            if n > 1024:
                zc = int((code == 0).nonzero())
                assert a[2].item() == 0.0 and bool((q[512:768] == zc).all())
            if floor:
                assert bool((q.cpu()[x > 0] > 0).all())
    _log("quantize_blockwise8", signed=signed, share_of_differing_codes=res)


def test_quantize_unaligned_views(dev):
    """pointers off the 16-byte / 4-byte grid take the element-wise path: same result"""
    from opendwm_amd import train_ops as T
    code = dynamic_code(True)
    x = _heavy(5000, 3)
    buf = torch.zeros(5001, device=dev)
    buf[1:] = x.to(dev)
    q, a = T.quantize_blockwise8(buf[1:], code.to(dev))
    q_ref, a_ref = R.encode(x, code)
    assert torch.equal(q.cpu(), q_ref) and torch.equal(a.cpu(), a_ref)
    qb = torch.zeros(5001, dtype=torch.uint8, device=dev)
    qb[1:] = q
    assert torch.equal(T.dequantize_blockwise8(qb[1:], a, code.to(dev)).cpu(), R.decode(q_ref, a_ref, code))


# ------------------------------------------------------------------------------- one step from identical state
def test_adamw8_step_matches_restatement(dev):
    """three consecutive dwm_adamw8_multi steps over a list with odd lengths, a tensor longer than one workgroup's chunk and a
    gradient off the 16-byte grid; before each step the restatement is given the kernel's state, so every comparison is one
    step from identical state.  p to the bound test_adamw_matches_torch holds the fp32 kernel to; the shadow is p.to(bf16); the
    new codes within R.CODE_CAP (share over the whole list), one adjacent code at most."""
    from opendwm_amd import train_ops as T
    numels = [4099, 2 * T.ADAMW_CHUNK + 777, 256, 1000, 70_000, 5]
    assert max(numels) > T.ADAMW_CHUNK
    hyper = dict(lr=3e-4, b1=0.9, b2=0.95, eps=1e-8, wd=0.01)
    kw = dict(lr=3e-4, beta1=0.9, beta2=0.95, eps=1e-8, weight_decay=0.01)
    ps = [_heavy(n, 10 + i).to(dev) for i, n in enumerate(numels)]
    st = [[t.to(dev) for t in R.fresh_state(n)] for n in numels]
    shadows = [None if i == 3 else torch.empty(n, dtype=bf16, device=dev) for i, n in enumerate(numels)]
    worst_p, worst_share = 0.0, 0.0
    for t in range(1, 4):
        gs = [_heavy(n, 100 * t + i) for i, n in enumerate(numels)]
        gbuf = torch.zeros(numels[4] + 1, device=dev)
        gbuf[1:] = gs[4].to(dev)
        gd = [gbuf[1:] if i == 4 else g.to(dev) for i, g in enumerate(gs)]
        before = [(p.cpu(), [s.cpu() for s in s4]) for p, s4 in zip(ps, st)]
        # grad_scale = 0.5 on doubled gradients is the same step (a power of two: exact) - checked bit for bit on a copy
        ps2, st2 = [p.clone() for p in ps], [[s.clone() for s in s4] for s4 in st]
        T.adamw8_multi_(ps2, [2 * g for g in gd[:4]] + [(2 * gbuf)[1:]] + [2 * gd[5]], *map(list, zip(*st2)), [None] * len(ps),
                        step=t, grad_scale=0.5, **kw)
        T.adamw8_multi_(ps, gd, *map(list, zip(*st)), shadows, step=t, **kw)
        differ = total = 0
        for i, n in enumerate(numels):
            p0, s0 = before[i]
            p_ref, mq, ma, vq, va = R.step(p0, gs[i], *s0, t, **hyper)
            worst_p = max(worst_p, rel_err(ps[i], p_ref))
            assert rel_err(ps[i], p_ref) < 1e-6, (t, n)
            if shadows[i] is not None:
                assert torch.equal(shadows[i], ps[i].to(bf16))
            for got, want in ((st[i][0], mq), (st[i][2], vq)):
                share, dist = R.code_disagreement(got.cpu(), want)
                assert dist <= 1, (t, n, dist)
                differ, total = differ + round(share * n), total + n
            for got, want in ((st[i][1], ma), (st[i][3], va)):
                assert torch.allclose(got.cpu(), want, rtol=1e-6, atol=0), (t, n)
            assert torch.equal(ps[i], ps2[i]) and all(torch.equal(a, b) for a, b in zip(st[i], st2[i])), (t, n)
        worst_share = max(worst_share, differ / total)
        assert differ / total <= R.CODE_CAP, (t, differ, total)
    _log("adamw8_step", worst_rel_p=worst_p, worst_share_of_differing_codes=worst_share, steps=3, tensors=len(numels))


# ------------------------------------------------------------------------------- against fp32 AdamW
def test_trajectory_against_fp32_adamw(dev):
    """the 50-step heavy-tailed trajectory through train.AdamW8bit (HIP) and through torch.optim.AdamW: the relative deviation
    |p8 - p32| / |p32 - p0| is held to 1.25 x the CPU restatement's figure for the same trajectory"""
    from opendwm_amd.train import AdamW8bit
    p0, grads = R.trajectory_inputs()
    p8 = torch.nn.Parameter(p0.to(dev))
    opt = AdamW8bit([p8], lr=R.HYPER["lr"], betas=(R.HYPER["b1"], R.HYPER["b2"]), eps=R.HYPER["eps"], weight_decay=R.HYPER["wd"])
    for g in grads:
        p8.grad = g.to(dev)
        opt.step()
    assert opt.t == len(grads) and opt.state[p8]["exp_avg"].dtype == torch.uint8
    p32 = R.fp32_adamw_trajectory(p0, grads)
    ref8, _ = R.trajectory(torch.float32, p0, grads)
    dev8 = ((p8.detach().cpu() - p32).norm() / (p32 - p0).norm()).item()
    vs_restatement = ((p8.detach().cpu() - ref8).norm() / (ref8 - p0).norm()).item()
    _log("adamw8_trajectory", deviation_from_fp32_adamw=dev8, restatement=TRAJECTORY_DEVIATION_RESTATEMENT, bound=TRAJECTORY_BOUND,
         hip_vs_restatement=vs_restatement)
    assert dev8 <= TRAJECTORY_BOUND


# ------------------------------------------------------------------------------- through the trainer
def _small_problem(dev):
    from oracle import ctsd_oracle as O
    from tests.common import small_config, small_inputs, to_dev
    cfg = small_config()
    sd = {k: v.to(bf16).float() for k, v in O.make_state_dict(cfg, 0).items()}
    inp = small_inputs(cfg, 0)
    inp = {k: (v.to(bf16).float() if v.is_floating_point() and k not in ("timestep", "added_time_ids") else v) for k, v in inp.items()}
    lat = inp.pop("sample")
    inp.pop("timestep")
    return cfg, sd, lat.to(dev), to_dev(inp, dev)


def _train(dev, problem, bits, seed, steps, training_config=None):
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.pipeline import CTSDTrainer
    cfg, sd, lat, cond = problem
    m = DiTCrossviewTemporalConditionModel(**cfg)
    m.load_state_dict(sd)
    tr = CTSDTrainer(m.to(dev).train(), lr=2e-4, weight_decay=0.0, optimizer_bits=bits, training_config=training_config)
    noise = torch.randn(lat.shape, generator=torch.Generator().manual_seed(seed))
    idx = torch.tensor([250, 800])
    losses = [tr.train_step(lat, cond, timestep_indices=idx, noise=noise).item() for _ in range(steps)]
    return tr, losses


def test_trainer_with_8bit_optimizer(dev):
    """the smallest DiT config tests/test_train_gpu.py trains, 20 steps on one batch: both loss curves fall and the 8-bit final
    loss lies within twice the spread of the 32-bit final loss over three noise seeds; with the GradScaler and the gradient
    clip in the loop the 8-bit run stays finite.  The margin is measured in the test itself; on an MI355X while writing: finals
    with fp32 moments 0.969870 / 0.969797 / 0.965127 (margin 0.009487), with 8-bit moments 0.969581."""
    from opendwm_amd.train import AdamW8bit
    problem, steps = _small_problem(dev), 20
    runs32 = [_train(dev, problem, 32, seed, steps)[1] for seed in (5, 6, 7)]
    tr8, run8 = _train(dev, problem, 8, 5, steps)
    assert type(tr8.optimizer) is AdamW8bit
    n8 = sum(1 for st in tr8.optimizer.state.values() if st["exp_avg"].dtype == torch.uint8)
    finals = [r[-1] for r in runs32]
    margin = 2.0 * (max(finals) - min(finals))
    _log("adamw8_trainer", first_loss=run8[0], final_8bit=run8[-1], finals_32bit=finals, margin=margin,
         quantised_tensors=n8, tensors=len(tr8.optimizer.state))
    assert n8 > 0 and abs(run8[0] - runs32[0][0]) <= 1e-6 * abs(run8[0])                      # same start, and the 8-bit kernel really ran
    assert all(r[-1] < r[0] for r in runs32) and run8[-1] < run8[0]
    assert abs(run8[-1] - finals[0]) <= margin
    _, scaled = _train(dev, problem, 8, 5, 6, training_config={"enable_grad_scaler": True, "max_norm_for_grad_clip": 1.0})
    _log("adamw8_trainer_scaler_clip", losses=scaled)
    assert all(math.isfinite(x) for x in scaled)


# ------------------------------------------------------------------------------- checkpoints
def _toy_trainer(dev, zero=False):
    from opendwm_amd.pipeline import CTSDTrainer
    torch.manual_seed(11)
    model = torch.nn.Sequential(torch.nn.Linear(64, 129), torch.nn.SiLU(), torch.nn.Linear(129, 64)).to(dev)    # 8256-element weights
    if zero:
        with torch.no_grad():
            for q in model.parameters():
                q.zero_()
    return CTSDTrainer(model, lr=1e-2, betas=(0.9, 0.95), weight_decay=0.05, optimizer_bits=8)


def _toy_step(tr, t, dev):
    g = torch.Generator().manual_seed(1000 + t)
    for q in tr.model.parameters():
        q.grad = (torch.randn(q.shape, generator=g) * math.exp(t % 3)).to(dev)
    tr.optimizer.step()
    tr.optimizer.zero_grad()


def test_checkpoint_resume_is_bit_identical(dev, tmp_path):
    """save after three steps, load into a fresh trainer, one more step: parameters and state equal the uninterrupted run's, bit
    for bit (gradients are given, so nothing but the optimizer and the checkpoint layout is in the loop)"""
    a = _toy_trainer(dev)
    for t in range(3):
        _toy_step(a, t, dev)
    a.save_checkpoint(str(tmp_path), 3)
    _toy_step(a, 3, dev)
    b = _toy_trainer(dev, zero=True)
    b.load_checkpoint(str(tmp_path), 3)
    assert b.optimizer.t == 3 and (b.optimizer.lr, b.optimizer.betas) == (1e-2, (0.9, 0.95))
    _toy_step(b, 3, dev)
    kinds = set()
    for qa, qb in zip(a.model.parameters(), b.model.parameters()):
        assert torch.equal(qa, qb)
        sa, sb = a.optimizer.state[qa], b.optimizer.state[qb]
        assert sorted(sa) == sorted(sb)
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and torch.equal(sa[k].cpu(), sb[k].cpu()), k
        kinds.add(sa["exp_avg"].dtype)
    assert kinds == {torch.uint8, torch.float32}                  # weights quantised, biases (< min_8bit_size) fp32


@pytest.mark.parametrize("case", ["reference_checkpoint", "reference_checkpoint_frozen"])
def test_reference_fp32_optimizer_file_loads_and_exports(dev, case):
    """the fp32 optimizer file written by the reference's save path loads into AdamW8bit (quantised on load), and
    state_dict_fp32() gives every moment back within one code step of its block scale, in a layout torch.optim.AdamW loads"""
    from opendwm_amd.pipeline import CTSDTrainer, freeze_modules
    from opendwm_amd.train import AdamW8bit
    from tests.golden.make_reference_checkpoint_fixture import FREEZING_PATTERN, tiny_model
    root = os.path.join(GOLDEN, case)
    theirs = torch.load(os.path.join(root, "optimizer", "3.pth"), map_location="cpu", weights_only=True)
    tr = CTSDTrainer.__new__(CTSDTrainer)
    tr.model = tiny_model().to(dev)
    if case.endswith("frozen"):
        freeze_modules(tr.model, FREEZING_PATTERN)
    tr.optimizer = AdamW8bit(tr.model.parameters(), lr=123.0, min_8bit_size=1)
    tr.load_checkpoint(root, 3)
    opt = tr.optimizer
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay, opt.t) == (1e-2, (0.9, 0.95), 1e-8, 0.05, 3)
    assert len(opt.state) == len(theirs["state"])
    assert all(st["exp_avg"].dtype == torch.uint8 and st["exp_avg_sq_absmax"].dtype == torch.float32 for st in opt.state.values())
    back = opt.state_dict_fp32()
    assert sorted(back["state"]) == sorted(theirs["state"]) and back["param_groups"][0]["params"] == theirs["param_groups"][0]["params"]
    worst = 0.0
    for i, st in theirs["state"].items():
        assert sorted(back["state"][i]) == ["exp_avg", "exp_avg_sq", "step"] and float(back["state"][i]["step"]) == 3.0
        for key, signed in (("exp_avg", True), ("exp_avg_sq", False)):
            want, got = st[key].flatten(), back["state"][i][key].cpu().flatten()
            assert got.dtype == torch.float32 and back["state"][i][key].shape == st[key].shape
            code = dynamic_code(signed)
            scale = want.abs().max()                                   # n <= 256: one block
            err = ((got - want).abs().max() / scale).item()
            worst = max(worst, err)
            assert err <= (code[1:] - code[:-1]).max().item()
            if not signed:
                assert bool((got[want > 0] > 0).all())                 # the guard: no positive second moment came back as zero
    ref_opt = torch.optim.AdamW(tiny_model().parameters())
    ref_opt.load_state_dict({"state": {i: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in st.items()}
                                       for i, st in back["state"].items()}, "param_groups": back["param_groups"]})
    _log("adamw8_reference_checkpoint", case=case, worst_error_over_block_scale=worst)


# ------------------------------------------------------------------------------- memory
def test_state_memory_is_lower_by_the_arithmetic_amount(dev):
    """torch.cuda.memory_allocated after the first step, AdamW8bit against train.AdamW on the same list: lower by
    2 * (4 n - n - 4 ceil(n / 256)) summed over the quantised tensors, within the allocator's rounding (2 MiB per tensor)"""
    import gc
    from opendwm_amd.blocks import STORE
    from opendwm_amd.train import AdamW, AdamW8bit
    shapes = [(1536, 1536), (4608, 1536), (1536,), (3, 1000, 1001), (64,)]

    def held(cls):
        STORE.bump()
        gc.collect()
        torch.cuda.synchronize()
        params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
        for q in params:
            q.grad = torch.ones_like(q)
        opt = cls(params, lr=1e-3)
        base = torch.cuda.memory_allocated(dev)
        opt.step()
        torch.cuda.synchronize()
        used = torch.cuda.memory_allocated(dev) - base
        quantised = [q.numel() for q in params if opt.state[q]["exp_avg"].dtype == torch.uint8]
        del opt, params
        return used, quantised

    used32, q32 = held(AdamW)
    used8, q8 = held(AdamW8bit)
    STORE.bump()
    want = sum(2 * (4 * n - n - 4 * math.ceil(n / 256)) for n in q8)
    _log("adamw8_memory", fp32_state_bytes=used32, int8_state_bytes=used8, saved=used32 - used8, arithmetic=want)
    assert q32 == [] and sorted(q8) == sorted(math.prod(s) for s in shapes if math.prod(s) >= 4096)
    assert abs((used32 - used8) - want) <= len(q8) * (2 << 20)
