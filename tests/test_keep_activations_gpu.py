"""GPU leg (`-m gpu`) of the kept-activation mode of the SD 3.5 train step: the two kernels that re-derive an activation inside its
backward, each block kind with its activations kept against the same block recomputing them, and the model / trainer / DDP
behaviour of CTSDTrainer(activations=..., activation_budget_gib=...).

The keep path hands the same operands to the same kernels as the recompute path, so a gradient that recompute runs reproduce bit
for bit must come out bit-identical with the activations kept; the others are finished by fp32 atomics (train.hip) whose order
depends on the state the run finds the device in, and are held to the per-kernel tolerances of tests/test_train_gpu.py
(_compare_keep_with_recompute says how the two classes are told apart).  Measured on one MI355X: 85-93 % of the returned tensors of
every block kind are bit-identical (the condition is 80 %), the others 3e-8 to 1.1e-7 apart."""
import contextlib
import ctypes
import os
import socket

import pytest
import torch
import torch.nn.functional as F

from tests import gemm_check as gc
from tests.common import capture_segsum_diff, rel_err, small_config, small_inputs, to_dev
from tests.test_train_gpu import TOL_KERNEL, TOL_REDUCE, _log, _oracle_grads, _rand, _train_model

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
GRID_STRIDE = 256 * 32 * 256                # threads of a full grid of the element-wise kernels (train.hip grid_for): 8 elements each


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _fresh_param_store():
    """blocks.STORE keys its derived tensors (transposed / fused weights) on the identity of a parameter: the blocks and models of
    the test before are gone, and a new parameter may get the identity and the address of an old one of another shape"""
    from opendwm_amd.blocks import STORE
    STORE.bump()
    yield


# ------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (GRID_STRIDE + 3)])
@pytest.mark.parametrize("act", ["gelu_tanh", "silu"])
def test_act_bwd_recompute(dev, act, n):
    """y_out / dx bit-equal to dwm_act_fwd / dwm_act_bwd, within the tolerance of test_activation_fwd_bwd of fp64 autograd, written
    into fenced buffers: one vector, several blocks with a part-filled last one, and more vectors than a full grid has threads"""
    from opendwm_amd import ops, train_ops as T
    code = ops.ACT_GELU_TANH if act == "gelu_tanh" else ops.ACT_SILU
    f = (lambda t: F.gelu(t, approximate="tanh")) if act == "gelu_tanh" else F.silu
    x, dy = _rand((n,), dev, 1, 2.0), _rand((n,), dev, 2)
    y, ybuf = gc.fenced_vec(n, bf16, dev, fill="sentinel")
    dx, dxbuf = gc.fenced_vec(n, bf16, dev, fill="sentinel")
    T.act_bwd_recompute(x, dy, code, y_out=y, dx=dx)
    assert gc.untouched(ybuf, y) and gc.untouched(dxbuf, dx)
    assert torch.equal(y, T.act_fwd(x, code)) and torch.equal(dx, T.act_bwd(x, dy, code))
    xr = x.double().requires_grad_(True)
    yr = f(xr)
    yr.backward(dy.double())
    e1, e2 = rel_err(y, yr.detach()), rel_err(dx, xr.grad)
    _log("act_bwd_recompute", act=act, n=n, fwd=e1, bwd=e2)
    assert e1 < TOL_KERNEL and e2 < TOL_KERNEL
    y2, dx2 = T.act_bwd_recompute(x, dy, code)                 # the allocating form
    assert torch.equal(y2, y) and torch.equal(dx2, dx)


@pytest.mark.parametrize("inner", [8, 40])
@pytest.mark.parametrize("rows", [1, 3, 67])
def test_geglu_bwd_recompute(dev, rows, inner):
    """g_out / du bit-equal to dwm_geglu_fwd / dwm_geglu_bwd and within the tolerance of test_geglu_fwd_bwd of fp64 autograd, every
    leading dimension larger than the logical width, outputs fenced"""
    from opendwm_amd import train_ops as T
    u = _rand((rows, 2 * inner + 24), dev, 1, 1.5)[:, 8:8 + 2 * inner]
    dg = _rand((rows, inner + 8), dev, 2)[:, :inner]
    g, gbuf = gc.fenced((rows, inner), bf16, dev, col_off=8, pad_cols=16, fill="sentinel")
    du, dubuf = gc.fenced((rows, 2 * inner), bf16, dev, col_off=16, pad_cols=8, fill="sentinel")
    assert u.stride(0) > 2 * inner and dg.stride(0) > inner and g.stride(0) > inner and du.stride(0) > 2 * inner
    T.geglu_bwd_recompute(u, dg, g_out=g, du=du)
    assert gc.untouched(gbuf, g) and gc.untouched(dubuf, du)
    assert torch.equal(g, T.geglu_fwd(u)) and torch.equal(du, T.geglu_bwd(u, dg))
    ur = u.double().requires_grad_(True)
    hv, gt = ur.chunk(2, -1)
    gr = hv * F.gelu(gt)
    gr.backward(dg.double())
    e1, e2 = rel_err(g, gr.detach()), rel_err(du, ur.grad)
    _log("geglu_bwd_recompute", rows=rows, inner=inner, fwd=e1, bwd=e2)
    assert e1 < TOL_KERNEL and e2 < TOL_KERNEL
    g2, du2 = T.geglu_bwd_recompute(u, dg)
    assert torch.equal(g2, g) and torch.equal(du2, du)


def test_recompute_kernels_reject_bad_arguments(dev):
    """the argument checks of the one-output siblings, before any launch: DWM_EINVAL (-1) for a null pointer, n % 8 != 0, an unknown
    activation, inner % 8 != 0 or a leading dimension below the row; DWM_EALIGN (-2) for a pointer or a leading dimension off 16 bytes"""
    from opendwm_amd import _lib, ops, train_ops as T
    lib = _lib.load()
    null = ctypes.c_void_p(None)
    x, dy, y, dx = (torch.zeros(64, device=dev, dtype=bf16) for _ in range(4))
    p = lambda t: t.data_ptr()
    fa, code = lib.dwm_act_bwd_recompute, ops.ACT_GELU_TANH
    assert fa(p(x), p(dy), p(y), p(dx), 12, code, None) == -1
    assert fa(p(x), p(dy), p(y), p(dx), 0, code, None) == -1
    assert fa(p(x), p(dy), p(y), p(dx), 64, 99, None) == -1
    for i in range(4):
        ptrs = [p(x), p(dy), p(y), p(dx)]
        ptrs[i] = null
        assert fa(*ptrs, 64, code, None) == -1
        ptrs[i] = p((x, dy, y, dx)[i]) + 2
        assert fa(*ptrs, 32, code, None) == -2
    with pytest.raises(RuntimeError, match="DWM_EINVAL"):
        T.act_bwd_recompute(x[:12], dy[:12], code)
    with pytest.raises(RuntimeError, match="DWM_EALIGN"):
        T.act_bwd_recompute(x[1:33], dy[:32], code)
    fg = lib.dwm_geglu_bwd_recompute
    u, du = torch.zeros(4, 32, device=dev, dtype=bf16), torch.zeros(4, 32, device=dev, dtype=bf16)
    dg, g = torch.zeros(4, 16, device=dev, dtype=bf16), torch.zeros(4, 16, device=dev, dtype=bf16)
    ok = [p(u), 32, p(dg), 16, 4, 16, p(g), 16, p(du), 32]

    def call(**over):
        names = ["u", "ldu", "dg", "lddg", "rows", "inner", "g", "ldg", "du", "lddu"]
        a = list(ok)
        for k, v in over.items():
            a[names.index(k)] = v
        return fg(*a, None)
    for k in ("u", "dg", "g", "du"):
        assert call(**{k: null}) == -1
        assert call(**{k: ok[["u", "ldu", "dg", "lddg", "rows", "inner", "g", "ldg", "du", "lddu"].index(k)] + 2}) == -2
    assert call(rows=0) == -1 and call(inner=12) == -1 and call(inner=0) == -1
    assert call(ldu=24) == -1 and call(lddg=8) == -1 and call(ldg=8) == -1 and call(lddu=24) == -1
    assert call(ldu=36) == -2 and call(lddg=20) == -2 and call(ldg=20) == -2 and call(lddu=36) == -2
    assert call(rows=2, ldu=40, lddg=24, ldg=24, lddu=40) == 0             # wider rows within the buffers: accepted
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ blocks
# D = 128 (two heads of 64), 3 images of 24 tokens (4 x 6), 10 context tokens
D, HEADS, IMGS, GH, GW, LC = 128, 2, 3, 4, 6, 10
NTOK = GH * GW


def _held_bytes(out: torch.Tensor) -> int:
    """bytes the autograd context behind `out` holds (every saved tensor once)"""
    seen, total = set(), 0
    for t in out.grad_fn.saved_tensors:
        if t is not None and t.data_ptr() not in seen:
            seen.add(t.data_ptr())
            total += t.numel() * t.element_size()
    return total


EXTRA_RUNS = 6


@contextlib.contextmanager
def _idle_device_before_training_kernels():
    """every train_ops launch waits for the device to drain first: the workgroups of a kernel then start on an idle device instead of
    beside the tail of the launch before, which changes where they are placed and with it the order of their atomics"""
    from opendwm_amd import train_ops as T
    c0 = T._call

    def call(name, *args):
        torch.cuda.synchronize()
        return c0(name, *args)
    T._call = call
    try:
        yield
    finally:
        T._call = c0


@contextlib.contextmanager
def _other_state(fn_name, i):
    """a recompute run in another memory and cache state: a live allocation whose size depends on i makes the allocator hand the run
    other addresses, for even i the caches are evicted between the recomputed forward and the backward walk (train.<fn_name>,
    which the recomputing backward calls after its training forward, first rewrites 1 GiB), and for i % 3 == 2 every training kernel
    starts on an idle device"""
    from opendwm_amd import train
    f0 = getattr(train, fn_name)
    shift = torch.empty(512 * (2 * i + 3) + 8 * i, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(2 ** 28, dtype=torch.float32, device="cuda") if i % 2 == 0 else None

    def walk(*a, **kw):
        if scratch is not None:
            scratch.fill_(1.0)
        return f0(*a, **kw)
    setattr(train, fn_name, walk)
    try:
        with (_idle_device_before_training_kernels() if i % 3 == 2 else contextlib.nullcontext()):
            yield
    finally:
        setattr(train, fn_name, f0)
        del shift


def _compare_keep_with_recompute(name, r1, r2, k, rerun, alpha_index=None, abs_terms=None, rerun_keep=None):
    """r1, r2: the gradients of two recompute runs (the second in another state, _other_state), k: those of the keep run,
    rerun(i): one more recompute run in state i.
    A gradient that the recompute runs reproduce bit for bit must be bit-identical on the keep path; the others are finished by fp32
    atomics and meet the per-kernel tolerance of their dtype (fp32 reductions TOL_REDUCE, bf16 outputs TOL_KERNEL), d(alpha) - one
    cancelling fp32 sum - the kernel's own bound of test_segsum_diff_kernel_exact_on_its_own_inputs (2e-6 of the sum of the absolute
    terms, for each of the two values compared).
    Two runs alone do not tell the classes apart on this hardware: which of the racing waves reaches an atomic first follows the
    addresses and the cache state of its operands, so a sum whose order is not fixed still comes out the same in two like runs and one
    ulp off in the keep run, whose operands lie elsewhere and were written a forward earlier (norm_added_q.weight of the dual block:
    equal in the first two runs, 5.5e-8 off with the activations kept; pos_embed.proj.bias between three runs of the default trainer).
    So a gradient that agrees in the first two runs and differs on the keep path counts as atomics-finished only if one of
    EXTRA_RUNS further recompute runs, each in another state, gives other bits than the first, or - the order noise can sit on the
    keep side alone - one of EXTRA_RUNS further keep runs in other states gives exactly the recompute bits, which a different
    computation would not; a gradient that neither moves is computed differently on the keep path, and the test fails."""
    assert len(r1) == len(r2) == len(k)
    exact, loose, extra, again = 0, [], [], []
    for i, (a, b, c) in enumerate(zip(r1, r2, k)):
        assert (a is None) == (c is None), (name, i)
        if a is None:
            continue
        assert a.shape == c.shape and a.dtype == c.dtype and bool(torch.isfinite(c.float()).all()), (name, i)
        reproduced = torch.equal(a, b)
        if reproduced and not torch.equal(a, c):
            if not extra:
                extra.extend(rerun(j) for j in range(EXTRA_RUNS))
            reproduced = all(torch.equal(a, e[i]) for e in extra)
            if reproduced and rerun_keep is not None:     # no recompute run moves it: then some keep run in another state must hit its bits
                if not again:
                    again.extend(rerun_keep(j) for j in range(EXTRA_RUNS))
                reproduced = not any(torch.equal(a, e[i]) for e in again)
            assert not reproduced, (name, i, rel_err(c, a))          # the keep path computes something else
        if reproduced:
            exact += 1
        elif i == alpha_index:
            loose.append((i, float((a.double() - c.double()).abs().max()) / abs_terms))
            assert float((a.double() - c.double()).abs().max()) <= 2 * 2e-6 * abs_terms, (name, i, loose[-1])
        else:
            loose.append((i, rel_err(c, a)))
            assert loose[-1][1] < (TOL_REDUCE if a.dtype == torch.float32 else TOL_KERNEL), (name, loose[-1])
    n = exact + len(loose)
    _log("keep_vs_recompute", case=name, tensors=n, bit_identical=exact, share=exact / n, others=loose, extra_runs=len(extra))
    assert exact >= 0.8 * n, (name, exact, n)               # a condition of the design, not a measurement


def _init_block(blk, dev, seed):
    torch.manual_seed(seed)
    for n, p in blk.named_parameters():
        with torch.no_grad():
            if p.dim() == 1 and "norm" in n:
                p.copy_(1.0 + 0.2 * torch.randn(p.shape))
            elif p.dim() == 1:
                p.copy_(0.1 * torch.randn(p.shape))
            else:
                p.copy_(torch.randn(p.shape) * p.shape[-1] ** -0.5)
    return blk.to(dev).train()


@pytest.mark.parametrize("kind", ["plain", "dual", "context_pre_only", "plain_frozen"])
def test_joint_block_keep_equals_recompute(dev, kind):
    from opendwm_amd import train
    from opendwm_amd.blocks import STORE, JointTransformerBlock
    STORE.set_precision(bf16)
    pre, dual = kind == "context_pre_only", kind == "dual"
    blk = _init_block(JointTransformerBlock(D, HEADS, 64, context_pre_only=pre, qk_norm="rms_norm", use_dual_attention=dual), dev, 3)
    if kind == "plain_frozen":          # frozen second linears / projections: their operands are not re-derived at all
        for lin in (blk.ff.net[2], blk.ff_context.net[0].proj, blk.attn.to_q, blk.attn.to_k, blk.attn.to_v):
            lin.weight.requires_grad_(False)
    h, c, st = _rand((IMGS * NTOK, D), dev, 1), _rand((IMGS * LC, D), dev, 2), _rand((IMGS, D), dev, 3, 0.5)
    dh, dc = _rand((IMGS * NTOK, D), dev, 4), _rand((IMGS * LC, D), dev, 5)
    params = [p for p in blk.parameters() if p.requires_grad]

    def run(keep):
        ins = [t.clone().requires_grad_(True) for t in (h, c, st)]
        h_out, c_out = train.joint_block_train(blk, *ins, IMGS, keep=keep)
        held = _held_bytes(h_out)
        outs, gouts = ([h_out], [dh]) if pre else ([h_out, c_out], [dh, dc])
        grads = torch.autograd.grad(outs, ins + params, gouts, allow_unused=True)
        return [h_out.detach()] + ([] if pre else [c_out.detach()]) + list(grads), held
    def rerun(i):
        with _other_state("joint_block_backward_kept", i):
            return run(False)[0][n_out:]
    n_out = 1 if pre else 2
    r1, held_rec = run(False)
    r2 = [r1[j] for j in range(n_out)] + rerun(0)
    k, held_keep = run(True)
    want = train.joint_kept_bytes(blk, h, c, IMGS)
    assert held_keep == want and held_rec == 2 * (h.numel() + c.numel() + st.numel())
    # the block outputs come from different kernels (fused inference path / un-fused training forward): same values to one rounding
    for a, b in zip(r1[:n_out], k[:n_out]):
        assert rel_err(b, a) < TOL_KERNEL
    def rerun_keep(i):
        with _other_state("joint_block_backward_kept", i):
            return run(True)[0][n_out:]
    _compare_keep_with_recompute("joint_" + kind, r1[n_out:], r2[n_out:], k[n_out:], rerun, rerun_keep=rerun_keep)
    assert all(g is not None for g in k[n_out:n_out + 3])            # dh, dc, dst


@pytest.mark.parametrize("kind", ["temporal_rowwise", "temporal_pointwise", "temporal_full", "crossview_rowwise"])
def test_vt_block_keep_equals_recompute(dev, kind):
    from oracle import ctsd_oracle as O
    from opendwm_amd import ops, train
    from opendwm_amd.blocks import STORE, VTSelfAttentionBlock
    STORE.set_precision(bf16)
    blk = _init_block(VTSelfAttentionBlock(D, D, HEADS, 64, qk_norm="rms_norm"), dev, 5)
    B, Tn, V = (1, 1, IMGS) if kind.startswith("crossview") else (1, IMGS, 1)
    rm = getattr(ops, "rowmap_" + kind)(B, Tn, V, GH, GW)
    gmask = None
    if kind.startswith("crossview"):             # the cross-view group mask: view 0 does not see view 2
        gmask = O.ring_crossview_mask(B, V).to(dev)
        gmask[0, 0, 2] = False
    R = IMGS * NTOK
    h, emb, dy = _rand((R, D), dev, 1), _rand((IMGS, D), dev, 2, 0.5), _rand((R, D), dev, 3)
    alpha = torch.tensor([0.3], device=dev)
    params = [p for p in blk.parameters() if p.requires_grad]

    def run(keep):
        ins = [h.clone().requires_grad_(True), emb.clone().requires_grad_(True), alpha.clone().requires_grad_(True)]
        out = train.vt_block_train(blk, ins[0], rm, ins[1], NTOK, ins[2], R, group_mask=gmask, keep=keep)
        held = _held_bytes(out)
        with capture_segsum_diff() as calls:
            grads = torch.autograd.grad([out], ins + params, [dy], allow_unused=True)
        assert len(calls) == 1
        return [out.detach()] + list(grads), held, calls[0]["abs"]
    def rerun(i):
        with _other_state("vt_block_backward_kept", i):
            return run(False)[0][1:]
    r1, held_rec, abs1 = run(False)
    r2 = rerun(0)
    k, held_keep, _ = run(True)
    assert held_keep == train.vt_kept_bytes(blk, h, rm, emb, alpha) and held_rec == 2 * (h.numel() + emb.numel()) + 4
    assert rel_err(k[0], r1[0]) < TOL_KERNEL
    def rerun_keep(i):
        with _other_state("vt_block_backward_kept", i):
            return run(True)[0][1:]
    _compare_keep_with_recompute("vt_" + kind, r1[1:], r2, k[1:], rerun, alpha_index=2, abs_terms=abs1, rerun_keep=rerun_keep)
    assert all(g is not None for g in k[1:4])                        # dh, demb, dalpha


def test_blocks_keep_nothing_without_autograd(dev):
    """under no_grad the keep flag is ignored: the fused forward runs and no context is built"""
    from opendwm_amd import train
    from opendwm_amd.blocks import STORE, JointTransformerBlock
    STORE.set_precision(bf16)
    blk = _init_block(JointTransformerBlock(D, HEADS, 64, qk_norm="rms_norm"), dev, 3)
    h, c, st = _rand((IMGS * NTOK, D), dev, 1), _rand((IMGS * LC, D), dev, 2), _rand((IMGS, D), dev, 3, 0.5)
    with torch.no_grad():
        a, _ = train.joint_block_train(blk, h, c, st, IMGS, keep=True)
        b, _ = train.joint_block_train(blk, h, c, st, IMGS, keep=False)
    assert a.grad_fn is None and torch.equal(a, b)


# ------------------------------------------------------------------------------------------ model
class _Case:
    """the small full-graph configuration of test_model_gradients_vs_oracle with its fp32 oracle gradients, computed once per
    temporal attention type and shared (read-only) by the tests below"""
    cache = {}

    def __init__(self, tt, dev):
        from oracle import ctsd_oracle as O
        self.cfg = small_config(temporal_attention_type=tt)
        self.sd = {k: v.to(bf16).float() for k, v in O.make_state_dict(self.cfg, 0).items()}
        inp = small_inputs(self.cfg, 0)
        self.inp = {k: (v.to(bf16).float() if v.is_floating_point() and k not in ("timestep", "added_time_ids") else v)
                    for k, v in inp.items()}
        self.di = to_dev(self.inp, dev)
        self.wgt = torch.randn(self.inp["sample"].shape, generator=torch.Generator(device="cpu").manual_seed(11)).to(dev)
        self.ref, self.gref = _oracle_grads(self.sd, self.cfg, self.di, self.wgt, dev)

    @classmethod
    def get(cls, tt, dev):
        if tt not in cls.cache:
            cls.cache[tt] = cls(tt, dev)
        return cls.cache[tt]

    def forward(self, m):
        from opendwm_amd import train
        kw = dict(self.di)
        return train.forward_train(m, kw.pop("sample"), kw.pop("timestep"), kw.pop("encoder_hidden_states"),
                                   kw.pop("pooled_projections"), crossview_attention_mask=kw.get("crossview_attention_mask"),
                                   added_time_ids=kw.get("added_time_ids"))

    def errors(self, m):
        """(forward error, global gradient error) of one forward + backward of m against the oracle, as
        test_model_gradients_vs_oracle measures them"""
        out = self.forward(m)
        e_fwd = rel_err(out, self.ref)
        (out.float() * self.wgt).sum().backward()
        num = den = 0.0
        for name, p in m.named_parameters():
            if name not in self.gref or self.gref[name] is None:
                continue
            assert p.grad is not None, name
            a, b = p.grad.double().cpu(), self.gref[name].double().cpu()
            num += float((a - b).pow(2).sum())
            den += float(b.pow(2).sum())
        return e_fwd, (num / den) ** 0.5


def _family(name):
    return "joint" if name.startswith("transformer_blocks.") else name.split("_")[0]


@pytest.mark.parametrize("tt", ["rowwise", "pointwise"])
def test_model_keep_gradients_vs_oracle(dev, tt):
    case = _Case.get(tt, dev)
    m = _train_model(case.cfg, case.sd, dev)
    m.activation_policy = "keep"
    e_fwd, glob = case.errors(m)
    plan = m.activation_plan
    _log("model_gradients_keep", temporal=tt, fwd=e_fwd, global_rel=glob, kept_bytes=plan.total_bytes, blocks=len(plan))
    assert len(plan) == 4 + 1 + 2 and all(b[1] == "keep" and b[2] > 0 for b in plan.blocks)
    assert plan.total_bytes == sum(b[2] for b in plan.blocks)
    assert e_fwd < 2e-2 and glob < 3e-2, (e_fwd, glob)


def test_model_config_policy_keeps_the_families_whose_switch_is_off(dev):
    case = _Case.get("rowwise", dev)
    m = _train_model(case.cfg, case.sd, dev)
    m.activation_policy = "config"
    for gcp, tgc, cgc in ((False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        m.gradient_checkpointing, m.temporal_gradient_checkpointing, m.crossview_gradient_checkpointing = gcp, tgc, cgc
        case.forward(m)
        off = dict(joint=not gcp, temporal=not tgc, crossview=not cgc)
        plan = m.activation_plan
        assert sorted({_family(b[0]) for b in plan.blocks}) == ["crossview", "joint", "temporal"]
        for name, what, nbytes in plan.blocks:
            assert what == ("keep" if off[_family(name)] else "recompute"), (name, what, (gcp, tgc, cgc))
            assert (nbytes > 0) == (what == "keep")


def _trainer_inputs(case, dev):
    inp = dict(case.inp)
    lat = inp.pop("sample").to(dev)
    inp.pop("timestep")
    noise = torch.randn(lat.shape, generator=torch.Generator().manual_seed(5))
    return lat, to_dev(inp, dev), torch.tensor([250, 800]), noise


def test_trainer_budget_zero_equals_default_trainer(dev):
    """budget 0: the plan is all "recompute" and one train_step (a micro-step of gradient accumulation, so the gradients stay)
    gives the loss and gradients of a trainer built without the new arguments - bit-identical where default runs are, within
    the global bound of test_model_gradients_vs_oracle (3e-2) per parameter otherwise"""
    from opendwm_amd.pipeline import CTSDTrainer
    case = _Case.get("rowwise", dev)
    lat, di, idx, noise = _trainer_inputs(case, dev)
    def step(**kw):
        from opendwm_amd.blocks import STORE
        STORE.bump()
        m = _train_model(case.cfg, case.sd, dev)
        tr = CTSDTrainer(m, lr=2e-4, weight_decay=0.0, training_config={"gradient_accumulation_steps": 2}, **kw)
        loss = tr.train_step(lat, di, timestep_indices=idx, noise=noise).item()
        return loss, {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}, tr.activation_plan
    (l1, g1, p1), (l2, g2, _), (l3, g3, p3) = step(), step(), step(activations="keep", activation_budget_gib=0)
    assert [b[1] for b in p3.blocks] == ["recompute"] * len(p3) and p3.total_bytes == 0 and len(p3) == 7
    assert [b[1] for b in p1.blocks] == ["recompute"] * 7 and [b[0] for b in p1.blocks] == [b[0] for b in p3.blocks]
    assert l1 == l2 == l3 and set(g1) == set(g3) and len(g1) > 100
    exact, extra, again = 0, [], []
    for n in g1:
        reproduced = torch.equal(g1[n], g2[n])
        if reproduced and not torch.equal(g1[n], g3[n]):       # (see _compare_keep_with_recompute: two like runs can agree on an atomic sum)
            if not extra:
                for i in range(EXTRA_RUNS):                    # default trainers in other states: other addresses, an idle device
                    shift = torch.empty(512 * (2 * i + 3), dtype=torch.uint8, device=dev)
                    with (_idle_device_before_training_kernels() if i % 2 else contextlib.nullcontext()):
                        extra.append(step()[1])
                    del shift
            reproduced = all(torch.equal(g1[n], e[n]) for e in extra)
            if reproduced:           # no default run moves it: the order noise may sit on the other side - some budget-0 run must hit the bits
                if not again:
                    for i in range(EXTRA_RUNS):
                        shift = torch.empty(512 * (2 * i + 3), dtype=torch.uint8, device=dev)
                        with (_idle_device_before_training_kernels() if i % 2 else contextlib.nullcontext()):
                            again.append(step(activations="keep", activation_budget_gib=0)[1])
                        del shift
                reproduced = not any(torch.equal(g1[n], e[n]) for e in again)
            assert not reproduced, (n, rel_err(g3[n], g1[n]))
        if reproduced:
            exact += 1
        else:
            assert rel_err(g3[n], g1[n]) < 3e-2, n
    _log("budget_zero_equals_default", params=len(g1), bit_identical=exact, extra_runs=len(extra), extra_budget_zero_runs=len(again))


def test_model_half_budget_gives_a_mixed_plan_within_the_bounds(dev):
    case = _Case.get("rowwise", dev)
    m = _train_model(case.cfg, case.sd, dev)
    m.activation_policy = "keep"
    case.forward(m)
    full = m.activation_plan
    m.activation_budget_gib = full.total_bytes / 2 / 2 ** 30
    e_fwd, glob = case.errors(m)
    plan = m.activation_plan
    kinds = [b[1] for b in plan.blocks]
    _log("model_gradients_half_budget", fwd=e_fwd, global_rel=glob, plan=plan.blocks, full=full.total_bytes)
    assert "keep" in kinds and "recompute" in kinds and 0 < plan.total_bytes <= full.total_bytes // 2
    for (name, what, nbytes), (_, _, fb) in zip(plan.blocks, full.blocks):
        assert nbytes == (fb if what == "keep" else 0), name
    assert e_fwd < 2e-2 and glob < 3e-2, (e_fwd, glob)


def test_keep_raises_the_peak_and_backward_releases_it(dev):
    """peak memory of a "keep" step exceeds that of a "recompute" step; after backward the allocation is back to within the kept-byte
    total of the recompute step's, and below the step's own peak"""
    case = _Case.get("rowwise", dev)
    m = _train_model(case.cfg, case.sd, dev)
    stats = {}
    for mode in ("recompute", "keep", "recompute", "keep"):            # the first round allocates gradients and weight copies
        m.activation_policy = mode
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        out = case.forward(m)
        held = torch.cuda.memory_allocated()
        (out.float() * case.wgt).sum().backward()
        del out
        torch.cuda.synchronize()
        stats[mode] = dict(peak=torch.cuda.max_memory_allocated(), held=held, after=torch.cuda.memory_allocated(),
                           kept=m.activation_plan.total_bytes)
    _log("keep_memory", **stats)
    kept = stats["keep"]["kept"]
    assert kept > 0 and stats["recompute"]["kept"] == 0
    assert stats["keep"]["peak"] > stats["recompute"]["peak"]
    assert stats["keep"]["held"] > stats["recompute"]["held"]
    assert stats["keep"]["after"] <= stats["recompute"]["after"] + kept and stats["keep"]["after"] < stats["keep"]["peak"]
    assert stats["keep"]["after"] < stats["keep"]["held"]


# ------------------------------------------------------------------------------------------ DDP
@pytest.fixture()
def rccl(dev):
    """a one-rank process group over RCCL on cuda:0 (the pattern of tests/test_rccl_gpu.py), torn down after the test"""
    import torch.distributed as dist
    torch.cuda.set_device(dev)
    assert not dist.is_initialized()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    yield dev
    dist.destroy_process_group()


def test_ddp_keep_with_gradient_accumulation_equals_plain(rccl):
    """CTSDTrainer(activations="keep", ddp=True) on a one-rank RCCL group with gradient_accumulation_steps = 2: the micro-step runs
    under no_sync, the optimizing step all-reduces the accumulated gradient; losses and parameters after the optimizing step equal
    the non-DDP keep run's within the bound of test_ddp_train_step_over_rccl_equals_plain_step"""
    from opendwm_amd.pipeline import CTSDTrainer
    dev = rccl
    case = _Case.get("rowwise", dev)
    lat, di, idx, noise = _trainer_inputs(case, dev)
    results = {}
    for name, ddp in (("plain", False), ("ddp", True)):
        m = _train_model(case.cfg, case.sd, dev)
        tr = CTSDTrainer(m, lr=2e-4, weight_decay=0.01, ddp=ddp, activations="keep",
                         training_config={"gradient_accumulation_steps": 2})
        losses = [tr.train_step(lat, di, timestep_indices=idx, noise=noise).item() for _ in range(2)]
        assert all(b[1] == "keep" for b in tr.activation_plan.blocks) and tr.activation_plan.total_bytes > 0
        results[name] = (losses, {n: p.detach().clone() for n, p in m.named_parameters()})
        del tr, m
    (lp, pp), (ld, pd) = results["plain"], results["ddp"]
    assert any(not torch.equal(pp[n], case.sd[n].to(dev)) for n in pp)          # the optimizing step happened
    diff = [n for n in pp if not torch.equal(pp[n], pd[n])]
    worst = max(((pp[n].double() - pd[n].double()).norm() / pp[n].double().norm().clamp_min(1e-30)).item() for n in pp)
    _log("ddp_keep_one_rank", losses_plain=lp, losses_ddp=ld, params=len(pp), params_different=len(diff), worst_rel=worst)
    assert lp == ld and len(diff) <= len(pp) // 4 and worst < 1e-6, (diff[:5], worst)
