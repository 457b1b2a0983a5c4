"""GPU leg (`-m gpu`) of the order-deterministic training mode (include/dwm_hip.h "Ordered reductions").

Inside train_ops.ordered_reductions(True) the five gradient reductions that finish with fp32 atomics by default write per-chunk
partials and fold them in ascending chunk order, so every output is a function of the input values, the shapes and the library build.
Checked here: each op at the smallest shapes that have every seam (against fp64, against the default op, over perturbed device states,
against the documented fold re-done in torch on the returned partials), the launch census of a train step in both modes, keep against
recompute per block kind - every gradient bit-equal - and whole train steps of the MMDiT and UNet trainers.

Inputs are bf16 normal data with each row scaled by 2^k, k uniform in [-8, 8] (K_RANGE), so that the order of fp32 additions shows in the
last bits of a column sum; the fp64 references hold TOL_REDUCE on them (rel_err is a Frobenius ratio, dominated by the large rows: an
fp32 accumulation error of ~1e-6 of the largest terms stays three orders below it; the range was not narrowed).
TOL_REDUCE / TOL_KERNEL live in tests/test_train_gpu.py (2e-3 / 6e-3), rel_err in tests/common.py."""
import collections
import contextlib
import os
import socket

import pytest
import torch
import torch.nn.functional as F

from tests.common import rel_err, to_dev
from tests.test_keep_activations_gpu import D, GH, GW, HEADS, IMGS, LC, NTOK, _Case, _init_block, _trainer_inputs
from tests.test_train_gpu import TOL_KERNEL, TOL_REDUCE, _log, _rand, _train_model  # noqa: F401  (TOL_KERNEL: the bf16 bound, for reference)

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16 = torch.bfloat16
K_RANGE = 8
STATES = 6
DEFAULT_SYMBOLS = ("dwm_segsum", "dwm_segsum_diff", "dwm_layernorm_bwd", "dwm_rmsnorm_heads_bwd", "dwm_groupnorm_bwd")


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


# ------------------------------------------------------------------------------------------ helpers
def _data(shape, dev, seed, scale=1.0):
    """bf16 normal data, each row scaled by 2^k with k uniform in [-K_RANGE, K_RANGE], from a seeded CPU generator"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(*shape, generator=g) * scale
    k = torch.randint(-K_RANGE, K_RANGE + 1, (shape[0], 1), generator=g)
    return (x * torch.exp2(k.float())).to(dev).to(bf16)


@contextlib.contextmanager
def _state(i):
    """perturbed device state i: a live allocation of 512 (2i + 3) + 8i bytes (operands get other addresses); even i: 1 GiB is
    rewritten right before the body (caches evicted); i % 3 == 2: the device is drained before every train_ops launch"""
    from opendwm_amd import train_ops as T
    shift = torch.empty(512 * (2 * i + 3) + 8 * i, dtype=torch.uint8, device="cuda")
    c0 = T._call

    def call(name, *args):
        torch.cuda.synchronize()
        return c0(name, *args)
    if i % 2 == 0:
        scratch = torch.empty(2 ** 28, dtype=torch.float32, device="cuda")
        scratch.fill_(float(i))
        del scratch
    if i % 3 == 2:
        T._call = call
    try:
        yield
    finally:
        T._call = c0
        del shift


def _same(a, b):
    assert len(a) == len(b)
    return all((x is None and y is None) or (x is not None and y is not None and x.dtype == y.dtype and torch.equal(x, y))
               for x, y in zip(a, b))


def _assert_repeatable(name, fn):
    """fn() -> list of tensors; the plain run and the runs in states 0 .. STATES - 1 are all torch.equal"""
    plain = fn()
    for i in range(STATES):
        with _state(i):
            r = fn()
        bad = [j for j, (x, y) in enumerate(zip(plain, r)) if not _same([x], [y])]
        assert not bad, (name, "state", i, "tensors", bad)
    return plain


def _fold(p, dim):
    """the documented stage 2 in torch fp32: a plain left fold over ascending index of `dim`"""
    t = p.select(dim, 0).clone()
    for k in range(1, p.shape[dim]):
        t = t + p.select(dim, k)
    return t


def _poison(n, dev):
    """leave n floats of NaN in the caching allocator: the next torch.empty of that size finds them (the workspace comes uninitialised)"""
    t = torch.full((n,), float("nan"), dtype=torch.float32, device=dev)
    del t


@contextlib.contextmanager
def _short_workspace(how):
    """every dwm_*_ordered launch through train_ops._call is handed a workspace one float too small / a null workspace"""
    from opendwm_amd import train_ops as T
    c0 = T._call

    def call(name, *args):
        if name.endswith("_ordered"):
            args = (*args[:-1], args[-1] - 1) if how == "small" else (*args[:-2], None, args[-1])
        return c0(name, *args)
    T._call = call
    try:
        yield
    finally:
        T._call = c0


def _check_op(name, dev, call, out_shapes, refs, fold):
    """call(outs, return_partials) -> (other outputs, partials) runs the op in the mode of the moment, accumulating into the fp32
    tensors `outs`; refs: fp64 references of the reductions; fold(partials) -> the totals stage 2 adds to outs.  Points (a) - (f)
    of the per-op contract."""
    from opendwm_amd import train_ops as T
    zeros = lambda: [torch.zeros(s, dtype=torch.float32, device=dev) for s in out_shapes]
    d_outs = zeros()
    d_others, d_parts = call(d_outs, True)
    assert d_parts is None                                            # outside the scope: the default symbols, no partials
    with T.ordered_reductions(True):
        o_outs = zeros()
        o_others, parts = call(o_outs, True)
        assert parts is not None and parts.dtype == torch.float32
        n_ws = parts.numel()
        # (a) fp64 and the default op
        errs = {}
        for j, (o, d, r) in enumerate(zip(o_outs, d_outs, refs)):
            errs[j] = (rel_err(o, r), rel_err(o, d))
            assert errs[j][0] < TOL_REDUCE and errs[j][1] < TOL_REDUCE, (name, j, errs[j])
        # (b) everything that is not a reduction
        assert _same(o_others, d_others), name
        # (c) + (d) the op and its partials repeat over the device states, on a workspace that starts as NaN
        def run():
            _poison(n_ws, dev)
            outs = zeros()
            others, p = call(outs, True)
            return outs + list(others) + [p]
        plain = _assert_repeatable(name, run)
        assert _same(plain[:len(o_outs)], o_outs) and _same([plain[-1]], [parts]) and bool(torch.isfinite(parts).all()), name
        # (d) out = prior contents + the documented fold of the partials, bit for bit
        pre = [torch.randn(s, generator=torch.Generator().manual_seed(40 + j)).to(dev) for j, s in enumerate(out_shapes)]
        outs = [p.clone() for p in pre]
        _, p2 = call(outs, True)
        assert torch.equal(p2, parts), name
        totals = fold(p2)
        for j, (o, p, t) in enumerate(zip(outs, pre, totals)):
            assert torch.equal(o, p + t.view(p.shape)), (name, "fold", j, rel_err(o, p + t.view(p.shape)))
        # (e) accumulate onto the zero-start result: exactly s + s
        outs = [s.clone() for s in o_outs]
        call(outs, False)
        for j, (o, s) in enumerate(zip(outs, o_outs)):
            assert torch.equal(o, s + s), (name, "accumulate", j)
        # (f) a too-small or null workspace is refused before any launch
        for how in ("small", "null"):
            with _short_workspace(how), pytest.raises(RuntimeError, match="DWM_EINVAL"):
                call(zeros(), False)
        torch.cuda.synchronize()
    _log("ordered_" + name, errs=errs, workspace_floats=n_ws)


# ------------------------------------------------------------------------------------------ 1. the five ops
def _seg_inputs(case, dev):
    if case == "strided":
        mk = lambda s: _data((1000, 264), dev, s)[:, :256]
        rpg = None
    elif case == "129x8":
        mk = lambda s: _data((129, 8), dev, s)
        rpg = None
    else:
        mk = lambda s: _data((1001, 1536), dev, s)
        rpg = 154 if case == "1001x1536_rpg154" else None
    return mk(3), mk(4), mk(5), rpg


def _group_sums(t, rpg):
    rows = t.shape[0]
    rpg = rows if rpg is None else rpg
    return torch.stack([t[g * rpg:(g + 1) * rpg].sum(0) for g in range((rows + rpg - 1) // rpg)])


@pytest.mark.parametrize("case", ["1001x1536_rpg154", "129x8", "strided", "1001x1536_none"])
@pytest.mark.parametrize("op", ["segsum", "segsum_b", "segsum_diff"])
def test_segsum_ordered(dev, op, case):
    """chunks of 128 rows: (1001, 1536) in groups of 154 = 7 groups of 128 + 26 rows, the last group 77 rows and an EMPTY second chunk;
    (129, 8) = two chunks and one part-filled column block; a strided view; one group of all rows (8 chunks)"""
    from opendwm_amd import train_ops as T
    a, b, b2, rpg = _seg_inputs(case, dev)
    rows, ncols = a.shape
    if op == "segsum":
        ref = _group_sums(a.double(), rpg)
        call = lambda outs, rp: ((), T.segsum(a, rows_per_group=rpg, out=outs[0], return_partials=True)[1])
    elif op == "segsum_b":
        ref = _group_sums(a.double() * b.double(), rpg)
        call = lambda outs, rp: ((), T.segsum(a, b, rows_per_group=rpg, out=outs[0], return_partials=True)[1])
    else:
        ref = _group_sums(a.double() * (b.double() - b2.double()), rpg)
        call = lambda outs, rp: ((), T.segsum_diff(a, b, b2, rows_per_group=rpg, out=outs[0], return_partials=True)[1])
    groups = ref.shape[0]
    with T.ordered_reductions(True):
        p = call([torch.zeros(groups, ncols, device=dev)], True)[1]
    assert p.shape == (groups, (min(rpg or rows, rows) + 127) // 128, ncols)
    _check_op(f"{op}_{case}", dev, call, [(groups, ncols)], [ref], lambda parts: [_fold(parts, 1)])
    if op == "segsum":                                                   # the allocating forms return what the accumulating ones add
        with T.ordered_reductions(True):
            s = T.segsum(a, rows_per_group=rpg)
            assert rel_err(s, ref) < TOL_REDUCE and torch.equal(s, T.segsum(a, rows_per_group=rpg, out=torch.zeros_like(s)))


@pytest.mark.parametrize("D_,mode", [(1536, "mod"), (1536, "mod2"), (1536, "affine"), (1536, "affine_add"), (320, "affine")])
def test_layernorm_bwd_ordered(dev, D_, mode):
    """the five cases of test_layernorm_bwd: I = 5 groups of N = 77 rows = chunks of 64 + 13 per group (per-group modulation
    gradients) or 7 chunks of all 385 rows (affine gradients, folded into row 0); D = 320 = the ragged 512-column pass, 1536 = NI 3"""
    from opendwm_amd import train_ops as T
    I, N = 5, 77
    rows = I * N
    x, dy, dy2 = _data((rows, D_), dev, 1, 1.5), _data((rows, D_), dev, 2), _data((rows, D_), dev, 3)
    idx = torch.arange(rows, device=dev) // N
    xr = x.double().requires_grad_(True)
    if mode in ("mod", "mod2"):
        two = mode == "mod2"
        sc, sc2 = _rand((I, D_), dev, 4, 0.3), _rand((I, D_), dev, 6, 0.3)
        scr, shr, sc2r, sh2r = (t.double().requires_grad_(True) for t in (sc, torch.zeros_like(sc), sc2, torch.zeros_like(sc2)))
        xh = F.layer_norm(xr, (D_,), eps=1e-6)
        loss = ((xh * (1 + scr[idx]) + shr[idx]) * dy.double()).sum()
        if two:
            loss = loss + ((xh * (1 + sc2r[idx]) + sh2r[idx]) * dy2.double()).sum()
        loss.backward()
        refs = [scr.grad, shr.grad] + ([sc2r.grad, sh2r.grad] if two else [])
        shapes = [(I, D_)] * len(refs)

        def call(outs, rp):
            g = list(outs) + [None] * (4 - len(outs))
            dx, p = T.layernorm_bwd(x, dy, eps=1e-6, scale=sc, scale2=sc2 if two else None, rows_per_mod=N, dy2=dy2 if two else None,
                                    dgamma=g[0], dbeta=g[1], dgamma2=g[2], dbeta2=g[3], grad_per_group=True, return_partials=True)
            return [dx], p
        fold = lambda parts: [_fold(parts[s], 1) for s in range(parts.shape[0])]
        pshape = (len(refs), I, 2, D_)
    else:
        w, b = _rand((D_,), dev, 4, 0.2) + 1, _rand((D_,), dev, 5, 0.2)
        wr, br = w.double().requires_grad_(True), b.double().requires_grad_(True)
        emb = _rand((I, D_), dev, 6) if mode == "affine_add" else None
        xin = xr
        if emb is not None:
            ssum = xr + emb.double()[idx]
            xin = ssum.detach().to(bf16).double() + (ssum - ssum.detach())    # the forward rounds the sum to bf16 (straight-through)
        (F.layer_norm(xin, (D_,), wr, br, eps=1e-5) * dy.double()).sum().backward()
        refs, shapes = [wr.grad.view(1, D_), br.grad.view(1, D_)], [(1, D_), (1, D_)]
        pre = _rand((rows, D_), dev, 8)

        def call(outs, rp):
            dx = pre.clone()
            _, p = T.layernorm_bwd(x, dy, eps=1e-5, dx=dx, accumulate=True, weight=w, addvec=emb, rows_per_add=N, dgamma=outs[0],
                                   dbeta=outs[1], return_partials=True)
            return [dx], p
        fold = lambda parts: [_fold(parts[s].reshape(-1, D_), 0) for s in range(parts.shape[0])]
        pshape = (2, 1, 7, D_)
    with T.ordered_reductions(True):
        p = call([torch.zeros(s, device=dev) for s in shapes], True)[1]
    assert p.shape == pshape
    _check_op(f"layernorm_bwd_{D_}_{mode}", dev, call, shapes, refs, fold)


def test_layernorm_bwd_ordered_without_accumulators(dev):
    """no accumulator, no workspace: dx alone, bit-equal to the default kernel's"""
    from opendwm_amd import train_ops as T
    x, dy = _data((200, 512), dev, 1), _data((200, 512), dev, 2)
    d = T.layernorm_bwd(x, dy, eps=1e-6)
    with T.ordered_reductions(True):
        o, p = T.layernorm_bwd(x, dy, eps=1e-6, return_partials=True)
    assert p is None and torch.equal(o, d)


@pytest.mark.parametrize("rows,heads", [(333, 24), (37, 64)])
def test_rmsnorm_heads_bwd_ordered(dev, rows, heads):
    """rows = 333 = 10 chunks of 32 + 13, ncols = 3072 (six passes of 512 columns), y and dy strided views; dw against the fp64 sum of
    the kernel's own inputs dy * (y / w).  (37, 64 heads): ncols = 8192 = two column tiles of the ordered kernel's LDS rows (4096 each),
    a second chunk of 5 rows in which three of the four waves get one row or none"""
    from opendwm_amd import train_ops as T
    ncols = 2 * heads * 64
    y = _data((rows, ncols + 64), dev, 1, 1.3)[:, :ncols].clone()
    dy0 = _data((rows, ncols + 64), dev, 2)
    w = torch.cat([(_rand((64,), dev, 3, 0.2) + 1).repeat(heads), (_rand((64,), dev, 4, 0.2) + 1).repeat(heads)]).contiguous()
    ybuf = torch.zeros(rows, ncols + 64, dtype=bf16, device=dev)
    yv = ybuf[:, :ncols]
    yv.copy_(y)
    rinv = T.rmsnorm_heads_train_(yv, w, 1e-6)                            # in place: yv = xhat * w
    ref = (dy0[:, :ncols].double() * (yv.double() / w.double())).sum(0)

    def call(outs, rp):
        d = dy0.clone()[:, :ncols]                                        # in place on dy (-> dx), a strided view
        assert d.stride(0) == ncols + 64 and yv.stride(0) == ncols + 64
        dx, p = T.rmsnorm_heads_bwd_(yv, rinv, w, d, outs[0], return_partials=True)
        return [dx], p
    with T.ordered_reductions(True):
        p = call([torch.zeros(ncols, device=dev)], True)[1]
    assert p.shape == ((rows + 31) // 32, ncols)
    _check_op(f"rmsnorm_heads_bwd_{rows}x{ncols}", dev, call, [(ncols,)], [ref], lambda parts: [_fold(parts, 0)])


@pytest.mark.parametrize("C,silu,mode", [(320, True, "plain"), (128, True, "padded"), (640, False, "plain"), (256, True, "temporal"),
                                         (1920, True, "plain")])
def test_groupnorm_bwd_ordered(dev, C, silu, mode):
    """the grid of test_groupnorm_bwd at its shapes: 12 images of 48 pixels = one chunk per image, or (temporal) 4 images of 144
    pixels = chunks of 64 + 64 + 16; the fold runs over all image x chunk blocks, image-major.  dx and the accumulate form bit-equal."""
    from opendwm_amd import ops, train_ops as T
    from opendwm_amd.ops import PaddedGrid
    B, Tn, V, h, w = 2, 3, 2, 6, 8
    I, N = B * Tn * V, h * w
    x, dz = _data((I * N, C), dev, 1), _data((I * N, C), dev, 2)
    gamma, beta = (_rand((C,), dev, 3) * 0.2 + 1), _rand((C,), dev, 4, 0.2)
    xr = x.double().requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    if mode == "temporal":
        x5 = xr.view(B, Tn, V, N, C).permute(0, 2, 4, 1, 3).reshape(B * V, C, Tn, N)
        yy = F.group_norm(x5, 32, gr, br, 1e-5)
        yy = (F.silu(yy) if silu else yy).view(B, V, C, Tn, N).permute(0, 3, 1, 4, 2).reshape(I * N, C)
        kw, Ii, Pp, chunks = dict(img_map=(V, N, Tn * V * N, N, V * N)), B * V, Tn * N, 3
    else:
        yy = F.group_norm(xr.view(I, N, C).transpose(1, 2), 32, gr, br, 1e-5)
        yy = (F.silu(yy) if silu else yy).transpose(1, 2).reshape(I * N, C)
        kw, Ii, Pp, chunks = {}, I, N, 1
    (yy * dz.double()).sum().backward()
    grid = PaddedGrid(I, h, w) if mode == "padded" else None
    dzk = ops.pad_tokens(dz, grid) if mode == "padded" else dz
    base = _rand((I * N, C), dev, 9)

    def call(outs, rp):
        dx, p = T.groupnorm_bwd(x, dzk, Ii, Pp, gamma, beta, 32, 1e-5, outs[0], outs[1], silu=silu, dz_grid=grid, return_partials=True, **kw)
        dx2 = base.clone()                                                # the accumulate form, into throw-away accumulators
        T.groupnorm_bwd(x, dzk, Ii, Pp, gamma, beta, 32, 1e-5, torch.zeros_like(outs[0]), torch.zeros_like(outs[1]), silu=silu, dx=dx2,
                        accumulate=True, dz_grid=grid, **kw)
        return [dx, dx2], p
    with T.ordered_reductions(True):
        p = call([torch.zeros(C, device=dev), torch.zeros(C, device=dev)], True)[1]
    assert p.shape == (Ii, chunks, 2, C)
    fold = lambda parts: [_fold(parts.reshape(-1, 2, C)[:, 0], 0), _fold(parts.reshape(-1, 2, C)[:, 1], 0)]
    _check_op(f"groupnorm_bwd_{C}_{mode}", dev, call, [(C,), (C,)], [gr.grad, br.grad], fold)


# ------------------------------------------------------------------------------------------ 2. launch census
@contextlib.contextmanager
def _census():
    from opendwm_amd import train_ops as T
    names, c0 = [], T._call

    def call(name, *args):
        names.append(name)
        return c0(name, *args)
    T._call = call
    try:
        yield names
    finally:
        T._call = c0


def _unet_case(dev):
    from oracle import unet_oracle as U
    from tests.test_unet_train_gpu import _small_unet_cfg
    cfg = _small_unet_cfg()
    sd = {k: v.to(bf16).float() for k, v in U.make_unet_state_dict(cfg, 0).items()}
    inp = U.make_unet_inputs(cfg, 2, 2, 3, 8, 16, text_len=10)
    cond = to_dev({k: v for k, v in inp.items() if k not in ("sample", "timesteps")}, dev)
    lat = torch.randn(2, 2, 3, 4, 8, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    noise = torch.randn(lat.shape, generator=torch.Generator().manual_seed(5))
    return cfg, sd, lat, cond, torch.tensor([250, 800]), noise


def _make_trainer(kind, dev, case, **kw):
    from opendwm_amd.blocks import STORE
    from opendwm_amd.pipeline import CTSDTrainer
    STORE.bump()
    if kind == "unet":
        from tests.test_unet_train_gpu import _unet_model
        m = _unet_model(case[0], case[1], dev)
    else:
        m = _train_model(case.cfg, case.sd, dev)
    return m, CTSDTrainer(m, lr=2e-4, weight_decay=0.01, **kw)


def _step_inputs(kind, dev, case):
    return case[2:] if kind == "unet" else _trainer_inputs(case, dev)


@pytest.mark.parametrize("kind", ["mmdit", "unet"])
def test_launch_census(dev, kind):
    """deterministic=False launches exactly the symbols of a trainer built without the argument, none of them *_ordered;
    deterministic=True launches none of the five default reductions (and does launch their ordered forms)"""
    case = _unet_case(dev) if kind == "unet" else _Case.get("rowwise", dev)
    lat, cond, idx, noise = _step_inputs(kind, dev, case)
    seen = {}
    for name, kw in (("absent", {}), ("off", dict(deterministic=False)), ("on", dict(deterministic=True))):
        m, tr = _make_trainer(kind, dev, case, **kw)
        with _census() as names:
            tr.train_step(lat, cond, timestep_indices=idx, noise=noise)
        torch.cuda.synchronize()
        seen[name] = collections.Counter(names)
        assert getattr(m, "ordered_reductions") is (name == "on")
        assert "ordered_reductions" not in m.state_dict() and not any("ordered" in k for k in m.state_dict())
        del tr, m
    assert seen["off"] == seen["absent"] and not any(n.endswith("_ordered") for n in seen["off"])
    assert not any(n in seen["on"] for n in DEFAULT_SYMBOLS), {n: seen["on"][n] for n in DEFAULT_SYMBOLS}
    for n in DEFAULT_SYMBOLS:                                  # each reduction of the default step has its ordered launch, one for one
        assert seen["on"][n + "_ordered"] == seen["off"][n], n
    other = lambda c: {n: k for n, k in c.items() if not n.endswith("_ordered") and n not in DEFAULT_SYMBOLS}
    assert other(seen["on"]) == other(seen["off"])
    used = [n for n in DEFAULT_SYMBOLS if seen["off"][n]]
    _log("ordered_census", kind=kind, reductions={n: seen["off"][n] for n in used})
    assert "dwm_segsum" in used and "dwm_layernorm_bwd" in used and ("dwm_groupnorm_bwd" if kind == "unet" else "dwm_rmsnorm_heads_bwd") in used


# ------------------------------------------------------------------------------------------ 3. blocks
@pytest.mark.parametrize("kind", ["plain", "dual", "context_pre_only"])
def test_joint_block_keep_equals_recompute_bitwise(dev, kind):
    """inside the scope EVERY gradient of a kept joint block equals the recomputing block's bit for bit, and both repeat over the
    device states"""
    from opendwm_amd import train, train_ops as T
    from opendwm_amd.blocks import STORE, JointTransformerBlock
    STORE.set_precision(bf16)
    pre, dual = kind == "context_pre_only", kind == "dual"
    blk = _init_block(JointTransformerBlock(D, HEADS, 64, context_pre_only=pre, qk_norm="rms_norm", use_dual_attention=dual), dev, 3)
    h, c, st = _data((IMGS * NTOK, D), dev, 1), _data((IMGS * LC, D), dev, 2), _rand((IMGS, D), dev, 3, 0.5)
    dh, dc = _data((IMGS * NTOK, D), dev, 4), _data((IMGS * LC, D), dev, 5)
    params = [p for p in blk.parameters() if p.requires_grad]

    def run(keep):
        ins = [t.clone().requires_grad_(True) for t in (h, c, st)]
        h_out, c_out = train.joint_block_train(blk, *ins, IMGS, keep=keep)
        outs, gouts = ([h_out], [dh]) if pre else ([h_out, c_out], [dh, dc])
        return list(torch.autograd.grad(outs, ins + params, gouts, allow_unused=True))
    with T.ordered_reductions(True), _census() as names:
        rec = _assert_repeatable("joint_recompute_" + kind, lambda: run(False))
        kept = _assert_repeatable("joint_keep_" + kind, lambda: run(True))
    assert any(n.endswith("_ordered") for n in names) and not any(n in DEFAULT_SYMBOLS for n in names)
    bad = [i for i, (a, b) in enumerate(zip(rec, kept)) if not _same([a], [b])]
    _log("ordered_keep_vs_recompute", case="joint_" + kind, tensors=sum(g is not None for g in rec), different=bad)
    assert not bad and all(g is not None for g in kept[:3]), bad


@pytest.mark.parametrize("kind", ["temporal_rowwise", "crossview_rowwise"])
def test_vt_block_keep_equals_recompute_bitwise(dev, kind):
    from oracle import ctsd_oracle as O
    from opendwm_amd import ops, train, train_ops as T
    from opendwm_amd.blocks import STORE, VTSelfAttentionBlock
    STORE.set_precision(bf16)
    blk = _init_block(VTSelfAttentionBlock(D, D, HEADS, 64, qk_norm="rms_norm"), dev, 5)
    B, Tn, V = (1, 1, IMGS) if kind.startswith("crossview") else (1, IMGS, 1)
    rm = getattr(ops, "rowmap_" + kind)(B, Tn, V, GH, GW)
    gmask = None
    if kind.startswith("crossview"):
        gmask = O.ring_crossview_mask(B, V).to(dev)
        gmask[0, 0, 2] = False
    R = IMGS * NTOK
    h, emb, dy = _data((R, D), dev, 1), _rand((IMGS, D), dev, 2, 0.5), _data((R, D), dev, 3)
    alpha = torch.tensor([0.3], device=dev)
    params = [p for p in blk.parameters() if p.requires_grad]

    def run(keep):
        ins = [h.clone().requires_grad_(True), emb.clone().requires_grad_(True), alpha.clone().requires_grad_(True)]
        out = train.vt_block_train(blk, ins[0], rm, ins[1], NTOK, ins[2], R, group_mask=gmask, keep=keep)
        return list(torch.autograd.grad([out], ins + params, [dy], allow_unused=True))
    with T.ordered_reductions(True), _census() as names:
        rec = _assert_repeatable("vt_recompute_" + kind, lambda: run(False))
        kept = _assert_repeatable("vt_keep_" + kind, lambda: run(True))
    assert "dwm_segsum_diff_ordered" in names and not any(n in DEFAULT_SYMBOLS for n in names)
    bad = [i for i, (a, b) in enumerate(zip(rec, kept)) if not _same([a], [b])]
    _log("ordered_keep_vs_recompute", case="vt_" + kind, tensors=sum(g is not None for g in rec), different=bad)
    assert not bad and all(g is not None for g in kept[:3]), bad


# ------------------------------------------------------------------------------------------ 4. trainers
def _two_steps(kind, dev, case, **kw):
    """(losses, parameters, optimizer state tensors) after two train_steps of a fresh trainer on fixed timestep indices and noise"""
    lat, cond, idx, noise = _step_inputs(kind, dev, case)
    m, tr = _make_trainer(kind, dev, case, **kw)
    losses = [tr.train_step(lat, cond, timestep_indices=idx, noise=noise).item() for _ in range(2)]
    params = {n: p.detach().clone() for n, p in m.named_parameters()}
    state = {}
    for i, st in tr.optimizer.state_dict()["state"].items():
        for k, v in st.items():
            if torch.is_tensor(v):
                state[f"{i}.{k}"] = v.detach().clone()
    torch.cuda.synchronize()
    return losses, params, state


def _assert_same_run(name, r1, r2, sd=None):
    (l1, p1, s1), (l2, p2, s2) = r1, r2
    assert l1 == l2, (name, l1, l2)
    assert set(p1) == set(p2) and set(s1) == set(s2) and len(s1) > 0
    dp = [n for n in p1 if not torch.equal(p1[n], p2[n])]
    ds = [n for n in s1 if not torch.equal(s1[n], s2[n])]
    _log("ordered_trainer", case=name, losses=l1, params=len(p1), params_different=len(dp), state_tensors=len(s1), state_different=len(ds))
    assert not dp and not ds, (name, dp[:5], ds[:5])
    if sd is not None:
        assert any(not torch.equal(p1[n].cpu(), sd[n]) for n in p1), name              # the optimizing steps happened


@pytest.mark.parametrize("opts", ["fp32_torch", "8bit_fused"])
def test_mmdit_trainer_steps_are_bit_reproducible(dev, opts):
    """two fresh CTSDTrainer(deterministic=True) from one state dict, the second in perturbed state 2: equal losses, parameters and
    optimizer moments after two steps - also with the 8-bit optimizer and the fused gradient conditioning (clip at 1.0) together"""
    case = _Case.get("rowwise", dev)
    kw = dict(deterministic=True)
    if opts == "8bit_fused":
        kw.update(optimizer_bits=8, grad_conditioning="fused", max_grad_norm=1.0)
    r1 = _two_steps("mmdit", dev, case, **kw)
    with _state(2):
        r2 = _two_steps("mmdit", dev, case, **kw)
    _assert_same_run("mmdit_" + opts, r1, r2, case.sd)


def test_unet_trainer_steps_are_bit_reproducible(dev):
    case = _unet_case(dev)
    r1 = _two_steps("unet", dev, case, deterministic=True)
    with _state(2):
        r2 = _two_steps("unet", dev, case, deterministic=True)
    _assert_same_run("unet", r1, r2, case[1])


def test_ddp_one_rank_equals_plain_bitwise(rccl):
    """plain against ddp=True on a one-rank RCCL group, both deterministic: every parameter (240 in the small configuration) equal"""
    dev = rccl
    case = _Case.get("rowwise", dev)
    r1 = _two_steps("mmdit", dev, case, deterministic=True)
    r2 = _two_steps("mmdit", dev, case, deterministic=True, ddp=True)
    assert len(r1[1]) == 240
    _assert_same_run("mmdit_ddp_one_rank", r1, r2, case.sd)


def test_model_gradients_vs_oracle_in_deterministic_mode(dev):
    """the fp32-oracle gradient check of the small configuration (test_model_gradients_vs_oracle: forward < 2e-2, global gradient
    error < 3e-2; 8e-3-class as measured) with the ordered reductions"""
    case = _Case.get("rowwise", dev)
    m = _train_model(case.cfg, case.sd, dev)
    m.ordered_reductions = True
    with _census() as names:
        e_fwd, glob = case.errors(m)
    _log("model_gradients_deterministic", fwd=e_fwd, global_rel=glob)
    assert any(n.endswith("_ordered") for n in names) and not any(n in DEFAULT_SYMBOLS for n in names)
    assert e_fwd < 2e-2 and glob < 3e-2, (e_fwd, glob)
