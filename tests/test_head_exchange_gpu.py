"""GPU leg of the frame shard's HEAD exchange (opendwm_amd.sharding, `CTSDDenoiser(frame_exchange="heads")`): the pack / unpack
kernel dwm_head_exchange against torch.permute bit for bit, the attention kernels on the received layout through the exchanged row
maps against an fp64 softmax, and the whole denoise loop of a "full" temporal-attention model on two ranks (gloo, both on the
one GPU) and on a one-rank RCCL group against the single-process run.  The host half is tests/test_head_exchange_cpu.py."""
import os
import socket

import pytest
import torch

from oracle import ctsd_oracle as O
from tests.common import rel_err, small_config, small_inputs, to_dev
from tests.test_fp32_gpu import TOL_F32, _fp32_model
from tests.test_hip_gpu import TOL_KERNEL, _bf16_round_sd, _hip_model, _log, _random_cameras      # _log: the suite's parity log

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
f32 = torch.float32
TOL_SHARD = 5e-3        # test_frame_shard_two_ranks: bf16 round-off of differently shaped launches


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ 1. the copy kernel
GUARD = 4096            # bytes of sentinel on both sides of every output


def _guarded(numel, dtype, dev, fill):
    """(whole buffer, the `numel` elements in its middle): GUARD bytes of `fill` on both sides"""
    pad = GUARD // torch.empty((), dtype=dtype).element_size()
    buf = torch.full((numel + 2 * pad,), fill, dtype=dtype, device=dev)
    return buf, buf[pad:pad + numel], pad


def _guards_intact(buf, pad, fill):
    return bool((buf[:pad] == fill).all()) and bool((buf[-pad:] == fill).all())


def _source(shape, dtype, dev, seed):
    """distinct, exactly representable values would not survive bf16: random bits are enough for an equality test of a copy"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g).to(dtype).to(dev)


@pytest.mark.parametrize("dtype", [bf16, f32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("S,R,Dr", [(3, 2, 64), (1, 3, 64), (3, 8, 192), (1, 1, 128)])
def test_head_exchange_matches_torch_permute(dev, dtype, S, R, Dr):
    """split: [row][s][j][Dr] -> [j][row][s][Dr]; merge: the way back - torch.equal with the torch permute for one row, an odd row
    count and several workgroups, the guard bytes around every output untouched"""
    from opendwm_amd import ops
    fill = -7.0
    for rows in (1, 37, 256):
        x = _source((rows, S, R, Dr), dtype, dev, rows)
        buf, out, pad = _guarded(x.numel(), dtype, dev, fill)
        ops.head_exchange(x.view(rows, S * R * Dr), out, rows, S, R, Dr)
        want = x.permute(2, 0, 1, 3).contiguous()
        assert torch.equal(out.view(R, rows, S, Dr), want) and _guards_intact(buf, pad, fill), ("split", rows)
        buf2, back, pad = _guarded(x.numel(), dtype, dev, fill)
        ops.head_exchange(want, back.view(rows, S * R * Dr), rows, S, R, Dr, merge=True)
        assert torch.equal(back.view(rows, S, R, Dr), x) and _guards_intact(buf2, pad, fill), ("merge", rows)


@pytest.mark.parametrize("dtype", [bf16, f32], ids=["bf16", "fp32"])
def test_head_exchange_column_slice_of_a_wider_buffer(dev, dtype):
    """the row-major side as a column slice (ld > S * R * Dr): the fused q | k | v buffer of a joint block, say.  The merge must leave
    every column outside the slice as it was."""
    from opendwm_amd import ops
    rows, S, R, Dr, fill = 37, 3, 2, 64, -7.0
    n, lead, ld = S * R * Dr, 64, S * R * Dr + 64 + 40
    wide = _source((rows, ld), dtype, dev, 5)
    x = wide[:, lead:lead + n]
    buf, out, pad = _guarded(rows * n, dtype, dev, fill)
    ops.head_exchange(x, out, rows, S, R, Dr)
    want = x.reshape(rows, S, R, Dr).permute(2, 0, 1, 3).contiguous()
    assert torch.equal(out.view(R, rows, S, Dr), want) and _guards_intact(buf, pad, fill)
    buf2, w2, pad = _guarded(rows * ld, dtype, dev, fill)
    w2 = w2.view(rows, ld)
    ops.head_exchange(want, w2[:, lead:lead + n], rows, S, R, Dr, merge=True)
    assert torch.equal(w2[:, lead:lead + n], x) and _guards_intact(buf2, pad, fill)
    assert bool((w2[:, :lead] == fill).all()) and bool((w2[:, lead + n:] == fill).all())


def test_head_exchange_more_passes_than_workgroups(dev):
    """above 4096 x 16 KiB the capped grid strides over the buffer, and the last pass is a partial one: 7300 rows of the UniMLVG
    q | k | v row at R = 8 (67 MB) - the only size at which a workgroup takes a second pass"""
    from opendwm_amd import ops
    rows, S, R, Dr, fill = 7300, 3, 8, 192, -7.0
    assert rows * S * R * Dr * 2 // 16 > 4096 * 1024 and (rows * S * R * Dr * 2 // 16) % 1024 != 0
    x = _source((rows, S, R, Dr), bf16, dev, 9)
    buf, out, pad = _guarded(x.numel(), bf16, dev, fill)
    ops.head_exchange(x.view(rows, S * R * Dr), out, rows, S, R, Dr)
    want = x.permute(2, 0, 1, 3).contiguous()
    assert torch.equal(out.view(R, rows, S, Dr), want) and _guards_intact(buf, pad, fill)
    buf2, back, pad = _guarded(x.numel(), bf16, dev, fill)
    ops.head_exchange(want, back.view(rows, S * R * Dr), rows, S, R, Dr, merge=True)
    assert torch.equal(back.view(rows, S, R, Dr), x) and _guards_intact(buf2, pad, fill)


def test_head_exchange_rejects_bad_arguments(dev):
    import ctypes
    from opendwm_amd import _lib, ops
    a = torch.zeros(4, 3 * 2 * 60, device=dev, dtype=bf16)
    with pytest.raises(RuntimeError, match="DWM_EALIGN"):
        ops.head_exchange(a, torch.zeros(a.numel(), device=dev, dtype=bf16), 4, 3, 2, 60)             # 120-byte runs
    b = torch.zeros(4, 3 * 2 * 64, device=dev, dtype=bf16)
    with pytest.raises(RuntimeError):
        ops.head_exchange(b, torch.zeros(b.numel() - 8, device=dev, dtype=bf16), 4, 3, 2, 64)         # sizes differ
    with pytest.raises(RuntimeError):
        ops.head_exchange(b, torch.zeros(b.numel(), device=dev, dtype=f32), 4, 3, 2, 64)              # dtypes differ
    with pytest.raises(RuntimeError):
        ops.head_exchange(b.t(), torch.zeros(b.numel(), device=dev, dtype=bf16), 4, 3, 2, 64)         # rows not contiguous
    with pytest.raises(RuntimeError):
        ops.head_exchange(b.cpu(), b.cpu().reshape(-1), 4, 3, 2, 64)                                  # no CPU fallback
    fn = _lib.load().dwm_head_exchange
    null = ctypes.c_void_p(None)
    assert fn(null, b.data_ptr(), 4, 3, 2, 64, 2, 384, 0, None) == -1                                 # DWM_EINVAL
    assert fn(b.data_ptr(), null, 4, 3, 2, 64, 2, 384, 1, None) == -1
    assert fn(b.data_ptr(), b.data_ptr(), 0, 3, 2, 64, 2, 384, 0, None) == -1
    assert fn(b.data_ptr() + 2, b.data_ptr(), 4, 3, 2, 64, 2, 384, 0, None) == -2                     # DWM_EALIGN


# ------------------------------------------------------------------------------------------ 2. attention on the received layout
@pytest.mark.parametrize("kind", ["full", "rowwise"])
@pytest.mark.parametrize("h,w", [(8, 6), (8, 24)], ids=["8x6", "8x24"])
def test_attention_on_the_exchanged_layout(dev, kind, h, w):
    """one process, 4 heads, two emulated ranks: the receive buffer of rank 0 is built with ops.head_exchange from both ranks' fused
    q | k | v, ops.attention runs on it with the exchanged map on 2 heads - "full": L = 192 (a resident kernel) and 768 (the tiled
    one), row-wise: L = 24 and 96 - and every (problem, token, head) must equal an fp64 softmax of the same bf16 inputs"""
    from opendwm_amd import ops
    B, T, V, heads, R = 2, 4, 3, 4, 2
    N, D, Tl = h * w, heads * 64, T // R
    Dr, rows = D // R, B * Tl * V * N
    g = torch.Generator().manual_seed(31)
    whole = torch.randn(B, T, V, N, 3 * D, generator=g).to(bf16)                      # the unsharded fused projection, rows (b, t, v, n)
    sends = []
    for r in range(R):
        mine = whole[:, r * Tl:(r + 1) * Tl].reshape(rows, 3 * D).contiguous().to(dev)
        sends.append(ops.head_exchange(mine, torch.empty(R, rows, 3, Dr, dtype=bf16, device=dev), rows, 3, R, Dr))
    rank = 0
    rx = torch.cat([s[rank] for s in sends]).view(R * rows, 3 * Dr)                    # what the all-to-all hands rank 0: [src i][rows][3][Dr]
    mk = ops.rowmap_temporal_full_exchanged if kind == "full" else ops.rowmap_temporal_rowwise_exchanged
    rm = mk(B, Tl, R, V, h, w)
    ox = torch.zeros(R * rows, Dr, dtype=bf16, device=dev)
    ops.attention(rx[:, :Dr], rx[:, Dr:2 * Dr], rx[:, 2 * Dr:], ox, rm, heads // R)
    # fp64 reference on the CPU from the unsharded tensor: rank 0's heads, the reference's own rearrange
    x = whole.double().view(B, T, V, h, w, 3, heads, 64)[..., rank * (heads // R):(rank + 1) * (heads // R), :]
    if kind == "full":
        x = x.permute(0, 2, 5, 6, 1, 3, 4, 7).reshape(B * V, 3, heads // R, T * N, 64)                 # (b v) s head (t h w) d
    else:
        x = x.permute(0, 2, 3, 5, 6, 1, 4, 7).reshape(B * V * h, 3, heads // R, T * w, 64)             # (b v h) s head (t w) d
    q, k, v = x[:, 0], x[:, 1], x[:, 2]
    ref = torch.softmax(q @ k.transpose(-1, -2) * 64 ** -0.5, -1) @ v                                  # [P, heads / R, L, 64]
    ref = ref.transpose(1, 2).reshape(rm.n_problems, rm.L0, Dr)
    got = ox.cpu()[rm.rows()]
    e = rel_err(got, ref)
    worst = (got.double() - ref).abs().max().item()
    _log("attention_exchanged", kind=kind, h=h, w=w, L=rm.L0, rel=e, max_abs=worst)
    assert got.shape == ref.shape and e < TOL_KERNEL, e


# ------------------------------------------------------------------------------------------ 3.-6. the whole loop on two ranks
def _scenarios():
    """name -> dict(cfg, sd, lat, cond, kw, fp32, exchange): built alike (seeded) by the test process and by both ranks"""
    out = {}
    lat = torch.randn(1, 4, 3, 16, 8, 12, generator=torch.Generator().manual_seed(13))
    img = torch.randn(1, 4, 3, 16, 8, 12, generator=torch.Generator().manual_seed(14))

    def conds(cfg, explicit=False):
        inp = small_inputs(cfg, 0, T=4)
        if explicit:
            inp.pop("added_time_ids")
        cond = {k: v for k, v in inp.items() if k not in ("sample", "timestep")}
        if explicit:
            K, M = _random_cameras(1, 4, 3, 21)
            cond["camera_intrinsics_norm"] = torch.cat([K, K])                     # CFG-doubled, as every other condition
            cond["camera2referego"] = torch.cat([M, M])
        return cond
    cfg = small_config(temporal_attention_type="full")                             # 2 heads: one per rank
    sd = _bf16_round_sd(O.make_state_dict(cfg, 0))
    out["full"] = dict(cfg=cfg, sd=sd, lat=lat, cond=conds(cfg), kw={}, fp32=False, exchange="heads", refusal=True)
    out["full_reference_frames"] = dict(cfg=cfg, sd=sd, lat=lat, cond=conds(cfg), kw=dict(image_latents=img, reference_frame_count=1),
                                        fp32=False, exchange="heads")
    cfg = small_config(perspective_modeling_type="explicit", temporal_attention_type="full")
    out["full_explicit"] = dict(cfg=cfg, sd=_bf16_round_sd(O.make_state_dict(cfg, 0)), lat=lat, cond=conds(cfg, True), kw={}, fp32=False,
                                exchange="heads")
    cfg = small_config(temporal_attention_type="rowwise")
    out["rowwise_heads"] = dict(cfg=cfg, sd=_bf16_round_sd(O.make_state_dict(cfg, 0)), lat=lat, cond=conds(cfg), kw={}, fp32=False,
                                exchange="heads")
    cfg = small_config(temporal_attention_type="full")
    out["full_fp32"] = dict(cfg=cfg, sd=O.make_state_dict(cfg, 0), lat=lat, cond=conds(cfg), kw={}, fp32=True, exchange="auto")
    return out


def _denoise(s, dev, **group_kw):
    from opendwm_amd.pipeline import CTSDDenoiser
    m = (_fp32_model if s["fp32"] else _hip_model)(s["cfg"], s["sd"], dev)
    den = CTSDDenoiser(m, guidance_scale=4.0, inference_steps=4, **group_kw)
    kw = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in s["kw"].items()}
    return den.run(s["lat"].to(dev), to_dev(s["cond"], dev), stop=None if s["fp32"] else 3, **kw).cpu()


def _two_rank_worker(rank, world, port, path):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    res = {}
    for name, s in _scenarios().items():
        if s.get("refusal"):                    # the row exchange still refuses "full" (before any collective: both ranks raise alike)
            try:
                _denoise(s, dev, frame_group=dist.group.WORLD)
                res[name + "/refused"] = False
            except NotImplementedError:
                res[name + "/refused"] = True
        res[name] = _denoise(s, dev, frame_group=dist.group.WORLD, frame_exchange=s["exchange"])
    torch.save(res, f"{path}.{rank}")
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def two_ranks(dev):
    """ONE spawn of two ranks (gloo, both on the one GPU) that runs every scenario: rank -> {scenario: latents of the whole sample}"""
    import tempfile
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = 29500 + (os.getpid() + 29) % 2000
    path = os.path.join(tempfile.mkdtemp(), "head_exchange")
    procs = [ctx.Process(target=_two_rank_worker, args=(r, 2, port, path)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    return torch.load(path + ".0"), torch.load(path + ".1")


@pytest.fixture(scope="module")
def scenarios():
    return _scenarios()


def _check_against_single(name, two_ranks, scenarios, dev):
    a, b = two_ranks[0][name], two_ranks[1][name]
    single = _denoise(scenarios[name], dev)
    e = rel_err(a, single)
    _log("head_exchange_two_ranks", scenario=name, ranks_equal=bool(torch.equal(a, b)), rel_vs_single=e)
    assert a.shape == single.shape and torch.equal(a, b) and e < TOL_SHARD, e


@pytest.mark.parametrize("mode", ["full", "full_reference_frames"])
def test_head_exchange_two_ranks_full_attention(dev, two_ranks, scenarios, mode):
    """the 4 frames of one sample of a "full" temporal-attention model on two ranks, one head each: q | k | v out and the attention
    output back around the attention of every temporal block, everything else on the rank's own frames.  Both ranks bit-identical,
    within bf16 round-off of the single-process run; without frame_exchange the construction is refused as before."""
    _check_against_single(mode, two_ranks, scenarios, dev)
    assert two_ranks[0]["full/refused"] and two_ranks[1]["full/refused"]


def test_head_exchange_two_ranks_explicit_perspective(dev, two_ranks, scenarios):
    """perspective_modeling_type="explicit": on this path the temporal blocks stay on the rank's own frames, so their per-token ray
    embedding comes from the local camera matrices - no gather"""
    _check_against_single("full_explicit", two_ranks, scenarios, dev)


def test_head_exchange_two_ranks_rowwise_forced(dev, two_ranks, scenarios):
    """row-wise temporal attention with the head exchange forced (what lifts the height % R condition)"""
    _check_against_single("rowwise_heads", two_ranks, scenarios, dev)


def test_head_exchange_two_ranks_fp32_vs_cpu_oracle(dev, two_ranks, scenarios):
    """compute_dtype = float32: fp32 q | k | v and attention output through the same kernel (4-byte elements), "auto" choosing the
    heads for "full"; the whole guided loop within the mode's tolerance of the CPU oracle's unsharded one"""
    s = scenarios["full_fp32"]
    a, b = two_ranks[0]["full_fp32"], two_ranks[1]["full_fp32"]
    ref = O.denoise(s["sd"], s["cfg"], s["lat"], s["cond"], steps=4, guidance_scale=4.0)
    e = rel_err(a, ref)
    _log("head_exchange_two_ranks_fp32", ranks_equal=bool(torch.equal(a, b)), rel_vs_oracle=e)
    assert a.dtype == f32 and a.shape == ref.shape and torch.equal(a, b) and e < TOL_F32, e


# ------------------------------------------------------------------------------------------ 7. RCCL
def _free_port() -> int:
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.fixture()
def rccl(dev):
    """a one-rank process group over RCCL on cuda:0 (tests/test_rccl_gpu.py), torn down after the test"""
    import torch.distributed as dist
    torch.cuda.set_device(dev)
    assert not dist.is_initialized()
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, device_id=dev)
    yield dev
    dist.destroy_process_group()


def test_head_exchange_over_rccl_equals_unsharded(rccl, scenarios):
    """FrameShard with R = 1 over RCCL and frame_exchange="heads": the new buffers go through the DEVICE all_to_all_single (four per
    temporal block), the attention through the exchanged map at Tl = T; one rank holds all frames and all heads, so the latents
    must equal the unsharded denoiser's (5e-3; the arithmetic is the same)"""
    import torch.distributed as dist
    from opendwm_amd import sharding
    dev, s = rccl, scenarios["full"]
    calls = {"n": 0}
    orig = sharding.dist.all_to_all_single

    def counting(*a, **k):
        assert a[0].is_cuda and a[1].is_cuda            # device tensors straight into RCCL: no host staging
        calls["n"] += 1
        return orig(*a, **k)
    sharding.dist.all_to_all_single = counting
    try:
        single = _denoise(s, dev)
        assert calls["n"] == 0
        sharded = _denoise(s, dev, frame_group=dist.group.WORLD, frame_exchange="heads")
    finally:
        sharding.dist.all_to_all_single = orig
    e = rel_err(sharded, single)
    n_temporal = len(s["cfg"]["temporal_block_layers"])
    _log("head_exchange_over_rccl_one_rank", all_to_all_calls=calls["n"], equal=bool(torch.equal(single, sharded)), rel=e)
    assert calls["n"] == 2 * n_temporal * 3 and e < TOL_SHARD, (calls["n"], e)        # 2 per block and forward, 3 steps
