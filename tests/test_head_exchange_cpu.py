"""Frame sharding through a HEAD exchange (opendwm_amd.sharding: FrameShard.plan / heads_gather / heads_scatter, the exchanged row
maps of opendwm_amd.ops) - the host half, over gloo on the CPU: the exchange itself, the row-map tables, a "full" temporal block +
mixer with its attention run per head group over the exchange against the unsharded block (the oracle is the row compute), and the
plan rules.  The device half is tests/test_head_exchange_gpu.py."""
import ctypes
import os
import socket

import pytest
import torch
import torch.multiprocessing as mp

from opendwm_amd import dist as D

# the geometry of every case here: T divides by 2 and 3, and so do the 6 heads
B, T, V, HEIGHT, WIDTH = 2, 6, 2, 2, 3
HEADS, HEAD_DIM = 6, 8


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _raises(fn):
    try:
        fn()
        return None
    except Exception as e:                  # noqa: BLE001  (the class name is what the test asserts on)
        return type(e).__name__


def _block_over_head_exchange(O, fs, sd, cfg, typ, h_loc, emb_loc, Tl, dis):
    """temporal block k = 0 + mixer on the rows [B * Tl * V * N, C] of this rank's frames, the leaves of oracle.vt_self_attention_block in
    its order - with the attention run on heads / R heads of ALL frames: heads_gather, problems and tokens through the exchanged
    row map, heads_scatter"""
    import torch.nn.functional as F
    from opendwm_amd import ops
    p, R = "temporal_transformer_blocks.0", fs.size
    N, C = HEIGHT * WIDTH, HEADS * HEAD_DIM
    rows = B * Tl * V * N
    x = (h_loc + emb_loc).reshape(rows, C)
    y = F.layer_norm(x, (C,), sd[p + ".norm_in.weight"], sd[p + ".norm_in.bias"], 1e-5)
    x = O.feed_forward(sd, p + ".ff_in", y, "geglu") + x
    y = F.layer_norm(x, (C,), sd[p + ".norm1.weight"], sd[p + ".norm1.bias"], 1e-5)
    q, k, v = (O.linear(sd, f"{p}.attn1.to_{n}", y) for n in "qkv")
    q = O.rms_norm(q.view(rows, HEADS, HEAD_DIM), sd[p + ".attn1.norm_q.weight"], 1e-5).reshape(rows, C)      # per head: travels with it
    k = O.rms_norm(k.view(rows, HEADS, HEAD_DIM), sd[p + ".attn1.norm_k.weight"], 1e-5).reshape(rows, C)
    wide = torch.zeros(rows, 3 * C + 5)                                            # the fused buffer as a column slice: strided rows
    qkv = wide[:, :3 * C]
    qkv.copy_(torch.cat([q, k, v], 1))
    rx = fs.heads_gather(qkv, rows, 3)                                             # [R * rows, q | k | v of my heads]
    Dr = C // R
    mk = ops.rowmap_temporal_full_exchanged if typ == "full" else ops.rowmap_temporal_rowwise_exchanged
    idx = mk(B, Tl, R, V, HEIGHT, WIDTH).rows()                                    # [problems, L] rows of the received buffer
    qh, kh, vh = (O._heads(rx[:, i * Dr:(i + 1) * Dr][idx], HEADS // R) for i in range(3))
    o = O._unheads(O.sdpa(qh, kh, vh))                                             # [problems, L, Dr]
    ox = torch.zeros(R * rows, Dr)
    ox[idx.reshape(-1)] = o.reshape(-1, Dr)
    a = O.linear(sd, p + ".attn1.to_out.0", fs.heads_scatter(ox, rows))
    x = a + x
    y = F.layer_norm(x, (C,), sd[p + ".norm3.weight"], sd[p + ".norm3.bias"], 1e-5)
    x = O.feed_forward(sd, p + ".ff", y, "geglu") + x
    return O.alpha_blender(sd, "time_mixers.0", h_loc.reshape(B, Tl * V, N, C), x.view(B, Tl * V, N, C), dis).flatten(0, 1)


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.set_num_threads(1)
    D.init("gloo")
    from opendwm_amd import ops
    from opendwm_amd.sharding import FrameShard
    from oracle import ctsd_oracle as O
    from tests.common import small_config
    fs = FrameShard(temporal_exchange="heads")
    R, N, C = world, HEIGHT * WIDTH, HEADS * HEAD_DIM
    Tl, Hr = T // R, HEADS // R
    Dr = Hr * HEAD_DIM
    t0, t1 = fs.frame_range(T)
    rows = B * Tl * V * N
    res = {}
    g = torch.Generator().manual_seed(0)

    # 1. the exchange itself
    full = torch.randn(B, T, V, N, 3, HEADS, HEAD_DIM, generator=g)
    mine = full[:, t0:t1].reshape(rows, 3 * C).contiguous()
    rx = fs.heads_gather(mine, rows, 3)
    my_heads = full[..., rank * Hr:(rank + 1) * Hr, :]                             # [B, T, V, N, 3, Hr, hd]: my heads of every frame
    want = my_heads.reshape(B, R, Tl, V, N, 3 * Dr).permute(1, 0, 2, 3, 4, 5).reshape(R * rows, 3 * Dr)      # rows (i, b, tl, v, n)
    res["gather_shape"] = tuple(rx.shape) == (R * rows, 3 * Dr)
    res["gather_ok"] = bool(torch.equal(rx, want))
    # ... in the order the exchanged row maps assume: (problem, token) of the map = the unsharded rearrange of the whole sample
    idx = ops.rowmap_temporal_full_exchanged(B, Tl, R, V, HEIGHT, WIDTH).rows()
    res["order_full"] = bool(torch.equal(rx[idx], my_heads.reshape(B, T, V, N, 3 * Dr).permute(0, 2, 1, 3, 4).reshape(B * V, T * N, 3 * Dr)))
    idx = ops.rowmap_temporal_rowwise_exchanged(B, Tl, R, V, HEIGHT, WIDTH).rows()
    res["order_rowwise"] = bool(torch.equal(rx[idx], my_heads.reshape(B, T, V, HEIGHT, WIDTH, 3 * Dr).permute(0, 2, 3, 1, 4, 5)
                                            .reshape(B * V * HEIGHT, T * WIDTH, 3 * Dr)))
    # heads_scatter of it is the identity: q | k | v go back one by one (S = 1) and land in a column slice of a wider buffer
    back = torch.zeros(rows, 3 * C + 7)
    for s in range(3):
        fs.heads_scatter(rx[:, s * Dr:(s + 1) * Dr].contiguous(), rows, out=back[:, s * C:(s + 1) * C])
    res["round_trip"] = bool(torch.equal(back[:, :3 * C], mine)) and bool((back[:, 3 * C:] == 0).all())
    res["scatter_alloc"] = bool(torch.equal(fs.heads_scatter(rx[:, :Dr].contiguous(), rows), mine[:, :C]))

    # 3. a temporal block + mixer over the exchange == the same block on the whole sample
    for typ in ("full", "rowwise"):
        cfg = small_config(temporal_attention_type=typ, num_attention_heads=HEADS, attention_head_dim=HEAD_DIM)
        sd = O.make_state_dict(cfg, 0)
        h = torch.randn(B * T * V, N, C, generator=g)
        emb = torch.randn(B * T * V, 1, C, generator=g) * 0.3
        dis = torch.tensor([False, True])
        whole = O.temporal_block_and_mix(sd, cfg, 0, h, emb, B, T, V, WIDTH, dis).view(B, T, V, N, C)
        out = _block_over_head_exchange(O, fs, sd, cfg, typ, h.view(B, T, V, N, C)[:, t0:t1], emb.view(B, T, V, 1, C)[:, t0:t1], Tl, dis)
        res["block_" + typ] = float((out.view(B, Tl, V, N, C) - whole[:, t0:t1]).abs().max())
        res["block_scale_" + typ] = float(whole.abs().max())

    # 4. plan
    rows_, heads_, auto_ = FrameShard(), fs, FrameShard(temporal_exchange="auto")
    res["plan"] = dict(
        default=rows_.temporal_exchange,
        rows_full=_raises(lambda: rows_.plan(R * 4, HEADS, "full")),
        rows_rowwise=rows_.plan(R * 4, HEADS, "rowwise"),
        rows_uneven=_raises(lambda: rows_.plan(R * 4 + 1, HEADS, "rowwise")),
        check_full=_raises(lambda: rows_.check(R * 4, "full")),
        auto_full=auto_.plan(R * 4, HEADS, "full"),
        auto_rowwise_even=auto_.plan(R * 4, HEADS, "rowwise"),
        auto_pointwise_even=auto_.plan(R * 4, HEADS, "pointwise"),
        auto_rowwise_16=auto_.plan(16, HEADS, "rowwise"),
        auto_pointwise_uneven=_raises(lambda: auto_.plan(R * 4 + 1, HEADS, "pointwise")),
        heads_full=heads_.plan(R * 4 + 1, HEADS, "full"),
        heads_rowwise=heads_.plan(R * 4, HEADS, "rowwise"),
        heads_pointwise=_raises(lambda: heads_.plan(R * 4, HEADS, "pointwise")),
        heads_uneven=_raises(lambda: heads_.plan(R * 4, HEADS + 1, "full")),
        auto_heads_uneven=_raises(lambda: auto_.plan(R * 4, HEADS + 1, "full")),
        bad_mode=_raises(lambda: FrameShard(temporal_exchange="views")),
    )
    q.put((rank, res))
    D.shutdown()


_RESULTS = {}


def _run(world):
    """one spawn per world size, shared by the tests below"""
    if world not in _RESULTS:
        port = _free_port()
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
        for p in procs:
            p.start()
        res = dict(q.get(timeout=300) for _ in procs)
        for p in procs:
            p.join(timeout=60)
            assert p.exitcode == 0
        _RESULTS[world] = res
    return _RESULTS[world]


@pytest.mark.parametrize("world", [2, 3])
def test_head_exchange_gather_and_scatter_gloo(world):
    """heads_gather leaves rank r with heads [r H/R, (r+1) H/R) of q, k and v of EVERY frame, rows ordered (source rank, b, tl, v, n)
    as the exchanged row maps assume; heads_scatter of it is the identity (torch.equal), also into a column slice"""
    res = _run(world)
    for r in range(world):
        for key in ("gather_shape", "gather_ok", "order_full", "order_rowwise", "round_trip", "scatter_alloc"):
            assert res[r][key], (r, key, res[r])


@pytest.mark.parametrize("R", [2, 3])
def test_exchanged_rowmaps_enumerate_the_unsharded_maps(R):
    """a pure table comparison: problem by problem and token by token the exchanged maps name, on rows ordered (i, b, tl, v, n), the
    same (b, t, v, n) as rowmap_temporal_full / rowmap_temporal_rowwise on the unsharded rows (b, t, v, n)"""
    from opendwm_amd import ops
    Tl, N = T // R, HEIGHT * WIDTH
    # received row -> unsharded row
    i, b, tl, v, n = torch.meshgrid(torch.arange(R), torch.arange(B), torch.arange(Tl), torch.arange(V), torch.arange(N), indexing="ij")
    to_unsharded = (((b * T + i * Tl + tl) * V + v) * N + n).reshape(-1)
    for mkx, mk in ((ops.rowmap_temporal_full_exchanged, ops.rowmap_temporal_full),
                    (ops.rowmap_temporal_rowwise_exchanged, ops.rowmap_temporal_rowwise)):
        rx, ru = mkx(B, Tl, R, V, HEIGHT, WIDTH), mk(B, T, V, HEIGHT, WIDTH)
        assert (rx.L0, rx.n_problems) == (ru.L0, ru.n_problems)
        got = rx.rows()
        assert got.shape == ru.rows().shape and got.min() == 0 and got.max() == R * B * Tl * V * N - 1
        assert got.reshape(-1).unique().numel() == got.numel()                    # every received row exactly once
        assert torch.equal(to_unsharded[got], ru.rows())


@pytest.mark.parametrize("world", [2, 3])
def test_temporal_block_over_head_exchange_gloo(world):
    """a "full" (and a row-wise) temporal block + mixer of the oracle on the whole sample against the same block on each rank's
    frames with its attention per head group over the exchange: 1e-5 absolute, as for the row exchange (fp32 oracle compute; only
    the summation order inside torch kernels may differ)"""
    res = _run(world)
    for r in range(world):
        assert res[r]["block_scale_full"] > 0.5 and res[r]["block_scale_rowwise"] > 0.5, res[r]          # (the bound means something)
        assert res[r]["block_full"] < 1e-5 and res[r]["block_rowwise"] < 1e-5, res[r]


def test_plan_rules():
    """FrameShard.plan: "rows" keeps today's rules and errors; "auto" takes rows where they serve and heads otherwise; "heads" serves
    full / rowwise, needs heads % R == 0 and refuses pointwise"""
    for world in (2, 3):
        for r, res in _run(world).items():
            p = res["plan"]
            assert p["default"] == "rows"
            assert p["rows_full"] == "NotImplementedError" and p["check_full"] == "NotImplementedError"
            assert p["rows_rowwise"] == "rows" and p["rows_uneven"] == "ValueError"
            assert p["auto_full"] == "heads"
            assert p["auto_rowwise_even"] == "rows" and p["auto_pointwise_even"] == "rows"
            assert p["auto_rowwise_16"] == ("rows" if world == 2 else "heads")       # 16 token rows do not split over 3 ranks
            assert p["auto_pointwise_uneven"] == "NotImplementedError"
            assert p["heads_full"] == "heads" and p["heads_rowwise"] == "heads"
            assert p["heads_pointwise"] == "NotImplementedError"
            assert p["heads_uneven"] == "ValueError" and p["auto_heads_uneven"] == "ValueError"
            assert p["bad_mode"] == "ValueError"


def test_denoiser_passes_the_exchange_on():
    from opendwm_amd.pipeline import CTSDDenoiser
    with pytest.raises(ValueError):
        CTSDDenoiser(torch.nn.Identity(), frame_exchange="heads")                 # no frame_group to exchange over
    assert CTSDDenoiser(torch.nn.Identity()).frame_shard is None


def test_head_exchange_entry_point_rejects_bad_arguments():
    """dwm_head_exchange returns before any launch: null pointers / non-positive sizes / a row stride below the row DWM_EINVAL (-1),
    a run or stride off the 16-byte grid or a misaligned pointer DWM_EALIGN (-2), 2^31 or more 16-byte pieces DWM_EUNSUPPORTED (-3)"""
    from opendwm_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    fn = lib.dwm_head_exchange
    fn.restype, fn.argtypes = _lib.SIGNATURES["dwm_head_exchange"]

    def rc(src=0x10000, dst=0x20000, rows=4, S=3, R=2, Dr=64, es=2, ld=None, d=0):
        return fn(src, dst, rows, S, R, Dr, es, S * R * Dr if ld is None else ld, d, None)
    assert rc(src=0) == -1 and rc(dst=None) == -1
    assert rc(rows=0) == -1 and rc(S=0) == -1 and rc(R=-1) == -1 and rc(Dr=0) == -1
    assert rc(es=3) == -1 and rc(es=8) == -1 and rc(d=2) == -1
    assert rc(ld=3 * 2 * 64 - 8) == -1                                           # rows would overlap
    assert rc(Dr=60, ld=512) == -2 and rc(Dr=4, ld=64) == -2                      # 120- and 8-byte runs
    assert rc(Dr=6, es=4, ld=64) == -2                                           # 24-byte fp32 run
    assert rc(ld=3 * 2 * 64 + 4) == -2                                           # stride off the grid
    assert rc(src=0x10008) == -2 and rc(dst=0x20004) == -2
    assert rc(rows=1 << 31) == -3 and rc(rows=1 << 24, R=8, Dr=192) == -3         # 2^24 * 3 * 8 * 24 pieces
