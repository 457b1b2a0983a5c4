"""Measurements of the frame shard's head exchange (opendwm_amd/sharding.py, `CTSDDenoiser(frame_exchange="heads")`) on ONE GPU: the
pack / unpack kernel dwm_head_exchange next to dwm_block_permute on the same number of bytes, and what the exchange's launches add
to a denoise step of a "full" temporal-attention model.  One process, a one-rank RCCL group (as tests/test_rccl_gpu.py), device
events, every shape warmed up, the candidates ALTERNATED inside every iteration.  One JSON line per measurement, printed and appended
to --out (default profiles/head_exchange_kernel.log).  The links are not measured here: with one rank every all-to-all is a
device-local copy.

    python scripts/measure_head_exchange.py --copies [--iters 20]
        the UniMLVG geometry: CFG batch 2, T = 20 frames, V = 6 views, 16 x 28 tokens, D = 1536 (24 heads), bf16.  One rank of R = 2 / 8
        holds rows = 2 * 20 * 6 * 448 / R token rows (at R = 8 that is the byte count of 2.5 frames: T = 20 does not split over 8
        ranks, the copy only sees a row count).  "split" / "merge": dwm_head_exchange with S = 3 (q | k | v out) and S = 1 (attention
        output back), runs of D / R channels.  "block_permute": dwm_block_permute in the frames_to_rows geometry - [image][j] blocks
        of (16 / R) token rows x 28 x (S * D) channels -> [j][image] - on the same bytes.  "copy_": torch's dense device copy of the
        same bytes, the rate a copy can reach on this device.  TB/s = 2 x bytes / time (every byte is read once and written once).
    python scripts/measure_head_exchange.py --step [--step-iters 5]
        one denoise step (CFG batch 2 x 20 frames x 6 views, 32 x 56 latents, the 24-layer model of bench.py with
        temporal_attention_type="full") unsharded against frame_exchange="heads" over the one-rank group: per temporal block one
        split, two device all_to_all_single and one merge more, and the attention on the exchanged row map.
"""
import argparse
import json
import os
import socket
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (model constants, seeded synthetic weights / conditions; not edited)

bf16 = torch.bfloat16
OUT = None
B2, T, V, HEIGHT, WIDTH, HEADS = 2, 20, 6, 16, 28, 24
D = HEADS * 64


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(fns: dict, iters: int, warmup: int = 3) -> dict:
    """{name: [ms, ...]}: the candidates take turns inside every iteration"""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {n: [] for n in fns}
    for _ in range(iters):
        for n, fn in fns.items():
            ts[n].append(timed(fn))
    return ts


def stats(ts, nbytes=None) -> dict:
    mean = sum(ts) / len(ts)
    r = {"iters": len(ts), "ms_min": min(ts), "ms_mean": mean, "ms_max": max(ts)}
    if nbytes is not None:
        r["TB_per_s_mean"] = 2.0 * nbytes / (mean * 1e-3) / 1e12
        r["TB_per_s_best"] = 2.0 * nbytes / (min(ts) * 1e-3) / 1e12
    return r


def measure_copies(iters: int) -> None:
    from opendwm_amd import ops
    dev = torch.device("cuda:0")
    N = HEIGHT * WIDTH
    for R in (2, 8):
        rows, images, hl = B2 * T * V * N // R, B2 * T * V // R, HEIGHT // R
        Dr = D // R
        for S in (3, 1):
            g = torch.Generator().manual_seed(R * 10 + S)
            wide = torch.randn(rows, S * D, generator=g).to(bf16).to(dev)
            dense = torch.empty(R, rows, S, Dr, dtype=bf16, device=dev)
            back = torch.empty_like(wide)
            perm = torch.empty_like(wide)
            plain = torch.empty_like(wide)
            blk = hl * WIDTH * S * D
            fns = {"split": lambda: ops.head_exchange(wide, dense, rows, S, R, Dr),
                   "merge": lambda: ops.head_exchange(dense, back, rows, S, R, Dr, merge=True),
                   "block_permute": lambda: ops.block_permute(wide, perm, (R, images, 1, 1), (1, R, 1, 1), blk),
                   "copy_": lambda: plain.copy_(wide)}
            ts = alternate(fns, iters)
            nbytes = wide.numel() * wide.element_size()
            ok = torch.equal(dense, wide.view(rows, S, R, Dr).permute(2, 0, 1, 3)) and torch.equal(back, wide) and \
                torch.equal(perm.view(R, images, blk), wide.view(images, R, blk).transpose(0, 1))
            emit({"measurement": "copy", "R": R, "S": S, "rows": rows, "Dr": Dr, "run_bytes": Dr * 2, "block_permute_block_bytes": blk * 2,
                  "bytes": nbytes, "dtype": "bf16", "results_equal_torch": bool(ok), **{n: stats(t, nbytes) for n, t in ts.items()}})
            if not ok:
                raise SystemExit("a copy differs from its torch permute")


def measure_step(iters: int) -> None:
    import torch.distributed as dist
    from opendwm_amd.pipeline import CTSDDenoiser
    dev = torch.device("cuda:0")
    kwargs = dict(bench.MODEL_KWARGS, temporal_attention_type="full")
    model = bench.build_model(kwargs, dev, 0)
    w = dict(bench.WORKLOAD, B=B2 // 2, T=T)
    cond = bench.make_conditions(dev, 0, w)
    lat = torch.randn(w["B"], T, V, w["C"], w["H"], w["W"], device=dev, generator=torch.Generator(device="cuda").manual_seed(3))
    dens = {"unsharded": CTSDDenoiser(model, guidance_scale=w["guidance_scale"], inference_steps=w["inference_steps"]),
            "heads_R1": CTSDDenoiser(model, guidance_scale=w["guidance_scale"], inference_steps=w["inference_steps"],
                                     frame_group=dist.group.WORLD, frame_exchange="heads")}
    for den in dens.values():
        den.prepare(lat, cond)

    def step_of(den):
        def run():
            model.frame_shard = den.frame_shard              # one model under both denoisers: prepare() set the last one's
            den.step(0)
            den.latents.copy_(lat)                           # the same step every time
            den._refresh_model_in()
        return run
    with torch.no_grad():
        ts = alternate({n: step_of(d) for n, d in dens.items()}, iters, warmup=1)
        outs = {}
        for n, den in dens.items():
            model.frame_shard = den.frame_shard
            den.step(0)
            outs[n] = den.latents.clone()
    diff = (outs["heads_R1"].double() - outs["unsharded"].double()).norm() / outs["unsharded"].double().norm()
    n_t = len(kwargs["temporal_block_layers"])
    tokens = B2 * T * V * HEIGHT * WIDTH
    emit({"measurement": "denoise_step", "temporal_attention_type": "full", "cfg_batch": B2, "frames": T, "views": V,
          "tokens_per_image": HEIGHT * WIDTH, "layers": kwargs["num_layers"], "temporal_blocks": n_t, "full_attention_L": T * HEIGHT * WIDTH,
          "exchange_bytes_per_block_R1": 4 * tokens * D * 2, "rel_diff_latents": diff.item(),
          **{n: stats(t) for n, t in ts.items()}})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--step-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_exchange_kernel.log"))
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters: at least 20 timed iterations per shape")
    OUT = a.out
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    from opendwm_amd import _lib
    _lib.load()
    if not torch.cuda.is_available():
        raise SystemExit("measure_head_exchange.py measures on a HIP device; none is visible")
    if a.copies:
        measure_copies(a.iters)
    if a.step:
        import torch.distributed as dist
        torch.cuda.set_device(0)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=torch.device("cuda", 0))
        try:
            measure_step(a.step_iters)
        finally:
            dist.destroy_process_group()
