"""ms/step of the SD 2.1 denoise loop (pipeline.UNetDenoiser, full-width UNet of examples/ctsd_21_6views_*_generation.json, bf16,
DPM-Solver++ (2M), guidance 3), eager against the replay of the whole-step HIP graph, and the grouped scheduler kernel against
the scalar one.  Device events around every step, every variant warmed up (the graph's capture happens there), the variants
ALTERNATED inside every iteration of one process.  One JSON line per measurement, printed and appended to --out.

    python scripts/measure_unet_video.py --steps [--iters 10] [--out profiles/unet_video_step.log]
        geometries (views x frames, latents): 6 x 1 at 32 x 32 (ctsd_21_6views_image_generation.json), 6 x 6 at 32 x 56
        (bench.py --unet) and 6 x 12 at 32 x 56 with 3 reference frames (ctsd_21_6views_video_generation.json).
        "eager_scalar": the loop as it was before the video modes - coefficients as launch scalars (dwm_cfg_multistep);
        "eager_tables": the same step from the device tables (dwm_cfg_multistep_grouped; with reference frames the only eager form);
        "graph_replay": enable_graph(), refresh of the static buffers + one replay.
    python scripts/measure_unet_video.py --kernel [--kernel-iters 40] [--out profiles/unet_video_kernel.log]
        dwm_cfg_multistep against dwm_cfg_multistep_grouped (one broadcast row; a row per image + reference flags) on the
        same buffers of the 6 x 12 geometry, 50 back-to-back launches per timed sample: 24 bytes per latent element move in each
        (flagged images write 4 fewer).
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                    # UNET_KWARGS, the synthetic UNet weights and conditions of bench.py --unet

bf16 = torch.bfloat16
OUT = None
GEOMETRIES = [   # name, views, frames, latent h, w, reference frames
    ("6v x 1f 32x32", 6, 1, 32, 32, 0),
    ("6v x 6f 32x56", 6, 6, 32, 56, 0),
    ("6v x 12f 32x56, 3 reference frames", 6, 12, 32, 56, 3),
]
STEPS, GUIDANCE = 50, 3.0


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


def stats(ts) -> dict:
    return {"ms_median": round(statistics.median(ts), 4), "ms_min": round(min(ts), 4), "ms_max": round(max(ts), 4), "n": len(ts)}


def build_unet(dev):
    from opendwm_amd.unet import UNetCrossviewTemporalConditionModel
    old = torch.get_default_dtype()
    torch.set_default_dtype(bf16)
    try:
        with torch.device(dev):
            model = UNetCrossviewTemporalConditionModel(**bench.UNET_KWARGS)
    finally:
        torch.set_default_dtype(old)
    model = model.to(device=dev, dtype=bf16).eval()
    g = torch.Generator(device="cuda").manual_seed(0)
    with torch.no_grad():                       # the seeded synthetic weights of bench.py --unet
        for name, p in model.named_parameters():
            if name.endswith("mix_factor"):
                p.fill_(2.0)
            elif p.dim() == 1:
                p.normal_(0.0, 0.05, generator=g)
                if name.endswith(".weight"):
                    p.add_(1.0)
            else:
                std = p[0].numel() ** -0.5
                if ".conv2." in name or name.endswith("proj_out.weight") or ".net.2." in name or ".to_out.0." in name:
                    std *= 0.5
                p.normal_(0.0, std, generator=g)
    return model


def conditions(dev, V, T):
    c = bench._make_conditions(dev, 0, dict(B=1, T=T, V=V, text_len=77), 11, text_dim=1024, pooled_dim=8)
    c.pop("pooled_projections")
    return c


def measure_steps(dev, iters: int) -> None:
    from opendwm_amd.pipeline import UNetDenoiser
    model = build_unet(dev)
    for name, V, T, h, w, ref in GEOMETRIES:
        g = torch.Generator(device="cuda").manual_seed(1)
        lat = torch.randn(1, T, V, 4, h, w, device=dev, generator=g)
        il = torch.randn(1, T, V, 4, h, w, device=dev, generator=g) if ref else None
        cond = conditions(dev, V, T)
        kw = dict(image_latents=il, reference_frame_count=ref) if ref else {}
        dens = {"eager_scalar": UNetDenoiser(model, GUIDANCE, STEPS).prepare(lat, cond)}
        if ref:
            dens["eager_tables"] = UNetDenoiser(model, GUIDANCE, STEPS).prepare(lat, cond, **kw)
        else:
            tab = UNetDenoiser(model, GUIDANCE, STEPS).prepare(lat, cond)
            tab._tables = tab._step_tables()                      # the tables without a graph or a reference frame: what
                                                                  # the device-resident numbers alone cost
            dens["eager_tables"] = tab
        dens["graph_replay"] = UNetDenoiser(model, GUIDANCE, STEPS).enable_graph().prepare(lat, cond, **kw)
        count = {n: 0 for n in dens}

        def stepper(n):
            def run():
                dens[n].step(1 + count[n] % (STEPS - 2))          # second-order steps, as bench.py --unet times them
                count[n] += 1
            return run
        ts = alternate({n: stepper(n) for n in dens}, iters)
        for n, t in ts.items():
            emit({"what": "unet_denoise_step", "geometry": name, "variant": n, "reference_frames": ref if n != "eager_scalar" else 0,
                  "finite": bool(torch.isfinite(dens[n].latents).all()), **stats(t)})
        del dens
        torch.cuda.empty_cache()


def measure_kernel(dev, iters: int) -> None:
    from opendwm_amd import ops
    _, V, T, h, w, ref = GEOMETRIES[-1]
    ge, G = 4 * h * w, T * V
    n = G * ge
    g = torch.Generator(device="cuda").manual_seed(2)
    pred = torch.randn(2 * n, device=dev, generator=g).to(bf16)
    lat, prev = torch.randn(n, device=dev, generator=g), torch.randn(n, device=dev, generator=g)
    model_in = torch.empty(2 * n, dtype=bf16, device=dev)
    row = torch.tensor([[0.5, -0.8, 0.9, 0.3, -0.1]], device=dev)
    rows = row.repeat(G, 1).contiguous()
    flags = (torch.arange(G, device=dev) // V < ref).to(torch.int32)
    launches = {
        "scalar": lambda: ops.cfg_multistep(pred, lat, prev, GUIDANCE, 0.5, -0.8, 0.9, 0.3, -0.1, model_in=model_in),
        "grouped_one_row": lambda: ops.cfg_multistep_grouped(pred, lat, prev, GUIDANCE, row, ge, model_in=model_in),
        "grouped_rows_and_flags": lambda: ops.cfg_multistep_grouped(pred, lat, prev, GUIDANCE, rows, ge, keep_model_in=flags,
                                                                    model_in=model_in),
    }
    reps = 50                                   # launches per event pair: one launch is a few microseconds

    def burst(fn):
        def run():
            for _ in range(reps):
                fn()
        return run
    ts = alternate({k: burst(fn) for k, fn in launches.items()}, iters, warmup=10)
    for name, t in ts.items():
        s = stats([x / reps for x in t])
        emit({"what": "cfg_multistep_kernel", "variant": name, "elements": n, "bytes": 24 * n, "launches_per_sample": reps,
              "GB_per_s_at_median": round(24 * n / (s["ms_median"] * 1e-3) / 1e9, 1), **s})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--kernel-iters", type=int, default=40)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_unet_video.py measures on an MI355X; no HIP device found")
    OUT = a.out or os.path.join(ROOT, "profiles", "unet_video_step.log" if a.steps else "unet_video_kernel.log")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    dev = torch.device("cuda:0")
    from opendwm_amd import _lib
    _lib.load()
    emit({"what": "run", "device": torch.cuda.get_device_name(0), "steps": a.steps, "kernel": a.kernel, "iters": a.iters,
          "kernel_iters": a.kernel_iters})
    if a.kernel:
        measure_kernel(dev, a.kernel_iters)
    if a.steps:
        measure_steps(dev, a.iters)


if __name__ == "__main__":
    main()
