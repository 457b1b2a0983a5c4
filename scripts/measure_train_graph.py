"""Train step eager against CTSDTrainer(graph=True) in ONE process on ONE model: an eager trainer and a graph trainer share
the model and take turns, step by step, after warm-up - so clocks, allocator state and the weights' values are the same for both.  The
eager trainer is the trainer of `bench.py --train`: the yardstick.  Random weights, synthetic inputs.  One JSON line per measurement,
printed and appended to --out.

    python scripts/measure_train_graph.py --geometry unet|interactive|config4 [--iters 8] [--warmup 2] [--layers N] [--out FILE]

Geometries: `unet` = the `bench.py --train --unet` workload; `interactive` = the reduced SD 3.5 model of the reference's interactive
configuration as scripts/measure_streaming.py writes it out (12 layers, 20 heads, 3 views x 6 frames of 176 x 304); `config4` =
BASELINE config 4, the `bench.py --train` workload (--layers caps its depth).

Reported per mode:
  * ms per step: `host_ms` = wall time until train_step returns (what the host spends issuing the step), `device_ms` = device events
    around train_step, `wall_ms` = wall time until the device has finished the step; median, min, max over the alternated steps;
  * `loop_ms_per_step`: wall time around a loop of back-to-back steps of one mode with one synchronisation at its end;
  * `library_launches`: calls into libdwm_hip.so the host makes per step (torch's own launches are not counted);
  * `capture_seconds`, `graph_pool_GiB` (what the capture's pool and static buffers pin that an eager step frees) and the peak GiB
    of a step of each mode;
  * the optimizer part alone on the same gradients: the eager fused route (one read of the gradients, a host read of its result,
    the by-value AdamW launch) against the queued route (the same read, the *_dev AdamW launch, no host read)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                    # model kwargs, workloads and the seeded synthetic weights of the benchmark

bf16 = torch.bfloat16
OUT = None


def emit(rec: dict) -> None:
    line = json.dumps(rec)
    print(line, flush=True)
    with open(OUT, "a") as f:
        f.write(line + "\n")


def stats(ts) -> dict:
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3), "n": len(ts)}


def timed_call(fn) -> tuple:
    """(host ms until fn returns, device ms between events around it, wall ms until the device is done)"""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0), e0.elapsed_time(e1), 1e3 * (t2 - t0)


class LaunchCount:
    """counts the calls into the library made through ops._call / train_ops._call while active"""

    def __enter__(self):
        from opendwm_amd import ops, train_ops
        self.n, self.mods, self.saved = 0, (ops, train_ops), (ops._call, train_ops._call)
        c0 = ops._call

        def call(name, *args):
            self.n += 1
            return c0(name, *args)
        ops._call = train_ops._call = call
        return self

    def __exit__(self, *exc):
        for m, f in zip(self.mods, self.saved):
            m._call = f


def build(geometry: str, dev, layers):
    """(model with fp32 master parameters, latents, conditions, description)"""
    if geometry == "unet":
        from opendwm_amd.unet import UNetCrossviewTemporalConditionModel
        with torch.device(dev):
            model = UNetCrossviewTemporalConditionModel(**bench.UNET_KWARGS)
        bench._unet_synth_init_(model, 0)
        w = bench.UNET_WORKLOAD
        B, T, V = w["B"], w["T"], w["V"]
        g = torch.Generator(device="cuda").manual_seed(1000)
        ring = torch.zeros(V, V, dtype=torch.bool)
        for i in range(V):
            for d in (-1, 0, 1):
                ring[i, (i + d) % V] = True
        cond = dict(encoder_hidden_states=(torch.randn(B, T, V, w["text_len"], 1024, device=dev, generator=g) * 0.5).to(bf16),
                    disable_crossview=torch.zeros(B, dtype=torch.bool, device=dev),
                    disable_temporal=torch.zeros(B, dtype=torch.bool, device=dev),
                    crossview_attention_mask=ring[None].repeat(B, 1, 1).to(dev),
                    added_time_ids=torch.rand(B, T, V, 11, device=dev, generator=g) * 2 - 1)
        lat = torch.randn(B, T, V, w["C"], w["H"], w["W"], device=dev, generator=g)
        return model, lat, cond, "bench.py --train --unet workload: SD 2.1 UNet, one [1,6,6,4,32,56] sample"
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    if geometry == "interactive":
        from scripts.measure_streaming import MODEL_KWARGS, WORKLOAD
        kwargs, w, layout = dict(MODEL_KWARGS), dict(WORKLOAD), True
        what = "reduced SD 3.5 model of the interactive configuration: 12 layers, 20 heads, layout adapter, 3 views x 6 frames of 176 x 304"
    else:
        kwargs, w, layout = dict(bench.MODEL_KWARGS), dict(bench.WORKLOAD), False
        what = "BASELINE config 4 (bench.py --train): SD 3.5 MMDiT, one [1,16,6,16,32,56] sample"
    if layers is not None:
        kwargs.update(num_layers=layers, dual_attention_layers=[i for i in kwargs["dual_attention_layers"] if i < layers],
                      crossview_block_layers=[i for i in kwargs["crossview_block_layers"] if i < layers],
                      temporal_block_layers=[i for i in kwargs["temporal_block_layers"] if i < layers])
        what += f", first {layers} layers"
    with torch.device(dev):
        model = DiTCrossviewTemporalConditionModel(**kwargs)
    bench.synth_init_(model, 0)
    cond = {k: (v[:w["B"]] if torch.is_tensor(v) else v) for k, v in bench.make_conditions(dev, 0, w, layout=layout).items()}
    g = torch.Generator(device="cuda").manual_seed(0)
    lat = torch.randn(w["B"], w["T"], w["V"], w["C"], w["H"], w["W"], device=dev, generator=g)
    return model, lat, cond, what


def measure(geometry: str, dev, iters: int, warmup: int, layers) -> None:
    from opendwm_amd import train, train_ops as T
    from opendwm_amd.pipeline import CTSDTrainer
    model, lat, cond, what = build(geometry, dev, layers)
    n_params = sum(p.numel() for p in model.parameters())
    emit({"what": "geometry", "geometry": geometry, "workload": what, "parameters": n_params, "device": torch.cuda.get_device_name(dev),
          "iters": iters, "warmup": warmup})
    trainers = {"eager": CTSDTrainer(model, lr=1e-5, weight_decay=0.01), "graph": CTSDTrainer(model, lr=1e-5, weight_decay=0.01, graph=True)}
    gen = torch.Generator().manual_seed(1234)
    step = {k: (lambda tr=tr: tr.train_step(lat, cond, generator=gen)) for k, tr in trainers.items()}
    for _ in range(warmup):
        step["eager"]()
    tg = trainers["graph"]
    step["graph"]()                                  # the graph trainer's eager warm-up step
    torch.cuda.synchronize()
    assert tg.graph_captures == 0
    before = torch.cuda.memory_allocated(dev)
    step["graph"]()                                  # capture + first replay
    torch.cuda.synchronize()
    pool = torch.cuda.memory_allocated(dev) - before
    emit({"what": "capture", "geometry": geometry, "capture_seconds": round(tg.graph_capture_seconds, 3), "graph_captures": tg.graph_captures,
          "graph_pool_GiB": round(pool / 2 ** 30, 3)})
    per = {k: {"host_ms": [], "device_ms": [], "wall_ms": []} for k in step}
    launches, peak = {}, {}
    for i in range(iters):                           # alternated, step by step
        for k in ("eager", "graph"):
            torch.cuda.reset_peak_memory_stats(dev)
            with LaunchCount() as lc:
                h, d, wl = timed_call(step[k])
            per[k]["host_ms"].append(h); per[k]["device_ms"].append(d); per[k]["wall_ms"].append(wl)
            launches[k] = lc.n
            peak[k] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    loop = {}
    for k in ("eager", "graph", "eager", "graph"):   # back-to-back steps of one mode, one synchronisation at the end
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            step[k]()
        torch.cuda.synchronize()
        loop.setdefault(k, []).append(1e3 * (time.perf_counter() - t0) / iters)
    for k in ("eager", "graph"):
        emit({"what": "train_step", "geometry": geometry, "mode": k, **{n: stats(v) for n, v in per[k].items()},
              "loop_ms_per_step": [round(x, 3) for x in loop[k]], "library_launches": launches[k], "peak_GiB": round(peak[k], 3),
              "graph_replays": trainers[k].graph_replays, "graph_captures": trainers[k].graph_captures})
    # ---- the optimizer part alone, on the gradients the graph holds: fused eager route (host read) against the queued route
    params = [p for p, _ in tg._g_grads]
    for p, g in tg._g_grads:
        p.grad = g
    gs = [g for _, g in tg._g_grads]
    opt_e, opt_d = trainers["eager"].optimizer, tg.optimizer

    def eager_route():
        _, coef, found = train.grad_norm_and_coef(params, 1.0)
        if not found:
            opt_e.step(grad_scale=coef)

    def queued_route():
        opt_d.step(device_operands=(None, T.grad_sumsq_multi(gs, 1.0, 1.0, reuse_items=True)))
    routes = {"fused_eager": eager_route, "queued_dev": queued_route}
    res = {k: {"host_ms": [], "device_ms": [], "wall_ms": []} for k in routes}
    for i in range(iters + 1):
        for k, fn in routes.items():
            with LaunchCount() as lc:
                h, d, wl = timed_call(fn)
            if i:                                    # the first round builds the item arrays
                res[k]["host_ms"].append(h); res[k]["device_ms"].append(d); res[k]["wall_ms"].append(wl)
            launches[k] = lc.n
    for k in routes:
        emit({"what": "optimizer_part", "geometry": geometry, "route": k, **{n: stats(v) for n, v in res[k].items()},
              "library_launches": launches[k], "tensors": len(gs)})
    for p in params:
        p.grad = None


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--geometry", choices=["unet", "interactive", "config4"], required=True)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    OUT = args.out or os.path.join(ROOT, "profiles", f"train_graph_{args.geometry}.log")
    from opendwm_amd import _lib
    from opendwm_amd.build import ensure_built
    ensure_built()
    _lib.load()
    measure(args.geometry, torch.device("cuda:0"), args.iters, args.warmup, args.layers)


if __name__ == "__main__":
    main()
