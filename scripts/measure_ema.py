"""Measurements of the EMA of the weights on the `bench.py --train` model (constants imported from bench.py, which is
not edited), or on its first N layers (`--layers N`).  One process, the routes alternated, device events around every measurement;
one JSON line per measurement, on stdout and appended to profiles/ema_<what>.log.

    python scripts/measure_ema.py --kernels [--launches 6] [--layers N]
        the optimizer launches alone on the model's parameter list (shapes from a meta-device build; no forward), for fp32 and
        8-bit moments: the plain AdamW launch (30 / 18 bytes per parameter), the fused AdamW + EMA launch (38 / 26) and the
        two-launch route (the plain launch, then dwm_ema_multi: 30 + 12 / 18 + 12).  ms, achieved TB/s, share of the HBM peak.
    python scripts/measure_ema.py --step [--steps 3 --warmup 2] [--layers N] [--bits 32]
        ms per train step at the --train geometry of ONE trainer whose route is switched from step to step: without EMA, with the
        fused EMA, with the two-launch route (`train.EMA.fused = False`); peak GiB with and without the shadows.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HBM_TBPS = 8.0          # MI355X HBM3E peak


def _emit(what: str, row: dict) -> None:
    line = json.dumps(row)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", f"ema_{what}.log"), "a") as f:
        f.write(line + "\n")


def _model_kwargs(layers):
    kwargs = dict(bench.MODEL_KWARGS)
    if layers is not None:
        kwargs.update(num_layers=layers, dual_attention_layers=[i for i in kwargs["dual_attention_layers"] if i < layers],
                      crossview_block_layers=[i for i in kwargs["crossview_block_layers"] if i < layers],
                      temporal_block_layers=[i for i in kwargs["temporal_block_layers"] if i < layers])
    return kwargs


def _timed(fn) -> float:
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure_kernels(launches: int, layers) -> None:
    from opendwm_amd import _lib, quant8
    from opendwm_amd import train_ops as T
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    _lib.load()
    dev = torch.device("cuda:0")
    with torch.device("meta"):
        numels = [p.numel() for p in DiTCrossviewTemporalConditionModel(**_model_kwargs(layers)).parameters()]
    big = [i for i, n in enumerate(numels) if n >= 4096]
    pick = lambda lst: [lst[i] for i in big]
    ps = [torch.zeros(n, device=dev) for n in numels]
    gs = [torch.full((n,), 1e-3, device=dev) for n in numels]
    es = [torch.zeros(n, device=dev) for n in numels]
    sh = [torch.empty(n, dtype=torch.bfloat16, device=dev) if n % 4 == 0 else None for n in numels]
    ms, vs = [torch.zeros(n, device=dev) for n in numels], [torch.zeros(n, device=dev) for n in numels]
    mq = [torch.full((numels[i],), quant8.zero_code(True), dtype=torch.uint8, device=dev) for i in big]
    vq = [torch.zeros(numels[i], dtype=torch.uint8, device=dev) for i in big]
    ma = [torch.zeros(quant8.n_blocks(numels[i]), device=dev) for i in big]
    va = [torch.zeros(quant8.n_blocks(numels[i]), device=dev) for i in big]
    kw = dict(lr=1e-5, beta1=0.9, beta2=0.975, eps=1e-8, weight_decay=0.01)
    omd = 1e-4
    a32, a8 = (ps, gs, ms, vs, sh), (pick(ps), pick(gs), mq, ma, vq, va, pick(sh))
    routes = {
        (32, "plain"): lambda s: T.adamw_multi_(*a32, step=s, **kw),
        (32, "fused"): lambda s: T.adamw_ema_multi_(*a32, es, step=s, one_minus_decay=omd, **kw),
        (32, "two_launch"): lambda s: (T.adamw_multi_(*a32, step=s, **kw), T.ema_multi_(es, ps, one_minus_decay=omd)),
        (8, "plain"): lambda s: T.adamw8_multi_(*a8, step=s, **kw),
        (8, "fused"): lambda s: T.adamw8_ema_multi_(*a8, pick(es), step=s, one_minus_decay=omd, **kw),
        (8, "two_launch"): lambda s: (T.adamw8_multi_(*a8, step=s, **kw), T.ema_multi_(pick(es), pick(ps), one_minus_decay=omd)),
    }
    times = {k: [] for k in routes}
    for it in range(launches + 1):                      # launch 0 of each is the warm-up
        for k, fn in routes.items():
            t = _timed(lambda: fn(it + 1))
            if it:
                times[k].append(t)
    bytes_per = {(32, "plain"): 30, (32, "fused"): 38, (32, "two_launch"): 42, (8, "plain"): 18, (8, "fused"): 26, (8, "two_launch"): 30}
    for (bits, route), ts in times.items():
        n = sum(numels) if bits == 32 else sum(numels[i] for i in big)
        mean = sum(ts) / len(ts)
        tbps = n * bytes_per[(bits, route)] / (mean * 1e-3) / 1e12
        _emit("kernels", {"optimizer_bits": bits, "route": route, "layers": layers, "tensors": len(numels) if bits == 32 else len(big),
                          "elements": n, "bytes_per_element": bytes_per[(bits, route)], "launches": len(ts), "ms_min": min(ts),
                          "ms_mean": mean, "ms_max": max(ts), "TB_per_s_mean": tbps, "share_of_hbm_peak": tbps / HBM_TBPS})


def measure_step(steps: int, warmup: int, layers, bits: int) -> None:
    from opendwm_amd import _lib
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.pipeline import CTSDTrainer
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    w = bench.WORKLOAD
    with torch.device(dev):
        model = DiTCrossviewTemporalConditionModel(**_model_kwargs(layers))
    bench.synth_init_(model, 0)
    cond = {k: (v[:w["B"]] if torch.is_tensor(v) else v) for k, v in bench.make_conditions(dev, seed=0).items()}
    latents = torch.randn(w["B"], w["T"], w["V"], w["C"], w["H"], w["W"], device=dev, generator=torch.Generator(device="cuda").manual_seed(0))
    gen = torch.Generator().manual_seed(1234)
    trainer = CTSDTrainer(model, lr=1e-5, weight_decay=0.01, optimizer_bits=bits)
    torch.cuda.reset_peak_memory_stats(dev)
    for _ in range(warmup):
        trainer.train_step(latents, cond, generator=gen)
    torch.cuda.synchronize()
    peak_plain = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    from opendwm_amd.train import EMA
    ema = EMA(trainer._named_optimized(), decay=0.9999)
    ema.optimization_step = 1000                        # past the first step (decay 0) and the ramp: a steady-state 1 - decay

    def route(name):
        trainer.ema, ema.fused = (None if name == "none" else ema), name != "two_launch"
    times = {"none": [], "fused": [], "two_launch": []}
    for it in range(steps + 1):                         # round 0 warms every route up
        for name in times:
            route(name)
            t = _timed(lambda: trainer.train_step(latents, cond, generator=gen))
            if it:
                times[name].append(t)
    peak_ema = torch.cuda.max_memory_allocated(dev) / 2 ** 30
    n = sum(p.numel() for p in model.parameters())
    for name, ts in times.items():
        _emit("step", {"route": name, "optimizer_bits": bits, "layers": layers, "parameters": n, "steps": len(ts),
                       "ms_per_step_mean": sum(ts) / len(ts), "ms_per_step_min": min(ts),
                       "peak_memory_GiB": peak_plain if name == "none" else peak_ema, "shadow_GiB": 4 * n / 2 ** 30})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--launches", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--layers", type=int, default=None, help="truncate the model to its first N layers")
    ap.add_argument("--bits", type=int, default=32, choices=(8, 32))
    a = ap.parse_args()
    if a.kernels:
        measure_kernels(a.launches, a.layers)
    if a.step:
        measure_step(a.steps, a.warmup, a.layers, a.bits)
