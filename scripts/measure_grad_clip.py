"""Measurements of the fused gradient clip / unscale / non-finite check (CTSDTrainer(grad_conditioning="fused")) on
the `bench.py --train` model (constants imported from bench.py, which is not edited).  One JSON line per measurement; the
reference of every time is the "torch" route of the same process.

    python scripts/measure_grad_clip.py [--rounds 5]
        On the full parameter list of the --train model (shapes from a meta-device build; no forward; gradients filled with
        scaled noise): the stretch from the end of the backward to the end of optimizer.step, by device events, the two routes
        alternated - "torch": GradScaler.unscale_, torch.nn.utils.clip_grad_norm_(1.0), GradScaler.step, update; "fused":
        train.grad_norm_and_coef, AdamW.step(grad_scale=coef), LossScaler.update - and dwm_grad_sumsq_multi alone (both of its
        launches and the upload of its item table): ms, TB/s, share of the HBM peak.
    python scripts/measure_grad_clip.py --step [--steps 3 --warmup 2]
        ms per whole train step at the --train geometry with GradScaler + clip 1.0, "torch" then "fused" in the same call.
"""
import argparse
import gc
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HBM_TBPS = 8.0          # MI355X HBM3E peak
TRAINING_CONFIG = {"enable_grad_scaler": True, "max_norm_for_grad_clip": 1.0}


def _stats(ts):
    return {"ms_min": min(ts), "ms_mean": sum(ts) / len(ts), "ms_max": max(ts), "runs": len(ts)}


def measure_optimizer_stretch(rounds: int) -> None:
    from opendwm_amd import _lib, train
    from opendwm_amd import train_ops as T
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    _lib.load()
    dev = torch.device("cuda:0")
    with torch.device("meta"):
        shapes = [tuple(p.shape) for p in DiTCrossviewTemporalConditionModel(**bench.MODEL_KWARGS).parameters()]
    params = [torch.nn.Parameter(torch.zeros(s, device=dev)) for s in shapes]
    total = sum(p.numel() for p in params)
    scale = 65536.0
    gen = torch.Generator(device="cuda").manual_seed(0)
    g0 = [torch.randn(s, device=dev, generator=gen) * (1e-3 * scale) for s in shapes]      # what a scaled backward leaves
    for p, g in zip(params, g0):
        p.grad = g.clone()
    grads = [p.grad for p in params]
    opt = train.AdamW(params, lr=1e-5, betas=(0.9, 0.975), weight_decay=0.01)
    theirs, ours = torch.amp.GradScaler("cuda", init_scale=scale), train.LossScaler(init_scale=scale)
    theirs.scale(torch.zeros((), device=dev))            # GradScaler makes its scale tensor on first use

    def torch_route():
        theirs.unscale_(opt)
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        theirs.step(opt)
        theirs.update()

    def fused_route():
        _, coef, found_inf = train.grad_norm_and_coef(params, 1.0, 1.0 / ours.get_scale())
        if not found_inf:
            opt.step(grad_scale=coef)
        ours.update(found_inf)

    def norm_kernel():
        T.grad_sumsq_multi(grads, 1.0 / scale, 1.0)

    times = {"torch": [], "fused": [], "norm_kernel": []}
    for it in range(rounds + 1):                          # round 0 of each is the warm-up
        for name, fn in (("torch", torch_route), ("fused", fused_route), ("norm_kernel", norm_kernel)):
            torch._foreach_copy_(grads, g0)               # the torch route rewrites the gradients: every run starts from the same
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it:
                times[name].append(e0.elapsed_time(e1))
    out = T.grad_sumsq_multi(grads, 1.0 / scale, 1.0).tolist()
    base = {"tensors": len(params), "elements": total, "grad_GB": total * 4 / 1e9}
    for name in ("torch", "fused"):
        print(json.dumps({"route": name, "stretch": "end of backward -> end of optimizer.step (GradScaler + clip 1.0)", **base,
                          **_stats(times[name])}))
    st = _stats(times["norm_kernel"])
    tbps = total * 4 / (st["ms_mean"] * 1e-3) / 1e12
    print(json.dumps({"kernel": "grad_sumsq_multi_kernel + grad_finish_kernel", **base, **st, "TB_per_s_mean": tbps,
                      "share_of_hbm_peak": tbps / HBM_TBPS, "TB_per_s_best": total * 4 / (st["ms_min"] * 1e-3) / 1e12,
                      "float4_copy_share": 0.79, "adamw_multi_kernel_share": 0.71, "layernorm_share": 0.68,
                      "norm": out[0], "coef": out[1], "found_inf": out[2]}))
    mt, mf = _stats(times["torch"])["ms_mean"], _stats(times["fused"])["ms_mean"]
    print(json.dumps({"saved_ms_per_optimizer_step": mt - mf, "torch_over_fused": mt / mf}))


def measure_step(steps: int, warmup: int) -> None:
    from opendwm_amd import _lib
    from opendwm_amd.blocks import STORE
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.pipeline import CTSDTrainer
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    w = bench.WORKLOAD
    for mode in ("torch", "fused"):
        with torch.device(dev):
            model = DiTCrossviewTemporalConditionModel(**bench.MODEL_KWARGS)
        bench.synth_init_(model, 0)
        trainer = CTSDTrainer(model, lr=1e-5, weight_decay=0.01, training_config=dict(TRAINING_CONFIG), grad_conditioning=mode)
        cond = {k: (v[:w["B"]] if torch.is_tensor(v) else v) for k, v in bench.make_conditions(dev, seed=0).items()}
        g = torch.Generator(device="cuda").manual_seed(0)
        latents = torch.randn(w["B"], w["T"], w["V"], w["C"], w["H"], w["W"], device=dev, generator=g)
        gen = torch.Generator().manual_seed(1234)
        torch.cuda.reset_peak_memory_stats(dev)
        losses = []
        for _ in range(warmup):
            losses.append(trainer.train_step(latents, cond, generator=gen))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            losses.append(trainer.train_step(latents, cond, generator=gen))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        print(json.dumps({"grad_conditioning": mode, "ms_per_step": 1e3 * dt / steps, "steps": steps, "warmup": warmup,
                          "peak_memory_GiB": torch.cuda.max_memory_allocated(dev) / 2 ** 30,
                          "parameters": sum(p.numel() for p in model.parameters()), "optimizer_t": trainer.optimizer.t,
                          "skipped_steps": trainer.skipped_steps, "last_grad_norm": trainer.last_grad_norm if mode == "fused" else None,
                          "scale": trainer.grad_scaler.get_scale(), "loss_first": float(losses[0]), "loss_last": float(losses[-1])}))
        del trainer, model, cond, latents, losses
        STORE.bump()
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.step:
        measure_step(a.steps, a.warmup)
    else:
        measure_optimizer_stretch(a.rounds)
