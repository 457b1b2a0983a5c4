"""Measurements of the block-wise 8-bit AdamW on the `bench.py --train` model (constants imported from bench.py, which is
not edited).  One JSON line per measurement.

    python scripts/measure_adam8bit.py --kernels [--launches 6]
        adamw_multi_kernel and adamw8_multi_kernel alternated on the full parameter list of the --train model (shapes from a
        meta-device build; no forward): ms per launch by events, achieved bytes/s from 30 and 18 bytes per element.  Under
        `rocprofv3 --kernel-trace --stats -- python scripts/measure_adam8bit.py --kernels` the kernel table holds the same.
    python scripts/measure_adam8bit.py --step [--steps 3 --warmup 2]
        ms per train step and peak_memory_GiB at the --train geometry, train.AdamW then train.AdamW8bit in the same call.
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


def measure_kernels(launches: int) -> None:
    from opendwm_amd import _lib, quant8
    from opendwm_amd import train_ops as T
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    _lib.load()
    dev = torch.device("cuda:0")
    with torch.device("meta"):
        shapes = [tuple(p.shape) for p in DiTCrossviewTemporalConditionModel(**bench.MODEL_KWARGS).parameters()]
    numels = [int(torch.Size(s).numel()) for s in shapes]
    total = sum(numels)
    ps = [torch.zeros(n, device=dev) for n in numels]
    gs = [torch.full((n,), 1e-3, device=dev) for n in numels]
    sh = [torch.empty(n, dtype=torch.bfloat16, device=dev) if n % 4 == 0 else None for n in numels]
    big = [i for i, n in enumerate(numels) if n >= 4096]
    ms, vs = [torch.zeros(n, device=dev) for n in numels], [torch.zeros(n, device=dev) for n in numels]
    mq = [torch.full((numels[i],), quant8.zero_code(True), dtype=torch.uint8, device=dev) for i in big]
    vq = [torch.zeros(numels[i], dtype=torch.uint8, device=dev) for i in big]
    ma = [torch.zeros(quant8.n_blocks(numels[i]), device=dev) for i in big]
    va = [torch.zeros(quant8.n_blocks(numels[i]), device=dev) for i in big]
    n8 = sum(numels[i] for i in big)
    kw = dict(lr=1e-5, beta1=0.9, beta2=0.975, eps=1e-8, weight_decay=0.01)
    pick = lambda lst: [lst[i] for i in big]
    t32, t8 = [], []
    for it in range(launches + 1):                      # launch 0 of each is the warm-up
        for which in (32, 8):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            if which == 32:
                T.adamw_multi_(ps, gs, ms, vs, sh, step=it + 1, **kw)
            else:
                T.adamw8_multi_(pick(ps), pick(gs), mq, ma, vq, va, pick(sh), step=it + 1, **kw)
            e1.record()
            torch.cuda.synchronize()
            if it:
                (t32 if which == 32 else t8).append(e0.elapsed_time(e1))
    for name, ts, n, bpe in (("adamw_multi_kernel", t32, total, 30), ("adamw8_multi_kernel", t8, n8, 18)):
        best, mean = min(ts), sum(ts) / len(ts)
        print(json.dumps({"kernel": name, "tensors": len(numels) if bpe == 30 else len(big), "elements": n, "bytes_per_element": bpe,
                          "launches": len(ts), "ms_min": best, "ms_mean": mean, "ms_max": max(ts),
                          "TB_per_s_mean": n * bpe / (mean * 1e-3) / 1e12, "share_of_hbm_peak": n * bpe / (mean * 1e-3) / 1e12 / HBM_TBPS,
                          "ns_per_kelement": mean * 1e6 / (n / 1e3)}))


def measure_step(steps: int, warmup: int) -> None:
    from opendwm_amd import _lib
    from opendwm_amd.blocks import STORE
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.pipeline import CTSDTrainer
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    w = bench.WORKLOAD
    for bits in (32, 8):
        with torch.device(dev):
            model = DiTCrossviewTemporalConditionModel(**bench.MODEL_KWARGS)
        bench.synth_init_(model, 0)
        trainer = CTSDTrainer(model, lr=1e-5, weight_decay=0.01, optimizer_bits=bits)
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
        state = sum(t.numel() * t.element_size() for st in trainer.optimizer.state.values() for k, t in st.items() if k != "step")
        print(json.dumps({"optimizer_bits": bits, "ms_per_step": 1e3 * dt / steps, "steps": steps, "warmup": warmup,
                          "peak_memory_GiB": torch.cuda.max_memory_allocated(dev) / 2 ** 30, "optimizer_state_GiB": state / 2 ** 30,
                          "parameters": sum(p.numel() for p in model.parameters()),
                          "loss_first": float(losses[0]), "loss_last": float(losses[-1])}))
        del trainer, model, cond, latents, losses
        STORE.bump()
        gc.collect()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--launches", type=int, default=6)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.kernels:
        measure_kernels(a.launches)
    if a.step:
        measure_step(a.steps, a.warmup)
