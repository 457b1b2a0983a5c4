"""The SD 3.5 train step with kept block activations against the gradient-checkpointed one (CTSDTrainer(activations="keep") against
"recompute") on the `bench.py --train` model and workload (constants imported from bench.py, which is not edited).

    python scripts/measure_keep_activations.py [--layers N] [--budget GIB] [--steps 3] [--warmup 2] [--out profiles]

One process, one model, two trainers over it that share one AdamW (so the second trainer costs no optimizer state); the two modes
alternate step by step - recompute, keep, recompute, keep ... - after `--warmup` steps of each, every step timed by device events
around train_step.  Written to <out>/keep_activations_<full | layersN>[_budgetG].log, one JSON line per mode (ms per step: min / mean
/ max; peak GiB of the mode's steps), the plan of the last "keep" forward (kept-byte total, per block kind, blocks kept /
recomputed) and a summary line with the ratio - whichever way it falls."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

MODES = ("recompute", "keep")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None, help="truncate the model to N layers (a short run)")
    ap.add_argument("--budget", type=float, default=None, help="activation_budget_gib of the keep trainer")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()

    from opendwm_amd import _lib
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.pipeline import CTSDTrainer
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    kwargs = dict(bench.MODEL_KWARGS)
    if a.layers is not None:
        n = a.layers
        kwargs.update(num_layers=n, dual_attention_layers=[i for i in kwargs["dual_attention_layers"] if i < n],
                      crossview_block_layers=[i for i in kwargs["crossview_block_layers"] if i < n],
                      temporal_block_layers=[i for i in kwargs["temporal_block_layers"] if i < n])
    with torch.device(dev):
        model = DiTCrossviewTemporalConditionModel(**kwargs)
    bench.synth_init_(model, 0)
    trainers = {m: CTSDTrainer(model, lr=1e-5, weight_decay=0.01, activations=m,
                               activation_budget_gib=a.budget if m == "keep" else None) for m in MODES}
    trainers["keep"].optimizer = trainers["recompute"].optimizer
    w = bench.WORKLOAD
    cond = {k: (v[:w["B"]] if torch.is_tensor(v) else v) for k, v in bench.make_conditions(dev, seed=0).items()}
    latents = torch.randn(w["B"], w["T"], w["V"], w["C"], w["H"], w["W"], device=dev, generator=torch.Generator(device="cuda").manual_seed(0))
    gen = torch.Generator().manual_seed(1234)

    ms = {m: [] for m in MODES}
    peak = {m: 0 for m in MODES}
    losses = {m: [] for m in MODES}
    for it in range(a.warmup + a.steps):
        for m in MODES:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            e0.record()
            loss = trainers[m].train_step(latents, cond, generator=gen)
            e1.record()
            torch.cuda.synchronize()
            losses[m].append(float(loss))
            if it >= a.warmup:
                ms[m].append(e0.elapsed_time(e1))
                peak[m] = max(peak[m], torch.cuda.max_memory_allocated(dev))

    tag = ("full" if a.layers is None else f"layers{a.layers}") + ("" if a.budget is None else f"_budget{a.budget:g}")
    base = {"layers": kwargs["num_layers"], "budget_gib": a.budget, "steps": a.steps, "warmup": a.warmup,
            "workload": [w[k] for k in ("B", "T", "V", "C", "H", "W")], "device": torch.cuda.get_device_name(0)}
    lines = []
    for m in MODES:
        t = ms[m]
        lines.append({"activations": m, **base, "ms_per_step_mean": sum(t) / len(t), "ms_per_step_min": min(t), "ms_per_step_max": max(t),
                      "ms_per_step": t, "peak_GiB": peak[m] / 2 ** 30, "loss_first": losses[m][0], "loss_last": losses[m][-1],
                      "finite": all(x == x and abs(x) != float("inf") for x in losses[m])})
    plan = trainers["keep"].activation_plan
    kinds = {}
    for name, what, nbytes in plan.blocks:
        k = kinds.setdefault(name.split(".")[0], {"keep": 0, "recompute": 0, "kept_GiB": 0.0, "kept_bytes_largest_block": 0})
        k[what] += 1
        k["kept_GiB"] += nbytes / 2 ** 30
        k["kept_bytes_largest_block"] = max(k["kept_bytes_largest_block"], nbytes)
    lines.append({"plan": "last keep forward", "kept_bytes_total": plan.total_bytes, "kept_GiB_total": plan.total_bytes / 2 ** 30,
                  "blocks": len(plan), "kept": sum(b[1] == "keep" for b in plan.blocks), "per_family": kinds})
    r, k = lines[0]["ms_per_step_mean"], lines[1]["ms_per_step_mean"]
    lines.append({"summary": "keep against recompute, alternated in one process", "recompute_ms": r, "keep_ms": k, "keep_over_recompute": k / r,
                  "saved_ms_per_step": r - k, "keep_is_faster": k < r, "peak_GiB_recompute": lines[0]["peak_GiB"],
                  "peak_GiB_keep": lines[1]["peak_GiB"]})
    os.makedirs(a.out, exist_ok=True)
    path = os.path.join(a.out, f"keep_activations_{tag}.log")
    with open(path, "w") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")
    print(f"written {path}")


if __name__ == "__main__":
    main()
