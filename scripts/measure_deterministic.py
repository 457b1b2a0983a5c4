"""The SD 3.5 train step with ordered gradient reductions against the default one (CTSDTrainer(deterministic=True) against False,
DESIGN.md s22) on the `bench.py --train` model and workload (constants imported from bench.py, which is not edited).

    python scripts/measure_deterministic.py [--layers N] [--steps 3] [--warmup 2] [--out profiles]
    python scripts/measure_deterministic.py --kernels [--reps 20] [--out profiles]

Step comparison: one process, one model, two trainers over it that share one AdamW; the two modes alternate step by step - default,
deterministic, default, ... - after `--warmup` steps of each, every step timed by device events around train_step.  Written to
<out>/deterministic_<full | layersN>.log: one JSON line per mode (ms per step: min / mean / max; peak GiB of the mode's steps) and a
summary line with the ratio - whichever way it falls.  The yardstick is the default mode of the same process.

--kernels: each of the five reductions alone at the config-4 shapes (96 images x 448 tokens = 43 008 rows of 1536 columns, 154 context
tokens per image; the UNet's first level for GroupNorm), ordered against default, alternated call by call, `--reps` timed calls each
after 3 warm-up calls, device events around the wrapper (so the ordered form's workspace allocation and second launch are inside).
Written to <out>/deterministic_kernels.log, one JSON line per op with the workspace size."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

MODES = ("default", "deterministic")
bf16 = torch.bfloat16


def _timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def kernels(a) -> None:
    from opendwm_amd import _lib, train_ops as T
    lib = _lib.load()
    dev = torch.device("cuda:0")
    w = bench.WORKLOAD
    I, N, Lc, D = w["B"] * w["T"] * w["V"], (w["H"] // 2) * (w["W"] // 2), w["text_len"], 1536
    rows = I * N
    g = torch.Generator(device="cuda").manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g).to(bf16)
    x, dy, y2 = rnd(rows, D), rnd(rows, D), rnd(rows, D)
    mod = rnd(I, D) * 0.3
    dg, db = torch.zeros(I, D, device=dev), torch.zeros(I, D, device=dev)
    qk, dqk = rnd(rows, 2 * D), rnd(rows, 2 * D)
    wq = (rnd(2 * D) * 0.2 + 1).contiguous()
    rinv = T.rmsnorm_heads_train_(qk, wq, 1e-6)
    dw = torch.zeros(2 * D, device=dev)
    uw = bench.UNET_WORKLOAD
    gI, gP, gC = uw["B"] * uw["T"] * uw["V"], uw["H"] * uw["W"], 320
    gx, gdz = rnd(gI * gP, gC), rnd(gI * gP, gC)
    gam, bet = (rnd(gC) * 0.2 + 1), rnd(gC) * 0.2
    gdg, gdb = torch.zeros(gC, device=dev), torch.zeros(gC, device=dev)
    la = _lib.LayerNormBwdArgs()
    la.rows, la.D, la.rows_per_mod, la.dgamma, la.dbeta = rows, D, N, 16, 16
    ops = {
        "segsum_bias": (lambda: T.segsum(dy), 2 * rows * D, lib.dwm_segsum_ordered_floats(rows, D, rows)),
        "segsum_gate_per_image": (lambda: T.segsum(x, dy, rows_per_group=N), 4 * rows * D, lib.dwm_segsum_ordered_floats(rows, D, N)),
        "segsum_diff": (lambda: T.segsum_diff(dy, x, y2, rows_per_group=rows), 6 * rows * D, lib.dwm_segsum_diff_ordered_floats(rows, D, rows)),
        "layernorm_bwd_mod": (lambda: T.layernorm_bwd(x, dy, eps=1e-6, scale=mod, rows_per_mod=N, dgamma=dg, dbeta=db, grad_per_group=True),
                              6 * rows * D, lib.dwm_layernorm_bwd_ordered_floats(la)),
        "rmsnorm_heads_bwd": (lambda: T.rmsnorm_heads_bwd_(qk, rinv, wq, dqk, dw), 12 * rows * D,
                              lib.dwm_rmsnorm_heads_bwd_ordered_floats(rows, 2 * D)),
        "groupnorm_bwd": (lambda: T.groupnorm_bwd(gx, gdz, gI, gP, gam, bet, 32, 1e-5, gdg, gdb), 10 * gI * gP * gC,
                          lib.dwm_groupnorm_bwd_ordered_floats(gI, gP, gC)),
    }
    lines = []
    for name, (fn, in_bytes, ws_floats) in ops.items():
        ms = {m: [] for m in MODES}
        for it in range(3 + a.reps):
            for m in MODES:
                with T.ordered_reductions(m == "deterministic"):
                    t, _ = _timed(fn)
                if it >= 3:
                    ms[m].append(t)
        med = {m: sorted(v)[len(v) // 2] * 1e3 for m, v in ms.items()}
        lines.append({"op": name, "default_us_median": med["default"], "ordered_us_median": med["deterministic"],
                      "default_us_min": min(ms["default"]) * 1e3, "ordered_us_min": min(ms["deterministic"]) * 1e3,
                      "ordered_over_default": med["deterministic"] / med["default"], "kernel_traffic_MB": in_bytes / 1e6,
                      "workspace_MB": 4 * ws_floats / 1e6, "workspace_share_of_traffic": 4 * ws_floats / in_bytes, "reps": a.reps,
                      "device": torch.cuda.get_device_name(0)})
    _write(a.out, "deterministic_kernels.log", lines)


def _write(out, name, lines) -> None:
    os.makedirs(out, exist_ok=True)
    path = os.path.join(out, name)
    with open(path, "w") as f:
        for ln in lines:
            print(json.dumps(ln))
            f.write(json.dumps(ln) + "\n")
    print(f"written {path}")


def steps(a) -> None:
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
    trainers = {m: CTSDTrainer(model, lr=1e-5, weight_decay=0.01, deterministic=m == "deterministic") for m in MODES}
    trainers["deterministic"].optimizer = trainers["default"].optimizer
    w = bench.WORKLOAD
    cond = {k: (v[:w["B"]] if torch.is_tensor(v) else v) for k, v in bench.make_conditions(dev, seed=0).items()}
    latents = torch.randn(w["B"], w["T"], w["V"], w["C"], w["H"], w["W"], device=dev, generator=torch.Generator(device="cuda").manual_seed(0))
    gen = torch.Generator().manual_seed(1234)

    ms = {m: [] for m in MODES}
    peak = {m: 0 for m in MODES}
    losses = {m: [] for m in MODES}
    for it in range(a.warmup + a.steps):
        for m in MODES:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            t, loss = _timed(lambda: trainers[m].train_step(latents, cond, generator=gen))
            losses[m].append(float(loss))
            if it >= a.warmup:
                ms[m].append(t)
                peak[m] = max(peak[m], torch.cuda.max_memory_allocated(dev))
    tag = "full" if a.layers is None else f"layers{a.layers}"
    base = {"layers": kwargs["num_layers"], "steps": a.steps, "warmup": a.warmup,
            "workload": [w[k] for k in ("B", "T", "V", "C", "H", "W")], "device": torch.cuda.get_device_name(0)}
    lines = []
    for m in MODES:
        t = ms[m]
        lines.append({"mode": m, **base, "ms_per_step_mean": sum(t) / len(t), "ms_per_step_min": min(t), "ms_per_step_max": max(t),
                      "ms_per_step": t, "peak_GiB": peak[m] / 2 ** 30, "loss_first": losses[m][0], "loss_last": losses[m][-1],
                      "finite": all(x == x and abs(x) != float("inf") for x in losses[m])})
    d, o = lines[0]["ms_per_step_mean"], lines[1]["ms_per_step_mean"]
    lines.append({"summary": "deterministic against default, alternated in one process", "default_ms": d, "deterministic_ms": o,
                  "deterministic_over_default": o / d, "extra_ms_per_step": o - d, "peak_GiB_default": lines[0]["peak_GiB"],
                  "peak_GiB_deterministic": lines[1]["peak_GiB"]})
    _write(a.out, f"deterministic_{tag}.log", lines)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None, help="truncate the model to N layers (a short run)")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernels", action="store_true", help="time the five reductions in isolation instead of train steps")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles"))
    a = ap.parse_args()
    kernels(a) if a.kernels else steps(a)


if __name__ == "__main__":
    main()
