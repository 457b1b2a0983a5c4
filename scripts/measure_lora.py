"""Low-rank fine-tuning against full fine-tuning on the `bench.py --train` model and geometry (constants imported from bench.py, which
is not edited).  One JSON line per configuration; the lines of a run are kept as profiles/lora_*.log.

    python scripts/measure_lora.py [--steps 4 --warmup 2 --ranks 16 64 --bits 32]

The configurations - full fine-tuning (the parent's train step, `lora=None`), then CTSDTrainer(lora=dict(rank=r)) per rank with the
default targets - are built side by side in one process and their steps ALTERNATED (full, r16, r64, full, ...), so clocks and
neighbours are shared.  Per configuration: ms per step by device events around train_step; of that the ms between the events
around optimizer.step, lora.merge_ and lora.project_grads_; peak GiB of a step as if the configuration were alone (the peak of its
steps minus what the other configurations hold at rest); optimizer-state bytes; bytes of the checkpoint a save writes for it (the
adapter file, or for full fine-tuning the fp32 state dict by its size, which is not written)."""
import argparse
import gc
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


class Timed:
    """device events around every call of a bound method"""
    def __init__(self, obj, name):
        self.fn, self.spans = getattr(obj, name), []
        setattr(obj, name, self)

    def __call__(self, *a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = self.fn(*a, **kw)
        e1.record()
        self.spans.append((e0, e1))
        return out

    def take_ms(self) -> float:
        ms, self.spans = sum(a.elapsed_time(b) for a, b in self.spans), []
        return ms


def main(steps: int, warmup: int, ranks, bits: int) -> None:
    from opendwm_amd import _lib
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.pipeline import CTSDTrainer
    _lib.load()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    w = bench.WORKLOAD
    cond = {k: (v[:w["B"]] if torch.is_tensor(v) else v) for k, v in bench.make_conditions(dev, seed=0).items()}
    latents = torch.randn(w["B"], w["T"], w["V"], w["C"], w["H"], w["W"], device=dev, generator=torch.Generator(device="cuda").manual_seed(0))
    runs = []
    for rank in [None] + list(ranks):
        gc.collect()
        torch.cuda.synchronize()
        at_start = torch.cuda.memory_allocated(dev)
        with torch.device(dev):
            model = DiTCrossviewTemporalConditionModel(**bench.MODEL_KWARGS)
        bench.synth_init_(model, 0)
        lora = None if rank is None else dict(rank=rank, alpha=float(rank), generator=torch.Generator().manual_seed(7))
        tr = CTSDTrainer(model, lr=1e-5, weight_decay=0.01, optimizer_bits=bits, lora=lora)
        run = dict(name="full" if rank is None else f"lora_r{rank}", rank=rank, trainer=tr, gen=torch.Generator().manual_seed(1234),
                   timed=[Timed(tr.optimizer, "step")] + ([] if rank is None else [Timed(tr.lora, "merge_"), Timed(tr.lora, "project_grads_")]),
                   losses=[], ms=[], inner_ms=[], peak=0)
        for _ in range(warmup):
            run["losses"].append(float(tr.train_step(latents, cond, generator=run["gen"])))
        torch.cuda.synchronize()
        for t in run["timed"]:
            t.take_ms()
        gc.collect()
        run["held"] = torch.cuda.memory_allocated(dev) - at_start
        runs.append(run)
    held_all = sum(r["held"] for r in runs)
    for _ in range(steps):
        for run in runs:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats(dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            loss = run["trainer"].train_step(latents, cond, generator=run["gen"])
            e1.record()
            torch.cuda.synchronize()
            run["ms"].append(e0.elapsed_time(e1))
            run["inner_ms"].append(sum(t.take_ms() for t in run["timed"]))
            run["peak"] = max(run["peak"], torch.cuda.max_memory_allocated(dev) - (held_all - run["held"]))
            run["losses"].append(float(loss))
    full_ms = sum(runs[0]["ms"]) / steps
    for run in runs:
        tr = run["trainer"]
        state = sum(t.numel() * t.element_size() for st in tr.optimizer.state.values() for k, t in st.items() if k != "step")
        if tr.lora is None:
            ckpt = sum(p.numel() * p.element_size() for p in tr.model.parameters())
        else:
            with tempfile.TemporaryDirectory() as d:
                tr.save_checkpoint(d, 0)
                ckpt = os.path.getsize(os.path.join(d, "lora", "0.pth"))
        ms = sum(run["ms"]) / steps
        print(json.dumps({
            "config": run["name"], "optimizer_bits": bits, "steps": steps, "warmup": warmup, "ms_per_step": ms, "ms_per_step_min": min(run["ms"]),
            "ms_per_step_max": max(run["ms"]), "vs_full": ms / full_ms, "ms_optimizer_merge_project": sum(run["inner_ms"]) / steps,
            "peak_GiB_alone": run["peak"] / 2 ** 30, "held_at_rest_GiB": run["held"] / 2 ** 30, "optimizer_state_bytes": state,
            "checkpoint_bytes": ckpt, "adapter_bytes": 0 if tr.lora is None else tr.lora.held_bytes(),
            "adapted_weights": 0 if tr.lora is None else len(tr.lora.names),
            "trainable_parameters": sum(p.numel() for p in tr._optimized()), "parameters": sum(p.numel() for p in tr.model.parameters()),
            "loss_first": run["losses"][0], "loss_last": run["losses"][-1]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--bits", type=int, default=32)
    a = ap.parse_args()
    main(a.steps, a.warmup, a.ranks, a.bits)
