"""ms per steady-state frame of frame-in / frame-out generation (drivers.StreamingDriver over pipeline.CTSDDenoiser) at the geometry of
the reference's streaming config (configs/experimental/streaming/ctsd_35_xs_df6v3_tirda_bm_nwao_streaming.json, written out below:
the reference tree is not needed): the existing driver against the persistent stream session, each eager and with the whole-step
HIP graph.  Device events around every send_frame_condition, the four modes ALTERNATED inside every iteration of one process,
random weights.  One JSON line per measurement, printed and appended to --out.

    python scripts/measure_streaming.py [--iters 12] [--warmup 3] [--out profiles/streaming_session.log]

Reported per mode: ms per steady-state frame (median, min, max), frames/s, graphs captured per frame, images the layout adapter
computed per frame; and the slide launch of the persistent session alone (dwm_fifo_slide_multi over latents, model input, every
per-frame condition and the cached adapter residuals): microseconds and TB/s of the bytes it reads and writes."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench                                    # build_model (seeded synthetic weights), make_conditions

bf16 = torch.bfloat16
OUT = None
# the streaming model: 12 joint blocks, all dual, 20 heads x 64, cross-view (row-wise) after the odd layers, temporal (point-wise)
# after every layer, implicit perspective, a 6 x 1280 layout adapter on 6-channel condition images
MODEL_KWARGS = dict(
    dual_attention_layers=list(range(12)), attention_head_dim=64, caption_projection_dim=1280, in_channels=16, joint_attention_dim=4096,
    num_attention_heads=20, num_layers=12, out_channels=16, patch_size=2, pooled_projection_dim=2048, pos_embed_max_size=384,
    qk_norm="rms_norm", qk_norm_on_additional_modules="rms_norm", sample_size=128, perspective_modeling_type="implicit",
    projection_class_embeddings_input_dim=3328, enable_crossview=True, crossview_attention_type="rowwise",
    crossview_block_layers=[1, 3, 5, 7, 9, 11], enable_temporal=True, temporal_attention_type="pointwise",
    temporal_block_layers=list(range(12)), mixer_type="AlphaBlender", merge_factor=2,
    condition_image_adapter_config=dict(in_channels=6, channels=[1280] * 6, is_downblocks=[True] + [False] * 5, num_res_blocks=2,
                                        downscale_factor=8, use_zero_convs=True))
# 3 views x 6 frames of 176 x 304 images (22 x 38 latents, 11 x 19 = 209 tokens), 24 steps (4 per frame), guidance 4, one sample
WORKLOAD = dict(B=1, T=6, V=3, C=16, H=22, W=38, text_len=154, guidance_scale=4.0, inference_steps=24)
FALLBACK_W = 40                                 # 176 x 320 images (220 tokens), if the model refuses 19-token rows
NON_TEMPORAL = ["disable_crossview", "disable_temporal", "crossview_attention_mask"]
MODES = [("existing_eager", False, False), ("existing_graph", False, True), ("persistent_eager", True, False),
         ("persistent_graph", True, True)]


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


def stats(ts) -> dict:
    return {"ms_median": round(statistics.median(ts), 3), "ms_min": round(min(ts), 3), "ms_max": round(max(ts), 3), "n": len(ts)}


def make_drivers(model, w, dev):
    from opendwm_amd.drivers import StreamingDriver
    from opendwm_amd.pipeline import CTSDDenoiser
    cfg = dict(inference_steps=w["inference_steps"], sequence_length_per_iteration=w["T"],
               autoregression_condition_exception_for_take_sequence=NON_TEMPORAL)
    shape = (w["B"], w["T"], w["V"], w["C"], w["H"], w["W"])
    drivers = {}
    for name, persistent, graph in MODES:
        den = CTSDDenoiser(model, guidance_scale=w["guidance_scale"], inference_steps=w["inference_steps"]).enable_graph(graph)
        d = StreamingDriver(den, cfg, generator=torch.Generator().manual_seed(1), persistent=persistent)
        d.reset_streaming(shape, dev)
        drivers[name] = d
    return drivers


def measure(dev, iters: int, warmup: int) -> None:
    from opendwm_amd.drivers import take_sequence_clip
    w = dict(WORKLOAD)
    model = bench.build_model(MODEL_KWARGS, dev)
    images = [0]
    real_run = model.condition_image_adapter.run

    def counting_run(x, *a, **kw):
        images[0] += x[..., 0, 0, 0].numel()
        return real_run(x, *a, **kw)
    model.condition_image_adapter.run = counting_run

    def frame_conditions(cond, i):
        return {k: (v if k in NON_TEMPORAL else take_sequence_clip(v, i % w["T"], i % w["T"] + 1)) for k, v in cond.items()}

    def fill(drivers, cond):                    # gather T frames: the last one runs the warm-up window and emits frame 0
        for d in drivers.values():
            for i in range(w["T"]):
                d.send_frame_condition(frame_conditions(cond, i))
            d.receive_frame()
        torch.cuda.synchronize()
    try:
        cond = bench.make_conditions(dev, 0, w, layout=True)
        drivers = make_drivers(model, w, dev)
        fill(drivers, cond)
    except (RuntimeError, NotImplementedError, ValueError) as e:
        emit({"what": "geometry_fallback", "refused": f"{8 * w['H']} x {8 * w['W']} images ({w['H'] // 2 * (w['W'] // 2)} tokens)",
              "error": str(e)[:300], "using": f"{8 * w['H']} x {8 * FALLBACK_W} images"})
        w["W"] = FALLBACK_W
        cond = bench.make_conditions(dev, 0, w, layout=True)
        drivers = make_drivers(model, w, dev)
        fill(drivers, cond)
    tokens = (w["H"] // 2) * (w["W"] // 2)
    emit({"what": "geometry", "layers": MODEL_KWARGS["num_layers"], "heads": MODEL_KWARGS["num_attention_heads"], "views": w["V"],
          "frames": w["T"], "image": [8 * w["H"], 8 * w["W"]], "tokens_per_image": tokens, "inference_steps": w["inference_steps"],
          "steps_per_frame": w["inference_steps"] // w["T"], "guidance": w["guidance_scale"], "weights": "random (bench.synth_init_)"})
    ts = {n: [] for n in drivers}
    per_frame = {n: {"captures": [], "adapter_images": []} for n in drivers}
    for it in range(warmup + iters):
        for n, d in drivers.items():
            fc = frame_conditions(cond, w["T"] + it)
            c0, i0 = d.denoiser.graph_captures, images[0]
            ms = timed(lambda: d.send_frame_condition(fc))
            d.receive_frame()
            if it >= warmup:
                ts[n].append(ms)
                per_frame[n]["captures"].append(d.denoiser.graph_captures - c0)
                per_frame[n]["adapter_images"].append(images[0] - i0)
    for n, t in ts.items():
        s = stats(t)
        emit({"what": "streaming_steady_frame", "mode": n, "frames_per_s": round(1e3 / s["ms_median"], 2),
              "graph_captures_per_frame": statistics.median(per_frame[n]["captures"]),
              "graph_captures_total": drivers[n].denoiser.graph_captures,
              "adapter_images_per_frame": statistics.median(per_frame[n]["adapter_images"]),
              "finite": bool(torch.isfinite(drivers[n].denoiser.latents).all()), **s})
    base, best = statistics.median(ts["existing_eager"]), statistics.median(ts["persistent_graph"])
    emit({"what": "streaming_summary", "existing_eager_ms": round(base, 3), "persistent_graph_ms": round(best, 3),
          "speedup": round(base / best, 3), "existing_eager_range_ms": round(max(ts["existing_eager"]) - min(ts["existing_eager"]), 3),
          "persistent_graph_range_ms": round(max(ts["persistent_graph"]) - min(ts["persistent_graph"]), 3)})
    # the slide launch alone (it moves real queue state, so it is measured last): bursts of back-to-back launches per event pair
    den = drivers["persistent_graph"].denoiser
    plan, reps = den._session.plan, 20

    def burst():
        for _ in range(reps):
            plan.run()
    for _ in range(3):
        burst()
    us = [timed(burst) * 1e3 / reps for _ in range(10)]
    med = statistics.median(us)
    emit({"what": "fifo_slide_launch", "buffers": len(plan.host_items), "bytes_read_and_written": plan.bytes_moved,
          "workgroups": plan.block_item.numel(), "us_median": round(med, 2), "us_min": round(min(us), 2), "us_max": round(max(us), 2),
          "TB_per_s_at_median": round(plan.bytes_moved / (med * 1e-6) / 1e12, 3), "launches_per_sample": reps})


def main():
    global OUT
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("measure_streaming.py measures on an MI355X; no HIP device found")
    OUT = a.out or os.path.join(ROOT, "profiles", "streaming_session.log")
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    dev = torch.device("cuda:0")
    from opendwm_amd import _lib
    _lib.load()
    emit({"what": "run", "device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup})
    measure(dev, a.iters, a.warmup)


if __name__ == "__main__":
    main()
