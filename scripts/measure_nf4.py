"""Time the text encoders with NF4 4-bit weights against their bf16 path, at their real sizes with random weights: CLIP-L 12 x 768,
CLIP-G 32 x 1280, T5-XXL 24 x 4096 / 10240; 3, 9, 12 and 192 rows of 77 tokens.

    python scripts/measure_nf4.py [--log profiles/nf4_mi355x.log] [--reps 5] [--only clip_l,clip_g,t5] [--rows 3,9,12,192]

Three legs per encoder, the same weights in each: bf16 (the unquantised model: the path the NF4 routes are compared against), NF4
route "fused" (one ops.gemm_nf4 launch per quantised layer) and NF4 route "dequant" (ops.nf4_dequantize into a scratch buffer, then
the bf16 GEMM).  The legs are ALTERNATED rep by rep in one process and timed with device events; the figure is the median of --reps.
Also: the bytes each model holds in parameters and buffers before and after its first forward (the quantisation), the relative
difference of each NF4 leg from the bf16 leg, and per-shape times of ops.gemm_nf4 against ops.gemm for T5-XXL's four GEMM shapes at
M = 231, 693 and 924 (events around --inner back-to-back launches, median of --reps).  No pass / fail threshold on time."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from opendwm_amd import ops, text_encoders as E  # noqa: E402
from opendwm_amd._lib import EPI_RESID  # noqa: E402

bf16 = torch.bfloat16
CONFIGS = {
    "clip_l": ("clip", dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, projection_dim=768, num_hidden_layers=12,
                            num_attention_heads=12, hidden_act="quick_gelu", eos_token_id=2)),
    "clip_g": ("clip", dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, projection_dim=1280, num_hidden_layers=32,
                            num_attention_heads=20, hidden_act="gelu", eos_token_id=2)),
    "t5": ("t5", dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, feed_forward_proj="gated-gelu")),
}
LEGS = ("bf16", "fused", "dequant")
# T5-XXL's GEMMs: name, N, K, whether the result is added into the fp32 residual stream
T5_SHAPES = (("q|k|v", 12288, 4096, False), ("o", 4096, 4096, True), ("wi_0|wi_1", 20480, 4096, False), ("wo", 4096, 10240, True))


def timed(fn, inner=1):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner, out


def held_bytes(m):
    return sum(t.numel() * t.element_size() for t in list(m.parameters()) + list(m.buffers()))


def rows_of_ids(n, vocab, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, vocab - 1, (n, 77), generator=g)
    ids[:, 40:] = vocab - 1
    return ids


def nf4(route):
    return dict(load_in_4bit=True, bnb_4bit_quant_type="nf4", route=route)


def encoders(name, dev, say):
    kind, cfg = CONFIGS[name]
    cls = E.T5EncoderModel if kind == "t5" else E.CLIPTextModelWithProjection
    with torch.device(dev):
        models = {"bf16": cls(cfg).to(bf16).requires_grad_(False)}
        sd = {k: v.clone() for k, v in models["bf16"].state_dict().items()}
        for route in ("fused", "dequant"):
            m = cls(cfg, quantization_config=nf4(route)).to(bf16).requires_grad_(False)
            m.load_state_dict(sd)
            models[route] = m
    del sd
    run = {leg: ((lambda ids, m=m: m(ids)[0]) if kind == "t5" else (lambda ids, m=m: m(ids, output_hidden_states=True).hidden_states[-2]))
           for leg, m in models.items()}
    first = rows_of_ids(2, cfg["vocab_size"], 0)
    for leg in LEGS:
        before = held_bytes(models[leg])
        run[leg](first)                                             # packs (and quantises) the operands
        torch.cuda.synchronize()
        say(f"#   {name} {leg:7s}: parameters + buffers {before / 2**20:10.1f} MiB before the first forward, "
            f"{held_bytes(models[leg]) / 2**20:10.1f} MiB after")
    return cfg, run


def measure_encoders(args, dev, say):
    say("# encoder rows | bf16 ms | fused ms  fused / bf16 | dequant ms  dequant / bf16 | rel diff from bf16: fused, dequant")
    for name in args.only.split(","):
        cfg, run = encoders(name, dev, say)
        for n in [int(r) for r in args.rows.split(",")]:
            ids = rows_of_ids(n, cfg["vocab_size"], n)
            outs = {leg: run[leg](ids).float() for leg in LEGS}    # warm, and the outputs
            diff = {leg: float((outs[leg] - outs["bf16"]).norm() / outs["bf16"].norm()) for leg in ("fused", "dequant")}
            del outs
            t = {leg: [] for leg in LEGS}
            for _ in range(args.reps):
                for leg in LEGS:
                    t[leg].append(timed(lambda: run[leg](ids))[0])
            m = {leg: statistics.median(t[leg]) for leg in LEGS}
            say(f"{name:7s} {n:4d} | {m['bf16']:8.2f} | {m['fused']:8.2f}  {m['fused'] / m['bf16']:6.2f}      | {m['dequant']:8.2f}  "
                f"{m['dequant'] / m['bf16']:6.2f}        | {diff['fused']:.2e}, {diff['dequant']:.2e}")
        del run
        torch.cuda.empty_cache()


def measure_shapes(args, dev, say):
    say("# T5-XXL GEMM shapes: us per launch, ops.gemm (bf16 weights, split_k = 1 / RESID into the fp32 stream) against ops.gemm_nf4")
    say("# layer          N      K     M | bf16 us | nf4 us | nf4 / bf16 | weight MiB bf16, nf4")
    g = torch.Generator().manual_seed(1)
    for label, N, K, stream in T5_SHAPES:
        w = (torch.randn(N, K, generator=g) * K ** -0.5).to(dev).to(bf16)
        q, absmax = ops.nf4_quantize(w)
        for M in (231, 693, 924):
            a = torch.randn(M, K, generator=g).to(dev).to(bf16)
            h = torch.zeros(M, N, dtype=torch.float32, device=dev)
            if stream:
                legs = {"bf16": lambda: ops.gemm(a, w, epilogue=EPI_RESID, res=h, out32=h, mirror=False),
                        "nf4": lambda: ops.gemm_nf4(a, q, absmax, out32=h)}
            else:
                out = torch.empty(M, N, dtype=bf16, device=dev)
                legs = {"bf16": lambda: ops.gemm(a, w, out=out, split_k=1), "nf4": lambda: ops.gemm_nf4(a, q, absmax, out=out)}
            t = {k: [] for k in legs}
            for fn in legs.values():
                timed(fn, 3)                                        # warm
            for _ in range(args.reps):
                for k, fn in legs.items():
                    t[k].append(timed(fn, args.inner)[0] * 1e3)
            mb, mn = statistics.median(t["bf16"]), statistics.median(t["nf4"])
            say(f"{label:10s} {N:6d} {K:6d} {M:5d} | {mb:7.1f} | {mn:6.1f} | {mn / mb:6.2f}     | {2 * N * K / 2**20:6.1f}, "
                f"{(q.numel() + 4 * absmax.numel()) / 2**20:6.1f}")
        del w, q, absmax
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=os.path.join(ROOT, "profiles", "nf4_mi355x.log"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--only", default="clip_l,clip_g,t5")
    ap.add_argument("--rows", default="3,9,12,192")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# NF4 text encoders on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d')}; 77 tokens per row, "
        f"median of {args.reps} alternated reps, device events")
    measure_shapes(args, dev, say)
    measure_encoders(args, dev, say)
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
