"""Measurements of the fused VAE mid-block attention (ops.vae_attention, csrc/vae_attention.hip) next to the GEMM route it
complements, all bf16 at C = 512.  Device events, every shape warmed up, the two routes ALTERNATED in one process.  One JSON line per
measurement, printed and appended to --out (default profiles/vae_attention_kernel.log).

    python scripts/measure_vae_attention.py --kernels [--iters 20]
        (I, P) = (8, 1792): one decode chunk of the headline config, both routes; (18, 836): 3 views x 6 frames of the
        interactive-generation config, fused only (the GEMM route does not take it); (6, 6360): a 480 x 848 decode, fused only.
        "fused": the one launch of dwm_vae_attention.  "gemm_core": what it replaces on the GEMM route - per image the score GEMM,
        softmax_rows and the P.V GEMM (3 I launches; V^T is prepared outside the timed region, as the v projection is on the fused
        route).  "block_*": the whole _VaeAttention.run (GroupNorm, projections, attention, out projection) by each route.
        TFLOP/s = 4 I P^2 C / t; share of the 2.5 PF dense bf16 peak.
    python scripts/measure_vae_attention.py --decode [--decode-iters 5]
        AutoencoderKL.decode at the released widths: 96 latents of 32 x 56 by both routes, 18 latents of 22 x 38 (fused).
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0          # MI355X dense bf16
C = 512
bf16 = torch.bfloat16
OUT = None


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


def stats(ts, flop=None) -> dict:
    mean = sum(ts) / len(ts)
    r = {"iters": len(ts), "ms_min": min(ts), "ms_mean": mean, "ms_max": max(ts)}
    if flop is not None:
        r["TFLOP_per_s_mean"] = flop / (mean * 1e-3) / 1e12
        r["TFLOP_per_s_best"] = flop / (min(ts) * 1e-3) / 1e12
        r["share_of_bf16_peak_mean"] = r["TFLOP_per_s_mean"] / PEAK_BF16_TFLOPS
    return r


def measure_kernels(iters: int) -> None:
    from opendwm_amd import ops
    from opendwm_amd.vae import _VaeAttention, mid_attention_route
    dev = torch.device("cuda:0")
    attn = _VaeAttention(C).to(dev).to(bf16).eval()
    for I, P, what in ((8, 1792, "one decode chunk of the headline config"), (18, 836, "3 views x 6 frames, interactive config"),
                       (6, 6360, "a 480 x 848 decode")):
        g = torch.Generator(device="cpu").manual_seed(P)
        qkv = torch.randn(I * P, 3 * C, generator=g).to(bf16).to(dev)
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        x = torch.randn(I * P, C, generator=g).to(bf16).to(dev)
        out = torch.empty(I * P, C, dtype=bf16, device=dev)
        both = mid_attention_route(P, C, bf16, "auto") == "gemm"
        flop = 4.0 * I * P * P * C
        fns = {"fused": lambda: ops.vae_attention(q, k, v, out, I, P, C ** -0.5),
               "block_fused": lambda: attn.run(x, I, P, "fused")}
        if both:
            kc = k.contiguous()
            vt = [v[i * P:(i + 1) * P].t().contiguous() for i in range(I)]
            s = torch.empty(P, P, dtype=bf16, device=dev)
            o2 = torch.empty(I * P, C, dtype=bf16, device=dev)

            def gemm_core():
                for i in range(I):
                    sl = slice(i * P, (i + 1) * P)
                    ops.gemm(q[sl], kc[sl], out=s, w_is_activation=True)
                    ops.softmax_rows(s, C ** -0.5, out=s)
                    ops.gemm(s, vt[i], out=o2[sl], w_is_activation=True)
            fns["gemm_core"] = gemm_core
            fns["block_gemm"] = lambda: attn.run(x, I, P, "gemm")
        with torch.no_grad():
            ts = alternate(fns, iters)
            rec = {"measurement": "kernel", "I": I, "P": P, "C": C, "dtype": "bf16", "what": what, "flop": flop,
                   "routes": "both" if both else "fused only"}
            for n, t in ts.items():
                rec[n] = stats(t, flop if n in ("fused", "gemm_core") else None)
            if both:
                rec["max_abs_diff_fused_vs_gemm_core"] = (out.float() - o2.float()).abs().max().item()
        emit(rec)


def measure_decode(iters: int) -> None:
    from opendwm_amd.vae import AutoencoderKL
    dev = torch.device("cuda:0")
    vae = AutoencoderKL().to(dev).to(bf16).eval()
    for n, h, w in ((96, 32, 56), (18, 22, 38)):
        z = torch.randn(n, 16, h, w, generator=torch.Generator().manual_seed(0)).to(bf16).to(dev)
        modes = ("gemm", "fused") if (h * w) % 64 == 0 and h * w <= 4096 else ("fused",)

        def run(mode):
            vae.mid_attention = mode
            return vae.decode(z, return_dict=False)[0]
        ts = alternate({m: (lambda m=m: run(m)) for m in modes}, iters, warmup=1)
        vae.mid_attention = "auto"
        emit({"measurement": "decode", "latents": n, "h": h, "w": w, "pixels_per_latent": h * w, "chunk": 8,
              **{m: stats(t) for m, t in ts.items()}})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--decode", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--decode-iters", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vae_attention_kernel.log"))
    a = ap.parse_args()
    if a.iters < 20:
        ap.error("--iters: at least 20 timed iterations per shape")
    OUT = a.out
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    from opendwm_amd import _lib
    _lib.load()
    if a.kernels:
        measure_kernels(a.iters)
    if a.decode:
        measure_decode(a.decode_iters)
