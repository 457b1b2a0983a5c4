"""Time the text encoders at their real sizes (random weights): CLIP-L 12 x 768, CLIP-G 32 x 1280, T5-XXL 24 x 4096 / 10240, 77 tokens,
for 12 sequences (one streaming prompt refresh) and 192 (the headline geometry's flat prompt list under CFG).

    python scripts/measure_text_encoders.py [--log profiles/text_encoders_mi355x.log] [--reps 5] [--only clip_l,clip_g,t5]

Per encoder and in total: ms per encode on the HIP path (device events, warm, median of --reps) with dedupe off (every row) and on
(the distinct rows of a prompt list in which half the rows are the empty prompt and the rest repeat a few prompts), the share of
that time spent inside ops.gemm (a separate pass with an event pair around every GEMM), and beside it the same encoder as
tests/text_ref.py in bf16 through torch on the same GPU - what a user runs today.  The two sides are ALTERNATED rep by rep in one
process.  Also checks that dedupe on / off are bit-equal at these sizes.  No pass / fail threshold on time.

    python scripts/measure_text_encoders.py --fp32 [--log profiles/text_encoders_fp32_mi355x.log] [--reps 3] [--only ...]

The fp32 accuracy path as the yardstick: per encoder, at 12 and 192 prompts, ms per fp32 encode (every row, warm, median of --reps),
the bytes each model holds (weights, plus operand planes in fp32, plus scratch on the NF4 "dequant" route), and the relative
Frobenius error of the bf16 model and of both NF4 routes AGAINST THE FP32 DEVICE RUN, per output tensor.  All four models hold the
same weight values: random weights are drawn once, rounded to bf16, and the fp32 model is loaded from those rounded values - so
the figures are the cost of bf16 arithmetic (and of the 4-bit codes), not of rounding the checkpoint.  First measurements: there
is nothing earlier to compare them with.  No thresholds."""
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
from tests import text_ref as R  # noqa: E402

bf16 = torch.bfloat16
CONFIGS = {
    "clip_l": ("clip", dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, projection_dim=768, num_hidden_layers=12,
                            num_attention_heads=12, hidden_act="quick_gelu", eos_token_id=2)),
    "clip_g": ("clip", dict(vocab_size=49408, hidden_size=1280, intermediate_size=5120, projection_dim=1280, num_hidden_layers=32,
                            num_attention_heads=20, hidden_act="gelu", eos_token_id=2)),
    "t5": ("t5", dict(vocab_size=32128, d_model=4096, d_kv=64, d_ff=10240, num_layers=24, num_heads=64, feed_forward_proj="gated-gelu")),
}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def prompt_ids(n, vocab, distinct, seed):
    """[n, 77]: the first half one "empty prompt" row, the rest cycling through `distinct` prompts; the largest id closes each row"""
    g = torch.Generator().manual_seed(seed)
    rows = torch.randint(3, vocab - 1, (distinct + 1, 77), generator=g)
    rows[:, 40:] = vocab - 1
    rows[0, 2:] = vocab - 1
    pick = torch.cat([torch.zeros(n // 2, dtype=torch.long), 1 + torch.arange(n - n // 2) % distinct])
    return rows[pick]


def gemm_share(run):
    """fraction of the device time of run() spent inside ops.gemm"""
    events, real = [], ops.gemm

    def wrapped(*a, **k):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        out = real(*a, **k)
        e.record()
        events.append((s, e))
        return out

    ops.gemm = wrapped
    try:
        total, _ = timed(run)
    finally:
        ops.gemm = real
    torch.cuda.synchronize()
    return sum(s.elapsed_time(e) for s, e in events) / total


def outputs(kind, model, ids):
    """{name: tensor} of what the reference reads off the encoder"""
    o = model(ids, output_hidden_states=True)
    if kind == "t5":
        return dict(last_hidden_state=o.last_hidden_state)
    return dict(last_hidden_state=o.last_hidden_state, penultimate=o.hidden_states[-2], text_embeds=o.text_embeds,
                pooler_output=o.pooler_output)


def measure_fp32(args, dev, say):
    f32 = torch.float32
    say(f"# text encoders, fp32 accuracy path on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d')}; "
        f"77 tokens, random weights")
    say("# every model of an encoder holds the SAME weight values: drawn once, rounded to bf16; the fp32 model is loaded from the rounded")
    say("# values, so only the arithmetic (bf16) and the quantisation (NF4) differ.  rel = relative Frobenius error against the fp32")
    say(f"# device run.  ms: one fp32 encode of every row, warm, median of {args.reps}.  First measurements; no thresholds.")
    for name in args.only.split(","):
        kind, cfg = CONFIGS[name]
        cls = E.T5EncoderModel if kind == "t5" else E.CLIPTextModelWithProjection
        with torch.device(dev):
            seed = cls(cfg)
        sd = {k: v.detach().to(bf16) for k, v in seed.state_dict().items()}
        del seed
        with torch.device(dev):
            m32 = cls(cfg)
        m32.load_state_dict(sd)
        m32 = m32.to(f32).requires_grad_(False)
        vocab = cfg["vocab_size"]
        idsets = {n: prompt_ids(n, vocab, distinct, n) for n, distinct in ((12, 2), (192, 8))}
        want = {}
        for n, ids in idsets.items():
            want[n] = {k: v.double() for k, v in outputs(kind, m32, ids).items()}
            uniq, index = E.dedupe_rows(ids)
            first = next(iter(want[n]))
            assert torch.equal(outputs(kind, m32, uniq)[first].index_select(0, index.to(dev)).double(), want[n][first]), \
                "fp32: dedupe on / off are not bit-equal"
            ts = [timed(lambda: outputs(kind, m32, ids))[0] for _ in range(args.reps)]
            say(f"{name:8s} fp32          N={n:4d} | {statistics.median(ts):9.2f} ms per encode | holds {m32.held_bytes() / 2 ** 30:7.2f} GiB "
                f"(weights + operand planes); dedupe on / off bit-equal")
        del m32
        torch.cuda.empty_cache()
        routes = [("bf16", None)] + [(f"nf4 {r}", dict(load_in_4bit=True, bnb_4bit_quant_type="nf4", route=r)) for r in E.NF4_ROUTES]
        for label, qc in routes:
            with torch.device(dev):
                m = cls(cfg, quantization_config=qc)
            m.load_state_dict(sd)
            m = m.to(bf16).requires_grad_(False)
            for n, ids in idsets.items():
                got = outputs(kind, m, ids)
                errs = "  ".join(f"{k} {float((got[k].double() - w).norm() / w.norm()):.3e}" for k, w in want[n].items())
                say(f"{name:8s} {label:13s} N={n:4d} | rel vs fp32: {errs} | holds {m.held_bytes() / 2 ** 30:7.2f} GiB")
            del m, got
            torch.cuda.empty_cache()
        del sd, want
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--only", default="clip_l,clip_g,t5")
    ap.add_argument("--fp32", action="store_true", help="measure the fp32 accuracy path and the bf16 / NF4 errors against it")
    args = ap.parse_args()
    if args.log is None:
        args.log = os.path.join(ROOT, "profiles", "text_encoders_fp32_mi355x.log" if args.fp32 else "text_encoders_mi355x.log")
    if args.reps is None:
        args.reps = 3 if args.fp32 else 5
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.fp32:
        measure_fp32(args, dev, say)
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")
        return
    say(f"# text encoders on {torch.cuda.get_device_name(0)}, torch {torch.__version__}, {time.strftime('%Y-%m-%d')}; ms per encode, "
        f"median of {args.reps} alternated reps, 77 tokens")
    say("# encoder   N  rows  | hip ms  gemm share | torch bf16 ms | hip / torch")
    totals = {}
    for name in args.only.split(","):
        kind, cfg = CONFIGS[name]
        with torch.device(dev):
            model = (E.T5EncoderModel(cfg) if kind == "t5" else E.CLIPTextModelWithProjection(cfg))
        model = model.to(bf16).requires_grad_(False)
        vocab = cfg["vocab_size"]
        hip = (lambda ids: model(ids)[0]) if kind == "t5" else (lambda ids: model(ids, output_hidden_states=True).hidden_states[-2])
        hip(prompt_ids(2, vocab, 1, 0))                             # packs the operands; the parameters become views of them
        sd = model.state_dict()
        ref = (lambda ids: R.t5(sd, model.config, ids.to(dev))["last_hidden_state"]) if kind == "t5" else \
              (lambda ids: R.clip(sd, model.config, ids.to(dev))["penultimate"])
        for n, distinct in ((12, 2), (192, 8)):
            ids = prompt_ids(n, vocab, distinct, n)
            uniq, index = E.dedupe_rows(ids)
            full = hip(ids)
            assert torch.equal(hip(uniq).index_select(0, index.to(dev)), full), "dedupe on / off are not bit-equal"
            e = float((full.float() - ref(ids).float()).norm() / ref(ids).float().norm())
            for label, rows in (("all", ids), ("dedupe", uniq)):
                hip(rows), ref(rows)                                # warm
                th, tt = [], []
                for _ in range(args.reps):
                    th.append(timed(lambda: hip(rows))[0])
                    tt.append(timed(lambda: ref(rows))[0])
                mh, mt = statistics.median(th), statistics.median(tt)
                share = gemm_share(lambda: hip(rows))
                totals.setdefault((n, label), [0.0, 0.0])
                totals[(n, label)][0] += mh
                totals[(n, label)][1] += mt
                say(f"{name:8s} {n:4d} {rows.shape[0]:5d} ({label:6s}) | {mh:8.2f}  {share:6.2f}     | {mt:10.2f}    | {mh / mt:5.2f}")
            say(f"#   {name} N={n}: hip vs torch-bf16 restatement rel diff {e:.2e}; dedupe on / off bit-equal")
        del model, sd
        torch.cuda.empty_cache()
    for (n, label), (mh, mt) in sorted(totals.items()):
        say(f"total    {n:4d}       ({label:6s}) | {mh:8.2f}             | {mt:10.2f}    | {mh / mt:5.2f}")
    os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
    with open(args.log, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
