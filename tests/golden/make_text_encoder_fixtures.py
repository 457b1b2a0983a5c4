"""Fixtures of the text encoders, produced by EXECUTING the transformers classes (T5EncoderModel, CLIPTextModel,
CLIPTextModelWithProjection) on the CPU in fp32.  Needs `transformers`; never runs on the GPU machine.

    python tests/golden/make_text_encoder_fixtures.py            # writes tests/golden/text_encoders_t5.pt, text_encoders_clip.pt

Per model: config, the seed and SHA-256 of the weights (tests.text_ref.make_*_state_dict rebuilds them bit for bit - bf16 values,
i.e. rounded BEFORE the reference runs; the weights themselves would put a fixture over the size limit for a committed file), the
state-dict key set under the checkpoint names, token ids, the fp32 outputs (last_hidden_state, hidden_states[-2], pooled /
text_embeds) and `bf16_ref_err`: the relative Frobenius error of the SAME transformers model run in bf16 on the CPU against its fp32
run - the measured yardstick of the GPU tolerance (tests/test_text_encoders_gpu.py).  T5 also: the bucket-index matrix and the bias
tensor for L = 128 out of transformers' own `compute_bias`.

`build()` returns the two dictionaries without writing (tests/test_text_encoders_cpu.py re-runs it where transformers is there)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import text_ref as R  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
T5_CFG = dict(vocab_size=256, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=3, relative_attention_num_buckets=32,
              relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
CLIP_CFGS = {
    # the legacy pooling rule (eos_token_id == 2: the position of the largest id), quick-GELU: CLIP-L's form
    "l": dict(vocab_size=128, hidden_size=128, intermediate_size=256, projection_dim=96, num_hidden_layers=3, num_attention_heads=2,
              max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=2),
    # the first position equal to eos_token_id (ids above it occur elsewhere), erf-GELU: CLIP-G's form
    "g": dict(vocab_size=128, hidden_size=192, intermediate_size=384, projection_dim=96, num_hidden_layers=3, num_attention_heads=3,
              max_position_embeddings=77, hidden_act="gelu", layer_norm_eps=1e-5, eos_token_id=120),
}
SEEDS = {"t5": 11, "l": 21, "g": 31}
EOS_AT = (10, 40, 76)


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def clip_ids(cfg, seed):
    g = torch.Generator().manual_seed(seed)
    legacy = cfg["eos_token_id"] == 2
    top = cfg["vocab_size"] - 1
    ids = torch.randint(3, top if legacy else cfg["vocab_size"], (len(EOS_AT), 77), generator=g)
    for r, at in enumerate(EOS_AT):
        if legacy:
            ids[r, at:] = top                                   # EOS = the largest id, and the pad token repeats it
        else:
            ids[r] = torch.where(ids[r] == cfg["eos_token_id"], ids[r] - 1, ids[r])
            ids[r, at] = cfg["eos_token_id"]
            ids[r, at + 1:] = 0
    return ids


def _load(model, sd):
    own = model.state_dict().keys()
    if not any(k.startswith("text_model.") for k in own):       # this transformers version names CLIPTextModel's keys without the prefix
        sd = {k[len("text_model."):] if k.startswith("text_model.") else k: v for k, v in sd.items()}
    missing = model.load_state_dict({k: v.float() for k, v in sd.items()}, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    return model.eval()


def build():
    """(t5 fixture, clip fixtures).  Runs single-threaded, so that the fp32 sums do not depend on the machine's thread count."""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _build()
    finally:
        torch.set_num_threads(threads)


def _build():
    import transformers
    out_t5, out_clip = {}, {}
    with torch.no_grad():
        # ---- T5
        cfg = T5_CFG
        sd = R.make_t5_state_dict(cfg, SEEDS["t5"])
        ids = torch.randint(0, cfg["vocab_size"], (3, 77), generator=torch.Generator().manual_seed(SEEDS["t5"] + 1))
        ids[1, 30:] = 0
        ids[2, 5:] = 0                                          # pad tokens: they attend and are attended to (no mask is passed)
        tcfg = transformers.T5Config(**cfg)
        m = _load(transformers.T5EncoderModel(tcfg), sd)
        o = m(ids, output_hidden_states=True)
        attn = m.encoder.block[0].layer[0].SelfAttention
        pos = torch.arange(128)
        buckets = attn._relative_position_bucket(pos[None, :] - pos[:, None], bidirectional=True, num_buckets=32, max_distance=128)
        bias = attn.compute_bias(128, 128)[0]
        assert torch.equal(bias, attn.relative_attention_bias(buckets).permute(2, 0, 1))
        ob = m.to(torch.bfloat16)(ids, output_hidden_states=True)
        out_t5 = dict(config=cfg, seed=SEEDS["t5"], digest=R.state_dict_digest(sd), keys=sorted(sd), ids=ids,
                      last_hidden_state=o.last_hidden_state.clone(), penultimate=o.hidden_states[-2].clone(),
                      n_hidden_states=len(o.hidden_states), buckets128=buckets.to(torch.int16), bias128=bias.clone(),
                      bf16_ref_err=dict(last_hidden_state=rel(ob.last_hidden_state, o.last_hidden_state),
                                        penultimate=rel(ob.hidden_states[-2], o.hidden_states[-2])),
                      transformers_version=transformers.__version__)
        # ---- CLIP
        for name, cfg in CLIP_CFGS.items():
            sd = R.make_clip_state_dict(cfg, SEEDS[name])
            ids = clip_ids(cfg, SEEDS[name] + 1)
            ccfg = transformers.CLIPTextConfig(**cfg, bos_token_id=1, pad_token_id=0)
            m = _load(transformers.CLIPTextModelWithProjection(ccfg), sd)
            plain = _load(transformers.CLIPTextModel(ccfg), {k: v for k, v in sd.items() if k != "text_projection.weight"})
            o = m(ids, output_hidden_states=True)
            op = plain(ids, output_hidden_states=True)
            assert torch.equal(op.last_hidden_state, o.last_hidden_state)
            ob = m.to(torch.bfloat16)(ids, output_hidden_states=True)
            obp = plain.to(torch.bfloat16)(ids)
            out_clip[name] = dict(config=cfg, seed=SEEDS[name], digest=R.state_dict_digest(sd), keys=sorted(sd), ids=ids, eos_at=list(EOS_AT),
                                  last_hidden_state=o.last_hidden_state.clone(), penultimate=o.hidden_states[-2].clone(),
                                  n_hidden_states=len(o.hidden_states), pooler_output=op.pooler_output.clone(),
                                  text_embeds=o.text_embeds.clone(),
                                  bf16_ref_err=dict(last_hidden_state=rel(ob.last_hidden_state, o.last_hidden_state),
                                                    penultimate=rel(ob.hidden_states[-2], o.hidden_states[-2]),
                                                    pooler_output=rel(obp.pooler_output, op.pooler_output),
                                                    text_embeds=rel(ob.text_embeds, o.text_embeds)),
                                  transformers_version=transformers.__version__)
    return out_t5, out_clip


if __name__ == "__main__":
    t5, clip = build()
    torch.save(t5, os.path.join(HERE, "text_encoders_t5.pt"))
    torch.save(clip, os.path.join(HERE, "text_encoders_clip.pt"))
    print("T5 bf16_ref_err", t5["bf16_ref_err"])
    for k, v in clip.items():
        print("CLIP", k, "bf16_ref_err", v["bf16_ref_err"])
