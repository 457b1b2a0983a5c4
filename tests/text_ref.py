"""Plain-PyTorch restatement of the three text encoders (CLIPTextModel, CLIPTextModelWithProjection, T5EncoderModel), written from
their definitions and working from a checkpoint-format state dict.  Any dtype / device: fp32 on the CPU it is the reference of
tests/test_text_encoders_cpu.py (pinned there against fixtures produced by the transformers classes themselves); in bf16 on the GPU
it is "what a user runs today" in scripts/measure_text_encoders.py.

`Mut` holds the mutation switches the sensitivity test flips, one at a time:
    t5_scale      multiply T5's scores by this (T5 has NO 1/sqrt(d) scale: 1.0; the mutation uses 1/8)
    clip_scale    CLIP's score scale (1/8; the mutation uses 1.0)
    bias          "ok" | "zero" | "transposed"   T5's relative-position bias
    causal        CLIP's causal mask on / off
    hidden        which entry of hidden_states is reported as `penultimate` (-2; the mutation uses -1)
    pool_shift    added to the pooled position (0; the mutation uses -1)"""
import math
from dataclasses import dataclass

import torch
import torch.nn.functional as F


@dataclass
class Mut:
    t5_scale: float = 1.0
    clip_scale: float = 0.125
    bias: str = "ok"
    causal: bool = True
    hidden: int = -2
    pool_shift: int = 0


def act(x, kind):
    if kind == "quick_gelu":
        return x * torch.sigmoid(1.702 * x)
    if kind == "gelu":
        return F.gelu(x)
    if kind in ("gelu_new", "gelu_pytorch_tanh"):
        return F.gelu(x, approximate="tanh")
    raise ValueError(kind)


def _heads(x, H):
    N, L, _ = x.shape
    return x.view(N, L, H, -1).transpose(1, 2)


def _attend(q, k, v, H, scale, add=None):
    s = _heads(q, H) @ _heads(k, H).transpose(-1, -2) * scale
    if add is not None:
        s = s + add
    o = torch.softmax(s.float(), -1).to(v.dtype) @ _heads(v, H)
    return o.transpose(1, 2).reshape(q.shape[0], q.shape[1], -1)


def t5_buckets(L, num_buckets=32, max_distance=128):
    """bidirectional relative-position buckets [L, L] (key - query), written out with integer tests instead of tensor algebra:
    per sign 16 buckets; distances 0..7 exact, 8.. logarithmic up to max_distance, the logarithm in fp32 as the released models'
    framework computes it"""
    nb = num_buckets // 2
    exact = nb // 2
    d = torch.arange(L)
    far = exact + (torch.log(d.float() / exact) / math.log(max_distance / exact) * (nb - exact)).long()
    per_distance = torch.where(d < exact, d, far.clamp(max=nb - 1))
    out = torch.empty(L, L, dtype=torch.long)
    for i in range(L):
        for j in range(L):
            out[i, j] = per_distance[abs(j - i)] + (nb if j > i else 0)
    return out


def t5(sd, cfg, ids, mut: Mut = Mut()):
    """-> dict(last_hidden_state, penultimate, hidden_states, bias [H, L, L], buckets [L, L])"""
    H, eps, n = cfg["num_heads"], cfg.get("layer_norm_epsilon", 1e-6), cfg["num_layers"]
    w = lambda name: sd[name]
    norm = lambda x, g: (x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype) * g
    L = ids.shape[1]
    buckets = t5_buckets(L, cfg.get("relative_attention_num_buckets", 32), cfg.get("relative_attention_max_distance", 128))
    table = w("encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight")
    bias = table[buckets.to(table.device)].permute(2, 0, 1)
    used = {"ok": bias, "zero": torch.zeros_like(bias), "transposed": bias.transpose(-1, -2)}[mut.bias]
    x = w("shared.weight")[ids]
    states = [x]
    for i in range(n):
        p = f"encoder.block.{i}.layer."
        y = norm(x, w(p + "0.layer_norm.weight"))
        a = _attend(y @ w(p + "0.SelfAttention.q.weight").T, y @ w(p + "0.SelfAttention.k.weight").T,
                    y @ w(p + "0.SelfAttention.v.weight").T, H, mut.t5_scale, used[None])
        x = x + a @ w(p + "0.SelfAttention.o.weight").T
        y = norm(x, w(p + "1.layer_norm.weight"))
        g = act(y @ w(p + "1.DenseReluDense.wi_0.weight").T, "gelu_new") * (y @ w(p + "1.DenseReluDense.wi_1.weight").T)
        x = x + g @ w(p + "1.DenseReluDense.wo.weight").T
        if i < n - 1:
            states.append(x)
    last = norm(x, w("encoder.final_layer_norm.weight"))
    states.append(last)
    return dict(last_hidden_state=last, penultimate=states[mut.hidden], hidden_states=states, bias=bias, buckets=buckets)


def clip(sd, cfg, ids, mut: Mut = Mut()):
    """-> dict(last_hidden_state, penultimate, pooler_output, text_embeds (if the state dict has a projection), hidden_states)"""
    H, eps, n = cfg["num_attention_heads"], cfg.get("layer_norm_eps", 1e-5), cfg["num_hidden_layers"]
    w = lambda name: sd["text_model." + name]
    ln = lambda x, p: F.layer_norm(x, x.shape[-1:], w(p + ".weight"), w(p + ".bias"), eps)
    lin = lambda x, p: x @ w(p + ".weight").T + w(p + ".bias")
    N, L = ids.shape
    x = w("embeddings.token_embedding.weight")[ids] + w("embeddings.position_embedding.weight")[:L]
    hidden = [x]
    mask = torch.full((L, L), float("-inf"), device=x.device, dtype=x.dtype).triu(1) if mut.causal else None
    for i in range(n):
        p = f"encoder.layers.{i}."
        y = ln(x, p + "layer_norm1")
        a = _attend(lin(y, p + "self_attn.q_proj"), lin(y, p + "self_attn.k_proj"), lin(y, p + "self_attn.v_proj"), H, mut.clip_scale, mask)
        x = x + lin(a, p + "self_attn.out_proj")
        y = ln(x, p + "layer_norm2")
        x = x + lin(act(lin(y, p + "mlp.fc1"), cfg.get("hidden_act", "quick_gelu")), p + "mlp.fc2")
        hidden.append(x)
    last = ln(x, "final_layer_norm")
    eos = cfg.get("eos_token_id", 49407)
    at = ids.argmax(-1) if eos == 2 else (ids == eos).int().argmax(-1)
    pooled = last[torch.arange(N, device=last.device), (at + mut.pool_shift).clamp(0, L - 1)]
    out = dict(last_hidden_state=last, penultimate=hidden[mut.hidden], pooler_output=pooled, hidden_states=hidden)
    if "text_projection.weight" in sd:
        out["text_embeds"] = pooled @ sd["text_projection.weight"].T
    return out


# ------------------------------------------------------------------------------------------------------- fixture weights
# The fixtures (tests/golden/text_encoders_*.pt) hold config, token ids, the outputs of the transformers classes and a SHA-256 of
# the weights those classes ran on, not the weights themselves (0.9 - 1.4 MB per model in bf16, over the size limit for a
# committed file): the weights are rebuilt here from a seed, as oracle.ctsd_oracle.make_state_dict does for the other models, and
# `state_dict_digest` proves that the rebuilt ones are bit for bit those of the generator run.  The scales are chosen so that the
# fixtures are not blind (score standard deviation ~2, a relative-position bias of standard deviation 2, norm weights 1 +- 0.2,
# nonzero biases): with a default initialisation every logit is ~0 and a wrong scale or a missing bias passes.
def _randn(g, *shape, std=1.0, mean=0.0):
    return (torch.randn(*shape, generator=g) * std + mean).to(torch.bfloat16)


def make_t5_state_dict(cfg, seed):
    """bf16 state dict of a T5EncoderModel under the checkpoint key names (both names of the tied embedding)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    D, H, Fd = cfg["d_model"], cfg["num_heads"], cfg["d_ff"]
    inner = H * cfg["d_kv"]
    qk = math.sqrt(2.0 / (8.0 * D))                       # score = sum over 64 of q k, q = y W_q: standard deviation 8 D std^2 = 2
    sd = {"shared.weight": _randn(g, cfg["vocab_size"], D)}
    sd["encoder.embed_tokens.weight"] = sd["shared.weight"]
    for i in range(cfg["num_layers"]):
        p = f"encoder.block.{i}.layer."
        sd[p + "0.SelfAttention.q.weight"] = _randn(g, inner, D, std=qk)
        sd[p + "0.SelfAttention.k.weight"] = _randn(g, inner, D, std=qk)
        sd[p + "0.SelfAttention.v.weight"] = _randn(g, inner, D, std=D ** -0.5)
        sd[p + "0.SelfAttention.o.weight"] = _randn(g, D, inner, std=0.5 * inner ** -0.5)
        if i == 0:
            sd[p + "0.SelfAttention.relative_attention_bias.weight"] = _randn(g, cfg["relative_attention_num_buckets"], H, std=2.0)
        sd[p + "0.layer_norm.weight"] = _randn(g, D, std=0.2, mean=1.0)
        sd[p + "1.DenseReluDense.wi_0.weight"] = _randn(g, Fd, D, std=D ** -0.5)
        sd[p + "1.DenseReluDense.wi_1.weight"] = _randn(g, Fd, D, std=D ** -0.5)
        sd[p + "1.DenseReluDense.wo.weight"] = _randn(g, D, Fd, std=0.5 * Fd ** -0.5)
        sd[p + "1.layer_norm.weight"] = _randn(g, D, std=0.2, mean=1.0)
    sd["encoder.final_layer_norm.weight"] = _randn(g, D, std=0.2, mean=1.0)
    return sd


def make_clip_state_dict(cfg, seed, projection=True):
    """bf16 state dict of a CLIPTextModel(WithProjection) under the checkpoint key names (`text_model.` prefix)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    D, Fd = cfg["hidden_size"], cfg["intermediate_size"]
    qk = math.sqrt(1.5 / D)                                # score = (1/8) sum over 64 of q k: standard deviation ~ D std^2 (+ biases) ~ 2
    t = "text_model."
    sd = {t + "embeddings.token_embedding.weight": _randn(g, cfg["vocab_size"], D),
          t + "embeddings.position_embedding.weight": _randn(g, cfg["max_position_embeddings"], D, std=0.5)}
    for i in range(cfg["num_hidden_layers"]):
        p = f"{t}encoder.layers.{i}."
        for name, std, bstd in (("k_proj", qk, 0.3), ("v_proj", D ** -0.5, 0.1), ("q_proj", qk, 0.3), ("out_proj", 0.5 * D ** -0.5, 0.1)):
            sd[p + f"self_attn.{name}.weight"] = _randn(g, D, D, std=std)
            sd[p + f"self_attn.{name}.bias"] = _randn(g, D, std=bstd)
        sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"] = _randn(g, D, std=0.2, mean=1.0), _randn(g, D, std=0.1)
        sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"] = _randn(g, Fd, D, std=D ** -0.5), _randn(g, Fd, std=0.2)
        sd[p + "mlp.fc2.weight"], sd[p + "mlp.fc2.bias"] = _randn(g, D, Fd, std=0.5 * Fd ** -0.5), _randn(g, D, std=0.1)
        sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"] = _randn(g, D, std=0.2, mean=1.0), _randn(g, D, std=0.1)
    sd[t + "final_layer_norm.weight"], sd[t + "final_layer_norm.bias"] = _randn(g, D, std=0.2, mean=1.0), _randn(g, D, std=0.1)
    if projection:
        sd["text_projection.weight"] = _randn(g, cfg["projection_dim"], D, std=D ** -0.5)
    return sd


def state_dict_digest(sd):
    """SHA-256 over the sorted key names and the raw bf16 bytes"""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].contiguous().view(torch.int16).numpy().tobytes())
    return h.hexdigest()
