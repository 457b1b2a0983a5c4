"""The frozen text encoders of `get_conditions` on the HIP path: CLIPTextModel / CLIPTextModelWithProjection (CLIP-L, CLIP-G, the
SD 2.1 CLIP) and T5EncoderModel (T5-XXL), drop-in for how the reference uses the transformers classes of the same names
(src/dwm/pipelines/ctsd.py:186-192, :205-253, :744-804): constructed from the keys of `config.json`, state-dict keys identical to
the released checkpoints' (`text_model.encoder.layers.N.self_attn.q_proj.weight`, ..., `text_projection.weight`; `shared.weight`,
`encoder.block.N.layer.0.SelfAttention.q.weight`, ..., `encoder.final_layer_norm.weight`), `.device`, `.dtype`,
`requires_grad_(False)`, and `model(input_ids, output_hidden_states=True)` returning `[0]`, `.last_hidden_state`, `.hidden_states`,
`.pooler_output`, `.text_embeds`.

Semantics, as the reference calls them (it passes `input_ids` only):
  * CLIP is causal and takes NO padding mask; T5 takes no mask at all - pad tokens attend and are attended to;
  * T5 attention has no 1/sqrt(d) scale and adds the relative-position bias of block 0 (bidirectional buckets) in every block; the
    [heads, L, L] fp32 bias is built once per L on the host (an integer table and a gather) and cached;
  * EOS pooling: `eos_token_id == 2` (the legacy configs) pools the position of the largest id, otherwise the first position equal
    to `eos_token_id`; the gather of the pooled rows is a torch.index_select (data movement).
Arithmetic: bf16 weights and activations, an fp32 residual stream updated in place by the RESID epilogue of the bf16 GEMM
(`out32`), CLIP's norms by ops.layernorm(x32=True), T5's by ops.rmsnorm_rows, attention by ops.text_attention (head width 64,
L <= 128), activations by ops.text_act; Q / K / V (and CLIP's biases, and T5's wi_0 | wi_1) are packed into one GEMM operand the
first time a model runs after loading, the parameters becoming views of the packed buffer (no second copy).  Every GEMM runs with
split_k = 1, so a row's result does not depend on how many rows the call has: encoding the distinct prompts once
(`SD3TextEncoders.encode(dedupe=True)`) is bit-equal to encoding every copy.  There is no PyTorch fallback: tensors off the device,
another head width, L > 128 or an activation the kernels do not have raise.

THE FP32 ACCURACY PATH: `model.to(device).to(torch.float32)` - the reference's `torch_dtype` load argument - selects
it for all three classes: fp32 weights, activations and residual stream, fp32 outputs.  Every linear layer is ops.gemm on fp32
operands (dwm_gemm_f32, split_k = 1 so that the row-independence above holds; the stream updates are its RESID epilogue in place),
CLIP's norms ops.layernorm on fp32, and rmsnorm_rows / text_attention / text_embed / text_act take their fp32 forms (exact fp32
contractions in the attention, library exp / erfc in the activations).  The pre-split bf16 planes of each GEMM operand
(ops.split_weight: 6 bytes per weight beside the 4 of the fp32 weight itself) are made where the operands are packed and are HELD BY
THE MODEL, in the same `_packed` entry, released with it by `.to()` / `load_state_dict`; they never enter the process-wide cache of
split_weight.  `.to(torch.bfloat16)` on the same object gives the bf16 model again, bit-equal to a freshly loaded one.
`quantization_config` is a bf16 feature: together with fp32 the forward raises NotImplementedError.  Other dtypes, and any model off
the device, raise RuntimeError.

TOKENISATION STAYS WITH THE CALLER: the tokenizers are host string code and no vocabulary files ship with this package; every
entry point here takes token ids (int64 [N, L], normally still on the host, where they are checked against the vocabulary).
Out of scope: training (the encoders are frozen in the reference), L > 128, HIP-graph capture, NF4 in fp32.

4-BIT WEIGHTS (`quantization_config`): all three classes take the dict the reference's example configs pass as
`text_encoder_load_args.quantization_config` (the key names of transformers.BitsAndBytesConfig; an object with `to_dict()` is
accepted too):
  * `load_in_4bit=True` with `bnb_4bit_quant_type="nf4"` is what is built (opendwm_amd/nf4.py); `bnb_4bit_compute_dtype` is accepted
    and IGNORED - the compute dtype here is bf16 whatever it says; fp4 (also the default of a config that names no type),
    `bnb_4bit_use_double_quant=True` and `load_in_8bit=True` raise NotImplementedError in the constructor;
  * `llm_int8_skip_modules`: name fragments of the linear layers that stay bf16; it REPLACES the default list, as in transformers.
    Defaults (transformers 4.48): T5 `["wo"]` (its `_keep_in_fp32_modules`), CLIP `["text_projection"]` (the last parameter).
    Every other nn.Linear of the encoder layers is quantised; embeddings, norms, biases and T5's relative bias table never are;
  * `route` (a key of this package): "fused" - every quantised layer is ONE ops.gemm_nf4 launch - or "dequant" - ops.nf4_dequantize
    into one bf16 scratch buffer (sized for the model's largest quantised operand, reused layer by layer in stream order), then
    the bf16 GEMM with exactly the arguments of the unquantised model.  Default "dequant", the faster one on T5-XXL at 9 rows of
    77 tokens ("fused" is faster up to ~3 rows, on CLIP up to 12).  Fixed per model, never chosen from the row count, so the
    dedupe guarantee above holds on both.  A quantised layer IS the bf16 layer on W' = bf16(code[q] * absmax): "dequant" is
    bit-equal to the unquantised model loaded with W'.
Quantisation happens where operand packing happens: at the first forward after `load_state_dict` / `.to()`; Q | K | V (and wi_0 |
wi_1) are packed first and quantised as one operand, then the bf16 storage of every quantised weight is released.  From then on
`state_dict()` shows `weight_nf4` (uint8 [N, K/2]) and `weight_absmax` (fp32 [N, K/64]) buffers in place of each quantised
`weight`.  LOADING SUCH A DICT BACK IS NOT BUILT: `load_state_dict` takes the released bf16 checkpoints only and raises a
RuntimeError that names the `weight_nf4` / `weight_absmax` keys it was given.  `.to()` and `load_state_dict` return the model to
"bf16, quantisation pending" (`.to()` by dequantising to W', which quantises back to the same codes)."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from . import ops
from ._lib import EPI_RESID

bf16 = torch.bfloat16
f32 = torch.float32


class TextEncoderOutput:
    """what the reference reads off a transformers ModelOutput: attributes, and `[i]` over the fields that are not None, in order"""

    def __init__(self, order, **fields):
        self._order = order
        self.last_hidden_state = self.hidden_states = self.pooler_output = self.text_embeds = None
        for k, v in fields.items():
            setattr(self, k, v)

    def to_tuple(self):
        return tuple(getattr(self, k) for k in self._order if getattr(self, k) is not None)

    def __getitem__(self, i):
        return getattr(self, i) if isinstance(i, str) else self.to_tuple()[i]


def t5_relative_buckets(L: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """[L, L] int64 bucket of (key position - query position), bidirectional (the T5 encoder).  Half of the buckets per sign; of
    those, half for exact distances, the rest logarithmic up to max_distance; evaluated in fp32 like the reference implementation,
    whose rounding at the bucket edges is part of the released weights' meaning."""
    rel = torch.arange(L)[None, :] - torch.arange(L)[:, None]
    nb = num_buckets // 2
    bucket = (rel > 0).to(torch.long) * nb
    dist = rel.abs()
    exact = nb // 2
    far = exact + (torch.log(dist.float() / exact) / math.log(max_distance / exact) * (nb - exact)).to(torch.long)
    far = torch.min(far, torch.full_like(far, nb - 1))
    return bucket + torch.where(dist < exact, dist, far)


def t5_relative_bias(table: torch.Tensor, L: int, num_buckets: int = 32, max_distance: int = 128) -> torch.Tensor:
    """[heads, L, L] fp32 from block 0's relative_attention_bias table [num_buckets, heads]"""
    idx = t5_relative_buckets(L, num_buckets, max_distance).to(table.device)
    return table.float()[idx].permute(2, 0, 1).contiguous()


def eos_positions(input_ids: torch.Tensor, eos_token_id: int) -> torch.Tensor:
    """the pooled position of every sequence (see the module docstring)"""
    if eos_token_id == 2:
        return input_ids.to(torch.int).argmax(-1)
    return (input_ids.to(torch.int) == eos_token_id).int().argmax(-1)


def dedupe_rows(ids: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(distinct rows [U, L], index [N] with distinct[index] == ids)"""
    distinct, index = torch.unique(ids, dim=0, return_inverse=True)
    return distinct, index


NF4_ROUTES = ("fused", "dequant")
NF4_DEFAULT_ROUTE = "dequant"        # the faster one on T5-XXL at 9 rows of 77 tokens (14.7 ms against 17.5 ms "fused"): DESIGN.md §24


def parse_quantization_config(qc, default_skip) -> Optional[dict]:
    """None, or dict(skip=[name fragments that stay bf16], route=...) from a BitsAndBytesConfig-style dict (see the module
    docstring).  Runs on the host, in the constructors."""
    if qc is None:
        return None
    qc = dict(qc.to_dict()) if hasattr(qc, "to_dict") else dict(qc)
    if qc.get("load_in_8bit"):
        raise NotImplementedError("quantization_config: load_in_8bit is not built (4-bit NF4 only)")
    if not qc.get("load_in_4bit"):
        raise ValueError("quantization_config: load_in_4bit=True is the one mode there is (pass quantization_config=None for bf16)")
    kind = qc.get("bnb_4bit_quant_type", "fp4")                       # BitsAndBytesConfig's own default
    if kind != "nf4":
        raise NotImplementedError(f"quantization_config: bnb_4bit_quant_type={kind!r} is not built; only 'nf4' is")
    if qc.get("bnb_4bit_use_double_quant"):
        raise NotImplementedError("quantization_config: bnb_4bit_use_double_quant (quantised absmax) is not built")
    route = qc.get("route", NF4_DEFAULT_ROUTE)
    if route not in NF4_ROUTES:
        raise ValueError(f"quantization_config: route must be one of {NF4_ROUTES}, got {route!r}")
    skip = qc.get("llm_int8_skip_modules")
    return dict(skip=list(default_skip if skip is None else skip), route=route)


class _Nf4Weight:
    """one quantised GEMM operand: q uint8 [N, K/2], absmax fp32 [N, K/64] (opendwm_amd/nf4.py)"""

    def __init__(self, q: torch.Tensor, absmax: torch.Tensor):
        self.q, self.absmax = q, absmax
        self.shape = (q.shape[0], 2 * q.shape[1])
        self.numel = self.shape[0] * self.shape[1]


class _F32Weight:
    """one GEMM operand of the fp32 path: the fp32 weight [N, K] and its pre-split bf16 planes [N, 3K] (ops.split_weight), which
    live exactly as long as the model's `_packed` entry that holds this object"""

    def __init__(self, w: torch.Tensor):
        self.w, self.planes = w, ops.split_weight(w, cache=False)


class _Frozen(nn.Module):
    """what the three classes share: config, `.device` / `.dtype`, the packed-operand cache and its invalidation, 4-bit weights"""
    NF4_DEFAULT_SKIP: Tuple[str, ...] = ()

    def __init__(self, defaults: dict, config: Optional[dict], kw: dict, quantization_config=None):
        super().__init__()
        cfg = dict(defaults)
        cfg.update(dict(config or {}))
        cfg.update(kw)
        self.config = cfg
        self._packed: Optional[dict] = None
        self.quantization = parse_quantization_config(quantization_config, self.NF4_DEFAULT_SKIP)
        self._quantised: List[nn.Module] = []            # the nn.Linear modules whose bf16 weight is released

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    def _apply(self, fn, *a, **k):          # .to() / .cuda() copy every parameter on its own: the packed views are gone
        self._packed = None
        self._unquantise(materialise=True)
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, state_dict, *a, **k):
        packed = sorted(key for key in state_dict if key.endswith((".weight_nf4", ".weight_absmax")))
        if packed:
            raise RuntimeError("load_state_dict: loading the state dict of a quantised model is not built - load the bf16 checkpoint "
                               f"and let the first forward quantise it; got {packed}")
        self._packed = None
        self._unquantise(materialise=False)
        return super().load_state_dict(self._checkpoint_keys(dict(state_dict)), *a, **k)

    # ---- 4-bit weights
    def _linear_groups(self):
        """tuples of module names, one per GEMM operand: the nn.Linear layers whose weights are stacked into it"""
        raise NotImplementedError

    def _stays_bf16(self, name: str) -> bool:
        return any(key == name or (key + ".") in (name + ".") for key in self.quantization["skip"])

    def _wants_nf4(self, names) -> bool:
        if self.quantization is None:
            return False
        stays = [self._stays_bf16(n) for n in names]
        if any(stays) and not all(stays):
            raise NotImplementedError(f"llm_int8_skip_modules splits {names}: they are one packed GEMM operand, quantised as a whole or not at all")
        return not stays[0]

    def quantised_modules(self) -> List[str]:
        """names of the nn.Linear layers this model's configuration quantises (host side; nothing is computed)"""
        return [n for names in self._linear_groups() if self._wants_nf4(names) for n in names]

    def _operand(self, names):
        """the GEMM operand of the layers `names`: their weights stacked into one tensor (several names; the parameters become
        views of it), as bf16 - or, where the configuration says so, quantised, the bf16 storage released"""
        mods = [self.get_submodule(n) for n in names]
        w = self._pack([m.weight for m in mods]) if len(mods) > 1 else mods[0].weight.data
        if w.dtype == f32:                              # the accuracy path (quantisation was refused by _ids)
            return _F32Weight(w)
        if not self._wants_nf4(names):
            return w
        q, absmax = ops.nf4_quantize(w.contiguous())
        r = 0
        for m in mods:
            n = m.weight.shape[0]
            m.weight = None
            m.register_buffer("weight_nf4", q[r:r + n])
            m.register_buffer("weight_absmax", absmax[r:r + n])
            self._quantised.append(m)
            r += n
        return _Nf4Weight(q, absmax)

    def _with_scratch(self, packed: dict, operands) -> dict:
        """the "dequant" route's one bf16 buffer, sized for the largest quantised operand"""
        sizes = [o.numel for o in operands if isinstance(o, _Nf4Weight)]
        if sizes and self.quantization["route"] == "dequant":
            packed["scratch"] = torch.empty(max(sizes), dtype=bf16, device=self.device)
        return packed

    def _unquantise(self, materialise: bool):
        """back to "bf16, quantisation pending": every released weight is a bf16 parameter again - holding W' (materialise), or
        uninitialised storage that load_state_dict is about to fill"""
        for m in self._quantised:
            q, absmax = m._buffers.pop("weight_nf4"), m._buffers.pop("weight_absmax")
            if materialise:
                w = ops.nf4_dequantize(q, absmax)
            else:
                w = torch.empty((q.shape[0], 2 * q.shape[1]), dtype=bf16, device=q.device)
            m.weight = nn.Parameter(w, requires_grad=False)
        self._quantised = []

    def _linear(self, x, op, bias=None, h=None):
        """x op^T (+ bias) -> bf16, or added in place into the fp32 residual stream h (which is returned).  op: a bf16 weight - the
        launches of the unquantised model - or an _Nf4Weight on the model's route; an _F32Weight: the same in fp32, x and the
        result fp32 (dwm_gemm_f32 on the planes the operand holds, never split over K)"""
        if isinstance(op, _F32Weight):
            if h is None:
                return ops.gemm(x, op.w, bias, split_k=1, w_planes=op.planes)
            return ops.gemm(x, op.w, bias, epilogue=EPI_RESID, res=h, out=h, split_k=1, w_planes=op.planes)
        if isinstance(op, _Nf4Weight):
            if self.quantization["route"] == "fused":
                return ops.gemm_nf4(x, op.q, op.absmax, bias, out32=h)
            op = ops.nf4_dequantize(op.q, op.absmax, out=self._packed["scratch"][:op.numel].view(op.shape))
        if h is None:
            return ops.gemm(x, op, bias, split_k=1)
        return ops.gemm(x, op, bias, epilogue=EPI_RESID, res=h, out32=h, mirror=False)

    def _checkpoint_keys(self, sd):
        return sd

    @staticmethod
    def _pack(params):
        """one contiguous tensor holding `params` stacked on axis 0; each parameter becomes a view of its slice"""
        buf = torch.cat([p.data for p in params], 0).contiguous()
        r = 0
        for p in params:
            p.data = buf[r:r + p.shape[0]]
            r += p.shape[0]
        return buf

    def _ids(self, input_ids):
        if input_ids.dim() != 2:
            raise RuntimeError(f"input_ids must be [N, L], got {tuple(input_ids.shape)}")
        if self.dtype not in (bf16, f32) or self.device.type != "cuda":
            raise RuntimeError("the text encoders run in bf16, or in fp32 (the accuracy path), on the HIP device "
                               "(model.to(device).to(torch.bfloat16) or .to(torch.float32)); there is no fallback")
        if self.dtype == f32 and self.quantization is not None:
            raise NotImplementedError("quantization_config (4-bit NF4 weights) together with torch.float32 is not built: quantisation is "
                                      "a bf16 feature - use .to(torch.bfloat16), or quantization_config=None for the fp32 accuracy path")
        return input_ids.to(torch.int64)

    def _snapshot(self, h):
        """the residual stream as an entry of `hidden_states`, in the model's dtype"""
        return h.clone() if self.dtype == f32 else ops.cast_bf16(h)

    def held_bytes(self) -> int:
        """bytes of device memory this model holds: parameters and buffers, and what `_packed` holds beside them (after a forward:
        the operand planes of the fp32 path, the scratch buffer of the NF4 "dequant" route)"""
        def walk(x):
            if isinstance(x, torch.Tensor):
                yield x
            elif isinstance(x, (_F32Weight, _Nf4Weight)):
                yield from walk(list(vars(x).values()))
            elif isinstance(x, (list, tuple, dict)):
                for y in (x.values() if isinstance(x, dict) else x):
                    yield from walk(y)
        storages = {t.untyped_storage().data_ptr(): t.untyped_storage().nbytes()
                    for t in walk([list(self.parameters()), list(self.buffers()), self._packed])}
        return sum(storages.values())


# ------------------------------------------------------------------------------------------------------------------- CLIP
CLIP_DEFAULTS = dict(vocab_size=49408, hidden_size=512, intermediate_size=2048, projection_dim=512, num_hidden_layers=12,
                     num_attention_heads=8, max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, eos_token_id=49407)


class _CLIPAttention(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.k_proj, self.v_proj, self.q_proj, self.out_proj = nn.Linear(D, D), nn.Linear(D, D), nn.Linear(D, D), nn.Linear(D, D)


class _CLIPMLP(nn.Module):
    def __init__(self, D, F):
        super().__init__()
        self.fc1, self.fc2 = nn.Linear(D, F), nn.Linear(F, D)


class _CLIPLayer(nn.Module):
    def __init__(self, D, F, eps):
        super().__init__()
        self.self_attn = _CLIPAttention(D)
        self.layer_norm1 = nn.LayerNorm(D, eps=eps)
        self.mlp = _CLIPMLP(D, F)
        self.layer_norm2 = nn.LayerNorm(D, eps=eps)


class _CLIPEmbeddings(nn.Module):
    def __init__(self, vocab, D, positions):
        super().__init__()
        self.token_embedding = nn.Embedding(vocab, D)
        self.position_embedding = nn.Embedding(positions, D)


class _CLIPEncoder(nn.Module):
    def __init__(self, n, D, F, eps):
        super().__init__()
        self.layers = nn.ModuleList([_CLIPLayer(D, F, eps) for _ in range(n)])


class _CLIPTextTransformer(nn.Module):
    def __init__(self, c):
        super().__init__()
        D = c["hidden_size"]
        self.embeddings = _CLIPEmbeddings(c["vocab_size"], D, c["max_position_embeddings"])
        self.encoder = _CLIPEncoder(c["num_hidden_layers"], D, c["intermediate_size"], c["layer_norm_eps"])
        self.final_layer_norm = nn.LayerNorm(D, eps=c["layer_norm_eps"])


class CLIPTextModel(_Frozen):
    """transformers.CLIPTextModel on the HIP path; `[0]` is last_hidden_state, `[1]` pooler_output.
    quantization_config: None (bf16) or the 4-bit NF4 dict of the module docstring"""
    OUTPUT_ORDER = ("last_hidden_state", "pooler_output", "hidden_states")
    NF4_DEFAULT_SKIP = ("text_projection",)

    def __init__(self, config: Optional[dict] = None, quantization_config=None, **kw):
        super().__init__(CLIP_DEFAULTS, config, kw, quantization_config)
        c = self.config
        if c["hidden_size"] != 64 * c["num_attention_heads"]:
            raise NotImplementedError(f"CLIP head width {c['hidden_size']} / {c['num_attention_heads']} is not 64")
        if c["hidden_act"] not in ops.TEXT_ACT_KINDS:
            raise NotImplementedError(f"CLIP activation {c['hidden_act']!r} is not one of {sorted(ops.TEXT_ACT_KINDS)}")
        self.text_model = _CLIPTextTransformer(c)
        self.eval()
        self.quantised_modules()                    # a skip list that splits a packed operand is refused here

    def _linear_groups(self):
        for i in range(self.config["num_hidden_layers"]):
            p = f"text_model.encoder.layers.{i}."
            yield tuple(p + f"self_attn.{n}_proj" for n in "qkv")
            yield (p + "self_attn.out_proj",)
            yield (p + "mlp.fc1",)
            yield (p + "mlp.fc2",)

    def _checkpoint_keys(self, sd):
        sd = {k: v for k, v in sd.items() if not k.endswith("position_ids")}         # a buffer of older checkpoints
        if not any(k.startswith("text_model.") for k in sd):                          # a state dict saved without the wrapper's prefix
            sd = {"text_model." + k: v for k, v in sd.items()}
        return sd

    def _operands(self):
        if self._packed is None:
            groups = list(self._linear_groups())
            layers = []
            for i, l in enumerate(self.text_model.encoder.layers):
                a = l.self_attn
                bqkv = self._pack([a.q_proj.bias, a.k_proj.bias, a.v_proj.bias])
                layers.append((self._operand(groups[4 * i]), bqkv) + tuple(self._operand(g) for g in groups[4 * i + 1:4 * i + 4]))
            more = [self._operand(g) for g in groups[4 * len(layers):]]            # text_projection, where there is one
            self._packed = self._with_scratch(dict(qkv=layers, more=more), [o for l in layers for o in l] + more)
        return self._packed

    @torch.no_grad()
    def _encode(self, input_ids, output_hidden_states):
        """(last_hidden_state [N, L, D], pooled [N, D], hidden_states or None), in the model's dtype"""
        ids = self._ids(input_ids)
        c, tm = self.config, self.text_model
        N, L = ids.shape
        D, H, eps = c["hidden_size"], c["num_attention_heads"], c["layer_norm_eps"]
        if L > c["max_position_embeddings"]:
            raise RuntimeError(f"{L} tokens exceed max_position_embeddings = {c['max_position_embeddings']}")
        pooled_at = eos_positions(ids, c["eos_token_id"]).to(self.device) + torch.arange(N, device=self.device) * L
        h = ops.text_embed(ids, tm.embeddings.token_embedding.weight, tm.embeddings.position_embedding.weight)
        x32 = self.dtype == bf16                   # bf16: the fp32 stream into bf16 norms; fp32: dwm_layernorm_f32
        states = [self._snapshot(h).view(N, L, D)] if output_hidden_states else None
        ao = torch.empty((N * L, D), dtype=self.dtype, device=self.device)
        for l, (wqkv, bqkv, wout, wfc1, wfc2) in zip(tm.encoder.layers, self._operands()["qkv"]):
            y = ops.layernorm(h, eps=eps, weight=l.layer_norm1.weight, bias=l.layer_norm1.bias, x32=x32)
            qkv = self._linear(y, wqkv, bqkv)
            ops.text_attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], ao, N, L, H, 0.125, causal=True)
            self._linear(ao, wout, l.self_attn.out_proj.bias, h)
            y = ops.layernorm(h, eps=eps, weight=l.layer_norm2.weight, bias=l.layer_norm2.bias, x32=x32, out=y)
            f = ops.text_act(self._linear(y, wfc1, l.mlp.fc1.bias), c["hidden_act"])
            self._linear(f, wfc2, l.mlp.fc2.bias, h)
            if output_hidden_states:
                states.append(self._snapshot(h).view(N, L, D))
        last = ops.layernorm(h, eps=eps, weight=tm.final_layer_norm.weight, bias=tm.final_layer_norm.bias, x32=x32)
        pooled = last.index_select(0, pooled_at)
        return last.view(N, L, D), pooled, (tuple(states) if output_hidden_states else None)

    def forward(self, input_ids, output_hidden_states: bool = False, **unused):
        last, pooled, states = self._encode(input_ids, output_hidden_states)
        return TextEncoderOutput(self.OUTPUT_ORDER, last_hidden_state=last, pooler_output=pooled, hidden_states=states)


class CLIPTextModelWithProjection(CLIPTextModel):
    """transformers.CLIPTextModelWithProjection: `[0]` is text_embeds = text_projection(pooled) (ctsd.py:792 relies on it)"""
    OUTPUT_ORDER = ("text_embeds", "last_hidden_state", "hidden_states")

    def __init__(self, config: Optional[dict] = None, quantization_config=None, **kw):
        super().__init__(config, quantization_config, **kw)
        if self.config["projection_dim"] % 8:
            raise NotImplementedError("projection_dim must be a multiple of 8")
        self.text_projection = nn.Linear(self.config["hidden_size"], self.config["projection_dim"], bias=False)

    def _linear_groups(self):
        yield from super()._linear_groups()
        yield ("text_projection",)

    def _checkpoint_keys(self, sd):
        proj = {k: v for k, v in sd.items() if k.startswith("text_projection.")}
        rest = super()._checkpoint_keys({k: v for k, v in sd.items() if k not in proj})
        return dict(rest, **proj)

    def forward(self, input_ids, output_hidden_states: bool = False, **unused):
        last, pooled, states = self._encode(input_ids, output_hidden_states)
        embeds = self._linear(pooled, self._operands()["more"][0])
        return TextEncoderOutput(self.OUTPUT_ORDER, text_embeds=embeds, last_hidden_state=last, hidden_states=states, pooler_output=pooled)


# --------------------------------------------------------------------------------------------------------------------- T5
T5_DEFAULTS = dict(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_heads=8, relative_attention_num_buckets=32,
                   relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="relu")


class _T5Norm(nn.Module):
    def __init__(self, D):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(D))


class _T5Attention(nn.Module):
    def __init__(self, D, inner, heads, buckets):
        super().__init__()
        self.q, self.k, self.v = (nn.Linear(D, inner, bias=False) for _ in range(3))
        self.o = nn.Linear(inner, D, bias=False)
        if buckets:
            self.relative_attention_bias = nn.Embedding(buckets, heads)


class _T5Dense(nn.Module):
    def __init__(self, D, F):
        super().__init__()
        self.wi_0, self.wi_1, self.wo = nn.Linear(D, F, bias=False), nn.Linear(D, F, bias=False), nn.Linear(F, D, bias=False)


class _T5Sub(nn.Module):
    def __init__(self, D, attn=None, dense=None):
        super().__init__()
        if attn is not None:
            self.SelfAttention = attn
        if dense is not None:
            self.DenseReluDense = dense
        self.layer_norm = _T5Norm(D)


class _T5Block(nn.Module):
    def __init__(self, c, first):
        super().__init__()
        D, inner = c["d_model"], c["num_heads"] * c["d_kv"]
        self.layer = nn.ModuleList([
            _T5Sub(D, attn=_T5Attention(D, inner, c["num_heads"], c["relative_attention_num_buckets"] if first else 0)),
            _T5Sub(D, dense=_T5Dense(D, c["d_ff"]))])


class _T5Stack(nn.Module):
    def __init__(self, c, shared):
        super().__init__()
        self.embed_tokens = shared
        self.block = nn.ModuleList([_T5Block(c, i == 0) for i in range(c["num_layers"])])
        self.final_layer_norm = _T5Norm(c["d_model"])


class T5EncoderModel(_Frozen):
    """transformers.T5EncoderModel on the HIP path (the gated-GELU encoders: T5 v1.1, T5-XXL); `[0]` is last_hidden_state"""
    OUTPUT_ORDER = ("last_hidden_state", "hidden_states")
    NF4_DEFAULT_SKIP = ("wo",)

    def __init__(self, config: Optional[dict] = None, quantization_config=None, **kw):
        super().__init__(T5_DEFAULTS, config, kw, quantization_config)
        c = self.config
        if c["d_kv"] != 64:
            raise NotImplementedError(f"T5 head width d_kv = {c['d_kv']} is not 64")
        act = c.get("dense_act_fn") if c.get("is_gated_act") else None
        if c["feed_forward_proj"] == "gated-gelu":
            act = "gelu_new"
        if act not in ("gelu_new", "gelu_pytorch_tanh"):
            raise NotImplementedError(f"T5 feed-forward {c['feed_forward_proj']!r}: only the gated tanh-GELU form is built")
        self.shared = nn.Embedding(c["vocab_size"], c["d_model"])
        self.encoder = _T5Stack(c, self.shared)
        self._bias: Dict[int, torch.Tensor] = {}
        self.eval()
        self.quantised_modules()

    def _linear_groups(self):
        for i in range(self.config["num_layers"]):
            a, d = f"encoder.block.{i}.layer.0.SelfAttention.", f"encoder.block.{i}.layer.1.DenseReluDense."
            yield (a + "q", a + "k", a + "v")
            yield (a + "o",)
            yield (d + "wi_0", d + "wi_1")
            yield (d + "wo",)

    def _apply(self, fn, *a, **k):
        self._bias = {}
        return super()._apply(fn, *a, **k)

    def _checkpoint_keys(self, sd):
        self._bias = {}
        a, b = "shared.weight", "encoder.embed_tokens.weight"                       # one tied table under two names
        if a in sd and b not in sd:
            sd[b] = sd[a]
        if b in sd and a not in sd:
            sd[a] = sd[b]
        return sd

    def relative_bias(self, L: int) -> torch.Tensor:
        """[heads, L, L] fp32, built at the first use of this L"""
        if L not in self._bias:
            c = self.config
            table = self.encoder.block[0].layer[0].SelfAttention.relative_attention_bias.weight
            self._bias[L] = t5_relative_bias(table, L, c["relative_attention_num_buckets"], c["relative_attention_max_distance"])
        return self._bias[L]

    def _operands(self):
        if self._packed is None:
            groups = list(self._linear_groups())
            blocks = [tuple(self._operand(g) for g in groups[4 * i:4 * i + 4]) for i in range(len(self.encoder.block))]
            self._packed = self._with_scratch(dict(blocks=blocks), [o for b in blocks for o in b])
        return self._packed

    @torch.no_grad()
    def forward(self, input_ids, output_hidden_states: bool = False, **unused):
        ids = self._ids(input_ids)
        c = self.config
        N, L = ids.shape
        D, H, eps = c["d_model"], c["num_heads"], c["layer_norm_epsilon"]
        inner = 64 * H
        bias = self.relative_bias(L)
        h = ops.text_embed(ids, self.shared.weight)
        states = [self._snapshot(h).view(N, L, D)] if output_hidden_states else None
        ao = torch.empty((N * L, inner), dtype=self.dtype, device=self.device)
        y = torch.empty((N * L, D), dtype=self.dtype, device=self.device)
        for i, (b, (wqkv, wo_attn, wi, wo)) in enumerate(zip(self.encoder.block, self._operands()["blocks"])):
            if output_hidden_states and i > 0:
                states.append(self._snapshot(h).view(N, L, D))
            ops.rmsnorm_rows(h, b.layer[0].layer_norm.weight, eps, out=y)
            qkv = self._linear(y, wqkv)
            ops.text_attention(qkv[:, :inner], qkv[:, inner:2 * inner], qkv[:, 2 * inner:], ao, N, L, H, 1.0, bias=bias)
            self._linear(ao, wo_attn, None, h)
            ops.rmsnorm_rows(h, b.layer[1].layer_norm.weight, eps, out=y)
            f = ops.text_act(self._linear(y, wi), "gelu_new", gated=True)
            self._linear(f, wo, None, h)
        last = ops.rmsnorm_rows(h, self.encoder.final_layer_norm.weight, eps).view(N, L, D)
        if output_hidden_states:
            states.append(last)                                   # as transformers: the last entry is the normed output
        return TextEncoderOutput(self.OUTPUT_ORDER, last_hidden_state=last, hidden_states=tuple(states) if output_hidden_states else None)


# ------------------------------------------------------------------------------------------------------------- SD 3 triple
class SD3TextEncoders:
    """CLIP-L, CLIP-G and T5 as `get_conditions` uses them for an SD 3 model (ctsd.py:205-253)"""

    def __init__(self, clip_l: CLIPTextModelWithProjection, clip_g: CLIPTextModelWithProjection, t5: Optional[T5EncoderModel]):
        self.clip_l, self.clip_g, self.t5 = clip_l, clip_g, t5

    @staticmethod
    def _run(fn, ids, dedupe):
        """fn(ids) -> tuple of tensors with the prompt on axis 0; dedupe: every distinct row of ids once, scattered back"""
        if not dedupe:
            return fn(ids)
        distinct, index = dedupe_rows(ids.cpu())
        outs = fn(distinct)
        index = index.to(outs[0].device)
        return tuple(o.index_select(0, index) for o in outs)

    def encode(self, ids_l: torch.Tensor, ids_g: torch.Tensor, ids_t5: Optional[torch.Tensor], dedupe: bool = True,
               joint_attention_dim: int = 4096):
        """token ids of the FLAT prompt list (conditions.flatten_clip_text) -> ([h_l, h_g], [pooled_l, pooled_g], t5_states) for
        conditions.assemble_sd3_text; h_* = hidden_states[-2], pooled_* = text_embeds.  dedupe: encode each distinct row of ids
        once (under CFG half the list is the empty prompt, and frames usually share prompts) - bit-equal to encoding every copy.
        Without a T5 encoder the T5 states are zeros [N, 77, joint_attention_dim], as ctsd.py:754-757."""
        def clip(model):
            def fn(ids):
                o = model(ids, output_hidden_states=True)
                return o.hidden_states[-2], o[0]
            return fn
        h_l, p_l = self._run(clip(self.clip_l), ids_l, dedupe)
        h_g, p_g = self._run(clip(self.clip_g), ids_g, dedupe)
        if self.t5 is None:
            t5 = torch.zeros((ids_l.shape[0], 77, joint_attention_dim), dtype=h_l.dtype, device=h_l.device)
        else:
            (t5,) = self._run(lambda ids: (self.t5(ids)[0],), ids_t5, dedupe)
        return [h_l, h_g], [p_l, p_g], t5
