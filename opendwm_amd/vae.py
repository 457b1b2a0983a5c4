"""MI355X-native decoder of diffusers' AutoencoderKL (the SD 3 / 3.5 VAE the CTSD pipeline
decodes with: src/dwm/pipelines/ctsd.py:953-964 construction, :1634-1640 decode call through
dwm.functional.memory_efficient_split_call, src/dwm/functional.py:184-193).

Module tree / state-dict keys follow diffusers 0.31.0 (decoder.conv_in, decoder.mid_block.resnets.N,
decoder.mid_block.attentions.0.{group_norm,to_q,to_k,to_v,to_out.0}, decoder.up_blocks.N.resnets.M,
decoder.up_blocks.N.upsamplers.0.conv, decoder.conv_norm_out, decoder.conv_out) so a released
`vae/diffusion_pytorch_model.safetensors` loads with strict=True.  Activations are token-major [I*H*W, C] bf16; every 3x3 convolution is an
implicit GEMM of dwm_gemm_bf16 over a zero-padded token grid; GroupNorm+SiLU, the nearest
upsample and the mid-block softmax are HIP kernels (csrc/vae.hip); at image sizes the softmax route does not take, the mid-block
attention is one fused kernel (csrc/vae_attention.hip), so any size encodes and decodes."""
from __future__ import annotations

import types
from typing import Optional

import torch
from torch import nn

from . import ops
from .blocks import STORE, _bf, drop_caches
from .ops import EPI_RESID, PaddedGrid

bf16 = torch.bfloat16


def _weights_key(*tensors) -> tuple:
    """memo key of packs of a frozen model: the weights as they are now, not the optimizer step (a state-dict load or `.to()`
    rebuilds them, a training step of another model does not)"""
    return tuple((t.data_ptr(), t._version) for t in tensors)


def _conv3_w(conv: nn.Conv2d, k_pad: Optional[int] = None) -> torch.Tensor:
    """[N, C, 3, 3] -> tap-major [N, 9*Cp] (channels zero-padded to Cp for K granularity 64)."""
    w = _bf(conv.weight)
    n, c = w.shape[:2]
    cp = k_pad or c
    t = torch.zeros((n, 3, 3, cp), dtype=w.dtype, device=w.device)
    t[..., :c] = w.permute(0, 2, 3, 1)
    return t.reshape(n, 9 * cp).contiguous()


class ResnetBlock2D(nn.Module):
    """diffusers ResnetBlock2D(temb_channels=None, groups=32, eps=1e-6, output_scale_factor=1)."""

    def __init__(self, in_channels: int, out_channels: int, groups: int = 32, eps: float = 1e-6):
        super().__init__()
        self.groups, self.eps = groups, eps
        self.norm1 = nn.GroupNorm(groups, in_channels, eps=eps)
        self.conv1 = nn.Conv2d(in_channels, out_channels, 3, padding=1)
        self.norm2 = nn.GroupNorm(groups, out_channels, eps=eps)
        self.conv2 = nn.Conv2d(out_channels, out_channels, 3, padding=1)
        self.conv_shortcut = nn.Conv2d(in_channels, out_channels, 1) if in_channels != out_channels else None

    def packed(self):
        convs = [c for c in (self.conv1, self.conv2, self.conv_shortcut) if c is not None]

        def make():
            pk = {"w1": _conv3_w(self.conv1), "w2": _conv3_w(self.conv2)}
            if self.conv_shortcut is not None:
                pk["ws"] = _bf(self.conv_shortcut.weight).reshape(self.conv_shortcut.weight.shape[0], -1).contiguous()
            return pk
        # one set per compute precision (bf16 / the fp32 accuracy path)
        return STORE.memo(self, ("packed", STORE.precision), _weights_key(*(c.weight for c in convs)), make, per_step=False)

    def run(self, x: torch.Tensor, grid: PaddedGrid, scratch) -> torch.Tensor:
        pk = self.packed()
        I, P = grid.I, grid.h * grid.w
        p1 = ops.groupnorm_silu(x, I, P, _bf(self.norm1.weight), _bf(self.norm1.bias), self.groups, self.eps,
                                out=scratch(grid, x.shape[1]), out_grid=grid)
        h1 = ops.gemm(p1, pk["w1"], _bf(self.conv1.bias), a_grid=grid, conv3x3=True)
        p2 = ops.groupnorm_silu(h1, I, P, _bf(self.norm2.weight), _bf(self.norm2.bias), self.groups, self.eps,
                                out=scratch(grid, h1.shape[1]), out_grid=grid)
        sc = x if self.conv_shortcut is None else ops.gemm(x, pk["ws"], _bf(self.conv_shortcut.bias))
        return ops.gemm(p2, pk["w2"], _bf(self.conv2.bias), epilogue=EPI_RESID, res=sc, a_grid=grid, conv3x3=True, out=h1)


MID_ATTENTION_MODES = ("auto", "fused", "gemm")
GEMM_ROUTE_MAX_PIXELS = 4096          # dwm_softmax_rows holds a row of at most 4096 scores


def mid_attention_route(P: int, C: int, dtype: torch.dtype = bf16, mode: str = "auto") -> str:
    """Which route the mid-block attention takes for P pixels per image and C channels: "gemm" (per-image score GEMM, softmax_rows,
    P.V GEMM: needs P % 64 == 0 and P <= 4096) or "fused" (ops.vae_attention: any P, C in ops.VAE_ATTENTION_CHANNELS).  A pure
    function of its arguments, the same for both compute dtypes.  "auto" keeps the GEMM route wherever it applies, so whatever ran
    before the fused kernel existed runs the same code; "fused" / "gemm" force a route ("fused" with a C the kernel does not
    cover falls back to the GEMM route where that applies)."""
    if mode not in MID_ATTENTION_MODES:
        raise ValueError(f"mid_attention must be one of {MID_ATTENTION_MODES}, got {mode!r}")
    if dtype not in (bf16, torch.float32):
        raise ValueError(f"mid attention computes in bf16 or fp32, got {dtype}")
    gemm_ok = P % 64 == 0 and P <= GEMM_ROUTE_MAX_PIXELS
    fused_ok = C in ops.VAE_ATTENTION_CHANNELS
    if mode == "gemm":
        if not gemm_ok:
            raise NotImplementedError(f"VAE mid attention, mid_attention='gemm': needs pixels-per-image % 64 == 0 (GEMM K granularity) "
                                      f"and <= {GEMM_ROUTE_MAX_PIXELS} (softmax row), got {P}; mid_attention='auto' or 'fused' takes any size")
        return "gemm"
    if mode == "fused":
        if fused_ok:
            return "fused"
    elif gemm_ok:
        return "gemm"
    elif fused_ok:
        return "fused"
    if gemm_ok:                           # mode == "fused" and a C the kernel is not instantiated for
        return "gemm"
    raise NotImplementedError(f"VAE mid attention (mid_attention={mode!r}): the fused kernel covers channels in {ops.VAE_ATTENTION_CHANNELS} "
                              f"(got {C}) and the GEMM route pixels-per-image % 64 == 0 and <= {GEMM_ROUTE_MAX_PIXELS} (got {P})")


class _VaeAttention(nn.Module):
    """diffusers Attention as the VAE mid block builds it: one head of dim C, GroupNorm(32) first,
    biased q/k/v/out projections, residual connection."""

    def __init__(self, channels: int, groups: int = 32, eps: float = 1e-6):
        super().__init__()
        self.channels, self.groups, self.eps = channels, groups, eps
        self.group_norm = nn.GroupNorm(groups, channels, eps=eps)
        self.to_q = nn.Linear(channels, channels)
        self.to_k = nn.Linear(channels, channels)
        self.to_v = nn.Linear(channels, channels)
        self.to_out = nn.ModuleList([nn.Linear(channels, channels), nn.Identity()])

    def packed(self):
        """q | k | v weights [3C, C] and biases [3C] of the fused route, one set per compute precision"""
        qkv = (self.to_q, self.to_k, self.to_v)
        return STORE.memo(self, ("packed", STORE.precision), _weights_key(*(t for m in qkv for t in (m.weight, m.bias))),
                          lambda: {"w": torch.cat([_bf(m.weight) for m in qkv], 0).contiguous(),
                                   "b": torch.cat([_bf(m.bias) for m in qkv], 0).contiguous()}, per_step=False)

    def run(self, x: torch.Tensor, I: int, P: int, mode: str = "auto") -> torch.Tensor:
        Cc = self.channels
        to = self.to_out[0]
        if mid_attention_route(P, Cc, STORE.precision, mode) == "fused":
            # four launches whatever I is: GroupNorm, one q|k|v GEMM (the v bias with it), the attention kernel, the out projection
            xn = ops.groupnorm_silu(x, I, P, _bf(self.group_norm.weight), _bf(self.group_norm.bias), self.groups, self.eps,
                                    silu=False)
            pk = self.packed()
            qkv = ops.gemm(xn, pk["w"], pk["b"])                           # [I*P, 3C]
            o = torch.empty_like(x)
            ops.vae_attention(qkv[:, :Cc], qkv[:, Cc:2 * Cc], qkv[:, 2 * Cc:], o, I, P, Cc ** -0.5)
            return ops.gemm(o, _bf(to.weight), _bf(to.bias), epilogue=EPI_RESID, res=x, out=xn)
        xn = ops.groupnorm_silu(x, I, P, _bf(self.group_norm.weight), _bf(self.group_norm.bias), self.groups, self.eps,
                                silu=False)
        q = ops.gemm(xn, _bf(self.to_q.weight), _bf(self.to_q.bias))
        k = ops.gemm(xn, _bf(self.to_k.weight), _bf(self.to_k.bias))
        o = torch.empty_like(x)
        wv = _bf(self.to_v.weight)
        for i in range(I):
            sl = slice(i * P, (i + 1) * P)
            s = ops.gemm(q[sl], k[sl], w_is_activation=True)             # [P, P] scores
            ops.softmax_rows(s, Cc ** -0.5, out=s)
            vt = ops.gemm(wv, xn[sl], w_is_activation=True)              # V^T without bias: [C, P]
            # rows of softmax sum to 1, so P @ (V + 1 b^T) = P @ V + b^T: the v bias is the column bias here
            ops.gemm(s, vt, _bf(self.to_v.bias), out=o[sl], w_is_activation=True)
        return ops.gemm(o, _bf(to.weight), _bf(to.bias), epilogue=EPI_RESID, res=x, out=xn)      # (never into the A operand)


class _MidBlock(nn.Module):
    def __init__(self, channels: int, groups: int, eps: float, add_attention: bool):
        super().__init__()
        self.attentions = nn.ModuleList([_VaeAttention(channels, groups, eps)] if add_attention else [])
        self.resnets = nn.ModuleList([ResnetBlock2D(channels, channels, groups, eps) for _ in range(2)])


class _Upsampler(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, padding=1)


class _UpBlock(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, n_res: int, groups: int, eps: float, add_upsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_ch if j == 0 else out_ch, out_ch, groups, eps) for j in range(n_res)])
        self.upsamplers = nn.ModuleList([_Upsampler(out_ch)]) if add_upsample else None


class Decoder(nn.Module):
    def __init__(self, latent_channels: int, out_channels: int, block_out_channels, layers_per_block: int,
                 groups: int, eps: float = 1e-6, mid_block_add_attention: bool = True):
        super().__init__()
        self.groups, self.eps, self.out_channels = groups, eps, out_channels
        ch = list(block_out_channels)
        self.conv_in = nn.Conv2d(latent_channels, ch[-1], 3, padding=1)
        self.mid_block = _MidBlock(ch[-1], groups, eps, mid_block_add_attention)
        rev = ch[::-1]
        ups, prev = [], rev[0]
        for i, oc in enumerate(rev):
            ups.append(_UpBlock(prev, oc, layers_per_block + 1, groups, eps, add_upsample=i != len(rev) - 1))
            prev = oc
        self.up_blocks = nn.ModuleList(ups)
        self.conv_norm_out = nn.GroupNorm(groups, ch[0], eps=eps)
        self.conv_out = nn.Conv2d(ch[0], out_channels, 3, padding=1)


class _Downsampler(nn.Module):
    def __init__(self, channels: int):
        super().__init__()
        self.conv = nn.Conv2d(channels, channels, 3, stride=2, padding=0)


class _DownBlock(nn.Module):
    def __init__(self, in_ch: int, out_ch: int, n_res: int, groups: int, eps: float, add_downsample: bool):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock2D(in_ch if j == 0 else out_ch, out_ch, groups, eps) for j in range(n_res)])
        self.downsamplers = nn.ModuleList([_Downsampler(out_ch)]) if add_downsample else None


class Encoder(nn.Module):
    def __init__(self, in_channels: int, latent_channels: int, block_out_channels, layers_per_block: int,
                 groups: int, eps: float = 1e-6, mid_block_add_attention: bool = True):
        super().__init__()
        self.groups, self.eps = groups, eps
        ch = list(block_out_channels)
        self.conv_in = nn.Conv2d(in_channels, ch[0], 3, padding=1)
        downs, prev = [], ch[0]
        for i, oc in enumerate(ch):
            downs.append(_DownBlock(prev, oc, layers_per_block, groups, eps, add_downsample=i != len(ch) - 1))
            prev = oc
        self.down_blocks = nn.ModuleList(downs)
        self.mid_block = _MidBlock(ch[-1], groups, eps, mid_block_add_attention)
        self.conv_norm_out = nn.GroupNorm(groups, ch[-1], eps=eps)
        self.conv_out = nn.Conv2d(ch[-1], 2 * latent_channels, 3, padding=1)


class DiagonalGaussianDistribution:
    """diffusers DiagonalGaussianDistribution over the encoder moments [I, 2*latent, h, w]."""

    def __init__(self, parameters: torch.Tensor):
        self.parameters = parameters
        self.mean, logvar = torch.chunk(parameters, 2, dim=1)
        self.logvar = torch.clamp(logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        noise = torch.randn(self.mean.shape, generator=generator,
                            device=self.mean.device if generator is None or generator.device.type != "cpu" else "cpu",
                            dtype=self.mean.dtype).to(self.mean.device)
        return self.mean + self.std * noise

    def mode(self) -> torch.Tensor:
        return self.mean


class AutoencoderKL(nn.Module):
    """encode / decode stand-in for diffusers.AutoencoderKL (SD 3.5 medium VAE defaults)."""

    def __init__(self, in_channels: int = 3, out_channels: int = 3, latent_channels: int = 16,
                 block_out_channels=(128, 256, 512, 512), layers_per_block: int = 2, norm_num_groups: int = 32,
                 scaling_factor: float = 1.5305, shift_factor: Optional[float] = 0.0609,
                 use_quant_conv: bool = False, use_post_quant_conv: bool = False,
                 mid_block_add_attention: bool = True, **unused):
        super().__init__()
        # SD 2.1 VAE (diffusers defaults use_quant_conv = use_post_quant_conv = True there): 1x1 convs on the moments /
        # the latents, run as GEMMs on the 64-column padded token rows
        self.quant_conv = nn.Conv2d(2 * latent_channels, 2 * latent_channels, 1) if use_quant_conv else None
        self.post_quant_conv = nn.Conv2d(latent_channels, latent_channels, 1) if use_post_quant_conv else None
        self.encoder = Encoder(in_channels, latent_channels, block_out_channels, layers_per_block, norm_num_groups,
                               mid_block_add_attention=mid_block_add_attention)
        self.decoder = Decoder(latent_channels, out_channels, block_out_channels, layers_per_block, norm_num_groups,
                               mid_block_add_attention=mid_block_add_attention)
        self.config = types.SimpleNamespace(scaling_factor=scaling_factor, shift_factor=shift_factor,
                                            latent_channels=latent_channels, block_out_channels=tuple(block_out_channels),
                                            in_channels=in_channels, out_channels=out_channels,
                                            layers_per_block=layers_per_block, norm_num_groups=norm_num_groups)
        # torch.float32 selects the fp32 accuracy path of encode / decode (north_star's 1e-3 tolerance; the reference's CPU path,
        # BASELINE.json configs[0], decodes in fp32: ctsd.py:1189-1193, 1634-1640): fp32 activations and weights, convolutions
        # by dwm_gemm_f32, fp32 GroupNorm / softmax kernels
        self.compute_dtype = bf16
        # route of the mid-block attention of encoder and decoder, read at every encode / decode: see mid_attention_route
        self.mid_attention = "auto"

    @property
    def dtype(self):
        return self.decoder.conv_in.weight.dtype

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path: str, subfolder: Optional[str] = None, **kwargs):
        """Local-directory equivalent of diffusers' ModelMixin.from_pretrained as ctsd.py calls it
        (`vae_type.from_pretrained(path, subfolder="vae")`, src/dwm/pipelines/ctsd.py:953-959; the class is
        chosen by common_config["vae"]): reads <path>/<subfolder>/config.json and
        diffusion_pytorch_model.safetensors (or .bin)."""
        import json
        import os
        root = os.path.join(pretrained_model_name_or_path, subfolder) if subfolder else pretrained_model_name_or_path
        with open(os.path.join(root, "config.json")) as f:
            cfg = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
        model = cls(**cfg)
        st = os.path.join(root, "diffusion_pytorch_model.safetensors")
        if os.path.exists(st):
            from safetensors.torch import load_file
            sd = load_file(st)
        else:
            sd = torch.load(os.path.join(root, "diffusion_pytorch_model.bin"), map_location="cpu")
        model.load_state_dict(sd)
        return model.eval()

    def _apply(self, fn, *a, **kw):
        out = super()._apply(fn, *a, **kw)
        drop_caches(self)
        return out

    def load_state_dict(self, state_dict, *a, **kw):
        out = super().load_state_dict(state_dict, *a, **kw)
        drop_caches(self)
        return out

    def _pad_scratch(self, grid: PaddedGrid, channels: int) -> torch.Tensor:
        """zero-bordered padded buffers, reused (every producer rewrites the whole interior): one per level, channel count and
        precision, so the levels of one encode / decode do not evict each other; replaced when the image count changes"""
        dev = self.decoder.conv_in.weight.device
        return STORE.memo(self, ("scratch", grid.h, grid.w, channels, STORE.precision), (grid.I, dev),
                          lambda: torch.zeros((grid.rows, channels), dtype=STORE.precision, device=dev), per_step=False)

    @torch.no_grad()
    def encode(self, x: torch.Tensor, return_dict: bool = True, chunk: int = 8):
        """x [I, 3, H, W] in [-1, 1] -> object with .latent_dist (sample() / mode()), as ctsd.py uses it
        (ctsd.py:1213-1218 `.latent_dist.sample()`, :1689-1694 `.mode()`)."""
        if not x.is_cuda:
            raise RuntimeError("opendwm_amd VAE runs on an MI355X (HIP) device only")
        STORE.set_precision(self.compute_dtype)
        try:
            moments = torch.cat([self._encode_chunk(x[i:i + chunk]) for i in range(0, x.shape[0], chunk)], 0)
        finally:
            STORE.set_precision(bf16)
        dist = DiagonalGaussianDistribution(moments.float())
        if return_dict:
            return types.SimpleNamespace(latent_dist=dist)
        return (dist,)

    def _encode_chunk(self, x: torch.Tensor) -> torch.Tensor:
        e = self.encoder
        I, ic, H, W = x.shape
        cd = STORE.precision
        x = x.contiguous()
        if cd == torch.float32:
            x = x.float()
        elif x.dtype not in (torch.float32, bf16):
            x = x.to(bf16)
        scratch = self._pad_scratch
        grid = PaddedGrid(I, H, W)
        tok = ops.unshuffle_tokens(x, 1, 64 * ((ic + 63) // 64), dtype=cd)
        xp = ops.pad_tokens(tok, grid, out=scratch(grid, tok.shape[1]))
        h = ops.gemm(xp, _conv3_w(e.conv_in, tok.shape[1]), _bf(e.conv_in.bias), a_grid=grid, conv3x3=True)
        for db in e.down_blocks:
            for res in db.resnets:
                h = res.run(h, grid, scratch)
            if db.downsamplers is not None:
                ds = db.downsamplers[0]
                if grid.h % 2 or grid.w % 2:
                    raise NotImplementedError("VAE encoder needs even feature-map sizes at every downsample")
                hp = ops.pad_tokens(h, grid, out=scratch(grid, h.shape[1]))
                h = ops.gemm(hp, _conv3_w(ds.conv), _bf(ds.conv.bias), a_grid=grid, conv3x3=True, stride2=True)
                grid = PaddedGrid(I, grid.h // 2, grid.w // 2)
        h = e.mid_block.resnets[0].run(h, grid, scratch)
        for attn in e.mid_block.attentions:
            h = attn.run(h, I, grid.h * grid.w, self.mid_attention)
        h = e.mid_block.resnets[1].run(h, grid, scratch)
        hp = ops.groupnorm_silu(h, I, grid.h * grid.w, _bf(e.conv_norm_out.weight), _bf(e.conv_norm_out.bias), e.groups,
                                e.eps, out=scratch(grid, h.shape[1]), out_grid=grid)
        if self.quant_conv is None:
            m = ops.gemm(hp, _conv3_w(e.conv_out), _bf(e.conv_out.bias), a_grid=grid, conv3x3=True)      # [I*P, 2*latent]
        else:
            nm = self.quant_conv.weight.shape[0]
            kp = 64 * ((nm + 63) // 64)
            m64 = torch.zeros((I * grid.h * grid.w, kp), dtype=cd, device=h.device)        # K of the 1x1 conv padded to 64
            ops.gemm(hp, _conv3_w(e.conv_out), _bf(e.conv_out.bias), a_grid=grid, conv3x3=True, out=m64[:, :nm])
            wq = torch.zeros((nm, kp), dtype=cd, device=h.device)
            wq[:, :nm] = _bf(self.quant_conv.weight).reshape(nm, nm)
            m = ops.gemm(m64, wq, _bf(self.quant_conv.bias))
        return m.reshape(I, grid.h, grid.w, -1).permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def decode(self, z: torch.Tensor, return_dict: bool = False, chunk: int = 8):
        """z [I, latent_channels, h, w] -> images [I, 3, 8h, 8w] (bf16).  Returns a 1-tuple like
        diffusers' decode(..., return_dict=False)."""
        if not z.is_cuda:
            raise RuntimeError("opendwm_amd VAE runs on an MI355X (HIP) device only")
        STORE.set_precision(self.compute_dtype)
        try:
            outs = [self._decode_chunk(z[i:i + chunk]) for i in range(0, z.shape[0], chunk)]
        finally:
            STORE.set_precision(bf16)
        img = torch.cat(outs, 0)
        if return_dict:
            return types.SimpleNamespace(sample=img)
        return (img,)

    def _decode_chunk(self, z: torch.Tensor) -> torch.Tensor:
        d = self.decoder
        I, lc, h, w = z.shape
        cd = STORE.precision
        z = z.contiguous()
        if cd == torch.float32:
            z = z.float()
        elif z.dtype not in (torch.float32, bf16):
            z = z.to(bf16)
        grid = PaddedGrid(I, h, w)
        scratch = self._pad_scratch
        tok = ops.unshuffle_tokens(z, 1, 64 * ((lc + 63) // 64), dtype=cd)        # [I*h*w, 64], zero padded channels
        if self.post_quant_conv is not None:
            kp = tok.shape[1]
            wq = torch.zeros((kp, kp), dtype=cd, device=z.device)                 # output keeps the 64-column padding
            wq[:lc, :lc] = _bf(self.post_quant_conv.weight).reshape(lc, lc)
            bq = torch.zeros(kp, dtype=cd, device=z.device)
            bq[:lc] = _bf(self.post_quant_conv.bias)
            tok = ops.gemm(tok, wq, bq)
        zp = ops.pad_tokens(tok, grid, out=scratch(grid, tok.shape[1]))
        x = ops.gemm(zp, _conv3_w(d.conv_in, tok.shape[1]), _bf(d.conv_in.bias), a_grid=grid, conv3x3=True)
        x = d.mid_block.resnets[0].run(x, grid, scratch)
        for attn in d.mid_block.attentions:
            x = attn.run(x, I, h * w, self.mid_attention)
        x = d.mid_block.resnets[1].run(x, grid, scratch)
        for ub in d.up_blocks:
            for res in ub.resnets:
                x = res.run(x, grid, scratch)
            if ub.upsamplers is not None:
                up = ub.upsamplers[0]
                g2 = PaddedGrid(I, 2 * grid.h, 2 * grid.w)
                xp = ops.upsample2_padded(x, I, grid.h, grid.w, out=scratch(g2, x.shape[1]))
                x = ops.gemm(xp, _conv3_w(up.conv), _bf(up.conv.bias), a_grid=g2, conv3x3=True)
                grid = g2
        P = grid.h * grid.w
        xp = ops.groupnorm_silu(x, I, P, _bf(d.conv_norm_out.weight), _bf(d.conv_norm_out.bias), d.groups, d.eps,
                                out=scratch(grid, x.shape[1]), out_grid=grid)
        oc = d.out_channels
        w_out = _conv3_w(d.conv_out)
        wp = torch.zeros((8, w_out.shape[1]), dtype=cd, device=w_out.device)        # N padded 3 -> 8
        wp[:oc] = w_out
        bp = torch.zeros(8, dtype=cd, device=w_out.device)
        bp[:oc] = _bf(d.conv_out.bias)
        y = ops.gemm(xp, wp, bp, a_grid=grid, conv3x3=True)                          # [I*P, 8]
        return y[:, :oc].reshape(I, grid.h, grid.w, oc).permute(0, 3, 1, 2).contiguous()
