"""Training path of the CTSD MMDiT (reference: `train_step`, src/dwm/pipelines/ctsd.py:1195-1437,
forward under autocast with gradient checkpointing `:497-521`, `loss.backward()` `:1401-1404`,
optimizer `:1406-1432`; DDP wrap `:1051-1054`).

Design (MI355X-first rather than op-by-op autograd):
  * one `torch.autograd.Function` per transformer block.  By default its forward is the fused inference path
    (opendwm_amd.blocks.*.run) and keeps only the block inputs - the reference's gradient
    checkpointing; its backward re-runs the block un-fused (pre-activations are needed) and then
    walks it backwards with the hand-written HIP kernels of include/dwm_hip.h "Training".  A block
    that the model's activation_policy keeps (see "kept activations" below) runs the un-fused
    training forward as its forward, holds its kept set and goes straight to the backward walk.
  * parameters enter the Functions as inputs, so autograd's AccumulateGrad nodes - and with them
    `DistributedDataParallel`'s bucketed RCCL all-reduce - see every gradient as soon as its block
    is done; torch only orchestrates, all arithmetic on token-sized tensors is HIP.
  * master parameters may be fp32; compute copies are bf16 shadows (blocks.STORE) that the AdamW
    kernel refreshes in the same pass.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from . import ops, quant8
from . import train_ops as T
from .blocks import (STORE, AlphaBlender, JointTransformerBlock, TimestepEmbedding, VTSelfAttentionBlock, _bf, refreshable)
from .ops import ACT_GELU_TANH, ACT_SILU

bf16 = torch.bfloat16


# ------------------------------------------------------------------------------------------ helpers
class Grads:
    """fp32 gradient accumulator keyed by parameter (one block's worth)."""

    def __init__(self):
        self.g: Dict[int, torch.Tensor] = {}

    def add(self, p: Optional[torch.Tensor], g: Optional[torch.Tensor]) -> None:
        """g: bf16 or fp32, any shape with p.numel() elements"""
        if p is None or g is None or not p.requires_grad:
            return
        cur = self.g.get(id(p))
        if g.dtype == bf16:
            g2 = g.reshape(-1, g.shape[-1]) if g.dim() > 1 else g.reshape(1, -1)
            if cur is None:
                self.g[id(p)] = T.cast_f32(g2.contiguous()).view(p.shape)
            else:
                T.cast_f32(g2.contiguous(), out=cur.view(g2.shape), accumulate=True)
        else:
            g = g.reshape(p.shape).to(torch.float32)
            if cur is None:
                self.g[id(p)] = g.clone()
            else:
                cur.add_(g)

    def take(self, p: torch.Tensor) -> Optional[torch.Tensor]:
        g = self.g.get(id(p))
        if g is None:
            return None
        return g if g.dtype == p.dtype else g.to(p.dtype)


def w_t(w: torch.Tensor) -> torch.Tensor:
    """bf16 W^T [K, N] of a 2-D weight [N, K] (N % 8 == 0), cached for one optimizer step"""
    return STORE.derived(w, "T", lambda: T.transpose(_bf(w).reshape(w.shape[0], -1), rows_pad=w.shape[0]))


def lin_fwd(x: torch.Tensor, lin: torch.nn.Linear, **epi) -> torch.Tensor:
    return ops.gemm(x, _bf(lin.weight), _bf(lin.bias), **epi)


def lin_bwd(G: Grads, lin: torch.nn.Linear, x: torch.Tensor, dy: torch.Tensor, need_dx: bool = True,
            **epi) -> Optional[torch.Tensor]:
    """gradients of y = x W^T + b; `epi` = GEMM epilogue of the input-gradient GEMM (e.g. fused residual add)"""
    want_w = lin.weight.requires_grad
    want_b = lin.bias is not None and lin.bias.requires_grad
    if want_w:
        dw, db = T.linear_wgrad(dy, x, want_bias=want_b)
        G.add(lin.weight, dw)
        G.add(lin.bias, db)
    elif want_b:
        G.add(lin.bias, T.segsum(dy)[0])
    return T.linear_dgrad(dy, w_t(lin.weight), **epi) if need_dx else None


def _fused_t(attn, added: bool) -> torch.Tensor:
    """transpose of the fused qkv projection weight [3D, D] -> [D, 3D]"""
    pk = attn.packed()
    key = "wadd" if added else "wqkv"
    anchor = (attn.add_q_proj if added else attn.to_q).weight
    return STORE.derived(anchor, "fusedT", lambda: T.transpose(pk[key], rows_pad=pk[key].shape[0]))


def qkv_bwd(G: Grads, attn, x: torch.Tensor, dqkv: torch.Tensor, added: bool = False) -> torch.Tensor:
    """backward of the fused q/k/v projection: dqkv [rows, 3D] -> dx, parameter gradients split per projection"""
    lins = (attn.add_q_proj, attn.add_k_proj, attn.add_v_proj) if added else (attn.to_q, attn.to_k, attn.to_v)
    D = lins[0].weight.shape[0]
    if lins[0].weight.requires_grad:
        want_b = lins[0].bias is not None
        dw, db = T.linear_wgrad(dqkv, x, want_bias=want_b)
        for i, l in enumerate(lins):
            G.add(l.weight, dw[i * D:(i + 1) * D])
            if want_b:
                G.add(l.bias, db[i * D:(i + 1) * D])
    return T.linear_dgrad(dqkv, _fused_t(attn, added))


def qk_norm_bwd(G: Grads, attn, qkv: torch.Tensor, rinv: Optional[torch.Tensor], dqkv: torch.Tensor, added: bool = False) -> None:
    """in place on dqkv[:, :2D]; folds the per-column weight gradient back onto norm_{q,k}.weight [64]"""
    if rinv is None:
        return
    pk = attn.packed()
    rms = pk["rms_add" if added else "rms"]
    D2 = rms.numel()
    dw = torch.zeros(D2, dtype=torch.float32, device=qkv.device)
    T.rmsnorm_heads_bwd_(qkv[:, :D2], rinv, rms, dqkv[:, :D2], dw)
    nq, nk = (attn.norm_added_q, attn.norm_added_k) if added else (attn.norm_q, attn.norm_k)
    dw = dw.view(2, attn.heads, 64).sum(1)
    G.add(nq.weight, dw[0])
    G.add(nk.weight, dw[1])


def project_qkv_train(attn, x: torch.Tensor, added: bool = False):
    """fused projection + in-place per-head RMSNorm keeping 1/rms for the backward"""
    pk = attn.packed()
    w, b, rms = (pk["wadd"], pk["badd"], pk.get("rms_add")) if added else (pk["wqkv"], pk["bqkv"], pk.get("rms"))
    qkv = ops.gemm(x, w, b)
    rinv = T.rmsnorm_heads_train_(qkv[:, :rms.numel()], rms, attn.eps) if rms is not None else None
    return qkv, rinv


def small_mlp_fwd(m: TimestepEmbedding, x: torch.Tensor):
    u = lin_fwd(x, m.linear_1)
    a = T.act_fwd(u, ACT_SILU)
    return lin_fwd(a, m.linear_2), (x, u, a)


def small_mlp_bwd(G: Grads, m: TimestepEmbedding, saved, dy: torch.Tensor, need_dx: bool = False):
    x, u, a = saved
    da = lin_bwd(G, m.linear_2, a, dy)
    du = T.act_bwd(u, da, ACT_SILU)
    return lin_bwd(G, m.linear_1, x, du, need_dx=need_dx)


def _params(mod: torch.nn.Module) -> List[torch.nn.Parameter]:
    return [p for p in mod.parameters()]


def _grads_for(G: Grads, params, needs) -> tuple:
    return tuple((G.take(p) if need else None) for p, need in zip(params, needs))


# ------------------------------------------------------------------------------------------ kept activations
# A block either recomputes (its Function keeps the block inputs and backward runs the training forward first: gradient
# checkpointing, the default) or keeps (the training forward IS its forward and its kept set stays alive until backward).
ACTIVATION_POLICIES = ("recompute", "keep", "config")


def resolve_activation_policy(policy: str, gradient_checkpointing: bool = False, temporal_gradient_checkpointing: bool = False,
                              crossview_gradient_checkpointing: bool = False) -> Dict[str, bool]:
    """block family ("joint" | "temporal" | "crossview") -> True if the policy wants its blocks to keep their activations.
    "config": the reference's three switches decide, a family recomputes iff its switch is set
    (crossview_temporal_dit.py:497, :539, :570)."""
    if policy == "recompute":
        return {"joint": False, "temporal": False, "crossview": False}
    if policy == "keep":
        return {"joint": True, "temporal": True, "crossview": True}
    if policy == "config":
        return {"joint": not gradient_checkpointing, "temporal": not temporal_gradient_checkpointing,
                "crossview": not crossview_gradient_checkpointing}
    raise ValueError(f"activations: one of {ACTIVATION_POLICIES}, got {policy!r}")


class ActivationPlan:
    """The keep / recompute decisions of one forward.  `blocks`: (block name, "keep" | "recompute", kept bytes) in forward order,
    `total_bytes`: their sum.  A block that the policy wants kept is kept only while its bytes fit in what is left of the budget
    (budget_gib None: no cap; 0: nothing is kept); a refused block takes nothing, so a later smaller one may still fit."""

    def __init__(self, budget_gib: Optional[float] = None):
        if budget_gib is not None and budget_gib < 0:
            raise ValueError(f"activation_budget_gib: None or >= 0, got {budget_gib!r}")
        self.blocks: List[tuple] = []
        self.left: Optional[int] = None if budget_gib is None else int(budget_gib * 2 ** 30)

    def decide(self, name: str, wanted: bool, nbytes: int) -> bool:
        keep = bool(wanted) and (self.left is None or 0 < nbytes <= self.left)
        if keep and self.left is not None:
            self.left -= nbytes
        self.blocks.append((name, "keep" if keep else "recompute", nbytes if keep else 0))
        return keep

    @property
    def total_bytes(self) -> int:
        return sum(b[2] for b in self.blocks)

    def __iter__(self):
        return iter(self.blocks)

    def __len__(self):
        return len(self.blocks)


def plan_activations(blocks, budget_gib: Optional[float] = None) -> ActivationPlan:
    """blocks: (name, wanted by the policy, kept bytes) in forward order -> the plan under the budget"""
    plan = ActivationPlan(budget_gib)
    for name, wanted, nbytes in blocks:
        plan.decide(name, wanted, nbytes)
    return plan


def kept_bytes(kind: str, *, images: int, tokens: int, dim: int, heads: int, context_tokens: int = 0, ff_inner: Optional[int] = None,
               dual: bool = False, context_pre_only: bool = False, qk_norm: bool = True, emb_rows: int = 0, samples: int = 0,
               lse_rows: Optional[int] = None) -> int:
    """Bytes a kept block holds from its forward to its backward: its inputs, the outputs of its GEMM and attention launches with
    lse and the RMSNorm 1/rms, and the residual-stream values a LayerNorm reads.  LayerNorm and activation outputs are not kept
    (backward re-derives them), and none of the kept tensors is read by a weight gradient alone, so freezing weights changes the
    launches of the backward but not this figure.
    kind "joint": images x tokens sample rows, images x context_tokens context rows, ff_inner the width of the GELU.
    kind "vt": images x tokens rows, emb_rows embedding rows, samples alpha values, ff_inner the GEGLU output width (the
    projection is twice as wide), lse_rows = problems x padded problem length of the row map (default: the rows)."""
    R, Rc, D, H = images * tokens, images * context_tokens, dim, heads
    F = 4 * dim if ff_inner is None else ff_inner
    if kind == "joint":
        b16 = R * D + Rc * D + images * D                                  # h, c, st
        b16 += images * D * ((9 if dual else 6) + (2 if context_pre_only else 6))   # mod, cmod
        b16 += 3 * (R + Rc) * D + (R + Rc) * D                             # qkv, cqkv, ao, cao
        b16 += 2 * R * D + R * F + R * D                                   # t_att, h1, u, t_ff
        f32 = images * H * (tokens + context_tokens)                       # lse
        if qk_norm:
            f32 += 2 * H * (R + Rc)                                        # rinv, crinv
        if dual:
            b16 += 3 * R * D + 2 * R * D                                   # qkv2, ao2, t_att2
            f32 += images * H * tokens + (2 * H * R if qk_norm else 0)     # lse2, rinv2
        if not context_pre_only:
            b16 += 3 * Rc * D + Rc * F                                     # t_catt, c1, t_cff, cu
        return 2 * b16 + 4 * f32
    if kind == "vt":
        b16 = R * D + emb_rows * D                                         # h, emb
        b16 += 2 * (2 * R * F) + 3 * R * D                                 # u1, u3, qkv
        b16 += 4 * R * D                                                   # xs1, ao, xs2, out
        f32 = samples + H * (R if lse_rows is None else lse_rows)          # alpha, lse
        if qk_norm:
            f32 += 2 * H * R                                               # rinv
        return 2 * b16 + 4 * f32
    raise ValueError(f"kept_bytes: kind 'joint' or 'vt', got {kind!r}")


def joint_kept_bytes(blk: JointTransformerBlock, h: torch.Tensor, c: torch.Tensor, n_img: int) -> int:
    return kept_bytes("joint", images=n_img, tokens=h.shape[0] // n_img, context_tokens=c.shape[0] // n_img, dim=blk.dim,
                      heads=blk.heads, ff_inner=blk.ff.net[2].in_features, dual=blk.use_dual_attention,
                      context_pre_only=blk.context_pre_only, qk_norm=blk.attn.has_qk_norm)


def vt_kept_bytes(blk: VTSelfAttentionBlock, h: torch.Tensor, rowmap, emb: torch.Tensor, alpha: torch.Tensor) -> int:
    return kept_bytes("vt", images=1, tokens=h.shape[0], dim=blk.dim, heads=blk.heads, ff_inner=blk.ff.net[2].in_features,
                      qk_norm=blk.attn1.has_qk_norm, emb_rows=emb.shape[0], samples=alpha.numel(),
                      lse_rows=rowmap.n_problems * rowmap.L0)


def _act_lin_bwd(G: Grads, lin2: torch.nn.Linear, pre: torch.Tensor, act_out: Optional[torch.Tensor], dy: torch.Tensor,
                 act: Optional[int]) -> torch.Tensor:
    """backward of lin2(a), a = act(pre) (act None: GEGLU) -> d(pre).  act_out = a where the forward kept it; None: backward
    re-derives it in the pass that differentiates it - input gradient of lin2 first, then ONE read of `pre` for a and d(pre), then
    the weight gradient of lin2 on a.  The same operands reach the same kernels either way."""
    if act_out is not None:
        da = lin_bwd(G, lin2, act_out, dy)
        return T.geglu_bwd(pre, da) if act is None else T.act_bwd(pre, da, act)
    da = T.linear_dgrad(dy, w_t(lin2.weight))
    if not lin2.weight.requires_grad:            # nobody reads a: the one-output kernel
        dpre = T.geglu_bwd(pre, da) if act is None else T.act_bwd(pre, da, act)
    else:
        act_out, dpre = T.geglu_bwd_recompute(pre, da) if act is None else T.act_bwd_recompute(pre, da, act)
    lin_bwd(G, lin2, act_out, dy, need_dx=False)
    return dpre


# ------------------------------------------------------------------------------------------ joint block
def joint_block_forward_train(blk: JointTransformerBlock, h: torch.Tensor, c: torch.Tensor, st: torch.Tensor, n_img: int,
                              keep: bool = False):
    """Training forward of JointTransformerBlock.run (diffusers JointTransformerBlock.forward), un-fused where the backward needs
    a pre-activation.  h [I*N, D], c [I*Lc, D], st = silu(temb) [I, D].  Returns (h_out, c_out, kept).
    keep=False (the first half of a recomputing backward): kept holds every intermediate and the block outputs are not formed.
    keep=True (the forward of a kept block): the outputs are formed and kept holds what kept_bytes counts - LayerNorm and
    activation outputs are dropped, joint_block_backward_kept re-derives them."""
    D = blk.dim
    N, Lc = h.shape[0] // n_img, c.shape[0] // n_img
    dual, pre_only = blk.use_dual_attention, blk.context_pre_only
    sl = lambda m, i: m[:, i * D:(i + 1) * D]
    id_map = ops.rowmap_identity(n_img, N)
    K: Dict[str, Optional[torch.Tensor]] = dict(h=h, c=c, st=st)

    mod = lin_fwd(st, blk.norm1.linear)
    cmod = lin_fwd(st, blk.norm1_context.linear)
    nh2 = torch.empty_like(h) if dual else None
    nh = ops.layernorm(h, eps=1e-6, scale=sl(mod, 1), shift=sl(mod, 0), rows_per_mod=N,
                       scale2=sl(mod, 7) if dual else None, shift2=sl(mod, 6) if dual else None, out2=nh2)
    cs, cb = (0, 1) if pre_only else (1, 0)           # AdaLayerNormContinuous: scale first
    nc = ops.layernorm(c, eps=1e-6, scale=sl(cmod, cs), shift=sl(cmod, cb), rows_per_mod=Lc)
    qkv, rinv = project_qkv_train(blk.attn, nh)
    cqkv, crinv = project_qkv_train(blk.attn, nc, added=True)
    ao, cao = torch.empty_like(h), torch.empty_like(c)
    lse = torch.empty(n_img * blk.heads * (N + Lc), dtype=torch.float32, device=h.device)
    ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], ao, id_map, blk.heads,
                  q1=cqkv[:, :D], k1=cqkv[:, D:2 * D], v1=cqkv[:, 2 * D:], out1=cao, lse=lse)
    t_att = lin_fwd(ao, blk.attn.to_out[0])
    h1 = T.rowcombine(t_att, gate_a=sl(mod, 2), rows_per_gate_a=N, b=h)
    K.update(mod=mod, cmod=cmod, qkv=qkv, rinv=rinv, cqkv=cqkv, crinv=crinv, ao=ao, cao=cao, lse=lse, t_att=t_att)
    if dual:
        qkv2, rinv2 = project_qkv_train(blk.attn2, nh2)
        ao2 = torch.empty_like(h)
        lse2 = torch.empty(n_img * blk.heads * N, dtype=torch.float32, device=h.device)
        ops.attention(qkv2[:, :D], qkv2[:, D:2 * D], qkv2[:, 2 * D:], ao2, id_map, blk.heads, lse=lse2)
        t_att2 = lin_fwd(ao2, blk.attn2.to_out[0])
        h1 = T.rowcombine(t_att2, gate_a=sl(mod, 8), rows_per_gate_a=N, b=h1)
        K.update(qkv2=qkv2, rinv2=rinv2, ao2=ao2, lse2=lse2, t_att2=t_att2)
    nh3 = ops.layernorm(h1, eps=1e-6, scale=sl(mod, 4), shift=sl(mod, 3), rows_per_mod=N)
    f1, f2 = blk.ff.net[0].proj, blk.ff.net[2]
    u = lin_fwd(nh3, f1)
    ffh = T.act_fwd(u, ACT_GELU_TANH)
    t_ff = lin_fwd(ffh, f2)
    K.update(h1=h1, u=u, t_ff=t_ff)
    if not keep:
        K.update(nh=nh, nh2=nh2, nc=nc, nh3=nh3, ffh=ffh)
    h_out = T.rowcombine(t_ff, gate_a=sl(mod, 5), rows_per_gate_a=N, b=h1) if keep else None
    c_out = None
    if not pre_only:
        t_catt = lin_fwd(cao, blk.attn.to_add_out)
        c1 = T.rowcombine(t_catt, gate_a=sl(cmod, 2), rows_per_gate_a=Lc, b=c)
        nc3 = ops.layernorm(c1, eps=1e-6, scale=sl(cmod, 4), shift=sl(cmod, 3), rows_per_mod=Lc)
        c1f, c2f = blk.ff_context.net[0].proj, blk.ff_context.net[2]
        cu = lin_fwd(nc3, c1f)
        cffh = T.act_fwd(cu, ACT_GELU_TANH)
        t_cff = lin_fwd(cffh, c2f)
        K.update(t_catt=t_catt, c1=c1, cu=cu, t_cff=t_cff)
        if keep:
            c_out = T.rowcombine(t_cff, gate_a=sl(cmod, 5), rows_per_gate_a=Lc, b=c1)
        else:
            K.update(nc3=nc3, cffh=cffh)
    return h_out, c_out, K


def joint_block_backward_kept(blk: JointTransformerBlock, K: Dict[str, Optional[torch.Tensor]], n_img: int, dh: torch.Tensor,
                              dc: Optional[torch.Tensor], G: Grads):
    """Backward of the block from the kept set of joint_block_forward_train; dh / dc: gradients of the block outputs.  A LayerNorm
    or activation output the set does not hold is re-derived right before the weight gradient that reads it (not at all when
    that weight is frozen).  Returns (dh_in, dc_in, dst)."""
    D = blk.dim
    h, c, st, mod, cmod = K["h"], K["c"], K["st"], K["mod"], K["cmod"]
    N, Lc = h.shape[0] // n_img, c.shape[0] // n_img
    dual, pre_only = blk.use_dual_attention, blk.context_pre_only
    sl = lambda m, i: m[:, i * D:(i + 1) * D]
    id_map = ops.rowmap_identity(n_img, N)
    cs, cb = (0, 1) if pre_only else (1, 0)
    qkv, rinv, cqkv, crinv, ao, cao, lse = K["qkv"], K["rinv"], K["cqkv"], K["crinv"], K["ao"], K["cao"], K["lse"]
    t_att, h1, u, t_ff = K["t_att"], K["h1"], K["u"], K["t_ff"]
    f1, f2 = blk.ff.net[0].proj, blk.ff.net[2]
    wants = lambda lin: lin.weight.requires_grad

    dmod = torch.zeros(mod.shape, dtype=torch.float32, device=h.device)
    dcmod = torch.zeros(cmod.shape, dtype=torch.float32, device=h.device)

    # ---------------- context stream tail (needed first: the joint attention backward wants d(cao))
    if not pre_only:
        t_catt, c1, cu, t_cff = K["t_catt"], K["c1"], K["cu"], K["t_cff"]
        c1f, c2f = blk.ff_context.net[0].proj, blk.ff_context.net[2]
        # c2 = c1 + gate_mlp * t_cff
        T.segsum(t_cff, dc, rows_per_group=Lc, out=sl(dcmod, 5))
        dct = T.rowcombine(dc, gate_a=sl(cmod, 5), rows_per_gate_a=Lc)
        dcu = _act_lin_bwd(G, c2f, cu, K.get("cffh"), dct, ACT_GELU_TANH)
        nc3 = K.get("nc3")
        if nc3 is None and wants(c1f):
            nc3 = ops.layernorm(c1, eps=1e-6, scale=sl(cmod, 4), shift=sl(cmod, 3), rows_per_mod=Lc)
        dnc3 = lin_bwd(G, c1f, nc3, dcu)
        dc1 = dc.clone()
        T.layernorm_bwd(c1, dnc3, eps=1e-6, dx=dc1, accumulate=True, scale=sl(cmod, 4), rows_per_mod=Lc,
                        dgamma=sl(dcmod, 4), dbeta=sl(dcmod, 3), grad_per_group=True)
        # c1 = c + gate_msa * t_catt
        T.segsum(t_catt, dc1, rows_per_group=Lc, out=sl(dcmod, 2))
        dct1 = T.rowcombine(dc1, gate_a=sl(cmod, 2), rows_per_gate_a=Lc)
        dcao = lin_bwd(G, blk.attn.to_add_out, cao, dct1)
    else:
        dc1 = torch.zeros_like(c)
        dcao = torch.zeros_like(c)

    # ---------------- sample stream: h2 = h1 + gate_mlp * t_ff
    T.segsum(t_ff, dh, rows_per_group=N, out=sl(dmod, 5))
    dt = T.rowcombine(dh, gate_a=sl(mod, 5), rows_per_gate_a=N)
    du = _act_lin_bwd(G, f2, u, K.get("ffh"), dt, ACT_GELU_TANH)
    nh3 = K.get("nh3")
    if nh3 is None and wants(f1):
        nh3 = ops.layernorm(h1, eps=1e-6, scale=sl(mod, 4), shift=sl(mod, 3), rows_per_mod=N)
    dnh3 = lin_bwd(G, f1, nh3, du)
    del nh3
    dh1 = dh.clone()
    T.layernorm_bwd(h1, dnh3, eps=1e-6, dx=dh1, accumulate=True, scale=sl(mod, 4), rows_per_mod=N,
                    dgamma=sl(dmod, 4), dbeta=sl(dmod, 3), grad_per_group=True)
    nh, nh2 = K.get("nh"), K.get("nh2")
    if nh is None and (wants(blk.attn.to_q) or (dual and wants(blk.attn2.to_q))):
        nh2 = torch.empty_like(h) if dual else None
        nh = ops.layernorm(h, eps=1e-6, scale=sl(mod, 1), shift=sl(mod, 0), rows_per_mod=N,
                           scale2=sl(mod, 7) if dual else None, shift2=sl(mod, 6) if dual else None, out2=nh2)
    dnh2 = None
    if dual:       # h1 = h1a + gate2 * t_att2
        qkv2, rinv2, ao2, lse2, t_att2 = K["qkv2"], K["rinv2"], K["ao2"], K["lse2"], K["t_att2"]
        T.segsum(t_att2, dh1, rows_per_group=N, out=sl(dmod, 8))
        dt2 = T.rowcombine(dh1, gate_a=sl(mod, 8), rows_per_gate_a=N)
        dao2 = lin_bwd(G, blk.attn2.to_out[0], ao2, dt2)
        dqkv2 = torch.empty_like(qkv2)
        ops.attention_bwd(qkv2[:, :D], qkv2[:, D:2 * D], qkv2[:, 2 * D:], ao2, dao2,
                          dqkv2[:, :D], dqkv2[:, D:2 * D], dqkv2[:, 2 * D:], id_map, blk.heads, lse2)
        qk_norm_bwd(G, blk.attn2, qkv2, rinv2, dqkv2)
        dnh2 = qkv_bwd(G, blk.attn2, nh2, dqkv2)
    # h1a = h + gate_msa * t_att
    T.segsum(t_att, dh1, rows_per_group=N, out=sl(dmod, 2))
    dt1 = T.rowcombine(dh1, gate_a=sl(mod, 2), rows_per_gate_a=N)
    dao = lin_bwd(G, blk.attn.to_out[0], ao, dt1)

    # ---------------- joint attention
    dqkv, dcqkv = torch.empty_like(qkv), torch.empty_like(cqkv)
    ops.attention_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], ao, dao, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:],
                      id_map, blk.heads, lse, q1=cqkv[:, :D], k1=cqkv[:, D:2 * D], v1=cqkv[:, 2 * D:], out1=cao, dout1=dcao,
                      dq1=dcqkv[:, :D], dk1=dcqkv[:, D:2 * D], dv1=dcqkv[:, 2 * D:])
    qk_norm_bwd(G, blk.attn, qkv, rinv, dqkv)
    qk_norm_bwd(G, blk.attn, cqkv, crinv, dcqkv, added=True)
    dnh = qkv_bwd(G, blk.attn, nh, dqkv)
    nc = K.get("nc")
    if nc is None and wants(blk.attn.add_q_proj):
        nc = ops.layernorm(c, eps=1e-6, scale=sl(cmod, cs), shift=sl(cmod, cb), rows_per_mod=Lc)
    dnc = qkv_bwd(G, blk.attn, nc, dcqkv, added=True)

    # ---------------- the two AdaLN layers at the block input
    T.layernorm_bwd(h, dnh, eps=1e-6, dx=dh1, accumulate=True, scale=sl(mod, 1), scale2=sl(mod, 7) if dual else None,
                    rows_per_mod=N, dy2=dnh2, dgamma=sl(dmod, 1), dbeta=sl(dmod, 0),
                    dgamma2=sl(dmod, 7) if dual else None, dbeta2=sl(dmod, 6) if dual else None, grad_per_group=True)
    T.layernorm_bwd(c, dnc, eps=1e-6, dx=dc1, accumulate=True, scale=sl(cmod, cs), rows_per_mod=Lc,
                    dgamma=sl(dcmod, cs), dbeta=sl(dcmod, cb), grad_per_group=True)

    # ---------------- modulation linears (M = images)
    dst = lin_bwd(G, blk.norm1.linear, st, dmod.to(bf16))
    dst2 = lin_bwd(G, blk.norm1_context.linear, st, dcmod.to(bf16))
    ops.add_(dst, dst2)
    return dh1, dc1, dst


def joint_block_backward(blk: JointTransformerBlock, h: torch.Tensor, c: torch.Tensor, st: torch.Tensor, n_img: int,
                         dh: torch.Tensor, dc: Optional[torch.Tensor], G: Grads):
    """Recompute + backward of JointTransformerBlock.run: the training forward from the block INPUTS, then the backward from
    its kept set.  dh / dc: gradients of the block outputs.  Returns (dh_in, dc_in, dst)."""
    _, _, K = joint_block_forward_train(blk, h, c, st, n_img, keep=False)
    return joint_block_backward_kept(blk, K, n_img, dh, dc, G)


def _save_kept(ctx, K: Dict[str, Optional[torch.Tensor]]) -> None:
    ctx.kept_names = list(K)
    ctx.save_for_backward(*K.values())


def _load_kept(ctx) -> Dict[str, Optional[torch.Tensor]]:
    return dict(zip(ctx.kept_names, ctx.saved_tensors))


@ops.carries_gemm_scope
class JointBlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, blk, n_img, keep, h, c, st, *params):
        ctx.blk, ctx.n_img, ctx.keep = blk, n_img, keep
        ctx.np = len(params)
        with torch.no_grad():
            if keep:
                h_out, c_out, K = joint_block_forward_train(blk, h, c, st, n_img, keep=True)
                _save_kept(ctx, K)
            else:
                ctx.save_for_backward(h, c, st)
                c_out, h_out = blk.run(h.clone(), c.clone(), st, n_img)
        if c_out is None:
            c_out = c.new_zeros(())           # context_pre_only: the context stream ends here
        return h_out, c_out

    @staticmethod
    def backward(ctx, dh, dc):
        blk = ctx.blk
        G = Grads()
        dc = None if blk.context_pre_only else dc.contiguous()
        if ctx.keep:
            dh_in, dc_in, dst = joint_block_backward_kept(blk, _load_kept(ctx), ctx.n_img, dh.contiguous(), dc, G)
        else:
            h, c, st = ctx.saved_tensors
            dh_in, dc_in, dst = joint_block_backward(blk, h, c, st, ctx.n_img, dh.contiguous(), dc, G)
        ps = _params(blk)
        return (None, None, None, dh_in, dc_in, dst) + _grads_for(G, ps, ctx.needs_input_grad[6:])


def joint_block_train(blk: JointTransformerBlock, h, c, st, n_img: int, keep: bool = False):
    """keep: the block keeps its activations instead of recomputing them in backward (ignored without autograd: nothing is kept)"""
    return JointBlockFn.apply(blk, n_img, bool(keep) and torch.is_grad_enabled(), h, c, st, *_params(blk))


# ------------------------------------------------------------------------------------------ VT block + mixer
def vt_block_forward_train(blk: VTSelfAttentionBlock, h: torch.Tensor, emb: torch.Tensor, rows_per_emb: int, rowmap,
                           group_mask, dense_mask, alpha: torch.Tensor, rows_per_alpha: int, keep: bool = False):
    """Training forward of VTSelfAttentionBlock.run followed by the AlphaBlender (crossview_temporal.py:562-582, 68-72;
    crossview_temporal_dit.py:320-327,363-370).  Returns (blended, kept).  keep=False: every intermediate is in kept and the blend
    is not formed; keep=True: blended = alpha * h + (1 - alpha) * out is, and kept holds what kept_bytes counts - `out` from before
    the blend among it, for d(alpha)."""
    D = blk.dim
    ln = lambda x, n, **kw: ops.layernorm(x, eps=1e-5, weight=_bf(n.weight), bias=_bf(n.bias), **kw)
    xs0 = torch.empty_like(h)
    y = ln(h, blk.norm_in, addvec=emb, rows_per_add=rows_per_emb, xsum=xs0)          # xs0 = h + emb
    pi, l2i = blk.ff_in.net[0].proj, blk.ff_in.net[2]
    u1 = lin_fwd(y, pi)
    g1 = T.geglu_fwd(u1)
    xs1 = lin_fwd(g1, l2i, epilogue=ops.EPI_RESID, res=xs0)
    y1 = ln(xs1, blk.norm1)
    qkv, rinv = project_qkv_train(blk.attn1, y1)
    ao = torch.empty_like(h)
    lse = torch.empty(rowmap.n_problems * blk.heads * rowmap.L0, dtype=torch.float32, device=h.device)
    ops.attention(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], ao, rowmap, blk.heads, group_mask=group_mask,
                  dense_mask=dense_mask, lse=lse)
    xs2 = lin_fwd(ao, blk.attn1.to_out[0], epilogue=ops.EPI_RESID, res=xs1)
    y3 = ln(xs2, blk.norm3)
    p3, l23 = blk.ff.net[0].proj, blk.ff.net[2]
    u3 = lin_fwd(y3, p3)
    g3 = T.geglu_fwd(u3)
    out = lin_fwd(g3, l23, epilogue=ops.EPI_RESID, res=xs2)
    K = dict(h=h, emb=emb, alpha=alpha, u1=u1, xs1=xs1, qkv=qkv, rinv=rinv, ao=ao, lse=lse, xs2=xs2, u3=u3, out=out)
    if not keep:
        K.update(y=y, g1=g1, y1=y1, y3=y3, g3=g3)
        return None, K
    one_minus = (1.0 - alpha).contiguous()
    blended = T.rowcombine(h, coef_a=alpha, rows_per_coef_a=rows_per_alpha, b=out, coef_b=one_minus, rows_per_coef_b=rows_per_alpha)
    return blended, K


def vt_block_backward_kept(blk: VTSelfAttentionBlock, K: Dict[str, Optional[torch.Tensor]], rows_per_emb: int, rowmap,
                           group_mask, dense_mask, rows_per_alpha: int, dy: torch.Tensor, G: Grads):
    """Backward of the VT block and its mixer from the kept set of vt_block_forward_train (a LayerNorm or GEGLU output it does
    not hold is re-derived, as in joint_block_backward_kept).  Returns (dh, demb fp32 [G, D], dalpha fp32 [B])."""
    D = blk.dim
    ln = lambda x, n, **kw: ops.layernorm(x, eps=1e-5, weight=_bf(n.weight), bias=_bf(n.bias), **kw)
    h, emb, alpha = K["h"], K["emb"], K["alpha"]
    u1, xs1, qkv, rinv, ao, lse, xs2, u3 = K["u1"], K["xs1"], K["qkv"], K["rinv"], K["ao"], K["lse"], K["xs2"], K["u3"]
    pi, l2i = blk.ff_in.net[0].proj, blk.ff_in.net[2]
    p3, l23 = blk.ff.net[0].proj, blk.ff.net[2]
    to_out = blk.attn1.to_out[0]
    wants = lambda lin: lin.weight.requires_grad

    # ---------------- mixer: blended = alpha * h + (1 - alpha) * out
    one_minus = (1.0 - alpha).contiguous()
    # d(alpha) = <dy, h - out>: one pass, fp32 difference before the product, fp32 column sums, summed in fp64 - the value
    # is a heavily cancelling sum (sum|terms| / |sum| = 200-3000 on the test configurations), so no partial sum is rounded
    dalpha = T.segsum_diff(dy, h, K.pop("out"), rows_per_group=rows_per_alpha).double().sum(-1).float()
    dout = T.rowcombine(dy, coef_a=one_minus, rows_per_coef_a=rows_per_alpha)

    def ln_bwd(x, n, dyy, dx, **kw):
        dg = torch.zeros(1, D, dtype=torch.float32, device=h.device)
        db = torch.zeros(1, D, dtype=torch.float32, device=h.device)
        T.layernorm_bwd(x, dyy, eps=1e-5, dx=dx, accumulate=True, weight=_bf(n.weight), dgamma=dg, dbeta=db, **kw)
        G.add(n.weight, dg[0])
        G.add(n.bias, db[0])

    # out = xs2 + ff(norm3(xs2))
    dxs2 = dout
    du3 = _act_lin_bwd(G, l23, u3, K.get("g3"), dout, None)
    y3 = K.get("y3")
    if y3 is None and wants(p3):
        y3 = ln(xs2, blk.norm3)
    dy3 = lin_bwd(G, p3, y3, du3)
    del y3
    ln_bwd(xs2, blk.norm3, dy3, dxs2)
    # xs2 = xs1 + to_out(attn(norm1(xs1)))
    dao = lin_bwd(G, to_out, ao, dxs2)
    dqkv = torch.empty_like(qkv)
    ops.attention_bwd(qkv[:, :D], qkv[:, D:2 * D], qkv[:, 2 * D:], ao, dao, dqkv[:, :D], dqkv[:, D:2 * D], dqkv[:, 2 * D:],
                      rowmap, blk.heads, lse, group_mask=group_mask, dense_mask=dense_mask)
    qk_norm_bwd(G, blk.attn1, qkv, rinv, dqkv)
    y1 = K.get("y1")
    if y1 is None and wants(blk.attn1.to_q):
        y1 = ln(xs1, blk.norm1)
    dy1 = qkv_bwd(G, blk.attn1, y1, dqkv)
    del y1
    dxs1 = dxs2
    ln_bwd(xs1, blk.norm1, dy1, dxs1)
    # xs1 = xs0 + ff_in(norm_in(xs0))
    du1 = _act_lin_bwd(G, l2i, u1, K.get("g1"), dxs1, None)
    y = K.get("y")
    if y is None and wants(pi):
        y = ln(h, blk.norm_in, addvec=emb, rows_per_add=rows_per_emb)
    dyin = lin_bwd(G, pi, y, du1)
    del y
    dxs0 = dxs1
    ln_bwd(h, blk.norm_in, dyin, dxs0, addvec=emb, rows_per_add=rows_per_emb)
    # xs0 = h + emb[row // rows_per_emb]   (one embedding row per token - explicit perspective modelling - needs no sum)
    demb = dxs0 if rows_per_emb == 1 else T.segsum(dxs0, rows_per_group=rows_per_emb)
    dh = T.rowcombine(dy, coef_a=alpha, rows_per_coef_a=rows_per_alpha, b=dxs0)
    return dh, demb, dalpha


def vt_block_backward(blk: VTSelfAttentionBlock, h: torch.Tensor, emb: torch.Tensor, rows_per_emb: int, rowmap,
                      group_mask, dense_mask, alpha: torch.Tensor, rows_per_alpha: int, dy: torch.Tensor, G: Grads):
    """Recompute + backward of VTSelfAttentionBlock.run followed by the AlphaBlender: the training forward from the block
    INPUTS, then the backward from its kept set.  Returns (dh, demb fp32 [G, D], dalpha fp32 [B])."""
    _, K = vt_block_forward_train(blk, h, emb, rows_per_emb, rowmap, group_mask, dense_mask, alpha, rows_per_alpha, keep=False)
    return vt_block_backward_kept(blk, K, rows_per_emb, rowmap, group_mask, dense_mask, rows_per_alpha, dy, G)


@ops.carries_gemm_scope
class VTBlockFn(torch.autograd.Function):
    """h_out = AlphaBlender(h, VTSelfAttentionBlock(h + emb)); inputs that carry gradients: h, emb, alpha."""

    @staticmethod
    def forward(ctx, blk, rowmap, rows_per_emb, rows_per_alpha, group_mask, dense_mask, keep, h, emb, alpha, *params):
        ctx.blk, ctx.rowmap, ctx.rpe, ctx.rpa = blk, rowmap, rows_per_emb, rows_per_alpha
        ctx.gm, ctx.dm, ctx.keep = group_mask, dense_mask, keep
        with torch.no_grad():
            if keep:
                out, K = vt_block_forward_train(blk, h, emb, rows_per_emb, rowmap, group_mask, dense_mask, alpha, rows_per_alpha,
                                                keep=True)
                _save_kept(ctx, K)
            else:
                ctx.save_for_backward(h, emb, alpha)
                out = h.clone()
                blk.run(out, rowmap, emb=emb, rows_per_emb=rows_per_emb, group_mask=group_mask, dense_mask=dense_mask,
                        blend_alpha=alpha, rows_per_alpha=rows_per_alpha, blend_into=out)
        return out

    @staticmethod
    def backward(ctx, dy):
        G = Grads()
        if ctx.keep:
            K = _load_kept(ctx)
            emb, alpha = K["emb"], K["alpha"]
            dh, demb, dalpha = vt_block_backward_kept(ctx.blk, K, ctx.rpe, ctx.rowmap, ctx.gm, ctx.dm, ctx.rpa, dy.contiguous(), G)
        else:
            h, emb, alpha = ctx.saved_tensors
            dh, demb, dalpha = vt_block_backward(ctx.blk, h, emb, ctx.rpe, ctx.rowmap, ctx.gm, ctx.dm, alpha, ctx.rpa,
                                                 dy.contiguous(), G)
        ps = _params(ctx.blk)
        return (None, None, None, None, None, None, None, dh, demb.to(emb.dtype), dalpha.to(alpha.dtype)) + \
            _grads_for(G, ps, ctx.needs_input_grad[10:])


def vt_block_train(blk, h, rowmap, emb, rows_per_emb, alpha, rows_per_alpha, group_mask=None, dense_mask=None, keep: bool = False):
    """keep: the block keeps its activations instead of recomputing them in backward (ignored without autograd)"""
    return VTBlockFn.apply(blk, rowmap, rows_per_emb, rows_per_alpha, group_mask, dense_mask, bool(keep) and torch.is_grad_enabled(),
                           h, emb, alpha, *_params(blk))


def alpha_train(mixer: AlphaBlender, image_only_indicator: Optional[torch.Tensor], batch: int) -> torch.Tensor:
    """AlphaBlender.get_alpha with autograd on mix_factor (one scalar: plain torch)."""
    mf = mixer.mix_factor.float()
    if mixer.merge_strategy == "fixed":
        return mf.expand(batch).contiguous()
    if mixer.merge_strategy == "learned":
        return torch.sigmoid(mf).expand(batch).contiguous()
    flag = image_only_indicator.reshape(batch).to(device=mf.device, dtype=torch.bool)
    return torch.where(flag, torch.ones((), device=mf.device), torch.sigmoid(mf).expand(batch)).contiguous()


# ------------------------------------------------------------------------------------------ small modules
@ops.carries_gemm_scope
class MlpFn(torch.autograd.Function):
    """TimestepEmbedding: linear_2(silu(linear_1(x))) [+ res]; x carries no gradient (sinusoids / pooled text)."""

    @staticmethod
    def forward(ctx, m, x, res, *params):
        ctx.m = m
        with torch.no_grad():
            y, saved = small_mlp_fwd(m, x)
            if res is not None:
                y = T.rowcombine(y, b=res)
        ctx.saved = saved
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        G = Grads()
        dy = dy.contiguous()
        small_mlp_bwd(G, ctx.m, ctx.saved, dy)
        ps = _params(ctx.m)
        return (None, None, dy if ctx.has_res else None) + _grads_for(G, ps, ctx.needs_input_grad[3:])


def mlp_train(m: TimestepEmbedding, x: torch.Tensor, res: Optional[torch.Tensor] = None) -> torch.Tensor:
    return MlpFn.apply(m, x, res, *_params(m))


@ops.carries_gemm_scope
class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lin, x, *params):
        ctx.lin = lin
        ctx.save_for_backward(x)
        with torch.no_grad():
            return lin_fwd(x, lin)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        G = Grads()
        dx = lin_bwd(G, ctx.lin, x, dy.contiguous(), need_dx=ctx.needs_input_grad[1])
        return (None, dx) + _grads_for(G, _params(ctx.lin), ctx.needs_input_grad[2:])


def linear_train(lin: torch.nn.Linear, x: torch.Tensor) -> torch.Tensor:
    return LinearFn.apply(lin, x, *_params(lin))


class SiluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.save_for_backward(x)
        with torch.no_grad():
            return T.act_fwd(x, ACT_SILU)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return T.act_bwd(x, dy.contiguous(), ACT_SILU)


class AddFn(torch.autograd.Function):
    """a + b on bf16 matrices (HIP)"""

    @staticmethod
    def forward(ctx, a, b):
        with torch.no_grad():
            return T.rowcombine(a, b=b)

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


@ops.carries_gemm_scope
class PatchEmbedFn(torch.autograd.Function):
    """SD3 PatchEmbed (strided conv as patchify + GEMM, + cropped pos embed); the latents carry no gradient."""

    @staticmethod
    def forward(ctx, pe, x, *params):
        ctx.pe = pe
        ctx.save_for_backward(x)
        with torch.no_grad():
            return pe.run(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        pe = ctx.pe
        G = Grads()
        if pe.proj.weight.requires_grad:
            wp = pe.packed_weight()
            cols = ops.patchify(x, pe.patch_size, wp.shape[1])
            dw, db = T.linear_wgrad(dy.contiguous(), cols)
            k = pe.proj.weight[0].numel()
            G.add(pe.proj.weight, dw[:, :k].contiguous())
            G.add(pe.proj.bias, db)
        return (None, None) + _grads_for(G, _params(pe), ctx.needs_input_grad[2:])


@ops.carries_gemm_scope
class OutFn(torch.autograd.Function):
    """norm_out (AdaLayerNormContinuous) + proj_out + unpatchify"""

    @staticmethod
    def forward(ctx, model, geom, h, st, *params):
        ctx.model, ctx.geom = model, geom
        ctx.save_for_backward(h, st)
        I, C, hh, ww, p, N, D = geom
        with torch.no_grad():
            mod = lin_fwd(st, model.norm_out.linear)
            nh = ops.layernorm(h, eps=1e-6, scale=mod[:, :D], shift=mod[:, D:], rows_per_mod=N)
            y = lin_fwd(nh, model.proj_out)
            return ops.unpatchify(y, I, C, hh, ww, p)

    @staticmethod
    def backward(ctx, dout):
        h, st = ctx.saved_tensors
        model = ctx.model
        I, C, hh, ww, p, N, D = ctx.geom
        G = Grads()
        mod = lin_fwd(st, model.norm_out.linear)
        nh = ops.layernorm(h, eps=1e-6, scale=mod[:, :D], shift=mod[:, D:], rows_per_mod=N)
        # unpatchify is a permutation: its transpose is the patch gather with (py, px, c) column order
        do = dout.to(bf16).contiguous().view(I, C, hh, p, ww, p).permute(0, 2, 4, 3, 5, 1).reshape(I * hh * ww, p * p * C).contiguous()
        dnh = lin_bwd(G, model.proj_out, nh, do)
        dmod = torch.zeros(mod.shape, dtype=torch.float32, device=h.device)
        dh = T.layernorm_bwd(h, dnh, eps=1e-6, scale=mod[:, :D], rows_per_mod=N, dgamma=dmod[:, :D], dbeta=dmod[:, D:],
                             grad_per_group=True)
        dst = lin_bwd(G, model.norm_out.linear, st, dmod.to(bf16))
        ps = _params(model.norm_out) + _params(model.proj_out)
        return (None, None, dh, dst) + _grads_for(G, ps, ctx.needs_input_grad[4:])


# ------------------------------------------------------------------------------------------ layout ImageAdapter
def _conv3_wgrad(dh: torch.Tensor, x_pad: torch.Tensor, grid, idx: torch.Tensor) -> torch.Tensor:
    """dW [N, 9*C] (tap-major, bf16) of h = conv3x3(x): dW[n, t, c] = sum_pixels dh[pixel, n] * x_pad[row(pixel) + shift_t, c].
    (train_ops.conv_wgrad: dh scattered onto the padded grid, all nine taps one dwm_gemm_tn launch)"""
    return T.conv_wgrad(dh, x_pad, idx, grid.tap_shifts())


def _conv3_flip(w: torch.Tensor) -> torch.Tensor:
    """weight of the input-gradient convolution: [N, C, 3, 3] -> tap-major [C, 9*N] with the taps mirrored"""
    return STORE.derived(w, "c3flip", lambda: _bf(w).flip(2, 3).permute(1, 2, 3, 0).reshape(w.shape[1], -1).contiguous())


@ops.carries_gemm_scope
class AdapterFn(torch.autograd.Function):
    """dwm.models.adapters.ImageAdapter (src/dwm/models/adapters.py:40-60) with a hand-written backward.  Forward =
    the inference path (opendwm_amd.adapters.ImageAdapter.run) keeping only the condition images (the reference wraps
    the adapter body in gradient checkpointing, adapters.py:44-52); backward recomputes the body level by level, keeping
    each resnet's input grid and ReLU output, then walks it in reverse: 1x1 convolutions as GEMMs, the 3x3 input gradient
    as the implicit GEMM with mirrored taps, the 3x3 weight gradient as nine tap-shifted GEMMs."""

    @staticmethod
    def forward(ctx, adapter, x, *params):
        ctx.adapter = adapter
        ctx.save_for_backward(x)
        with torch.no_grad():
            return tuple(adapter.run(x))

    @staticmethod
    def backward(ctx, *dfeats):
        from .ops import ACT_RELU, EPI_RESID, PaddedGrid
        (x,) = ctx.saved_tensors
        ad = ctx.adapter
        G = Grads()
        x = x.flatten(0, -4).contiguous()
        if x.dtype not in (torch.float32, bf16):
            x = x.to(bf16)
        I, _, H, W = x.shape
        r = ad.downscale_factor
        h, w = H // r, W // r
        # ---- recompute, keeping what the backward needs.  A level = one AdapterBlock; its grid changes where the block
        # starts with AvgPool2d (the MMDiT layout adapters pool in the first block only, the SD 2.1 UNet's in blocks 1-3)
        cur = ops.unshuffle_tokens(x, r)            # compact tokens; None while the running tensor lives on a padded grid
        levels = []
        xp, grid, idx = None, None, None
        for bi, (blk, zc) in enumerate(zip(ad.body, ad.zero_convs)):
            lv = {"blk": blk, "zc": zc, "res": [], "pooled_from": None}
            if blk.downsample is not None:
                if cur is None:
                    cur = xp[idx]                                                 # compact rows of the previous level's output
                if h % 2 or w % 2:
                    raise NotImplementedError("AvgPool2d(ceil_mode) on odd sizes")
                cur = ops.avgpool2_tokens(cur, I, h, w)
                lv["pooled_from"] = (h, w)
                h, w = h // 2, w // 2
                xp = None
            if xp is None:
                grid = PaddedGrid(I, h, w)
                idx = grid.interior_index(x.device)
                if blk.in_conv is not None:
                    wi = _bf(blk.in_conv.weight).reshape(blk.in_conv.weight.shape[0], -1)
                    if wi.shape[1] != cur.shape[1]:                               # first block: K padded to 64 by unshuffle_tokens
                        wpad = torch.zeros((wi.shape[0], cur.shape[1]), dtype=bf16, device=wi.device)
                        wpad[:, :wi.shape[1]] = wi
                        wi = wpad
                    xp = ops.gemm(cur, wi.contiguous(), _bf(blk.in_conv.bias), c_grid=grid)
                    lv["in"] = ("compact", cur)
                else:
                    xp = ops.pad_tokens(cur, grid)
                    lv["in"] = ("pad", None)
                cur = None
            elif blk.in_conv is not None:
                wi = _bf(blk.in_conv.weight).reshape(blk.in_conv.weight.shape[0], -1).contiguous()
                lv["in"] = ("grid", xp)
                xp = ops.gemm(xp, wi, _bf(blk.in_conv.bias), a_grid=grid, c_grid=grid)
            else:
                lv["in"] = ("same", None)
            lv["grid"], lv["idx"], lv["first"] = grid, idx, bi == 0
            for res in blk.resnets:
                pk = res.packed()
                h1 = ops.gemm(xp, pk["w3"], _bf(res.block1.bias), act=ACT_RELU, a_grid=grid, conv3x3=True)
                xn = ops.gemm(h1, pk["w1"], _bf(res.block2.bias), epilogue=EPI_RESID, res=xp, c_grid=grid)
                lv["res"].append((res, xp, h1))
                xp = xn
            lv["out"] = xp
            levels.append(lv)
        # ---- backward, last level first; dx: gradient w.r.t. the level's output grid (padded rows, zero border)
        dx = None
        quarter = torch.full((1,), 0.25, dtype=torch.float32, device=x.device)
        for lv, df in zip(reversed(levels), reversed(dfeats)):
            grid, idx = lv["grid"], lv["idx"]
            if df is not None:
                df = df.to(bf16).contiguous()
                zc = lv["zc"]
                if zc is not None:
                    xc = lv["out"][idx]                                           # compact rows of the level output
                    dwz, dbz = T.linear_wgrad(df, xc, want_bias=True)
                    G.add(zc.weight, dwz)
                    G.add(zc.bias, dbz)
                    wz_t = w_t(zc.weight)
                    dx = ops.gemm(df, wz_t, None, c_grid=grid) if dx is None else \
                        ops.gemm(df, wz_t, None, epilogue=EPI_RESID, res=dx, out=dx, c_grid=grid)
                else:
                    dpad = ops.pad_tokens(df, grid)
                    dx = dpad if dx is None else T.rowcombine(dx, b=dpad)
            if dx is None:
                continue
            for res, xin, h1 in reversed(lv["res"]):
                dyc = dx[idx]                                                     # compact gradient of the block output
                dw1, db1 = T.linear_wgrad(dyc, h1, want_bias=True)
                G.add(res.block2.weight, dw1)
                G.add(res.block2.bias, db1)
                dh1 = T.linear_dgrad(dyc, w_t(res.block2.weight))
                T.act_bwd(h1, dh1, ACT_RELU, out=dh1)
                G.add(res.block1.bias, T.segsum(dh1)[0])
                G.add(res.block1.weight, _conv3_wgrad(dh1, xin, grid, idx).view(dh1.shape[1], 3, 3, -1).permute(0, 3, 1, 2))
                dhp = ops.pad_tokens(dh1, grid)
                ops.gemm(dhp, _conv3_flip(res.block1.weight), None, a_grid=grid, conv3x3=True, epilogue=EPI_RESID, res=dx,
                         out=dx, c_grid=grid)                                     # dx += conv3x3^T(dh1), in place
            kind, saved = lv["in"]
            blk = lv["blk"]
            dcur = None                           # gradient w.r.t. the compact tensor that entered this level (if it had one)
            if kind == "grid":                    # in_conv on the previous level's grid (same resolution)
                dxc = dx[idx]
                dwi, dbi = T.linear_wgrad(dxc, saved[idx], want_bias=True)
                G.add(blk.in_conv.weight, dwi)
                G.add(blk.in_conv.bias, dbi)
                dx = ops.gemm(dxc, w_t(blk.in_conv.weight), None, c_grid=grid)
            elif kind == "compact":
                dxc = dx[idx]
                dwi, dbi = T.linear_wgrad(dxc, saved, want_bias=True)
                ci = blk.in_conv.weight.shape[1]
                G.add(blk.in_conv.weight, dwi[:, :ci].contiguous())
                G.add(blk.in_conv.bias, dbi)
                if not lv["first"]:
                    dcur = T.linear_dgrad(dxc, w_t(blk.in_conv.weight))
            elif kind == "pad":
                if not lv["first"]:
                    dcur = dx[idx]
            # kind == "same": the previous level's grid IS this level's input: dx carries on unchanged
            if kind in ("compact", "pad"):
                if lv["first"] or dcur is None:
                    dx = None                                                     # the condition images carry no gradient
                else:
                    if lv["pooled_from"] is None:
                        raise RuntimeError("adapter backward: a level that re-grids without pooling")
                    # AvgPool2d(2) backward: every child pixel gets a quarter of the pooled gradient - nearest 2x upsample
                    # straight onto the previous level's padded grid
                    hp, wp_ = lv["pooled_from"]
                    up = ops.upsample2_padded(dcur, I, hp // 2, wp_ // 2)
                    dx = T.rowcombine(up, coef_a=quarter, rows_per_coef_a=up.shape[0])
        ps = _params(ad)
        return (None, None) + _grads_for(G, ps, ctx.needs_input_grad[2:])


@ops.carries_gemm_scope
class RayEmbFn(torch.autograd.Function):
    """Explicit perspective modelling (crossview_temporal_dit.py:440-458, 528-568): per-token embedding of a cross-view /
    temporal block = per-image index embedding [I, D] + RayEncoder.proj(ray features [I*N, 72]).  One K = 128 GEMM with the
    per-image row as the epilogue residual; the ray features carry no gradient, `proj.weight` and the index embedding do."""

    @staticmethod
    def forward(ctx, renc, n_tok, ray_feat, emb_img, *params):
        ctx.renc, ctx.n_tok = renc, n_tok
        ctx.save_for_backward(ray_feat)
        with torch.no_grad():
            return ops.gemm(ray_feat, renc.packed(), None, epilogue=ops.EPI_RESID, res=emb_img.contiguous(), res_mod=-n_tok)

    @staticmethod
    def backward(ctx, dout):
        (ray_feat,) = ctx.saved_tensors
        renc = ctx.renc
        G = Grads()
        dout = dout.contiguous()
        if renc.proj.weight.requires_grad:
            dw, _ = T.linear_wgrad(dout, ray_feat, want_bias=False)                  # [D, 128]: K was zero-padded from 72
            G.add(renc.proj.weight, dw[:, :renc.proj.weight.shape[1]].contiguous())
        demb = ops.cast_bf16(T.segsum(dout, rows_per_group=ctx.n_tok))
        return (None, None, None, demb) + _grads_for(G, _params(renc), ctx.needs_input_grad[4:])


# ------------------------------------------------------------------------------------------ model forward
@ops.opens_ordered_scope
def forward_train(model, sample, timestep, encoder_hidden_states, pooled_projections, disable_crossview=None,
                  disable_temporal=None, crossview_attention_mask=None, added_time_ids=None, condition_image_tensor=None,
                  camera_intrinsics_norm=None, camera2referego=None):
    """Autograd-enabled forward of DiTCrossviewTemporalConditionModel (text-conditioned configuration;
    crossview_temporal_dit.py:372-630).  Returns the prediction [B, T, V, C, H, W] (bf16) with a grad_fn."""
    STORE.set_precision(bf16)               # training runs in bf16 compute over fp32 masters
    B, Tn, V, _, H, W = sample.shape
    p = model._cfg.patch_size
    height, width = H // p, W // p
    N, I, D = height * width, B * Tn * V, model.inner_dim
    dev = sample.device

    def as_bf16(t):
        return t if t.dtype == bf16 else (ops.cast_bf16(t.contiguous()) if t.dtype == torch.float32 else t.to(bf16))

    x = sample.flatten(0, 2).contiguous()
    h = PatchEmbedFn.apply(model.pos_embed, x, *_params(model.pos_embed))
    ehs = as_bf16(encoder_hidden_states.flatten(0, 2))
    Lc = ehs.shape[1]
    c = linear_train(model.context_embedder, ehs.reshape(I * Lc, -1))
    pooled = as_bf16(pooled_projections.flatten(0, 2)).contiguous()
    tte = model.time_text_embed
    t_emb = mlp_train(tte.timestep_embedder, ops.timestep_sinusoid(timestep.flatten(), 256))
    temb = mlp_train(tte.text_embedder, pooled, res=t_emb)
    st = SiluFn.apply(temb)

    view_cam_emb = None
    ray_feat = None
    if model.perspective_modeling_type == "explicit":                                              # :440-458
        if camera_intrinsics_norm is None or camera2referego is None:
            raise RuntimeError("perspective_modeling_type='explicit' needs camera_intrinsics_norm and camera2referego")
        with torch.no_grad():
            ray_feat = model.rayencoder.features(camera_intrinsics_norm, camera2referego, height, width)

    def with_rays(emb_img):
        """(embedding for the VT block, rows per embedding row): the per-image row alone, or row + ray projection per token"""
        if ray_feat is None:
            return emb_img, N
        return RayEmbFn.apply(model.rayencoder, N, ray_feat, emb_img, *_params(model.rayencoder)), 1
    if model.perspective_modeling_type == "implicit":
        ve = ops.timestep_sinusoid(added_time_ids.flatten(), 256).view(I, -1)
        view_cam_emb = mlp_train(model.view_embedding, ve)
    if model.enable_crossview and disable_crossview is None:
        disable_crossview = torch.zeros(B, dtype=torch.bool, device=dev)
    if model.enable_temporal and disable_temporal is None:
        disable_temporal = torch.zeros(B, dtype=torch.bool, device=dev)

    wants = resolve_activation_policy(getattr(model, "activation_policy", "recompute"), model.gradient_checkpointing,
                                      model.temporal_gradient_checkpointing, model.crossview_gradient_checkpointing)
    plan = ActivationPlan(getattr(model, "activation_budget_gib", None))

    residuals: List[torch.Tensor] = []
    if model.condition_image_adapter is not None and condition_image_tensor is not None:            # :459-462
        ad = model.condition_image_adapter
        residuals = list(AdapterFn.apply(ad, condition_image_tensor, *_params(ad)))
        for f in residuals:
            if f.shape != h.shape:
                raise RuntimeError(f"condition residual {tuple(f.shape)} does not match hidden states {tuple(h.shape)}")

    for i, block in enumerate(model.transformer_blocks):
        if residuals:
            h = AddFn.apply(h, residuals.pop(0))                                                   # :491-494
        h, c = joint_block_train(block, h, c, st, I, keep=plan.decide(f"transformer_blocks.{i}", wants["joint"],
                                                                       joint_kept_bytes(block, h, c, I)))
        if model.enable_temporal and i in model.temporal_block_layers:
            k = model.temporal_block_layers.index(i)
            idx = torch.arange(Tn, device=dev).view(1, Tn, 1).expand(B, Tn, V)
            seq = ops.timestep_sinusoid(idx, D)
            use_cam = model.enable_crossview and not model.disable_view_emb_on_temporal_module and view_cam_emb is not None
            seq_emb = mlp_train(model.time_pos_embeds[k], seq, res=view_cam_emb if use_cam else None)
            rpe = N
            if model.enable_crossview and not model.disable_view_emb_on_temporal_module:           # :559-566
                seq_emb, rpe = with_rays(seq_emb)
            tt = model.temporal_attention_type
            mk = ops.rowmap_temporal_full if tt == "full" else \
                ops.rowmap_temporal_rowwise if tt == "rowwise" else ops.rowmap_temporal_pointwise
            alpha = alpha_train(model.time_mixers[k], disable_temporal, B)
            tblk, rm = model.temporal_transformer_blocks[k], mk(B, Tn, V, height, width)
            h = vt_block_train(tblk, h, rm, seq_emb, rpe, alpha, Tn * V * N,
                               keep=plan.decide(f"temporal_transformer_blocks.{k}", wants["temporal"],
                                                vt_kept_bytes(tblk, h, rm, seq_emb, alpha)))
        if model.enable_crossview and i in model.crossview_block_layers:
            k = model.crossview_block_layers.index(i)
            idx = torch.arange(V, device=dev).view(1, 1, V).expand(B, Tn, V)
            vemb = mlp_train(model.view_pos_embeds[k], ops.timestep_sinusoid(idx, D), res=view_cam_emb)
            vemb, rpe = with_rays(vemb)                                                             # :528-537
            ct = model.crossview_attention_type
            gmask = dmask = None
            if ct == "rowwise":
                rm = ops.rowmap_crossview_rowwise(B, Tn, V, height, width)
                gmask = crossview_attention_mask
            elif ct == "full":
                rm = ops.rowmap_crossview_full(B, Tn, V, height, width)
                dmask = crossview_attention_mask
            else:
                raise NotImplementedError(f"Not support {ct}")
            alpha = alpha_train(model.view_mixers[k], disable_crossview, B)
            cblk = model.crossview_transformer_blocks[k]
            h = vt_block_train(cblk, h, rm, vemb, rpe, alpha, Tn * V * N, group_mask=gmask, dense_mask=dmask,
                               keep=plan.decide(f"crossview_transformer_blocks.{k}", wants["crossview"],
                                                vt_kept_bytes(cblk, h, rm, vemb, alpha)))

    model.activation_plan = plan
    geom = (I, model.out_channels, height, width, p, N, D)
    out = OutFn.apply(model, geom, h, st, *(_params(model.norm_out) + _params(model.proj_out)))
    return out.view(B, Tn, V, model.out_channels, height * p, width * p)


# ------------------------------------------------------------------------------------------ optimizer
def _fp32_grad(p) -> Optional[torch.Tensor]:
    """the gradient of p as the optimizer step and the gradient norm read it: `None` if there is none, else its values as an fp32
    contiguous tensor - `p.grad` itself where it is one, a `.float()` / `.contiguous()` copy otherwise"""
    g = p.grad
    if g is None:
        return None
    return (g if g.dtype == torch.float32 else g.float()).contiguous()


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW semantics with the update done by the HIP kernel (`dwm_adamw_multi`, one launch per step count), which
    also refreshes the bf16 compute shadows of blocks.STORE.

    It IS a torch.optim.Optimizer: parameter groups, the (sparse) per-parameter state with its own step count, and the
    state-dict format are torch's bookkeeping, so `optimizer/<step>.pth` files interchange with the reference's
    torch.optim.AdamW (src/dwm/distributed.py:7-70) - including the warm-up configs whose `freezing_pattern` leaves frozen
    parameters in the list (ctsd.py:1014-1022, 1089-1092: the optimizer is built from ALL `model_wrapper.parameters()`) -
    and torch LR schedulers attach to it (ctsd.py:1098-1100, 1434-1435)."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                        foreach=None, capturable=False, differentiable=False, fused=None)
        super().__init__(params, defaults)

    # group-0 hyper-parameters (the trainer has one group) and the step count, for callers and tests
    lr = property(lambda self: self.param_groups[0]["lr"])
    betas = property(lambda self: tuple(self.param_groups[0]["betas"]))
    eps = property(lambda self: self.param_groups[0]["eps"])
    weight_decay = property(lambda self: self.param_groups[0]["weight_decay"])

    @property
    def t(self) -> int:
        """largest per-parameter step count"""
        return max((int(float(st["step"])) for st in self.state.values() if "step" in st), default=0)

    def _init_state(self, p) -> dict:
        """fresh state of p: step 0, zero fp32 moments"""
        st = self.state[p]
        st["step"] = torch.tensor(0.0)
        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
        return st

    @torch.no_grad()
    def step(self, closure=None, grad_scale: float = 1.0, device_operands: Optional[tuple] = None, ema: Optional["EMA"] = None):
        """the step of `AdamW` and of `AdamW8bit`: a parameter whose `exp_avg` is uint8 goes to the `dwm_adamw8_multi` batch of its
        step count, every other one to the `dwm_adamw_multi` batch; per group the 8-bit batches are launched first.
        ema (an `EMA`; None: every launch as without it): its counter advances, and its shadows move with this step's decay - in the
        same pass as the update for the parameters of a batch (`dwm_adamw_ema_multi` / `dwm_adamw8_ema_multi`; a batch without a
        single shadow takes the plain entry), in one `dwm_ema_multi` launch for the parameters that have a shadow but no gradient in
        this step.  With device_operands the decay travels in the fourth float of the hyper row and a set non-finite flag leaves
        the shadows alone as well; a given `hyper` tensor then needs that fourth float filled (`train_ops.adamw_hyper`).
        device_operands = (hyper, cond): the step is queued without a host read (`dwm_adamw_multi_dev` / `dwm_adamw8_multi_dev`).
        cond: None, or the device tensor `train_ops.grad_sumsq_multi` returned - the kernels take the gradient coefficient and the
        non-finite flag from it and change nothing when the flag is set; `grad_scale` is not used.  hyper: None - lr and the bias
        corrections of every batch (the values the by-value route passes) go to the device in ONE asynchronous copy from pinned
        memory - or a device tensor [>= 3] = (lr, bias_corr1, bias_corr2) used for every batch as it is.  The per-parameter step
        counts advance as if the step took place; a caller that later reads a set flag undoes that with `undo_step()`."""
        name = type(self).__name__
        self._last_stepped = []
        launches = []                           # (wrapper, lists, step, hyper) of the step, launched together at the end
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        omd, averaged = 0.0, set()              # 1 - decay of this step; data_ptr() of the parameters whose shadow moves inside a batch
        if ema is not None:
            if ema.swapped:
                raise RuntimeError(f"{name}.step(ema=...): the parameters and the shadows are exchanged (EMA.swap_()); swap back first")
            omd = ema.advance()
        for group in self.param_groups:
            if group.get("amsgrad") or group.get("maximize"):
                raise NotImplementedError(f"{name}: amsgrad / maximize")
            b1, b2 = group["betas"]
            hyper = dict(lr=float(group["lr"]), beta1=b1, beta2=b2, eps=group["eps"], weight_decay=group["weight_decay"],
                         grad_scale=grad_scale)
            batches8: dict = {}                 # step count -> lists for ONE dwm_adamw8_multi launch (normally a single batch)
            batches32: dict = {}                # the same for the fp32-moment tensors (dwm_adamw_multi)
            for p in group["params"]:
                g = _fp32_grad(p)
                if g is None:                   # frozen, or unused in this step: no state, no step (as torch)
                    continue
                if p.dtype != torch.float32:
                    raise RuntimeError(f"{name}: fp32 master parameters expected")
                st = self.state[p]
                if len(st) == 0:
                    st = self._init_state(p)
                st["step"] += 1
                self._last_stepped.append(p)
                shadow = STORE.bf(p) if refreshable(p) else None
                if shadow is None:
                    STORE.forget(p)                     # re-cast on next use
                if st["exp_avg"].dtype == torch.uint8:
                    batches, row = batches8, (p.data, g, st["exp_avg"], st["exp_avg_absmax"], st["exp_avg_sq"],
                                              st["exp_avg_sq_absmax"], shadow)
                elif p.is_contiguous() and st["exp_avg"].is_contiguous() and st["exp_avg_sq"].is_contiguous():
                    batches, row = batches32, (p.data, g, st["exp_avg"], st["exp_avg_sq"], shadow)
                else:
                    raise RuntimeError(f"{name}: the parameter of shape {tuple(p.shape)} or its moments are not contiguous "
                                       "(the kernels take contiguous tensors; there is no strided path)")
                if ema is not None:             # one more list per batch: the EMA shadow of p, or None
                    row += (ema.shadow_of(p),)
                step = int(st["step"].item())
                if step not in batches:
                    batches[step] = tuple([] for _ in row)
                for lst, t in zip(batches[step], row):
                    lst.append(t)
            for plain, fused, batches in ((T.adamw8_multi_, T.adamw8_ema_multi_, batches8), (T.adamw_multi_, T.adamw_ema_multi_, batches32)):
                for step, lists in batches.items():
                    if ema is None:
                        launches.append((plain, lists, step, hyper))
                    elif omd == 0.0 or not ema.fused or all(e is None for e in lists[-1]):     # nothing to average inside this batch
                        launches.append((plain, lists[:-1], step, hyper))
                    else:
                        averaged.update(t.data_ptr() for t, e in zip(lists[0], lists[-1]) if e is not None)
                        launches.append((fused, lists, step, dict(hyper, one_minus_decay=omd)))
        # shadows whose parameter is in no batch (no gradient in this step, or not this optimizer's): one launch of the average alone
        # (`lists[0]` holds `p.data`, a fresh tensor per access: the parameters are told apart by their storage)
        rest = []
        if ema is not None and omd != 0.0:
            rest = [(e, p.data) for p, e in ema.pairs() if p.data_ptr() not in averaged]
        if device_operands is None:
            for fn, lists, step, hyper in launches:
                fn(*lists, step=step, **hyper)
            if rest:
                T.ema_multi_([e for e, _ in rest], [p for _, p in rest], one_minus_decay=omd)
        elif launches or rest:
            given, cond = device_operands
            dev = launches[0][1][0][0].device if launches else rest[0][1].device
            if given is None:                   # one row of (lr, bias_corr1, bias_corr2, 1 - decay) per launch, one copy for all of them
                host = torch.empty((len(launches) + bool(rest), 4), dtype=torch.float32, pin_memory=True)
                for row, (_, _, step, hyper) in zip(host, launches):
                    T.adamw_hyper(hyper["lr"], hyper["beta1"], hyper["beta2"], step, out=row, one_minus_decay=omd)
                if rest:
                    host[-1].zero_()
                    host[-1, 3] = omd
                rows = host.to(dev, non_blocking=True)
            for i, (fn, lists, step, hyper) in enumerate(launches):
                fn(*lists, step=step, **hyper, device_operands=(rows[i] if given is None else given, cond))
            if rest:
                T.ema_multi_([e for e, _ in rest], [p for _, p in rest], device_operands=(rows[-1] if given is None else given, cond))
        STORE.bump(keep_shadows=True)
        return loss

    def undo_step(self) -> None:
        """take back the bookkeeping of the last `step(device_operands=...)` whose kernels found the non-finite flag set and left
        every tensor alone: the step counts go back by one, and a state that step created (zero moments, now step 0) is dropped,
        as if `step` had not been called"""
        for p in getattr(self, "_last_stepped", []):
            st = self.state[p]
            st["step"] -= 1
            if float(st["step"]) == 0.0:
                del self.state[p]
        self._last_stepped = []


class AdamW8bit(AdamW):
    """`AdamW` with both moments kept in the block-wise 8-bit format of opendwm_amd.quant8 (one byte per element and moment plus
    one fp32 scale per 256 elements: 2.03 bytes of state per parameter instead of 8), updated by `dwm_adamw8_multi`.  It fills the
    slot the reference's docs/CtsdPipelineFaqs.md ("Single GPU training", step 2) gives to `bitsandbytes.optim.Adam8bit`.

    State per quantised parameter: `step`, `exp_avg` (uint8, the parameter's shape), `exp_avg_absmax` (fp32 [ceil(n / 256)]),
    `exp_avg_sq`, `exp_avg_sq_absmax`.  Parameters of fewer than `min_8bit_size` elements keep fp32 moments; `AdamW.step`, the only
    `step`, sorts by the dtype of `exp_avg`.  The parameter update is computed from the fresh fp32 moments; quantisation only
    affects what the next step starts from.

    `load_state_dict` takes its own files and fp32-moment files (torch.optim.AdamW's, the reference's, `AdamW`'s: quantised on
    load); `state_dict_fp32()` hands the state back in torch.optim.AdamW's layout."""

    def __init__(self, params, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, min_8bit_size=4096):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.min_8bit_size = int(min_8bit_size)

    def _wants_8bit(self, p) -> bool:
        return p.numel() >= self.min_8bit_size and p.is_contiguous()

    def _init_state(self, p) -> dict:
        """fresh state of p: zero moments (8-bit: the code of 0.0 everywhere, scales 0)"""
        if not self._wants_8bit(p):
            return super()._init_state(p)
        st = self.state[p]
        st["step"] = torch.tensor(0.0)
        nb = quant8.n_blocks(p.numel())
        for key, signed in (("exp_avg", True), ("exp_avg_sq", False)):
            st[key] = torch.full(p.shape, quant8.zero_code(signed), dtype=torch.uint8, device=p.device)
            st[key + "_absmax"] = torch.zeros(nb, dtype=torch.float32, device=p.device)
        return st

    @torch.no_grad()
    def load_state_dict(self, state_dict) -> None:
        """own files (8-bit state) and fp32-moment files; the latter are quantised here for every tensor that wants 8 bits"""
        super().load_state_dict(state_dict)
        for p, st in self.state.items():
            if "exp_avg_absmax" in st:          # torch casts every state tensor to the parameter's dtype: codes back to bytes (exact)
                for key in ("exp_avg", "exp_avg_sq"):
                    st[key] = st[key].to(torch.uint8)
                    st[key + "_absmax"] = st[key + "_absmax"].to(torch.float32)
            elif "exp_avg" in st and self._wants_8bit(p):
                code_m, code_v = quant8.device_codes(p.device)
                for key, code, floor in (("exp_avg", code_m, False), ("exp_avg_sq", code_v, True)):
                    st[key], st[key + "_absmax"] = T.quantize_blockwise8(st[key].float().contiguous(), code, floor_positive=floor)

    @torch.no_grad()
    def state_dict_fp32(self) -> dict:
        """the state dict with every moment dequantised, in torch.optim.AdamW's layout: what torch.optim.AdamW, the reference's
        resume path and `AdamW` load"""
        sd = self.state_dict()
        params = [p for group in self.param_groups for p in group["params"]]
        ids = [i for group in sd["param_groups"] for i in group["params"]]
        state = {}
        for i, p in zip(ids, params):
            if i not in sd["state"]:
                continue
            st = dict(sd["state"][i])
            if "exp_avg_absmax" in st:
                code_m, code_v = quant8.device_codes(p.device)
                for key, code in (("exp_avg", code_m), ("exp_avg_sq", code_v)):
                    st[key] = T.dequantize_blockwise8(st[key], st.pop(key + "_absmax"), code)
            state[i] = st
        return {"state": state, "param_groups": sd["param_groups"]}


# ------------------------------------------------------------------------------------------ EMA of the weights
class EMA:
    """Exponential moving average of the trained weights with the semantics of diffusers 0.31 `EMAModel` (decay schedule and update
    formula), kept in one fp32 shadow per parameter that `requires_grad` and moved by the optimizer's own kernels
    (`AdamW.step(ema=...)`: `dwm_adamw_ema_multi` & co.).  Frozen parameters get no shadow: evaluating "with EMA" uses
    their own value.

    parameters: an iterable of parameters or of (name, parameter) pairs; the names key `state_dict()` (without names: "0", "1", ...).
    Shadows start as a copy of their parameter.

    The decay of the step with counter value n (`get_decay(n)`): s = max(0, n - update_after_step - 1); s <= 0: 0, else
    1 - (1 + s / inv_gamma) ** -power with `use_ema_warmup`, (1 + s) / (10 + s) without, clamped to [min_decay, decay].  A step
    then does  shadow += (1 - decay) * (parameter - shadow)  on the parameter the optimizer has just written.

    `optimization_step` advances on every optimizing call (`advance()`, which `AdamW.step(ema=...)` calls), as diffusers' `step()`
    does - including a call whose optimizer step was skipped for non-finite gradients.  ONE DELIBERATE DIFFERENCE from calling
    `EMAModel.step` after a skipped optimizer step: the skipped step leaves the shadows untouched here (diffusers would average the
    unchanged parameters in once more).  Only the counter moves, which is also what keeps the decay known on the host when the
    skip is decided on the device (`CTSDTrainer(graph=True)`).

    `swap_()` exchanges parameters and shadows in place (`dwm_ema_swap_multi`: no third copy, storage addresses unchanged, bf16
    compute copies that blocks.STORE refreshes in place rewritten by the same kernel, the others forgotten); `swapped` tells which
    way round they are.  `averaged_state_dict(model)` is `model.state_dict()` with the shadows substituted."""

    SETTINGS = ("decay", "min_decay", "update_after_step", "use_ema_warmup", "inv_gamma", "power")
    # True: `AdamW.step(ema=...)` moves the shadows inside the optimizer's launches.  False: the plain optimizer launches, then one
    # `dwm_ema_multi` launch over every shadow (the same element rule on the same p') - the two-launch route that
    # scripts/measure_ema.py times against the fused one.
    fused = True

    def __init__(self, parameters, decay: float = 0.9999, min_decay: float = 0.0, update_after_step: int = 0,
                 use_ema_warmup: bool = False, inv_gamma: float = 1.0, power: float = 2 / 3):
        if not 0.0 <= min_decay <= decay <= 1.0:
            raise ValueError(f"EMA: 0 <= min_decay <= decay <= 1 expected, got min_decay={min_decay!r}, decay={decay!r}")
        self.decay, self.min_decay, self.update_after_step = float(decay), float(min_decay), int(update_after_step)
        self.use_ema_warmup, self.inv_gamma, self.power = bool(use_ema_warmup), float(inv_gamma), float(power)
        self.optimization_step = 0
        self.swapped = False
        self._names, self._params, self._shadows = [], [], []
        for i, item in enumerate(parameters):
            name, p = item if isinstance(item, (tuple, list)) else (str(i), item)
            if not p.requires_grad or any(p is q for q in self._params):
                continue
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"EMA: parameter {name!r} is {p.dtype}, contiguous={p.is_contiguous()}; fp32 contiguous master "
                                 "parameters expected")
            self._names.append(str(name))
            self._params.append(p)
            self._shadows.append(p.detach().clone())
        self._by_id = {id(p): e for p, e in zip(self._params, self._shadows)}

    def get_decay(self, optimization_step: int) -> float:
        """the decay factor of the step that brings the counter to `optimization_step` (diffusers' EMAModel.get_decay)"""
        step = max(0, optimization_step - self.update_after_step - 1)
        if step <= 0:
            return 0.0
        if self.use_ema_warmup:
            cur = 1 - (1 + step / self.inv_gamma) ** -self.power
        else:
            cur = (1 + step) / (10 + step)
        return max(min(cur, self.decay), self.min_decay)

    def advance(self) -> float:
        """count one optimizing call and return its 1 - decay, the scalar the kernels take"""
        self.optimization_step += 1
        return 1.0 - self.get_decay(self.optimization_step)

    def shadow_of(self, p) -> Optional[torch.Tensor]:
        """the shadow held for the parameter `p`, or None"""
        return self._by_id.get(id(p))

    def pairs(self) -> list:
        """[(parameter, shadow)] in the order of construction"""
        return list(zip(self._params, self._shadows))

    def named_shadows(self) -> list:
        return list(zip(self._names, self._shadows))

    @torch.no_grad()
    def step(self) -> None:
        """the update alone, for callers with an optimizer of their own: counts the call and averages every parameter in
        (`dwm_ema_multi`, one launch)"""
        if self.swapped:
            raise RuntimeError("EMA.step: the parameters and the shadows are exchanged; swap back first")
        omd = self.advance()
        if omd != 0.0:
            T.ema_multi_(self._shadows, [p.data for p in self._params], one_minus_decay=omd)

    @torch.no_grad()
    def swap_(self) -> None:
        """parameters <-> shadows, in place; a second call restores every byte"""
        copies = []
        for p in self._params:
            c = STORE.shadow_of(p) if refreshable(p) else None
            if c is not None and (c.dtype != torch.bfloat16 or not c.is_contiguous() or c.numel() != p.numel()):
                c = None
            if c is None:
                STORE.forget(p)                         # re-cast on next use
            copies.append(c)
        T.ema_swap_multi_([p.data for p in self._params], self._shadows, copies)
        self.swapped = not self.swapped
        STORE.bump(keep_shadows=True)

    @torch.no_grad()
    def reset_(self) -> None:
        """shadows = the parameters as they are now, counter 0: the start of a run"""
        if self.swapped:
            raise RuntimeError("EMA.reset_: the parameters and the shadows are exchanged; swap back first")
        for p, e in zip(self._params, self._shadows):
            e.copy_(p.detach())
        self.optimization_step = 0

    def state_dict(self) -> dict:
        """{"shadows": {name: tensor}, the six settings, "optimization_step"}; not while exchanged (the shadows would be the raw
        weights)"""
        if self.swapped:
            raise RuntimeError("EMA.state_dict: the parameters and the shadows are exchanged; swap back first")
        sd = {k: getattr(self, k) for k in self.SETTINGS}
        sd["optimization_step"] = self.optimization_step
        sd["shadows"] = {n: e.detach() for n, e in zip(self._names, self._shadows)}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict: dict) -> None:
        if self.swapped:
            raise RuntimeError("EMA.load_state_dict: the parameters and the shadows are exchanged; swap back first")
        shadows = state_dict["shadows"]
        missing, unexpected = [n for n in self._names if n not in shadows], [n for n in shadows if n not in set(self._names)]
        if missing or unexpected:
            raise RuntimeError(f"EMA.load_state_dict: missing shadows {missing[:3]}, unexpected shadows {unexpected[:3]}")
        for n, e in zip(self._names, self._shadows):
            if tuple(shadows[n].shape) != tuple(e.shape):
                raise RuntimeError(f"EMA.load_state_dict: shadow {n!r} is {tuple(shadows[n].shape)}, expected {tuple(e.shape)}")
        for n, e in zip(self._names, self._shadows):
            e.copy_(shadows[n])
        self.decay, self.min_decay = float(state_dict["decay"]), float(state_dict["min_decay"])
        self.update_after_step, self.use_ema_warmup = int(state_dict["update_after_step"]), bool(state_dict["use_ema_warmup"])
        self.inv_gamma, self.power = float(state_dict["inv_gamma"]), float(state_dict["power"])
        self.optimization_step = int(state_dict["optimization_step"])

    def averaged_state_dict(self, model: torch.nn.Module) -> dict:
        """`model.state_dict()` (detached tensors that share the parameters' storage) with the averaged value in place of every entry
        that has one: what to write as an inference checkpoint, without exchanging anything.  While exchanged, the averaged values
        are the parameters themselves."""
        out = type(model.state_dict())()
        for k, v in model.state_dict(keep_vars=True).items():
            e = None if self.swapped else self._by_id.get(id(v))
            out[k] = v.detach() if e is None else e
        return out


# ------------------------------------------------------------------------------------------ gradient clip / loss scale
def _grad_list(parameters) -> list:
    """[(the parameter's grad, `_fp32_grad` of it)] of the parameters that have a gradient: what `AdamW.step` reads"""
    if torch.is_tensor(parameters):
        parameters = [parameters]
    return [(p.grad, _fp32_grad(p)) for p in parameters if p.grad is not None]


@torch.no_grad()
def grad_norm_and_coef(parameters, max_norm: Optional[float] = None, inv_scale: float = 1.0):
    """(total_norm, coef, found_inf) of the gradients of `parameters` in ONE read of them (`dwm_grad_sumsq_multi`) and one host
    sync: total_norm = the L2 norm of inv_scale * grad over the whole list (torch.nn.utils.clip_grad_norm_'s norm after
    GradScaler.unscale_), coef = inv_scale * min(1, max_norm / (total_norm + 1e-6)) - what `AdamW.step(grad_scale=coef)` needs to
    see the unscaled, clipped gradient without anyone rewriting it - and found_inf = some gradient element is inf or nan
    (GradScaler's test).  max_norm None: no clip, coef = inv_scale."""
    gs = [g for _, g in _grad_list(parameters)]
    total_norm, coef, found, _ = T.grad_sumsq_multi(gs, inv_scale, max_norm).tolist()
    return total_norm, coef, found != 0.0


@torch.no_grad()
def clip_grad_norm_(parameters, max_norm: float, inv_scale: float = 1.0) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (L2) for callers with an optimizer of their own: returns the total norm of
    inv_scale * grad and multiplies every gradient in place by coef = inv_scale * min(1, max_norm / (norm + 1e-6)) with one launch
    (`dwm_grad_scale_multi`); coef == 1.0 - torch multiplies by 1.0 there - launches nothing.  One host sync."""
    pairs = _grad_list(parameters)
    out = T.grad_sumsq_multi([g for _, g in pairs], inv_scale, max_norm)
    coef = float(out[1])
    if coef != 1.0:
        T.grad_scale_multi_([g for _, g in pairs], coef)
        for grad, g in pairs:
            if g is not grad:                   # the kernel scaled the fp32 / contiguous copy: hand the values back
                grad.copy_(g)
    return out[0]


class LossScaler:
    """The dynamic loss scale of torch.amp.GradScaler kept on the host, for a step whose non-finite flag already is on the host
    (`grad_norm_and_coef`): `scale(loss)` multiplies, `update(found_inf)` backs off (scale *= backoff_factor, tracker = 0) after
    a step that found an inf / nan, otherwise counts and grows (scale *= growth_factor, tracker = 0) every `growth_interval`
    clean steps.  The state dict has GradScaler's keys, so the two load each other's."""

    def __init__(self, init_scale: float = 65536.0, growth_factor: float = 2.0, backoff_factor: float = 0.5,
                 growth_interval: int = 2000):
        if growth_factor <= 1.0 or not 0.0 < backoff_factor < 1.0 or growth_interval < 1:
            raise ValueError("LossScaler: growth_factor > 1, 0 < backoff_factor < 1, growth_interval >= 1")
        self._scale = float(torch.tensor(init_scale, dtype=torch.float32))      # GradScaler keeps the scale in fp32
        self.growth_factor, self.backoff_factor, self.growth_interval = float(growth_factor), float(backoff_factor), int(growth_interval)
        self._growth_tracker = 0

    def scale(self, loss: torch.Tensor) -> torch.Tensor:
        return loss * self._scale

    def get_scale(self) -> float:
        return self._scale

    def update(self, found_inf: bool) -> None:
        if found_inf:
            self._scale, self._growth_tracker = self._scale * self.backoff_factor, 0
        else:
            self._growth_tracker += 1
            if self._growth_tracker == self.growth_interval:
                self._scale, self._growth_tracker = self._scale * self.growth_factor, 0
        self._scale = float(torch.tensor(self._scale, dtype=torch.float32))

    def state_dict(self) -> dict:
        return {"scale": self._scale, "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": self._growth_tracker}

    def load_state_dict(self, state_dict: dict) -> None:
        self._scale = float(state_dict["scale"])
        self.growth_factor, self.backoff_factor = float(state_dict["growth_factor"]), float(state_dict["backoff_factor"])
        self.growth_interval, self._growth_tracker = int(state_dict["growth_interval"]), int(state_dict["_growth_tracker"])
