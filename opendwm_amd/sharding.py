"""Intra-sample sharding of ONE multi-view video across GPUs (not in the reference, which only
ever runs whole samples per GPU: src/dwm/train.py:116-122).

Shard axis = frames.  With the frames of a sample split over R ranks

  * the joint MMDiT blocks, the embeddings, the ImageAdapter, the CFG combine and the scheduler update are per image
    -> local;
  * the cross-view blocks attend over the views of ONE frame (crossview_temporal_dit.py:223-327) -> local;
  * the temporal blocks attend over all frames of one (view, token row / token) (:329-370) -> the hidden state is
    re-sharded from "my frames, all token rows" to "all frames, my token rows" with ONE all-to-all before the block and
    one after it (RCCL over xGMI: every rank sends 1/R of its shard to every peer, which is the full-mesh traffic
    pattern the point-to-point links are built for).  Everything inside the temporal block except its attention is
    row-wise, so the block runs unchanged on the re-sharded rows.

Per denoise step at BASELINE config 3 / 8 GPUs: 24 all-to-alls of 33 MB per rank (29 MB leave the GPU).
That row re-shard (`temporal_exchange="rows"`, the default) serves "rowwise" and "pointwise" temporal attention (a token row
never mixes with another one) where the token rows split over the ranks.  "full" temporal attention couples every token of a
view - a problem is one (batch, view) with T x h x w tokens and leaves no token-row axis to split - and would have to shard by
view instead, or exchange HEADS:

`temporal_exchange="heads"` (or "auto") keeps the block on "my frames, all token rows" for all of its row-wise work and, around the
attention alone, exchanges "my frames, all heads" for "all frames, my heads" (attention is independent per head): the fused
q | k | v projection out, the attention output back - four exchanges per temporal block instead of two, 4 / R of one sample's
hidden state per rank and block, no duplicated work, and no `height % R` condition (it needs `heads % R == 0`).  The pack /
unpack of these exchanges is dwm_head_exchange (runs of (heads / R) * 64 channels: too small for dwm_block_permute's one
workgroup per block); the attention addresses the received buffer through ops.rowmap_temporal_*_exchanged."""
from __future__ import annotations

from typing import Optional

import torch
import torch.distributed as dist


def all_to_all_chunks(out: torch.Tensor, inp: torch.Tensor, group) -> None:
    """out[j] <- rank j's inp[my rank]; both [R, ...] contiguous.  RCCL for device tensors; the gloo backend (CPU
    tests, and the two-ranks-on-one-GPU test) only moves host memory, so device tensors are staged through it there."""
    if dist.get_backend(group) == "gloo" and inp.is_cuda:
        o = torch.empty(out.shape, dtype=out.dtype)
        dist.all_to_all_single(o, inp.cpu(), group=group)
        out.copy_(o)
        return
    dist.all_to_all_single(out, inp, group=group)


def _permute_blocks(src: torch.Tensor, dims, src_strides, block_elems: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """a dense copy of `src`'s blocks in the order `dims`, block (i0..i3) taken from block index sum(i_k * src_strides[k]) of `src`:
    ONE HIP launch (dwm_block_permute) for device tensors - the pack / unpack of the exchange is not torch glue; host tensors (the
    gloo CPU tests) go through the equivalent torch view"""
    out = torch.empty_like(src) if out is None else out
    if out.numel() != src.numel() or out.dtype != src.dtype or not out.is_contiguous():
        raise ValueError("_permute_blocks: `out` must be a contiguous tensor of the source's size and dtype")
    if src.is_cuda:
        from . import ops
        return ops.block_permute(src, out, dims, src_strides, block_elems)
    flat = src.reshape(-1, block_elems)
    idx = sum(torch.arange(dims[k]).view([-1 if i == k else 1 for i in range(4)]) * src_strides[k] for k in range(4)).reshape(-1)
    out.view(-1, block_elems).copy_(flat[idx])
    return out


def _head_exchange(src: torch.Tensor, dst: torch.Tensor, rows: int, S: int, R: int, Dr: int, merge: bool) -> torch.Tensor:
    """[rows][S][R][Dr] (row-major side: 2-D, rows may be strided) <-> dense [R][rows][S][Dr]: ONE HIP launch (dwm_head_exchange) for
    device tensors; host tensors (the gloo CPU tests) go through the equivalent torch view"""
    if src.is_cuda:
        from . import ops
        return ops.head_exchange(src, dst, rows, S, R, Dr, merge=merge)
    wide, dense = (dst, src) if merge else (src, dst)
    if wide.dim() != 2 or wide.stride(1) != 1 or tuple(wide.shape) != (rows, S * R * Dr) or dense.numel() != wide.numel() \
            or not dense.is_contiguous() or dense.dtype != wide.dtype:
        raise ValueError("_head_exchange: [rows, S * R * Dr] with contiguous rows and a dense tensor of its size and dtype expected")
    w4, d4 = wide.view(rows, S, R, Dr), dense.view(R, rows, S, Dr)
    if merge:
        w4.copy_(d4.permute(1, 2, 0, 3))
    else:
        d4.copy_(w4.permute(2, 0, 1, 3))
    return dst


class FrameShard:
    """The frame-axis shard of one rank: rank r of R holds frames [r*T/R, (r+1)*T/R)."""

    def __init__(self, group=None, temporal_exchange: str = "rows"):
        """temporal_exchange: what the temporal blocks exchange - "rows" (token rows: rowwise / pointwise attention, height % R == 0),
        "heads" (attention heads: full / rowwise attention, heads % R == 0) or "auto" (rows where they serve, else heads)"""
        if temporal_exchange not in ("rows", "heads", "auto"):
            raise ValueError(f"temporal_exchange must be 'rows', 'heads' or 'auto', not {temporal_exchange!r}")
        self.group = group if group is not None else dist.group.WORLD
        self.size = dist.get_world_size(self.group)
        self.rank = dist.get_rank(self.group)
        self.temporal_exchange = temporal_exchange

    def frame_range(self, total_frames: int):
        if total_frames % self.size:
            raise ValueError(f"{total_frames} frames do not split over {self.size} ranks")
        n = total_frames // self.size
        return self.rank * n, (self.rank + 1) * n

    def check(self, height: int, temporal_attention_type: str):
        if temporal_attention_type not in ("rowwise", "pointwise"):
            raise NotImplementedError(f"frame sharding by token rows supports rowwise / pointwise temporal attention, not "
                                      f"{temporal_attention_type!r} (the head exchange does: temporal_exchange='heads')")
        if height % self.size:
            raise ValueError(f"{height} token rows do not split over {self.size} ranks")

    def plan(self, height: int, heads: int, temporal_attention_type: str) -> str:
        """what the temporal blocks of a model exchange, "rows" or "heads"; raises where `temporal_exchange` cannot serve it"""
        tt = temporal_attention_type
        if self.temporal_exchange == "rows":
            self.check(height, tt)
            return "rows"
        if self.temporal_exchange == "auto" and tt in ("rowwise", "pointwise") and height % self.size == 0:
            return "rows"
        if tt not in ("full", "rowwise"):
            # pointwise: sequences of T tokens - an exchange of all of q, k, v for them is not worth building
            raise NotImplementedError(f"the head exchange supports full / rowwise temporal attention, not {tt!r}")
        if heads % self.size:
            raise ValueError(f"{heads} attention heads do not split over {self.size} ranks")
        return "heads"

    # ---- [B, Tl, V, height, width] rows of my frames  <->  [B, T, V, height / R, width] rows of all frames
    def frames_to_rows(self, h: torch.Tensor, B: int, Tl: int, V: int, height: int, width: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        R, D = self.size, h.shape[-1]
        hl = height // R
        blk = hl * width * D                                                                       # one (image, row block): contiguous
        h = h.contiguous()
        # pack: [b, tl, v, j] blocks -> [dest j][b, tl, v]
        send = _permute_blocks(h, (R, B, Tl, V), (1, Tl * V * R, V * R, R), blk)
        recv = torch.empty_like(send)
        all_to_all_chunks(recv.view(R, -1), send.view(R, -1), self.group)                          # [src j = frame block][b, tl, v]
        # unpack: -> [b, j, tl, v] = all frames (j, tl) of my token rows
        return _permute_blocks(recv, (B, R, Tl, V), (Tl * V, B * Tl * V, V, 1), blk, out=out).view(B * R * Tl * V * hl * width, D)

    def rows_to_frames(self, hx: torch.Tensor, B: int, Tl: int, V: int, height: int, width: int,
                       out: Optional[torch.Tensor] = None) -> torch.Tensor:
        R, D = self.size, hx.shape[-1]
        hl = height // R
        blk = hl * width * D
        hx = hx.contiguous()
        # pack: [b, j, tl, v] blocks -> [dest j = frame block][b, tl, v]
        send = _permute_blocks(hx, (R, B, Tl, V), (Tl * V, R * Tl * V, V, 1), blk)
        recv = torch.empty_like(send)
        all_to_all_chunks(recv.view(R, -1), send.view(R, -1), self.group)                          # [src j = row block][b, tl, v]
        # unpack: -> [b, tl, v, j] = all token rows of my frames
        return _permute_blocks(recv, (B, Tl, V, R), (Tl * V, V, 1, B * Tl * V), blk, out=out).view(B * Tl * V * height * width, D)

    # ---- [rows of my frames, S x (all heads)]  <->  [src rank i][rows of its frames, S x (my heads)]
    def heads_gather(self, qkv: torch.Tensor, rows: int, S: int) -> torch.Tensor:
        """qkv [rows, S * D]: S stacked tensors (q | k | v) of all heads for the rows of MY frames (rows may be strided: a column
        slice).  Returns [R * rows, S * Dr], Dr = D / R: MY head group of every rank's rows, ordered (source rank i, row) as received
        - with rows = (b, tl, v, n) that is the order of ops.rowmap_temporal_*_exchanged, and it is not unpacked."""
        R = self.size
        if qkv.dim() != 2 or qkv.shape[0] != rows or qkv.shape[1] % (S * R):
            raise ValueError(f"heads_gather: [{rows}, {S} x (a multiple of {R} head groups)] expected, got {tuple(qkv.shape)}")
        Dr = qkv.shape[1] // (S * R)
        send = _head_exchange(qkv, torch.empty(R, rows, S, Dr, dtype=qkv.dtype, device=qkv.device), rows, S, R, Dr, merge=False)
        recv = torch.empty_like(send)
        all_to_all_chunks(recv.view(R, -1), send.view(R, -1), self.group)                          # [src i][rows][S][Dr]
        return recv.view(R * rows, S * Dr)

    def heads_scatter(self, out_x: torch.Tensor, rows: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out_x [R * rows, Dr]: MY head group of every rank's rows, ordered (rank i, row) (the attention output on the received
        layout).  Returns [rows, D]: all heads of MY rows (written into `out` if given)."""
        R = self.size
        if out_x.dim() != 2 or out_x.shape[0] != R * rows or not out_x.is_contiguous():
            raise ValueError(f"heads_scatter: a contiguous [{R} * {rows}, Dr] expected, got {tuple(out_x.shape)}")
        Dr = out_x.shape[1]
        recv = torch.empty_like(out_x)
        all_to_all_chunks(recv.view(R, -1), out_x.view(R, -1), self.group)                         # [head group j][rows][Dr]
        if out is None:
            out = torch.empty(rows, R * Dr, dtype=out_x.dtype, device=out_x.device)
        return _head_exchange(recv, out, rows, 1, R, Dr, merge=True)

    def gather_frames(self, x: torch.Tensor, frame_dim: int = 1) -> torch.Tensor:
        """all ranks' frame blocks concatenated along `frame_dim` (per-image vectors, final latents)."""
        x = x.contiguous()
        parts = [torch.empty_like(x) for _ in range(self.size)]
        dist.all_gather(parts, x, group=self.group)
        return torch.cat(parts, frame_dim)
