"""Low-rank adapters (LoRA) for the linear layers of the MMDiT, held OUTSIDE the model so that the model's state dict keeps the
reference's keys (include/dwm_hip.h "Low-rank adapters").

An adapted weight is W + s * B A with W [N, K] the frozen fp32 master, A [r, K], B [N, r] fp32 and s = alpha / rank.  Nothing in the
forward or backward kernels knows about it: blocks.STORE keeps one bf16 compute copy per master, and `merge_()` writes
bf16(W + s B A) into that copy (`dwm_lora_merge_multi`) where a plain step has bf16(W).  The block Functions of opendwm_amd.train
produce the gradient dW of the adapted weight as they always do; `project_grads_()` turns it into dA = s B^T dW and
dB = s dW A^T (`dwm_lora_project_multi`) and drops it.  `fold_into_` / `unfold_from_` add / subtract s B A in a model's own
parameters (fp32 or bf16): how an adapter is applied for inference.

A compute copy does not outlive `STORE.bump()`, a state-dict load or `.to()`: the next forward would silently run the base model.
`merged()` says whether every copy written by the last `merge_()` is still the one the forward will read; CTSDTrainer asks before
every step."""
from __future__ import annotations

import math
import re
from collections import OrderedDict
from typing import List, Optional

import torch
from torch import nn

from . import train_ops as T
from .blocks import STORE, drop_caches

bf16 = torch.bfloat16
MAX_RANK = 64
# the attention projections of the joint and the cross-view / temporal blocks
DEFAULT_TARGET = r"(^|\.)(to_q|to_k|to_v|to_out\.0|add_[qkv]_proj|to_add_out)\.weight$"
# summed dA scratch of one dwm_lora_project_multi call (fp32 elements): longer lists are projected in several calls
PROJECT_SCRATCH_FLOATS = 1 << 26


class LoraAdapters(nn.Module):
    """LoraAdapters(model, rank=16, alpha=16.0, target=<regex searched in parameter names>, generator=None)

    Targets: every parameter of `model` whose name the pattern matches; each must be the 2-D fp32 `weight` of an nn.Linear with
    K % 4 == 0 (ValueError otherwise, and for rank outside 1..64 or a pattern that matches nothing).  A is kaiming-uniform with
    a = sqrt(5) (peft's convention: U(-1 / sqrt(K), 1 / sqrt(K))) drawn from `generator` on the CPU, B = 0, scale = alpha / rank.
    `parameters()` are the A and B tensors, in target order; `state_dict()` names them `<module path>.lora_A.weight` /
    `<module path>.lora_B.weight` and carries rank and alpha in its `_metadata[""]`."""

    def __init__(self, model: nn.Module, rank: int = 16, alpha: float = 16.0, target: str = DEFAULT_TARGET,
                 generator: Optional[torch.Generator] = None):
        super().__init__()
        rank = int(rank)
        if not 1 <= rank <= MAX_RANK:
            raise ValueError(f"LoraAdapters: rank must be in 1..{MAX_RANK} (the kernels keep A's tile in LDS), got {rank}")
        self.rank, self.alpha, self.target = rank, float(alpha), target
        linear_weights = {id(m.weight): name for name, m in model.named_modules() if isinstance(m, nn.Linear)}
        pat = re.compile(target)
        self.names: List[str] = []                 # parameter names of the targets, e.g. "transformer_blocks.0.attn.to_q.weight"
        targets = []
        for name, p in model.named_parameters():
            if pat.search(name) is None:
                continue
            if id(p) not in linear_weights or p.dim() != 2 or p.dtype != torch.float32:
                raise ValueError(f"LoraAdapters: target {name!r} is not the 2-D fp32 master weight of a linear layer "
                                 f"(shape {tuple(p.shape)}, {p.dtype})")
            if p.shape[1] % 4 != 0:
                raise ValueError(f"LoraAdapters: target {name!r} has K = {p.shape[1]}, not a multiple of 4")
            self.names.append(name)
            targets.append(p)
        if not targets:
            raise ValueError(f"LoraAdapters: the pattern {target!r} matches no parameter of the model")
        object.__setattr__(self, "_targets", targets)      # the model's parameters are not this module's
        A, B = [], []
        for p in targets:
            N, K = p.shape
            bound = 1.0 / math.sqrt(K)
            a = (torch.rand(rank, K, generator=generator) * 2.0 - 1.0) * bound
            A.append(nn.Parameter(a.to(p.device)))
            B.append(nn.Parameter(torch.zeros(N, rank, dtype=torch.float32, device=p.device)))
        self.lora_A, self.lora_B = nn.ParameterList(A), nn.ParameterList(B)
        self._merged = None                        # [(compute copy, master data_ptr, master version)] of the last merge_()
        self._tables = {}                          # tuple of shapes -> train_ops.LoraTables

    scale = property(lambda self: self.alpha / self.rank)

    def targets(self) -> List[nn.Parameter]:
        """the adapted parameters of the model, in the order of `names`"""
        return list(self._targets)

    def _tab(self, dev, shapes) -> "T.LoraTables":
        key = (str(dev), tuple(shapes))
        if key not in self._tables:
            self._tables[key] = T.LoraTables(dev, shapes)
        return self._tables[key]

    def _shapes(self, idx=None) -> tuple:
        idx = range(len(self._targets)) if idx is None else idx
        return tuple((self._targets[i].shape[0], self._targets[i].shape[1], self.rank) for i in idx)

    # ------------------------------------------------------------------------------------------------ merge / staleness
    @torch.no_grad()
    def merge_(self) -> None:
        """bf16(W + s B A) into the STORE compute copy of every target (made through STORE.bf where there is none), then
        STORE.bump(keep_shadows=True): packed / transposed operands are rebuilt from the copies by the next forward"""
        if STORE.precision != bf16:
            raise RuntimeError("LoraAdapters.merge_: the fp32 accuracy path reads the masters themselves; adapters need the bf16 "
                               "compute copies (STORE.set_precision(torch.bfloat16))")
        ps = self._targets
        copies = [STORE.bf(p) for p in ps]
        for p, c in zip(ps, copies):
            if c.dtype != bf16 or c.data_ptr() == p.data_ptr() or not c.is_contiguous():
                raise RuntimeError("LoraAdapters.merge_: a target has no bf16 compute copy of its own")
        T.lora_merge_multi([p.data for p in ps], [a.data for a in self.lora_A], [b.data for b in self.lora_B], copies,
                           [self.scale] * len(ps), tables=self._tab(ps[0].device, self._shapes()))
        self._merged = [(c, p.data_ptr(), p._version) for p, c in zip(ps, copies)]
        STORE.bump(keep_shadows=True)

    def merged(self) -> bool:
        """is every compute copy the last merge_() wrote still the one the next forward reads?  False before the first merge_(),
        after STORE.bump() / STORE.forget, after the model's load_state_dict or .to(), and after this module's load_state_dict."""
        if self._merged is None:
            return False
        for p, (c, ptr, version) in zip(self._targets, self._merged):
            if STORE.shadow_of(p) is not c or p.data_ptr() != ptr or p._version != version:
                return False
        return True

    # ------------------------------------------------------------------------------------------------ gradients
    @torch.no_grad()
    def project_grads_(self) -> None:
        """A.grad (+)= s B^T dW and B.grad (+)= s dW A^T from the `.grad` of every target that has one, which is then set to None.
        Existing adapter gradients are accumulated into (gradient accumulation: the projection is linear)."""
        fresh, more = [], []
        for i, p in enumerate(self._targets):
            if p.grad is None:
                continue
            (fresh if self.lora_A[i].grad is None and self.lora_B[i].grad is None else more).append(i)
        for idx, accumulate in ((fresh, False), (more, True)):
            start = 0
            while start < len(idx):                # calls of bounded scratch
                stop, floats = start, 0
                while stop < len(idx) and (stop == start or floats + self._scratch(idx[stop]) <= PROJECT_SCRATCH_FLOATS):
                    floats += self._scratch(idx[stop])
                    stop += 1
                self._project(idx[start:stop], accumulate)
                start = stop

    def _scratch(self, i: int) -> int:
        N, K = self._targets[i].shape
        return (N + T.LORA_DA_ROWS - 1) // T.LORA_DA_ROWS * self.rank * K

    def _project(self, idx, accumulate: bool) -> None:
        gs = []
        for i in idx:
            g = self._targets[i].grad
            gs.append(g if g.dtype in (torch.float32, bf16) and g.is_contiguous() else g.float().contiguous())
        A, B = [self.lora_A[i] for i in idx], [self.lora_B[i] for i in idx]
        for a, b in zip(A, B):
            for t in (a, b):
                if t.grad is None:
                    t.grad = torch.zeros_like(t) if accumulate else torch.empty_like(t)
        T.lora_project_multi(gs, [a.data for a in A], [b.data for b in B], [a.grad for a in A], [b.grad for b in B],
                             [self.scale] * len(idx), accumulate=accumulate, tables=self._tab(gs[0].device, self._shapes(idx)))
        for i in idx:
            self._targets[i].grad = None

    # ------------------------------------------------------------------------------------------------ fold / unfold
    def _fold(self, model: nn.Module, sign: float) -> None:
        params = dict(model.named_parameters())
        missing = [n for n in self.names if n not in params]
        if missing:
            raise KeyError(f"LoraAdapters: the model has no parameter {missing[0]!r} (and {len(missing) - 1} more)")
        ws = [params[n] for n in self.names]
        for n, w, t in zip(self.names, ws, self._targets):
            if w.shape != t.shape or w.dtype not in (torch.float32, bf16) or not w.is_contiguous():
                raise ValueError(f"LoraAdapters: {n!r} of the model is {tuple(w.shape)} {w.dtype}; a contiguous fp32 or bf16 "
                                 f"{tuple(t.shape)} weight expected")
        dev = ws[0].device
        with torch.no_grad():
            T.lora_merge_multi([w.data for w in ws], [a.data.to(dev) for a in self.lora_A], [b.data.to(dev) for b in self.lora_B],
                               [w.data for w in ws], [sign * self.scale] * len(ws), tables=self._tab(dev, self._shapes()))
        drop_caches(model)
        for w in ws:
            STORE.forget(w)
        STORE.bump(keep_shadows=True)              # operands derived from the old values (transposes, fused qkv) are rebuilt

    def fold_into_(self, model: nn.Module) -> None:
        """W <- W + s B A in the parameters of `model` that carry the targets' names, in their own dtype (fp32 masters or the bf16
        weights of an inference model); the model's caches and the compute copies of those parameters are dropped"""
        self._fold(model, 1.0)

    def unfold_from_(self, model: nn.Module) -> None:
        """W <- W - s B A: takes a fold back to within one rounding of the parameter's dtype per element"""
        self._fold(model, -1.0)

    # ------------------------------------------------------------------------------------------------ state
    def _keys(self, i: int) -> tuple:
        path = self.names[i][:-len(".weight")]
        return path + ".lora_A.weight", path + ".lora_B.weight"

    def state_dict(self, *args, destination=None, prefix: str = "", keep_vars: bool = False):
        sd = OrderedDict() if destination is None else destination
        for i in range(len(self.names)):
            ka, kb = self._keys(i)
            a, b = self.lora_A[i], self.lora_B[i]
            sd[prefix + ka], sd[prefix + kb] = (a, b) if keep_vars else (a.detach(), b.detach())
        if not hasattr(sd, "_metadata"):
            sd._metadata = OrderedDict()
        sd._metadata[prefix[:-1] if prefix else ""] = dict(version=1, rank=self.rank, alpha=self.alpha)
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = False):
        """A and B by the keys of `state_dict()`; alpha is taken from the metadata where it is there, a different rank is an error.
        The compute copies go stale: `merged()` is False afterwards."""
        meta = (getattr(state_dict, "_metadata", None) or {}).get("", {})
        if "rank" in meta and int(meta["rank"]) != self.rank:
            raise ValueError(f"LoraAdapters.load_state_dict: the file holds rank {meta['rank']}, these adapters rank {self.rank}")
        want = {}
        for i in range(len(self.names)):
            ka, kb = self._keys(i)
            want[ka], want[kb] = self.lora_A[i], self.lora_B[i]
        missing, unexpected = [k for k in want if k not in state_dict], [k for k in state_dict if k not in want]
        if strict and (missing or unexpected):
            raise RuntimeError(f"LoraAdapters.load_state_dict: missing keys {missing[:3]}, unexpected keys {unexpected[:3]}")
        for k, p in want.items():
            if k in state_dict:
                v = state_dict[k]
                if tuple(v.shape) != tuple(p.shape):
                    raise RuntimeError(f"LoraAdapters.load_state_dict: {k} is {tuple(v.shape)}, expected {tuple(p.shape)}")
                p.copy_(v)
        if "alpha" in meta:
            self.alpha = float(meta["alpha"])
        self._merged = None
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def held_bytes(self) -> int:
        """device memory of the adapters: A, B and the gradients they hold now"""
        n = 0
        for p in self.parameters():
            n += p.numel() * p.element_size()
            if p.grad is not None:
                n += p.grad.numel() * p.grad.element_size()
        return n
