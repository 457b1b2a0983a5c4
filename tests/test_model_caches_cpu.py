"""blocks.STORE.memo - the one cache of what a module keeps between forwards - and blocks.drop_caches, on CPU modules: the memo's
semantics with a counting `make`, the VAE blocks' packs following their weights (and not the optimizer step), and `held_tensors`
(tests/common.py, which knows no attribute names) finding every cache and finding nothing after the drop."""
import copy
import types

import pytest
import torch
from torch import nn

from opendwm_amd import blocks, dit, vae
from opendwm_amd.blocks import STORE, drop_caches
from tests.common import held_tensors

bf16 = torch.bfloat16


@pytest.fixture(autouse=True)
def _bf16_store():
    STORE.set_precision(bf16)
    yield
    STORE.set_precision(bf16)


class _Counting:
    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return torch.full((2,), float(self.calls))


def test_memo_hit_bump_and_key():
    owner, make = nn.Identity(), _Counting()
    a = STORE.memo(owner, "w", (1, 2), make)
    assert STORE.memo(owner, "w", (1, 2), make) is a and make.calls == 1                  # a hit: the same object
    keep = STORE.memo(owner, "grid", (1, 2), make, per_step=False)
    STORE.bump()
    assert STORE.peek(owner, "w") is None and STORE.peek(owner, "grid") is keep           # stale after the step / not per step
    b = STORE.memo(owner, "w", (1, 2), make)
    assert b is not a and make.calls == 3                                                 # per_step: rebuilt after bump() ...
    assert STORE.memo(owner, "grid", (1, 2), make, per_step=False) is keep and make.calls == 3      # ... iff per_step
    c = STORE.memo(owner, "w", (1, 3), make)
    assert c is not b and make.calls == 4 and STORE.peek(owner, "w") is c                 # a changed key rebuilds ...
    assert STORE.memo(owner, "w", (1, 2), make) is not b and make.calls == 5              # ... and REPLACED the entry
    assert set(vars(owner)["_memo"]) == {"w", "grid"}
    assert "_memo" not in owner.state_dict() and not list(owner.buffers()) and not list(owner.children())


def test_memo_precisions_side_by_side_and_drop():
    owner, make = nn.Identity(), _Counting()
    by = {}
    for dt in (bf16, torch.float32, bf16, torch.float32):
        STORE.set_precision(dt)
        by.setdefault(dt, []).append(STORE.memo(owner, ("w", STORE.precision), None, make))
    assert make.calls == 2 and by[bf16][0] is by[bf16][1] and by[torch.float32][0] is by[torch.float32][1]
    other = STORE.memo(owner, "other", None, make)
    STORE.drop(owner, ("w", bf16))
    assert STORE.peek(owner, ("w", bf16)) is None
    assert STORE.peek(owner, ("w", torch.float32)) is by[torch.float32][0] and STORE.peek(owner, "other") is other
    STORE.drop(owner)
    assert STORE.peek(owner, "other") is None and not held_tensors(owner)
    STORE.drop(owner)                                                                      # (nothing to drop: no error)
    STORE.drop(owner, "other")


def test_cached_is_per_precision_and_per_step():
    owner, make = nn.Identity(), _Counting()
    a = STORE.cached(owner, make)
    STORE.set_precision(torch.float32)
    b = STORE.cached(owner, make)
    STORE.set_precision(bf16)
    assert STORE.cached(owner, make) is a and b is not a and make.calls == 2
    STORE.bump()
    assert STORE.cached(owner, make) is not a and make.calls == 3


def _other_weights(module, seed):
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randn(v.shape, generator=g) for k, v in module.state_dict().items()}


def _equal_packs(a: dict, b: dict) -> bool:
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("make_block", [lambda: vae.ResnetBlock2D(32, 64), lambda: vae._VaeAttention(64)], ids=["resnet", "attention"])
def test_vae_block_packs_follow_their_weights(make_block):
    """a state-dict load and an `_apply` rebuild the packed weights of a VAE block (they did not: the block handed out the packs of
    the weights it was first run with); an optimizer step - of some other model: the VAE is frozen - does not"""
    torch.manual_seed(0)
    block = make_block()
    first = block.packed()
    assert block.packed() is first
    STORE.bump()
    assert block.packed() is first                                    # object identity: not rebuilt by a step
    sd = _other_weights(block, 1)
    block.load_state_dict(sd)
    fresh = make_block()
    fresh.load_state_dict(sd)
    got = block.packed()
    assert got is not first and _equal_packs(got, fresh.packed()) and not _equal_packs(got, first)
    moved = copy.deepcopy(block).to(torch.float64).to(torch.float32)
    with torch.no_grad():
        for p in moved.parameters():
            p.mul_(0.5)
    fresh.load_state_dict(moved.state_dict())
    assert _equal_packs(moved.packed(), fresh.packed()) and not _equal_packs(moved.packed(), got)
    assert block.packed() is got                                      # (the copy's caches are its own)


def _populated_root():
    torch.manual_seed(0)
    root = nn.Module()
    root.attn = blocks.Attention(128, 2, 64, bias=True, added_kv=True, qk_norm="rms_norm")
    root.patch = dit.PatchEmbed(32, 2, 4, 64, 16)
    root.mixer = blocks.AlphaBlender(0.3, merge_strategy="learned_with_images")
    root.res = vae.ResnetBlock2D(32, 64)
    root.attn.packed()
    root.patch.cropped(4, 4)
    root.patch.packed_weight()
    root.mixer.get_alpha(torch.tensor([False, True]), 2)
    root.res.packed()
    return root


def test_held_tensors_finds_every_cache_and_none_after_the_drop():
    root = _populated_root()
    owners = {id(t) for t in list(root.parameters()) + list(root.buffers())}
    held = held_tensors(root)
    assert held and not any(id(t) in owners for t in held)
    # each populated module contributes: its packs / table / alpha are among the held tensors
    ptrs = {t.data_ptr() for t in held}
    pk = root.attn.packed()
    assert {pk["wqkv"].data_ptr(), pk["rms_ps"].data_ptr(), pk["wadd"].data_ptr()} <= ptrs
    assert {root.patch.cropped(4, 4).data_ptr(), root.patch.packed_weight().data_ptr(), root.res.packed()["w1"].data_ptr()} <= ptrs
    root.plain = {"anywhere": [types.SimpleNamespace(t=torch.zeros(3))]}                    # a cache under a name nobody lists
    assert any(t is root.plain["anywhere"][0].t for t in held_tensors(root))
    del root.plain
    drop_caches(root)
    assert held_tensors(root) == []
    assert torch.equal(root.attn.packed()["wqkv"], pk["wqkv"]) and root.attn.packed()["wqkv"] is not pk["wqkv"]


def test_patch_embed_table_survives_a_step_and_the_packed_weight_does_not():
    pe = dit.PatchEmbed(32, 2, 4, 64, 16)
    table, w = pe.cropped(4, 4), pe.packed_weight()
    assert pe.cropped(4, 4) is table and pe.packed_weight() is w
    STORE.bump()
    assert pe.cropped(4, 4) is table and pe.packed_weight() is not w
    STORE.set_precision(torch.float32)
    t32 = pe.cropped(4, 4)
    STORE.set_precision(bf16)
    assert t32.dtype == torch.float32 and pe.cropped(4, 4) is table                       # both precisions side by side
    assert pe.cropped(4, 6) is not table and pe.cropped(4, 4) is not table                # another crop replaced the entry


def test_alpha_is_kept_per_indicator_object_and_step():
    mixer = blocks.AlphaBlender(0.3, merge_strategy="learned_with_images")
    ind = torch.tensor([False, True])
    a = mixer.get_alpha(ind, 2)
    assert mixer.get_alpha(ind, 2) is a
    assert mixer.get_alpha(ind.clone(), 2) is not a                                       # equal values, another tensor object
    b = mixer.get_alpha(ind, 2)
    ind[0] = True                                                                         # written in place: its version changes
    c = mixer.get_alpha(ind, 2)
    assert c is not b and c.tolist() == [1.0, 1.0]
    STORE.bump()
    assert mixer.get_alpha(ind, 2) is not c
