"""CPU leg of the kept-activation mode of the SD 3.5 train step (CTSDTrainer(activations=..., activation_budget_gib=...)): how a
policy resolves per block family, how the byte budget plans a forward, what the byte counter says a kept block holds, and the C
surface of the two kernels that re-derive an activation inside its backward.  Nothing here needs a device."""
import itertools
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIB = 2 ** 30


# ------------------------------------------------------------------------------------------ policy
def test_policy_values_resolve_per_family():
    from opendwm_amd import train
    assert train.ACTIVATION_POLICIES == ("recompute", "keep", "config")
    for gc, tgc, cgc in itertools.product((False, True), repeat=3):
        assert train.resolve_activation_policy("recompute", gc, tgc, cgc) == dict(joint=False, temporal=False, crossview=False)
        assert train.resolve_activation_policy("keep", gc, tgc, cgc) == dict(joint=True, temporal=True, crossview=True)
        # "config": a family recomputes iff its reference switch is set
        assert train.resolve_activation_policy("config", gc, tgc, cgc) == dict(joint=not gc, temporal=not tgc, crossview=not cgc)
    for bad in ("Keep", "none", "", None, 1):
        with pytest.raises(ValueError):
            train.resolve_activation_policy(bad)


def test_model_attribute_and_trainer_arguments():
    """activation_policy is a plain attribute (default "recompute"), neither a constructor argument nor part of the config or the
    state dict; the trainer validates its two arguments and hands them to the model"""
    import inspect
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.pipeline import CTSDTrainer
    from tests.common import small_config
    assert DiTCrossviewTemporalConditionModel.activation_policy == "recompute"
    assert "activation_policy" not in inspect.signature(DiTCrossviewTemporalConditionModel.__init__).parameters
    m = DiTCrossviewTemporalConditionModel(**small_config())
    keys = set(m.state_dict())
    assert m.activation_policy == "recompute" and m.activation_budget_gib is None
    sig = inspect.signature(CTSDTrainer.__init__).parameters
    assert sig["activations"].default == "recompute" and sig["activation_budget_gib"].default is None
    tr = CTSDTrainer(m)
    assert (m.activation_policy, m.activation_budget_gib, tr.activation_plan) == ("recompute", None, None)
    tr = CTSDTrainer(m, activations="keep", activation_budget_gib=1.5)
    assert (m.activation_policy, m.activation_budget_gib) == ("keep", 1.5) and tr.activations == "keep"
    CTSDTrainer(m, activations="config")
    assert m.activation_policy == "config" and m.activation_budget_gib is None
    assert set(m.state_dict()) == keys and not any("activation" in k for k in keys)
    assert not any("activation" in k for k in vars(m.config))
    for bad in ("all", "KEEP", None, 0):
        with pytest.raises(ValueError):
            CTSDTrainer(m, activations=bad)
    with pytest.raises(ValueError):
        CTSDTrainer(m, activations="keep", activation_budget_gib=-1)
    assert m.activation_policy == "config"                     # a refused construction leaves the model alone


def test_unet_refuses_anything_but_recompute():
    from opendwm_amd.pipeline import CTSDTrainer
    from opendwm_amd.unet import UNetCrossviewTemporalConditionModel
    from tests.golden.make_golden import unet_small_config
    u = UNetCrossviewTemporalConditionModel(**unet_small_config())
    assert CTSDTrainer(u).is_unet and CTSDTrainer(u, activations="recompute", activation_budget_gib=2).activations == "recompute"
    for pol in ("keep", "config"):
        with pytest.raises(NotImplementedError, match="UNet"):
            CTSDTrainer(u, activations=pol)
    with pytest.raises(ValueError):
        CTSDTrainer(u, activations="nope")


# ------------------------------------------------------------------------------------------ budget
BLOCKS = [("a", True, 3 * GIB), ("b", True, 5 * GIB), ("c", False, 1 * GIB), ("d", True, 2 * GIB), ("e", True, 4 * GIB),
          ("f", True, 1 * GIB)]


def test_budget_none_keeps_every_wanted_block():
    from opendwm_amd import train
    plan = train.plan_activations(BLOCKS, None)
    assert plan.blocks == [("a", "keep", 3 * GIB), ("b", "keep", 5 * GIB), ("c", "recompute", 0), ("d", "keep", 2 * GIB),
                           ("e", "keep", 4 * GIB), ("f", "keep", 1 * GIB)]
    assert plan.total_bytes == 15 * GIB and len(plan) == 6 and list(plan) == plan.blocks


def test_budget_zero_keeps_nothing():
    from opendwm_amd import train
    plan = train.plan_activations(BLOCKS, 0)
    assert [b[1] for b in plan.blocks] == ["recompute"] * 6 and [b[0] for b in plan.blocks] == list("abcdef")
    assert plan.total_bytes == 0 and all(b[2] == 0 for b in plan.blocks)


def test_budget_fits_some_and_a_later_smaller_block_still_fits():
    """forward order, 6 GiB: a (3) fits, b (5) does not, c is not wanted, d (2) fits in the 3 left, e (4) does not fit in the 1 left,
    f (1) takes the last GiB exactly"""
    from opendwm_amd import train
    plan = train.plan_activations(BLOCKS, 6)
    assert plan.blocks == [("a", "keep", 3 * GIB), ("b", "recompute", 0), ("c", "recompute", 0), ("d", "keep", 2 * GIB),
                           ("e", "recompute", 0), ("f", "keep", 1 * GIB)]
    assert plan.total_bytes == 6 * GIB and plan.left == 0
    frac = train.plan_activations(BLOCKS, 3.5)                  # a fractional cap: a fits, nothing else fits in the 0.5 GiB left
    assert [b[1] for b in frac.blocks] == ["keep", "recompute", "recompute", "recompute", "recompute", "recompute"]
    with pytest.raises(ValueError):
        train.plan_activations(BLOCKS, -0.5)


# ------------------------------------------------------------------------------------------ byte counter
# one small shape: 3 images x 24 tokens, 10 context tokens, D = 128 (2 heads of 64), GELU width 512
I, N, LC, D, H, F = 3, 24, 10, 128, 2, 512
R, RC = I * N, I * LC            # 72 sample rows, 30 context rows
SHAPE = dict(images=I, tokens=N, context_tokens=LC, dim=D, heads=H, ff_inner=F)


def test_kept_bytes_joint_plain():
    from opendwm_amd import train
    bf16_elems = [R * D, RC * D, I * D,                 # inputs: h, c, st
                  I * 6 * D, I * 6 * D,                 # mod, cmod
                  R * 3 * D, RC * 3 * D,                # qkv, cqkv
                  R * D, RC * D,                        # ao, cao
                  R * D, R * D,                         # t_att, h1
                  R * F, R * D,                         # u, t_ff
                  RC * D, RC * D, RC * F, RC * D]       # t_catt, c1, cu, t_cff
    f32_elems = [I * H * (N + LC),                      # lse
                 R * 2 * H, RC * 2 * H]                 # rinv, crinv: one value per row and q / k head
    want = 2 * sum(bf16_elems) + 4 * sum(f32_elems)
    assert want == 2 * 161664 + 4 * 612 == 325776
    assert train.kept_bytes("joint", **SHAPE) == want
    # no q / k RMSNorm: no 1 / rms
    assert train.kept_bytes("joint", qk_norm=False, **SHAPE) == want - 4 * (R * 2 * H + RC * 2 * H)


def test_kept_bytes_joint_dual():
    from opendwm_amd import train
    bf16_elems = [R * D, RC * D, I * D, I * 9 * D, I * 6 * D, R * 3 * D, RC * 3 * D, R * D, RC * D, R * D, R * D, R * F, R * D,
                  RC * D, RC * D, RC * F, RC * D,
                  R * 3 * D, R * D, R * D]              # the second attention: qkv2, ao2, t_att2
    f32_elems = [I * H * (N + LC), R * 2 * H, RC * 2 * H,
                 I * H * N, R * 2 * H]                  # lse2, rinv2
    want = 2 * sum(bf16_elems) + 4 * sum(f32_elems)
    assert train.kept_bytes("joint", dual=True, **SHAPE) == want
    assert want - train.kept_bytes("joint", **SHAPE) == 2 * (I * 3 * D + 5 * R * D) + 4 * (I * H * N + R * 2 * H)


def test_kept_bytes_joint_context_pre_only():
    from opendwm_amd import train
    bf16_elems = [R * D, RC * D, I * D, I * 6 * D, I * 2 * D,      # cmod has two chunks, and the context stream ends after the attention
                  R * 3 * D, RC * 3 * D, R * D, RC * D, R * D, R * D, R * F, R * D]
    f32_elems = [I * H * (N + LC), R * 2 * H, RC * 2 * H]
    want = 2 * sum(bf16_elems) + 4 * sum(f32_elems)
    assert train.kept_bytes("joint", context_pre_only=True, **SHAPE) == want


def test_kept_bytes_vt():
    from opendwm_amd import train
    bf16_elems = [R * D, I * D,                         # inputs: h, emb (one row per image)
                  R * 2 * F, R * 2 * F,                 # u1, u3: the GEGLU projections, [value | gate]
                  R * 3 * D,                            # qkv
                  R * D, R * D, R * D, R * D]           # xs1, ao, xs2, out (before the blend)
    f32_elems = [2,                                     # alpha, one per sample
                 H * 96,                                # lse: 4 problems padded to 24 rows each
                 R * 2 * H]                             # rinv
    want = 2 * sum(bf16_elems) + 4 * sum(f32_elems)
    got = train.kept_bytes("vt", images=I, tokens=N, dim=D, heads=H, ff_inner=F, emb_rows=I, samples=2, lse_rows=96)
    assert got == want == 2 * 221568 + 4 * 482 == 445064
    # defaults: lse rows = the rows, ff_inner = 4 D
    assert train.kept_bytes("vt", images=I, tokens=N, dim=D, heads=H, emb_rows=I, samples=2) == want - 4 * H * (96 - R)
    with pytest.raises(ValueError):
        train.kept_bytes("unet", **SHAPE)


def test_kept_bytes_needs_no_device_and_matches_module_shapes():
    """the helpers that read the shapes off a block and its inputs agree with the counter; meta tensors: no storage, no device"""
    from opendwm_amd import train
    from opendwm_amd.blocks import JointTransformerBlock, VTSelfAttentionBlock
    h, c = torch.empty(R, D, device="meta"), torch.empty(RC, D, device="meta")
    for dual, pre in ((False, False), (True, False), (False, True)):
        blk = JointTransformerBlock(D, H, 64, context_pre_only=pre, qk_norm="rms_norm", use_dual_attention=dual)
        assert train.joint_kept_bytes(blk, h, c, I) == train.kept_bytes("joint", dual=dual, context_pre_only=pre, **SHAPE)
    vt = VTSelfAttentionBlock(D, D, H, 64, qk_norm="rms_norm")

    class Map:
        n_problems, L0 = 4, 24
    emb, alpha = torch.empty(I, D, device="meta"), torch.empty(2, device="meta")
    assert train.vt_kept_bytes(vt, h, Map, emb, alpha) == \
        train.kept_bytes("vt", images=I, tokens=N, dim=D, heads=H, ff_inner=F, emb_rows=I, samples=2, lse_rows=96)


# ------------------------------------------------------------------------------------------ ABI surface
def test_header_and_signatures_declare_the_recompute_kernels():
    from opendwm_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
    for name, arity in (("dwm_act_bwd_recompute", 7), ("dwm_geglu_bwd_recompute", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert m is not None, name
        assert len(m.group(1).split(",")) == arity, name
        res, args = _lib.SIGNATURES[name]
        assert len(args) == arity and res is _lib.SIGNATURES["dwm_act_bwd"][0]
    # (x, dy, y_out, dx, n, act, stream) and (u, ldu, dg, lddg, rows, inner, g_out, ldg, du, lddu, stream)
    i64, i32, vp = _lib.SIGNATURES["dwm_act_bwd"][1][3], _lib.SIGNATURES["dwm_act_bwd"][1][4], _lib.SIGNATURES["dwm_act_bwd"][1][0]
    assert _lib.SIGNATURES["dwm_act_bwd_recompute"][1] == [vp, vp, vp, vp, i64, i32, vp]
    assert _lib.SIGNATURES["dwm_geglu_bwd_recompute"][1] == [vp, i64, vp, i64, i64, i64, vp, i64, vp, i64, vp]
    assert _lib.ABI_VERSION == 18 and re.search(r"#define DWM_ABI_VERSION 18\b", hdr)          # additions only
