"""CPU leg of the low-rank adapters (opendwm_amd/lora.py): targeting, key names, the refusals, the C ABI additions and
the host-side argument checks of the two entry points; and the proof that the element bounds of tests/lora_ref.py admit a correct
fp32 evaluation at the shapes of the GPU test and reject wrong ones."""
import ctypes
import os
import re

import pytest
import torch

from tests import lora_ref as R
from tests.common import small_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bf16, f32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def model():
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    return DiTCrossviewTemporalConditionModel(**small_config())


# ------------------------------------------------------------------------------------------------------------ the module
def test_default_targets_are_the_attention_projections(model):
    from opendwm_amd.lora import LoraAdapters
    la = LoraAdapters(model, rank=4, alpha=8.0, generator=torch.Generator().manual_seed(0))
    leaf = {n.split(".")[-2] if not n.endswith("to_out.0.weight") else "to_out.0" for n in la.names}
    assert leaf == {"to_q", "to_k", "to_v", "to_out.0", "add_q_proj", "add_k_proj", "add_v_proj", "to_add_out"}
    params = dict(model.named_parameters())
    # every 2-D attention projection of the joint, cross-view and temporal blocks, and nothing else
    want = [n for n, p in params.items() if p.dim() == 2 and re.search(r"\.(attn|attn1|attn2)\.", n) and n.endswith(".weight")]
    assert la.names == want and len(want) > 40
    assert any(n.startswith("crossview_transformer_blocks.") for n in want) and any(n.startswith("temporal_transformer_blocks.") for n in want)
    assert la.scale == 2.0 and len(list(la.parameters())) == 2 * len(want)
    for n, a, b in zip(la.names, la.lora_A, la.lora_B):
        N, K = params[n].shape
        assert tuple(a.shape) == (4, K) and tuple(b.shape) == (N, 4) and a.dtype == f32 and b.dtype == f32
        assert float(b.detach().abs().max()) == 0.0 and 0.0 < float(a.detach().abs().max()) <= K ** -0.5          # kaiming-uniform(a = sqrt 5): U(-1/sqrt K, 1/sqrt K)
    again = LoraAdapters(model, rank=4, generator=torch.Generator().manual_seed(0))
    assert all(torch.equal(a, b) for a, b in zip(la.lora_A, again.lora_A))
    # the adapters live outside the model: its keys are the reference's
    assert not any("lora" in k for k in model.state_dict()) and not la.merged()
    assert la.held_bytes() == sum(p.numel() * 4 for p in la.parameters())


def test_regex_targeting(model):
    from opendwm_amd.lora import LoraAdapters
    la = LoraAdapters(model, rank=2, target=r"^transformer_blocks\.1\.attn\.to_[qk]\.weight$")
    assert la.names == ["transformer_blocks.1.attn.to_q.weight", "transformer_blocks.1.attn.to_k.weight"]
    ff = LoraAdapters(model, rank=2, target=r"^transformer_blocks\.0\.ff\.net\.2\.weight")
    assert ff.names == ["transformer_blocks.0.ff.net.2.weight"] and ff.lora_A[0].shape[1] == model.transformer_blocks[0].ff.net[2].weight.shape[1]


def test_state_dict_keys_and_round_trip(model):
    from opendwm_amd.lora import LoraAdapters
    la = LoraAdapters(model, rank=3, alpha=6.0, target=r"transformer_blocks\.0\.attn\.(to_q|to_out\.0)\.weight$")
    sd = la.state_dict()
    assert list(sd) == ["transformer_blocks.0.attn.to_q.lora_A.weight", "transformer_blocks.0.attn.to_q.lora_B.weight",
                        "transformer_blocks.0.attn.to_out.0.lora_A.weight", "transformer_blocks.0.attn.to_out.0.lora_B.weight"]
    assert sd._metadata[""]["rank"] == 3 and sd._metadata[""]["alpha"] == 6.0
    with torch.no_grad():
        for b in la.lora_B:
            b.normal_()
    sd = la.state_dict()
    other = LoraAdapters(model, rank=3, alpha=1.0, target=la.target)
    other._merged = []                                   # as if merged: a load makes the copies stale
    other.load_state_dict(sd)
    assert other.alpha == 6.0 and other._merged is None and not other.merged()
    assert all(torch.equal(sd[k], v) for k, v in other.state_dict().items())
    with pytest.raises(ValueError):
        LoraAdapters(model, rank=2, target=la.target).load_state_dict(sd)                # another rank
    with pytest.raises(RuntimeError):
        other.load_state_dict({k: v for k, v in list(sd.items())[:2]})                   # strict


def test_constructor_refusals(model):
    from opendwm_amd.lora import LoraAdapters
    with pytest.raises(ValueError, match="rank"):
        LoraAdapters(model, rank=65)
    with pytest.raises(ValueError, match="rank"):
        LoraAdapters(model, rank=0)
    with pytest.raises(ValueError, match="2-D"):
        LoraAdapters(model, target=r"attn\.norm_q\.weight$")                              # a 1-D target
    with pytest.raises(ValueError, match="2-D"):
        LoraAdapters(model, target=r"transformer_blocks\.0\.attn\.to_q\.bias$")
    with pytest.raises(ValueError, match="matches no"):
        LoraAdapters(model, target=r"no_such_layer")
    lin = torch.nn.Sequential(torch.nn.Linear(6, 8))
    with pytest.raises(ValueError, match="multiple of 4"):
        LoraAdapters(lin, target=r"0\.weight$")
    with pytest.raises(ValueError, match="fp32"):
        LoraAdapters(torch.nn.Sequential(torch.nn.Linear(8, 8)).to(bf16), target=r"0\.weight$")


# ----------------------------------------------------------------------------------------------------------- the trainer
def test_trainer_refusals_and_freezing():
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.lora import LoraAdapters
    from opendwm_amd.pipeline import CTSDTrainer
    from opendwm_amd import train
    m = DiTCrossviewTemporalConditionModel(**small_config())
    with pytest.raises(ValueError, match="ddp"):
        CTSDTrainer(m, lora=dict(rank=4), ddp=True)
    with pytest.raises(ValueError, match="graph"):
        CTSDTrainer(m, lora=dict(rank=4), graph=True, grad_conditioning="fused")
    with pytest.raises(ValueError, match="rank"):
        CTSDTrainer(m, lora=dict(rank=65))
    assert all(p.requires_grad for p in m.parameters())                                   # a refusal changes nothing
    with pytest.raises(ValueError, match="another model"):
        CTSDTrainer(m, lora=LoraAdapters(DiTCrossviewTemporalConditionModel(**small_config()), rank=2))
    tr = CTSDTrainer(m, lora=dict(rank=4, alpha=8.0), optimizer_bits=8)
    assert isinstance(tr.lora, LoraAdapters) and isinstance(tr.optimizer, train.AdamW8bit)
    adapted = {id(p) for p in tr.lora.targets()}
    assert all(p.requires_grad == (id(p) in adapted) for p in m.parameters())
    opt = [p for g in tr.optimizer.param_groups for p in g["params"]]
    assert [id(p) for p in opt] == [id(p) for p in tr.lora.parameters()] and not {id(p) for p in opt} & {id(p) for p in m.parameters()}
    given = LoraAdapters(m, rank=2)
    assert CTSDTrainer(m, lora=given).lora is given


def test_unet_is_refused():
    from opendwm_amd.pipeline import CTSDTrainer
    from opendwm_amd.unet import UNetCrossviewTemporalConditionModel
    unet = UNetCrossviewTemporalConditionModel.__new__(UNetCrossviewTemporalConditionModel)       # the refusal needs no weights
    with pytest.raises(NotImplementedError, match="UNet"):
        CTSDTrainer(unet, lora=dict(rank=4))


def test_lora_none_is_the_trainer_as_before():
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    from opendwm_amd.pipeline import CTSDTrainer
    from opendwm_amd import train
    m = DiTCrossviewTemporalConditionModel(**small_config())
    tr = CTSDTrainer(m, training_config={"freezing_pattern": r"^pos_embed"})
    assert tr.lora is None and type(tr.optimizer) is train.AdamW
    opt = [p for g in tr.optimizer.param_groups for p in g["params"]]
    assert [id(p) for p in opt] == [id(p) for p in m.parameters()]                        # every parameter, frozen ones included
    frozen = {id(p) for p in m.pos_embed.parameters()}
    assert all(p.requires_grad == (id(p) not in frozen) for p in m.parameters())
    assert [id(p) for p in tr._optimized()] == [id(p) for p in m.parameters()]


# ----------------------------------------------------------------------------------------------------------------- C ABI
NEW = {"dwm_lora_merge_multi": 7, "dwm_lora_project_multi": 15, "dwm_lora_project_ws_floats": 3}


def test_header_declares_and_lib_binds_the_new_symbols():
    from opendwm_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
    assert re.search(rf"#define DWM_ABI_VERSION {_lib.ABI_VERSION}\b", hdr)                 # additions only: the version stays
    for name, arity in NEW.items():
        m = re.search(rf"^(?:int|int64_t) {name}\(([^;]*?)\);", hdr, flags=re.M | re.S)
        assert m and len(m.group(1).split(",")) == arity == len(_lib.SIGNATURES[name][1]), name
    body = hdr[hdr.index("typedef struct dwm_lora_item"):hdr.index("} dwm_lora_item;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    pos = -1
    for fname, _ in _lib.LoraItem._fields_:                                                # the ctypes mirror: same fields, same order
        m = re.search(rf"[\s\*,]{fname}\s*[,;]", body[pos + 1:])
        assert m, fname
        pos = pos + 1 + m.start()
    assert ctypes.sizeof(_lib.LoraItem) == 88
    assert "lora.hip" in build.SOURCES


def _fake_call(lib, name, rows, project, n_blocks=None, fin_chunk=1 << 14):
    """the entry point on a host item array with fake (aligned, never dereferenced) device addresses: the checks run before any launch"""
    from opendwm_amd import _lib
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    items = (_lib.LoraItem * len(rows))()
    cd = lambda a, b: (a + b - 1) // b
    sums = [0, 0, 0, 0]
    for it, (N, K, r, over) in zip(items, rows):
        it.w, it.a, it.b, it.out, it.out2, it.ws = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000
        it.N, it.K, it.r, it.flags, it.scale, it.n = N, K, r, 0, 1.0, r * K
        for k, v in over.items():
            setattr(it, k, v)
        sums = [sums[0] + cd(N, 32) * cd(K, 128), sums[1] + cd(N, 512) * cd(K, 128), sums[2] + cd(max(r * K, 1), fin_chunk), sums[3] + cd(N, 32)]
    fake = 0x70000
    if not project:
        return fn(ctypes.addressof(items), len(rows), fake, fake, fake, sums[0] if n_blocks is None else n_blocks, None)
    nb = sums[1:] if n_blocks is None else n_blocks
    return fn(ctypes.addressof(items), len(rows), fake, fake, fake, nb[0], fake, fake, nb[1], fin_chunk, fake, fake, nb[2], 0, None)


def test_entry_points_check_their_items_on_the_host():
    from opendwm_amd import build
    lib = ctypes.CDLL(build.build())
    EINVAL, EALIGN, EUNSUPPORTED = -1, -2, -3
    for name, project in (("dwm_lora_merge_multi", False), ("dwm_lora_project_multi", True)):
        assert _fake_call(lib, name, [(8, 64, 65, {})], project) == EUNSUPPORTED            # r > 64
        assert _fake_call(lib, name, [(8, 6, 2, {})], project) == EUNSUPPORTED              # K % 4 != 0
        assert _fake_call(lib, name, [(8, 64, 4, {}), (8, 64, 65, {})], project) == EUNSUPPORTED      # any item of the list
        assert _fake_call(lib, name, [(8, 64, 0, {})], project) == EINVAL
        assert _fake_call(lib, name, [(8, 64, 4, {"a": 0})], project) == EINVAL
        assert _fake_call(lib, name, [(8, 64, 4, {"n": 5})], project) == EINVAL
        assert _fake_call(lib, name, [(8, 64, 4, {"w": 0x10008})], project) == EALIGN
        assert _fake_call(lib, name, [(8, 64, 4, {"b": 0x30002})], project) == EALIGN
    assert _fake_call(lib, "dwm_lora_merge_multi", [(40, 200, 4, {})], False, n_blocks=3) == EINVAL      # 2 x 2 tiles, not 3
    assert _fake_call(lib, "dwm_lora_project_multi", [(40, 200, 4, {})], True, n_blocks=(2, 1, 3)) == EINVAL
    assert _fake_call(lib, "dwm_lora_project_multi", [(40, 200, 4, {})], True, fin_chunk=1000) == EINVAL
    assert _fake_call(lib, "dwm_lora_project_multi", [(8, 64, 4, {"ws": 0})], True) == EINVAL
    assert _fake_call(lib, "dwm_lora_project_multi", [(8, 64, 4, {"flags": 2})], True) == EINVAL         # dA / dB are fp32
    lib.dwm_lora_project_ws_floats.restype = ctypes.c_int64
    lib.dwm_lora_project_ws_floats.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_int32]
    assert lib.dwm_lora_project_ws_floats(1100, 132, 5) == 3 * 5 * 132 and lib.dwm_lora_project_ws_floats(512, 4, 1) == 4


def test_wrappers_refuse_what_is_not_on_the_device():
    from opendwm_amd import train_ops as T
    z = torch.zeros
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.lora_merge_multi([z(8, 64)], [z(4, 64)], [z(8, 4)], [z(8, 64)], [1.0])


# ----------------------------------------------------------------------------------------------------- the bounds bite
def _fp32_merge(W, A, B, s, out_dtype):
    """a correct fp32 evaluation in plain torch (its own summation order)"""
    return (W.float() + torch.tensor(s, dtype=f32) * (B @ A)).to(out_dtype)


@pytest.mark.parametrize("wd", [f32, bf16], ids=["w32", "wbf16"])
def test_bounds_admit_fp32_arithmetic_and_reject_wrong_results(wd):
    s = 0.75
    for N in R.NS:
        for K in R.KS:
            for r in R.RS:
                W, A, B, G = R.operands(N, K, r, 1000 + N + 7 * K + 13 * r, wd)
                exact, mag = R.merge_exact(W, A, B, s)
                for od in (bf16, wd):
                    assert R.ratio(_fp32_merge(W, A, B, s, od), exact, R.merge_bound(exact, mag, r, od)) <= 1, (N, K, r, od)
                (ea, ma), (eb, mb) = R.project_exact(G, A, B, s)
                Gf = G.float()
                assert R.ratio(s * (B.T @ Gf), ea, R.project_bound(ma, N)) <= 1 and R.ratio(s * (Gf @ A.T), eb, R.project_bound(mb, K)) <= 1
                old_a, old_b = torch.full((r, K), 0.01), torch.full((N, r), -0.01)
                (ea2, ma2), (eb2, mb2) = R.project_exact(G, A, B, s, old_a, old_b)
                assert R.ratio(old_a + s * (B.T @ Gf), ea2, R.project_bound(ma2, N)) <= 1
                assert R.ratio(old_b + s * (Gf @ A.T), eb2, R.project_bound(mb2, K)) <= 1
    # wrong results at one middle shape: factors rounded to bf16, a factor one row off, a missing scale, a truncated bf16 rounding
    N, K, r = 64, 192, 16
    W, A, B, G = R.operands(N, K, r, 5, wd)
    exact, mag = R.merge_exact(W, A, B, s)
    bound = R.merge_bound(exact, mag, r, bf16)
    assert R.ratio(_fp32_merge(W, A.to(bf16).float(), B, s, bf16), exact, bound) > 1
    assert R.ratio(_fp32_merge(W, A.roll(1, 0), B, s, bf16), exact, bound) > 1
    assert R.ratio(_fp32_merge(W, A, B, 1.0, bf16), exact, bound) > 1
    v = W.float() + s * (B @ A)
    assert R.ratio((v.view(torch.int32) & -65536).view(f32).to(bf16), exact, bound) > 1
    assert R.ratio(_fp32_merge(W, A, B, s, bf16).float(), exact, R.merge_bound(exact, mag, r, f32)) > 1      # a bf16 result is no fold
    (ea, ma), (eb, mb) = R.project_exact(G, A, B, s)
    Gf = G.float()
    assert R.ratio(s * (B.roll(1, 0).T @ Gf), ea, R.project_bound(ma, N)) > 1
    assert R.ratio(s * (Gf @ A.T)[:, torch.arange(r).roll(1)], eb, R.project_bound(mb, K)) > 1
    assert R.ratio(s * (B.T @ Gf).to(bf16).float(), ea, R.project_bound(ma, N)) > 1
    assert R.ratio(s * (B[:-1].T @ Gf[:-1]), ea, R.project_bound(ma, N)) > 1                               # the last row dropped
