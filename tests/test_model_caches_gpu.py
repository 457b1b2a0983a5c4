"""GPU leg (`-m gpu`) of the model caches (blocks.STORE.memo, blocks.drop_caches): what the small models keep between
forwards, found by `held_tensors` (tests/common.py: any attribute of any module, no names known).

Per model - the small MMDiT with and without its layout adapter, the small SD 2.1 UNet, the small AutoencoderKL and the small
CogVideoX VAE - a second forward on the same inputs rebuilds nothing, `drop_caches` leaves nothing held, the forward after the drop
computes the same bits, and after an optimizer step's `STORE.bump(keep_shadows=True)` the entries that depend on the weights are new
objects while scratch grids and position tables are the same ones.  Per trainer kind: after the first captured step of
CTSDTrainer(graph=True) the model holds nothing (so nothing outside the trainer points into the capture's pool) and the compute
copies the graph reads are the ones the store hands out."""
import pytest
import torch

from tests.common import held_tensors, small_config, to_dev
from tests.test_cogvideox_gpu import _bf_sd, _model as _cogvideox_model, small_cfg as cogvideox_cfg
from tests.test_deterministic_train_gpu import _unet_case
from tests.test_train_graph_gpu import KINDS, _mmdit_case, _run
from tests.test_vae_attention_gpu import small_vae  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, pytest.mark.quick]
bf16 = torch.bfloat16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _entries(model) -> dict:
    """(module name, tag) -> (per step?, value) of every memo entry of the model"""
    return {(name, tag): (full[1] is not None, value)
            for name, m in model.named_modules() for tag, (full, value) in vars(m).get("_memo", {}).items()}


def _check_caches(model, run):
    """the four properties of the module docstring; `run()` -> output tensor, on the same input objects every time"""
    from opendwm_amd.blocks import STORE, drop_caches
    drop_caches(model)
    assert held_tensors(model) == []
    out1 = run()
    ptrs1 = {t.data_ptr() for t in held_tensors(model)}
    out2 = run()
    ptrs2 = {t.data_ptr() for t in held_tensors(model)}
    assert ptrs1 and ptrs1 == ptrs2                                    # the second forward rebuilt nothing
    before = _entries(model)
    STORE.bump(keep_shadows=True)
    out3 = run()
    after = _entries(model)
    assert set(after) == set(before)
    stepped = [k for k, (per_step, _) in before.items() if per_step]
    kept = [k for k, (per_step, _) in before.items() if not per_step]
    assert all(after[k][1] is not before[k][1] for k in stepped), [k for k in stepped if after[k][1] is before[k][1]]
    assert all(after[k][1] is before[k][1] for k in kept), [k for k in kept if after[k][1] is not before[k][1]]
    drop_caches(model)
    assert held_tensors(model) == []
    out4 = run()
    torch.cuda.synchronize()
    assert torch.isfinite(out1.float()).all()
    assert torch.equal(out1, out2) and torch.equal(out1, out3) and torch.equal(out1, out4)
    return stepped, kept


@pytest.mark.parametrize("layout", [False, True], ids=["text", "layout"])
def test_mmdit_caches(dev, layout):
    from opendwm_amd.blocks import STORE
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    case = _mmdit_case(layout=layout)
    m = DiTCrossviewTemporalConditionModel(**case.cfg)
    m.load_state_dict(case.sd)
    m = m.to(dev).to(bf16).eval()
    di = to_dev(case.inp, dev)
    sample, timestep = di.pop("sample"), di.pop("timestep")
    stepped, kept = _check_caches(m, lambda: m(sample, timestep, **di)[0][0])
    # the packed weights are per step; the cropped position table and the index sinusoids are not
    assert any(name.endswith("attn") for name, _ in stepped) and ("pos_embed", ("pos", bf16)) in kept
    assert any(name == "" and tag[0] == "sinusoid" for name, tag in kept)
    if layout:
        cit = di["condition_image_tensor"]
        feats = m.adapter_cache_of(cit)
        assert feats is not None and ("", "adapter") in stepped
        STORE.drop(m, "adapter")
        assert m.adapter_cache_of(cit) is None
        assert any(t is m.transformer_blocks[0].attn.packed()["wqkv"] for t in held_tensors(m))      # (the other entries stay)
        m.install_adapter_cache(cit, feats)
        assert m.adapter_cache_of(cit) is feats and m.adapter_cache_of(cit.clone()) is None          # this very tensor only
        assert m.refill_adapter_cache(cit) and m.adapter_cache_of(cit) is feats                     # recomputed INTO the held tensors
        STORE.bump(keep_shadows=True)
        assert m.adapter_cache_of(cit) is None and not m.refill_adapter_cache(cit)                   # the weights may have changed


def test_unet_caches(dev):
    from oracle import unet_oracle as U
    from tests.test_unet_train_gpu import _unet_model
    cfg, sd = _unet_case(dev)[:2]
    m = _unet_model(cfg, sd, dev).to(bf16).eval()
    di = to_dev(U.make_unet_inputs(cfg, 2, 2, 3, 8, 16, text_len=10), dev)
    sample, timesteps = di.pop("sample"), di.pop("timesteps")
    stepped, kept = _check_caches(m, lambda: m(sample, timesteps, **di)[0][0])
    assert ("", "text") in stepped and ("", "scratch") in kept and any(tag == "emb" for _, tag in stepped)


def test_vae_caches(dev, small_vae):  # noqa: F811
    vae, _ = small_vae
    x = (torch.rand(2, 3, 48, 80, generator=torch.Generator().manual_seed(4)) * 2 - 1).to(dev)

    def run():
        z = vae.encode(x).latent_dist.mode()
        return vae.decode(z, return_dict=False)[0]
    stepped, kept = _check_caches(vae, run)
    assert not stepped and any(tag[0] == "packed" for _, tag in kept) and any(tag[0] == "scratch" for _, tag in kept)


def test_cogvideox_caches(dev):
    from oracle import cogvideox_vae_oracle as CV
    cfg = cogvideox_cfg()
    m = _cogvideox_model(cfg, _bf_sd(CV.make_state_dict(cfg, 0)), dev)
    x = torch.randn(1, 3, 5, 32, 48, generator=torch.Generator().manual_seed(3)).to(dev)

    def run():
        z = m.encode(x).latent_dist.mode()
        return m.decode(z, return_dict=False)[0]
    stepped, kept = _check_caches(m, run)
    assert not stepped and any(tag[0] == "packed" for _, tag in kept) and any(tag[0] == "scratch" for _, tag in kept)


@pytest.mark.parametrize("kind", KINDS)
def test_graph_trainer_leaves_nothing_held(dev, kind):
    """DESIGN §25's invariant: after the capture nothing the model holds points into the capture's pool (it holds nothing at all),
    and the compute copies the replay reads are the store's own"""
    from opendwm_amd.blocks import STORE
    m, tr, _ = _run(kind, dev, True, steps=1, deterministic=True)
    warm = tr.graph_warmup
    assert tr.graph_captures == 0 and held_tensors(m)                   # the eager warm-up steps do keep their caches
    m, tr, _ = _run(kind, dev, True, steps=warm + 1, deterministic=True)
    assert tr.graph_captures == 1 and tr.graph_replays == 1
    assert held_tensors(tr.model) == []
    shadows = tr._graph_shadows()
    assert any(s is not None for s in shadows)
    assert all(s is None or s is STORE.shadow_of(p) for s, p in zip(shadows, tr.model.parameters()))
    assert all(a is b for a, b in zip(shadows, tr._g_shadows))
