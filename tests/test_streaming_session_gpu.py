"""The persistent streaming session (pipeline.CTSDDenoiser.begin_stream / advance_stream / stream_window under
drivers.StreamingDriver(persistent=True)) against the driver it leaves untouched and against the restated reference FIFO over the fp32
oracle model.  Eager and graph runs of this project are bit-identical and the slide is a copy, so the session must reproduce the
existing driver bit for bit where no kernel choice depends on the row count (the text-only model); with cached layout residuals the
adapter runs on 2B V instead of 2B T V images and the bound is the existing driver's own distance from the oracle.

Measured on an MI355X (the `streaming_session_*` lines of the suite's GPU parity log, written by the logger of
tests/test_drivers_gpu.py): see the figures in DESIGN.md s20."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import ctsd_oracle as O          # noqa: E402
from oracle import drivers_oracle as DO      # noqa: E402
from tests.common import rel_err, small_config, small_inputs, to_dev   # noqa: E402
from tests.test_drivers_gpu import _log      # noqa: E402  (one parity log for the driver tests)

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
TOL_CHAIN = 3e-2                 # tests/test_drivers_gpu.py: the bf16 bound of a chain of windows
G, STEPS, TOTAL = 4.0, 6, 5
SHAPE = (1, 3, 3, 16, 8, 12)     # T = 3: two steps per frame
NON_TEMPORAL = ["disable_crossview", "disable_temporal", "crossview_attention_mask"]
ADAPTER = dict(in_channels=6, channels=[128, 128, 128], is_downblocks=[True, False, False], num_res_blocks=2, downscale_factor=8,
               use_zero_convs=True)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def _model(cfg, dev):
    from opendwm_amd.dit import DiTCrossviewTemporalConditionModel
    sd = {k: (v.to(bf16).float() if v.is_floating_point() else v) for k, v in O.make_state_dict(cfg, 0).items()}
    m = DiTCrossviewTemporalConditionModel(**cfg)
    m.load_state_dict(sd)
    return m.to(dev).to(bf16).eval(), sd


@pytest.fixture(scope="module")
def text_model(dev, small_cfg):
    return _model(small_cfg, dev)[0]


@pytest.fixture(scope="module")
def layout(dev):
    """(model, state dict, config) of the text + layout model: pointwise temporal attention and an ImageAdapter as wide as the model"""
    cfg = small_config(temporal_attention_type="pointwise", condition_image_adapter_config=ADAPTER)
    return _model(cfg, dev) + (cfg,)


def conditions(cfg, frames, layout_images=False):
    inp = small_inputs(cfg, 3, T=frames)
    cond = {k: v for k, v in inp.items() if k not in ("sample", "timestep")}
    if layout_images:
        g = torch.Generator().manual_seed(77)
        cond["condition_image_tensor"] = torch.rand(2, frames, 3, 6, 64, 96, generator=g).to(bf16).float()
    return cond


def drv_cfg(T=SHAPE[1]):
    return dict(inference_steps=STEPS, sequence_length_per_iteration=T, autoregression_data_exception_for_take_sequence=NON_TEMPORAL,
                autoregression_condition_exception_for_take_sequence=NON_TEMPORAL)


def fifo(model, cond, dev, persistent, graph=False, seed=22, den=None, shape=SHAPE, total=TOTAL):
    from opendwm_amd.drivers import StreamingDriver
    from opendwm_amd.pipeline import CTSDDenoiser
    if den is None:
        den = CTSDDenoiser(model, guidance_scale=G, inference_steps=STEPS).enable_graph(graph)
    drv = StreamingDriver(den, drv_cfg(shape[1]), generator=torch.Generator().manual_seed(seed), persistent=persistent)
    out = drv.fifo(shape, to_dev(cond, dev), total, dev)
    torch.cuda.synchronize()
    return out, den


# ---------------------------------------------------------------- 1, 2: the text-only model
def test_text_model_is_bit_identical_and_captures_once(dev, small_cfg, text_model):
    cond = conditions(small_cfg, TOTAL)
    base, _ = fifo(text_model, cond, dev, persistent=False)
    eager, den_e = fifo(text_model, cond, dev, persistent=True)
    assert eager.shape == base.shape and eager.shape[0] == TOTAL * SHAPE[2]
    assert torch.equal(eager, base)
    assert den_e.graph_captures == 0 and den_e.slide_launches == TOTAL - SHAPE[1]
    graph, den = fifo(text_model, cond, dev, persistent=True, graph=True)
    assert torch.equal(graph, eager)
    assert den.graph_captures == 1                                # warm-up + steady frames + flush: one capture
    # a second stream of the same shape: the buffers and the graph are reused - and rewritten, not just kept
    ptr = den.latents.data_ptr()
    again, _ = fifo(text_model, cond, dev, persistent=True, den=den)
    assert den.graph_captures == 1 and den.latents.data_ptr() == ptr and torch.equal(again, graph)
    other, _ = fifo(text_model, conditions(small_cfg, TOTAL + 1), dev, persistent=True, den=den, seed=23, total=TOTAL + 1)
    want, _ = fifo(text_model, conditions(small_cfg, TOTAL + 1), dev, persistent=False, seed=23, total=TOTAL + 1)
    assert den.graph_captures == 1 and torch.equal(other, want)
    # another queue length: rebuilt
    short = (1, 2) + SHAPE[2:]
    cond2 = conditions(small_cfg, 4)
    got2, _ = fifo(text_model, cond2, dev, persistent=True, den=den, shape=short, total=4)
    want2, _ = fifo(text_model, cond2, dev, persistent=False, shape=short, total=4)
    assert den.graph_captures == 2 and torch.equal(got2, want2)


# ---------------------------------------------------------------- 3: cached layout residuals advance by one frame
def test_layout_model_runs_the_adapter_on_the_new_frame_only(dev, layout, monkeypatch):
    m, sd, cfg = layout
    assert m.cache_adapter_residuals and m.compute_dtype == bf16
    cond = conditions(cfg, TOTAL, layout_images=True)
    B, T, V = SHAPE[:3]
    counts = []
    real = m.condition_image_adapter.run

    def counting(x, *a, **kw):
        counts.append(x[..., 0, 0, 0].numel())
        return real(x, *a, **kw)
    monkeypatch.setattr(m.condition_image_adapter, "run", counting)
    base, _ = fifo(m, cond, dev, persistent=False)
    base_counts, counts[:] = list(counts), []
    pers, _ = fifo(m, cond, dev, persistent=True)
    pers_counts, counts[:] = list(counts), []
    graph, den = fifo(m, cond, dev, persistent=True, graph=True)
    graph_counts = list(counts)
    # the existing driver hands the model a new condition tensor for every frame: 2B T V images each time
    assert base_counts[:1 + TOTAL - T] == [2 * B * T * V] * (1 + TOTAL - T) and set(base_counts) == {2 * B * T * V}
    assert pers_counts == [2 * B * T * V] + [2 * B * V] * (TOTAL - T)
    assert graph_counts == pers_counts and den.graph_captures == 1
    assert torch.equal(graph, pers)

    def window(latent_shape, conditions_, latents, start, stop, take_time):
        lat = O.denoise(sd, cfg, latents, conditions_, STEPS, G, stop=stop, start=start, image_latents=latents,
                        diffusion_forcing=True, take_time=take_time)
        return lat, (lat[:, take_time].flatten(0, 1) if stop >= STEPS else None)
    want = DO.Streaming(window, drv_cfg(), torch.Generator().manual_seed(22)).fifo(SHAPE, cond, TOTAL)
    e_base, e_pers = rel_err(base, want), rel_err(pers, want)
    same = bool(torch.equal(pers, base))
    print(f"streaming_session_layout rel_existing={e_base:.3e} rel_persistent={e_pers:.3e} bit_equal={same}")
    _log("streaming_session_layout", frames=TOTAL, rel_existing=e_base, rel_persistent=e_pers, bit_equal=same,
         persistent_vs_existing=rel_err(pers, base))
    assert pers.shape == want.shape
    assert e_pers < TOL_CHAIN
    assert e_pers <= 1.1 * e_base


def test_session_keeps_its_residuals_when_another_driver_shares_the_model(dev, layout, monkeypatch):
    """The model's residual cache has one slot.  An existing driver that streams on the same model between the session's frames takes
    the slot over with every frame (and re-captures its graph, which empties the allocator's cache): the session holds its residuals
    itself - the captured graph and the slide tables keep their addresses - and puts them back, so it still runs the adapter on
    the new frame only and emits the frames it emits alone."""
    from opendwm_amd.drivers import StreamingDriver, take_sequence_clip
    from opendwm_amd.pipeline import CTSDDenoiser
    m, _, cfg = layout
    B, T, V = SHAPE[:3]
    frames = T + 3
    cond = to_dev(conditions(cfg, frames, layout_images=True), dev)
    counts = []
    real = m.condition_image_adapter.run
    monkeypatch.setattr(m.condition_image_adapter, "run", lambda x, *a, **kw: (counts.append(x[..., 0, 0, 0].numel()), real(x, *a, **kw))[1])

    def driver(persistent, graph):
        den = CTSDDenoiser(m, guidance_scale=G, inference_steps=STEPS).enable_graph(graph)
        d = StreamingDriver(den, drv_cfg(), generator=torch.Generator().manual_seed(13), persistent=persistent)
        d.reset_streaming(SHAPE, dev)
        d.out = []
        return d

    def send(d, i):
        n = len(counts)
        d.send_frame_condition({k: (v if k in NON_TEMPORAL else take_sequence_clip(v, i, i + 1)) for k, v in cond.items()})
        f = d.receive_frame()
        if f is not None:
            d.out.append(f)
        return counts[n:]
    alone = driver(True, False)
    for i in range(frames):
        send(alone, i)
    ses, other = driver(True, True), driver(False, True)
    mine = []
    for i in range(frames):
        send(other, i)
        mine += send(ses, i)
    torch.cuda.synchronize()
    feats = ses.denoiser._session.cache_feats
    assert feats is not None and m.adapter_cache_of(ses.denoiser.conditions["condition_image_tensor"]) is feats
    assert mine == [2 * B * T * V] + [2 * B * V] * (frames - T)
    assert ses.denoiser.graph_captures == 1 and other.denoiser.graph_captures == 1 + frames - T
    assert len(ses.out) == 1 + frames - T and torch.equal(torch.cat(ses.out), torch.cat(alone.out))


# ---------------------------------------------------------------- 4: replaced and queued conditions
def test_condition_buffers_follow_the_existing_driver(dev, small_cfg, text_model):
    """three steady frames with a different disable_temporal / crossview mask per frame (replaced: they are exceptions) and the
    132-byte added_time_ids rows (queued on the narrow path): the session's buffers equal the existing driver's conditions, and
    so do the frames"""
    from opendwm_amd.drivers import StreamingDriver, take_sequence_clip
    from opendwm_amd.pipeline import CTSDDenoiser
    T, frames = SHAPE[1], SHAPE[1] + 3
    cond = to_dev(conditions(small_cfg, frames), dev, float_dtype=None)
    cond = {k: (v.to(bf16) if v.is_floating_point() and k != "added_time_ids" else v) for k, v in cond.items()}
    assert cond["added_time_ids"].dtype == torch.float32 and cond["added_time_ids"][0, 0].numel() * 4 == 132
    ring = cond["crossview_attention_mask"]

    def frame(i):
        f = {k: (v if k in NON_TEMPORAL else take_sequence_clip(v, i, i + 1)) for k, v in cond.items()}
        f["disable_temporal"] = torch.tensor([False, i % 2 == 1], device=dev)
        f["crossview_attention_mask"] = ring if i % 2 == 0 else torch.ones_like(ring)
        return f
    drivers = []
    for persistent in (False, True):
        den = CTSDDenoiser(text_model, guidance_scale=G, inference_steps=STEPS)
        d = StreamingDriver(den, drv_cfg(), generator=torch.Generator().manual_seed(5), persistent=persistent)
        d.reset_streaming(SHAPE, dev)
        d.out = []
        for i in range(frames):
            d.send_frame_condition(frame(i))
            f = d.receive_frame()
            if f is not None:
                d.out.append(f)
        drivers.append(d)
    ref, ses = drivers
    torch.cuda.synchronize()
    assert ses.conditions is ses.denoiser.conditions and set(ses.conditions) == set(ref.conditions)
    for k, v in ref.conditions.items():
        assert ses.conditions[k].shape == v.shape and ses.conditions[k].dtype == v.dtype, k
        assert torch.equal(ses.conditions[k], v), k
    assert torch.equal(ses.conditions["disable_temporal"], torch.tensor([False, (frames - 1) % 2 == 1], device=dev))
    assert ses.conditions["added_time_ids"].shape[1] == T
    assert len(ses.out) == len(ref.out) == 4 and torch.equal(torch.cat(ses.out), torch.cat(ref.out))


# ---------------------------------------------------------------- 5: the other modes
@pytest.mark.parametrize("mode", ["fp32", "no_cache"])
def test_other_modes_equal_the_existing_driver(dev, layout, mode):
    """compute_dtype = float32, and cache_adapter_residuals = False: no cached residuals - the adapter is recomputed from the slid
    condition_image_tensor by every forward, as today"""
    m, _, cfg = layout
    cond = conditions(cfg, TOTAL, layout_images=True)
    try:
        if mode == "fp32":
            m.compute_dtype = torch.float32
        else:
            m.cache_adapter_residuals = False
        base, _ = fifo(m, cond, dev, persistent=False)
        pers, den = fifo(m, cond, dev, persistent=True)
        assert den.model_in.dtype == (torch.float32 if mode == "fp32" else bf16)
    finally:
        m.compute_dtype, m.cache_adapter_residuals = bf16, True
    e = rel_err(pers, base)
    _log("streaming_session_mode", mode=mode, persistent_vs_existing=e, bit_equal=bool(torch.equal(pers, base)))
    assert torch.equal(pers, base) or e < 1e-5


def test_sharded_denoiser_has_no_stream_session(dev, text_model):
    from opendwm_amd.pipeline import CTSDDenoiser
    den = CTSDDenoiser(text_model, guidance_scale=G, inference_steps=STEPS)
    den.frame_shard = object()            # what CTSDDenoiser(frame_group=...) holds; no process group, no collective
    with pytest.raises(ValueError, match="frame_group / cfg_group"):
        den.begin_stream(torch.zeros(SHAPE, device=dev), {})


# ---------------------------------------------------------------- 6: nothing grows
def test_steady_state_allocates_nothing_that_stays(dev, layout):
    """the first steady frame builds the slide tables and the staging rows of the cached residuals, once; from then on the
    allocated bytes after a frame do not grow (the existing driver re-allocates its queue per frame and cannot promise that)"""
    from opendwm_amd.drivers import StreamingDriver, take_sequence_clip
    from opendwm_amd.pipeline import CTSDDenoiser
    m, _, cfg = layout
    frames = SHAPE[1] + 6
    cond = to_dev(conditions(cfg, frames, layout_images=True), dev)
    den = CTSDDenoiser(m, guidance_scale=G, inference_steps=STEPS).enable_graph()
    d = StreamingDriver(den, drv_cfg(), generator=torch.Generator().manual_seed(9), persistent=True)
    d.reset_streaming(SHAPE, dev)
    used = []
    for i in range(frames):
        d.send_frame_condition({k: (v if k in NON_TEMPORAL else take_sequence_clip(v, i, i + 1)) for k, v in cond.items()})
        f = d.receive_frame()
        del f
        torch.cuda.synchronize()
        used.append(torch.cuda.memory_allocated(dev))
    steady = used[SHAPE[1]:]                                      # after steady frames 1 .. 6
    assert len(steady) == 6 and den.slide_launches == 6 and den.graph_captures == 1
    assert all(u <= steady[0] for u in steady[1:]), steady
