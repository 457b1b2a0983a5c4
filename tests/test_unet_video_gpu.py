"""GPU leg (`-m gpu`): the video modes of the SD 2.1 denoise loop - pipeline.UNetDenoiser with reference frames, diffusion
forcing, the whole-step HIP graph and drivers.AutoregressiveDriver over it - and the kernels under them
(dwm_cfg_multistep_grouped*, dwm_cfg_ddim_step_masked).

The reference loops (inference_pipeline, ctsd.py:1439-1654, restated over oracle.unet_oracle.unet_forward) are written here.
One model and one shape serve every model test: `_small_unet_cfg()` of tests/test_unet_gpu.py, B = 1, T = 3, V = 2, latents
16 x 24, 10 text tokens, 3 steps, guidance 3; every oracle loop is computed once per session and shared.

Why the parity tests run on the fp32 accuracy path: at this shape the oracle's generated frames move by 3.3e-2 when one
reference frame is injected and by only 9.2e-3 when the reference's timestep is not zeroed, so the bf16 loop bound (3e-2)
sees neither mistake; TOL_F32 = 1e-3 lies 9x below the smaller effect.  The bf16 route is checked structurally (what the
model is fed at every step) and against the same loop bound as tests/test_unet_gpu.py."""
import pytest
import torch

from tests.common import rel_err, to_dev
from tests.test_fp32_gpu import TOL_F32
from tests.test_unet_gpu import _log, _small_unet_cfg      # _log: the suite's parity log

pytestmark = pytest.mark.gpu
bf16, f32 = torch.bfloat16, torch.float32
TOL_BF16_LOOP = 3e-2                      # tests/test_unet_gpu.py: test_unet_denoise_loop_vs_oracle
B, T, V, H, W, TEXT = 1, 3, 2, 16, 24, 10
STEPS, GUIDANCE, TOTAL = 3, 3.0, 5
SEED = 11                                 # the host generator of the driver test; its first draw starts every single-window case
AR_CFG = dict(inference_steps=STEPS, sequence_length_per_iteration=T, reference_frame_count=1,
              autoregression_data_exception_for_take_sequence=["crossview_attention_mask"])


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.fail("the gpu-marked tests need a HIP device (torch.cuda.is_available() is False)")
    from opendwm_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------------ kernels
def _multistep_case(dev, pred_dtype, group_elems, seed):
    g = torch.Generator().manual_seed(seed)
    G = 2 * 3 * 2                                                         # (sample, frame, view)
    n = G * group_elems
    pred = torch.randn(2 * n, generator=g).to(pred_dtype).to(dev)
    lat, prev = torch.randn(n, generator=g).to(dev), torch.randn(n, generator=g).to(dev)
    coef = (torch.rand(G, 5, generator=g) * 2 - 1).to(dev)                # every row different
    flags = torch.zeros(2, 3, 2, dtype=torch.int32)
    flags[:, 0] = 1                                                       # frame 0 of both samples
    return pred, lat, prev, coef.contiguous(), flags.flatten().to(dev), n, G


def _multistep_fp64(pred, lat, prev, coef, group_elems, guidance):
    n = lat.numel()
    u, c = pred[:n].double(), pred[n:].double()
    k = coef.double().repeat_interleave(group_elems, 0)
    x0 = k[:, 0] * lat.double() + k[:, 1] * (u + guidance * (c - u))
    return k[:, 2] * lat.double() + k[:, 3] * x0 + k[:, 4] * prev.double(), x0


@pytest.mark.parametrize("group_elems", [240, 1536])
@pytest.mark.parametrize("pred_dtype", [bf16, f32])
def test_cfg_multistep_grouped(dev, pred_dtype, group_elems):
    """dwm_cfg_multistep_grouped / _f32: 12 groups with a coefficient row each, group borders inside a workgroup's 1024 elements
    (240) and several workgroups per group (1536); the groups of frame 0 flagged.  latents / x0_prev of the unflagged groups
    against the formula in fp64 (rtol 1e-5, atol 1e-6: six fp32 operations); model_in of the unflagged groups = the produced
    latents in the compute dtype, bit for bit, in both CFG halves; model_in of the flagged groups = the sentinel it held."""
    from opendwm_amd import ops
    pred, lat, prev, coef, flags, n, G = _multistep_case(dev, pred_dtype, group_elems, 3)
    want_x, want_x0 = _multistep_fp64(pred, lat, prev, coef, group_elems, GUIDANCE)
    model_in = torch.full((2, n), -7.0, dtype=pred_dtype, device=dev)
    got_x, got_prev = lat.clone(), prev.clone()
    ops.cfg_multistep_grouped(pred, got_x, got_prev, GUIDANCE, coef, group_elems, keep_model_in=flags, model_in=model_in)
    keep = flags.bool().repeat_interleave(group_elems)
    upd = ~keep
    ex = (got_x.double() - want_x).abs()[upd].max().item()
    e0 = (got_prev.double() - want_x0).abs()[upd].max().item()
    _log("cfg_multistep_grouped", dtype=str(pred_dtype), group_elems=group_elems, max_abs_latents=ex, max_abs_x0=e0)
    torch.testing.assert_close(got_x.double()[upd], want_x[upd], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(got_prev.double()[upd], want_x0[upd], rtol=1e-5, atol=1e-6)
    for half in model_in:
        assert torch.equal(half[upd], got_x.to(pred_dtype)[upd])
        assert torch.equal(half[keep], torch.full_like(half[keep], -7.0))
    # one broadcast row, no flags: the scalar kernel's result
    row = coef[5:6].contiguous()
    a_x, a_prev, a_in = lat.clone(), prev.clone(), torch.empty((2, n), dtype=pred_dtype, device=dev)
    b_x, b_prev, b_in = lat.clone(), prev.clone(), torch.empty((2, n), dtype=pred_dtype, device=dev)
    ops.cfg_multistep_grouped(pred, a_x, a_prev, GUIDANCE, row, group_elems, model_in=a_in)
    ops.cfg_multistep(pred, b_x, b_prev, GUIDANCE, *row[0].tolist(), model_in=b_in)
    torch.testing.assert_close(a_x, b_x, rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(a_prev, b_prev, rtol=1e-5, atol=1e-6)
    assert torch.equal(a_in[0], a_x.to(pred_dtype)) and torch.equal(a_in[1], a_in[0])


def test_cfg_multistep_grouped_rejects_bad_groups(dev):
    from opendwm_amd import _lib, ops
    pred, lat, prev, coef, flags, n, G = _multistep_case(dev, bf16, 240, 4)
    for ge in (242, 6, 0, 7 * 240):                   # no multiple of 4 / does not divide n
        with pytest.raises(RuntimeError):
            ops.cfg_multistep_grouped(pred, lat.clone(), prev.clone(), GUIDANCE, coef, ge)
    # the entry point itself refuses them too, before any launch
    lib = _lib.load()
    for name in ("dwm_cfg_multistep_grouped", "dwm_cfg_multistep_grouped_f32"):
        fn = getattr(lib, name)
        ok = (pred.data_ptr(), lat.data_ptr(), prev.data_ptr(), None, n, GUIDANCE, coef.data_ptr())
        assert fn(*ok, G, None, 242, None) != 0 and fn(*ok, 480, None, 6, None) != 0
        assert fn(*ok, 5, None, 240, None) != 0      # neither one row nor one per group


@pytest.mark.parametrize("pred_dtype", [bf16, f32])
def test_cfg_ddim_step_flags(dev, pred_dtype):
    """ops.cfg_ddim_step(skip=...): flagged groups keep latents, x0_out and model_in bit for bit; the others equal the call
    without flags bit for bit (the arithmetic of the existing entry point is untouched)"""
    from opendwm_amd import ops
    from opendwm_amd.schedulers import DDIMScheduler
    ge = 240
    pred, lat, _, _, flags, n, G = _multistep_case(dev, pred_dtype, ge, 5)
    sch = DDIMScheduler()
    sch.set_timesteps(12)
    coef = sch.coefficients(sch.timesteps.to(dev)[:G]).contiguous()                       # a timestep per group
    kw = dict(guidance=GUIDANCE)
    plain_x, plain_x0, plain_in = lat.clone(), torch.empty(n, device=dev), torch.empty(2, n, dtype=bf16, device=dev)
    ops.cfg_ddim_step(pred, plain_x, coef, ge, 2, x0_out=plain_x0, model_in=plain_in, **kw)
    x, x0 = lat.clone(), torch.full((n,), 5.0, device=dev)
    model_in = torch.full((2, n), -7.0, dtype=bf16, device=dev)
    ops.cfg_ddim_step(pred, x, coef, ge, 2, x0_out=x0, model_in=model_in, skip=flags, **kw)
    keep = flags.bool().repeat_interleave(ge)
    assert keep.sum().item() == 4 * ge
    assert torch.equal(x[keep], lat[keep]) and torch.equal(x0[keep], torch.full_like(x0[keep], 5.0))
    assert torch.equal(model_in[:, keep], torch.full_like(model_in[:, keep], -7.0))
    assert torch.equal(x[~keep], plain_x[~keep]) and torch.equal(x0[~keep], plain_x0[~keep])
    assert torch.equal(model_in[:, ~keep], plain_in[:, ~keep])
    with pytest.raises(RuntimeError):
        ops.cfg_ddim_step(pred, x, coef, ge, 2, skip=flags[:-1].contiguous(), **kw)


# ------------------------------------------------------------------------------------------------ the shared world
class _World:
    """weights, conditions of the 5-frame sequence, start latents and every oracle loop (computed on first use, kept)"""

    def __init__(self):
        from oracle import unet_oracle as U
        from opendwm_amd.schedulers import DDIMScheduler
        self.U = U
        self.cfg = _small_unet_cfg()
        self.sd = {k: v.to(bf16).float() for k, v in U.make_unet_state_dict(self.cfg, 0).items()}
        inp = U.make_unet_inputs(self.cfg, 2 * B, TOTAL, V, H, W, text_len=TEXT)
        inp.pop("sample")
        inp.pop("timesteps")
        self.cond5 = {k: (v.to(bf16).float() if v.is_floating_point() and k != "added_time_ids" else v) for k, v in inp.items()}
        self.cond = self.clip(0, T)
        self.shape = (B, T, V, self.cfg["in_channels"], H, W)
        self.lat = torch.randn(self.shape, generator=torch.Generator().manual_seed(SEED))   # = the driver's first draw
        self.image_latents = torch.randn(self.shape, generator=torch.Generator().manual_seed(SEED + 1))
        self.sch = DDIMScheduler()
        self.sch.set_timesteps(STEPS)
        self._memo, self._models = {}, {}

    def clip(self, a, b):
        from oracle import drivers_oracle as DO
        exc = AR_CFG["autoregression_data_exception_for_take_sequence"]
        return {k: (v if k in exc else DO.take_sequence_clip(v, a, b)) for k, v in self.cond5.items()}

    def memo(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def guided(self, x_in, timesteps, cond):
        out = self.U.unet_forward(self.sd, self.cfg, torch.cat([x_in, x_in]), torch.cat([timesteps, timesteps]).float(), **cond)
        u, c = out.chunk(2)
        return u + GUIDANCE * (c - u)

    def window(self, scheduler, lat, cond, image_latents=None, r=0):
        """full-sequence inference_pipeline (ctsd.py:1496-1575, 1623-1627), reference frames included; never changes its inputs"""
        U = self.U
        ts, sig = U.dpm_solver_tables(STEPS)
        x, prev = lat.float().clone(), torch.zeros_like(lat, dtype=f32)
        for i in range(STEPS):
            t = (ts[i] if scheduler == "dpm" else self.sch.timesteps[i]).expand(B, T, V).clone()
            x_in = x
            if image_latents is not None:                                               # :1514-1526
                x_in = torch.cat([image_latents[:, :r], x[:, r:]], 1)
                t[:, :r] = 0
            o = self.guided(x_in, t, cond)
            if scheduler == "dpm":
                kx, ko, A, Bc, Cc = U.dpm_solver_coefficients(sig, i, "v_prediction")
                x0 = kx * x + ko * o
                x, prev = A * x + Bc * x0 + Cc * prev, x0
            else:
                from oracle import scheduler_oracle as SO
                x, _ = SO.ddim_step(self.sch.alphas_cumprod.cpu(), self.sch.final_alpha_cumprod.cpu(), 1000, STEPS, "v_prediction", o,
                                    self.sch.timesteps[i].expand(B, T, V), x)
        return x if image_latents is None else torch.cat([image_latents[:, :r], x[:, r:]], 1)

    def forcing(self, lat, cond, start, stop, take_time, spi, record=None):
        """diffusion-forcing inference_pipeline (ctsd.py:1498-1507, 1554-1572) with the tensor-timestep DDIM step"""
        from oracle import scheduler_oracle as SO
        x = lat.float().clone()
        for i in range(start, stop):
            idx = torch.tensor([min(i - take_time * spi, max(0, i - j * spi)) for j in range(T)])
            t = self.sch.timesteps[idx].view(1, T, 1).repeat(B, 1, V)
            o = self.guided(x, t, cond)
            staging, _ = SO.ddim_step(self.sch.alphas_cumprod.cpu(), self.sch.final_alpha_cumprod.cpu(), 1000, STEPS, "v_prediction", o, t, x)
            in_range = torch.tensor([i - j * spi >= 0 for j in range(T)]).view(1, T, 1, 1, 1, 1)
            x = torch.where(in_range, staging, x)
            if record is not None:
                record.append(x.clone())
        return x

    def oracle(self, scheduler, ref):
        return self.memo(("window", scheduler, ref), lambda: self.window(
            scheduler, self.lat, self.cond, self.image_latents if ref else None, 1 if ref else 0))

    def model(self, dev, dtype):
        if dtype not in self._models:
            from opendwm_amd.unet import UNetCrossviewTemporalConditionModel
            m = UNetCrossviewTemporalConditionModel(**self.cfg)
            m.load_state_dict(self.sd)
            if dtype == f32:
                m = m.to(dev).eval()
                m.compute_dtype = f32
            else:
                m = m.to(dev).to(bf16).eval()
            self._models[dtype] = m
        return self._models[dtype]

    def denoiser(self, dev, dtype, scheduler, model=None):
        from opendwm_amd.pipeline import UNetDenoiser
        from opendwm_amd.schedulers import DDIMScheduler
        return UNetDenoiser(model if model is not None else self.model(dev, dtype), GUIDANCE, STEPS,
                            scheduler=None if scheduler == "dpm" else DDIMScheduler())

    def bf16_reference_window(self, dev, scheduler):
        """(result, error against the oracle) of the bf16 run with one reference frame: case 2, shared with the driver's bound"""
        def run():
            out = self.denoiser(dev, bf16, scheduler).run(self.lat.to(dev), to_dev(self.cond, dev), image_latents=self.image_latents.to(dev),
                                                           reference_frame_count=1)
            return out, rel_err(out[:, 1:], self.oracle(scheduler, True)[:, 1:])
        return self.memo(("bf16 window", scheduler), run)


@pytest.fixture(scope="module")
def world():
    return _World()


# ------------------------------------------------------------------------------------------------ reference frames
@pytest.mark.parametrize("scheduler", ["dpm", "ddim"])
def test_reference_frames_fp32_vs_oracle(dev, world, scheduler):
    """r = 1 clean reference frame (ctsd.py:1514-1526, 1623-1627) on the fp32 accuracy path, DPM-Solver++ through
    dwm_cfg_multistep_grouped_f32 and DDIM through the flag of dwm_cfg_ddim_step_masked, against this file's oracle loop at
    TOL_F32.  The oracle without the reference differs by more than 1e-2 in the generated frames, so the case cannot pass with
    the reference ignored."""
    want, without = world.oracle(scheduler, True), world.oracle(scheduler, False)
    effect = rel_err(want[:, 1:], without[:, 1:])
    il = world.image_latents.to(dev)
    got = world.denoiser(dev, f32, scheduler).run(world.lat.to(dev), to_dev(world.cond, dev), image_latents=il, reference_frame_count=1)
    e = rel_err(got[:, 1:], want[:, 1:])
    _log("unet_reference_frames_fp32", scheduler=scheduler, rel=e, reference_effect=effect)
    assert effect > 1e-2
    assert got.dtype == f32 and torch.equal(got[:, :1], il[:, :1])
    assert e < TOL_F32, e


class _Recorder:
    """the model, remembering what it was fed"""

    def __init__(self, model):
        self.model, self.calls = model, []

    def __call__(self, sample, timesteps, **kw):
        self.calls.append((sample.clone(), timesteps.clone()))
        return self.model(sample, timesteps, **kw)


@pytest.mark.parametrize("scheduler", ["dpm", "ddim"])
def test_reference_frames_bf16_model_input(dev, world, scheduler):
    """the bf16 route, structurally: at every step both CFG halves of frame 0 of the model input are image_latents in bf16 and
    their timesteps are 0, the other frames carry the scheduler's timestep; the result is within the bf16 loop bound"""
    il = world.image_latents.to(dev)
    rec = _Recorder(world.model(dev, bf16))
    got = world.denoiser(dev, bf16, scheduler, model=rec).run(world.lat.to(dev), to_dev(world.cond, dev), image_latents=il,
                                                             reference_frame_count=1)
    assert len(rec.calls) == STEPS
    step_ts = world.U.dpm_solver_tables(STEPS)[0] if scheduler == "dpm" else world.sch.timesteps
    for i, (sample, ts) in enumerate(rec.calls):
        assert sample.dtype == bf16 and sample.shape[0] == 2 * B
        for half in sample.chunk(2):
            assert torch.equal(half[:, :1], il[:, :1].to(bf16))
        assert torch.count_nonzero(ts[:, :1]) == 0 and torch.all(ts[:, 1:] == float(step_ts[i]))
        if i > 0:                                                     # the generated frames do move
            assert not torch.equal(sample[:, 1:], rec.calls[i - 1][0][:, 1:])
    assert torch.equal(got[:, :1], il[:, :1])
    ref_run, e_shared = world.bf16_reference_window(dev, scheduler)
    assert torch.equal(got, ref_run)                                 # the recorder changes nothing
    _log("unet_reference_frames_bf16", scheduler=scheduler, rel=e_shared)
    assert e_shared < TOL_BF16_LOOP, e_shared


# ------------------------------------------------------------------------------------------------ diffusion forcing
SPI = STEPS // T


def _forcing_calls():
    """(start, stop, take_time) of the queue warm-up and of the first steady-state call (ctsd.py:1710-1727, 1752-1760)"""
    return (0, STEPS - SPI, 0), (STEPS - SPI, STEPS, 0)


def test_diffusion_forcing_fp32_vs_oracle(dev, world):
    """queue warm-up (start 0, stop steps - spi) then one steady-state call (take_time 0) with DDIMScheduler on the fp32 path:
    per-frame timestep indices, tensor-timestep DDIM step, frames outside the schedule range untouched - against this file's
    loop at TOL_F32; after step 0 the frames 1.. equal their start values bit for bit"""
    warm, steady = _forcing_calls()
    trace = []
    w1 = world.memo("forcing warm", lambda: world.forcing(world.lat, world.cond, *warm, SPI, record=trace))
    w2 = world.memo("forcing steady", lambda: world.forcing(w1, world.cond, *steady, SPI))
    den = world.denoiser(dev, f32, "ddim")
    cond, lat = to_dev(world.cond, dev), world.lat.to(dev)
    den.prepare(lat, cond, diffusion_forcing=True, take_time=0)
    den.step(0)
    assert torch.equal(den.latents[:, 1:], lat[:, 1:]) and not torch.equal(den.latents[:, :1], lat[:, :1])
    if trace:
        assert torch.equal(trace[0][:, 1:], world.lat[:, 1:])
    g1 = den.run(lat, cond, start=warm[0], stop=warm[1], diffusion_forcing=True, take_time=warm[2])
    e1 = rel_err(g1, w1)
    g2 = den.run(lat, cond, start=steady[0], stop=steady[1], image_latents=g1, diffusion_forcing=True, take_time=steady[2])
    e2 = rel_err(g2, w2)
    _log("unet_diffusion_forcing_fp32", rel_warmup=e1, rel_steady=e2)
    assert torch.equal(g1[:, 2:], lat[:, 2:])                        # slot 2 enters the schedule at step 2 * spi
    assert e1 < TOL_F32 and e2 < TOL_F32, (e1, e2)


def test_dpm_solver_refuses_diffusion_forcing(dev, world):
    den = world.denoiser(dev, bf16, "dpm")
    cond, lat = to_dev(world.cond, dev), world.lat.to(dev)
    with pytest.raises(ValueError, match="multistep"):
        den.run(lat, cond, diffusion_forcing=True)
    with pytest.raises(ValueError, match="multistep"):
        den.run(lat, cond, start=1)


# ------------------------------------------------------------------------------------------------ graph
@pytest.mark.parametrize("scheduler", ["dpm", "ddim"])
def test_graph_replay_equals_eager_reference_frames(dev, world, scheduler):
    """enable_graph(): case 2 on bf16 - one capture per prepare(), replayed with the step's timesteps / coefficient rows / flags
    from static buffers; the final latents equal the eager ones bit for bit, and a second prepare() captures again"""
    eager, _ = world.bf16_reference_window(dev, scheduler)
    il = world.image_latents.to(dev)
    den = world.denoiser(dev, bf16, scheduler).enable_graph()
    cond, lat = to_dev(world.cond, dev), world.lat.to(dev)
    got = den.run(lat, cond, image_latents=il, reference_frame_count=1)
    first = den._graph
    assert first is not None and torch.equal(got, eager)
    again = den.run(lat, cond, image_latents=il, reference_frame_count=1)
    assert den._graph is not None and den._graph is not first and torch.equal(again, eager)


def test_graph_replay_equals_eager_diffusion_forcing(dev, world):
    """enable_graph(): case 3 (fp32 path, DDIM, warm-up then a steady-state call) equals the eager run bit for bit"""
    warm, steady = _forcing_calls()
    cond, lat = to_dev(world.cond, dev), world.lat.to(dev)
    out = []
    for graph in (False, True):
        den = world.denoiser(dev, f32, "ddim").enable_graph(graph)
        g1 = den.run(lat, cond, start=warm[0], stop=warm[1], diffusion_forcing=True, take_time=warm[2])
        out.append((g1, den.run(lat, cond, start=steady[0], stop=steady[1], image_latents=g1, diffusion_forcing=True,
                                take_time=steady[2])))
        assert (den._graph is not None) == graph
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


# ------------------------------------------------------------------------------------------------ driver
def test_autoregressive_driver_over_unet_denoiser(dev, world):
    """drivers.AutoregressiveDriver(UNetDenoiser): 5 frames in windows of 3 with 1 reference frame = two chained windows (the
    second starts from the last frame of the first), against oracle.drivers_oracle.autoregressive over this file's window loop.
    fp32 path: TOL_F32.  bf16: the chain error is bounded by twice the single-window bf16 error of the reference-frame case
    (the carried frame is one more bf16 pass), capped at 5e-2.
    Measured on an MI355X (profiles/unet_video_gpu_parity.log): fp32 chain 1.6e-5; bf16 chain 1.99e-2 against a single-window
    error of 2.01e-2, i.e. a bound of 4.0e-2 - the second window's error does not add to the first's, because only its one
    carried frame comes from the first window."""
    from oracle import drivers_oracle as DO
    from opendwm_amd.drivers import AutoregressiveDriver

    def window(latent_shape, cond, image_latents, r, start, stop, take_time, noise):
        if image_latents is None and torch.equal(noise, world.lat):
            x = world.oracle("dpm", False)                              # the first window is the plain single-window case
        else:
            x = world.window("dpm", noise, cond, image_latents, r)
        return {"latents": x, "images": x.flatten(0, 2)}
    want = world.memo("driver", lambda: DO.autoregressive(window, world.shape, world.cond5, TOTAL, AR_CFG, False,
                                                          torch.Generator().manual_seed(SEED)))
    assert want["images"].shape[0] == TOTAL * V
    got = {}
    for dtype in (f32, bf16):
        drv = AutoregressiveDriver(world.denoiser(dev, dtype, "dpm"), AR_CFG, generator=torch.Generator().manual_seed(SEED))
        assert [(w.reference, w.carry) for w in drv.plan(T, TOTAL, False)] == [(0, "tail"), (1, "none")]
        got[dtype] = drv.run(world.shape, to_dev(world.cond5, dev), TOTAL, dev)["images"]
        assert got[dtype].shape == want["images"].shape
    e32, e16 = rel_err(got[f32], want["images"]), rel_err(got[bf16], want["images"])
    _, single = world.bf16_reference_window(dev, "dpm")
    bound = min(2 * single, 5e-2)
    _log("unet_autoregressive_driver", rel_fp32=e32, rel_bf16_chain=e16, rel_bf16_single_window=single, bf16_bound=bound)
    assert e32 < TOL_F32, e32
    assert e16 < bound, (e16, bound)
