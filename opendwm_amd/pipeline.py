"""Denoise-loop harness: the hot loop of CrossviewTemporalSD.inference_pipeline
(src/dwm/pipelines/ctsd.py:1496-1575) for the full-sequence / classifier-free-guidance /
FlowMatch-Euler case (examples/ctsd_35_6views_video_generation.json:34-35), driving
opendwm_amd.dit.DiTCrossviewTemporalConditionModel.  It exists so the path can be timed
and parity-checked without diffusers / the dataset stack; with diffusers installed the
unchanged ctsd.py drives the same model class.
"""
from __future__ import annotations

import contextlib
from typing import Dict, Optional

import torch

from . import ops

bf16 = torch.bfloat16


class FlowMatchEulerSchedule:
    """Sigma table of diffusers FlowMatchEulerDiscreteScheduler (0.31.0) without dynamic
    shifting: set_timesteps(n) -> sigmas[n+1] (trailing 0), timesteps = sigmas[:-1]*1000;
    step: x += (sigma[i+1] - sigma[i]) * v   (fp32)."""

    def __init__(self, num_train_timesteps: int = 1000, shift: float = 3.0):
        self.num_train_timesteps, self.shift = num_train_timesteps, shift
        ts = torch.linspace(1, num_train_timesteps, num_train_timesteps).flip(0) / num_train_timesteps
        ts = shift * ts / (1 + (shift - 1) * ts)
        self._sigma_max, self._sigma_min = ts[0].item(), ts[-1].item()
        self.sigmas = None
        self.timesteps = None

    def set_timesteps(self, num_inference_steps: int):
        n = self.num_train_timesteps
        t = torch.linspace(self._sigma_max * n, self._sigma_min * n, num_inference_steps)
        sig = t / n
        sig = self.shift * sig / (1 + (self.shift - 1) * sig)
        self.sigmas = torch.cat([sig, torch.zeros(1)]).float()
        self.timesteps = self.sigmas[:-1] * n
        return self


class CTSDDenoiser:
    """latents [B,T,V,C,H,W] fp32 on device; conditions = the CFG-doubled model kwargs
    ([2B,...], unconditional half first, as get_conditions builds them, ctsd.py:416-453).

    Modes of inference_pipeline (ctsd.py:1439-1575):
      * full-sequence denoising (default);
      * reference frames: `image_latents` + `reference_frame_count` — the first frames are fed as clean
        latents at timestep 0 every step and restored at the end (:1514-1526, :1623-1627);
      * diffusion forcing: per-frame timestep indices min(i - take_time*spi, max(0, i - j*spi)), per-frame
        scheduler step, frames outside the schedule range left untouched (:1498-1507, :1554-1572)."""

    def __init__(self, model, guidance_scale: float = 4.0, inference_steps: int = 40, shift: float = 3.0,
                 cfg_group=None, frame_group=None, frame_exchange: str = "rows"):
        """frame_group: a torch.distributed process group whose R ranks hold T/R frames each of ONE sample
        (opendwm_amd.sharding: one all-to-all before and after every temporal block; everything else is local).  Every
        rank passes the same full latents / conditions to prepare() and gets the full result() back.
        frame_exchange: what the temporal blocks of the frame shards exchange (sharding.FrameShard): "rows" = token rows (rowwise /
        pointwise temporal attention, token rows % R == 0), "heads" = attention heads around the attention alone (full / rowwise
        temporal attention, heads % R == 0), "auto" = rows where they serve, else heads.

        cfg_group: a torch.distributed process group of size 2 -> classifier-free-guidance split: the
        two halves of the CFG batch are independent inside the model, so rank 0 of the group runs the unconditional
        half and rank 1 the conditional half of ONE sample, the halves of the prediction are exchanged with one
        all-gather per step (2.2 MB at config 3; RCCL over xGMI) and both ranks apply the same guidance + scheduler
        update, keeping bit-identical latents.  Halves the per-sample latency; throughput scaling stays with replicas."""
        self.model = model
        self.cfg_group = cfg_group
        self.cfg_rank = 0
        self.frame_shard = None
        if frame_group is not None:
            from .sharding import FrameShard
            self.frame_shard = FrameShard(frame_group, temporal_exchange=frame_exchange)
        elif frame_exchange != "rows":
            raise ValueError("frame_exchange chooses the exchange of a frame_group: pass one")
        if cfg_group is not None:
            import torch.distributed as dist
            if dist.get_world_size(cfg_group) != 2:
                raise ValueError("the CFG split needs a process group of exactly two ranks")
            self.cfg_rank = dist.get_rank(cfg_group)
        self.guidance_scale = guidance_scale
        self.schedule = FlowMatchEulerSchedule(shift=shift).set_timesteps(inference_steps)
        self.inference_steps = inference_steps
        self._ts_dev = None
        self.use_graph = False
        self._graph = None
        self._side = None
        self.graph_captures = 0          # whole-step graphs captured so far (a stream session captures one and keeps it)
        self.slide_launches = 0          # dwm_fifo_slide_multi launches of the stream sessions so far
        self._session = None

    def prepare(self, latents: torch.Tensor, conditions: Dict[str, torch.Tensor],
                image_latents: Optional[torch.Tensor] = None, reference_frame_count: int = 0,
                diffusion_forcing: bool = False, take_time: int = 0, clear_reference_frame_count: int = 0):
        dev = latents.device
        self._graph = None                                             # buffers below are re-created: capture again
        self._session = None                                           # ... and a stream session has lost its buffers
        self.diffusion_forcing = diffusion_forcing
        self.take_time = take_time
        if diffusion_forcing and image_latents is not None:
            latents = image_latents                                   # ctsd.py:1470-1471
            image_latents = None
        B, T = latents.shape[:2]
        self.total_frames, self.t0 = T, 0
        self.ref = reference_frame_count if image_latents is not None else 0
        if diffusion_forcing:
            if self.inference_steps % (T - clear_reference_frame_count) != 0:
                raise ValueError("inference_steps must be a multiple of the frame count in diffusion-forcing mode")
            self.spi = self.inference_steps // (T - clear_reference_frame_count)
        if hasattr(self.model, "frame_shard"):
            self.model.frame_shard = self.frame_shard
        elif self.frame_shard is not None:
            raise ValueError("this model has no frame-sharded forward")
        if self.frame_shard is not None:                               # keep this rank's frames of everything per-frame
            if self.use_graph:
                raise NotImplementedError("frame sharding is not captured into a HIP graph")
            t0, t1 = self.frame_shard.frame_range(T)
            self.t0 = t0
            latents = latents[:, t0:t1]
            if image_latents is not None:
                image_latents = image_latents[:, t0:t1]
            self.ref = min(max(self.ref - t0, 0), t1 - t0)
            conditions = {k: (v[:, t0:t1] if torch.is_tensor(v) and k not in self.NO_FRAME_AXIS and v.dim() >= 2 and v.shape[1] == T
                              else v) for k, v in conditions.items()}
        self.latents = latents.to(torch.float32).contiguous().clone()
        self.image_latents = None if image_latents is None else image_latents.to(torch.float32).to(dev)
        # model input / conditions / prediction in the model's compute dtype: bf16, or fp32 for the accuracy path
        # (`model.compute_dtype = torch.float32`)
        self.cd = cd = getattr(self.model, "compute_dtype", bf16)
        self.model_in = torch.empty((2 * B, *latents.shape[1:]), dtype=cd, device=dev)
        self._refresh_model_in()
        self.conditions = {k: (v.to(cd) if torch.is_tensor(v) and v.is_floating_point() and k != "added_time_ids" else v)
                           for k, v in conditions.items()}
        if self.cfg_group is not None:                                 # this rank's half of every CFG-doubled condition
            r = self.cfg_rank
            self.conditions = {k: (v[r * B:(r + 1) * B].contiguous() if torch.is_tensor(v) and v.dim() >= 1 and v.shape[0] == 2 * B else v)
                               for k, v in self.conditions.items()}
            self._pred_full = torch.empty((2 * B, *latents.shape[1:]), dtype=cd, device=dev)
        self._ts_dev = self.schedule.timesteps.to(dev)
        self._sig_dev = self.schedule.sigmas.to(dev)
        return self

    # conditions without a frame axis at dim 1 (crossview_temporal_dit.py:372-391)
    NO_FRAME_AXIS = ("disable_crossview", "disable_temporal", "crossview_attention_mask", "crossview_attention_index")

    def _refresh_model_in(self):
        B = self.latents.shape[0]
        lat16 = self.latents if self.cd == torch.float32 else ops.cast_bf16(self.latents)
        self.model_in[:B].copy_(lat16)
        self.model_in[B:].copy_(lat16)
        self._inject_reference()

    def _inject_reference(self):
        if self.ref > 0:                                              # clean reference frames, every step
            B = self.latents.shape[0]
            r16 = self.image_latents[:, :self.ref].to(self.cd)
            self.model_in[:B, :self.ref].copy_(r16)
            self.model_in[B:, :self.ref].copy_(r16)

    def _step_inputs(self, i: int):
        """(timesteps [2B,T,V] device fp32, sigma step: host float or device fp32 [B,T,V]) of step i"""
        B, T, V = self.latents.shape[:3]
        if self.diffusion_forcing:
            j = self.t0 + torch.arange(T)                              # this rank's frames of the sample
            idx = torch.minimum(torch.full((T,), i - self.take_time * self.spi), torch.clamp(i - j * self.spi, min=0))
            idx = idx.to(self._ts_dev.device)
            ts = self._ts_dev[idx].view(1, T, 1).expand(2 * B, T, V)
            in_range = (i - j * self.spi >= 0).to(self._sig_dev.device)
            dsig = torch.where(in_range, self._sig_dev[idx + 1] - self._sig_dev[idx], torch.zeros((), device=idx.device))
            return ts, dsig.view(1, T, 1).expand(B, T, V).contiguous().float()
        ts = self._ts_dev[i].expand(2 * B, T, V)
        if self.ref > 0:
            ts = ts.clone()
            ts[:, :self.ref] = 0
        return ts, float(self.schedule.sigmas[i + 1] - self.schedule.sigmas[i])

    def _step_body(self, ts: torch.Tensor, dsig):
        if self.cfg_group is None:
            out, _, _ = self.model(self.model_in, ts, **self.conditions)
            pred = out[0]
        else:
            import torch.distributed as dist
            B, r = self.latents.shape[0], self.cfg_rank
            out, _, _ = self.model(self.model_in[r * B:(r + 1) * B], ts[r * B:(r + 1) * B], **self.conditions)
            dist.all_gather(list(self._pred_full.split(B)), out[0].contiguous(), group=self.cfg_group)
            pred = self._pred_full
        if torch.is_tensor(dsig):
            ops.cfg_euler_step(pred, self.latents, self.guidance_scale, dsig, model_in=self.model_in,
                               group_elems=self.latents[0, 0, 0].numel())
        else:
            ops.cfg_euler_step(pred, self.latents, self.guidance_scale, dsig, model_in=self.model_in)
        self._inject_reference()

    def step(self, i: int):
        """One denoise step = model forward at the CFG batch + guidance combine + scheduler update."""
        ts, dsig = self._step_inputs(i)
        if self.use_graph:
            self._graph_step(ts, dsig)
        else:
            self._step_body(ts, dsig)

    # ---- whole-step HIP graph: the ~600 launches of one step (model forward, CFG combine, scheduler
    # update, reference re-injection) are captured once per prepare() and replayed; per-step inputs (timesteps, sigma
    # steps) live in static device buffers that are refreshed before each replay.
    def enable_graph(self, on: bool = True):
        self.use_graph = on
        self._graph = None
        return self

    def _graph_step(self, ts: torch.Tensor, dsig):
        B, T, V = self.latents.shape[:3]
        if not torch.is_tensor(dsig):
            dsig = torch.full((B, T, V), dsig, dtype=torch.float32, device=self.latents.device)
        if self._graph is None:
            self._g_ts = ts.to(torch.float32).contiguous().clone()
            self._g_dsig = dsig.clone()
            # one eager pass on a side stream fills every cache the forward keeps (packed weights, adapter residuals,
            # scratch buffers) and warms the allocator; the state it touched is restored before the capture
            keep_lat, keep_in = self.latents.clone(), self.model_in.clone()
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.latents.device)
            side = self._side
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._step_body(self._g_ts, self._g_dsig)
            torch.cuda.current_stream().wait_stream(side)
            self.latents.copy_(keep_lat)
            self.model_in.copy_(keep_in)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._step_body(self._g_ts, self._g_dsig)
            self.graph_captures = getattr(self, "graph_captures", 0) + 1
        self._g_ts.copy_(ts)
        self._g_dsig.copy_(dsig)
        self._graph.replay()

    def result(self) -> torch.Tensor:
        out = self.latents
        if self.ref > 0:                                              # ctsd.py:1623-1627
            out = torch.cat([self.image_latents[:, :self.ref], self.latents[:, self.ref:]], 1)
        if self.frame_shard is not None:
            out = self.frame_shard.gather_frames(out, 1)               # every rank returns the whole sample
        return out

    # ---- persistent stream session (frame-in / frame-out generation, drivers.StreamingDriver(persistent=True)): what run() rebuilds
    # for every incoming frame - the latents, the model input, every condition, the cached adapter residuals, the captured graph -
    # is built ONCE and lives in static device buffers.  A new frame is one dwm_fifo_slide_multi launch over all of them (every
    # buffer moves by one frame along the time axis and takes the new frame's noise / conditions / residuals at its end) plus the
    # adapter on the 2B V images of that frame; the whole-step graph keeps replaying, since no address changed.  The steps of the
    # warm-up, the steady state and the flush differ in the timestep / sigma-step tables alone, which _graph_step refreshes anyway.
    def begin_stream(self, latents: torch.Tensor, conditions: Dict[str, torch.Tensor], replace_keys=()):
        """Start a session from the latents [B,T,V,C,H,W] (the queue's noise) and the conditions of its T frames: what
        prepare(latents, conditions, image_latents=latents, diffusion_forcing=True) sets up, in buffers that survive the frames.
        Conditions with a frame axis at dim 1 will slide; those of NO_FRAME_AXIS, those named in `replace_keys` (the driver's
        autoregression_condition_exception_for_take_sequence) and tensors of at most one dimension are replaced wholesale by
        advance_stream.  A session of the same shapes is already open: its buffers, its slide tables and its graph are reused."""
        if self.frame_shard is not None or self.cfg_group is not None:
            raise ValueError("a stream session keeps one sample on one GPU: frame_group / cfg_group sessions are not built")
        from types import SimpleNamespace
        dev = latents.device
        B, T = latents.shape[:2]
        if self.inference_steps % T != 0:
            raise ValueError("inference_steps must be a multiple of the frame count in diffusion-forcing mode")
        cd = getattr(self.model, "compute_dtype", bf16)
        replaced = set(self.NO_FRAME_AXIS) | set(replace_keys)

        def converted(k, v):
            return v.to(cd) if torch.is_tensor(v) and v.is_floating_point() and k != "added_time_ids" else v
        slide_keys = tuple(k for k, v in conditions.items()
                           if torch.is_tensor(v) and k not in replaced and v.dim() >= 2 and v.shape[1] == T)
        sig = (str(dev), tuple(latents.shape), cd, slide_keys,
               tuple((k, tuple(v.shape), cd if v.is_floating_point() and k != "added_time_ids" else v.dtype) if torch.is_tensor(v)
                     else (k, None, repr(v)) for k, v in conditions.items()))
        s = self._session
        if s is not None and s.sig == sig:
            self.latents.copy_(latents)
            for k, v in conditions.items():
                if torch.is_tensor(v):
                    self.conditions[k].copy_(v)
            # the cached adapter residuals belong to the condition images just overwritten: recompute them where they are (the
            # graph and the slide tables hold their addresses)
            self._hold_adapter_cache(s)
            if s.cache_feats is not None and not self.model.refill_adapter_cache(self.conditions["condition_image_tensor"]):
                self._graph, s.plan, s.cache_feats, s.cache_fresh = None, None, None, None
        else:
            self._graph = None
            self.latents = latents.to(torch.float32).contiguous().clone()
            self.cd = cd
            self.model_in = torch.empty((2 * B, *latents.shape[1:]), dtype=cd, device=dev)
            self.conditions = {k: (converted(k, v).contiguous().clone() if torch.is_tensor(v) else v) for k, v in conditions.items()}
            s = self._session = SimpleNamespace(
                sig=sig, slide_keys=slide_keys, plan=None, cache_feats=None, cache_fresh=None, cache_step=None,
                noise=torch.empty((B, 1, *latents.shape[2:]), dtype=torch.float32, device=dev),
                staging={k: torch.empty_like(self.conditions[k][:, :1]) for k in slide_keys},
                snapshot=torch.empty_like(self.latents))
            self._ts_dev = self.schedule.timesteps.to(dev)
            self._sig_dev = self.schedule.sigmas.to(dev)
        self.diffusion_forcing, self.take_time = True, 0
        self.total_frames, self.t0, self.ref, self.image_latents = T, 0, 0, None
        self.spi = self.inference_steps // T
        if hasattr(self.model, "frame_shard"):
            self.model.frame_shard = None
        self._refresh_model_in()
        return self

    def _stream(self):
        if self._session is None:
            raise RuntimeError("no stream session: begin_stream() first (prepare() / run() end one)")
        return self._session

    def _hold_adapter_cache(self, s):
        """The model's cached adapter residuals of the session's condition images slide with the images, and the captured graph
        reads them at their addresses.  The model's cache has one slot, which any forward with another condition tensor (another
        driver on the same model) takes over - the residuals it drops would be freed under the graph.  So the session adopts the
        list once the model has computed it, keeps it alive, and puts it back into the model's slot before every use."""
        cit = self.conditions.get("condition_image_tensor")
        if not torch.is_tensor(cit) or "condition_image_tensor" not in s.slide_keys or not hasattr(self.model, "adapter_cache_of"):
            return
        from .blocks import STORE
        if s.cache_feats is None:
            feats = self.model.adapter_cache_of(cit)
            if feats is not None:
                s.cache_feats, s.cache_step, s.plan = feats, STORE.step, None           # (the plan is rebuilt with them in it)
        elif s.cache_step != STORE.step:                                                # other weights: other residuals, other graph
            s.cache_feats, s.cache_fresh, s.plan, self._graph = None, None, None, None
        elif self.model.adapter_cache_of(cit) is not s.cache_feats:
            self.model.install_adapter_cache(cit, s.cache_feats)

    def _plan_stream_slide(self, s):
        B, T = self.latents.shape[:2]
        pairs = [(self.latents, s.noise, B, T), (self.model_in, s.noise, 2 * B, T)]      # both CFG halves take the one noise frame
        pairs += [(self.conditions[k], s.staging[k], self.conditions[k].shape[0], T) for k in s.slide_keys]
        s.cache_fresh = None
        if s.cache_feats is not None:                                                   # per level [2B T V N, D] = [2B][T][V N D]
            s.cache_fresh = [torch.empty((f.shape[0] // T, f.shape[1]), dtype=f.dtype, device=f.device) for f in s.cache_feats]
            pairs += [(f, n, self.conditions["condition_image_tensor"].shape[0], T) for f, n in zip(s.cache_feats, s.cache_fresh)]
        s.plan = ops.FifoSlide(pairs)

    def advance_stream(self, noise_frame: torch.Tensor, frame_conditions: Dict[str, torch.Tensor]):
        """One frame in: the queue drops its oldest frame and takes `noise_frame` [B,1,V,C,H,W] (fp32, host or device) and the
        one-frame conditions at its end.  Small copies into static staging buffers, the adapter on the new frame's images if the
        model caches its residuals, ONE slide launch over every buffer, in-place copies of the replaced conditions."""
        s = self._stream()
        s.noise.copy_(noise_frame)
        for k in s.slide_keys:
            v = frame_conditions.get(k)
            if not torch.is_tensor(v) or tuple(v.shape) != tuple(s.staging[k].shape):
                raise ValueError(f"advance_stream: condition {k!r} of one frame must be a tensor {tuple(s.staging[k].shape)}")
            s.staging[k].copy_(v)
        self._hold_adapter_cache(s)
        if s.plan is None:
            self._plan_stream_slide(s)
        if s.cache_fresh is not None:
            self.model.advance_adapter_cache(s.staging["condition_image_tensor"], out=s.cache_fresh)
        s.plan.run()
        self.slide_launches += 1
        for k, v in frame_conditions.items():
            if k in s.slide_keys:
                continue
            cur = self.conditions.get(k)
            if torch.is_tensor(v) and torch.is_tensor(cur) and cur.shape == v.shape:
                cur.copy_(v)
            elif not torch.is_tensor(v) and not torch.is_tensor(cur) and k in self.conditions:
                if cur != v:
                    self.conditions[k], self._graph = v, None                           # a python value is baked into the capture
            else:
                raise ValueError(f"advance_stream: condition {k!r} is new or changed its shape: begin a new stream")
        return self

    def stream_window(self, start: int, stop: int, take_time: int = 0) -> torch.Tensor:
        """Steps start .. stop - 1 on the session's queue, as run(..., start=, stop=, take_time=) on it; returns a COPY of queue
        slot `take_time` [B,1,V,C,H,W] (the frame a stream emits: the queue itself is overwritten by the next frame).  In the flush
        (take_time > 0) the slots up to take_time keep their state of before the window, as the driver's merge does."""
        s = self._stream()
        self.take_time = take_time
        if take_time > 0:
            s.snapshot.copy_(self.latents)
        self._hold_adapter_cache(s)
        for i in range(start, stop):
            self.step(i)
        self._hold_adapter_cache(s)                                   # (adopts the residuals the first forward computed)
        frame = self.latents[:, take_time:take_time + 1].clone()
        if take_time > 0:
            self.latents[:, :take_time + 1].copy_(s.snapshot[:, :take_time + 1])
            self._refresh_model_in()
        return frame

    def run(self, latents: torch.Tensor, conditions: Dict[str, torch.Tensor], stop: Optional[int] = None,
            start: int = 0, **prepare_kw):
        self.prepare(latents, conditions, **prepare_kw)
        for i in range(start, self.inference_steps if stop is None else stop):
            self.step(i)
        return self.result()


# ------------------------------------------------------------------------------------------ training
def flow_match_train_sigmas(num_train_timesteps: int = 1000, shift: float = 3.0) -> torch.Tensor:
    """sigmas[i] of the *training* FlowMatchEulerDiscreteScheduler (timesteps[i] = 1000 * sigmas[i], descending);
    ctsd.py:1255-1270 indexes it with floor(u * num_train_timesteps)."""
    s = torch.linspace(1, num_train_timesteps, num_train_timesteps).flip(0) / num_train_timesteps
    return (shift * s / (1 + (shift - 1) * s)).float()


def sample_timestep_indices(shape, generator: Optional[torch.Generator] = None, weighting_scheme: str = "logit_normal",
                            num_train_timesteps: int = 1000, logit_mean: float = 0.0, logit_std: float = 1.0) -> torch.Tensor:
    """sd3_compute_density_for_timestep_sampling + `(u * num_train_timesteps).long()` (ctsd.py:1256-1262)."""
    if weighting_scheme == "logit_normal":
        u = torch.sigmoid(torch.randn(shape, generator=generator) * logit_std + logit_mean)
    elif weighting_scheme in ("none", "uniform"):
        u = torch.rand(shape, generator=generator)
    else:
        raise NotImplementedError(weighting_scheme)
    return (u * num_train_timesteps).long().clamp_(max=num_train_timesteps - 1)


def make_input_for_prediction(noisy_input: torch.Tensor, latents: torch.Tensor, timesteps: torch.Tensor, training_config: dict,
                              common_config: dict, generator: Optional[torch.Generator] = None, reference_latent_count=None):
    """CrossviewTemporalSD.try_make_input_for_prediction (ctsd.py:619-741): the training task mixer.  Host random draws in the
    reference's order (CPU generator), tensors stay on the latents' device.

    frame_prediction_style None: nothing changes.  "diffusion_forcing": per-sample image task (temporal blocks disabled, with
    probability image_generation_ratio), otherwise the reference-frame scale / offset augmentation of the noisy input.
    "ctsd": generation vs prediction tasks - for prediction the first `reference_latent_count` frames (an int, or a
    {count: probability} dict) are shown clean (timestep 0), all of them or a random subset.
    Returns (model input, timesteps, extra conditions or None, reference_frame_indicator [B, T, V])."""
    import itertools
    dev = latents.device
    B, T, V = noisy_input.shape[:3]
    rf_scale, rf_offset = 1, 0
    if "reference_frame_scale_std" in training_config:
        rf_scale = (torch.randn(latents.shape[:2], generator=generator) * training_config["reference_frame_scale_std"] + 1) \
            .view(B, T, 1, 1, 1, 1).to(dev)
    if "reference_frame_offset_std" in training_config:
        rf_offset = (torch.randn(latents.shape[:2], generator=generator) * training_config["reference_frame_offset_std"]) \
            .view(B, T, 1, 1, 1, 1).to(dev)
    style = common_config.get("frame_prediction_style", None)
    indicator = torch.zeros(B, T, V, dtype=torch.bool, device=dev)
    if style is None:
        return noisy_input, timesteps, None, indicator
    if style == "diffusion_forcing":
        disable_temporal = torch.rand((B, 1, 1), generator=generator) < training_config.get("image_generation_ratio", 0.0)
        made = torch.where(disable_temporal.view(B, 1, 1, 1, 1, 1).to(dev), noisy_input, noisy_input * rf_scale + rf_offset)
        return made, timesteps, {"disable_temporal": disable_temporal.to(dev)}, indicator
    if style != "ctsd":
        raise ValueError("Unknown frame prediction type")
    generation = torch.rand((B, 1, 1), generator=generator) < training_config.get("generation_task_ratio", 0.0)
    disable_temporal = torch.logical_and(
        torch.rand((B, 1, 1), generator=generator) < training_config.get("image_generation_ratio", 0.0), generation)
    all_visible = torch.rand((B, 1, 1), generator=generator) < training_config.get("all_reference_visible_ratio", 0.0)
    partial = torch.rand((B, T, V), generator=generator) < training_config.get("reference_visible_rate", 1.0)
    if isinstance(reference_latent_count, int):
        count = reference_latent_count * torch.ones((B, 1, 1), dtype=torch.int32)
    elif isinstance(reference_latent_count, dict):
        counts = torch.tensor([int(i) for i in reference_latent_count.keys()], dtype=torch.int32)
        cum = torch.tensor(list(itertools.accumulate(reference_latent_count.values())))
        count = counts[torch.searchsorted(cum, torch.rand((B, 1, 1), generator=generator))]
    else:
        raise NotImplementedError("Un implemented dynamic reference frame count")
    in_count = torch.arange(T, dtype=torch.int32).view(1, T, 1).repeat(B, 1, V) < count
    indicator = torch.logical_and(torch.logical_and(torch.logical_not(generation), torch.logical_or(all_visible, partial)), in_count)
    made = torch.where(indicator.view(B, T, V, 1, 1, 1).to(dev), latents * rf_scale + rf_offset, noisy_input)
    made_timesteps = torch.where(indicator.to(timesteps.device), torch.zeros_like(timesteps), timesteps)
    return made, made_timesteps, {"disable_temporal": disable_temporal.to(dev)}, indicator


def freeze_modules(model, pattern: str):
    """training_config["freezing_pattern"] (ctsd.py:1014-1022): requires_grad_(False) on every module whose qualified name
    the regex matches (re.match: anchored at the start); returns the names"""
    import re
    pat, names = re.compile(pattern), []
    for name, module in model.named_modules():
        if pat.match(name) is not None:
            module.requires_grad_(False)
            names.append(name)
    return names


class CTSDTrainer:
    """The SD 3 branch of CrossviewTemporalSD.train_step (ctsd.py:1195-1437) on latents that are already
    VAE-encoded and conditions that are already embedded:

        idx ~ logit-normal, sigma = sigmas[idx], t = 1000 sigma           :1255-1266
        x_t = sigma * noise + (1 - sigma) * x0,  target = x0               :1267-1272
        pred = model(x_t, t, conditions);  x0_hat = pred * (-sigma) + x_t  :1355-1360
        loss = mse(x0_hat.float(), x0.float()) * coef                      :1368-1370
        loss.backward(); [clip_grad_norm_]; optimizer.step(); zero_grad    :1401-1432

    With the SD 2.1 UNet as the model the trainer takes the reference's other branch (ctsd.py:1240-1253):

        t ~ randint(0, num_train_timesteps) per sample (per frame with diffusion forcing), from the pipeline generator
        x_t = train_scheduler.add_noise(x0, noise, t)          (schedulers.DDPMScheduler, tensor timesteps)
        target = noise ("epsilon") | train_scheduler.get_velocity(x0, noise, t) ("v_prediction")
        loss = mse(model(x_t, t, conditions).float(), target.float()) * coef

    `ddp=True` wraps the model in torch DistributedDataParallel (ctsd.py:1051-1054): the block Functions of
    opendwm_amd.train hand their parameter gradients to autograd block by block, so the bucketed RCCL
    all-reduce overlaps the rest of the backward.  The buckets are fp32 by default, as the reference's DDP all-reduces them
    (ctsd.py:1051-1054), 200 MB each; `ddp_comm_dtype=torch.bfloat16` is the opt-in throughput mode (torch's
    bf16_compress_hook: 7.6 GB instead of 15.1 GB per step at 3.78 B parameters - the ring all-reduce is bound by the xGMI
    links, SURVEY.md s5 - at the price of a bf16 rounding of every averaged gradient, accumulated micro-steps included).

    training_config keys honoured as the reference does: "freezing_pattern" (regex over module names, ctsd.py:1014-1022),
    "gradient_accumulation_steps" (optimizer step every k-th call, :1401-1432; the micro-steps in between run under DDP's
    no_sync, so one all-reduce per optimizer step carries the accumulated gradient - the same sum the reference gets
    with an all-reduce per micro-step), "max_norm_for_grad_clip", "enable_grad_scaler" (torch.amp.GradScaler around our fused
    AdamW: :1040-1048, :1401-1432).  `lr_scheduler` (a callable optimizer -> scheduler, or
    a scheduler) is stepped once per train_step (:1434-1435)."""

    def __init__(self, model, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 shift: float = 3.0, num_train_timesteps: int = 1000, loss_coef: float = 1.0,
                 max_grad_norm: Optional[float] = None, weighting_scheme: str = "logit_normal", ddp: bool = False,
                 ddp_kwargs: Optional[dict] = None, common_config: Optional[dict] = None, training_config: Optional[dict] = None,
                 reference_latent_count=0, lr_scheduler=None, ddp_comm_dtype: Optional[torch.dtype] = None,
                 train_scheduler=None, optimizer_bits: int = 32, grad_conditioning: str = "torch",
                 activations: str = "recompute", activation_budget_gib: Optional[float] = None, deterministic: bool = False,
                 graph: bool = False, lora=None, ema=None):
        """common_config["frame_prediction_style"] (None | "diffusion_forcing" | "ctsd") and training_config select the
        training task mix of `make_input_for_prediction`; with "diffusion_forcing" every frame draws its own timestep
        (ctsd.py:1232-1237).  optimizer_bits: 32 = train.AdamW (fp32 moments), 8 = train.AdamW8bit (block-wise 8-bit moments: the
        reference's single-GPU recipe, docs/CtsdPipelineFaqs.md "Single GPU training").
        grad_conditioning: how an optimizing step unscales, clips and checks the gradients.  "torch" (default): GradScaler.unscale_,
        torch.nn.utils.clip_grad_norm_, GradScaler.step - three passes of torch arithmetic over every gradient.  "fused": ONE read
        (train.grad_norm_and_coef: norm, non-finite flag, coefficient) and the coefficient handed to the AdamW kernel as its
        grad_scale; the gradients are never rewritten, the loss scale is a train.LossScaler (GradScaler's dynamics and state dict),
        `last_grad_norm` / `skipped_steps` are kept for logging.  One deviation from the reference's control flow, in this mode
        only: with a clip but NO scaler a step whose gradients hold an inf / nan is skipped (with one warning) - the torch route
        clips by a nan coefficient there and writes nan into every weight.
        activations (MMDiT only): what the transformer blocks hold between forward and backward.  "recompute" (default): the block
        inputs - every block is gradient-checkpointed and its backward runs its forward again.  "keep": every joint block and every
        cross-view / temporal block keeps its activations (train.kept_bytes) and skips the recompute.  "config": per family, as the
        reference's switches say - joint blocks recompute iff model.gradient_checkpointing, temporal blocks iff
        temporal_gradient_checkpointing, cross-view blocks iff crossview_gradient_checkpointing.  activation_budget_gib caps the
        kept bytes of one forward: blocks are visited in forward order and one that does not fit in what is left recomputes
        (0: nothing is kept, None: no cap).  `activation_plan` reports the decisions of the last forward.
        deterministic (MMDiT and UNet): True = the gradient reductions that finish with fp32 atomics by default (bias / modulation /
        norm-weight / d(alpha) sums) run their ordered form (ops.ordered_reductions): loss, gradients, parameters and
        optimizer state of a step are then a function of the inputs and the library build only - bit-equal from run to run, between
        "keep" and "recompute", and under a one-rank DDP wrap - for 1.2 % of step time at config 4.  False (default): the atomics, as
        before.  Multi-rank all-reduce order is RCCL's and not covered.
        graph (MMDiT and UNet, one GPU): True = after `graph_warmup` (1) eager steps a train_step is host-side staging
        (the draws and the task mixer, as before), a replay of ONE HIP graph that holds forward, loss, loss scaling and backward, and
        an optimizer step that is queued without a host read (`dwm_adamw_multi_dev` / `dwm_adamw8_multi_dev`); the loss returned is
        a copy of the graph's loss buffer.  The clip coefficient and the non-finite flag stay on the device; the host reads them one
        step late, so `last_grad_norm` and `skipped_steps` lag by one step (`graph_sync()` brings them up to date).
        `graph_captures` / `graph_replays` count.  The graph is captured again when the keys, shapes or dtypes of the inputs change
        or the parameters' compute copies were replaced (a state-dict load, `.to()`); a forward of the model outside the trainer
        needs no recapture.  ValueError with ddp=True, with a clip or a scaler under grad_conditioning="torch", and for a model
        that is not on the device.  False (default): every launch as before.
        lora (MMDiT, one GPU, eager): None (default) = full fine-tuning, every launch as before.  A dict of
        lora.LoraAdapters' keyword arguments (rank, alpha, target, generator) or a LoraAdapters built on this model = low-rank
        fine-tuning: every base parameter is out of the optimizer, the targeted weights keep requires_grad (the block Functions
        produce their dW), all others lose it (their weight-gradient GEMMs are skipped), the optimizer (`optimizer_bits`) holds the
        adapter tensors only.  A step is backward, `project_grads_()`, the configured clip / scaler / grad_conditioning on the adapter
        gradients, the optimizer step, `merge_()`; before every step the trainer re-merges if `lora.merged()` is False.
        `save_checkpoint` / `load_checkpoint` write and read `<output>/lora/<step>.pth` in place of the base checkpoint.
        ValueError with ddp=True and with graph=True, NotImplementedError with the SD 2.1 UNet.
        ema (MMDiT and UNet, every mode above): None (default) = no average, every launch as before.  A dict of
        train.EMA's keyword arguments (decay, min_decay, update_after_step, use_ema_warmup, inv_gamma, power: diffusers' EMAModel)
        or a train.EMA = an exponential moving average of the optimized parameters (with `lora` the adapter tensors), one fp32
        shadow each, moved inside the AdamW kernels of every optimizing call (so once per gradient-accumulation cycle; in graph mode
        without a host read: the decay rides in the optimizer's hyper row).  A step skipped for non-finite gradients advances
        `ema.optimization_step` and leaves the shadows alone.  `with trainer.ema_weights():` evaluates with the averaged weights
        (an in-place exchange: no third copy, no graph recapture); `train_step` inside it raises RuntimeError.  `save_checkpoint`
        also writes `<output>/ema/<step>.pth`, `load_checkpoint` reads it - or, where it is absent (resuming a run that had no
        EMA), restarts the shadows from the loaded parameters with one warning."""
        from . import train as _train
        from .unet import UNetCrossviewTemporalConditionModel
        if activations not in _train.ACTIVATION_POLICIES:
            raise ValueError(f"activations: one of {_train.ACTIVATION_POLICIES}, got {activations!r}")
        if activation_budget_gib is not None and activation_budget_gib < 0:
            raise ValueError(f"activation_budget_gib: None or >= 0, got {activation_budget_gib!r}")
        self.is_unet = isinstance(model, UNetCrossviewTemporalConditionModel)
        if lora is not None:
            if ddp:
                raise ValueError("CTSDTrainer(lora=...): ddp=True is not built (the adapter gradients are made after the backward, "
                                 "outside the bucketed all-reduce); train one GPU per process")
            if graph:
                raise ValueError("CTSDTrainer(lora=...): graph=True is not built (the projection and the merge are not part of the "
                                 "captured step); leave graph off")
            if self.is_unet:
                raise NotImplementedError("CTSDTrainer(lora=...) with the SD 2.1 UNet: only the MMDiT's linear layers are adapted")
        if self.is_unet and activations != "recompute":
            raise NotImplementedError(f"activations={activations!r} with the SD 2.1 UNet: its ResNet / transformer Functions "
                                      "(train_unet) have no kept-activation form yet, only the MMDiT blocks do")
        self.activations, self.activation_budget_gib = activations, activation_budget_gib
        if not self.is_unet:
            model.activation_policy, model.activation_budget_gib = activations, activation_budget_gib
        self.deterministic = bool(deterministic)
        model.ordered_reductions = self.deterministic     # a plain attribute, like activation_policy: the training forwards read it
        if optimizer_bits not in (8, 32):
            raise ValueError(f"optimizer_bits: 8 or 32, got {optimizer_bits!r}")
        if grad_conditioning not in ("torch", "fused"):
            raise ValueError(f"grad_conditioning: 'torch' or 'fused', got {grad_conditioning!r}")
        self.grad_conditioning = grad_conditioning
        self.graph = bool(graph)
        if self.graph:
            tc = training_config or {}
            if ddp:
                raise ValueError("CTSDTrainer(graph=True): ddp=True is not captured (the bucketed all-reduce runs on RCCL's own "
                                 "streams); train one GPU per process without the wrap, or leave graph off")
            if grad_conditioning != "fused" and (tc.get("max_norm_for_grad_clip", max_grad_norm) is not None
                                                 or tc.get("enable_grad_scaler", False)):
                raise ValueError("CTSDTrainer(graph=True): a gradient clip or a grad scaler needs grad_conditioning='fused' - the "
                                 "'torch' route rewrites the gradients through host-synchronising torch calls")
            if any(not p.is_cuda for p in model.parameters()):
                raise ValueError("CTSDTrainer(graph=True): the model is not on the device (a HIP graph holds device launches only)")
        self.last_grad_norm, self.skipped_steps, self._warned_nonfinite = 0.0, 0, False
        self.model = model.train()
        self.wrapper = model
        self.common_config, self.training_config = dict(common_config or {}), dict(training_config or {})
        self.frozen_modules = freeze_modules(model, self.training_config["freezing_pattern"]) \
            if "freezing_pattern" in self.training_config else []
        self.ddp = bool(ddp)
        self.ddp_comm_dtype = ddp_comm_dtype
        if ddp:
            dev = next(model.parameters()).device
            kw = dict(device_ids=[dev.index] if dev.type == "cuda" else None, gradient_as_bucket_view=True, bucket_cap_mb=200)
            kw.update(ddp_kwargs or {})
            self.wrapper = torch.nn.parallel.DistributedDataParallel(model, **kw)
            if ddp_comm_dtype == bf16:
                from torch.distributed.algorithms.ddp_comm_hooks import default_hooks
                self.wrapper.register_comm_hook(None, default_hooks.bf16_compress_hook)
            elif ddp_comm_dtype not in (None, torch.float32):
                raise ValueError("ddp_comm_dtype: torch.bfloat16, torch.float32 or None")
        self.lora = None
        if lora is not None:
            from .lora import LoraAdapters
            self.lora = lora if isinstance(lora, LoraAdapters) else LoraAdapters(model, **lora)
            adapted = {id(p) for p in self.lora.targets()}
            if not adapted <= {id(p) for p in model.parameters()}:
                raise ValueError("CTSDTrainer(lora=...): the adapters were built on another model")
            for p in model.parameters():            # targets: dW is wanted; everything else: frozen, its wgrad GEMMs are skipped
                p.requires_grad_(id(p) in adapted)
        # every parameter, frozen ones included, as the reference builds it (ctsd.py:1089-1092): state-dict indices match
        # (with adapters: the adapter tensors, and nothing of the base model)
        opt_cls = _train.AdamW8bit if optimizer_bits == 8 else _train.AdamW
        self.optimizer = opt_cls(self._optimized(), lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.lr_scheduler = lr_scheduler(self.optimizer) if callable(lr_scheduler) else lr_scheduler
        self.ema = None
        if ema is not None:                         # over what the optimizer steps, under the names of the checkpoint it belongs to
            if not isinstance(ema, (dict, _train.EMA)):
                raise TypeError(f"CTSDTrainer(ema=...): None, a dict of train.EMA's keyword arguments or a train.EMA, got {type(ema)}")
            self.ema = ema if isinstance(ema, _train.EMA) else _train.EMA(self._named_optimized(), **ema)
        self.global_step = 0
        self.sigmas = flow_match_train_sigmas(num_train_timesteps, shift)
        self.num_train_timesteps, self.loss_coef = num_train_timesteps, loss_coef
        self.max_grad_norm = self.training_config.get("max_norm_for_grad_clip", max_grad_norm)
        # "enable_grad_scaler" (every shipped training config sets it: ctsd.py:1040-1048, :1401-1432): dynamic loss scaling with
        # torch.amp.GradScaler's defaults and state.  The compute type here is bf16, whose exponent range is fp32's, so
        # the scale changes no rounding (a power of two) - what the mode keeps is the reference's control flow: gradients are
        # unscaled before the clip, and a step whose gradients hold an inf / nan is SKIPPED and halves the scale.
        self.grad_scaler = None
        if self.training_config.get("enable_grad_scaler", False):
            # ctsd.py:1040-1048: a plain GradScaler unless torch.distributed is initialised AND the framework is fsdp (then the
            # reference takes ShardedGradScaler, which belongs to the FSDP wrap this package does not build) - a single-process run of
            # a shipped fsdp config gets the plain scaler, as in the reference
            import torch.distributed as _dist
            if (self.common_config.get("distribution_framework", "ddp") != "ddp" and _dist.is_available() and _dist.is_initialized()):
                raise NotImplementedError("enable_grad_scaler with distribution_framework != 'ddp' in a distributed run "
                                          "(ShardedGradScaler / FSDP) - SURVEY.md s2")
            dev_type = next(model.parameters()).device.type
            self.grad_scaler = _train.LossScaler() if grad_conditioning == "fused" else torch.amp.GradScaler(dev_type)
        self.weighting_scheme = weighting_scheme
        self.reference_latent_count = reference_latent_count
        self.graph_warmup, self.graph_captures, self.graph_replays = 1, 0, 0     # graph_warmup: eager steps before the first capture
        self._g_eager_done = 0
        self._graph, self._g_key, self._g_pending, self._g_grads_fresh = None, None, None, True
        # SD 2.1 branch (ctsd.py:1240-1253): the model is the UNet -> DDPM noising, epsilon / v_prediction target
        if self.is_unet and train_scheduler is None:
            from .schedulers import DDPMScheduler
            train_scheduler = DDPMScheduler(num_train_timesteps=num_train_timesteps)
        self.train_scheduler = train_scheduler

    def _optimized(self) -> list:
        """the parameters the optimizer steps and the clip reads: the model's, or with adapters theirs"""
        lora = getattr(self, "lora", None)
        return list(self.model.parameters() if lora is None else lora.parameters())

    def _named_optimized(self) -> list:
        """`_optimized()` as (state-dict key, parameter) pairs: the keys of the model's checkpoint, or with adapters of theirs"""
        lora = getattr(self, "lora", None)
        names = {id(v): k for k, v in (self.model if lora is None else lora).state_dict(keep_vars=True).items()}
        return [(names.get(id(p), str(i)), p) for i, p in enumerate(self._optimized())]

    # ---- EMA of the weights
    def _ema_exchange(self) -> None:
        """parameters <-> shadows, then everything derived from the old values goes: train.EMA.swap_ rewrites the compute copies that
        blocks.STORE refreshes in place and forgets the others, the model's caches are dropped here, and with adapters the targets'
        compute copies are merged again from the tensors that are the adapters now"""
        from .blocks import drop_caches
        self.ema.swap_()
        drop_caches(self.model)
        if getattr(self, "lora", None) is not None:
            self.lora.merge_()

    @contextlib.contextmanager
    def ema_weights(self):
        """`with trainer.ema_weights() as model:` - inside, the model (with adapters: their merged compute copies) holds the
        averaged weights; on exit, exceptions included, the trained ones are back bit for bit.  No parameter, shadow or compute
        copy changes its address, so the graph of graph mode stays valid."""
        if getattr(self, "ema", None) is None:
            raise RuntimeError("CTSDTrainer.ema_weights(): the trainer was built without ema=")
        if self.ema.swapped:
            raise RuntimeError("CTSDTrainer.ema_weights(): already inside ema_weights()")
        self._ema_exchange()
        try:
            yield self.model
        finally:
            self._ema_exchange()

    @property
    def activation_plan(self):
        """train.ActivationPlan of the last training forward: `.blocks` = (block name, "keep" | "recompute", kept bytes) per
        transformer block in forward order, `.total_bytes` their sum; None before the first forward"""
        return getattr(self.model, "activation_plan", None)

    def draw_condition_masks(self, batch_size: int, generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """the per-sample condition dropout masks of the training step in the reference's draw order (ctsd.py:1278-1301):
        keyword arguments of conditions.build_conditions (text_condition_mask is a list, for the caller's text encoders)"""
        tc, draw = self.training_config, lambda: torch.rand((batch_size,), generator=generator)
        out = {"text_condition_mask": (draw() < tc.get("text_prompt_condition_ratio", 1.0)).tolist(),
               "_3dbox_condition_mask": draw() < tc.get("3dbox_condition_ratio", 1.0),
               "hdmap_condition_mask": draw() < tc.get("hdmap_condition_ratio", 1.0),
               "action_condition_mask": draw() < tc.get("action_condition_ratio", 1.0)}
        if self.common_config.get("explicit_view_modeling", False):
            out["explicit_view_modeling_mask"] = draw() < tc.get("explicit_view_modeling_ratio", 1.0)
        return out

    def draw_training_inputs(self, latents_shape, generator: Optional[torch.Generator] = None):
        """(noise, timestep_indices, condition masks) of one training step, drawn in the reference's order (ctsd.py:1229-1301:
        noise from the pipeline generator, timestep density from the global generator, then the dropout masks); pass the
        first two to loss() / train_step() - whose task mixer continues on the same generator - and the masks to
        conditions.build_conditions."""
        B, T = latents_shape[:2]
        noise = torch.randn(tuple(latents_shape), generator=generator)
        per_frame = self.common_config.get("frame_prediction_style") == "diffusion_forcing"
        if getattr(self, "is_unet", False): # :1241-1244: integer timesteps from the SAME generator, right after the noise
            idx = torch.randint(0, self.num_train_timesteps, (B, T) if per_frame else (B,), generator=generator)
        else:
            idx = sample_timestep_indices((B, T) if per_frame else (B,), None, self.weighting_scheme, self.num_train_timesteps)
        return noise, idx, self.draw_condition_masks(B, generator)

    def make_training_pair(self, latents: torch.Tensor, generator: Optional[torch.Generator] = None,
                           timestep_indices: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None):
        """returns (noisy_latents, timesteps [B,T,V], sigmas [B,1|T,1,1,1,1], noise); host RNG like the reference (CPU
        generator).  One timestep per sample, or per (sample, frame) in the diffusion-forcing style (ctsd.py:1232-1272)."""
        B, T, V = latents.shape[:3]
        if noise is None:
            noise = torch.randn(latents.shape, generator=generator)
        if timestep_indices is None:
            per_frame = getattr(self, "common_config", {}).get("frame_prediction_style") == "diffusion_forcing"
            timestep_indices = sample_timestep_indices((B, T) if per_frame else (B,), generator, self.weighting_scheme, self.num_train_timesteps)
        sig = self.sigmas[timestep_indices.cpu()]
        F = sig.shape[1] if sig.dim() == 2 else 1
        timesteps = (sig * self.num_train_timesteps).view(B, F, 1).expand(B, T, V).contiguous()
        dev = latents.device
        sig_b = sig.view(B, F, 1, 1, 1, 1).to(dev)
        noise = noise.to(dev)
        noisy = sig_b * noise + (1.0 - sig_b) * latents.float()
        return noisy, timesteps.to(dev), sig_b, noise

    def make_unet_training_pair(self, latents: torch.Tensor, generator: Optional[torch.Generator] = None,
                                timesteps: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None):
        """SD 2.1 branch (ctsd.py:1229-1253, 1273-1276): returns (noisy_latents, timesteps [B,T,V] int64, target, noise)"""
        B, T, V = latents.shape[:3]
        if noise is None:
            noise = torch.randn(latents.shape, generator=generator)
        if timesteps is None:
            per_frame = self.common_config.get("frame_prediction_style") == "diffusion_forcing"
            timesteps = torch.randint(0, self.num_train_timesteps, (B, T) if per_frame else (B,), generator=generator)
        dev = latents.device
        noise, timesteps = noise.to(dev), timesteps.to(dev)
        sch = self.train_scheduler
        noisy = sch.add_noise(latents.float(), noise, timesteps)
        pt = sch.config.prediction_type
        if pt == "epsilon":
            target = noise
        elif pt == "v_prediction":
            target = sch.get_velocity(latents.float(), noise, timesteps)
        else:
            raise Exception("Unknown training target of the UNet.")
        while timesteps.dim() < 3:                                                     # :1273-1276
            timesteps = timesteps.unsqueeze(-1).repeat_interleave(latents.shape[timesteps.dim()], -1)
        return noisy, timesteps, target.float(), noise

    def _stage_inputs(self, latents, conditions, generator, timestep_indices, noise) -> dict:
        """the host side of `loss`: the draws, the noising and the task mixer in the reference's order and the condition casts ->
        what the model forward and the loss read (noisy, timesteps, sig - None for the UNet -, target, reference, cond)"""
        if hasattr(self, "deterministic"):      # this trainer's mode holds for its forwards (trainers may share a model)
            self.model.ordered_reductions = self.deterministic
        sig = None
        if getattr(self, "is_unet", False):
            noisy, timesteps, target, _ = self.make_unet_training_pair(latents, generator, timestep_indices, noise)
        else:
            noisy, timesteps, sig, _ = self.make_training_pair(latents, generator, timestep_indices, noise)
        noisy, timesteps, extra, reference = make_input_for_prediction(
            noisy, latents.float(), timesteps, self.training_config, self.common_config, generator, self.reference_latent_count)
        cond = {k: (v.to(bf16) if torch.is_tensor(v) and v.is_floating_point() and k != "added_time_ids" else v)
                for k, v in conditions.items()}
        if extra is not None:
            cond.update(extra)
        if sig is not None:
            target = latents.float()
        return dict(noisy=noisy, timesteps=timesteps, sig=sig, target=target, reference=reference, cond=cond)

    def _loss_of(self, s: dict) -> torch.Tensor:
        """the device side of `loss`: model forward and the loss on what `_stage_inputs` made"""
        noisy, timesteps, sig, target, reference, cond = (s[k] for k in ("noisy", "timesteps", "sig", "target", "reference", "cond"))
        if sig is None:
            pred = self.wrapper(noisy.to(bf16), timesteps, **cond)[0][0].float()           # :1358-1360: sd_pred[0] as it is
            if self.training_config.get("disable_reference_frame_loss", False):          # :1363-1367
                keep = ~reference.view(*pred.shape[:3], 1, 1, 1).to(pred.device)
                pred, target = pred * keep, target * keep
            return torch.nn.functional.mse_loss(pred, target, reduction="mean") * self.loss_coef
        if hasattr(self, "activations"):        # this trainer's policy holds for its forwards (trainers may share a model)
            self.model.activation_policy, self.model.activation_budget_gib = self.activations, self.activation_budget_gib
        pred = self.wrapper(noisy.to(bf16), timesteps, **cond)[0][0]
        x0_hat = pred.float() * (-sig) + noisy
        if self.training_config.get("disable_reference_frame_loss", False):          # ctsd.py:1363-1367
            keep = ~reference.view(*x0_hat.shape[:3], 1, 1, 1).to(x0_hat.device)
            x0_hat, target = x0_hat * keep, target * keep
        return torch.nn.functional.mse_loss(x0_hat, target, reduction="mean") * self.loss_coef

    def loss(self, latents: torch.Tensor, conditions: Dict[str, torch.Tensor], generator=None,
             timestep_indices=None, noise=None) -> torch.Tensor:
        lora = getattr(self, "lora", None)
        if lora is not None and not lora.merged():       # first forward, or the compute copies were dropped (state-dict load, .to(), bump):
            lora.merge_()                                # never a silent forward of the base model
        return self._loss_of(self._stage_inputs(latents, conditions, generator, timestep_indices, noise))

    # ---- checkpoint / resume in the reference's on-disk layout (ctsd.py:1134-1155 save_checkpoint, :988-992 and
    # :1093-1096 resume; src/dwm/distributed.py): <output>/checkpoints/<step>.pth = the model's state dict (reference
    # keys), <output>/optimizer/<step>.pth = the optimizer state in torch.optim.AdamW's format.  Rank 0 writes.
    def save_checkpoint(self, output_path: str, steps: int) -> None:
        import os
        import torch.distributed as dist
        if dist.is_initialized() and dist.get_rank() != 0:
            return
        os.makedirs(os.path.join(output_path, "optimizer"), exist_ok=True)
        lora = getattr(self, "lora", None)
        if lora is not None:                        # the base model did not change: its checkpoint is not written again
            os.makedirs(os.path.join(output_path, "lora"), exist_ok=True)
            torch.save({"state": {k: v.detach().cpu() for k, v in lora.state_dict().items()}, "rank": lora.rank, "alpha": lora.alpha,
                        "target": lora.target}, os.path.join(output_path, "lora", f"{steps}.pth"))
        else:
            os.makedirs(os.path.join(output_path, "checkpoints"), exist_ok=True)
            torch.save({k: v.detach().cpu() for k, v in self.model.state_dict().items()},
                       os.path.join(output_path, "checkpoints", f"{steps}.pth"))
        osd = self.optimizer.state_dict()
        osd["state"] = {i: {k: (v.detach().cpu() if torch.is_tensor(v) else v) for k, v in st.items()} for i, st in osd["state"].items()}
        torch.save(osd, os.path.join(output_path, "optimizer", f"{steps}.pth"))
        ema = getattr(self, "ema", None)
        if ema is not None:                         # the shadows under the checkpoint's keys, the six settings and the counter
            os.makedirs(os.path.join(output_path, "ema"), exist_ok=True)
            esd = ema.state_dict()
            esd["shadows"] = {k: v.cpu() for k, v in esd["shadows"].items()}
            torch.save(esd, os.path.join(output_path, "ema", f"{steps}.pth"))

    def load_checkpoint(self, output_path: str, resume_from: int) -> None:
        """model + optimizer state of step `resume_from`; the call counter continues there, so the gradient-accumulation
        phase `(global_step + 1) % k` lines up with the reference loop, which passes the resumed global_step
        (ctsd.py:1401-1404).  The lr_scheduler is NOT restored: the reference re-creates it on every start too."""
        import os
        self.global_step = int(resume_from)
        lora = getattr(self, "lora", None)
        if lora is not None:                        # adapters + their optimizer state; the base model is the caller's
            f = torch.load(os.path.join(output_path, "lora", f"{resume_from}.pth"), map_location="cpu", weights_only=True)
            if int(f["rank"]) != lora.rank:
                raise ValueError(f"load_checkpoint: the file holds rank {f['rank']}, the trainer's adapters rank {lora.rank}")
            lora.alpha = float(f["alpha"])
            lora.load_state_dict(f["state"])
        else:
            self.model.load_state_dict(torch.load(os.path.join(output_path, "checkpoints", f"{resume_from}.pth"),
                                                  map_location="cpu", weights_only=True))
        self.optimizer.load_state_dict(torch.load(os.path.join(output_path, "optimizer", f"{resume_from}.pth"),
                                                  map_location="cpu", weights_only=True))
        ema = getattr(self, "ema", None)
        if ema is not None:
            path = os.path.join(output_path, "ema", f"{resume_from}.pth")
            if os.path.exists(path):
                ema.load_state_dict(torch.load(path, map_location="cpu", weights_only=True))
            else:                                   # resuming a run that had no EMA: the average starts at the loaded weights
                import warnings
                warnings.warn(f"CTSDTrainer.load_checkpoint: {path} is absent - the EMA shadows restart from the loaded parameters "
                              "with optimization_step = 0")
                ema.reset_()

    def _fused_optimizer_step(self, scaler) -> None:
        """the optimizing part of train_step in grad_conditioning="fused": one read of the gradients, one host sync, the AdamW
        launch with the coefficient; nothing extra when neither a clip nor a scaler is configured"""
        ekw = self._ema_kw()
        if scaler is None and self.max_grad_norm is None:
            self.optimizer.step(**ekw)
        else:
            from .train import grad_norm_and_coef
            inv_scale = 1.0 if scaler is None else 1.0 / scaler.get_scale()
            self.last_grad_norm, coef, found_inf = grad_norm_and_coef(self._optimized(), self.max_grad_norm, inv_scale)
            if found_inf:
                self.skipped_steps += 1
                if ekw:                              # the skipped call counts, the shadows stay (train.EMA)
                    self.ema.advance()
                if scaler is None and not self._warned_nonfinite:
                    import warnings
                    warnings.warn("CTSDTrainer(grad_conditioning='fused'): non-finite gradient without a grad scaler - the optimizer "
                                  "step is skipped (further ones silently; see skipped_steps)")
                    self._warned_nonfinite = True
            else:
                self.optimizer.step(grad_scale=coef, **ekw)
            if scaler is not None:
                scaler.update(found_inf)
        self.optimizer.zero_grad()

    def _ema_kw(self) -> dict:
        """the keyword that hands the EMA to `optimizer.step`; without one the call is made as it always was"""
        ema = getattr(self, "ema", None)
        return {} if ema is None else {"ema": ema}

    # ---- whole-step HIP graph.  The captured region is `_loss_of` + backward on static copies of what `_stage_inputs`
    # makes.  A replay reads three kinds of memory only: allocations of the capture's own pool (activations, gradients, every
    # packed / transposed / padded operand - the model-level caches are dropped before the capture, so the replay rebuilds them, once
    # per replay as the eager forward does once per optimizer step), tensors this trainer holds (`_g_in`, `_g_scale`, the parameters
    # and their bf16 compute copies `_g_shadows`, which AdamW refreshes in place), and the split-K GEMM workspace of the capture
    # stream (`_g_workspace`).  A forward of the model outside the trainer therefore cannot take anything away from a replay.
    _graph_streams: dict = {}

    @staticmethod
    def _graph_signature(staged: dict) -> tuple:
        def sig(k, v):
            return (k, tuple(v.shape), v.dtype, str(v.device)) if torch.is_tensor(v) else (k, repr(v))
        flat = [sig(k, v) for k, v in staged.items() if k != "cond"]
        return tuple(flat + [sig("cond." + k, v) for k, v in sorted(staged["cond"].items())])

    def _graph_shadows(self) -> list:
        """the bf16 compute copies AdamW writes in place, as blocks.STORE holds them now (None: none, or one that is re-cast)"""
        from .blocks import STORE, refreshable
        return [STORE.shadow_of(p) if refreshable(p) else None for p in self.model.parameters()]

    def _graph_drop_model_caches(self) -> None:
        """every tensor the model keeps between forwards except the parameters' in-place compute copies: the capture re-creates what
        it needs inside its pool"""
        from .blocks import STORE, drop_caches, refreshable
        drop_caches(self.model)
        for p in self.model.parameters():           # compute copies AdamW does not write: re-cast inside the capture
            if not refreshable(p):
                STORE.forget(p)
        STORE.bump(keep_shadows=True)

    def _graph_capture(self, staged: dict, key: tuple, scaler) -> None:
        import time
        dev = staged["noisy"].device
        clone = lambda v: v.clone() if torch.is_tensor(v) else v
        self._g_in = {k: (clone(v) if k != "cond" else {ck: clone(cv) for ck, cv in v.items()}) for k, v in staged.items()}
        self._g_scale = torch.ones((), dtype=torch.float32, device=dev)
        # one capture stream per device for every trainer of the process, and with it ONE split-K workspace (ops keeps one per
        # stream, for good): made here, outside any graph's pool, and held by every trainer whose graph names it
        if dev.index not in CTSDTrainer._graph_streams:
            CTSDTrainer._graph_streams[dev.index] = torch.cuda.Stream(device=dev)
        self._g_stream = CTSDTrainer._graph_streams[dev.index]
        with torch.cuda.stream(self._g_stream):
            self._g_workspace = ops._gemm_workspace(dev)
        params = list(self.model.parameters())
        carried = None if self._g_grads_fresh else {id(p): p.grad for p in params if p.grad is not None}
        for p in params:                             # the capture's backward allocates the gradients in its pool
            p.grad = None
        self._graph = self._g_grads = self._g_acc = self._g_loss = None
        self._graph_drop_model_caches()
        t0 = time.perf_counter()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=self._g_stream, capture_error_mode="thread_local"):
            loss = self._loss_of(self._g_in)
            (loss if scaler is None else loss * self._g_scale).backward()
            self._g_loss = loss.detach()
        del loss
        self.graph_capture_seconds = time.perf_counter() - t0
        self._graph, self._g_key = graph, key
        self._g_grads = [(p, p.grad) for p in params if p.grad is not None]
        self._g_shadows = self._graph_shadows()
        self._graph_drop_model_caches()              # nothing outside the trainer keeps pointing into the pool
        self._g_acc = None
        if self.training_config.get("gradient_accumulation_steps") is not None:
            # the replay ASSIGNS the micro-step's gradients; the running sum of a cycle lives beside them and is what p.grad is
            self._g_acc = [torch.zeros_like(g) if carried is None or id(p) not in carried else carried[id(p)].clone()
                           for p, g in self._g_grads]
            self._g_grads_fresh = carried is None
        for p, _ in self._g_grads:
            p.grad = None
        self.graph_captures += 1

    def _graph_resolve(self, scaler) -> None:
        """read the (norm, coef, found) of the last optimizing step, which its kernels already acted on: wait for the copy queued
        behind them, then the host bookkeeping of the eager fused route"""
        pend, self._g_pending = self._g_pending, None
        if pend is None:
            return
        host, event = pend
        event.synchronize()
        self.last_grad_norm, _, found = host.tolist()[:3]
        if found != 0.0:
            self.skipped_steps += 1
            self.optimizer.undo_step()
            if scaler is None and not self._warned_nonfinite:
                import warnings
                warnings.warn("CTSDTrainer(grad_conditioning='fused'): non-finite gradient without a grad scaler - the optimizer "
                              "step is skipped (further ones silently; see skipped_steps)")
                self._warned_nonfinite = True
        if scaler is not None:
            scaler.update(found != 0.0)

    def graph_sync(self) -> None:
        """graph mode: bring `last_grad_norm`, `skipped_steps`, the optimizer's step counts and the loss scale up to date with the
        last train_step (waits for it); a no-op otherwise"""
        self._graph_resolve(getattr(self, "grad_scaler", None))

    def _graph_optimizer_step(self, scaler) -> None:
        from . import train_ops as _T
        from .train import _fp32_grad
        ekw = self._ema_kw()                         # the decay is host-known (the counter advances on skipped steps too)
        if scaler is None and self.max_grad_norm is None:
            self.optimizer.step(device_operands=(None, None), **ekw)
            return
        gs = [_fp32_grad(p) for p, _ in self._g_grads]
        inv_scale = 1.0 if scaler is None else 1.0 / scaler.get_scale()
        cond = _T.grad_sumsq_multi(gs, inv_scale, self.max_grad_norm, reuse_items=True)
        self.optimizer.step(device_operands=(None, cond), **ekw)
        host = torch.empty(4, dtype=torch.float32, pin_memory=True)
        host.copy_(cond, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self._g_pending = (host, event)

    def _graph_train_step(self, staged: dict, key: tuple, should_optimize: bool, scaler) -> torch.Tensor:
        if scaler is not None:                       # the loss scale of this step depends on the flag of the last one
            self._graph_resolve(scaler)
        # (a compute copy that did not exist at the capture is not read by the graph: only the ones it holds are compared)
        if self._graph is None or key != self._g_key or any(b is not None and a is not b
                                                            for a, b in zip(self._graph_shadows(), self._g_shadows)):
            self._graph_resolve(scaler)
            self._graph_capture(staged, key, scaler)
        for k, v in staged.items():
            for kk, vv in (v.items() if k == "cond" else ((k, v),)):
                dst = self._g_in["cond"][kk] if k == "cond" else self._g_in[kk]
                if torch.is_tensor(vv):
                    dst.copy_(vv, non_blocking=True)
        if scaler is not None:
            self._g_scale.fill_(scaler.get_scale())
        self._graph.replay()
        self.graph_replays += 1
        loss = self._g_loss.clone()                  # the next replay overwrites the buffer
        grads = [g for _, g in self._g_grads]
        if self._g_acc is not None:
            if self._g_grads_fresh:
                torch._foreach_copy_(self._g_acc, grads)
            else:
                torch._foreach_add_(self._g_acc, grads)
            self._g_grads_fresh = False
            grads = self._g_acc
        for (p, _), g in zip(self._g_grads, grads):  # the gradients are where autograd would have left them
            p.grad = g
        self._graph_resolve(scaler)                  # (already done with a scaler) behind the queued graph, before the scalars
        if should_optimize:
            self._graph_optimizer_step(scaler)
            self._g_grads_fresh = True
            for p, _ in self._g_grads:               # optimizer.zero_grad(): the buffers stay with the trainer
                p.grad = None
        return loss

    def train_step(self, latents: torch.Tensor, conditions: Dict[str, torch.Tensor], generator=None,
                   timestep_indices=None, noise=None, global_step: Optional[int] = None) -> torch.Tensor:
        """one call of the reference's train_step (ctsd.py:1195-1437); `global_step` defaults to the number of calls so far"""
        import contextlib
        gs = self.global_step if global_step is None else global_step
        k = self.training_config.get("gradient_accumulation_steps")
        should_optimize = k is None or (gs + 1) % k == 0                                 # :1401-1404
        scaler = getattr(self, "grad_scaler", None)
        ema = getattr(self, "ema", None)
        if ema is not None and ema.swapped:
            raise RuntimeError("CTSDTrainer.train_step: inside ema_weights() the model holds the averaged weights; training on them "
                               "would move the average into the run - leave the context first")
        if getattr(self, "graph", False) and self._g_eager_done >= self.graph_warmup:
            staged = self._stage_inputs(latents, conditions, generator, timestep_indices, noise)
            loss = self._graph_train_step(staged, self._graph_signature(staged), should_optimize, scaler)
            if self.lr_scheduler is not None:
                self.lr_scheduler.step()
            self.global_step = gs + 1
            return loss
        lora = getattr(self, "lora", None)
        sync = contextlib.nullcontext() if (should_optimize or not self.ddp) else self.wrapper.no_sync()
        with sync:
            loss = self.loss(latents, conditions, generator, timestep_indices, noise)
            (loss if scaler is None else scaler.scale(loss)).backward()                   # :1401-1404
        if lora is not None:                             # dW of the targets -> A.grad, B.grad (accumulated); dW is dropped
            lora.project_grads_()
        if should_optimize and getattr(self, "grad_conditioning", "torch") == "fused":
            self._fused_optimizer_step(scaler)
        elif should_optimize:
            if self.max_grad_norm is not None:
                if scaler is not None:
                    scaler.unscale_(self.optimizer)                                      # :1411-1413
                torch.nn.utils.clip_grad_norm_(self._optimized(), self.max_grad_norm)
            ekw = self._ema_kw()
            if scaler is not None:
                counted = ema.optimization_step if ema is not None else 0
                scaler.step(self.optimizer, **ekw)                                       # :1426-1428 (skips on inf / nan)
                if ema is not None and ema.optimization_step == counted:                 # skipped: the call counts, the shadows stay
                    ema.advance()
                scaler.update()
            else:
                self.optimizer.step(**ekw)
            self.optimizer.zero_grad()
        if should_optimize and lora is not None:         # the new A, B reach the next forward through the compute copies
            lora.merge_()
        if getattr(self, "graph", False):            # an eager warm-up step of graph mode
            self._g_eager_done += 1
            self._g_grads_fresh = should_optimize
        if self.lr_scheduler is not None:                                                # :1434-1435, every call
            self.lr_scheduler.step()
        self.global_step = gs + 1
        return loss.detach()


# ------------------------------------------------------------------------------------------ SD 2.1 (UNet) denoise loop
def dpm_solver_tables(num_inference_steps: int, num_train_timesteps: int = 1000, beta_start: float = 0.00085,
                      beta_end: float = 0.012):
    """(timesteps [n], sigmas [n+1]) of diffusers DPMSolverMultistepScheduler.set_timesteps with the SD 2.1 scheduler
    config (scaled_linear betas, 'linspace' spacing, final sigma 0)."""
    import numpy as np
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    acp = torch.cumprod(1.0 - betas, 0).numpy().astype(np.float64)
    ts = np.linspace(0, num_train_timesteps - 1, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)
    sig = np.interp(ts, np.arange(num_train_timesteps), ((1 - acp) / acp) ** 0.5)
    return torch.from_numpy(ts), torch.from_numpy(np.concatenate([sig, [0.0]]))


def dpm_solver_coefficients(sigmas: torch.Tensor, i: int, prediction_type: str):
    """(kx, ko, A, B, C) of step i for dwm_cfg_multistep: dpmsolver++ with solver_order 2, midpoint, first order on the
    first step, x' = x0 on the last (final sigma 0)."""
    import math
    n = sigmas.numel() - 1

    def a_s(s):
        a = 1.0 / math.sqrt(s * s + 1.0)
        return a, s * a
    a0, s0 = a_s(float(sigmas[i]))
    kx, ko = (1.0 / a0, -s0 / a0) if prediction_type == "epsilon" else (a0, -s0)
    if i == n - 1:
        return kx, ko, 0.0, 1.0, 0.0
    at, st = a_s(float(sigmas[i + 1]))
    lam = lambda a, s: math.log(a) - math.log(s)
    h = lam(at, st) - lam(a0, s0)
    e = math.exp(-h) - 1.0
    A = st / s0
    if i == 0:
        return kx, ko, A, -at * e, 0.0
    a1, s1 = a_s(float(sigmas[i - 1]))
    r0 = (lam(a0, s0) - lam(a1, s1)) / h
    return kx, ko, A, -at * e * (1.0 + 0.5 / r0), 0.5 * at * e / r0


def dpm_solver_coefficient_table(sigmas: torch.Tensor, prediction_type: str) -> torch.Tensor:
    """[steps, 5] fp32: row i = dpm_solver_coefficients(sigmas, i, prediction_type) - the per-step numbers of
    dwm_cfg_multistep_grouped, which reads them from device memory (UNetDenoiser copies the table there once per prepare())."""
    n = sigmas.numel() - 1
    return torch.tensor([dpm_solver_coefficients(sigmas, i, prediction_type) for i in range(n)], dtype=torch.float64).float()


def diffusion_forcing_tables(inference_steps: int, frames: int, steps_per_inference: int, take_time: int):
    """Per-frame scheduler indices of the diffusion-forcing mode (ctsd.py:1498-1507, 1565-1570) for the steps i that a call with
    this `take_time` can run, i0 <= i < i0 + inference_steps with i0 = take_time * steps_per_inference (the emitted queue slot
    walks the whole schedule over them).  Returns (i0, idx int64 [inference_steps, frames], in_range bool [same]):
        idx[i - i0, j] = min(i - take_time * spi, max(0, i - j * spi)),    in_range[i - i0, j] = i - j * spi >= 0."""
    spi = steps_per_inference
    i0 = take_time * spi
    i = torch.arange(i0, i0 + inference_steps).view(-1, 1)
    j = torch.arange(frames).view(1, -1)
    idx = torch.minimum(i - take_time * spi, torch.clamp(i - j * spi, min=0))
    return i0, idx, (i - j * spi) >= 0


class UNetDenoiser:
    """Hot loop of inference_pipeline (ctsd.py:1439-1654) for the SD 2.1 configs
    (examples/ctsd_21_6views_*_generation.json: DPMSolverMultistepScheduler, guidance 3, 50 steps): UNet forward at the
    CFG batch + guidance combine + DPM-Solver++(2M) update in one kernel.  latents fp32 [B,T,V,4,H,W]; conditions =
    CFG-doubled model kwargs (unconditional half first).

    Modes of inference_pipeline, with the keywords of CTSDDenoiser (what drivers.AutoregressiveDriver calls):
      * full-sequence denoising from noise (default; ctsd.py:1473-1476, 1509-1511, 1574-1575);
      * reference frames: `image_latents` + `reference_frame_count` = r - the first r frames of both CFG halves of the model
        input hold image_latents[:, :r] at timestep 0 on every step (:1514-1526) and the result is
        cat(image_latents[:, :r], latents[:, r:]) (:1623-1627).  Both schedulers: the update kernels take a flag per
        (sample, frame, view) image and leave the model input of a flagged image alone;
      * diffusion forcing, `schedulers.DDIMScheduler` only: per-frame timestep indices min(i - take_time*spi,
        max(0, i - j*spi)) (:1498-1507), the tensor-timestep DDIM step (:1559-1561, temporal_independent.py:67-170), frames
        outside the schedule range bit-unchanged (:1565-1572), `image_latents` in place of the start latents (:1470-1471).
        DPMSolverMultistepScheduler has no tensor-timestep step in the reference either: diffusion forcing, or a start
        step other than 0, with it is a ValueError.
    With none of these and the graph off, the step is the scalar-coefficient kernel as before.  In every other case the
    per-step numbers (timesteps, coefficient rows, flags) are rows of device tables built once per prepare(), so that the
    step can be captured: `enable_graph()` replays the whole step as one HIP graph, as CTSDDenoiser does."""

    def __init__(self, model, guidance_scale: float = 3.0, inference_steps: int = 50, prediction_type: str = "v_prediction",
                 scheduler=None):
        """scheduler None: DPM-Solver++(2M) (the example JSONs); a schedulers.DDIMScheduler: the reference's default test
        scheduler of the UNet (ctsd.py:969-974, `inference_config` without "scheduler"), its tensor-timestep step
        (temporal_independent.py:67-170) fused with the guidance combine."""
        self.model, self.guidance_scale, self.inference_steps = model, guidance_scale, inference_steps
        self.prediction_type = prediction_type
        self.scheduler = scheduler
        if scheduler is not None:
            if scheduler.config.prediction_type != prediction_type:
                raise ValueError(f"UNetDenoiser: prediction_type {prediction_type!r} disagrees with the scheduler's "
                                 f"{scheduler.config.prediction_type!r}")
            scheduler.set_timesteps(inference_steps)
            self.timesteps, self.sigmas = scheduler.timesteps.cpu(), None
        else:
            self.timesteps, self.sigmas = dpm_solver_tables(inference_steps)
        self.use_graph = False
        self._graph = None
        self._side = None

    def _check_mode(self, diffusion_forcing: bool, start: int = 0):
        if self.scheduler is None and (diffusion_forcing or start != 0):
            raise ValueError("UNetDenoiser: diffusion forcing / a start step other than 0 needs scheduler=schedulers.DDIMScheduler(): "
                             "DPM-Solver++(2M) is a multistep solver - it carries the x0 of the previous step and has no "
                             "tensor-timestep step (the reference's DPMSolverMultistepScheduler has none either)")

    def prepare(self, latents: torch.Tensor, conditions: Dict[str, torch.Tensor], image_latents: Optional[torch.Tensor] = None,
                reference_frame_count: int = 0, diffusion_forcing: bool = False, take_time: int = 0,
                clear_reference_frame_count: int = 0):
        self._check_mode(diffusion_forcing)
        self._graph = None                                                   # buffers below are re-created: capture again
        if diffusion_forcing and image_latents is not None:
            latents, image_latents = image_latents, None                     # ctsd.py:1470-1471
        dev = latents.device
        B, T, V = latents.shape[:3]
        self.diffusion_forcing = diffusion_forcing
        self.ref = reference_frame_count if image_latents is not None else 0
        if not 0 <= self.ref <= T:
            raise ValueError(f"UNetDenoiser: reference_frame_count {reference_frame_count} outside the {T} frames of the window")
        if diffusion_forcing:
            if self.inference_steps % (T - clear_reference_frame_count) != 0:
                raise ValueError("inference_steps must be a multiple of the frame count in diffusion-forcing mode")
        self._spi = self.inference_steps // (T - clear_reference_frame_count) if diffusion_forcing else 0
        self._take_time = take_time
        self.latents = latents.to(torch.float32).contiguous().clone()        # init_noise_sigma = 1
        self.x0_prev = torch.zeros_like(self.latents)
        self.image_latents = None if image_latents is None else image_latents.to(device=dev, dtype=torch.float32)
        # model input / conditions / prediction in the model's compute dtype: bf16, or fp32 for the accuracy path
        # (`model.compute_dtype = torch.float32`: BASELINE.json configs[0], the reference's fp32 denoise)
        self.cd = cd = getattr(self.model, "compute_dtype", bf16)
        self.model_in = torch.empty((2 * B, *latents.shape[1:]), dtype=cd, device=dev)
        lat16 = self.latents if cd == torch.float32 else ops.cast_bf16(self.latents)
        self.model_in[:B].copy_(lat16)
        self.model_in[B:].copy_(lat16)
        if self.ref > 0:                                                     # clean reference frames: written once, the update
            r16 = self.image_latents[:, :self.ref].to(cd)                    # kernels leave them alone (ctsd.py:1514-1519)
            self.model_in[:B, :self.ref].copy_(r16)
            self.model_in[B:, :self.ref].copy_(r16)
        self.conditions = {k: (v.to(cd) if torch.is_tensor(v) and v.is_floating_point() and k != "added_time_ids" else v)
                           for k, v in conditions.items()}
        self._ts = self.timesteps.to(dev).float()
        # DDIM: the [steps, 6] coefficient rows of every step, on the device, once per prepare() (no host-to-device copy and
        # no fp64 table gather inside the loop: the step is a plain index, as in the DPM-Solver path)
        self._ddim_coef = None
        if self.scheduler is not None:
            self._ddim_coef = self.scheduler.coefficients(self.timesteps.to(dev))
        # reference frames / diffusion forcing / graph: timesteps, coefficient rows and flags of every step as device tables
        self._tables = self._step_tables() if (self.ref > 0 or diffusion_forcing or self.use_graph) else None
        return self

    def _step_tables(self):
        """(first step, timesteps fp32 [n, 2B, T, V], coefficient rows fp32 [n, G | 1, 6 | 5], flags int32 [n, G] or None) with
        G = B T V groups in (sample, frame, view) order; row k serves step first + k"""
        (B, T, V), dev = self.latents.shape[:3], self.latents.device
        n, G = self.inference_steps, B * T * V
        first, flags = 0, None
        if self.diffusion_forcing:
            first, idx, in_range = diffusion_forcing_tables(n, T, self._spi, self._take_time)
            t_frame = self.timesteps[idx].to(dev)                                           # [n, T] integer timesteps
            flags = (~in_range).to(dev)
        else:
            t_frame = self.timesteps.to(dev).view(n, 1).repeat(1, T)
            if self.ref > 0:
                flags = (torch.arange(T) < self.ref).view(1, T).expand(n, T).to(dev)
        ts = t_frame.float()
        if self.ref > 0:
            ts[:, :self.ref] = 0                                                            # ctsd.py:1520-1526
        ts = ts.view(n, 1, T, 1).expand(n, 2 * B, T, V).contiguous()
        if flags is not None:
            flags = flags.view(n, 1, T, 1).expand(n, B, T, V).reshape(n, G).to(torch.int32).contiguous()
        if self.scheduler is not None:
            coef = self.scheduler.coefficients(t_frame).view(n, 1, T, 1, 6).expand(n, B, T, V, 6).reshape(n, G, 6).contiguous()
        else:
            coef = dpm_solver_coefficient_table(self.sigmas, self.prediction_type).to(dev).view(n, 1, 5)
        return first, ts, coef, flags

    def _prediction(self, ts: torch.Tensor) -> torch.Tensor:
        out = self.model(self.model_in, ts, **self.conditions)
        return out["noise_pred"] if isinstance(out, dict) else out[0][0]

    def _ddim_args(self):
        from .schedulers import PREDICTION_TYPES
        sc = self.scheduler
        return dict(group_elems=self.latents[0, 0, 0].numel(), prediction_type=PREDICTION_TYPES[sc.config.prediction_type],
                    guidance=self.guidance_scale, clip_range=sc.config.clip_sample_range if sc.config.clip_sample else 0.0)

    def step(self, i: int):
        if self._tables is None and self.use_graph:   # enable_graph() after prepare()
            self._tables = self._step_tables()
        if self._tables is not None:
            k = i - self._tables[0]
            if not 0 <= k < self.inference_steps:
                raise ValueError(f"UNetDenoiser: step {i} outside the steps [{self._tables[0]}, {self._tables[0] + self.inference_steps}) "
                                 "this prepare() serves")
            if self.use_graph:
                self._graph_step(k)
            else:
                _, ts, coef, flags = self._tables
                self._step_body(ts[k], coef[k], None if flags is None else flags[k])
            return
        B, T, V = self.latents.shape[:3]
        pred = self._prediction(self._ts[i].expand(2 * B, T, V))
        if self.scheduler is not None:
            coef = self._ddim_coef[i].expand(B * T * V, 6).contiguous()
            f32_path = self.cd == torch.float32       # (the kernel writes a bf16 model input; the fp32 path copies the latents)
            ops.cfg_ddim_step(pred, self.latents, coef, model_in=None if f32_path else self.model_in, **self._ddim_args())
            if f32_path:
                self.model_in[:B].copy_(self.latents)
                self.model_in[B:].copy_(self.latents)
            return
        kx, ko, A, Bc, Cc = dpm_solver_coefficients(self.sigmas, i, self.prediction_type)
        ops.cfg_multistep(pred, self.latents, self.x0_prev, self.guidance_scale, kx, ko, A, Bc, Cc, model_in=self.model_in)

    def _step_body(self, ts: torch.Tensor, coef: torch.Tensor, flags: Optional[torch.Tensor]):
        """one step from device-resident per-step numbers: nothing here reads a device value on the host, so it can be captured"""
        B, r = self.latents.shape[0], self.ref
        pred = self._prediction(ts)
        if self.scheduler is None:
            ops.cfg_multistep_grouped(pred, self.latents, self.x0_prev, self.guidance_scale, coef, self.latents[0, 0, 0].numel(),
                                      keep_model_in=flags, model_in=self.model_in)
            return
        f32_path = self.cd == torch.float32           # (as in step(): the DDIM kernel writes a bf16 model input only)
        ops.cfg_ddim_step(pred, self.latents, coef, model_in=None if f32_path else self.model_in, skip=flags, **self._ddim_args())
        if f32_path:                                  # the reference frames of the model input stay the clean ones
            self.model_in[:B, r:].copy_(self.latents[:, r:])
            self.model_in[B:, r:].copy_(self.latents[:, r:])

    # ---- whole-step HIP graph, as CTSDDenoiser's: the launches of one step (UNet forward, CFG combine, scheduler update) are
    # captured once per prepare() and replayed; timesteps, coefficient rows and flags live in static device buffers that are
    # refreshed (device-to-device, from the tables of prepare()) before each replay.
    def enable_graph(self, on: bool = True):
        self.use_graph = on
        self._graph = None
        return self

    def _graph_step(self, k: int):
        _, ts, coef, flags = self._tables
        if self._graph is None:
            self._g_ts, self._g_coef = ts[k].clone(), coef[k].clone()
            self._g_flags = None if flags is None else flags[k].clone()
            # one eager pass on a side stream fills every cache the forward keeps (packed weights, text K/V, index embeddings,
            # scratch buffers) and warms the allocator; the state it touched is restored before the capture
            keep = [t.clone() for t in (self.latents, self.x0_prev, self.model_in)]
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.latents.device)
            side = self._side
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                self._step_body(self._g_ts, self._g_coef, self._g_flags)
            torch.cuda.current_stream().wait_stream(side)
            for t, k0 in zip((self.latents, self.x0_prev, self.model_in), keep):
                t.copy_(k0)
            self._graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self._graph):
                self._step_body(self._g_ts, self._g_coef, self._g_flags)
        self._g_ts.copy_(ts[k])
        self._g_coef.copy_(coef[k])
        if flags is not None:
            self._g_flags.copy_(flags[k])
        self._graph.replay()

    def result(self) -> torch.Tensor:
        if self.ref > 0:                                                     # ctsd.py:1623-1627
            return torch.cat([self.image_latents[:, :self.ref], self.latents[:, self.ref:]], 1)
        return self.latents

    def run(self, latents, conditions, stop: Optional[int] = None, start: int = 0, **prepare_kw):
        self._check_mode(prepare_kw.get("diffusion_forcing", False), start)
        self.prepare(latents, conditions, **prepare_kw)
        for i in range(start, self.inference_steps if stop is None else stop):
            self.step(i)
        return self.result()
