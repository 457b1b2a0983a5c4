"""The video modes of pipeline.UNetDenoiser, the part that needs no GPU: the device tables' host logic (DPM-Solver++ coefficient
rows, diffusion-forcing indices), the keyword validation, and the C ABI additions."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dpm_solver_coefficient_table_rows():
    """the [steps, 5] table dwm_cfg_multistep_grouped reads = dpm_solver_coefficients row by row (fp32 of the host doubles)"""
    from oracle import unet_oracle as U
    from opendwm_amd import pipeline as P
    for steps in (1, 3, 10):
        _, sig = P.dpm_solver_tables(steps)
        for pt in ("epsilon", "v_prediction"):
            tab = P.dpm_solver_coefficient_table(sig, pt)
            assert tab.shape == (steps, 5) and tab.dtype == torch.float32
            for i in range(steps):
                assert torch.equal(tab[i], torch.tensor(P.dpm_solver_coefficients(sig, i, pt), dtype=torch.float64).float())
                assert tab[i].tolist() == pytest.approx(U.dpm_solver_coefficients(U.dpm_solver_tables(steps)[1], i, pt), rel=1e-6)


def test_diffusion_forcing_tables_match_the_formula():
    """ctsd.py:1498-1507 / 1565-1570 for steps = 6, T = 3 (spi = 2) and T - clear = 2 (spi = 3), over every take_time: all the
    steps a call with that take_time can run (the emitted slot's index i - take_time * spi walks 0 .. steps - 1)"""
    from opendwm_amd.pipeline import diffusion_forcing_tables
    steps, T = 6, 3
    for spi in (2, 3):
        for take_time in range(T):
            i0, idx, in_range = diffusion_forcing_tables(steps, T, spi, take_time)
            assert i0 == take_time * spi and idx.shape == in_range.shape == (steps, T)
            assert idx.dtype == torch.int64 and in_range.dtype == torch.bool
            for k in range(steps):
                i = i0 + k
                assert idx[k].tolist() == [min(i - take_time * spi, max(0, i - j * spi)) for j in range(T)]
                assert in_range[k].tolist() == [i - j * spi >= 0 for j in range(T)]
            assert idx.min() >= 0 and idx.max() <= steps - 1                 # valid rows of scheduler.timesteps


def test_driver_windows_stay_inside_the_tables():
    """every window AutoregressiveDriver plans in diffusion-forcing mode runs steps the tables of its take_time hold"""
    from opendwm_amd.drivers import AutoregressiveDriver
    steps, T = 6, 3
    drv = AutoregressiveDriver(None, dict(inference_steps=steps, sequence_length_per_iteration=T, reference_frame_count=1),
                               diffusion_forcing=True)
    wins = drv.plan(T, 9, False)
    assert len(wins) > 3
    for w in wins:
        i0 = w.take_time * (steps // T)
        assert i0 <= w.start < w.stop <= i0 + steps


def test_keyword_validation():
    """what the modes refuse, before anything touches a device"""
    from opendwm_amd.pipeline import UNetDenoiser
    from opendwm_amd.schedulers import DDIMScheduler
    lat, cond = torch.zeros(1, 3, 2, 4, 8, 8), {}
    dpm = UNetDenoiser(None, 3.0, 6)
    with pytest.raises(ValueError, match="multistep solver"):
        dpm.run(lat, cond, diffusion_forcing=True)
    with pytest.raises(ValueError, match="multistep solver"):
        dpm.prepare(lat, cond, diffusion_forcing=True)
    with pytest.raises(ValueError, match="start step"):
        dpm.run(lat, cond, start=2)
    with pytest.raises(ValueError, match="reference_frame_count"):
        dpm.prepare(lat, cond, image_latents=lat, reference_frame_count=4)
    ddim = UNetDenoiser(None, 3.0, 6, scheduler=DDIMScheduler())
    with pytest.raises(ValueError, match="multiple of the frame count"):
        ddim.prepare(torch.zeros(1, 4, 2, 4, 8, 8), cond, diffusion_forcing=True)
    with pytest.raises(ValueError, match="multiple of the frame count"):
        ddim.prepare(lat, cond, diffusion_forcing=True, clear_reference_frame_count=-1)
    with pytest.raises(TypeError):
        dpm.run(lat, cond, no_such_keyword=1)


def test_abi_additions():
    """dwm_cfg_multistep_grouped / _f32 / dwm_cfg_ddim_step_masked: declared, bound and exported with one signature; additions
    do not move the ABI version.  Their argument checks run before any launch (fake, aligned device addresses)."""
    from opendwm_amd import _lib, build
    hdr = open(os.path.join(ROOT, "include", "dwm_hip.h")).read()
    lib = ctypes.CDLL(build.build())
    assert _lib.ABI_VERSION == 18 and re.search(r"#define DWM_ABI_VERSION 18\b", hdr)
    for name in ("dwm_cfg_multistep_grouped", "dwm_cfg_multistep_grouped_f32", "dwm_cfg_ddim_step_masked"):
        m = re.search(rf"^int {name}\(([^;]*)\);", hdr, flags=re.M)
        assert m, name
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(lib, name), name
    fake = 1 << 20
    for name in ("dwm_cfg_multistep_grouped", "dwm_cfg_multistep_grouped_f32"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]

        def call(n=2880, rows=12, ge=240, pred=fake, coef=fake, keep=None):
            return fn(pred, fake, fake, fake, n, 3.0, coef, rows, keep, ge, None)
        assert call(ge=242) != 0 and call(ge=6, rows=480) != 0            # group_elems % 4, n % group_elems
        assert call(ge=0) != 0 and call(n=0) != 0 and call(coef=None) != 0
        assert call(rows=5) != 0                                           # one row, or one per group
        assert call(pred=fake + 4) != 0 and call(keep=fake + 2) != 0       # alignment
    fn = lib.dwm_cfg_ddim_step_masked
    fn.restype, fn.argtypes = _lib.SIGNATURES["dwm_cfg_ddim_step_masked"]
    assert fn(fake, 0, 1, fake, fake, None, None, fake, 2880, 242, 3.0, 2, 0.0, 0, fake, None) != 0
    assert fn(fake, 0, 1, fake, fake, None, None, fake, 2880, 240, 3.0, 2, 0.0, 0, fake + 2, None) != 0
