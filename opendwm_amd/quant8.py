"""The number format of the block-wise 8-bit optimizer state (include/dwm_hip.h, "Block-wise 8-bit optimizer state"): the two
code tables.  They are data: the kernels receive them as device pointers, none is compiled in."""
from __future__ import annotations

import functools

import torch

BLOCK = 256                      # consecutive elements of one tensor that share one fp32 scale


def n_blocks(n: int) -> int:
    return (n + BLOCK - 1) // BLOCK


@functools.lru_cache(maxsize=None)
def _dynamic_code(signed: bool) -> torch.Tensor:
    # decade i of 7 covers [0.1, 1] * 10^(i-6) with 2^i (signed) or 2^(i+1) (unsigned) equal intervals; an entry is the middle of
    # its interval.  127 magnitudes per sign (signed) or 254 (unsigned), plus 0 and 1: 256 values.
    vals = [0.0, 1.0]
    for i in range(7):
        k = 2 ** i if signed else 2 ** (i + 1)
        for j in range(k):
            v = 10.0 ** (i - 6) * (0.1 + 0.9 * (j + 0.5) / k)
            vals += [v, -v] if signed else [v]
    code = torch.tensor(sorted(vals), dtype=torch.float64).to(torch.float32)
    assert code.numel() == 256 and bool((code[1:] > code[:-1]).all())
    return code


def dynamic_code(signed: bool) -> torch.Tensor:
    """256 sorted, distinct fp32 values: the dynamic map of "8-bit Optimizers via Block-wise Quantization" (Dettmers et al.
    2022) - a sign, 7 decades of exponent, a linear fraction whose resolution doubles with every decade, plus 0 and 1.
    signed: [-0.99297, 1], smallest non-zero magnitude 5.5e-7 (first moment); unsigned: [0, 1], 0, 3.25e-7, 7.75e-7, ...,
    0.98945, 0.99648, 1 (second moment).

    Built from the paper's description.  Files written by `bitsandbytes` are NOT a compatibility target: the package is not
    part of this stack, so agreement of the tables (and of the rounding) with it could not be checked."""
    return _dynamic_code(bool(signed)).clone()


_DEVICE_CODES: dict = {}


def device_codes(device: torch.device):
    """(signed, unsigned) tables on `device`, uploaded once"""
    key = (device.type, device.index)
    if key not in _DEVICE_CODES:
        _DEVICE_CODES[key] = (dynamic_code(True).to(device), dynamic_code(False).to(device))
    return _DEVICE_CODES[key]


def zero_code(signed: bool) -> int:
    """the code of 0.0: what fresh state is filled with"""
    return int((_dynamic_code(bool(signed)) == 0).nonzero().item())
