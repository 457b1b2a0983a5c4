"""The number format of the 4-bit text-encoder weights (include/dwm_hip.h, "NF4 4-bit weights"): the code table.  It is data: the
kernels receive it as a device pointer, nothing is compiled in.

A [N, K] weight is held as `q` (uint8 [N, K/2], element 2j of a row in the high nibble of byte j, element 2j+1 in the low one) and
`absmax` (fp32 [N, K/BLOCK], the largest |w| of BLOCK consecutive elements along K); its value is
W' = bf16_rne(fl32(CODE[q] * absmax)).  The quantiser is ops.nf4_quantize, the rule it implements is stated in the header.

No double quantisation, no fp4, no 8-bit.  Files written by `bitsandbytes` are NOT a compatibility target: the package is not part
of this stack, so agreement of the table (and of the rounding) with it could not be checked."""
from __future__ import annotations

import torch

BLOCK = 64                       # consecutive elements along K of one weight row that share one fp32 absmax

# the NF4 data type of "QLoRA: Efficient Finetuning of Quantized LLMs" (Dettmers et al. 2023), appendix E: 16 values in [-1, 1], each
# holding an equal share of a standard normal's mass, with an exact zero
_NF4 = (-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453,
        -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
        0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
        0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0)
CODE = torch.tensor(_NF4, dtype=torch.float32)
ZERO_CODE = 7                    # CODE[7] == 0.0: what an all-zero block is filled with


def n_blocks(k: int) -> int:
    if k % BLOCK:
        raise ValueError(f"K = {k} is not a multiple of {BLOCK}")
    return k // BLOCK


def packed_bytes(n: int, k: int) -> int:
    """bytes of q and absmax together for a [n, k] weight: n k / 2 + n k / 16 (bf16 holds 2 n k)"""
    return n * k // 2 + n * n_blocks(k) * 4


_DEVICE_CODE: dict = {}


def device_code(device: torch.device) -> torch.Tensor:
    """the table on `device`, uploaded once"""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    key = (device.type, device.index)
    if key not in _DEVICE_CODE:
        _DEVICE_CODE[key] = CODE.to(device)
    return _DEVICE_CODE[key]
