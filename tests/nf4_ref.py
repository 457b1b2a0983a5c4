"""The NF4 weight format in plain torch on the CPU, written from its rules (include/dwm_hip.h, "NF4 4-bit weights"); imports nothing
from the library.  tests/test_nf4_cpu.py pins the properties of the format on it, the GPU tests hold the kernels to it bit for bit.

  table     CODE, the 16 fp32 values of the QLoRA paper's NF4 data type
  blocks    BLOCK = 64 consecutive elements along K of one row share absmax = max |w| (a bf16 value held as fp32)
  codes     MID[i] = fl32((CODE[i] + CODE[i+1]) / 2); the code of w = #{i : fl32(MID[i] * absmax) < w}; absmax == 0: code 7
  packing   byte j of a row = element 2j in the high nibble, element 2j + 1 in the low one
  value     W' = bf16_rne(fl32(CODE[code] * absmax))"""
import torch

BLOCK = 64
CODE = torch.tensor([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453,
                     -0.28444138169288635, -0.18477343022823334, -0.09105003625154495, 0.0,
                     0.07958029955625534, 0.16093020141124725, 0.24611230194568634, 0.33791524171829224,
                     0.44070982933044434, 0.5626170039176941, 0.7229568362236023, 1.0], dtype=torch.float32)
MID = (CODE[:-1] + CODE[1:]) / 2                  # fp32 arithmetic: the sum rounds once, the halving is exact


def codes(w, code=CODE):
    """(codes int64 [N, K], absmax fp32 [N, K / BLOCK]) of a bf16 (or bf16-valued) [N, K] weight"""
    N, K = w.shape
    assert K % BLOCK == 0
    x = w.float().view(N, K // BLOCK, BLOCK)
    absmax = x.abs().amax(-1)
    mid = (code[:-1] + code[1:]) / 2
    edges = mid.view(1, 1, 1, 15) * absmax.view(N, -1, 1, 1)                       # fl32(MID[i] * absmax)
    c = (edges < x.unsqueeze(-1)).sum(-1)                                            # strict: a tie goes to the lower code
    c = torch.where((absmax == 0).unsqueeze(-1), torch.full_like(c, 7), c)
    return c.view(N, K), absmax


def pack(c):
    """codes [N, K] -> uint8 [N, K / 2]"""
    return ((c[:, 0::2] << 4) | c[:, 1::2]).to(torch.uint8)


def unpack(q):
    """uint8 [N, K / 2] -> codes int64 [N, K]"""
    q = q.long()
    return torch.stack([q >> 4, q & 15], -1).view(q.shape[0], -1)


def quantize(w, code=CODE):
    """-> (q uint8 [N, K / 2], absmax fp32 [N, K / BLOCK])"""
    c, absmax = codes(w, code)
    return pack(c), absmax


def dequantize(q, absmax, code=CODE):
    """-> W' bf16 [N, K]"""
    c = unpack(q)
    N, K = c.shape
    v = code[c].view(N, K // BLOCK, BLOCK) * absmax.view(N, -1, 1)                   # one fp32 product per element
    return v.view(N, K).to(torch.bfloat16)


def requantized_state_dict(sd, names):
    """a copy of the bf16 state dict `sd` with W' in place of the weight of every linear layer in `names` (module names)"""
    out = dict(sd)
    for n in names:
        out[n + ".weight"] = dequantize(*quantize(sd[n + ".weight"]))
    return out
