"""Low-rank adapters restated in fp64 plain torch on the CPU, with the element bounds the kernels of csrc/lora.hip are held to
(include/dwm_hip.h, "Low-rank adapters").  Imports nothing of the package.

    merge / fold   exact = W + s B A
                   |out - exact| <= 1/2 ulp_bf16(exact) + 2^-23 (r + 2) (|W| + |s| sum_j |B[n, j]| |A[j, k]|)
                   the first term for a bf16 `out` only: the fp32 fold is held to the second alone.
    project        dA = s B^T G (+ old), dB = s G A^T (+ old): per element 2^-23 (len + 2) sum |terms|, len = N for dA and K for
                   dB, the terms being the |s B G| / |s G A| products and, when accumulating, |old|.

Where the bounds come from: a sum of `len` fp32 products accumulated by fma in ANY order is off by at most (len - 1) 2^-24 times the
sum of the absolute terms; the multiplication by s and the final add are one rounding each, hence len + 2 with room to spare (the
bound uses 2^-23 per operation, twice the unit roundoff).  Rounding to bf16 (8 significand bits) moves a value by at most half a
bf16 ulp.  tests/test_lora_cpu.py runs a plain fp32 torch evaluation through them at the shapes of the GPU test."""
import torch

bf16, f32, f64 = torch.bfloat16, torch.float32, torch.float64
U23 = 2.0 ** -23

NS, KS, RS = (1, 7, 64, 200), (4, 60, 64, 192, 1536), (1, 4, 16, 64)


def ulp_bf16(x: torch.Tensor) -> torch.Tensor:
    """spacing of bf16 at |x| (fp64): 2^(floor(log2 |x|) - 7), the subnormal spacing 2^-133 below the normal range"""
    _, e = torch.frexp(x.abs().double())                 # |x| = m 2^e, m in [0.5, 1)
    return torch.ldexp(torch.ones_like(x, dtype=f64), (e - 8).clamp_min(-133))


def merge_exact(W, A, B, s):
    """(W + s B A, |W| + |s| |B| |A|) in fp64"""
    W, A, B = W.double(), A.double(), B.double()
    return W + s * (B @ A), W.abs() + abs(s) * (B.abs() @ A.abs())


def merge_bound(exact, mag, r: int, out_dtype) -> torch.Tensor:
    b = U23 * (r + 2) * mag
    return b + 0.5 * ulp_bf16(exact) if out_dtype == bf16 else b


def project_exact(G, A, B, s, old_dA=None, old_dB=None):
    """((dA, mag_dA), (dB, mag_dB)) in fp64; old_*: what the outputs held when accumulating"""
    G, A, B = G.double(), A.double(), B.double()
    dA, mA = s * (B.T @ G), abs(s) * (B.abs().T @ G.abs())
    dB, mB = s * (G @ A.T), abs(s) * (G.abs() @ A.abs().T)
    if old_dA is not None:
        dA, mA = dA + old_dA.double(), mA + old_dA.double().abs()
    if old_dB is not None:
        dB, mB = dB + old_dB.double(), mB + old_dB.double().abs()
    return (dA, mA), (dB, mB)


def project_bound(mag, length: int) -> torch.Tensor:
    return U23 * (length + 2) * mag


def ratio(got, exact, bound) -> float:
    """max |got - exact| / bound; a non-finite `got` gives inf; <= 1 passes"""
    g = got.double().cpu()
    d = (g - exact).abs()
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    r = torch.where(torch.isfinite(g), r, torch.full_like(r, float("inf")))
    return r.max().item() if r.numel() else 0.0


def operands(N: int, K: int, r: int, seed: int, w_dtype=f32):
    """(W, A, B, G) on the CPU: Gaussian weights of a linear layer's size, A of kaiming size, B and G random and non-zero, rows
    and columns of differing scale so that an index off by one moves a result out of its bound"""
    g = torch.Generator().manual_seed(seed)
    row = 1.0 + torch.arange(N, dtype=f32)[:, None] % 3
    col = 1.0 + 0.5 * (torch.arange(K, dtype=f32)[None, :] % 5)
    W = (torch.randn(N, K, generator=g) * 0.05 * row * col).to(w_dtype)
    A = (torch.rand(r, K, generator=g) * 2 - 1) * (K ** -0.5) * (1.0 + torch.arange(r, dtype=f32)[:, None] % 4)
    B = torch.randn(N, r, generator=g) * 0.1 * row
    G = (torch.randn(N, K, generator=g) * 0.01 * col).to(w_dtype)
    return W, A, B, G
