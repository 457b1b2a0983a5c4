// Backward-pass / optimizer kernels of the CTSD train step (reference: src/dwm/pipelines/ctsd.py
// :1195-1437, backward of the modules listed in include/dwm_hip.h).  All HBM-bound: 16-B bf16x8
// accesses, fp32 arithmetic, reductions accumulated with fp32 atomics into caller-zeroed buffers - or, in the ORDERED instantiation
// of the same kernels (dwm_*_ordered), written as per-workgroup partials and folded in a fixed order by ordered_finish_kernel.
#include "common.h"
#include "dwm_hip.h"

namespace {

// ---------------------------------------------------------------------------------- transpose
// 64 x 64 tile through LDS (row pitch 66 elements: conflict-free column reads); out[c][r] = in[r][c],
// output columns [rows, rows_pad) are zero-filled.
__global__ void __launch_bounds__(256)
transpose_kernel(const bf16_t* __restrict__ in, int64_t ld_in, int64_t rows, int64_t cols,
                 bf16_t* __restrict__ out, int64_t ld_out, int64_t rows_pad) {
    __shared__ bf16_t tile[64][66];
    const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t r = r0 + ty * 16 + i, c = c0 + tx;
        tile[ty * 16 + i][tx] = (r < rows && c < cols) ? in[r * ld_in + c] : (bf16_t)0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t c = c0 + ty * 16 + i, r = r0 + tx;
        if (c < cols && r < rows_pad) out[c * ld_out + r] = tile[tx][ty * 16 + i];
    }
}

// Vector form (cols % 8 == 0, rows_pad % 8 == 0, 16-byte aligned rows on both sides): a thread owns an 8 x 8 block -
// eight 16-byte row loads, a register transpose (v_perm_b32), eight 16-byte stores - so no LDS round trip and every
// store instruction of a wave writes 4 output rows x 256 contiguous bytes.  Workgroup = 128 rows x 128 cols.
__global__ void __launch_bounds__(256)
transpose8_kernel(const bf16_t* __restrict__ in, int64_t ld_in, int64_t rows, int64_t cols,
                  bf16_t* __restrict__ out, int64_t ld_out, int64_t rows_pad) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 128 + wave * 32 + (lane & 3) * 8;
    const int64_t r = (int64_t)blockIdx.y * 128 + (lane >> 2) * 8;
    if (c >= cols || r >= rows_pad) return;
    uint32_t v[8][4];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (r + i < rows) q = *(const uint4*)(in + (r + i) * ld_in + c);
        v[i][0] = q.x; v[i][1] = q.y; v[i][2] = q.z; v[i][3] = q.w;
    }
#pragma unroll
    for (int cc = 0; cc < 8; ++cc) {
        const uint32_t sel = (cc & 1) ? 0x07060302u : 0x05040100u;     // high / low halves of the two source dwords
        uint4 o;
        o.x = __builtin_amdgcn_perm(v[1][cc >> 1], v[0][cc >> 1], sel);
        o.y = __builtin_amdgcn_perm(v[3][cc >> 1], v[2][cc >> 1], sel);
        o.z = __builtin_amdgcn_perm(v[5][cc >> 1], v[4][cc >> 1], sel);
        o.w = __builtin_amdgcn_perm(v[7][cc >> 1], v[6][cc >> 1], sel);
        *(uint4*)(out + (c + cc) * ld_out + r) = o;
    }
}

// ---------------------------------------------------------------------------------- segmented sums
// out[g][n] += sum_{r in group g} a[r][n] * (b ? b[r][n] : 1).  Block = 256 threads = 32 column
// chunks (8 columns each) x 8 row lanes; a block covers 256 columns x up to RB rows of ONE group.
// ORDERED (dwm_segsum_ordered / dwm_segsum_diff_ordered): the block's 256 column sums go to row blockIdx.y = g * chunks_per_group + ch
// of the workspace `ws` [groups * chunks_per_group, ncols] with plain 16-byte stores - empty row ranges included, as zeros - and
// dwm_ordered_finish adds them into `out`.
constexpr int SEG_RB = 128;
template <bool ORDERED>
__global__ void __launch_bounds__(256)
segsum_kernel(const bf16_t* __restrict__ a, int64_t lda, const bf16_t* __restrict__ b, int64_t ldb,
              const bf16_t* __restrict__ b2, int64_t ldb2,
              int64_t rows, int64_t ncols, int64_t rpg, int chunks_per_group, float* __restrict__ out, int64_t ld_out,
              float* __restrict__ ws) {
    __shared__ float red[8][256];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int64_t g = blockIdx.y / chunks_per_group, ch = blockIdx.y % chunks_per_group;
    const int64_t rbeg = g * rpg + ch * SEG_RB;
    int64_t rend = rbeg + SEG_RB;
    const int64_t gend = (g + 1) * rpg < rows ? (g + 1) * rpg : rows;
    if (rend > gend) rend = gend;
    const int64_t c = (int64_t)blockIdx.x * 256 + cx * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (c < ncols) {
        for (int64_t r = rbeg + ry; r < rend; r += 8) {
            float va[8], vb[8];
            unpack8(*(const uint4*)(a + r * lda + c), va);
            if (b2) {           // a * (b - b2): the difference is taken in fp32 before the product (AlphaBlender d(alpha))
                float vc[8];
                unpack8(*(const uint4*)(b + r * ldb + c), vb);
                unpack8(*(const uint4*)(b2 + r * ldb2 + c), vc);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += va[j] * (vb[j] - vc[j]);
            } else if (b) {
                unpack8(*(const uint4*)(b + r * ldb + c), vb);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += va[j] * vb[j];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] += va[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) red[ry][cx * 8 + j] = acc[j];
    __syncthreads();
    if constexpr (ORDERED) {
        const int64_t c4 = (int64_t)blockIdx.x * 256 + threadIdx.x * 4;
        if (threadIdx.x < 64 && c4 < ncols) {
            float s[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int i = 0; i < 8; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] += red[i][threadIdx.x * 4 + j];
            *(float4*)(ws + (int64_t)blockIdx.y * ncols + c4) = make_float4(s[0], s[1], s[2], s[3]);
        }
    } else {
        const int col = threadIdx.x;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += red[i][col];
        const int64_t cc = (int64_t)blockIdx.x * 256 + col;
        if (cc < ncols && rbeg < rend) atomicAdd(out + g * ld_out + cc, s);
    }
}

// ---------------------------------------------------------------------------------- ordered finish
// Stage 2 of every ordered reduction (contract: DwmFoldArgs in common.h).  A thread owns 4 adjacent columns of one (slot, group): a
// wave reads 1 KiB of each partial row, 16 B per lane, FOLD_UNROLL rows requested before the first is added (the fold is a serial
// chain per column; only the loads overlap), and the running sums stay in registers.  Block = one wave, so that the few columns
// of a launch (1536 columns = 6 waves per group) spread over as many CUs as there are waves.
constexpr int FOLD_UNROLL = 32;           // 128 VGPRs of loads in flight per lane: the chain is nfold / 32 memory round trips long
__global__ void __launch_bounds__(64)
ordered_finish_kernel(const DwmFoldArgs f) {
    const int64_t c = ((int64_t)blockIdx.x * 64 + threadIdx.x) * 4;
    if (c >= f.ncols) return;
    const int64_t g = blockIdx.y;
    const float* __restrict__ p = f.ws[blockIdx.z] + g * f.group_stride + c;
    float t[4] = {0.f, 0.f, 0.f, 0.f};
    int64_t k = 0;
    for (; k + FOLD_UNROLL <= f.nfold; k += FOLD_UNROLL) {
        float4 v[FOLD_UNROLL];
#pragma unroll
        for (int u = 0; u < FOLD_UNROLL; ++u) v[u] = *(const float4*)(p + (k + u) * f.fold_stride);
#pragma unroll
        for (int u = 0; u < FOLD_UNROLL; ++u) { t[0] += v[u].x; t[1] += v[u].y; t[2] += v[u].z; t[3] += v[u].w; }
    }
    for (; k < f.nfold; ++k) {
        const float4 v = *(const float4*)(p + k * f.fold_stride);
        t[0] += v.x; t[1] += v.y; t[2] += v.z; t[3] += v.w;
    }
    float* __restrict__ o = f.out[blockIdx.z] + g * f.ld_out + c;
    if ((((uintptr_t)o) & 15u) == 0) {          // a float4 of the accumulator where it is aligned, four floats where it is not
        float4 a = *(const float4*)o;
        a.x += t[0]; a.y += t[1]; a.z += t[2]; a.w += t[3];
        *(float4*)o = a;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] += t[j];
    }
}

// ---------------------------------------------------------------------------------- activations
DWM_DEVINL float gelu_tanh_grad(float x) {
    // d/dx [x * sigmoid(2u)],  u = k (x + 0.044715 x^3)
    const float z = x * (2.302208198f + 0.1029432397f * x * x);                 // 2 u log2(e)
    const float s = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-z));   // sigmoid(2u)
    const float du2 = 1.5957691216f + 0.2140624845f * x * x;                    // d(2u)/dx = 2k (1 + 3*0.044715 x^2)
    return s + x * s * (1.f - s) * du2;
}
DWM_DEVINL float silu_grad(float x) {
    const float s = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
    return s * (1.f + x * (1.f - s));
}
DWM_DEVINL float gelu_erf_grad(float x) {
    // 0.5 (1 + erf(x / sqrt 2)) + x * exp(-x^2 / 2) / sqrt(2 pi)
    return 0.5f * (1.f + erf_fast_f(x * 0.7071067811865476f)) +
           x * 0.3989422804014327f * __builtin_amdgcn_exp2f(-0.7213475204444817f * x * x);
}

template <int ACT, bool BWD>
__global__ void __launch_bounds__(256)
act_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, bf16_t* __restrict__ out, int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        float v[8], d[8];
        unpack8(*(const uint4*)(x + i * 8), v);
        if (BWD) unpack8(*(const uint4*)(dy + i * 8), d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (!BWD) v[j] = ACT == DWM_ACT_GELU_TANH ? gelu_tanh_f(v[j]) : ACT == DWM_ACT_RELU ? fmaxf(v[j], 0.f) : silu_f(v[j]);
            else v[j] = ACT == DWM_ACT_RELU ? (v[j] > 0.f ? d[j] : 0.f)          // x may be the pre- or the post-activation
                                            : d[j] * (ACT == DWM_ACT_GELU_TANH ? gelu_tanh_grad(v[j]) : silu_grad(v[j]));
        }
        *(uint4*)(out + i * 8) = pack8(v);
    }
}

// Backward that also re-derives the activation it differentiates: y = act(x), dx = dy * act'(x) from one read of x.  The two results
// come from the expressions of act_kernel<ACT, false> and act_kernel<ACT, true>, so they are the values those kernels write.
template <int ACT>
__global__ void __launch_bounds__(256)
act_bwd_recompute_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy, bf16_t* __restrict__ y, bf16_t* __restrict__ dx,
                         int64_t n8) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
        float v[8], d[8], o[8];
        unpack8(*(const uint4*)(x + i * 8), v);
        unpack8(*(const uint4*)(dy + i * 8), d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            o[j] = ACT == DWM_ACT_GELU_TANH ? gelu_tanh_f(v[j]) : ACT == DWM_ACT_RELU ? fmaxf(v[j], 0.f) : silu_f(v[j]);
            d[j] = ACT == DWM_ACT_RELU ? (v[j] > 0.f ? d[j] : 0.f)
                                       : d[j] * (ACT == DWM_ACT_GELU_TANH ? gelu_tanh_grad(v[j]) : silu_grad(v[j]));
        }
        *(uint4*)(y + i * 8) = pack8(o);
        *(uint4*)(dx + i * 8) = pack8(d);
    }
}

// GEGLU: u [rows, 2*inner] = [value | gate];  g = value * gelu_erf(gate)
template <bool BWD>
__global__ void __launch_bounds__(256)
geglu_kernel(const bf16_t* __restrict__ u, int64_t ldu, const bf16_t* __restrict__ dg, int64_t lddg,
             bf16_t* __restrict__ out, int64_t ldo, int64_t rows, int64_t inner) {
    const int64_t c8 = inner / 8, total = rows * c8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / c8, c = (i - r * c8) * 8;
        float hv[8], gt[8];
        unpack8(*(const uint4*)(u + r * ldu + c), hv);
        unpack8(*(const uint4*)(u + r * ldu + inner + c), gt);
        if (!BWD) {
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = hv[j] * gelu_erf_f(gt[j]);
            *(uint4*)(out + r * ldo + c) = pack8(o);
        } else {
            float d[8], dv[8], dgt[8];
            unpack8(*(const uint4*)(dg + r * lddg + c), d);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                dv[j] = d[j] * gelu_erf_f(gt[j]);
                dgt[j] = d[j] * hv[j] * gelu_erf_grad(gt[j]);
            }
            *(uint4*)(out + r * ldo + c) = pack8(dv);
            *(uint4*)(out + r * ldo + inner + c) = pack8(dgt);
        }
    }
}

// geglu_kernel<true> that also writes g = value * gelu(gate), the operand of the second linear's weight gradient
__global__ void __launch_bounds__(256)
geglu_bwd_recompute_kernel(const bf16_t* __restrict__ u, int64_t ldu, const bf16_t* __restrict__ dg, int64_t lddg,
                           bf16_t* __restrict__ g, int64_t ldg, bf16_t* __restrict__ du, int64_t lddu, int64_t rows, int64_t inner) {
    const int64_t c8 = inner / 8, total = rows * c8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / c8, c = (i - r * c8) * 8;
        float hv[8], gt[8], d[8], o[8], dv[8], dgt[8];
        unpack8(*(const uint4*)(u + r * ldu + c), hv);
        unpack8(*(const uint4*)(u + r * ldu + inner + c), gt);
        unpack8(*(const uint4*)(dg + r * lddg + c), d);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            o[j] = hv[j] * gelu_erf_f(gt[j]);
            dv[j] = d[j] * gelu_erf_f(gt[j]);
            dgt[j] = d[j] * hv[j] * gelu_erf_grad(gt[j]);
        }
        *(uint4*)(g + r * ldg + c) = pack8(o);
        *(uint4*)(du + r * lddu + c) = pack8(dv);
        *(uint4*)(du + r * lddu + inner + c) = pack8(dgt);
    }
}

// out[r][n] = ca(r) * a[r][n] + cb(r) * b[r][n]
//   ca(r) = (ga ? ga[r / rpa][n] : 1) * (fa ? fa[r / rfa] : 1);  cb likewise without a per-column vector
__global__ void __launch_bounds__(256)
rowcombine_kernel(const bf16_t* __restrict__ a, int64_t lda, const bf16_t* __restrict__ ga, int64_t ld_ga, int64_t rpa,
                  const float* __restrict__ fa, int64_t rfa,
                  const bf16_t* __restrict__ b, int64_t ldb, const float* __restrict__ fb, int64_t rfb,
                  bf16_t* __restrict__ out, int64_t ldo, int64_t rows, int64_t ncols) {
    const int64_t c8 = ncols / 8, total = rows * c8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / c8, c = (i - r * c8) * 8;
        float va[8], o[8];
        unpack8(*(const uint4*)(a + r * lda + c), va);
        const float sa = fa ? fa[r / rfa] : 1.f;
        if (ga) {
            float vg[8];
            unpack8(*(const uint4*)(ga + (r / rpa) * ld_ga + c), vg);
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = va[j] * vg[j] * sa;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = va[j] * sa;
        }
        if (b) {
            float vb[8];
            unpack8(*(const uint4*)(b + r * ldb + c), vb);
            const float sb = fb ? fb[r / rfb] : 1.f;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] += vb[j] * sb;
        }
        *(uint4*)(out + r * ldo + c) = pack8(o);
    }
}

// ---------------------------------------------------------------------------------- LayerNorm backward
// One wave per row (row in registers), RB/4 rows per wave sequentially; per-lane fp32 partial
// sums of the parameter / modulation gradients over the wave's rows, reduced over the 4 waves in
// LDS and flushed with one atomic per column and workgroup.
constexpr int LN_BWD_RB = 64;        // (round 4: 128 -> 64.  One training sample is 43 008 rows = 336 blocks of 128: 1.3 blocks per CU, 32
                                     //  rows per wave one after the other, each a chain of three memory round trips - 219 us for 400 MB)
// ORDERED (dwm_layernorm_bwd_ordered): the flush writes the block's column sums of the s-th non-null accumulator (order dgamma, dbeta,
// dgamma2, dbeta2) to ws[(s * gridDim.x + blockIdx.x) * D ...] instead - every block, empty row ranges as zeros - for
// dwm_ordered_finish.  Everything before the flush is the one body of both forms.
template <int NI, bool ORDERED>
__global__ void __launch_bounds__(256)
layernorm_bwd_kernel(const dwm_layernorm_bwd_args p, int chunks_per_group, float* __restrict__ ws) {
    constexpr int RB = LN_BWD_RB;           // rows per block (a quarter per wave)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int D = p.D;
    const int64_t rpg = p.rows_per_mod > 0 ? p.rows_per_mod : p.rows;
    const int64_t g = blockIdx.x / chunks_per_group, ch = blockIdx.x % chunks_per_group;
    const int64_t rbeg = g * rpg + ch * RB;
    int64_t rend = rbeg + RB;
    const int64_t gend = (g + 1) * rpg < p.rows ? (g + 1) * rpg : p.rows;
    if (rend > gend) rend = gend;

    const bf16_t* __restrict__ w = (const bf16_t*)p.weight;
    const bf16_t* sc = p.scale ? (const bf16_t*)p.scale + g * p.ld_mod : nullptr;
    const bf16_t* sc2 = p.scale2 ? (const bf16_t*)p.scale2 + g * p.ld_mod : nullptr;
    float gam[NI][8], gam2[NI][8];          // effective gamma of output 1 / 2
    bool ok[NI];
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        const int c = (i * 64 + lane) * 8;
        ok[i] = c < D;
#pragma unroll
        for (int j = 0; j < 8; ++j) { gam[i][j] = 1.f; gam2[i][j] = 1.f; }
        if (ok[i]) {
            float t[8];
            if (w) { unpack8(*(const uint4*)(w + c), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) gam[i][j] = t[j]; }
            if (sc) { unpack8(*(const uint4*)(sc + c), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) gam[i][j] *= 1.f + t[j]; }
            if (sc2) { unpack8(*(const uint4*)(sc2 + c), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) gam2[i][j] = 1.f + t[j]; }
        }
    }
    float sg[NI][8], sb[NI][8], sg2[NI][8], sb2[NI][8];   // sum dy*xhat, sum dy (outputs 1 / 2)
#pragma unroll
    for (int i = 0; i < NI; ++i)
#pragma unroll
        for (int j = 0; j < 8; ++j) { sg[i][j] = sb[i][j] = sg2[i][j] = sb2[i][j] = 0.f; }

    for (int64_t row = rbeg + wave; row < rend; row += 4) {
        const bf16_t* __restrict__ x = (const bf16_t*)p.x + row * p.ldx;
        const bf16_t* addv = p.addvec ? (const bf16_t*)p.addvec + (row / p.rows_per_add) * p.ld_add : nullptr;
        float v[NI][8];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = (i * 64 + lane) * 8;
            if (ok[i]) {
                unpack8(*(const uint4*)(x + c), v[i]);
                if (addv) {
                    float a[8];
                    unpack8(*(const uint4*)(addv + c), a);
#pragma unroll
                    for (int j = 0; j < 8; ++j) v[i][j] += a[j];
                    const uint4 r = pack8(v[i]);          // same rounding point as the forward kernel
                    unpack8(r, v[i]);
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) s += v[i][j];
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
            }
        }
        // the incoming gradients are requested NOW, before the two wave reductions of the statistics (they do not depend on
        // them): one memory round trip per row less on the critical path
        const bf16_t* __restrict__ dy = (const bf16_t*)p.dy + row * p.lddy;
        const bf16_t* __restrict__ dy2 = p.dy2 ? (const bf16_t*)p.dy2 + row * p.lddy2 : nullptr;
        uint4 dyr[NI], dy2r[NI];
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = ok[i] ? (i * 64 + lane) * 8 : 0;
            dyr[i] = *(const uint4*)(dy + c);
            dy2r[i] = dy2 ? *(const uint4*)(dy2 + c) : dyr[i];
        }
        const float mean = wave_sum_dpp(s) / (float)D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            if (ok[i]) {
#pragma unroll
                for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; q += d * d; }
            }
        const float rstd = rsqrtf(wave_sum_dpp(q) / (float)D + p.eps);

        float dxh[NI][8];                    // d loss / d xhat
        float m1 = 0.f, m2 = 0.f;            // sum dxhat, sum dxhat * xhat
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const int c = (i * 64 + lane) * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) dxh[i][j] = 0.f;
            if (!ok[i]) continue;
            float d[8];
            unpack8(dyr[i], d);
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float xh = (v[i][j] - mean) * rstd;
                v[i][j] = xh;
                sg[i][j] += d[j] * xh;
                sb[i][j] += d[j];
                dxh[i][j] = d[j] * gam[i][j];
            }
            if (dy2) {
                unpack8(dy2r[i], d);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    sg2[i][j] += d[j] * v[i][j];
                    sb2[i][j] += d[j];
                    dxh[i][j] += d[j] * gam2[i][j];
                }
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) { m1 += dxh[i][j]; m2 += dxh[i][j] * v[i][j]; }
        }
        m1 = wave_sum_dpp(m1) / (float)D;
        m2 = wave_sum_dpp(m2) / (float)D;
        bf16_t* __restrict__ dx = (bf16_t*)p.dx + row * p.lddx;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            if (!ok[i]) continue;
            const int c = (i * 64 + lane) * 8;
            float o[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = rstd * (dxh[i][j] - m1 - v[i][j] * m2);
            if (p.accumulate) {
                float t[8];
                unpack8(*(const uint4*)(dx + c), t);
#pragma unroll
                for (int j = 0; j < 8; ++j) o[j] += t[j];
            }
            *(uint4*)(dx + c) = pack8(o);
        }
    }
    // flush: dgamma[gg][c], dbeta[gg][c]; gg = group for modulation gradients, 0 for affine parameters
    __shared__ float red[4][NI * 512];
    const int64_t gg = p.grad_per_group ? g : 0;
    float* const outs[4] = {p.dgamma, p.dbeta, p.dgamma2, p.dbeta2};
    int slot = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (outs[q] == nullptr) continue;               // kernel-argument uniform
        __syncthreads();
#pragma unroll
        for (int i = 0; i < NI; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j)
                red[wave][(i * 64 + lane) * 8 + j] = q == 0 ? sg[i][j] : q == 1 ? sb[i][j] : q == 2 ? sg2[i][j] : sb2[i][j];
        __syncthreads();
        if constexpr (ORDERED) {
            float* __restrict__ wrow = ws + ((int64_t)slot * gridDim.x + blockIdx.x) * D;
            for (int c = threadIdx.x * 4; c < D; c += 1024) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = (red[0][c + j] + red[1][c + j]) + (red[2][c + j] + red[3][c + j]);
                *(float4*)(wrow + c) = make_float4(v[0], v[1], v[2], v[3]);
            }
            ++slot;
        } else {
            for (int c = threadIdx.x; c < D; c += 256) {
                const float v = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
                if (rbeg < rend) atomicAdd(outs[q] + gg * p.ld_grad + c, v);
            }
        }
    }
}

// ---------------------------------------------------------------------------------- per-head RMSNorm
// forward (in place) with the reciprocal RMS kept for the backward; one wave per row, a lane pair per
// ... simpler: 8 lanes per head (8 elements each), ncols/8 lanes busy per row pass of 512 columns.
__global__ void __launch_bounds__(256)
rmsnorm_heads_train_kernel(bf16_t* __restrict__ x, int64_t ldx, int64_t rows, int64_t ncols,
                           const bf16_t* __restrict__ w, float eps, float* __restrict__ rinv_out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int64_t nh = ncols / 64;
    for (int64_t c = lane * 8; c < ncols; c += 512) {
        float v[8], t[8];
        unpack8(*(const uint4*)(x + row * ldx + c), v);
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
        ss += __shfl_xor(ss, 1, 64); ss += __shfl_xor(ss, 2, 64); ss += __shfl_xor(ss, 4, 64);
        const float rinv = rsqrtf(ss * (1.f / 64.f) + eps);
        unpack8(*(const uint4*)(w + c), t);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= rinv * t[j];
        *(uint4*)(x + row * ldx + c) = pack8(v);
        if (rinv_out && (lane & 7) == 0) rinv_out[row * nh + c / 64] = rinv;
    }
}

// backward in place on dy (-> dx); y = normalised output (xhat * w), rinv from the forward.
// dw[c] += sum_rows dy * xhat (fp32 atomics; block-local LDS reduction first).
// ORDERED (dwm_rmsnorm_heads_bwd_ordered): no atomics.  The columns are walked in tiles of RMS_ORD_TILE; each wave puts its sums of a
// tile into its own LDS row (every slot is written: a wave without rows writes zeros), the rows are added as ((w0 + w1) + w2) + w3
// and the result goes to row blockIdx.x of the workspace `ws` [blocks, ncols] for dwm_ordered_finish.  The default form is the
// same body with one tile = all columns.
constexpr int RMS_ORD_TILE = 4096;        // columns per tile of the ordered form: 4 LDS rows = 64 KiB
template <bool ORDERED>
__global__ void __launch_bounds__(256)
rmsnorm_heads_bwd_kernel(const bf16_t* __restrict__ y, int64_t ldy, const float* __restrict__ rinv,
                         const bf16_t* __restrict__ w, bf16_t* __restrict__ dy, int64_t lddy,
                         int64_t rows, int64_t ncols, float* __restrict__ dw, float* __restrict__ ws) {
    extern __shared__ float dwl[];            // [ncols]; ORDERED: [4][tile]
    const int64_t tile = ORDERED && ncols > RMS_ORD_TILE ? RMS_ORD_TILE : ncols;
    if constexpr (!ORDERED) {
        for (int i = threadIdx.x; i < ncols; i += 256) dwl[i] = 0.f;
        __syncthreads();
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t nh = ncols / 64;
    const int64_t rbeg = (int64_t)blockIdx.x * 32;
    for (int64_t c0 = 0; c0 < ncols; c0 += tile) {          // block-uniform; one trip in the default form
        const int64_t cend = c0 + tile < ncols ? c0 + tile : ncols;
        for (int64_t c = c0 + lane * 8; c < cend; c += 512) {
            float wv[8], acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            unpack8(*(const uint4*)(w + c), wv);
            for (int64_t row = rbeg + wave; row < rbeg + 32 && row < rows; row += 4) {
                float yv[8], d[8], xh[8], dxh[8];
                unpack8(*(const uint4*)(y + row * ldy + c), yv);
                unpack8(*(const uint4*)(dy + row * lddy + c), d);
                float m = 0.f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    xh[j] = wv[j] != 0.f ? yv[j] / wv[j] : 0.f;
                    acc[j] += d[j] * xh[j];
                    dxh[j] = d[j] * wv[j];
                    m += dxh[j] * xh[j];
                }
                m += __shfl_xor(m, 1, 64); m += __shfl_xor(m, 2, 64); m += __shfl_xor(m, 4, 64);
                m *= 1.f / 64.f;
                const float ri = rinv[row * nh + c / 64];
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = ri * (dxh[j] - xh[j] * m);
                *(uint4*)(dy + row * lddy + c) = pack8(d);
            }
            if constexpr (ORDERED) {
                float* const l = dwl + wave * tile + (c - c0);
                *(float4*)l = make_float4(acc[0], acc[1], acc[2], acc[3]);
                *(float4*)(l + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) atomicAdd(&dwl[c + j], acc[j]);
            }
        }
        __syncthreads();
        if constexpr (ORDERED) {
            for (int64_t i = threadIdx.x * 4; i < cend - c0; i += 1024) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = ((dwl[i + j] + dwl[tile + i + j]) + dwl[2 * tile + i + j]) + dwl[3 * tile + i + j];
                *(float4*)(ws + (int64_t)blockIdx.x * ncols + c0 + i) = make_float4(v[0], v[1], v[2], v[3]);
            }
            __syncthreads();                               // the next tile overwrites the rows
        } else {
            for (int i = threadIdx.x; i < ncols; i += 256)
                if (dwl[i] != 0.f) atomicAdd(dw + i, dwl[i]);
        }
    }
}

// ---------------------------------------------------------------------------------- optimizer / casts
// AdamW (decoupled weight decay, torch.optim.AdamW semantics) on fp32 master parameters; refreshes
// the bf16 compute copy in the same pass.
struct AdamwHyper { float lr, b1, b2, eps, wd, bc1, bc2, gscale; };

// One element: the new p; m and v go in as the old moments and come out as the new ones.  The callers read g, p, m, v in that order
// before the call: which product of a moment update the compiler fuses into the fma follows the order of the loads, and the last bit
// of m and v with it.
DWM_DEVINL float adamw_update(float p, float g, float& m, float& v, const AdamwHyper& h) {
    const float gi = g * h.gscale;
    float pi = p * (1.f - h.lr * h.wd);
    m = h.b1 * m + (1.f - h.b1) * gi;
    v = h.b2 * v + (1.f - h.b2) * gi * gi;
    pi -= h.lr * (m / h.bc1) / (sqrtf(v / h.bc2) + h.eps);
    return pi;
}

__global__ void __launch_bounds__(256)
adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
             bf16_t* __restrict__ pb, int64_t n, float lr, float b1, float b2, float eps, float wd,
             float bc1, float bc2, float gscale) {
    const AdamwHyper h{lr, b1, b2, eps, wd, bc1, bc2, gscale};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float gi = g[i], p0 = p[i];
        float mi = m[i], vi = v[i];
        const float pi = adamw_update(p0, gi, mi, vi, h);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (pb) pb[i] = f32_to_bf16(pi);
    }
}

// The same update for MANY tensors in one launch: block b works on elements [block_start[b], block_start[b] + chunk) of tensor
// block_item[b] (a model has 1.4-1.7 k parameter tensors: per-tensor launches made the optimizer step launch-bound).
//
// Exponential moving average of the weights (dwm_adamw_ema_multi & co., DESIGN s27): e' = e + omd * (p' - e) in fp32, p' the value
// the same thread stores to p, omd = 1 - decay uniform over the launch.  The two ends of the range are exact: omd == 0 touches no
// shadow at all, omd == 1 stores p' itself.
DWM_DEVINL float ema_update(float e, float p_new, float omd) { return omd == 1.f ? p_new : e + omd * (p_new - e); }

// the shadow pointer of a list item: null for the item types that have none
DWM_DEVINL float* item_ema(const dwm_adamw_item&) { return nullptr; }
DWM_DEVINL float* item_ema(const dwm_adamw8_item&) { return nullptr; }
DWM_DEVINL float* item_ema(const dwm_adamw_ema_item& it) { return it.ema; }
DWM_DEVINL float* item_ema(const dwm_adamw8_ema_item& it) { return it.ema; }

// Item = dwm_adamw_item (omd is not read) or dwm_adamw_ema_item: the shadow, where the item has one and omd != 0, is read after g, p,
// m, v and written after them - the parameter update is the same sequence in both instantiations.
template <typename Item>
DWM_DEVINL void adamw_multi_body(const Item* __restrict__ items, const int32_t* __restrict__ block_item,
                                 const int64_t* __restrict__ block_start, int64_t chunk, const AdamwHyper& h, float omd) {
    int64_t i0, i1;
    const Item it = dwm_list_chunk(items, block_item, block_start, chunk, i0, i1);
    float* __restrict__ p = it.p;
    const float* __restrict__ g = it.g;
    float* __restrict__ m = it.m;
    float* __restrict__ v = it.v;
    bf16_t* __restrict__ pb = (bf16_t*)it.p_bf16;
    float* __restrict__ ema = omd != 0.f ? item_ema(it) : nullptr;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const float gi = g[i], p0 = p[i];
        float mi = m[i], vi = v[i];
        const float e0 = ema ? ema[i] : 0.f;
        const float pi = adamw_update(p0, gi, mi, vi, h);
        p[i] = pi; m[i] = mi; v[i] = vi;
        if (pb) pb[i] = f32_to_bf16(pi);
        if (ema) ema[i] = ema_update(e0, pi, omd);
    }
}

__global__ void __launch_bounds__(256)
adamw_multi_kernel(const dwm_adamw_item* __restrict__ items, const int32_t* __restrict__ block_item,
                   const int64_t* __restrict__ block_start, int64_t chunk, float lr, float b1, float b2, float eps, float wd,
                   float bc1, float bc2, float gscale) {
    adamw_multi_body(items, block_item, block_start, chunk, AdamwHyper{lr, b1, b2, eps, wd, bc1, bc2, gscale}, 0.f);
}

__global__ void __launch_bounds__(256)
adamw_ema_multi_kernel(const dwm_adamw_ema_item* __restrict__ items, const int32_t* __restrict__ block_item,
                       const int64_t* __restrict__ block_start, int64_t chunk, float lr, float b1, float b2, float eps, float wd,
                       float bc1, float bc2, float gscale, float omd) {
    adamw_multi_body(items, block_item, block_start, chunk, AdamwHyper{lr, b1, b2, eps, wd, bc1, bc2, gscale}, omd);
}

// The per-step scalars from DEVICE memory (dwm_adamw_multi_dev / dwm_adamw8_multi_dev): hyper = [lr, bias_corr1, bias_corr2, _],
// cond = the out of dwm_grad_sumsq_multi [norm, coef, found, _] or null (coef 1, found 0).  Nobody on the host has to know the
// clip coefficient or the non-finite flag before the launch; a launch whose flag is set returns before its first store.  Every
// lane reads the same few floats (one scalar load each), then runs the body of the by-value kernel on the same values.
DWM_DEVINL bool adamw_dev_hyper(const float* __restrict__ hyper, const float* __restrict__ cond, float b1, float b2, float eps,
                                float wd, AdamwHyper& h) {
    if (cond && cond[2] != 0.f) return false;
    h = AdamwHyper{hyper[0], b1, b2, eps, wd, hyper[1], hyper[2], cond ? cond[1] : 1.f};
    return true;
}

__global__ void __launch_bounds__(256)
adamw_multi_dev_kernel(const dwm_adamw_item* __restrict__ items, const int32_t* __restrict__ block_item,
                       const int64_t* __restrict__ block_start, int64_t chunk, const float* __restrict__ hyper,
                       const float* __restrict__ cond, float b1, float b2, float eps, float wd) {
    AdamwHyper h;
    if (!adamw_dev_hyper(hyper, cond, b1, b2, eps, wd, h)) return;
    adamw_multi_body(items, block_item, block_start, chunk, h, 0.f);
}

// hyper[3] = omd (the slot dwm_adamw_multi_dev leaves unused)
__global__ void __launch_bounds__(256)
adamw_ema_multi_dev_kernel(const dwm_adamw_ema_item* __restrict__ items, const int32_t* __restrict__ block_item,
                           const int64_t* __restrict__ block_start, int64_t chunk, const float* __restrict__ hyper,
                           const float* __restrict__ cond, float b1, float b2, float eps, float wd) {
    AdamwHyper h;
    if (!adamw_dev_hyper(hyper, cond, b1, b2, eps, wd, h)) return;
    adamw_multi_body(items, block_item, block_start, chunk, h, hyper[3]);
}

// The average alone (dwm_ema_multi): parameters that have a shadow but no gradient in a step, and callers with an optimizer of their
// own.  hyper / cond as above, both optional.
__global__ void __launch_bounds__(256)
ema_multi_kernel(const dwm_ema_item* __restrict__ items, const int32_t* __restrict__ block_item,
                 const int64_t* __restrict__ block_start, int64_t chunk, float omd_value, const float* __restrict__ hyper,
                 const float* __restrict__ cond) {
    if (cond && cond[2] != 0.f) return;
    const float omd = hyper ? hyper[3] : omd_value;
    if (omd == 0.f) return;
    int64_t i0, i1;
    const dwm_ema_item it = dwm_list_chunk(items, block_item, block_start, chunk, i0, i1);
    float* __restrict__ ema = it.ema;
    const float* __restrict__ p = it.p;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) ema[i] = ema_update(ema[i], p[i], omd);
}

// p <-> ema element by element, the bf16 copy of the new p beside it (dwm_ema_swap_multi): a thread holds both values of its
// element before it stores either, so there is nothing to stage
__global__ void __launch_bounds__(256)
ema_swap_multi_kernel(const dwm_ema_swap_item* __restrict__ items, const int32_t* __restrict__ block_item,
                      const int64_t* __restrict__ block_start, int64_t chunk) {
    int64_t i0, i1;
    const dwm_ema_swap_item it = dwm_list_chunk(items, block_item, block_start, chunk, i0, i1);
    float* __restrict__ p = it.p;
    float* __restrict__ ema = it.ema;
    bf16_t* __restrict__ pb = (bf16_t*)it.p_bf16;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        const float a = p[i], b = ema[i];
        p[i] = b; ema[i] = a;
        if (pb) pb[i] = f32_to_bf16(b);
    }
}

// ---------------------------------------------------------------------------------- block-wise 8-bit optimizer state
// Format (include/dwm_hip.h, "Block-wise 8-bit optimizer state"): a value is code[q] * absmax[block], blocks of 256 consecutive
// elements of one tensor, `code` a table of 256 increasing floats handed in by the caller.  One wave owns one block: lane l holds
// elements 4 l .. 4 l + 3, so the four codes of a lane are one 32-bit word, fp32 data one 16-byte access, the bf16 shadow one
// 8-byte store, and the block maximum is a cross-lane reduction of the wave (no LDS barrier, no atomics).  The tables and their
// 255 midpoints sit in LDS: decoding is one gather, encoding an 8-step search over the midpoints.
constexpr int Q8_BLOCK = 256;

// table t -> LDS: tab[0..255] = code, tab[256..510] = midpoints of adjacent entries (tab[511] is never read).  All 256 threads.
DWM_DEVINL void q8_stage_table(const float* __restrict__ code, float* tab) {
    const int t = threadIdx.x;
    tab[t] = code[t];
    tab[256 + t] = t < 255 ? (code[t] + code[t + 1]) * 0.5f : 0.f;
}

// number of midpoints strictly below y (ties go down); a NaN gives 0
DWM_DEVINL uint32_t q8_encode(const float* tab, float y) {
    const float* mid = tab + 256;
    uint32_t c = 0;
#pragma unroll
    for (uint32_t s = 128; s > 0; s >>= 1) c += mid[c + s - 1] < y ? s : 0u;
    return c;
}

DWM_DEVINL float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// The four values of a lane -> four codes in one word.  y = x / absmax is a true division; a block of zeros gets the code of 0.
// floor_positive (the second moment): a strictly positive value never receives the zero code but the smallest positive entry.
// Without it an element whose gradient is tiny next to the largest of its block would lose v while keeping m, and take a step
// of lr * m / eps the next time its gradient is exactly zero.
DWM_DEVINL uint32_t q8_encode4(const float* tab, const float* x, float absmax, uint32_t zero_code, bool floor_positive) {
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t c = q8_encode(tab, absmax > 0.f ? x[j] / absmax : 0.f);
        if (floor_positive && x[j] > 0.f && c == zero_code) c = zero_code + 1;
        w |= c << (8 * j);
    }
    return w;
}

// elements e .. e + 3 of an n-element tensor: `full` (the whole block inside the tensor, pointers aligned) = one vector access,
// otherwise element by element with the tail masked (loads give `fill`)
DWM_DEVINL void q8_load4f(const float* __restrict__ src, int64_t e, int64_t n, bool full, float* f) {
    if (full) {
        const float4 a = *(const float4*)(src + e);
        f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = e + j < n ? src[e + j] : 0.f;
    }
}
DWM_DEVINL void q8_store4f(float* __restrict__ dst, int64_t e, int64_t n, bool full, const float* f) {
    if (full) {
        *(float4*)(dst + e) = make_float4(f[0], f[1], f[2], f[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (e + j < n) dst[e + j] = f[j];
    }
}
DWM_DEVINL uint32_t q8_load4c(const uint8_t* __restrict__ q, int64_t e, int64_t n, bool full, uint32_t fill) {
    if (full) return *(const uint32_t*)(q + e);
    uint32_t w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) w |= (e + j < n ? (uint32_t)q[e + j] : fill) << (8 * j);
    return w;
}
DWM_DEVINL void q8_store4c(uint8_t* __restrict__ q, int64_t e, int64_t n, bool full, uint32_t w) {
    if (full) {
        *(uint32_t*)(q + e) = w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (e + j < n) q[e + j] = (uint8_t)(w >> (8 * j));
    }
}
DWM_DEVINL bool q8_aligned(const void* p, uintptr_t bytes) { return (((uintptr_t)p) & (bytes - 1)) == 0; }

__global__ void __launch_bounds__(256)
quantize_blockwise8_kernel(const float* __restrict__ x, int64_t n, const float* __restrict__ code, int floor_positive,
                           uint8_t* __restrict__ q, float* __restrict__ absmax) {
    __shared__ float tab[512];
    q8_stage_table(code, tab);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t zc = q8_encode(tab, 0.f);
    const bool vec = q8_aligned(x, 16) && q8_aligned(q, 4);
    const int64_t nblk = (n + Q8_BLOCK - 1) / Q8_BLOCK;
    for (int64_t blk = (int64_t)blockIdx.x * 4 + wave; blk < nblk; blk += (int64_t)gridDim.x * 4) {
        const int64_t b0 = blk * Q8_BLOCK, e = b0 + lane * 4;
        const bool full = vec && b0 + Q8_BLOCK <= n;
        float f[4];
        q8_load4f(x, e, n, full, f);
        const float am = wave_max(fmaxf(fmaxf(fabsf(f[0]), fabsf(f[1])), fmaxf(fabsf(f[2]), fabsf(f[3]))));
        q8_store4c(q, e, n, full, q8_encode4(tab, f, am, zc, floor_positive != 0));
        if (lane == 0) absmax[blk] = am;
    }
}

__global__ void __launch_bounds__(256)
dequantize_blockwise8_kernel(const uint8_t* __restrict__ q, const float* __restrict__ absmax, int64_t n,
                             const float* __restrict__ code, float* __restrict__ x) {
    __shared__ float tab[256];
    tab[threadIdx.x] = code[threadIdx.x];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool vec = q8_aligned(x, 16) && q8_aligned(q, 4);
    const int64_t nblk = (n + Q8_BLOCK - 1) / Q8_BLOCK;
    for (int64_t blk = (int64_t)blockIdx.x * 4 + wave; blk < nblk; blk += (int64_t)gridDim.x * 4) {
        const int64_t b0 = blk * Q8_BLOCK, e = b0 + lane * 4;
        const bool full = vec && b0 + Q8_BLOCK <= n;
        const uint32_t w = q8_load4c(q, e, n, full, 0u);
        const float s = absmax[blk];
        float f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) f[j] = tab[(w >> (8 * j)) & 255u] * s;
        q8_store4f(x, e, n, full, f);
    }
}

// adamw_multi_kernel with both moments in the 8-bit format: decode, the same update, re-encode, in one pass (18 bytes per
// parameter instead of 30).  The parameter update uses the fresh fp32 moments; quantisation only affects what the next step
// starts from.  Wave w of a workgroup takes blocks w, w + 4, ... of the workgroup's chunk (a multiple of 256 elements).
// Item = dwm_adamw8_item or dwm_adamw8_ema_item (the shadow, where the item has one and omd != 0, is moved behind the update of its
// block; it takes the vector access where the rest of the block does and the shadow itself is 16-byte aligned).
template <typename Item>
DWM_DEVINL void adamw8_multi_body(const Item* __restrict__ items, const int32_t* __restrict__ block_item,
                                  const int64_t* __restrict__ block_start, int64_t chunk, const float* __restrict__ code_m,
                                  const float* __restrict__ code_v, const AdamwHyper& h, float omd) {
    __shared__ float tab_m[512], tab_v[512];
    q8_stage_table(code_m, tab_m);
    q8_stage_table(code_v, tab_v);
    __syncthreads();
    int64_t i0, i1;
    const Item it = dwm_list_chunk(items, block_item, block_start, chunk, i0, i1);
    float* __restrict__ ema = omd != 0.f ? item_ema(it) : nullptr;
    const bool vec_e = q8_aligned(ema, 16);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* __restrict__ p = it.p;
    const float* __restrict__ g = it.g;
    uint8_t* __restrict__ mq = it.m_q;
    uint8_t* __restrict__ vq = it.v_q;
    bf16_t* __restrict__ pb = (bf16_t*)it.p_bf16;
    const uint32_t zm = q8_encode(tab_m, 0.f), zv = q8_encode(tab_v, 0.f);
    const bool vec = q8_aligned(p, 16) && q8_aligned(g, 16) && q8_aligned(mq, 4) && q8_aligned(vq, 4) && q8_aligned(pb, 8);
    for (int64_t b0 = i0 + wave * Q8_BLOCK; b0 < i1; b0 += 4 * Q8_BLOCK) {
        const int64_t e = b0 + lane * 4, blk = b0 / Q8_BLOCK;
        const bool full = vec && b0 + Q8_BLOCK <= it.n;
        float pi[4], gi[4], mi[4], vi[4];
        q8_load4f(p, e, it.n, full, pi);
        q8_load4f(g, e, it.n, full, gi);
        const uint32_t wm = q8_load4c(mq, e, it.n, full, zm), wv = q8_load4c(vq, e, it.n, full, zv);
        const float sm = it.m_absmax[blk], sv = it.v_absmax[blk];
        float am = 0.f, av = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            mi[j] = tab_m[(wm >> (8 * j)) & 255u] * sm;
            vi[j] = tab_v[(wv >> (8 * j)) & 255u] * sv;
            pi[j] = adamw_update(pi[j], gi[j], mi[j], vi[j], h);
            am = fmaxf(am, fabsf(mi[j]));
            av = fmaxf(av, vi[j]);
        }
        am = wave_max(am);
        av = wave_max(av);
        q8_store4f(p, e, it.n, full, pi);
        if (pb) {
            if (full) {
                *(uint2*)(pb + e) = pack4(pi);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) if (e + j < it.n) pb[e + j] = f32_to_bf16(pi[j]);
            }
        }
        q8_store4c(mq, e, it.n, full, q8_encode4(tab_m, mi, am, zm, false));
        q8_store4c(vq, e, it.n, full, q8_encode4(tab_v, vi, av, zv, true));
        if (lane == 0) { it.m_absmax[blk] = am; it.v_absmax[blk] = av; }
        if (ema) {
            // The average is a pass of its own behind the update of the block: it reads back the p' this lane has just stored (a
            // cache hit) rather than using the registers.  Any further use of the update's values changes how the compiler packs
            // and contracts the update itself (seen: the last bit of m), and p, m, v must be the plain kernel's bits.
            __asm__ volatile("" ::: "memory");
            float pn[4], ei[4];
            q8_load4f(p, e, it.n, full, pn);
            q8_load4f(ema, e, it.n, full && vec_e, ei);
#pragma unroll
            for (int j = 0; j < 4; ++j) ei[j] = ema_update(ei[j], pn[j], omd);
            q8_store4f(ema, e, it.n, full && vec_e, ei);
        }
    }
}

__global__ void __launch_bounds__(256)
adamw8_multi_kernel(const dwm_adamw8_item* __restrict__ items, const int32_t* __restrict__ block_item,
                    const int64_t* __restrict__ block_start, int64_t chunk, const float* __restrict__ code_m,
                    const float* __restrict__ code_v, float lr, float b1, float b2, float eps, float wd,
                    float bc1, float bc2, float gscale) {
    adamw8_multi_body(items, block_item, block_start, chunk, code_m, code_v, AdamwHyper{lr, b1, b2, eps, wd, bc1, bc2, gscale}, 0.f);
}

__global__ void __launch_bounds__(256)
adamw8_ema_multi_kernel(const dwm_adamw8_ema_item* __restrict__ items, const int32_t* __restrict__ block_item,
                        const int64_t* __restrict__ block_start, int64_t chunk, const float* __restrict__ code_m,
                        const float* __restrict__ code_v, float lr, float b1, float b2, float eps, float wd,
                        float bc1, float bc2, float gscale, float omd) {
    adamw8_multi_body(items, block_item, block_start, chunk, code_m, code_v, AdamwHyper{lr, b1, b2, eps, wd, bc1, bc2, gscale}, omd);
}

// (the flag is uniform over the launch: every thread of a skipped launch leaves before the first barrier of the body)
__global__ void __launch_bounds__(256)
adamw8_multi_dev_kernel(const dwm_adamw8_item* __restrict__ items, const int32_t* __restrict__ block_item,
                        const int64_t* __restrict__ block_start, int64_t chunk, const float* __restrict__ code_m,
                        const float* __restrict__ code_v, const float* __restrict__ hyper, const float* __restrict__ cond,
                        float b1, float b2, float eps, float wd) {
    AdamwHyper h;
    if (!adamw_dev_hyper(hyper, cond, b1, b2, eps, wd, h)) return;
    adamw8_multi_body(items, block_item, block_start, chunk, code_m, code_v, h, 0.f);
}

__global__ void __launch_bounds__(256)
adamw8_ema_multi_dev_kernel(const dwm_adamw8_ema_item* __restrict__ items, const int32_t* __restrict__ block_item,
                            const int64_t* __restrict__ block_start, int64_t chunk, const float* __restrict__ code_m,
                            const float* __restrict__ code_v, const float* __restrict__ hyper, const float* __restrict__ cond,
                            float b1, float b2, float eps, float wd) {
    AdamwHyper h;
    if (!adamw_dev_hyper(hyper, cond, b1, b2, eps, wd, h)) return;
    adamw8_multi_body(items, block_item, block_start, chunk, code_m, code_v, h, hyper[3]);
}

__global__ void __launch_bounds__(256)
cast_bf16_to_f32_kernel(const bf16_t* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy,
                        int64_t rows, int64_t cols, int accumulate) {
    const int64_t total = rows * cols;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols, c = i - r * cols;
        const float v = bf16_to_f32(x[r * ldx + c]);
        float* d = y + r * ldy + c;
        *d = accumulate ? *d + v : v;
    }
}

// the same, 8 elements per thread (cols % 8 == 0, 16-byte aligned rows): the entry of the fp32 residual stream (132 M elements)
__global__ void __launch_bounds__(256)
cast_bf16_to_f32_vec_kernel(const bf16_t* __restrict__ x, int64_t ldx, float* __restrict__ y, int64_t ldy,
                            int64_t rows, int64_t cols8, int accumulate) {
    const int64_t total = rows * cols8;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols8, c = (i - r * cols8) * 8;
        float v[8];
        unpack8(*(const uint4*)(x + r * ldx + c), v);
        float* d = y + r * ldy + c;
        if (accumulate) {
            const float4 a = *(const float4*)d, b = *(const float4*)(d + 4);
            v[0] += a.x; v[1] += a.y; v[2] += a.z; v[3] += a.w; v[4] += b.x; v[5] += b.y; v[6] += b.z; v[7] += b.w;
        }
        *(float4*)d = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(d + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
}

inline unsigned grid_for(int64_t work_items) {
    int64_t b = (work_items + 255) / 256;
    if (b < 1) b = 1;
    if (b > 256 * 32) b = 256 * 32;
    return (unsigned)b;
}

}  // namespace


extern "C" int dwm_transpose_bf16(const void* in, int64_t ld_in, int64_t rows, int64_t cols, void* out,
                                  int64_t ld_out, int64_t rows_pad, void* stream) {
    if (!in || !out || rows <= 0 || cols <= 0 || rows_pad < rows || ld_in < cols || ld_out < rows_pad) return DWM_EINVAL;
    if (cols % 8 == 0 && rows_pad % 8 == 0 && ld_in % 8 == 0 && ld_out % 8 == 0 && dwm_aligned16(in) && dwm_aligned16(out)) {
        const dim3 grid8((unsigned)((cols + 127) / 128), (unsigned)((rows_pad + 127) / 128));
        hipLaunchKernelGGL(transpose8_kernel, grid8, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)in, ld_in, rows, cols,
                           (bf16_t*)out, ld_out, rows_pad);
        return dwm_launch_status();
    }
    const dim3 grid((unsigned)((cols + 63) / 64), (unsigned)((rows_pad + 63) / 64));
    hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)in, ld_in, rows, cols,
                       (bf16_t*)out, ld_out, rows_pad);
    return dwm_launch_status();
}

extern "C" int dwm_segsum(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t rows, int64_t ncols,
                          int64_t rows_per_group, float* out, int64_t ld_out, void* stream) {
    if (!a || !out || rows <= 0 || ncols <= 0 || ncols % 8 != 0 || rows_per_group <= 0) return DWM_EINVAL;
    if (lda % 8 != 0 || (b && ldb % 8 != 0) || !dwm_aligned16(a) || (b && !dwm_aligned16(b))) return DWM_EALIGN;
    const int64_t groups = (rows + rows_per_group - 1) / rows_per_group;
    const int64_t rpg = rows_per_group < rows ? rows_per_group : rows;
    const int cpg = (int)((rpg + SEG_RB - 1) / SEG_RB);
    if (groups * cpg >= 65536 * 16) return DWM_EUNSUPPORTED;
    const dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)(groups * cpg));
    hipLaunchKernelGGL(segsum_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a, lda, (const bf16_t*)b, ldb,
                       (const bf16_t*)nullptr, (int64_t)0, rows, ncols, rows_per_group, cpg, out, ld_out, (float*)nullptr);
    return dwm_launch_status();
}

extern "C" int dwm_segsum_diff(const void* a, int64_t lda, const void* b, int64_t ldb, const void* b2, int64_t ldb2, int64_t rows,
                               int64_t ncols, int64_t rows_per_group, float* out, int64_t ld_out, void* stream) {
    if (!a || !b || !b2 || !out || rows <= 0 || ncols <= 0 || ncols % 8 != 0 || rows_per_group <= 0) return DWM_EINVAL;
    if (lda % 8 != 0 || ldb % 8 != 0 || ldb2 % 8 != 0 || !dwm_aligned16(a) || !dwm_aligned16(b) || !dwm_aligned16(b2)) return DWM_EALIGN;
    const int64_t groups = (rows + rows_per_group - 1) / rows_per_group;
    const int64_t rpg = rows_per_group < rows ? rows_per_group : rows;
    const int cpg = (int)((rpg + SEG_RB - 1) / SEG_RB);
    if (groups * cpg >= 65536 * 16) return DWM_EUNSUPPORTED;
    const dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)(groups * cpg));
    hipLaunchKernelGGL(segsum_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a, lda, (const bf16_t*)b, ldb,
                       (const bf16_t*)b2, ldb2, rows, ncols, rows_per_group, cpg, out, ld_out, (float*)nullptr);
    return dwm_launch_status();
}

// ---- stage 2 of every ordered reduction, also called from vae.hip (declared in common.h)
void dwm_ordered_finish(const DwmFoldArgs& f, hipStream_t stream) {
    const dim3 grid((unsigned)((f.ncols / 4 + 63) / 64), (unsigned)f.groups, (unsigned)f.nslots);
    hipLaunchKernelGGL(ordered_finish_kernel, grid, dim3(64), 0, stream, f);
}

// ---- ordered forms of the two segmented sums: stage 1 = segsum_kernel<true> into the workspace, stage 2 = dwm_ordered_finish
extern "C" int64_t dwm_segsum_ordered_floats(int64_t rows, int64_t ncols, int64_t rows_per_group) {
    if (rows <= 0 || ncols <= 0 || rows_per_group <= 0) return 0;
    const int64_t groups = (rows + rows_per_group - 1) / rows_per_group;
    const int64_t rpg = rows_per_group < rows ? rows_per_group : rows;
    return groups * ((rpg + SEG_RB - 1) / SEG_RB) * ncols;
}
extern "C" int64_t dwm_segsum_diff_ordered_floats(int64_t rows, int64_t ncols, int64_t rows_per_group) {
    return dwm_segsum_ordered_floats(rows, ncols, rows_per_group);
}

static int segsum_ordered_launch(const void* a, int64_t lda, const void* b, int64_t ldb, const void* b2, int64_t ldb2, int64_t rows,
                                 int64_t ncols, int64_t rows_per_group, float* out, int64_t ld_out, float* workspace,
                                 int64_t workspace_floats, void* stream) {
    if (!workspace || workspace_floats < dwm_segsum_ordered_floats(rows, ncols, rows_per_group)) return DWM_EINVAL;
    if (!dwm_aligned16(workspace)) return DWM_EALIGN;
    const int64_t groups = (rows + rows_per_group - 1) / rows_per_group;
    const int64_t rpg = rows_per_group < rows ? rows_per_group : rows;
    const int cpg = (int)((rpg + SEG_RB - 1) / SEG_RB);
    if (groups * cpg >= 65536 * 16 || groups >= 65536) return DWM_EUNSUPPORTED;
    const dim3 grid((unsigned)((ncols + 255) / 256), (unsigned)(groups * cpg));
    hipLaunchKernelGGL(segsum_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a, lda, (const bf16_t*)b, ldb,
                       (const bf16_t*)b2, ldb2, rows, ncols, rows_per_group, cpg, out, ld_out, workspace);
    DwmFoldArgs f = {};
    f.ws[0] = workspace; f.out[0] = out; f.nslots = 1;
    f.nfold = cpg; f.fold_stride = ncols; f.group_stride = (int64_t)cpg * ncols; f.groups = groups; f.ncols = ncols; f.ld_out = ld_out;
    dwm_ordered_finish(f, (hipStream_t)stream);
    return dwm_launch_status();
}

extern "C" int dwm_segsum_ordered(const void* a, int64_t lda, const void* b, int64_t ldb, int64_t rows, int64_t ncols,
                                  int64_t rows_per_group, float* out, int64_t ld_out, float* workspace, int64_t workspace_floats,
                                  void* stream) {
    if (!a || !out || rows <= 0 || ncols <= 0 || ncols % 8 != 0 || rows_per_group <= 0) return DWM_EINVAL;
    if (lda % 8 != 0 || (b && ldb % 8 != 0) || !dwm_aligned16(a) || (b && !dwm_aligned16(b))) return DWM_EALIGN;
    return segsum_ordered_launch(a, lda, b, ldb, nullptr, 0, rows, ncols, rows_per_group, out, ld_out, workspace, workspace_floats, stream);
}

extern "C" int dwm_segsum_diff_ordered(const void* a, int64_t lda, const void* b, int64_t ldb, const void* b2, int64_t ldb2,
                                       int64_t rows, int64_t ncols, int64_t rows_per_group, float* out, int64_t ld_out,
                                       float* workspace, int64_t workspace_floats, void* stream) {
    if (!a || !b || !b2 || !out || rows <= 0 || ncols <= 0 || ncols % 8 != 0 || rows_per_group <= 0) return DWM_EINVAL;
    if (lda % 8 != 0 || ldb % 8 != 0 || ldb2 % 8 != 0 || !dwm_aligned16(a) || !dwm_aligned16(b) || !dwm_aligned16(b2)) return DWM_EALIGN;
    return segsum_ordered_launch(a, lda, b, ldb, b2, ldb2, rows, ncols, rows_per_group, out, ld_out, workspace, workspace_floats, stream);
}

extern "C" int dwm_act_fwd(const void* x, void* y, int64_t n, int32_t act, void* stream) {
    if (!x || !y || n <= 0 || n % 8 != 0) return DWM_EINVAL;
    if (!dwm_aligned16(x) || !dwm_aligned16(y)) return DWM_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (act == DWM_ACT_GELU_TANH) hipLaunchKernelGGL((act_kernel<DWM_ACT_GELU_TANH, false>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, nullptr, (bf16_t*)y, n / 8);
    else if (act == DWM_ACT_SILU) hipLaunchKernelGGL((act_kernel<DWM_ACT_SILU, false>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, nullptr, (bf16_t*)y, n / 8);
    else if (act == DWM_ACT_RELU) hipLaunchKernelGGL((act_kernel<DWM_ACT_RELU, false>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, nullptr, (bf16_t*)y, n / 8);
    else return DWM_EINVAL;
    return dwm_launch_status();
}

extern "C" int dwm_act_bwd(const void* x, const void* dy, void* dx, int64_t n, int32_t act, void* stream) {
    if (!x || !dy || !dx || n <= 0 || n % 8 != 0) return DWM_EINVAL;
    if (!dwm_aligned16(x) || !dwm_aligned16(dy) || !dwm_aligned16(dx)) return DWM_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (act == DWM_ACT_GELU_TANH) hipLaunchKernelGGL((act_kernel<DWM_ACT_GELU_TANH, true>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)dx, n / 8);
    else if (act == DWM_ACT_SILU) hipLaunchKernelGGL((act_kernel<DWM_ACT_SILU, true>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)dx, n / 8);
    else if (act == DWM_ACT_RELU) hipLaunchKernelGGL((act_kernel<DWM_ACT_RELU, true>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)dx, n / 8);
    else return DWM_EINVAL;
    return dwm_launch_status();
}

extern "C" int dwm_act_bwd_recompute(const void* x, const void* dy, void* y_out, void* dx, int64_t n, int32_t act, void* stream) {
    if (!x || !dy || !y_out || !dx || n <= 0 || n % 8 != 0) return DWM_EINVAL;
    if (!dwm_aligned16(x) || !dwm_aligned16(dy) || !dwm_aligned16(y_out) || !dwm_aligned16(dx)) return DWM_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    if (act == DWM_ACT_GELU_TANH) hipLaunchKernelGGL((act_bwd_recompute_kernel<DWM_ACT_GELU_TANH>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)y_out, (bf16_t*)dx, n / 8);
    else if (act == DWM_ACT_SILU) hipLaunchKernelGGL((act_bwd_recompute_kernel<DWM_ACT_SILU>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)y_out, (bf16_t*)dx, n / 8);
    else if (act == DWM_ACT_RELU) hipLaunchKernelGGL((act_bwd_recompute_kernel<DWM_ACT_RELU>), dim3(grid_for(n / 8)), dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)dy, (bf16_t*)y_out, (bf16_t*)dx, n / 8);
    else return DWM_EINVAL;
    return dwm_launch_status();
}

extern "C" int dwm_geglu_fwd(const void* u, int64_t ldu, int64_t rows, int64_t inner, void* g, int64_t ldg, void* stream) {
    if (!u || !g || rows <= 0 || inner <= 0 || inner % 8 != 0 || ldu < 2 * inner || ldg < inner) return DWM_EINVAL;
    if (ldu % 8 != 0 || ldg % 8 != 0 || !dwm_aligned16(u) || !dwm_aligned16(g)) return DWM_EALIGN;
    hipLaunchKernelGGL((geglu_kernel<false>), dim3(grid_for(rows * inner / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)u, ldu, nullptr, 0, (bf16_t*)g, ldg, rows, inner);
    return dwm_launch_status();
}

extern "C" int dwm_geglu_bwd(const void* u, int64_t ldu, const void* dg, int64_t lddg, int64_t rows, int64_t inner,
                             void* du, int64_t lddu, void* stream) {
    if (!u || !dg || !du || rows <= 0 || inner <= 0 || inner % 8 != 0 || ldu < 2 * inner || lddg < inner || lddu < 2 * inner) return DWM_EINVAL;
    if (ldu % 8 != 0 || lddg % 8 != 0 || lddu % 8 != 0 || !dwm_aligned16(u) || !dwm_aligned16(dg) || !dwm_aligned16(du)) return DWM_EALIGN;
    hipLaunchKernelGGL((geglu_kernel<true>), dim3(grid_for(rows * inner / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)u, ldu, (const bf16_t*)dg, lddg, (bf16_t*)du, lddu, rows, inner);
    return dwm_launch_status();
}

extern "C" int dwm_geglu_bwd_recompute(const void* u, int64_t ldu, const void* dg, int64_t lddg, int64_t rows, int64_t inner,
                                       void* g_out, int64_t ldg, void* du, int64_t lddu, void* stream) {
    if (!u || !dg || !g_out || !du || rows <= 0 || inner <= 0 || inner % 8 != 0 || ldu < 2 * inner || lddg < inner || ldg < inner ||
        lddu < 2 * inner) return DWM_EINVAL;
    if (ldu % 8 != 0 || lddg % 8 != 0 || ldg % 8 != 0 || lddu % 8 != 0 || !dwm_aligned16(u) || !dwm_aligned16(dg) ||
        !dwm_aligned16(g_out) || !dwm_aligned16(du)) return DWM_EALIGN;
    hipLaunchKernelGGL(geglu_bwd_recompute_kernel, dim3(grid_for(rows * inner / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)u, ldu, (const bf16_t*)dg, lddg, (bf16_t*)g_out, ldg, (bf16_t*)du, lddu, rows, inner);
    return dwm_launch_status();
}

extern "C" int dwm_rowcombine(const dwm_rowcombine_args* a, void* stream) {
    if (!a || !a->a || !a->out || a->rows <= 0 || a->ncols <= 0 || a->ncols % 8 != 0) return DWM_EINVAL;
    if (a->lda % 8 != 0 || a->ldo % 8 != 0 || (a->b && a->ldb % 8 != 0) || (a->gate_a && a->ld_gate_a % 8 != 0)) return DWM_EALIGN;
    if (!dwm_aligned16(a->a) || !dwm_aligned16(a->out) || (a->b && !dwm_aligned16(a->b)) || (a->gate_a && !dwm_aligned16(a->gate_a))) return DWM_EALIGN;
    if ((a->gate_a && a->rows_per_gate_a <= 0) || (a->coef_a && a->rows_per_coef_a <= 0) || (a->coef_b && a->rows_per_coef_b <= 0)) return DWM_EINVAL;
    hipLaunchKernelGGL(rowcombine_kernel, dim3(grid_for(a->rows * a->ncols / 8)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)a->a, a->lda, (const bf16_t*)a->gate_a, a->ld_gate_a, a->rows_per_gate_a,
                       a->coef_a, a->rows_per_coef_a, (const bf16_t*)a->b, a->ldb, a->coef_b, a->rows_per_coef_b,
                       (bf16_t*)a->out, a->ldo, a->rows, a->ncols);
    return dwm_launch_status();
}

extern "C" int dwm_layernorm_bwd(const dwm_layernorm_bwd_args* a, void* stream) {
    if (!a || !a->x || !a->dy || !a->dx || a->rows <= 0 || a->D <= 0 || a->D % 8 != 0 || a->D > 2048) return DWM_EINVAL;
    if (a->ldx % 8 != 0 || a->lddy % 8 != 0 || a->lddx % 8 != 0 || (a->dy2 && a->lddy2 % 8 != 0)) return DWM_EALIGN;
    if ((a->scale || a->scale2) && (a->rows_per_mod <= 0 || a->ld_mod % 8 != 0)) return DWM_EINVAL;
    if (a->addvec && (a->rows_per_add <= 0 || a->ld_add % 8 != 0)) return DWM_EINVAL;
    if ((a->dgamma || a->dbeta || a->dgamma2 || a->dbeta2) && a->ld_grad < a->D) return DWM_EINVAL;
    const int64_t rpg = a->rows_per_mod > 0 ? a->rows_per_mod : a->rows;
    const int64_t groups = (a->rows + rpg - 1) / rpg;
    const int cpg = (int)(((rpg < a->rows ? rpg : a->rows) + LN_BWD_RB - 1) / LN_BWD_RB);
    if (groups * cpg >= (1ll << 31)) return DWM_EUNSUPPORTED;
    const dim3 grid((unsigned)(groups * cpg));
    hipStream_t s = (hipStream_t)stream;
    const int ni = (a->D + 511) / 512;
    switch (ni) {
        case 1: hipLaunchKernelGGL((layernorm_bwd_kernel<1, false>), grid, dim3(256), 0, s, *a, cpg, (float*)nullptr); break;
        case 2: hipLaunchKernelGGL((layernorm_bwd_kernel<2, false>), grid, dim3(256), 0, s, *a, cpg, (float*)nullptr); break;
        case 3: hipLaunchKernelGGL((layernorm_bwd_kernel<3, false>), grid, dim3(256), 0, s, *a, cpg, (float*)nullptr); break;
        default: hipLaunchKernelGGL((layernorm_bwd_kernel<4, false>), grid, dim3(256), 0, s, *a, cpg, (float*)nullptr); break;
    }
    return dwm_launch_status();
}

static int ln_bwd_slots(const dwm_layernorm_bwd_args* a) {
    return (a->dgamma != nullptr) + (a->dbeta != nullptr) + (a->dgamma2 != nullptr) + (a->dbeta2 != nullptr);
}

extern "C" int64_t dwm_layernorm_bwd_ordered_floats(const dwm_layernorm_bwd_args* a) {
    if (!a || a->rows <= 0 || a->D <= 0) return 0;
    const int64_t rpg = a->rows_per_mod > 0 ? a->rows_per_mod : a->rows;
    const int64_t groups = (a->rows + rpg - 1) / rpg;
    const int64_t cpg = ((rpg < a->rows ? rpg : a->rows) + LN_BWD_RB - 1) / LN_BWD_RB;
    return ln_bwd_slots(a) * groups * cpg * a->D;
}

extern "C" int dwm_layernorm_bwd_ordered(const dwm_layernorm_bwd_args* a, float* workspace, int64_t workspace_floats, void* stream) {
    if (!a || !a->x || !a->dy || !a->dx || a->rows <= 0 || a->D <= 0 || a->D % 8 != 0 || a->D > 2048) return DWM_EINVAL;
    if (a->ldx % 8 != 0 || a->lddy % 8 != 0 || a->lddx % 8 != 0 || (a->dy2 && a->lddy2 % 8 != 0)) return DWM_EALIGN;
    if ((a->scale || a->scale2) && (a->rows_per_mod <= 0 || a->ld_mod % 8 != 0)) return DWM_EINVAL;
    if (a->addvec && (a->rows_per_add <= 0 || a->ld_add % 8 != 0)) return DWM_EINVAL;
    if ((a->dgamma || a->dbeta || a->dgamma2 || a->dbeta2) && a->ld_grad < a->D) return DWM_EINVAL;
    const int nslots = ln_bwd_slots(a);
    if (nslots > 0 && (!workspace || workspace_floats < dwm_layernorm_bwd_ordered_floats(a))) return DWM_EINVAL;
    if (nslots > 0 && !dwm_aligned16(workspace)) return DWM_EALIGN;
    const int64_t rpg = a->rows_per_mod > 0 ? a->rows_per_mod : a->rows;
    const int64_t groups = (a->rows + rpg - 1) / rpg;
    const int cpg = (int)(((rpg < a->rows ? rpg : a->rows) + LN_BWD_RB - 1) / LN_BWD_RB);
    if (groups * cpg >= (1ll << 31) || (a->grad_per_group && groups >= 65536)) return DWM_EUNSUPPORTED;
    const dim3 grid((unsigned)(groups * cpg));
    hipStream_t s = (hipStream_t)stream;
    const int ni = (a->D + 511) / 512;
    switch (ni) {
        case 1: hipLaunchKernelGGL((layernorm_bwd_kernel<1, true>), grid, dim3(256), 0, s, *a, cpg, workspace); break;
        case 2: hipLaunchKernelGGL((layernorm_bwd_kernel<2, true>), grid, dim3(256), 0, s, *a, cpg, workspace); break;
        case 3: hipLaunchKernelGGL((layernorm_bwd_kernel<3, true>), grid, dim3(256), 0, s, *a, cpg, workspace); break;
        default: hipLaunchKernelGGL((layernorm_bwd_kernel<4, true>), grid, dim3(256), 0, s, *a, cpg, workspace); break;
    }
    if (nslots > 0) {
        DwmFoldArgs f = {};
        float* const outs[4] = {a->dgamma, a->dbeta, a->dgamma2, a->dbeta2};
        for (int q = 0; q < 4; ++q)
            if (outs[q]) { f.ws[f.nslots] = workspace + (int64_t)f.nslots * groups * cpg * a->D; f.out[f.nslots++] = outs[q]; }
        f.fold_stride = a->D; f.ncols = a->D; f.ld_out = a->ld_grad;
        if (a->grad_per_group) { f.nfold = cpg; f.group_stride = (int64_t)cpg * a->D; f.groups = groups; }
        else { f.nfold = groups * cpg; f.group_stride = 0; f.groups = 1; }
        dwm_ordered_finish(f, s);
    }
    return dwm_launch_status();
}

extern "C" int dwm_rmsnorm_heads_train(void* x, int64_t ldx, int64_t rows, int64_t ncols, const void* w, float eps,
                                       float* rinv, void* stream) {
    if (!x || !w || rows <= 0 || ncols <= 0 || ncols % 64 != 0 || ldx % 8 != 0) return DWM_EINVAL;
    if (!dwm_aligned16(x) || !dwm_aligned16(w)) return DWM_EALIGN;
    hipLaunchKernelGGL(rmsnorm_heads_train_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (bf16_t*)x, ldx, rows, ncols, (const bf16_t*)w, eps, rinv);
    return dwm_launch_status();
}

extern "C" int dwm_rmsnorm_heads_bwd(const void* y, int64_t ldy, const float* rinv, const void* w, void* dy, int64_t lddy,
                                     int64_t rows, int64_t ncols, float* dw, void* stream) {
    if (!y || !rinv || !w || !dy || !dw || rows <= 0 || ncols <= 0 || ncols % 64 != 0 || ncols > 8192) return DWM_EINVAL;
    if (ldy % 8 != 0 || lddy % 8 != 0 || !dwm_aligned16(y) || !dwm_aligned16(dy) || !dwm_aligned16(w)) return DWM_EALIGN;
    hipLaunchKernelGGL(rmsnorm_heads_bwd_kernel<false>, dim3((unsigned)((rows + 31) / 32)), dim3(256), (size_t)ncols * sizeof(float),
                       (hipStream_t)stream, (const bf16_t*)y, ldy, rinv, (const bf16_t*)w, (bf16_t*)dy, lddy, rows, ncols, dw,
                       (float*)nullptr);
    return dwm_launch_status();
}

extern "C" int64_t dwm_rmsnorm_heads_bwd_ordered_floats(int64_t rows, int64_t ncols) {
    return rows <= 0 || ncols <= 0 ? 0 : (rows + 31) / 32 * ncols;
}

extern "C" int dwm_rmsnorm_heads_bwd_ordered(const void* y, int64_t ldy, const float* rinv, const void* w, void* dy, int64_t lddy,
                                             int64_t rows, int64_t ncols, float* dw, float* workspace, int64_t workspace_floats,
                                             void* stream) {
    if (!y || !rinv || !w || !dy || !dw || rows <= 0 || ncols <= 0 || ncols % 64 != 0 || ncols > 8192) return DWM_EINVAL;
    if (ldy % 8 != 0 || lddy % 8 != 0 || !dwm_aligned16(y) || !dwm_aligned16(dy) || !dwm_aligned16(w)) return DWM_EALIGN;
    if (!workspace || workspace_floats < dwm_rmsnorm_heads_bwd_ordered_floats(rows, ncols)) return DWM_EINVAL;
    if (!dwm_aligned16(workspace)) return DWM_EALIGN;
    const int64_t blocks = (rows + 31) / 32;
    const size_t lds = 4 * (size_t)(ncols > RMS_ORD_TILE ? RMS_ORD_TILE : ncols) * sizeof(float);
    hipLaunchKernelGGL(rmsnorm_heads_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, (const bf16_t*)y,
                       ldy, rinv, (const bf16_t*)w, (bf16_t*)dy, lddy, rows, ncols, dw, workspace);
    DwmFoldArgs f = {};
    f.ws[0] = workspace; f.out[0] = dw; f.nslots = 1;
    f.nfold = blocks; f.fold_stride = ncols; f.group_stride = 0; f.groups = 1; f.ncols = ncols; f.ld_out = ncols;
    dwm_ordered_finish(f, (hipStream_t)stream);
    return dwm_launch_status();
}

extern "C" int dwm_adamw(float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                         float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
                         void* stream) {
    if (!p || !g || !m || !v || n <= 0 || bias_corr1 <= 0.f || bias_corr2 <= 0.f) return DWM_EINVAL;
    hipLaunchKernelGGL(adamw_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (bf16_t*)p_bf16, n, lr,
                       beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale);
    return dwm_launch_status();
}

extern "C" int dwm_adamw_multi(const dwm_adamw_item* items, const int32_t* block_item, const int64_t* block_start, int64_t n_blocks,
                               int64_t chunk, float lr, float beta1, float beta2, float eps, float weight_decay, float bias_corr1,
                               float bias_corr2, float grad_scale, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk) || bias_corr1 <= 0.f || bias_corr2 <= 0.f)
        return DWM_EINVAL;
    hipLaunchKernelGGL(adamw_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item, block_start,
                       chunk, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale);
    return dwm_launch_status();
}

static int adamw_dev_operands(const float* hyper, const float* cond) {
    if (!hyper) return DWM_EINVAL;
    if ((((uintptr_t)hyper) & 3u) != 0 || (((uintptr_t)cond) & 3u) != 0) return DWM_EALIGN;
    return DWM_OK;
}

extern "C" int dwm_adamw_multi_dev(const dwm_adamw_item* items, const int32_t* block_item, const int64_t* block_start,
                                   int64_t n_blocks, int64_t chunk, const float* hyper, const float* cond, float beta1, float beta2,
                                   float eps, float weight_decay, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk)) return DWM_EINVAL;
    if (const int rc = adamw_dev_operands(hyper, cond)) return rc;
    hipLaunchKernelGGL(adamw_multi_dev_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, hyper, cond, beta1, beta2, eps, weight_decay);
    return dwm_launch_status();
}

extern "C" int dwm_quantize_blockwise8(const float* x, int64_t n, const float* code, int32_t floor_positive, uint8_t* q,
                                       float* absmax, void* stream) {
    if (!x || !code || !q || !absmax || n <= 0) return DWM_EINVAL;
    hipLaunchKernelGGL(quantize_blockwise8_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, n, code,
                       floor_positive, q, absmax);
    return dwm_launch_status();
}

extern "C" int dwm_dequantize_blockwise8(const uint8_t* q, const float* absmax, int64_t n, const float* code, float* x,
                                         void* stream) {
    if (!q || !absmax || !code || !x || n <= 0) return DWM_EINVAL;
    hipLaunchKernelGGL(dequantize_blockwise8_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, q, absmax, n,
                       code, x);
    return dwm_launch_status();
}

extern "C" int dwm_adamw8_multi(const dwm_adamw8_item* items, const int32_t* block_item, const int64_t* block_start,
                                int64_t n_blocks, int64_t chunk, const float* code_m, const float* code_v, float lr, float beta1,
                                float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
                                void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk) || !code_m || !code_v || chunk % Q8_BLOCK != 0 ||
        bias_corr1 <= 0.f || bias_corr2 <= 0.f) return DWM_EINVAL;
    hipLaunchKernelGGL(adamw8_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, code_m, code_v, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale);
    return dwm_launch_status();
}

extern "C" int dwm_adamw8_multi_dev(const dwm_adamw8_item* items, const int32_t* block_item, const int64_t* block_start,
                                    int64_t n_blocks, int64_t chunk, const float* code_m, const float* code_v, const float* hyper,
                                    const float* cond, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk) || !code_m || !code_v || chunk % Q8_BLOCK != 0)
        return DWM_EINVAL;
    if (const int rc = adamw_dev_operands(hyper, cond)) return rc;
    hipLaunchKernelGGL(adamw8_multi_dev_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, code_m, code_v, hyper, cond, beta1, beta2, eps, weight_decay);
    return dwm_launch_status();
}

// ---- EMA of the weights: the four fused entries, the stand-alone update and the exchange (include/dwm_hip.h, "EMA weights")
static bool ema_bad_omd(float one_minus_decay) { return !(one_minus_decay >= 0.f && one_minus_decay <= 1.f); }      // NaN included

extern "C" int dwm_adamw_ema_multi(const dwm_adamw_ema_item* items, const int32_t* block_item, const int64_t* block_start,
                                   int64_t n_blocks, int64_t chunk, float lr, float beta1, float beta2, float eps, float weight_decay,
                                   float bias_corr1, float bias_corr2, float grad_scale, float one_minus_decay, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk) || bias_corr1 <= 0.f || bias_corr2 <= 0.f ||
        ema_bad_omd(one_minus_decay)) return DWM_EINVAL;
    hipLaunchKernelGGL(adamw_ema_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale, one_minus_decay);
    return dwm_launch_status();
}

extern "C" int dwm_adamw_ema_multi_dev(const dwm_adamw_ema_item* items, const int32_t* block_item, const int64_t* block_start,
                                       int64_t n_blocks, int64_t chunk, const float* hyper, const float* cond, float beta1,
                                       float beta2, float eps, float weight_decay, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk)) return DWM_EINVAL;
    if (const int rc = adamw_dev_operands(hyper, cond)) return rc;
    hipLaunchKernelGGL(adamw_ema_multi_dev_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, hyper, cond, beta1, beta2, eps, weight_decay);
    return dwm_launch_status();
}

extern "C" int dwm_adamw8_ema_multi(const dwm_adamw8_ema_item* items, const int32_t* block_item, const int64_t* block_start,
                                    int64_t n_blocks, int64_t chunk, const float* code_m, const float* code_v, float lr, float beta1,
                                    float beta2, float eps, float weight_decay, float bias_corr1, float bias_corr2, float grad_scale,
                                    float one_minus_decay, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk) || !code_m || !code_v || chunk % Q8_BLOCK != 0 ||
        bias_corr1 <= 0.f || bias_corr2 <= 0.f || ema_bad_omd(one_minus_decay)) return DWM_EINVAL;
    hipLaunchKernelGGL(adamw8_ema_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, code_m, code_v, lr, beta1, beta2, eps, weight_decay, bias_corr1, bias_corr2, grad_scale,
                       one_minus_decay);
    return dwm_launch_status();
}

extern "C" int dwm_adamw8_ema_multi_dev(const dwm_adamw8_ema_item* items, const int32_t* block_item, const int64_t* block_start,
                                        int64_t n_blocks, int64_t chunk, const float* code_m, const float* code_v, const float* hyper,
                                        const float* cond, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk) || !code_m || !code_v || chunk % Q8_BLOCK != 0)
        return DWM_EINVAL;
    if (const int rc = adamw_dev_operands(hyper, cond)) return rc;
    hipLaunchKernelGGL(adamw8_ema_multi_dev_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, code_m, code_v, hyper, cond, beta1, beta2, eps, weight_decay);
    return dwm_launch_status();
}

extern "C" int dwm_ema_multi(const dwm_ema_item* items, const int32_t* block_item, const int64_t* block_start, int64_t n_blocks,
                             int64_t chunk, float one_minus_decay, const float* hyper, const float* cond, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk) || (!hyper && ema_bad_omd(one_minus_decay)))
        return DWM_EINVAL;
    if ((((uintptr_t)hyper) & 3u) != 0 || (((uintptr_t)cond) & 3u) != 0) return DWM_EALIGN;
    hipLaunchKernelGGL(ema_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item, block_start,
                       chunk, one_minus_decay, hyper, cond);
    return dwm_launch_status();
}

extern "C" int dwm_ema_swap_multi(const dwm_ema_swap_item* items, const int32_t* block_item, const int64_t* block_start,
                                  int64_t n_blocks, int64_t chunk, void* stream) {
    if (dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk)) return DWM_EINVAL;
    hipLaunchKernelGGL(ema_swap_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk);
    return dwm_launch_status();
}

extern "C" int dwm_cast_bf16_to_f32(const void* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int64_t cols,
                                    int32_t accumulate, void* stream) {
    if (!x || !y || rows <= 0 || cols <= 0 || ldx < cols || ldy < cols) return DWM_EINVAL;
    if (cols % 8 == 0 && ldx % 8 == 0 && ldy % 4 == 0 && dwm_aligned16(x) && dwm_aligned16(y))
        hipLaunchKernelGGL(cast_bf16_to_f32_vec_kernel, dim3(grid_for(rows * cols / 8)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, ldx, y, ldy, rows, cols / 8, accumulate);
    else
        hipLaunchKernelGGL(cast_bf16_to_f32_kernel, dim3(grid_for(rows * cols)), dim3(256), 0, (hipStream_t)stream,
                           (const bf16_t*)x, ldx, y, ldy, rows, cols, accumulate);
    return dwm_launch_status();
}
