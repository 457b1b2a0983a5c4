// NF4 4-bit weights (opendwm_amd/nf4.py; the format is stated in include/dwm_hip.h, "NF4 4-bit weights"): quantise, dequantise and
// the fused dequantising GEMM of the text encoders' linear layers.
//
//   dwm_nf4_quantize     bf16 [N, K] (row stride ldw) -> q uint8 [N, K/2], absmax fp32 [N, K/64]
//   dwm_nf4_dequantize   q, absmax -> W' bf16 [N, K] (row stride ldw),  W' = bf16_rne(fl32(code[q] * absmax))
//   dwm_gemm_nf4         out[M, N] = A[M, K] W'^T (+ bias), bf16 out or added into an fp32 stream
//
// Quantise / dequantise: one lane per 8 consecutive elements of a row (16 bytes of bf16, 4 bytes of q), so 8 lanes share a block
// of 64 and its absmax (three xor-shuffles); K % 64 == 0 keeps such a group inside one row and all live or all past the end.
//
// GEMM (nf4_gemm_kernel): 4 waves per workgroup, a 64-column x 128-row output tile, K steps of 128.  The product is formed
// TRANSPOSED, out^T = W' A^T, on v_mfma_f32_16x16x32_bf16: wave w owns the 16 weight rows n0 + 16 w .. + 15 as the MFMA's A operand
// and all (up to 8) 16-row blocks of the A tile as its B operand, so a lane ends with 4 CONSECUTIVE output columns of one output
// row (8-byte bf16 store, 16-byte fp32 read-modify-write).
//   * W never touches LDS: lane (c = lane & 15, g = lane >> 4) reads the 16 bytes = 32 codes of row c at k0 + 32 g .. + 31 straight
//     from memory - one block's half, one absmax - a step ahead of their use.  A byte goes through a 256-entry table in LDS
//     (byte -> the two fp32 code values, built from the 16-entry table the caller passes), each value is multiplied by absmax in fp32
//     and the pair rounded to bf16 by v_cvt_pk_bf16_f32: exactly the bits dwm_nf4_dequantize stores.  Nothing is scaled after the
//     MFMA.
//   * The contraction index of a step is permuted to match that load: slot e of lane group g in MFMA j (j = 0..3) is
//     k = k0 + 32 g + 8 j + e.  The A tile lies in LDS row-major (pitch 272 B: conflict-free 16-byte row reads) and is read under the
//     same permutation (byte offset 64 g + 16 j of its row), which is all a contraction needs.
//   * The A tile is double-buffered through registers: the loads of step t + 1 are issued before the MFMAs of step t and stored to
//     the other buffer after them; one barrier per step.
//   * Edges by address clamp and selection, never by a product with a mask: A rows >= M repeat row M - 1 and weight rows >= N row
//     N - 1 (their results are not stored); the half step past K of an odd block count reads offset 0 of its row and contributes
//     zero operands on both sides.  Nothing outside A[0:M, 0:K], q, absmax, bias[0:N] and out[0:M, 0:N] is addressed.
//   * The K loop is one fixed order for every launch (no split-K; the upper half of a tile that M ends before is skipped, which
//     changes no other row), so a row's result does not depend on how many rows the launch has, and two launches agree bit for bit.
#include "common.h"
#include "dwm_hip.h"

namespace {

// ---------------------------------------------------------------------------------------------------- quantise / dequantise
__global__ void __launch_bounds__(256)
nf4_quantize_kernel(const bf16_t* __restrict__ w, int64_t ldw, int64_t n_chunks, int kch, const float* __restrict__ code,
                    uint8_t* __restrict__ q, float* __restrict__ absmax) {
    __shared__ float mid[16];
    if (threadIdx.x < 15) mid[threadIdx.x] = (code[threadIdx.x] + code[threadIdx.x + 1]) * 0.5f;
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool live = c < n_chunks;                              // n_chunks % 8 == 0: the 8 lanes of a block agree
    const int64_t cc = live ? c : n_chunks - 1;
    const int64_t row = cc / kch;
    const int col = (int)(cc - row * kch);
    float f[8];
    unpack8(*(const uint4*)(w + row * ldw + (int64_t)col * 8), f);
    float am = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) am = fmaxf(am, __builtin_fabsf(f[e]));
    am = fmaxf(am, __shfl_xor(am, 1, 64));
    am = fmaxf(am, __shfl_xor(am, 2, 64));
    am = fmaxf(am, __shfl_xor(am, 4, 64));
    float edge[15];
#pragma unroll
    for (int i = 0; i < 15; ++i) edge[i] = mid[i] * am;
    uint32_t out = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        uint32_t k = 0;
#pragma unroll
        for (int i = 0; i < 15; ++i) k += edge[i] < f[e] ? 1u : 0u;       // strict: a tie goes to the lower code
        if (am == 0.f) k = 7;
        out |= k << (8 * (e >> 1) + (e & 1 ? 0 : 4));                        // byte e / 2: even element high nibble, odd low
    }
    if (live) {
        *(uint32_t*)(q + row * ((int64_t)kch * 4) + (int64_t)col * 4) = out;
        if ((col & 7) == 0) absmax[row * (kch >> 3) + (col >> 3)] = am;
    }
}

__global__ void __launch_bounds__(256)
nf4_dequantize_kernel(const uint8_t* __restrict__ q, const float* __restrict__ absmax, int64_t n_chunks, int kch,
                      const float* __restrict__ code, bf16_t* __restrict__ w, int64_t ldw) {
    __shared__ float tab[16];
    if (threadIdx.x < 16) tab[threadIdx.x] = code[threadIdx.x];
    __syncthreads();
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= n_chunks) return;
    const int64_t row = c / kch;
    const int col = (int)(c - row * kch);
    const uint32_t x = *(const uint32_t*)(q + row * ((int64_t)kch * 4) + (int64_t)col * 4);
    const float am = absmax[row * (kch >> 3) + (col >> 3)];
    float f[8];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const uint32_t byte = (x >> (8 * b)) & 0xffu;
        f[2 * b] = tab[byte >> 4] * am;
        f[2 * b + 1] = tab[byte & 15u] * am;
    }
    store8<bf16_t>(w + row * ldw + (int64_t)col * 8, f);
}

// ------------------------------------------------------------------------------------------------------------------- GEMM
constexpr int NF_TM = 128;                                       // output rows (rows of A) per workgroup
constexpr int NF_TN = 64;                                        // output columns (weight rows) per workgroup: 16 per wave
constexpr int NF_TK = 128;                                       // K step: 16 bytes of codes per lane
constexpr int NF_PITCH = 2 * NF_TK + 16;                         // bytes per A row in LDS
constexpr int NF_ABUF = NF_TM * NF_PITCH;                        // 34816 B
constexpr int NF_LDS = 2 * NF_ABUF + 256 * 8;                    // two A buffers + the byte table: 70 KiB, two workgroups per CU

struct NfParams {
    const bf16_t* A;
    const uint8_t* q;
    const float* absmax;
    const float* code;
    const bf16_t* bias;
    bf16_t* C;
    float* C32;
    int64_t lda, ldc, ldc32, M;
    int N, K;
};

template <bool F32OUT>
__global__ void __launch_bounds__(256, 2)                        // two waves per SIMD: two workgroups share a CU (and its 160 KiB of LDS)
nf4_gemm_kernel(const NfParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float2* const tab = (float2*)(smem + 2 * NF_ABUF);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c16 = lane & 15, g4 = lane >> 4;
    const int64_t m0 = (int64_t)blockIdx.y * NF_TM;
    const int n0 = blockIdx.x * NF_TN;
    const int K = p.K;
    const int nk = (K + NF_TK - 1) / NF_TK;

    tab[tid] = make_float2(p.code[tid >> 4], p.code[tid & 15]);  // byte -> (high-nibble value, low-nibble value)

    const int n = n0 + wave * 16 + c16;
    const int nc = n < p.N ? n : p.N - 1;
    const uint8_t* const qrow = p.q + (int64_t)nc * (K >> 1);
    const float* const amrow = p.absmax + (int64_t)nc * (K >> 6);

    // this thread's 8 chunks (16 B) of the A tile: chunk idx = tid + 256 i -> row idx / 16, columns 8 (idx % 16) .. + 7
    const int a_ch = tid & 15;
    const bf16_t* a_src[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int64_t m = m0 + (tid >> 4) + 16 * i;
        a_src[i] = p.A + (m < p.M ? m : p.M - 1) * p.lda;
    }
    auto load_a = [&](int kt, uint4 (&r)[8]) {
        const int k = kt * NF_TK + a_ch * 8;
        const bool live = k < K;
        const int kc = live ? k : 0;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const uint4 x = *(const uint4*)(a_src[i] + kc);
            r[i] = live ? x : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    auto store_a = [&](char* buf, const uint4 (&r)[8]) {
#pragma unroll
        for (int i = 0; i < 8; ++i) *(uint4*)(buf + ((tid >> 4) + 16 * i) * NF_PITCH + a_ch * 16) = r[i];
    };
    auto load_w = [&](int kt, uint4& wq, float& am) {
        const int k = kt * NF_TK + g4 * 32;
        const int kc = k < K ? k : 0;
        wq = *(const uint4*)(qrow + (kc >> 1));
        am = amrow[kc >> 6];
    };

    f32x4 acc[8];
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) acc[mb] = (f32x4){0.f, 0.f, 0.f, 0.f};

    uint4 ra[8], wq;
    float am;
    load_a(0, ra);
    load_w(0, wq, am);
    store_a(smem, ra);
    __syncthreads();

    const bool upper = p.M - m0 > NF_TM / 2;                     // workgroup-uniform
#pragma unroll 1
    for (int kt = 0; kt < nk; ++kt) {
        const char* const cur = smem + (kt & 1) * NF_ABUF;
        const bool more = kt + 1 < nk;
        uint4 wq_next = wq;
        float am_next = am;
        if (more) {
            load_a(kt + 1, ra);
            load_w(kt + 1, wq_next, am_next);
        }
        const bool k_live = kt * NF_TK + g4 * 32 < K;
        const uint32_t words[4] = {wq.x, wq.y, wq.z, wq.w};
        uint32_t wb[16];
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const float2 t = tab[(words[b >> 2] >> (8 * (b & 3))) & 0xffu];
            const uint32_t v = pack_bf16x2(t.x * am, t.y * am);
            wb[b] = k_live ? v : 0u;
        }
        const char* const a_rd = cur + c16 * NF_PITCH + g4 * 64;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bf16x8 wf = __builtin_bit_cast(bf16x8, make_uint4(wb[4 * j], wb[4 * j + 1], wb[4 * j + 2], wb[4 * j + 3]));
#pragma unroll
            for (int mb = 0; mb < 4; ++mb) {
                const bf16x8 af = *(const bf16x8*)(a_rd + mb * 16 * NF_PITCH + j * 16);
                acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc[mb], 0, 0, 0);
            }
            if (upper) {                                         // rows 64 .. 127 of the tile: skipped as a whole where M ends before them
#pragma unroll
                for (int mb = 4; mb < 8; ++mb) {
                    const bf16x8 af = *(const bf16x8*)(a_rd + mb * 16 * NF_PITCH + j * 16);
                    acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf, af, acc[mb], 0, 0, 0);
                }
            }
        }
        if (more) store_a(smem + ((kt + 1) & 1) * NF_ABUF, ra);
        __syncthreads();
        wq = wq_next;
        am = am_next;
    }

    // lane: output row m0 + 16 mb + c16, columns nq .. nq + 3
    const int nq = n0 + wave * 16 + 4 * g4;
    if (nq >= p.N) return;                                       // N % 8 == 0: a group of 4 columns is inside or outside as a whole
    float bv[4] = {0.f, 0.f, 0.f, 0.f};
    if (p.bias != nullptr) unpack4(*(const uint2*)(p.bias + nq), bv);
#pragma unroll
    for (int mb = 0; mb < 8; ++mb) {
        const int64_t m = m0 + mb * 16 + c16;
        if (m < p.M) {
            const float v[4] = {acc[mb][0] + bv[0], acc[mb][1] + bv[1], acc[mb][2] + bv[2], acc[mb][3] + bv[3]};
            if (F32OUT) {
                float4* const dst = (float4*)(p.C32 + m * p.ldc32 + nq);
                const float4 c = *dst;
                *dst = make_float4(c.x + v[0], c.y + v[1], c.z + v[2], c.w + v[3]);
            } else {
                *(uint2*)(p.C + m * p.ldc + nq) = pack4(v);
            }
        }
    }
}

bool nf4_bad_matrix(const void* a, const void* b, const void* c, const void* d, int64_t N, int64_t K) {
    return a == nullptr || b == nullptr || c == nullptr || d == nullptr || N <= 0 || K <= 0 || K % 64 != 0;
}

}  // namespace

extern "C" int dwm_nf4_quantize(const void* w, int64_t ldw, int64_t N, int64_t K, const float* code, uint8_t* q, float* absmax,
                                void* stream) {
    if (nf4_bad_matrix(w, code, q, absmax, N, K) || ldw < K) return DWM_EINVAL;
    if (K >= (1ll << 31) || N * (K / 8) >= (1ll << 39)) return DWM_EUNSUPPORTED;                    // one-dimensional grid of 256 chunks
    if (ldw % 8 != 0 || !dwm_aligned16(w) || !dwm_aligned16(q) || (((uintptr_t)absmax | (uintptr_t)code) & 3u) != 0) return DWM_EALIGN;
    const int64_t n_chunks = N * (K / 8);
    hipLaunchKernelGGL(nf4_quantize_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w,
                       ldw, n_chunks, (int)(K / 8), code, q, absmax);
    return dwm_launch_status();
}

extern "C" int dwm_nf4_dequantize(const uint8_t* q, const float* absmax, int64_t N, int64_t K, const float* code, void* w, int64_t ldw,
                                  void* stream) {
    if (nf4_bad_matrix(q, absmax, code, w, N, K) || ldw < K) return DWM_EINVAL;
    if (K >= (1ll << 31) || N * (K / 8) >= (1ll << 39)) return DWM_EUNSUPPORTED;
    if (ldw % 8 != 0 || !dwm_aligned16(w) || !dwm_aligned16(q) || (((uintptr_t)absmax | (uintptr_t)code) & 3u) != 0) return DWM_EALIGN;
    const int64_t n_chunks = N * (K / 8);
    hipLaunchKernelGGL(nf4_dequantize_kernel, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, absmax,
                       n_chunks, (int)(K / 8), code, (bf16_t*)w, ldw);
    return dwm_launch_status();
}

extern "C" int dwm_gemm_nf4(const dwm_gemm_nf4_args* a, void* stream) {
    if (a == nullptr || nf4_bad_matrix(a->A, a->q, a->absmax, a->code, a->N, a->K) || a->M <= 0) return DWM_EINVAL;
    if ((a->C != nullptr) == (a->C32 != nullptr)) return DWM_EINVAL;                                // exactly one output
    if (a->lda < a->K || (a->C != nullptr && a->ldc < a->N) || (a->C32 != nullptr && a->ldc32 < a->N)) return DWM_EINVAL;
    if (a->N % 8 != 0 || a->K >= (1ll << 31) || a->N >= (1ll << 31) - NF_TN || a->M > 65535ll * NF_TM) return DWM_EUNSUPPORTED;
    if (a->lda % 8 != 0 || !dwm_aligned16(a->A) || !dwm_aligned16(a->q) || (a->bias != nullptr && !dwm_aligned16(a->bias)) ||
        (((uintptr_t)a->absmax | (uintptr_t)a->code) & 3u) != 0)
        return DWM_EALIGN;
    if (a->C != nullptr && (a->ldc % 8 != 0 || !dwm_aligned16(a->C))) return DWM_EALIGN;
    if (a->C32 != nullptr && (a->ldc32 % 4 != 0 || !dwm_aligned16(a->C32))) return DWM_EALIGN;
    NfParams p;
    p.A = (const bf16_t*)a->A; p.q = a->q; p.absmax = a->absmax; p.code = a->code; p.bias = (const bf16_t*)a->bias;
    p.C = (bf16_t*)a->C; p.C32 = a->C32;
    p.lda = a->lda; p.ldc = a->ldc; p.ldc32 = a->ldc32; p.M = a->M;
    p.N = (int)a->N; p.K = (int)a->K;
    const dim3 grid((unsigned)((a->N + NF_TN - 1) / NF_TN), (unsigned)((a->M + NF_TM - 1) / NF_TM));
    if (a->C32 != nullptr) {
        const hipError_t e = dwm_allow_dynamic_lds<nf4_gemm_kernel<true>>(NF_LDS);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((nf4_gemm_kernel<true>), grid, dim3(256), (size_t)NF_LDS, (hipStream_t)stream, p);
    } else {
        const hipError_t e = dwm_allow_dynamic_lds<nf4_gemm_kernel<false>>(NF_LDS);
        if (e != hipSuccess) return (int)e;
        hipLaunchKernelGGL((nf4_gemm_kernel<false>), grid, dim3(256), (size_t)NF_LDS, (hipStream_t)stream, p);
    }
    return dwm_launch_status();
}
