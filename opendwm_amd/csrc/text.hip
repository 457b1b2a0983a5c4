// Kernels of the frozen text encoders (CLIP-L / CLIP-G / T5-XXL, opendwm_amd/text_encoders.py): what the GEMM, LayerNorm and
// elementwise files do not already cover.
//
//   dwm_text_attention   softmax(scale Q K^T [+ bias] [causal]) V for n_seq sequences of L <= 128 tokens, heads of width 64
//   dwm_rmsnorm_rows     T5LayerNorm: whole-row RMS norm of the fp32 residual stream, bf16 out
//   dwm_text_embed       token (+ position) embedding gather into the fp32 residual stream
//   dwm_text_act         quick-GELU / erf-GELU / tanh-GELU on bf16, plain or gated (act(x[:, :F]) * x[:, F:])
//
// Attention (text_attn_kernel): ONE wave per (sequence, head), 4 waves = 4 (sequence, head) items per workgroup, no data shared
// between waves.  A wave stages its head's K rows ([128][64] bf16, row pitch 144 B: conflict-free 16-byte row reads) and V
// TRANSPOSED ([64 channels][128 keys], pitch 272 B) into its own LDS slice, rows past L as zeros (selection on the value; the
// address is clamped to row L - 1), then walks the ceil(L / 16) query tiles:
//   S^T (keys x 16 queries) = K Q^T on v_mfma_f32_16x16x32_bf16, A = K rows from LDS, B = Q rows straight from memory: lane l holds
//     query (l & 15) and, of key block t, the keys 16 t + 4 (l >> 4) + r, r = 0..3.  All <= 8 key blocks of the tile stay in
//     registers (32 scores per lane), so the row maximum is EXACT and the softmax is two passes over registers: no online
//     rescaling, no fast path to fall back from.
//   x = scale s + bias[head, query, key] in fp32, natural-log domain; keys >= L and (causal) keys > query are removed BY SELECTION
//     (x = -inf for the maximum, p = 0 for the sum and the product): never a product with a mask, never a large negative addend.
//     Key 0 is always allowed, so the maximum is finite and the sum >= 1.
//   O^T (64 channels x 16 queries) = V^T P^T on the same MFMA: the contraction index of a 32-key step is ordered as the score
//     registers are - slot j of lane group g = key 32 s + 16 (j >> 2) + 4 g + (j & 3) - so P^T is the lane's own registers rounded
//     to bf16 and V^T is two 8-byte LDS reads per 16-channel block; A and B agree on that order, which is all a contraction needs.
//     The denominator is the fp32 sum of the unrounded p.  Causal: key blocks past the query tile's diagonal are skipped (their p
//     is 0 by the selection above either way).
//   Query rows >= L of the last tile are computed on row L - 1 (clamped address) and not stored; a workgroup's waves past the last
//     item repeat the last item and do not store.  Nothing outside rows [0, n_seq L) of q / k / v / out is addressed.
#include "common.h"
#include "dwm_hip.h"

namespace {

constexpr int TA_WAVES = 4;
constexpr int TA_KPITCH = 144;                                   // bytes per K row in LDS (64 bf16 + 16)
constexpr int TA_VPITCH = 272;                                   // bytes per channel of V^T in LDS (128 bf16 + 16)
constexpr int TA_WAVE_LDS = 128 * TA_KPITCH + 64 * TA_VPITCH;    // 35840 B per wave
constexpr int TA_LDS = TA_WAVES * TA_WAVE_LDS;                   // 140 KiB per workgroup

struct TaParams {
    const bf16_t *q, *k, *v;
    bf16_t* o;
    const float* bias;
    int64_t ld, ldo, n_items;
    int L, heads, causal;
    float scale;
};

__global__ void __launch_bounds__(64 * TA_WAVES, 1)
text_attn_kernel(const TaParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int64_t item = (int64_t)blockIdx.x * TA_WAVES + wave;
    const bool live_item = item < p.n_items;
    if (!live_item) item = p.n_items - 1;
    const int64_t seq = item / p.heads;
    const int h = (int)(item - seq * p.heads);
    const int L = p.L;
    const int64_t row0 = seq * L;
    const int nkb = (L + 15) >> 4;                               // key blocks of 16 = query tiles of 16
    const int ns = (L + 31) >> 5;                                // 32-key steps of the PV product
    char* const Ks = smem + wave * TA_WAVE_LDS;
    char* const Vt = Ks + 128 * TA_KPITCH;
    const bf16_t* const kg = p.k + h * 64;
    const bf16_t* const vg = p.v + h * 64;
    const bf16_t* const qg = p.q + h * 64;

    for (int idx = lane; idx < nkb * 16 * 8; idx += 64) {        // K rows 0 .. 16 nkb - 1, 8 chunks of 16 bytes each
        const int r = idx >> 3, ch = idx & 7;
        const uint4 x = *(const uint4*)(kg + (row0 + (r < L ? r : L - 1)) * p.ld + ch * 8);
        const uint32_t live = r < L ? 0xffffffffu : 0u;
        *(uint4*)(Ks + r * TA_KPITCH + ch * 16) = make_uint4(x.x & live, x.y & live, x.z & live, x.w & live);
    }
    {
        const int nk = ns * 32;                                  // V^T: keys 0 .. 32 ns - 1, key fastest over the lanes
        for (int idx = lane; idx < nk * 8; idx += 64) {
            const int ch = idx / nk, r = idx - ch * nk;
            const uint4 x = *(const uint4*)(vg + (row0 + (r < L ? r : L - 1)) * p.ld + ch * 8);
            const uint32_t live = r < L ? 0xffffffffu : 0u;
            const uint32_t w[4] = {x.x & live, x.y & live, x.z & live, x.w & live};
#pragma unroll
            for (int e = 0; e < 8; ++e)
                *(uint16_t*)(Vt + (ch * 8 + e) * TA_VPITCH + r * 2) = (uint16_t)(e & 1 ? w[e >> 1] >> 16 : w[e >> 1] & 0xffffu);
        }
    }
    __syncthreads();

    const int c16 = lane & 15, g4 = lane >> 4;
    const char* const k_rd = Ks + c16 * TA_KPITCH + g4 * 16;
    const char* const v_rd = Vt + c16 * TA_VPITCH + g4 * 8;
    for (int qt = 0; qt < nkb; ++qt) {
        const int iq = qt * 16 + c16;
        const int iqc = iq < L ? iq : L - 1;
        const int kend = p.causal ? qt + 1 : nkb;                // key blocks this tile can see
        const bf16_t* const qrow = qg + (row0 + iqc) * p.ld + g4 * 8;
        const bf16x8 qf0 = *(const bf16x8*)qrow;
        const bf16x8 qf1 = *(const bf16x8*)(qrow + 32);
        const float* const brow = p.bias ? p.bias + ((int64_t)h * L + iqc) * L : nullptr;

        float pv[8][4];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 8; ++t) {
#pragma unroll
            for (int r = 0; r < 4; ++r) pv[t][r] = -INFINITY;
            if (t < kend) {
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
                const bf16x8 k0 = *(const bf16x8*)(k_rd + t * 16 * TA_KPITCH);
                const bf16x8 k1 = *(const bf16x8*)(k_rd + t * 16 * TA_KPITCH + 64);
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf0, s, 0, 0, 0);
                s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf1, s, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = 16 * t + 4 * g4 + r;
                    const bool live = key < L && (!p.causal || key <= iqc);
                    float x = s[r] * p.scale;
                    if (brow) x += brow[key < L ? key : L - 1];
                    pv[t][r] = live ? x : -INFINITY;
                    mx = fmaxf(mx, pv[t][r]);
                }
            }
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));                  // finite: key 0 is live for every query
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 8; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = pv[t][r];
                const float e = __builtin_amdgcn_exp2f((x - mx) * 1.4426950408889634f);
                pv[t][r] = x == -INFINITY ? 0.f : e;             // selection: an excluded key contributes exactly 0
                sum += pv[t][r];
            }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        const float inv = 1.f / sum;

        f32x4 acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb) acc[cb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            if (s2 < ns && 2 * s2 < kend) {
                uint4 pw;
                pw.x = pack_bf16x2(pv[2 * s2][0], pv[2 * s2][1]);
                pw.y = pack_bf16x2(pv[2 * s2][2], pv[2 * s2][3]);
                pw.z = pack_bf16x2(pv[2 * s2 + 1][0], pv[2 * s2 + 1][1]);
                pw.w = pack_bf16x2(pv[2 * s2 + 1][2], pv[2 * s2 + 1][3]);
                const bf16x8 pf = __builtin_bit_cast(bf16x8, pw);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const char* const va = v_rd + cb * 16 * TA_VPITCH + s2 * 64;
                    const uint2 lo = *(const uint2*)va;          // keys 32 s2 + 4 g4 .. + 3      (block 2 s2)
                    const uint2 hi = *(const uint2*)(va + 32);   // keys 32 s2 + 16 + 4 g4 .. + 3 (block 2 s2 + 1)
                    const bf16x8 vf = __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
                    acc[cb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, acc[cb], 0, 0, 0);
                }
            }
        }
        if (live_item && iq < L) {
            bf16_t* const orow = p.o + (row0 + iq) * p.ldo + h * 64 + 4 * g4;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                const float f[4] = {acc[cb][0] * inv, acc[cb][1] * inv, acc[cb][2] * inv, acc[cb][3] * inv};
                *(uint2*)(orow + cb * 16) = pack4(f);
            }
        }
    }
}

// ---- T5LayerNorm: y = x rsqrt(mean(x^2) + eps) w; one workgroup per row, the row stays in registers (D <= 8192 = 256 x 4 x 8)
__global__ void __launch_bounds__(256)
rmsnorm_rows_kernel(const float* __restrict__ x, int64_t ldx, int D, const bf16_t* __restrict__ w, float eps,
                    bf16_t* __restrict__ y, int64_t ldy) {
    __shared__ float part[4];
    const int tid = threadIdx.x;
    const int nch = D >> 3;
    const float* const xr = x + (int64_t)blockIdx.x * ldx;
    float v[4][8];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = tid + 256 * i;
        if (ch < nch) {
            load8<float>(xr + ch * 8, v[i]);
#pragma unroll
            for (int e = 0; e < 8; ++e) ss = fmaf(v[i][e], v[i][e], ss);
        }
    }
    ss = wave_sum(ss);
    if ((tid & 63) == 0) part[tid >> 6] = ss;
    __syncthreads();
    const float tot = (part[0] + part[1]) + (part[2] + part[3]);
    const float r = 1.f / sqrtf(tot / (float)D + eps);
    bf16_t* const yr = y + (int64_t)blockIdx.x * ldy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = tid + 256 * i;
        if (ch < nch) {
            float g[8], f[8];
            load8<bf16_t>(w + ch * 8, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (v[i][e] * r) * g[e];
            store8<bf16_t>(yr + ch * 8, f);
        }
    }
}

// ---- out[i] = table[clamp(ids[i])] (+ pos[i % L]) in fp32; one workgroup per token
__global__ void __launch_bounds__(256)
text_embed_kernel(const int64_t* __restrict__ ids, const bf16_t* __restrict__ table, int64_t vocab, int D,
                  const bf16_t* __restrict__ pos, int64_t L, float* __restrict__ out, int64_t ldo) {
    const int64_t i = blockIdx.x;
    int64_t id = ids[i];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;              // a bad id never becomes an address outside the table
    const bf16_t* const tr = table + id * D;
    const bf16_t* const pr = pos ? pos + (i % L) * D : nullptr;
    float* const orow = out + i * ldo;
    for (int ch = threadIdx.x; ch < (D >> 3); ch += 256) {
        float f[8];
        load8<bf16_t>(tr + ch * 8, f);
        if (pr) {
            float g[8];
            load8<bf16_t>(pr + ch * 8, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] += g[e];
        }
        store8<float>(orow + ch * 8, f);
    }
}

// ---- activations.  erf-GELU as 0.5 x erfc(-x / sqrt 2): relative accuracy in the negative tail too (1 + erf cancels there)
template <int KIND> DWM_DEVINL float text_act_f(float x) {
    if (KIND == 0) return x / (1.f + __builtin_amdgcn_exp2f(-2.4554669595930157f * x));      // x sigmoid(1.702 x)
    if (KIND == 1) return 0.5f * x * erfcf(-0.7071067811865476f * x);
    // tanh-GELU = x sigmoid(z ln 2), z = 2 log2(e) sqrt(2 / pi) (x + 0.044715 x^3) (gelu_tanh_f's constants).  Far in the negative
    // tail the sigmoid itself drops under the smallest normal number while x times it does not: there 1 + 2^-z = 2^-z to fp32
    // precision and x 2^z = -2^(z + log2 |x|) is formed in the exponent
    const float z = x * (2.302208198f + 0.1029432397f * x * x);
    if (z < -30.f) return -__builtin_amdgcn_exp2f(z + __builtin_amdgcn_logf(-x));
    return x / (1.f + __builtin_amdgcn_exp2f(-z));
}

template <int KIND, bool GATED>
__global__ void __launch_bounds__(256)
text_act_kernel(const bf16_t* __restrict__ x, int64_t ldx, int64_t rows, int nch, bf16_t* __restrict__ y, int64_t ldy) {
    const int64_t total = rows * nch;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t r = idx / nch;
        const int c = (int)(idx - r * nch) * 8;
        float a[8], f[8];
        load8<bf16_t>(x + r * ldx + c, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = text_act_f<KIND>(a[e]);
        if (GATED) {
            float g[8];
            load8<bf16_t>(x + r * ldx + (int64_t)nch * 8 + c, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] *= g[e];
        }
        store8<bf16_t>(y + r * ldy + c, f);
    }
}

template <int KIND>
int text_act_launch(const void* x, int64_t ldx, int64_t rows, int nch, int gated, void* y, int64_t ldy, hipStream_t st) {
    const int64_t total = rows * nch;
    const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    if (gated)
        hipLaunchKernelGGL((text_act_kernel<KIND, true>), dim3(grid), dim3(256), 0, st, (const bf16_t*)x, ldx, rows, nch, (bf16_t*)y, ldy);
    else
        hipLaunchKernelGGL((text_act_kernel<KIND, false>), dim3(grid), dim3(256), 0, st, (const bf16_t*)x, ldx, rows, nch, (bf16_t*)y, ldy);
    return dwm_launch_status();
}

}  // namespace

extern "C" int dwm_text_attention(const dwm_text_attn_args* a, void* stream) {
    if (a == nullptr || a->q == nullptr || a->k == nullptr || a->v == nullptr || a->out == nullptr) return DWM_EINVAL;
    if (a->L < 1 || a->L > 128) return DWM_EUNSUPPORTED;
    if (a->n_seq <= 0 || a->heads <= 0 || (a->causal != 0 && a->causal != 1)) return DWM_EINVAL;
    const int64_t width = (int64_t)a->heads * 64;
    if (a->ld < width || a->ldo < width) return DWM_EINVAL;
    if (a->ld % 8 != 0 || a->ldo % 8 != 0) return DWM_EALIGN;
    if (!dwm_aligned16(a->q) || !dwm_aligned16(a->k) || !dwm_aligned16(a->v) || !dwm_aligned16(a->out)) return DWM_EALIGN;
    if (a->bias != nullptr && (((uintptr_t)a->bias) & 3u) != 0) return DWM_EALIGN;
    if (a->heads > (1 << 16) || a->n_seq > (1ll << 31) / a->heads - 1) return DWM_EUNSUPPORTED;      // one-dimensional grid
    TaParams p;
    p.q = (const bf16_t*)a->q; p.k = (const bf16_t*)a->k; p.v = (const bf16_t*)a->v; p.o = (bf16_t*)a->out;
    p.bias = a->bias;
    p.ld = a->ld; p.ldo = a->ldo;
    p.n_items = a->n_seq * a->heads;
    p.L = (int)a->L; p.heads = a->heads; p.causal = a->causal;
    p.scale = a->scale;
    const hipError_t e = dwm_allow_dynamic_lds<text_attn_kernel>(TA_LDS);
    if (e != hipSuccess) return (int)e;
    const int64_t nblk = (p.n_items + TA_WAVES - 1) / TA_WAVES;
    hipLaunchKernelGGL(text_attn_kernel, dim3((unsigned)nblk), dim3(64 * TA_WAVES), (size_t)TA_LDS, (hipStream_t)stream, p);
    return dwm_launch_status();
}

extern "C" int dwm_rmsnorm_rows(const float* x, int64_t ldx, int64_t rows, int64_t D, const void* w, float eps, void* y, int64_t ldy,
                                void* stream) {
    if (x == nullptr || w == nullptr || y == nullptr || rows <= 0 || D <= 0) return DWM_EINVAL;
    if (D % 8 != 0 || D > 8192) return DWM_EUNSUPPORTED;
    if (ldx < D || ldy < D) return DWM_EINVAL;
    if (ldx % 4 != 0 || ldy % 8 != 0 || !dwm_aligned16(x) || !dwm_aligned16(w) || !dwm_aligned16(y)) return DWM_EALIGN;
    if (rows >= (1ll << 31)) return DWM_EUNSUPPORTED;
    hipLaunchKernelGGL(rmsnorm_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, ldx, (int)D, (const bf16_t*)w, eps,
                       (bf16_t*)y, ldy);
    return dwm_launch_status();
}

extern "C" int dwm_text_embed(const int64_t* ids, int64_t n, const void* table, int64_t vocab, int64_t D, const void* pos, int64_t L,
                              float* out, int64_t ldo, void* stream) {
    if (ids == nullptr || table == nullptr || out == nullptr || n <= 0 || vocab <= 0 || D <= 0) return DWM_EINVAL;
    if (pos != nullptr && L <= 0) return DWM_EINVAL;
    if (D % 8 != 0 || D >= (1ll << 31)) return DWM_EUNSUPPORTED;
    if (ldo < D) return DWM_EINVAL;
    if (ldo % 4 != 0 || !dwm_aligned16(table) || !dwm_aligned16(out) || (pos != nullptr && !dwm_aligned16(pos)) ||
        (((uintptr_t)ids) & 7u) != 0)
        return DWM_EALIGN;
    if (n >= (1ll << 31)) return DWM_EUNSUPPORTED;
    hipLaunchKernelGGL(text_embed_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, ids, (const bf16_t*)table, vocab, (int)D,
                       (const bf16_t*)pos, pos != nullptr ? L : 1, out, ldo);
    return dwm_launch_status();
}

extern "C" int dwm_text_act(const void* x, int64_t ldx, int64_t rows, int64_t F, int32_t kind, int32_t gated, void* y, int64_t ldy,
                            void* stream) {
    if (x == nullptr || y == nullptr || rows <= 0 || F <= 0 || kind < 0 || kind > 2 || (gated != 0 && gated != 1)) return DWM_EINVAL;
    if (F % 8 != 0 || F >= (1ll << 31)) return DWM_EUNSUPPORTED;
    if (ldx < (gated ? 2 * F : F) || ldy < F) return DWM_EINVAL;
    if (ldx % 8 != 0 || ldy % 8 != 0 || !dwm_aligned16(x) || !dwm_aligned16(y)) return DWM_EALIGN;
    const int nch = (int)(F / 8);
    hipStream_t st = (hipStream_t)stream;
    if (kind == 0) return text_act_launch<0>(x, ldx, rows, nch, gated, y, ldy, st);
    if (kind == 1) return text_act_launch<1>(x, ldx, rows, nch, gated, y, ldy, st);
    return text_act_launch<2>(x, ldx, rows, nch, gated, y, ldy, st);
}
