// Kernels of the frozen text encoders (CLIP-L / CLIP-G / T5-XXL, opendwm_amd/text_encoders.py): what the GEMM, LayerNorm and
// elementwise files do not already cover.
//
//   dwm_text_attention   softmax(scale Q K^T [+ bias] [causal]) V for n_seq sequences of L <= 128 tokens, heads of width 64
//   dwm_rmsnorm_rows     T5LayerNorm: whole-row RMS norm of the fp32 residual stream, bf16 out
//   dwm_text_embed       token (+ position) embedding gather into the fp32 residual stream
//   dwm_text_act         quick-GELU / erf-GELU / tanh-GELU on bf16, plain or gated (act(x[:, :F]) * x[:, F:])
//   dwm_*_f32            the four above with fp32 operands: the fp32 accuracy path of the encoders (text_attn_f32_kernel and the
//                        float instantiations of the other three; exact fp32 contractions, library exp / erfc / log)
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
// (T: element type of w and y - bf16_t, or float on the fp32 accuracy path)
template <typename T>
__global__ void __launch_bounds__(256)
rmsnorm_rows_kernel(const float* __restrict__ x, int64_t ldx, int D, const T* __restrict__ w, float eps,
                    T* __restrict__ y, int64_t ldy) {
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
    T* const yr = y + (int64_t)blockIdx.x * ldy;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int ch = tid + 256 * i;
        if (ch < nch) {
            float g[8], f[8];
            load8<T>(w + ch * 8, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (v[i][e] * r) * g[e];
            store8<T>(yr + ch * 8, f);
        }
    }
}

// ---- out[i] = table[clamp(ids[i])] (+ pos[i % L]) in fp32; one workgroup per token (T: element type of the tables)
template <typename T>
__global__ void __launch_bounds__(256)
text_embed_kernel(const int64_t* __restrict__ ids, const T* __restrict__ table, int64_t vocab, int D,
                  const T* __restrict__ pos, int64_t L, float* __restrict__ out, int64_t ldo) {
    const int64_t i = blockIdx.x;
    int64_t id = ids[i];
    id = id < 0 ? 0 : id >= vocab ? vocab - 1 : id;              // a bad id never becomes an address outside the table
    const T* const tr = table + id * D;
    const T* const pr = pos ? pos + (i % L) * D : nullptr;
    float* const orow = out + i * ldo;
    for (int ch = threadIdx.x; ch < (D >> 3); ch += 256) {
        float f[8];
        load8<T>(tr + ch * 8, f);
        if (pr) {
            float g[8];
            load8<T>(pr + ch * 8, g);
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

// The fp32 accuracy path: the same three formulations on the library's exp / erfc / log (about an ulp each) instead of the hardware
// exp2 / log2 approximations, in the natural-log domain.  Kind 2: t = 2 sqrt(2 / pi) (x + 0.044715 x^3); below t = -20 the 1 of
// 1 + e^-t is under half an ulp of e^-t, and x e^t = -e^(t + ln |x|) is formed in the exponent, where a subnormal sigmoid cannot
// cost the product its precision
template <int KIND> DWM_DEVINL float text_act_f32_f(float x) {
    if (KIND == 0) return x / (1.f + expf(-1.702f * x));
    if (KIND == 1) return 0.5f * x * erfcf(-0.7071067811865476f * x);
    const float t = x * (1.5957691216057308f + 0.07135481627260025f * x * x);
    if (t < -20.f) return -expf(t + logf(-x));
    return x / (1.f + expf(-t));
}
template <int KIND, typename T> DWM_DEVINL float text_act_of(float x) {
    if constexpr (std::is_same<T, float>::value) return text_act_f32_f<KIND>(x);
    else return text_act_f<KIND>(x);
}

template <int KIND, bool GATED, typename T>
__global__ void __launch_bounds__(256)
text_act_kernel(const T* __restrict__ x, int64_t ldx, int64_t rows, int nch, T* __restrict__ y, int64_t ldy) {
    const int64_t total = rows * nch;
    for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
        const int64_t r = idx / nch;
        const int c = (int)(idx - r * nch) * 8;
        float a[8], f[8];
        load8<T>(x + r * ldx + c, a);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = text_act_of<KIND, T>(a[e]);
        if (GATED) {
            float g[8];
            load8<T>(x + r * ldx + (int64_t)nch * 8 + c, g);
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] *= g[e];
        }
        store8<T>(y + r * ldy + c, f);
    }
}

template <int KIND, typename T>
int text_act_launch(const void* x, int64_t ldx, int64_t rows, int nch, int gated, void* y, int64_t ldy, hipStream_t st) {
    const int64_t total = rows * nch;
    const unsigned grid = (unsigned)((total + 255) / 256 < 65536 ? (total + 255) / 256 : 65536);
    if (gated)
        hipLaunchKernelGGL((text_act_kernel<KIND, true, T>), dim3(grid), dim3(256), 0, st, (const T*)x, ldx, rows, nch, (T*)y, ldy);
    else
        hipLaunchKernelGGL((text_act_kernel<KIND, false, T>), dim3(grid), dim3(256), 0, st, (const T*)x, ldx, rows, nch, (T*)y, ldy);
    return dwm_launch_status();
}

// what dwm_text_act and dwm_text_act_f32 share; T: bf16_t or float, 16 / sizeof(T) elements per 16 bytes
template <typename T>
int text_act_entry(const void* x, int64_t ldx, int64_t rows, int64_t F, int32_t kind, int32_t gated, void* y, int64_t ldy, void* stream) {
    constexpr int64_t V = 16 / sizeof(T);
    if (x == nullptr || y == nullptr || rows <= 0 || F <= 0 || kind < 0 || kind > 2 || (gated != 0 && gated != 1)) return DWM_EINVAL;
    if (F % 8 != 0 || F >= (1ll << 31)) return DWM_EUNSUPPORTED;
    if (ldx < (gated ? 2 * F : F) || ldy < F) return DWM_EINVAL;
    if (ldx % V != 0 || ldy % V != 0 || !dwm_aligned16(x) || !dwm_aligned16(y)) return DWM_EALIGN;
    const int nch = (int)(F / 8);
    hipStream_t st = (hipStream_t)stream;
    if (kind == 0) return text_act_launch<0, T>(x, ldx, rows, nch, gated, y, ldy, st);
    if (kind == 1) return text_act_launch<1, T>(x, ldx, rows, nch, gated, y, ldy, st);
    return text_act_launch<2, T>(x, ldx, rows, nch, gated, y, ldy, st);
}

// ---- fp32 attention (dwm_text_attention_f32).  One head's K and V in fp32 are 64 KiB, so the bf16 plan (a wave owns a head, four
// heads per workgroup) does not fit 160 KiB of LDS: here ONE WORKGROUP of 4 waves owns a (sequence, head), stages its K rows
// ([L][64] fp32, row pitch 65 words: lane l reading row l at column d hits bank (l + d) % 64, conflict-free) and V rows ([L][64],
// pitch 64: lane = channel) once, and its waves take the queries round-robin.  Per query, in a wave:
//   scores: lane l owns keys l and l + 64; s = sum_d q[d] k[d] as a chain of 64 fp32 FMAs, d ascending (q read from a per-wave LDS
//     row, a broadcast); x = scale s + bias in fp32; excluded keys (>= L, causally hidden) by selection, their K row address
//     clamped to L - 1;
//   softmax: exact maximum and sum over the wave (xor trees: a fixed order), p = expf(x - m), 0 for an excluded key;
//   output: lane d owns channel d; o = sum_j p[j] V[j][d] as a chain of fp32 FMAs over the visible keys, j ascending (p through a
//     per-wave LDS row), then ONE division by the sum.  Nothing is rounded to bf16 anywhere.
// Every wave walks ceil(L / 4) queries (the barriers are uniform); a query >= L repeats row L - 1 and is not stored.
constexpr int TF_KPITCH = 65;
constexpr int TF_LDS = (128 * TF_KPITCH + 128 * 64 + 4 * 64 + 4 * 128) * 4;      // 69120 B: two workgroups per CU

struct TfParams {
    const float *q, *k, *v;
    float* o;
    const float* bias;
    int64_t ld, ldo;
    int L, heads, causal;
    float scale;
};

__global__ void __launch_bounds__(256)
text_attn_f32_kernel(const TfParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t seq = (int64_t)blockIdx.x / p.heads;
    const int h = (int)((int64_t)blockIdx.x - seq * p.heads);
    const int L = p.L;
    const int64_t row0 = seq * L;
    float* const Ks = (float*)smem;
    float* const Vs = Ks + 128 * TF_KPITCH;
    float* const qs = Vs + 128 * 64 + wave * 64;
    float* const ps = Vs + 128 * 64 + 4 * 64 + wave * 128;
    const float* const qg = p.q + h * 64;
    const float* const kg = p.k + h * 64;
    const float* const vg = p.v + h * 64;

    for (int idx = tid; idx < L * 16; idx += 256) {              // rows 0 .. L - 1, 16 chunks of 16 bytes each
        const int r = idx >> 4, c = (idx & 15) * 4;
        const float4 kk = *(const float4*)(kg + (row0 + r) * p.ld + c);
        const float4 vv = *(const float4*)(vg + (row0 + r) * p.ld + c);
        float* const kd = Ks + r * TF_KPITCH + c;
        kd[0] = kk.x; kd[1] = kk.y; kd[2] = kk.z; kd[3] = kk.w;
        *(float4*)(Vs + r * 64 + c) = vv;
    }
    __syncthreads();

    const int kr0 = lane < L ? lane : L - 1, kr1 = lane + 64 < L ? lane + 64 : L - 1;
    const float* const k0 = Ks + kr0 * TF_KPITCH;
    const float* const k1 = Ks + kr1 * TF_KPITCH;
    for (int q0 = 0; q0 < L; q0 += 4) {
        const int iq = q0 + wave;
        const int iqc = iq < L ? iq : L - 1;
        qs[lane] = qg[(row0 + iqc) * p.ld + lane];
        __syncthreads();
        float s0 = 0.f, s1 = 0.f;
#pragma unroll 16
        for (int d = 0; d < 64; ++d) {
            const float qd = qs[d];
            s0 = fmaf(qd, k0[d], s0);
            s1 = fmaf(qd, k1[d], s1);
        }
        float x0 = s0 * p.scale, x1 = s1 * p.scale;
        if (p.bias) {
            const float* const brow = p.bias + ((int64_t)h * L + iqc) * L;
            x0 += brow[kr0];
            x1 += brow[kr1];
        }
        const bool live0 = lane < L && (!p.causal || lane <= iqc);
        const bool live1 = lane + 64 < L && (!p.causal || lane + 64 <= iqc);
        float mx = fmaxf(live0 ? x0 : -INFINITY, live1 ? x1 : -INFINITY);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));      // finite: key 0 is live for every query
        const float p0 = live0 ? expf(x0 - mx) : 0.f;            // selection: an excluded key contributes exactly 0
        const float p1 = live1 ? expf(x1 - mx) : 0.f;
        const float sum = wave_sum(p0 + p1);
        ps[lane] = p0;
        ps[lane + 64] = p1;
        __syncthreads();
        const int nk = p.causal ? iqc + 1 : L;
        float acc = 0.f;
        for (int j = 0; j < nk; ++j) acc = fmaf(ps[j], Vs[j * 64 + lane], acc);
        if (iq < L) p.o[(row0 + iq) * p.ldo + h * 64 + lane] = acc / sum;
    }
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
    hipLaunchKernelGGL(rmsnorm_rows_kernel<bf16_t>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, ldx, (int)D, (const bf16_t*)w, eps,
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
    hipLaunchKernelGGL(text_embed_kernel<bf16_t>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, ids, (const bf16_t*)table, vocab, (int)D,
                       (const bf16_t*)pos, pos != nullptr ? L : 1, out, ldo);
    return dwm_launch_status();
}

extern "C" int dwm_text_act(const void* x, int64_t ldx, int64_t rows, int64_t F, int32_t kind, int32_t gated, void* y, int64_t ldy,
                            void* stream) {
    return text_act_entry<bf16_t>(x, ldx, rows, F, kind, gated, y, ldy, stream);
}

// ---- the fp32 accuracy path: the same refusals as the bf16 entries, strides in fp32 elements (16 bytes = 4 of them)
extern "C" int dwm_text_attention_f32(const dwm_text_attn_args* a, void* stream) {
    if (a == nullptr || a->q == nullptr || a->k == nullptr || a->v == nullptr || a->out == nullptr) return DWM_EINVAL;
    if (a->L < 1 || a->L > 128) return DWM_EUNSUPPORTED;
    if (a->n_seq <= 0 || a->heads <= 0 || (a->causal != 0 && a->causal != 1)) return DWM_EINVAL;
    const int64_t width = (int64_t)a->heads * 64;
    if (a->ld < width || a->ldo < width) return DWM_EINVAL;
    if (a->ld % 4 != 0 || a->ldo % 4 != 0) return DWM_EALIGN;
    if (!dwm_aligned16(a->q) || !dwm_aligned16(a->k) || !dwm_aligned16(a->v) || !dwm_aligned16(a->out)) return DWM_EALIGN;
    if (a->bias != nullptr && (((uintptr_t)a->bias) & 3u) != 0) return DWM_EALIGN;
    if (a->heads > (1 << 16) || a->n_seq > (1ll << 31) / a->heads - 1) return DWM_EUNSUPPORTED;      // one-dimensional grid
    TfParams p;
    p.q = (const float*)a->q; p.k = (const float*)a->k; p.v = (const float*)a->v; p.o = (float*)a->out;
    p.bias = a->bias;
    p.ld = a->ld; p.ldo = a->ldo;
    p.L = (int)a->L; p.heads = a->heads; p.causal = a->causal;
    p.scale = a->scale;
    const hipError_t e = dwm_allow_dynamic_lds<text_attn_f32_kernel>(TF_LDS);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(text_attn_f32_kernel, dim3((unsigned)(a->n_seq * a->heads)), dim3(256), (size_t)TF_LDS, (hipStream_t)stream, p);
    return dwm_launch_status();
}

extern "C" int dwm_rmsnorm_rows_f32(const float* x, int64_t ldx, int64_t rows, int64_t D, const float* w, float eps, float* y, int64_t ldy,
                                    void* stream) {
    if (x == nullptr || w == nullptr || y == nullptr || rows <= 0 || D <= 0) return DWM_EINVAL;
    if (D % 8 != 0 || D > 8192) return DWM_EUNSUPPORTED;
    if (ldx < D || ldy < D) return DWM_EINVAL;
    if (ldx % 4 != 0 || ldy % 4 != 0 || !dwm_aligned16(x) || !dwm_aligned16(w) || !dwm_aligned16(y)) return DWM_EALIGN;
    if (rows >= (1ll << 31)) return DWM_EUNSUPPORTED;
    hipLaunchKernelGGL(rmsnorm_rows_kernel<float>, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, ldx, (int)D, w, eps, y, ldy);
    return dwm_launch_status();
}

extern "C" int dwm_text_embed_f32(const int64_t* ids, int64_t n, const float* table, int64_t vocab, int64_t D, const float* pos, int64_t L,
                                  float* out, int64_t ldo, void* stream) {
    if (ids == nullptr || table == nullptr || out == nullptr || n <= 0 || vocab <= 0 || D <= 0) return DWM_EINVAL;
    if (pos != nullptr && L <= 0) return DWM_EINVAL;
    if (D % 8 != 0 || D >= (1ll << 31)) return DWM_EUNSUPPORTED;
    if (ldo < D) return DWM_EINVAL;
    if (ldo % 4 != 0 || !dwm_aligned16(table) || !dwm_aligned16(out) || (pos != nullptr && !dwm_aligned16(pos)) ||
        (((uintptr_t)ids) & 7u) != 0)
        return DWM_EALIGN;
    if (n >= (1ll << 31)) return DWM_EUNSUPPORTED;
    hipLaunchKernelGGL(text_embed_kernel<float>, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, ids, table, vocab, (int)D, pos,
                       pos != nullptr ? L : 1, out, ldo);
    return dwm_launch_status();
}

extern "C" int dwm_text_act_f32(const float* x, int64_t ldx, int64_t rows, int64_t F, int32_t kind, int32_t gated, float* y, int64_t ldy,
                                void* stream) {
    return text_act_entry<float>(x, ldx, rows, F, kind, gated, y, ldy, stream);
}
