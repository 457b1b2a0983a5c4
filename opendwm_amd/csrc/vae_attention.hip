// Single-head attention of the VAE mid block (diffusers Attention inside UNetMidBlock2D of AutoencoderKL): I images of P pixels,
// ONE head whose dimension is the channel count C (512 in the released VAEs, 128 / 256 at reduced widths).
//
//     out[i*P + r, :] = sum_j softmax_j(scale * <q[i*P + r, :], k[i*P + j, :]>) * v[i*P + j, :]
//
// Flash-attention form: no P x P matrix leaves the chip, so any P >= 1 runs (the GEMM route of vae.py stops at P % 64 != 0 and at
// P > 4096).  One launch covers all images: workgroup b handles query tile b % nqt of image b / nqt.
//
// bf16 kernel (vae_attn_kernel): 4 waves, 64 queries, key tiles of 32.
//   S^T (32 keys x 64 queries): wave w takes queries 16w .. 16w+15 against both 16-key blocks: 2 accumulators of
//     v_mfma_f32_16x16x32_bf16, A = K rows, B = Q rows (both read row-major from LDS), C / 32 steps each.  A lane then holds ONE query
//     (lane & 15) and 8 of its 32 keys, so the row maximum / sum are 7 in-lane operations and two shuffles, and the running
//     maximum m, sum l and the rescale factor alpha are one register each.
//   O^T (C channels x 64 queries): wave w owns channels w C/4 .. (w+1) C/4 of all 64 queries as 32 x 32 accumulators
//     (C / 128 channel blocks x 2 query blocks; at C = 512: 8 tiles, 128 registers), 2 v_mfma_f32_32x32x16_bf16 per tile and key
//     tile.  A = V^T (contraction over keys = the ROW index of the V image: ds_read_b64_tr_b16, as gemm_tn.hip reads its operands),
//     B = P^T from the bf16 probabilities the S phase left in LDS.  A lane holds one query per query block, so alpha is one
//     multiplier per accumulator.  Both phases cost the same MFMA cycles and nothing is computed twice.
//   LDS at C = 512: Q 65 KiB, K 32.5 KiB (row pitch 2C + 16 bytes: conflict-free 16-byte row reads), V 32 KiB (64-byte slots XORed
//     with row & 3 for the transposing reads), P 5 KiB, alpha 256 B: 135 KiB, one workgroup per CU.
//   The next key tile's K and V rows are fetched into registers while the current tile is computed and stored to LDS after it.
//   Rows past P: queries are clamped on the load and skipped on the store; key rows are clamped on the load, ZEROED in LDS
//   (selection) and their scores set to -inf (selection), so nothing past an image's rows reaches a product.
//
// fp32 kernel (vae_attn_f32_kernel): the accuracy path (as fp32path.hip: exactness, not speed).  16 queries per workgroup, key tiles
// of 32 through one LDS buffer that holds K, then V; plain FMAs; 16 lanes share a query (scores: 2 keys per lane; output: C / 16
// channels per lane), so the statistics stay in registers there too.
#include "common.h"
#include "dwm_hip.h"

namespace {

typedef __attribute__((ext_vector_type(4))) short s16x4;

struct VaParams {
    const void *q, *k, *v;
    void* o;
    int64_t ldq, ldk, ldv, ldo;
    int64_t P;
    int nqt;                      // query tiles per image
    int nkt;                      // key tiles per image
    float scale_log2;
};

constexpr int VA_QT = 64, VA_KT = 32;
constexpr int VA_PPITCH = 80;                                   // bytes per row of the P image (32 bf16 + 16: 16-byte row reads spread over the banks)
template <int C> constexpr int va_pitch() { return C * 2 + 16; }
template <int C> constexpr int va_lds_bytes() { return (VA_QT + VA_KT) * va_pitch<C>() + VA_KT * C * 2 + VA_QT * VA_PPITCH + VA_QT * 4; }

template <int C>
__global__ void __launch_bounds__(256, 1)
vae_attn_kernel(const VaParams p) {
    constexpr int PITCH = va_pitch<C>();
    constexpr int NCH = C / 8;                // 16-byte chunks per row
    constexpr int NQ = VA_QT * NCH / 256;     // chunks per thread of the Q tile
    constexpr int NKV = VA_KT * NCH / 256;    // chunks per thread of a K (V) tile
    constexpr int NCB = C / 128;              // 32-channel blocks per wave
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const Qs = smem;
    char* const Ks = Qs + VA_QT * PITCH;
    char* const Vs = Ks + VA_KT * PITCH;
    char* const Ps = Vs + VA_KT * C * 2;
    float* const Als = (float*)(Ps + VA_QT * VA_PPITCH);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int img = blockIdx.x / p.nqt, qt = blockIdx.x - img * p.nqt;
    const int P = (int)p.P;
    const int64_t row0 = (int64_t)img * p.P;                   // first row of this image
    const int q0 = qt * VA_QT;
    const bf16_t* const kg = (const bf16_t*)p.k;
    const bf16_t* const vg = (const bf16_t*)p.v;

    uint4 kreg[NKV], vreg[NKV];
    auto fetch_kv = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NKV; ++i) {
            const int idx = tid + 256 * i, r = idx / NCH, ch = idx - r * NCH;
            const int key = kt * VA_KT + r;
            const int64_t row = row0 + (key < P ? key : P - 1);
            kreg[i] = *(const uint4*)(kg + row * p.ldk + ch * 8);
            vreg[i] = *(const uint4*)(vg + row * p.ldv + ch * 8);
        }
    };
    auto store_kv = [&](int kt) {
#pragma unroll
        for (int i = 0; i < NKV; ++i) {
            const int idx = tid + 256 * i, r = idx / NCH, ch = idx - r * NCH;
            const uint32_t live = kt * VA_KT + r < P ? 0xffffffffu : 0u;       // a select per word (of values, not of addresses)
            const uint4 kv = kreg[i], vv = vreg[i];
            *(uint4*)(Ks + r * PITCH + ch * 16) = make_uint4(kv.x & live, kv.y & live, kv.z & live, kv.w & live);
            *(uint4*)(Vs + r * (C * 2) + ((ch ^ ((r & 3) << 2)) * 16)) = make_uint4(vv.x & live, vv.y & live, vv.z & live, vv.w & live);
        }
    };

    fetch_kv(0);
    {
        const bf16_t* const qg = (const bf16_t*)p.q;
#pragma unroll
        for (int i = 0; i < NQ; ++i) {
            const int idx = tid + 256 * i, r = idx / NCH, ch = idx - r * NCH;
            const int qr = q0 + r < P ? q0 + r : P - 1;
            *(uint4*)(Qs + r * PITCH + ch * 16) = *(const uint4*)(qg + (row0 + qr) * p.ldq + ch * 8);
        }
    }

    // S phase: lane -> query 16 wave + (lane & 15), keys 16 t + 4 (lane >> 4) + reg of key block t
    const int c16 = lane & 15, g4 = lane >> 4;
    const char* const q_rd = Qs + (16 * wave + c16) * PITCH + g4 * 16;
    const char* const k_rd = Ks + c16 * PITCH + g4 * 16;
    char* const p_wr = Ps + (16 * wave + c16) * VA_PPITCH + g4 * 8;
    // O phase: lane -> query 32 qb + (lane & 31), channels wave C/4 + 32 cb + (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
    const int l31 = lane & 31, half = lane >> 5;
    const int u = lane & 15, g1 = (lane >> 4) & 1;
    const char* const p_rd = Ps + l31 * VA_PPITCH + half * 16;
    // transposing read of V^T: 16-lane group = 4 keys x 16 channels, lane u addresses key (u >> 2), 8-byte piece (u & 3), receives
    // channel u of the group; the 64-byte slot XOR of a row is (row & 3) = (u >> 2) for every row this lane addresses
    int v_off[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
        v_off[cb] = (half * 8 + (u >> 2)) * (C * 2) + (((wave * (C / 4) + cb * 32 + g1 * 16) * 2 + (u & 3) * 8) ^ ((u >> 2) << 6));

    f32x16 acc[NCB][2];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int qb = 0; qb < 2; ++qb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][qb][r] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    for (int kt = 0; kt < p.nkt; ++kt) {
        store_kv(kt);
        __syncthreads();
        if (kt + 1 < p.nkt) fetch_kv(kt + 1);

        // ---- S^T = K Q^T for this wave's 16 queries
        f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < C / 32; ++ks) {
            const bf16x8 qf = *(const bf16x8*)(q_rd + ks * 64);
            const bf16x8 k0 = *(const bf16x8*)(k_rd + ks * 64);
            const bf16x8 k1 = *(const bf16x8*)(k_rd + 16 * PITCH + ks * 64);
            s0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k0, qf, s0, 0, 0, 0);
            s1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(k1, qf, s1, 0, 0, 0);
        }
        float sv[8], mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int key = kt * VA_KT + 16 * (e >> 2) + 4 * g4 + (e & 3);
            sv[e] = key < P ? (e < 4 ? s0[e & 3] : s1[e & 3]) * p.scale_log2 : -INFINITY;
            mx = fmaxf(mx, sv[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);                  // finite: every tile holds at least one key below P
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);      // 0 at the first tile (m_run = -inf)
        m_run = m_new;
        float sum = 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float pv[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                pv[r] = __builtin_amdgcn_exp2f(sv[4 * t + r] - m_new);
                sum += pv[r];
            }
            *(uint2*)(p_wr + t * 32) = pack4(pv);
        }
        sum += __shfl_xor(sum, 16, 64);
        sum += __shfl_xor(sum, 32, 64);
        l_run = l_run * alpha + sum;
        if (g4 == 0) Als[16 * wave + c16] = alpha;
        __syncthreads();

        // ---- O^T = alpha O^T + V^T P^T for this wave's channels
        const float a0 = Als[l31], a1 = Als[32 + l31];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[cb][0][r] *= a0;
                acc[cb][1][r] *= a1;
            }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pf0 = *(const bf16x8*)(p_rd + ks * 32);
            const bf16x8 pf1 = *(const bf16x8*)(p_rd + 32 * VA_PPITCH + ks * 32);
#pragma unroll
            for (int cb = 0; cb < NCB; ++cb) {
                const char* const va = Vs + v_off[cb] + ks * (16 * C * 2);
                const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va));
                const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(va + 4 * C * 2));
                const bf16x8 vf = (bf16x8)__builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                acc[cb][0] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf0, acc[cb][0], 0, 0, 0);
                acc[cb][1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf1, acc[cb][1], 0, 0, 0);
            }
        }
        __syncthreads();                                        // K, V, P and alpha are free for the next tile
    }

    if (g4 == 0) Als[16 * wave + c16] = 1.f / l_run;
    __syncthreads();
    bf16_t* const og = (bf16_t*)p.o;
#pragma unroll
    for (int qb = 0; qb < 2; ++qb) {
        const int qr = q0 + 32 * qb + l31;
        if (qr >= P) continue;
        const float inv = Als[32 * qb + l31];
        bf16_t* const orow = og + (row0 + qr) * p.ldo + wave * (C / 4) + 4 * half;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float f[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) f[r] = acc[cb][qb][4 * i + r] * inv;
                *(uint2*)(orow + cb * 32 + 8 * i) = pack4(f);
            }
    }
}

// ---- fp32 accuracy path
constexpr int VF_QT = 16, VF_KT = 32;
template <int C> constexpr int vf_lds_bytes() { return (VF_QT * C + VF_KT * (C + 4) + VF_QT * VF_KT) * 4; }

template <int C>
__global__ void __launch_bounds__(256)
vae_attn_f32_kernel(const VaParams p) {
    constexpr int KP = C + 4;                 // floats per row of the K / V buffer
    constexpr int NCH = C / 4;                // float4 chunks per row
    constexpr int NE = C / 64;                // float4 output chunks per lane
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const Qs = (float*)smem;
    float* const KVs = Qs + VF_QT * C;
    float* const Ps = KVs + VF_KT * KP;

    const int tid = threadIdx.x;
    const int qi = tid >> 4, j = tid & 15;
    const int img = blockIdx.x / p.nqt, qt = blockIdx.x - img * p.nqt;
    const int P = (int)p.P;
    const int64_t row0 = (int64_t)img * p.P;
    const int q0 = qt * VF_QT;

    for (int idx = tid; idx < VF_QT * NCH; idx += 256) {
        const int r = idx / NCH, ch = idx - r * NCH;
        const int qr = q0 + r < P ? q0 + r : P - 1;
        *(float4*)(Qs + r * C + ch * 4) = *(const float4*)((const float*)p.q + (row0 + qr) * p.ldq + ch * 4);
    }
    auto load_tile = [&](const float* src, int64_t ld, int kt) {          // rows past P: zeros (selection), read from row P - 1
        for (int idx = tid; idx < VF_KT * NCH; idx += 256) {
            const int r = idx / NCH, ch = idx - r * NCH;
            const int key = kt * VF_KT + r;
            const float4 x = *(const float4*)(src + (row0 + (key < P ? key : P - 1)) * ld + ch * 4);
            const bool live = key < P;
            *(float4*)(KVs + r * KP + ch * 4) = make_float4(live ? x.x : 0.f, live ? x.y : 0.f, live ? x.z : 0.f, live ? x.w : 0.f);
        }
    };

    float4 acc[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) acc[e] = make_float4(0.f, 0.f, 0.f, 0.f);
    float m_run = -INFINITY, l_run = 0.f;

    for (int kt = 0; kt < p.nkt; ++kt) {
        load_tile((const float*)p.k, p.ldk, kt);
        __syncthreads();
        float s0 = 0.f, s1 = 0.f;
        {
            const float* const qr = Qs + qi * C;
            const float* const k0 = KVs + j * KP;
            const float* const k1 = KVs + (j + 16) * KP;
            for (int c = 0; c < C; c += 4) {
                const float4 a = *(const float4*)(qr + c), b0 = *(const float4*)(k0 + c), b1 = *(const float4*)(k1 + c);
                s0 = fmaf(a.x, b0.x, s0); s0 = fmaf(a.y, b0.y, s0); s0 = fmaf(a.z, b0.z, s0); s0 = fmaf(a.w, b0.w, s0);
                s1 = fmaf(a.x, b1.x, s1); s1 = fmaf(a.y, b1.y, s1); s1 = fmaf(a.z, b1.z, s1); s1 = fmaf(a.w, b1.w, s1);
            }
        }
        s0 = kt * VF_KT + j < P ? s0 * p.scale_log2 : -INFINITY;
        s1 = kt * VF_KT + j + 16 < P ? s1 * p.scale_log2 : -INFINITY;
        float mx = fmaxf(s0, s1);
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = exp2f(m_run - m_new);
        m_run = m_new;
        const float p0 = exp2f(s0 - m_new), p1 = exp2f(s1 - m_new);
        float sum = p0 + p1;
#pragma unroll
        for (int o = 8; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
        l_run = l_run * alpha + sum;
        Ps[qi * VF_KT + j] = p0;
        Ps[qi * VF_KT + j + 16] = p1;
        __syncthreads();                                        // every lane is done with K
        load_tile((const float*)p.v, p.ldv, kt);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < NE; ++e) { acc[e].x *= alpha; acc[e].y *= alpha; acc[e].z *= alpha; acc[e].w *= alpha; }
        for (int key = 0; key < VF_KT; ++key) {
            const float pk = Ps[qi * VF_KT + key];
            const float* const vr = KVs + key * KP + 4 * j;
#pragma unroll
            for (int e = 0; e < NE; ++e) {
                const float4 x = *(const float4*)(vr + 64 * e);
                acc[e].x = fmaf(pk, x.x, acc[e].x); acc[e].y = fmaf(pk, x.y, acc[e].y);
                acc[e].z = fmaf(pk, x.z, acc[e].z); acc[e].w = fmaf(pk, x.w, acc[e].w);
            }
        }
        __syncthreads();                                        // V and P are free for the next tile
    }
    if (q0 + qi < P) {
        float* const orow = (float*)p.o + (row0 + q0 + qi) * p.ldo + 4 * j;
#pragma unroll
        for (int e = 0; e < NE; ++e)
            *(float4*)(orow + 64 * e) = make_float4(acc[e].x / l_run, acc[e].y / l_run, acc[e].z / l_run, acc[e].w / l_run);
    }
}

template <auto Kernel>
int va_launch(const VaParams& p, int64_t nblk, int lds, void* stream) {
    // above 64 KiB of dynamic LDS a kernel needs its limit raised: once per (kernel, device), see dwm_allow_dynamic_lds
    const hipError_t e = dwm_allow_dynamic_lds<Kernel>(lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(Kernel, dim3((unsigned)nblk), dim3(256), (size_t)lds, (hipStream_t)stream, p);
    return dwm_launch_status();
}

int vae_attention_impl(const dwm_vae_attn_args* a, void* stream, bool f32) {
    if (a == nullptr || a->q == nullptr || a->k == nullptr || a->v == nullptr || a->out == nullptr) return DWM_EINVAL;
    if (a->I <= 0 || a->P <= 0 || a->C <= 0) return DWM_EINVAL;
    if (a->C != 128 && a->C != 256 && a->C != 512) return DWM_EUNSUPPORTED;
    if (a->ldq < a->C || a->ldk < a->C || a->ldv < a->C || a->ldo < a->C) return DWM_EINVAL;
    const int gran = f32 ? 4 : 8;                              // elements per 16 bytes
    if (a->ldq % gran != 0 || a->ldk % gran != 0 || a->ldv % gran != 0 || a->ldo % gran != 0) return DWM_EALIGN;
    if (!dwm_aligned16(a->q) || !dwm_aligned16(a->k) || !dwm_aligned16(a->v) || !dwm_aligned16(a->out)) return DWM_EALIGN;
    const int qtile = f32 ? VF_QT : VA_QT, ktile = f32 ? VF_KT : VA_KT;
    if (a->P > (1ll << 30)) return DWM_EUNSUPPORTED;           // key / query indices are int inside an image; row offsets are 64-bit
    const int64_t nqt = (a->P + qtile - 1) / qtile;
    if (a->I > (1ll << 31) / nqt - 1) return DWM_EUNSUPPORTED;   // one-dimensional grid
    VaParams p;
    p.q = a->q; p.k = a->k; p.v = a->v; p.o = a->out;
    p.ldq = a->ldq; p.ldk = a->ldk; p.ldv = a->ldv; p.ldo = a->ldo;
    p.P = a->P;
    p.nqt = (int)nqt;
    p.nkt = (int)((a->P + ktile - 1) / ktile);
    p.scale_log2 = a->scale * 1.4426950408889634f;
    const int64_t nblk = a->I * nqt;
    if (f32) {
        if (a->C == 128) return va_launch<vae_attn_f32_kernel<128>>(p, nblk, vf_lds_bytes<128>(), stream);
        if (a->C == 256) return va_launch<vae_attn_f32_kernel<256>>(p, nblk, vf_lds_bytes<256>(), stream);
        return va_launch<vae_attn_f32_kernel<512>>(p, nblk, vf_lds_bytes<512>(), stream);
    }
    if (a->C == 128) return va_launch<vae_attn_kernel<128>>(p, nblk, va_lds_bytes<128>(), stream);
    if (a->C == 256) return va_launch<vae_attn_kernel<256>>(p, nblk, va_lds_bytes<256>(), stream);
    return va_launch<vae_attn_kernel<512>>(p, nblk, va_lds_bytes<512>(), stream);
}

}  // namespace

extern "C" int dwm_vae_attention(const dwm_vae_attn_args* args, void* stream) { return vae_attention_impl(args, stream, false); }
extern "C" int dwm_vae_attention_f32(const dwm_vae_attn_args* args, void* stream) { return vae_attention_impl(args, stream, true); }
