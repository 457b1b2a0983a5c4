// Gradient conditioning of the optimizer step in one read of the gradients: the global L2 norm of a LIST of fp32 tensors (after a
// scale factor), the non-finite check of torch.amp.GradScaler, and the coefficient torch.nn.utils.clip_grad_norm_ would multiply by
// - handed to dwm_adamw_multi / dwm_adamw8_multi as their grad_scale, so the gradients are never rewritten.  (include/dwm_hip.h,
// "Gradient norm, clip coefficient and non-finite check")
//
// Tables as in dwm_adamw_multi: workgroup b owns elements [block_start[b], min(block_start[b] + chunk, n)) of tensor block_item[b].
// No atomics anywhere: one fp64 partial and one flag word per workgroup, summed by a second one-workgroup kernel in a fixed order,
// so the four output floats are the same bits on every launch.
#include "common.h"

constexpr int GN_THREADS = 256;
constexpr int GN_UNROLL = 4;                 // independent 16-byte loads in flight per lane
// The gradient pointers come out of the item table, so the compiler knows no address space for them and would emit flat_*
// accesses (which also occupy the LDS counter); they are device memory by contract: global_load / global_store.
typedef __attribute__((address_space(1))) float gn_gf32;
typedef __attribute__((address_space(1))) f32x4 gn_gf32x4;

// elements [i0, i1) of g split on the 16-byte grid of the ADDRESS (a DDP bucket view starts anywhere, a partial last chunk ends
// anywhere): `head` scalar elements, `nvec` aligned float4, `tail` scalar elements.  Nothing outside [g + i0, g + i1) is touched.
struct GnSpan {
    int head, tail;
    int64_t nvec;
    gn_gf32* body;                           // 16-byte aligned, = g + i0 + head
};
DWM_DEVINL GnSpan gn_span(gn_gf32* g, int64_t i0, int64_t i1) {
    GnSpan s;
    const int64_t len = i1 - i0;
    const int64_t to_grid = (int64_t)((0u - (uint32_t)((uintptr_t)(g + i0) >> 2)) & 3u);
    s.head = (int)(to_grid < len ? to_grid : len);
    s.nvec = (len - s.head) >> 2;
    s.tail = (int)(len - s.head - 4 * s.nvec);
    s.body = g + i0 + s.head;
    return s;
}

DWM_DEVINL uint32_t gn_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

DWM_DEVINL double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// One workgroup, one chunk.  Lane t takes the float4 t, t + 256, ... of the chunk's aligned body; component j of every float4
// goes (times pre_scale, squared, by one fma) into accumulator j, so an accumulator receives at most chunk / 1024 squares; the at
// most three head and three tail elements go into a fifth accumulator (at most two per lane).
__global__ void __launch_bounds__(GN_THREADS)
grad_sumsq_multi_kernel(const dwm_grad_item* __restrict__ items, const int32_t* __restrict__ block_item,
                        const int64_t* __restrict__ block_start, int64_t chunk, float pre_scale, double* __restrict__ partials,
                        uint32_t* __restrict__ flags) {
    __shared__ double wsum[GN_THREADS / 64];
    __shared__ uint32_t wflag[GN_THREADS / 64];
    int64_t i0, i1;
    const dwm_grad_item it = dwm_list_chunk(items, block_item, block_start, chunk, i0, i1);
    const int t = threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, edge = 0.f;
    uint32_t bad = 0;
    if (i0 < i1) {
        gn_gf32* const g = (gn_gf32*)it.g;
        const GnSpan s = gn_span(g, i0, i1);
        const gn_gf32x4* const body = (const gn_gf32x4*)s.body;
        auto take = [&](const f32x4 v) {
            bad |= gn_nonfinite(v.x) | gn_nonfinite(v.y) | gn_nonfinite(v.z) | gn_nonfinite(v.w);
            const float x = v.x * pre_scale, y = v.y * pre_scale, z = v.z * pre_scale, w = v.w * pre_scale;
            a0 = fmaf(x, x, a0); a1 = fmaf(y, y, a1); a2 = fmaf(z, z, a2); a3 = fmaf(w, w, a3);
        };
        int64_t v = t;
        for (; v + (GN_UNROLL - 1) * GN_THREADS < s.nvec; v += GN_UNROLL * GN_THREADS) {
            f32x4 r[GN_UNROLL];
#pragma unroll
            for (int u = 0; u < GN_UNROLL; ++u) r[u] = body[v + u * GN_THREADS];
#pragma unroll
            for (int u = 0; u < GN_UNROLL; ++u) take(r[u]);
        }
        for (; v < s.nvec; v += GN_THREADS) take(body[v]);
        if (t < s.head) {
            const float e = g[i0 + t];
            bad |= gn_nonfinite(e);
            const float x = e * pre_scale;
            edge = fmaf(x, x, edge);
        }
        if (t < s.tail) {
            const float e = s.body[4 * s.nvec + t];
            bad |= gn_nonfinite(e);
            const float x = e * pre_scale;
            edge = fmaf(x, x, edge);
        }
    }
    double sum = (((double)a0 + (double)a1) + ((double)a2 + (double)a3)) + (double)edge;
    sum = wave_sum_f64(sum);
    const uint32_t any = __ballot(bad != 0) != 0 ? 1u : 0u;
    if ((t & 63) == 0) {
        wsum[t >> 6] = sum;
        wflag[t >> 6] = any;
    }
    __syncthreads();
    if (t == 0) {
        partials[blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        flags[blockIdx.x] = wflag[0] | wflag[1] | wflag[2] | wflag[3];
    }
}

// One workgroup: thread t sums partials t, t + 256, ... in that order, a fixed LDS tree sums the 256 threads, thread 0 writes
// out[0] = norm, out[1] = pre_scale * min(1, max_norm / (norm + 1e-6)) (fp32 arithmetic from the fp32 norm: clip_grad_norm_'s
// formula; max_norm <= 0: pre_scale), out[2] = 1 if any element was inf / nan, out[3] = 0.
__global__ void __launch_bounds__(GN_THREADS)
grad_finish_kernel(const double* __restrict__ partials, const uint32_t* __restrict__ flags, int64_t n_blocks, float pre_scale,
                   float max_norm, float* __restrict__ out) {
    __shared__ double ssum[GN_THREADS];
    __shared__ uint32_t sflag[GN_THREADS];
    const int t = threadIdx.x;
    double s = 0.0;
    uint32_t f = 0;
    for (int64_t i = t; i < n_blocks; i += GN_THREADS) {
        s += partials[i];
        f |= flags[i];
    }
    ssum[t] = s;
    sflag[t] = f;
    __syncthreads();
    for (int w = GN_THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            ssum[t] += ssum[t + w];
            sflag[t] |= sflag[t + w];
        }
        __syncthreads();
    }
    if (t == 0) {
        const float norm = (float)sqrt(ssum[0]);
        float coef = pre_scale;
        if (max_norm > 0.f) {
            const float q = max_norm / (norm + 1e-6f);
            coef = pre_scale * (q < 1.f ? q : 1.f);
        }
        out[0] = norm;
        out[1] = coef;
        out[2] = sflag[0] != 0 ? 1.f : 0.f;
        out[3] = 0.f;
    }
}

// g *= coef in place over the same tables (the stand-alone clip for callers with an optimizer of their own)
__global__ void __launch_bounds__(GN_THREADS)
grad_scale_multi_kernel(const dwm_grad_item* __restrict__ items, const int32_t* __restrict__ block_item,
                        const int64_t* __restrict__ block_start, int64_t chunk, float coef) {
    int64_t i0, i1;
    const dwm_grad_item it = dwm_list_chunk(items, block_item, block_start, chunk, i0, i1);
    if (i0 >= i1) return;
    const int t = threadIdx.x;
    gn_gf32* const g = (gn_gf32*)it.g;
    const GnSpan s = gn_span(g, i0, i1);
    gn_gf32x4* const body = (gn_gf32x4*)s.body;
    int64_t v = t;
    for (; v + (GN_UNROLL - 1) * GN_THREADS < s.nvec; v += GN_UNROLL * GN_THREADS) {
        f32x4 r[GN_UNROLL];
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u) r[u] = body[v + u * GN_THREADS];
#pragma unroll
        for (int u = 0; u < GN_UNROLL; ++u)
            body[v + u * GN_THREADS] = r[u] * coef;
    }
    for (; v < s.nvec; v += GN_THREADS) {
        const f32x4 r = body[v];
        body[v] = r * coef;
    }
    if (t < s.head) g[i0 + t] *= coef;
    if (t < s.tail) s.body[4 * s.nvec + t] *= coef;
}

// chunk: a multiple of 1024 (one float4 per lane and round) of at most 2^18, so that one fp32 accumulator receives at most 256 squares
static bool gn_bad_tables(const dwm_grad_item* items, const int32_t* block_item, const int64_t* block_start, int64_t n_blocks,
                          int64_t chunk) {
    return dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk) || chunk % 1024 != 0 || chunk > (1ll << 18);
}

extern "C" int dwm_grad_sumsq_multi(const dwm_grad_item* items, const int32_t* block_item, const int64_t* block_start,
                                    int64_t n_blocks, int64_t chunk, float pre_scale, float max_norm, double* partials,
                                    uint32_t* flags, float* out, void* stream) {
    if (gn_bad_tables(items, block_item, block_start, n_blocks, chunk) || !partials || !flags || !out) return DWM_EINVAL;
    hipLaunchKernelGGL(grad_sumsq_multi_kernel, dim3((unsigned)n_blocks), dim3(GN_THREADS), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, pre_scale, partials, flags);
    hipLaunchKernelGGL(grad_finish_kernel, dim3(1), dim3(GN_THREADS), 0, (hipStream_t)stream, (const double*)partials,
                       (const uint32_t*)flags, n_blocks, pre_scale, max_norm, out);
    return dwm_launch_status();
}

extern "C" int dwm_grad_scale_multi(const dwm_grad_item* items, const int32_t* block_item, const int64_t* block_start,
                                    int64_t n_blocks, int64_t chunk, float coef, void* stream) {
    if (gn_bad_tables(items, block_item, block_start, n_blocks, chunk)) return DWM_EINVAL;
    hipLaunchKernelGGL(grad_scale_multi_kernel, dim3((unsigned)n_blocks), dim3(GN_THREADS), 0, (hipStream_t)stream, items, block_item,
                       block_start, chunk, coef);
    return dwm_launch_status();
}
