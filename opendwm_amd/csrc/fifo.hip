// In-place "slide by one frame" of a LIST of dense buffers [outer][T][inner_bytes] in one launch (dwm_fifo_slide_multi, include/dwm_hip.h):
//   buf[o][t] = buf[o][t + 1] for t < T - 1,   buf[o][T - 1] = fresh[o % fresh_outer]   (convert: fresh fp32 -> bf16, nearest even).
// The FIFO step of a persistent streaming session (pipeline.CTSDDenoiser.advance_stream): latents, model input, every per-frame
// condition and the cached adapter residuals move by one frame without a second buffer.
//
// A row of inner_bytes is cut into pieces of W bytes (16 where the row size and both pointers allow it, else 4, else 2); column
// (o, piece) - the T pieces at one offset of one outer index - is owned by exactly ONE thread, which walks t upward and loads frame
// t + 1 before it stores frame t.  No other thread reads or writes that column, so the shift needs no barrier and no atomics and its
// result does not depend on scheduling.  The loads of FIFO_DEPTH frames (and of the fresh piece) are issued before the first store, so
// a column costs ~T / FIFO_DEPTH memory latencies instead of T.  Tables as in dwm_adamw_multi: workgroup b owns columns
// [block_start[b], min(block_start[b] + chunk, n)) of item block_item[b]; neighbouring threads own neighbouring pieces (coalesced).
#include "common.h"

namespace {

constexpr int FIFO_DEPTH = 4;                     // frames in flight per column
static_assert(FIFO_DEPTH == 4, "fifo_slide_columns is written out for four frames (named registers: arrays went to scratch)");

// piece width of an item: what the host checks `n` against and the kernel walks by
__host__ __device__ __forceinline__ int fifo_piece_bytes(const void* buf, const void* fresh, int64_t inner_bytes) {
    const uintptr_t a = (uintptr_t)buf | (uintptr_t)fresh | (uintptr_t)inner_bytes;
    return (a & 15u) == 0 ? 16 : (a & 3u) == 0 ? 4 : 2;
}

// the piece of the fresh frame that lands at byte `off` of buffer row o (row = the fresh row o % fresh_outer)
template <typename V>
DWM_DEVINL V fifo_fresh(const char* fresh, bool convert, int64_t off) {
    if (!convert) return *(const V*)(fresh + off);
    const float* f = (const float*)(fresh + 2 * off);                  // sizeof(V) / 2 fp32 values
    if constexpr (sizeof(V) == 16) {
        float x[8];
        load8<float>(f, x);
        return pack8(x);
    } else if constexpr (sizeof(V) == 4) {
        return pack_bf16x2(f[0], f[1]);
    } else {
        return f32_to_bf16(f[0]);
    }
}

template <typename V>
DWM_DEVINL void fifo_slide_columns(char* buf, const char* fresh, int64_t row, int64_t T, uint32_t fresh_outer, bool convert,
                                   int64_t i0, int64_t i1) {
    const uint32_t ppr = (uint32_t)(row / (int64_t)sizeof(V));                        // pieces per row; n = outer * ppr < 2^31
    for (int64_t c = i0 + threadIdx.x; c < i1; c += 256) {
        const uint32_t o = (uint32_t)c / ppr, piece = (uint32_t)c - o * ppr;
        char* col = buf + (int64_t)o * T * row + (int64_t)piece * sizeof(V);  // frame t of the column: col + t * row
        const V last = fifo_fresh<V>(fresh, convert, (int64_t)(o % fresh_outer) * row + (int64_t)piece * sizeof(V));
        int64_t t = 0;
        for (; t + FIFO_DEPTH <= T - 1; t += FIFO_DEPTH) {                             // four frames' loads, then their stores
            const V v0 = *(const V*)(col + (t + 1) * row), v1 = *(const V*)(col + (t + 2) * row);
            const V v2 = *(const V*)(col + (t + 3) * row), v3 = *(const V*)(col + (t + 4) * row);
            *(V*)(col + t * row) = v0;
            *(V*)(col + (t + 1) * row) = v1;
            *(V*)(col + (t + 2) * row) = v2;
            *(V*)(col + (t + 3) * row) = v3;
        }
        const int64_t left = T - 1 - t;                                                // < FIFO_DEPTH frames
        if (left > 0) {
            const V v0 = *(const V*)(col + (t + 1) * row);
            const V v1 = left > 1 ? *(const V*)(col + (t + 2) * row) : v0;
            const V v2 = left > 2 ? *(const V*)(col + (t + 3) * row) : v0;
            *(V*)(col + t * row) = v0;
            if (left > 1) *(V*)(col + (t + 1) * row) = v1;
            if (left > 2) *(V*)(col + (t + 2) * row) = v2;
        }
        *(V*)(col + (T - 1) * row) = last;
    }
}

__global__ void __launch_bounds__(256)
fifo_slide_multi_kernel(const dwm_fifo_item* __restrict__ items, int32_t n_items, const int32_t* __restrict__ block_item,
                        const int64_t* __restrict__ block_start, int64_t chunk) {
    const int32_t bi = block_item[blockIdx.x];
    if (bi < 0 || bi >= n_items) return;                                               // a table that disagrees with the list writes nothing
    const dwm_fifo_item* __restrict__ it = items + bi;                                 // (field by field: the 64-byte struct stays out of scratch)
    const int64_t n = it->n, i0 = block_start[blockIdx.x];
    if (i0 < 0) return;
    const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
    char* buf = (char*)it->buf;
    const char* fresh = (const char*)it->fresh;
    const int64_t row = it->inner_bytes, T = it->T;
    const uint32_t fo = (uint32_t)it->fresh_outer;
    const bool convert = it->convert != 0;
    const int w = fifo_piece_bytes(buf, fresh, row);
    if (w == 16) fifo_slide_columns<uint4>(buf, fresh, row, T, fo, convert, i0, i1);
    else if (w == 4) fifo_slide_columns<uint32_t>(buf, fresh, row, T, fo, convert, i0, i1);
    else fifo_slide_columns<uint16_t>(buf, fresh, row, T, fo, convert, i0, i1);
}

}  // namespace

extern "C" int dwm_fifo_slide_multi(const dwm_fifo_item* host_items, int64_t n_items, const dwm_fifo_item* items,
                                    const int32_t* block_item, const int64_t* block_start, int64_t n_blocks, int64_t chunk,
                                    void* stream) {
    if (host_items == nullptr || n_items <= 0 || dwm_bad_list_tables(items, block_item, block_start, n_blocks, chunk)) return DWM_EINVAL;
    if (chunk % 256 != 0 || chunk > (1ll << 20)) return DWM_EINVAL;
    if (n_items >= (1ll << 20)) return DWM_EUNSUPPORTED;
    int64_t blocks = 0;
    for (int64_t i = 0; i < n_items; ++i) {
        const dwm_fifo_item& it = host_items[i];
        if (it.buf == nullptr || it.fresh == nullptr || it.outer <= 0 || it.T <= 0 || it.inner_bytes <= 0 || it.fresh_outer <= 0)
            return DWM_EINVAL;
        if (it.inner_bytes % 2 != 0 || it.outer % it.fresh_outer != 0 || (it.convert != 0 && it.convert != 1)) return DWM_EINVAL;
        if ((((uintptr_t)it.buf) & 1u) || (((uintptr_t)it.fresh) & (it.convert ? 3u : 1u))) return DWM_EALIGN;
        if (it.outer >= (1ll << 31) || it.T >= (1ll << 31) || it.inner_bytes >= (1ll << 40)) return DWM_EUNSUPPORTED;
        const __int128 bytes = (__int128)it.outer * it.T * it.inner_bytes;
        const __int128 cols = (__int128)it.outer * (it.inner_bytes / fifo_piece_bytes(it.buf, it.fresh, it.inner_bytes));
        if (bytes >= ((__int128)1 << 46) || cols >= (1ll << 31)) return DWM_EUNSUPPORTED;
        if (it.n != (int64_t)cols) return DWM_EINVAL;
        const uintptr_t b0 = (uintptr_t)it.buf, b1 = b0 + (uintptr_t)bytes;
        const uintptr_t f0 = (uintptr_t)it.fresh, f1 = f0 + (uintptr_t)(it.fresh_outer * it.inner_bytes * (it.convert ? 2 : 1));
        if (f0 < b1 && b0 < f1) return DWM_EINVAL;                                     // fresh inside the buffer it is shifted into
        blocks += (it.n + chunk - 1) / chunk;
    }
    if (blocks != n_blocks) return DWM_EINVAL;
    hipLaunchKernelGGL(fifo_slide_multi_kernel, dim3((unsigned)n_blocks), dim3(256), 0, (hipStream_t)stream, items, (int32_t)n_items,
                       block_item, block_start, chunk);
    return dwm_launch_status();
}
