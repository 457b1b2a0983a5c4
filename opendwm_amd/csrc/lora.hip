// Low-rank adapters (opendwm_amd/lora.py; include/dwm_hip.h, "Low-rank adapters"): an adapted weight is
// W + scale * B A, W [N, K], A [r, K], B [N, r], r <= 64.  Two entry points over a LIST of weights (item array + block tables, as
// dwm_adamw_multi):
//   dwm_lora_merge_multi    out = W + scale * B A, as the bf16 compute copy of a training step (the merge) or in the weight's own
//                           type (the fold).  Bandwidth bound: one read of W, one write of out; A and the tile's rows of B sit in LDS.
//   dwm_lora_project_multi  dA (+)= scale * B^T G, dB (+)= scale * G A^T from the weight gradient G the block Functions produce.
// G IS READ TWICE, by two kernels of two shapes: dA sums over rows (a thread owns 4 columns and walks down), dB over columns (a
// thread owns a row and walks along).  One kernel for both would hold r x 128 + 32 x r partial sums per tile and reduce each across
// the workgroup; G is 9 MB per 1536 x 1536 weight and the two launches run back to back, so the second read mostly comes from the
// Infinity Cache - the simple form was chosen and its cost is in the measurement (DESIGN s26).
// No atomics: a dA element is the ascending sum of its row chunks' partials (a finishing launch adds them in order), a dB element has
// one owner that walks k in order.  The item pointers come out of a table, so they are cast to global (see gradnorm.hip).
#include "common.h"

constexpr int LR_THREADS = 256;
constexpr int LR_TN = 32;                    // rows of a tile
constexpr int LR_TK = 128;                   // columns of a tile: 32 lanes x 4
constexpr int LR_RMAX = 64;
constexpr int LR_DA_ROWS = 512;              // rows behind one dA partial
constexpr int LR_GPAD = LR_TK + 4;           // row pitch of the dB kernel's G tile: lane = row there, 4 floats of skew per row

typedef __attribute__((ext_vector_type(2))) uint32_t lr_u32x2;
typedef __attribute__((address_space(1))) float lr_gf32;
typedef __attribute__((address_space(1))) f32x4 lr_gf32x4;
typedef __attribute__((address_space(1))) bf16_t lr_gbf16;
typedef __attribute__((address_space(1))) lr_u32x2 lr_gu32x2;

// 4 consecutive elements at element index i (i % 4 == 0) of an fp32 (16-byte access) or bf16 (8-byte access) tensor
template <bool BF> DWM_DEVINL f32x4 lr_load4(const void* base, int64_t i) {
    if constexpr (BF) {
        const lr_u32x2 v = *(const lr_gu32x2*)((const lr_gbf16*)base + i);
        return (f32x4){bf16lo(v.x), bf16hi(v.x), bf16lo(v.y), bf16hi(v.y)};
    } else {
        return *(const lr_gf32x4*)((const lr_gf32*)base + i);
    }
}
template <bool BF> DWM_DEVINL void lr_store4(void* base, int64_t i, const f32x4 v) {
    if constexpr (BF) {
        *(lr_gu32x2*)((lr_gbf16*)base + i) = (lr_u32x2){pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w)};
    } else {
        *(lr_gf32x4*)((lr_gf32*)base + i) = v;
    }
}

DWM_DEVINL dwm_lora_item lr_item(const dwm_lora_item* __restrict__ items, const int32_t* __restrict__ block_item,
                                 const int64_t* __restrict__ block_start, int64_t& tile) {
    tile = block_start[blockIdx.x];
    return items[block_item[blockIdx.x]];
}

// rows [row0, row_end) x columns [k0, k0 + 128) of A-shaped or G-shaped data -> an LDS tile of `rows` x 128 floats with row pitch
// `pitch`, zero where the source has no element
template <bool BF>
DWM_DEVINL void lr_stage(float* tile, int pitch, int rows, const void* src, int64_t row0, int64_t row_end, int64_t k0, int64_t K) {
    for (int e = threadIdx.x; e < rows * (LR_TK / 4); e += LR_THREADS) {
        const int row = e >> 5, c = (e & 31) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + row < row_end && k0 + c < K) v = lr_load4<BF>(src, (row0 + row) * K + k0 + c);
        *(f32x4*)(tile + row * pitch + c) = v;
    }
}

// ---------------------------------------------------------------------------------------------------------------- merge / fold
// Thread (cg = t & 31, rg = t >> 5) owns columns k0 + 4 cg .. + 3 of rows n0 + 4 rg .. + 3: per j one 16-byte read of A's tile and one
// of the transposed B tile (both broadcast within a half wave), 16 fmas.
template <bool WBF, bool OBF>
DWM_DEVINL void lr_merge_tile(const dwm_lora_item& it, int64_t tile, float (*As)[LR_TK], float (*Bt)[LR_TN]) {
    const int t = threadIdx.x, r = it.r;
    const int64_t N = it.N, K = it.K;
    const int64_t ctiles = (K + LR_TK - 1) / LR_TK;
    const int64_t n0 = (tile / ctiles) * LR_TN, k0 = (tile % ctiles) * LR_TK;
    lr_stage<false>(&As[0][0], LR_TK, r, it.a, 0, r, k0, K);
    const lr_gf32* const b = (const lr_gf32*)it.b;
    for (int e = t; e < LR_TN * r; e += LR_THREADS) {
        const int row = e / r, j = e - row * r;
        Bt[j][row] = n0 + row < N ? b[(n0 + row) * r + j] : 0.f;
    }
    __syncthreads();
    const int cg = t & 31, rg = t >> 5;
    f32x4 acc[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) acc[rr] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < r; ++j) {
        const f32x4 a = *(const f32x4*)&As[j][cg * 4];
        const f32x4 bv = *(const f32x4*)&Bt[j][rg * 4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
#pragma unroll
            for (int c = 0; c < 4; ++c) acc[rr][c] = fmaf(bv[rr], a[c], acc[rr][c]);
        }
    }
    const int64_t k = k0 + cg * 4;
    if (k >= K) return;
    const float s = it.scale;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int64_t n = n0 + rg * 4 + rr;
        if (n >= N) break;
        const f32x4 w = lr_load4<WBF>(it.w, n * K + k);
        f32x4 v;
#pragma unroll
        for (int c = 0; c < 4; ++c) v[c] = fmaf(s, acc[rr][c], w[c]);
        lr_store4<OBF>(it.out, n * K + k, v);
    }
}

__global__ void __launch_bounds__(LR_THREADS)
lora_merge_multi_kernel(const dwm_lora_item* __restrict__ items, const int32_t* __restrict__ block_item,
                        const int64_t* __restrict__ block_start) {
    __shared__ __attribute__((aligned(16))) float As[LR_RMAX][LR_TK];
    __shared__ __attribute__((aligned(16))) float Bt[LR_RMAX][LR_TN];
    int64_t tile;
    const dwm_lora_item it = lr_item(items, block_item, block_start, tile);
    switch (it.flags & 3) {
        case 0: lr_merge_tile<false, false>(it, tile, As, Bt); break;
        case 1: lr_merge_tile<true, false>(it, tile, As, Bt); break;
        case 2: lr_merge_tile<false, true>(it, tile, As, Bt); break;
        default: lr_merge_tile<true, true>(it, tile, As, Bt); break;
    }
}

// --------------------------------------------------------------------------------------------------------------------- project
// dA partials.  Thread (cg = t & 31, jg = t >> 5) owns columns k0 + 4 cg .. + 3 of the jt = ceil(r / 8) factors j0 = jg jt ...: it walks
// down the chunk's rows, 32 at a time through LDS.
template <bool GBF>
DWM_DEVINL void lr_da_tile(const dwm_lora_item& it, int64_t tile, float (*Gs)[LR_TK], float (*Bs)[LR_RMAX]) {
    const int t = threadIdx.x, r = it.r;
    const int64_t N = it.N, K = it.K;
    const int64_t ctiles = (K + LR_TK - 1) / LR_TK;
    const int64_t rc = tile / ctiles, k0 = (tile % ctiles) * LR_TK;
    const int64_t nb = rc * LR_DA_ROWS, ne = nb + LR_DA_ROWS < N ? nb + LR_DA_ROWS : N;
    const int jt = (r + 7) >> 3, cg = t & 31, j0 = (t >> 5) * jt;
    const lr_gf32* const b = (const lr_gf32*)it.b;
    f32x4 acc[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) acc[jj] = (f32x4){0.f, 0.f, 0.f, 0.f};
    for (int64_t ns = nb; ns < ne; ns += LR_TN) {
        lr_stage<GBF>(&Gs[0][0], LR_TK, LR_TN, it.w, ns, ne, k0, K);
        for (int e = t; e < LR_TN * r; e += LR_THREADS) {
            const int row = e / r, j = e - row * r;
            Bs[row][j] = ns + row < ne ? b[(ns + row) * r + j] : 0.f;
        }
        __syncthreads();
        for (int n = 0; n < LR_TN; ++n) {
            const f32x4 g = *(const f32x4*)&Gs[n][cg * 4];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                if (jj < jt && j0 + jj < r) {
                    const float bv = Bs[n][j0 + jj];
#pragma unroll
                    for (int c = 0; c < 4; ++c) acc[jj][c] = fmaf(bv, g[c], acc[jj][c]);
                }
            }
        }
        __syncthreads();
    }
    const int64_t k = k0 + cg * 4;
    if (k >= K) return;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int j = j0 + jj;
        if (jj < jt && j < r) lr_store4<false>(it.ws, (rc * r + j) * K + k, acc[jj]);
    }
}

__global__ void __launch_bounds__(LR_THREADS)
lora_da_kernel(const dwm_lora_item* __restrict__ items, const int32_t* __restrict__ block_item, const int64_t* __restrict__ block_start) {
    __shared__ __attribute__((aligned(16))) float Gs[LR_TN][LR_TK];
    __shared__ __attribute__((aligned(16))) float Bs[LR_TN][LR_RMAX];
    int64_t tile;
    const dwm_lora_item it = lr_item(items, block_item, block_start, tile);
    if (it.flags & 1)
        lr_da_tile<true>(it, tile, Gs, Bs);
    else
        lr_da_tile<false>(it, tile, Gs, Bs);
}

// dA = scale * (the partials of its row chunks added in ascending order) (+ dA): elements [i0, i1) of the r * K of one item
__global__ void __launch_bounds__(LR_THREADS)
lora_da_finish_kernel(const dwm_lora_item* __restrict__ items, const int32_t* __restrict__ block_item,
                      const int64_t* __restrict__ block_start, int64_t chunk, int accumulate) {
    int64_t i0, i1;
    const dwm_lora_item it = dwm_list_chunk(items, block_item, block_start, chunk, i0, i1);
    const int64_t chunks = (it.N + LR_DA_ROWS - 1) / LR_DA_ROWS, plane = it.n;
    const float s = it.scale;
    for (int64_t e = i0 + threadIdx.x * 4; e < i1; e += LR_THREADS * 4) {
        f32x4 sum = lr_load4<false>(it.ws, e);
        for (int64_t c = 1; c < chunks; ++c) sum = sum + lr_load4<false>(it.ws, c * plane + e);
        f32x4 v;
        if (accumulate) {
            const f32x4 old = lr_load4<false>(it.out, e);
#pragma unroll
            for (int c = 0; c < 4; ++c) v[c] = fmaf(s, sum[c], old[c]);
        } else {
            v = sum * s;
        }
        lr_store4<false>(it.out, e, v);
    }
}

// dB.  Thread (nl = t & 31, jg = t >> 5) owns row n0 + nl and the jt factors j0 = jg jt ...; it walks along k, 128 columns at a time
// through LDS (the G tile with a skewed pitch: the lanes of a 16-byte read are 32 rows apart).
template <bool GBF>
DWM_DEVINL void lr_db_tile(const dwm_lora_item& it, int64_t tile, int accumulate, float (*Gs)[LR_GPAD], float (*As)[LR_TK]) {
    const int t = threadIdx.x, r = it.r;
    const int64_t N = it.N, K = it.K, n0 = tile * LR_TN;
    const int jt = (r + 7) >> 3, nl = t & 31, j0 = (t >> 5) * jt;
    float acc[8];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) acc[jj] = 0.f;
    for (int64_t k0 = 0; k0 < K; k0 += LR_TK) {
        lr_stage<GBF>(&Gs[0][0], LR_GPAD, LR_TN, it.w, n0, N, k0, K);
        lr_stage<false>(&As[0][0], LR_TK, r, it.a, 0, r, k0, K);
        __syncthreads();
        for (int c = 0; c < LR_TK; c += 4) {
            const f32x4 g = *(const f32x4*)&Gs[nl][c];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                if (jj < jt && j0 + jj < r) {
                    const f32x4 a = *(const f32x4*)&As[j0 + jj][c];
                    float s = acc[jj];
                    s = fmaf(g.x, a.x, s);
                    s = fmaf(g.y, a.y, s);
                    s = fmaf(g.z, a.z, s);
                    s = fmaf(g.w, a.w, s);
                    acc[jj] = s;
                }
            }
        }
        __syncthreads();
    }
    const int64_t n = n0 + nl;
    if (n >= N) return;
    lr_gf32* const db = (lr_gf32*)it.out2;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
        const int j = j0 + jj;
        if (jj < jt && j < r) {
            const int64_t i = n * r + j;
            db[i] = accumulate ? fmaf(it.scale, acc[jj], db[i]) : it.scale * acc[jj];
        }
    }
}

__global__ void __launch_bounds__(LR_THREADS)
lora_db_kernel(const dwm_lora_item* __restrict__ items, const int32_t* __restrict__ block_item, const int64_t* __restrict__ block_start,
               int accumulate) {
    __shared__ __attribute__((aligned(16))) float Gs[LR_TN][LR_GPAD];
    __shared__ __attribute__((aligned(16))) float As[LR_RMAX][LR_TK];
    int64_t tile;
    const dwm_lora_item it = lr_item(items, block_item, block_start, tile);
    if (it.flags & 1)
        lr_db_tile<true>(it, tile, accumulate, Gs, As);
    else
        lr_db_tile<false>(it, tile, accumulate, Gs, As);
}

// ------------------------------------------------------------------------------------------------------------------------ host
static inline int64_t lr_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline bool lr_off(const void* p, uintptr_t mask) { return (((uintptr_t)p) & mask) != 0; }

// the checks of one host item; on DWM_OK the tile counts of its launches are added to the four sums
static int lr_check_item(const dwm_lora_item& it, bool project, int64_t fin_chunk, int64_t sums[4]) {
    if (!it.w || !it.a || !it.b || !it.out || (project && (!it.out2 || !it.ws))) return DWM_EINVAL;
    if (it.N <= 0 || it.K <= 0 || it.r <= 0) return DWM_EINVAL;
    if (it.r > LR_RMAX || it.K % 4 != 0) return DWM_EUNSUPPORTED;
    if (it.N >= (1ll << 31) || it.K >= (1ll << 31) || it.N * it.K >= (1ll << 40)) return DWM_EUNSUPPORTED;
    if (it.n != (int64_t)it.r * it.K) return DWM_EINVAL;
    if (project && (it.flags & 2)) return DWM_EINVAL;                   // dA / dB are fp32
    if (lr_off(it.w, 15) || lr_off(it.a, 15) || lr_off(it.out, 15) || lr_off(it.b, 3)) return DWM_EALIGN;
    if (project && (lr_off(it.out2, 3) || lr_off(it.ws, 15))) return DWM_EALIGN;
    sums[0] += lr_cdiv(it.N, LR_TN) * lr_cdiv(it.K, LR_TK);
    sums[1] += lr_cdiv(it.N, LR_DA_ROWS) * lr_cdiv(it.K, LR_TK);
    sums[2] += project ? lr_cdiv(it.n, fin_chunk) : 0;
    sums[3] += lr_cdiv(it.N, LR_TN);
    return DWM_OK;
}

extern "C" int64_t dwm_lora_project_ws_floats(int64_t N, int64_t K, int32_t r) {
    if (N <= 0 || K <= 0 || r <= 0) return 0;
    return lr_cdiv(N, LR_DA_ROWS) * (int64_t)r * K;
}

extern "C" int dwm_lora_merge_multi(const dwm_lora_item* items, int64_t n_items, const dwm_lora_item* dev_items,
                                    const int32_t* block_item, const int64_t* block_start, int64_t n_blocks, void* stream) {
    if (!items || n_items <= 0 || dwm_bad_list_tables(dev_items, block_item, block_start, n_blocks, 1)) return DWM_EINVAL;
    int64_t sums[4] = {0, 0, 0, 0};
    for (int64_t i = 0; i < n_items; ++i) {
        const int rc = lr_check_item(items[i], false, 1, sums);
        if (rc != DWM_OK) return rc;
    }
    if (sums[0] != n_blocks) return DWM_EINVAL;
    hipLaunchKernelGGL(lora_merge_multi_kernel, dim3((unsigned)n_blocks), dim3(LR_THREADS), 0, (hipStream_t)stream, dev_items,
                       block_item, block_start);
    return dwm_launch_status();
}

extern "C" int dwm_lora_project_multi(const dwm_lora_item* items, int64_t n_items, const dwm_lora_item* dev_items,
                                      const int32_t* da_block_item, const int64_t* da_block_start, int64_t da_blocks,
                                      const int32_t* fin_block_item, const int64_t* fin_block_start, int64_t fin_blocks,
                                      int64_t fin_chunk, const int32_t* db_block_item, const int64_t* db_block_start,
                                      int64_t db_blocks, int32_t accumulate, void* stream) {
    if (!items || n_items <= 0 || dwm_bad_list_tables(dev_items, da_block_item, da_block_start, da_blocks, 1) ||
        dwm_bad_list_tables(dev_items, fin_block_item, fin_block_start, fin_blocks, fin_chunk) ||
        dwm_bad_list_tables(dev_items, db_block_item, db_block_start, db_blocks, 1) || fin_chunk % (LR_THREADS * 4) != 0)
        return DWM_EINVAL;
    int64_t sums[4] = {0, 0, 0, 0};
    for (int64_t i = 0; i < n_items; ++i) {
        const int rc = lr_check_item(items[i], true, fin_chunk, sums);
        if (rc != DWM_OK) return rc;
    }
    if (sums[1] != da_blocks || sums[2] != fin_blocks || sums[3] != db_blocks) return DWM_EINVAL;
    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(lora_da_kernel, dim3((unsigned)da_blocks), dim3(LR_THREADS), 0, s, dev_items, da_block_item, da_block_start);
    hipLaunchKernelGGL(lora_da_finish_kernel, dim3((unsigned)fin_blocks), dim3(LR_THREADS), 0, s, dev_items, fin_block_item,
                       fin_block_start, fin_chunk, (int)accumulate);
    hipLaunchKernelGGL(lora_db_kernel, dim3((unsigned)db_blocks), dim3(LR_THREADS), 0, s, dev_items, db_block_item, db_block_start,
                       (int)accumulate);
    return dwm_launch_status();
}
