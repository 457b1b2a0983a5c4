// Fused attention forward for gfx950, head_dim 64, bf16 in/out, fp32 softmax.
//
// Geometry: a workgroup of NW waves owns NW*QT*32 queries of one (problem, head);
// each wave owns QT 32-query tiles and walks the keys in tiles of 64.
//   S^T = K·Q^T   (A-operand = K fragment from LDS, B-operand = Q fragment in VGPRs)
// so after v_mfma_f32_32x32x16_bf16 lane (q = lane & 31, half = lane >> 5) holds, for ITS
// query, the scores of keys (r & 3) + 8 (r >> 2) + 4 half  (r = 0..15) of a 32-key
// sub-tile: the softmax row reduction is in-lane ops + one lane^32 exchange.
//   O^T += V^T·P^T (A-operand = V^T fragment, B-operand = the P registers as they
// are: the accumulator register -> key map of S^T is exactly the k-slot map chosen
// for the second MFMA, so P never moves across lanes), leaving O^T with the query
// again on the lane axis: the running max / sum rescale is a per-lane scalar.
//
// K tile in LDS: [64 keys][8 x 16-B chunks], chunk ^= (key >> 1) & 7 (conflict-free
// ds_read_b128 fragments).  V tile: row-major like K, chunk ^= ((key >> 1) & 1) << 2, its
// (transposed) fragments fetched with the gfx950 transposing read ds_read_b64_tr_b16.
// K/V tiles go global -> LDS by LDS-DMA (global_load_lds, no staging registers, no ds_write)
// into a ring of 3 stages: tile t+3 is requested right after the barrier that retires
// tile t, so two tiles are always in flight behind the one being consumed (first-touch HBM
// latency of a (problem, head)'s K/V is ~2 tile times) and the per-tile wait at the barrier is a counted
// vmcnt.  (The compiler still puts a vmcnt(0) in front of the transposing V reads, which it cannot tell apart from
// the pending LDS-DMA writes; issuing the DMA from inline asm removes it and changes nothing measurable - by then
// the tiles requested one and two iterations earlier have landed.)
//
// Addressing: q/k/v/o rows of segment 0 go through the row map of dwm_attn_args,
// which folds the reference's einops rearranges (crossview_temporal_dit.py:307-315,
// 336-361) into the loads/stores; segment 1 (text context of the joint attention)
// is dense.  Mask modes: none / [B,G,G] group mask (cross-view) / dense bytes.
#include "attention_common.h"

using namespace dwm_attn;

namespace {

// MASK: 0 none, 1 group mask, 2 dense byte mask.  NW = 4 waves (256 threads).
// occupancy target: 3 workgroups (waves per SIMD) for 32 queries/wave, 2 for 64 queries/wave
template <int QT, int MASK>
__global__ void __launch_bounds__(256, QT == 1 ? 3 : 2)
attn_fwd_kernel(const AttnParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = 4;
    constexpr int QB = NW * QT * 32;          // queries per block
    // [L] offset (in 16-byte units) of every token row of this problem inside ITS segment's buffers;
    // segment 1 rows add seg1_delta (kept 64-bit: the two allocations may be > 32 GiB apart)
    int32_t* __restrict__ rowtab = (int32_t*)(smem + NSTAGE * STAGE_BYTES);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;

    // block -> (problem, head, query block); query block fastest so the blocks that
    // share one (problem, head)'s K/V are neighbours on one XCD.
    uint32_t id = (uint32_t)xcd_remap(blockIdx.x, P.n_problems * (P.heads / P.hpb) * P.nqb);
    const uint32_t id1 = fdiv(id, P.fd_nqb);
    const int qb = (int)(id - id1 * P.fd_nqb.d);
    // a workgroup handles `hpb` consecutive heads of its (problem, query block) back to back: the K/V tile
    // stream simply continues into the next head (its first tiles are already in flight during the current
    // head's last ones), the row table is built once, and the next head's Q rows are fetched a head ahead -
    // the fixed cost per (problem, head, query block) is what limits short sequences
    const int prob = (int)fdiv(id1, P.fd_heads);
    const int hgrp = (int)(id1 - (uint32_t)prob * P.fd_heads.d);
    const int hpb = P.hpb;
    const int head0 = hgrp * hpb;

    const int L = P.L, L0 = P.L0;
    const int64_t hoff = (int64_t)head0 * 64;

    // ---- row table: token l -> row index in its segment's buffers (one div/mod chain per token
    //      per block instead of one per staged 16-B chunk)
    {
        const int64_t base0 = seg0_base(P.rm, prob);
        for (int l = tid; l < L; l += 256)
            rowtab[l] = (int32_t)((l < L0 ? seg0_row(P.rm, base0, l) * P.ld0
                                          : ((int64_t)prob * P.L1 + (l - L0)) * P.ld1) >> 3);
    }
    __syncthreads();

    // ---- this lane's queries
    bf16x8 qf[QT][4];
    const bf16_t* qbase[QT];
    bf16_t* optr[QT];
    bool qok[QT];
    uint32_t gbits[QT];
    const uint8_t* dense_row[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        const int lq = qb * QB + (wave * QT + t) * 32 + l31;
        qok[t] = lq < P.qend;
        const int lqc = qok[t] ? lq : P.qend - 1;
        const bf16_t* qptr = P.q0 + ((int64_t)rowtab[lqc] << 3) + (lqc < L0 ? 0 : P.seg1_delta) + hoff;      // q, k, v share the offset table
        qbase[t] = qptr;
        if (lqc < L0) optr[t] = P.o0 + seg0_row(P.rm, seg0_base(P.rm, prob), lqc) * P.ldo0 + hoff;
        else optr[t] = P.o1 + ((int64_t)prob * P.L1 + (lqc - L0)) * P.ldo1 + hoff;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[t][ks] = scale_frag(*(const bf16x8*)(qptr + ks * 16 + half * 8), P.scale_log2);
        gbits[t] = 0xffffffffu;
        dense_row[t] = nullptr;
        if (MASK == 1) {
            const int gq = (int)fmod_u(fdiv((uint32_t)lqc, P.fd_gs), P.fd_G);
            const uint8_t* mrow = P.mask + ((int64_t)fdiv((uint32_t)prob, P.fd_ppm) * P.mask_G + gq) * P.mask_G;
            uint32_t bits = 0;
            for (int g = 0; g < P.mask_G; ++g) bits |= (mrow[g] ? 1u : 0u) << g;
            gbits[t] = bits;
        } else if (MASK == 2) {
            dense_row[t] = P.mask + ((int64_t)prob * L + lqc) * L;
        }
    }

    // ---- staging by LDS-DMA: 16 B per lane, LDS destination lane-linear, so wave w's instruction i
    //      fills tile rows 16 w + 8 i + (lane >> 3) and the chunk swizzle is applied on the *source*
    //      column: LDS chunk position (lane & 7) of row r holds global chunk (lane & 7) ^ swz(r).
    const int nkt = (L - P.kbeg + KT - 1) / KT;
    const int srow0 = wave * 16 + (lane >> 3), srow1 = srow0 + 8;
    const bf16_t* const kg0 = P.k0 + hoff + (((lane & 7) ^ ((srow0 >> 1) & 7)) << 3);
    const bf16_t* const kg1 = P.k0 + hoff + (((lane & 7) ^ ((srow1 >> 1) & 7)) << 3);
    const bf16_t* const vg0 = P.v0 + hoff + (((lane & 7) ^ (((srow0 >> 1) & 1) << 2)) << 3);
    const bf16_t* const vg1 = P.v0 + hoff + (((lane & 7) ^ (((srow1 >> 1) & 1) << 2)) << 3);
    const int sdst = wave * 2048;                     // wave-uniform byte offset of this wave's rows in a tile image

    int dma_h = 0, dma_kt = 0;            // (head, key tile) of the next tile to request
#define DWM_DMA_NEXT(stage_)                                                                \
    do {                                                                                    \
        DWM_DMA_TILE(dma_kt, stage_, dma_h * 64);                                           \
        if (++dma_kt == nkt) { dma_kt = 0; ++dma_h; }                                       \
    } while (0)
#define DWM_DMA_TILE(kt_, stage_, ho_)                                                      \
    do {                                                                                    \
        const int kb_ = P.kbeg + (kt_) * KT;                                                \
        const int ra_ = kb_ + srow0 < L ? kb_ + srow0 : L - 1;                              \
        const int rb_ = kb_ + srow1 < L ? kb_ + srow1 : L - 1;                              \
        const int64_t oa_ = ((int64_t)rowtab[ra_] << 3) + (ra_ < L0 ? 0 : P.seg1_delta);    \
        const int64_t ob_ = ((int64_t)rowtab[rb_] << 3) + (rb_ < L0 ? 0 : P.seg1_delta);    \
        char* kl_ = smem + (stage_) * STAGE_BYTES + sdst;                                   \
        glds16(kg0 + oa_ + (ho_), kl_);                                                     \
        glds16(kg1 + ob_ + (ho_), kl_ + 1024);                                              \
        glds16(vg0 + oa_ + (ho_), kl_ + K_TILE_BYTES);                                      \
        glds16(vg1 + ob_ + (ho_), kl_ + K_TILE_BYTES + 1024);                               \
    } while (0)

    // Softmax bookkeeping in the exponent domain: Q is pre-multiplied by scale*log2(e) and the S MFMAs
    // start from C = -m (negm holds -m_run in all 16 registers), so the accumulator already is
    // s*c - m and the exponentials need no per-score multiply-add.
    f32x16 ot[QT][2], negm[QT];
    float l_run[QT];
    bool mvalid[QT];                     // m_run has been set from a finite score
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        l_run[t] = 0.f;
        mvalid[t] = false;
#pragma unroll
        for (int r = 0; r < 16; ++r) negm[t][r] = 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[t][i][r] = 0.f;
    }

    const int kswz = (lane >> 1) & 7;
    // tr-read lane geometry: 16-lane group g covers d columns [16g, 16g+16) of a 32-d tile; lane u
    // of the group supplies the address of V[key0 + (u >> 2)][.. + 4 (u & 3)] (8 bytes) and receives
    // column u: elements V[key0 + 0..3][16 g + u]
    const int tr_u = lane & 15, tr_g = (lane >> 4) & 1;
    int vra[2], vrb[2];                   // per d-tile byte offsets of the two tr reads at step s = 0
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        const int dcol = dt * 32 + tr_g * 16 + (tr_u & 3) * 4;
        const int keyA = half * 4 + (tr_u >> 2), keyB = keyA + 8;
        vra[dt] = keyA * 128 + (((dcol >> 3) ^ (((keyA >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
        vrb[dt] = keyB * 128 + (((dcol >> 3) ^ (((keyB >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
    }

    // prologue: tiles 0, 1, 2 requested (4 DMA instructions per wave and tile; the Q fragment loads
    // were issued before them, so "vmcnt(8)" also covers Q)
    const int NT = hpb * nkt;             // tiles of this workgroup's stream
    DWM_DMA_NEXT(0);
    if (NT > 1) DWM_DMA_NEXT(1);
    if (NSTAGE > 2 && NT > 2) DWM_DMA_NEXT(2);
    if (NSTAGE > 2 && NT > 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if (NT > 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    // a wave whose queries all lie past the end of the sequence (last query block) only takes part
    // in the staging and the barriers
    const bool wave_active = qb * QB + wave * QT * 32 < P.qend;
    int stage = 0;                        // ring slot of the current tile
    int hh = 0, kt = 0;                   // (head, key tile) of the current tile
    for (int sidx = 0; sidx < NT; ++sidx) {
        const char* kl = smem + stage * STAGE_BYTES;
        const char* vl = kl + K_TILE_BYTES;
        // the last tile of a head: its S MFMAs are the last readers of this head's Q fragments, so the next head's
        // (raw) Q rows are loaded straight into the same registers and scaled at the head switch below
        const bool fetch_q = kt == nkt - 1 && hh + 1 < hpb && wave_active;
        if (wave_active) {

        // ---- S^T = K Q^T for two 32-key sub-tiles (K fragments shared by the QT query tiles)
        f32x16 st[QT][2];
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 kf = *(const bf16x8*)(kl + (j * 32 + l31) * 128 + (((2 * ks + half) ^ kswz) << 4));
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    st[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[t][ks], ks == 0 ? negm[t] : st[t][j], 0, 0, 0);
            }
        __builtin_amdgcn_s_setprio(0);
        if (fetch_q) {
            // issued as inline asm: a compiler-visible load that is still pending on the loop's back edge makes the
            // compiler put "s_waitcnt vmcnt(0)" in front of the S MFMAs of EVERY tile - which also drains the K/V
            // LDS-DMA of the two tiles that are meant to stay in flight.  The wait for these loads is the explicit one
            // at the head switch below.
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int ks = 0; ks < 4; ++ks)
                    asm volatile("global_load_dwordx4 %0, %1, off"
                                 : "=v"(qf[t][ks]) : "v"(qbase[t] + (hh + 1) * 64 + ks * 16 + half * 8) : "memory");
        }

        // ---- masks (raw-score domain), online softmax; P^T fragments stay in registers
        const int kbase = P.kbeg + kt * KT;
        if (kbase + KT > L) {                       // ragged last tile (wave-uniform)
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        if (kbase + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half >= L) st[t][j][r] = -INFINITY;
        }
        if (MASK == 1) {
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int key = kbase + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                    int g = (int)(((float)key + 0.5f) * P.inv_group_size);
                    g -= P.mask_G * (int)(((float)g + 0.5f) * P.inv_G);
#pragma unroll
                    for (int t = 0; t < QT; ++t)
                        if (!((gbits[t] >> g) & 1u)) st[t][j][r] = -INFINITY;
                }
        } else if (MASK == 2) {
#pragma unroll
            for (int t = 0; t < QT; ++t)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int key = kbase + j * 32 + (r & 3) + 8 * (r >> 2) + 4 * half;
                        if (key < L && dense_row[t][key] == 0) st[t][j][r] = -INFINITY;
                    }
        }

        bf16x8 pf[QT][4];                      // B-operand fragments, step s = 2*j + s2
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const float mx = tile_max32(st[t][0], st[t][1]);     // relative to the running max
            // deferred rescale: keep the old running max while the new one exceeds it by < 2^6
            // (P <= 64, exact in the fp32 sums; bf16 P keeps its relative precision); the first
            // finite score of a row always sets it
            const bool finite = mx > -INFINITY;
            if (__any((mx > 6.f) || (!mvalid[t] && finite))) {
                const float delta = mvalid[t] ? fmaxf(mx, 0.f) : (finite ? mx : 0.f);
                const float alpha = mvalid[t] ? __builtin_amdgcn_exp2f(-delta) : 0.f;   // nothing accumulated before the first finite score
                mvalid[t] = mvalid[t] || finite;
                l_run[t] *= alpha;
#pragma unroll
                for (int r = 0; r < 16; ++r) negm[t][r] -= delta;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r) st[t][j][r] -= delta;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) ot[t][i][r] *= alpha;
            }
            f32x2 ps2[2] = {{0.f, 0.f}, {0.f, 0.f}};     // packed-fp32 partial row sums (v_pk_add_f32)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    float pv[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) pv[e] = __builtin_amdgcn_exp2f(st[t][j][s2 * 8 + e]);
#pragma unroll
                    for (int e = 0; e < 8; e += 2) ps2[(e >> 1) & 1] += (f32x2){pv[e], pv[e + 1]};
                    const uint4 pk = pack8(pv);
                    pf[t][j * 2 + s2] = *reinterpret_cast<const bf16x8*>(&pk);
                }
            l_run[t] += (ps2[0][0] + ps2[0][1]) + (ps2[1][0] + ps2[1][1]);
        }

        // ---- O^T += V^T P^T   (V fragments shared by the QT query tiles)
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(vl + vra[dt] + s * (16 * 128)));
                const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(vl + vrb[dt] + s * (16 * 128)));
                const bf16x8 vf = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int t = 0; t < QT; ++t)
                    ot[t][dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[t][s], ot[t][dt], 0, 0, 0);
            }
        __builtin_amdgcn_s_setprio(0);
        }

        // tile s+1 landed (tile s+2 may stay in flight), everyone is done with this tile's slot, which then
        // receives tile s+3 (loads return in order: the Q loads of this iteration are younger than tile s+2's DMA)
        if (NSTAGE > 2 && sidx + 2 < NT) {
            if (fetch_q) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(4 + 4 * QT) : "memory");
            else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        } else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();

        // ---- end of a head: normalise and store its output, reset the running state, switch Q.
        // The 32 x 64 bf16 output tile of a wave is transposed through the 4 KiB of the just-retired stage that
        // this wave's own DMA will refill next (rows 16 w .. 16 w + 15 of its K and V images), so that every
        // store instruction writes 8 full 128-byte rows (lane-per-query stores would be 8-byte pieces).
        if (kt == nkt - 1) {
            const int head = head0 + hh;
            char* const sc = smem + stage * STAGE_BYTES + sdst;     // + K_TILE_BYTES for rows 16..31
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                // lane (q, half) reg r of ot[dt] -> d = dt*32 + (r&3) + 8(r>>2) + 4 half
                const float l_tot = l_run[t] + __shfl_xor(l_run[t], 32, 64);
                const float inv = __builtin_amdgcn_rcpf(l_tot);
                if (P.lse != nullptr && qok[t] && half == 0)       // NEGATIVE log2-domain LSE: P = exp2(c q.k + neg_lse)
                    P.lse[((int64_t)prob * P.heads + head) * L + qb * QB + (wave * QT + t) * 32 + l31] = negm[t][0] - __builtin_amdgcn_logf(l_tot);
                if (wave_active) {
                    char* const myrow = sc + (l31 >> 4) * K_TILE_BYTES + (l31 & 15) * 128;
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                        for (int rg = 0; rg < 4; ++rg) {
                            float v[4];
#pragma unroll
                            for (int j = 0; j < 4; ++j) v[j] = ot[t][dt][rg * 4 + j] * inv;
                            const int chunk = (dt * 4 + rg) ^ (l31 & 7);            // 16-B chunk, swizzled by the row
                            *(uint2*)(myrow + (chunk << 4) + half * 8) = pack4(v);
                        }
                    // same-wave LDS ops complete in order: the reads below see the writes above
                    const int64_t orow = (int64_t)optr[t];
#pragma unroll
                    for (int pass = 0; pass < 4; ++pass) {
                        const int r = pass * 8 + (lane >> 3), c = lane & 7;       // 8 lanes per output row
                        const uint4 val = *(const uint4*)(sc + (r >> 4) * K_TILE_BYTES + (r & 15) * 128 + ((c ^ (r & 7)) << 4));
                        const int64_t rp = __shfl(orow, r, 64);                  // row pointer held by the lane that owns query r
                        const bool ok = qb * QB + (wave * QT + t) * 32 + r < P.qend;
                        if (ok) *(uint4*)((bf16_t*)rp + hh * 64 + c * 8) = val;
                    }
                }
                l_run[t] = 0.f;
                mvalid[t] = false;
#pragma unroll
                for (int r = 0; r < 16; ++r) negm[t][r] = 0.f;
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int r = 0; r < 16; ++r) ot[t][i][r] = 0.f;
                if (hh + 1 < hpb) {
                    // the next head's raw Q rows (asm loads of this head's last tile) have landed after this wait; the
                    // fragments are operands of the asm so that the scaling cannot be scheduled above it
                    asm volatile("s_waitcnt vmcnt(0)"
                                 : "+v"(qf[t][0]), "+v"(qf[t][1]), "+v"(qf[t][2]), "+v"(qf[t][3]) :: "memory");
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) qf[t][ks] = scale_frag(qf[t][ks], P.scale_log2);
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // scratch reads done before this wave's DMA refills it
        }
        if (sidx + NSTAGE < NT) DWM_DMA_NEXT(stage);
        stage = stage == NSTAGE - 1 ? 0 : stage + 1;
        if (++kt == nkt) { kt = 0; ++hh; }
    }
#undef DWM_DMA_NEXT
#undef DWM_DMA_TILE
}

// ---------------------------------------------------------------------------------------------------------------
// Short sequences (L <= 32, one segment, no mask): the point-wise temporal attention, L = frame count
// (crossview_temporal_dit.py:352-361; 5376 x 24 problems of L = 16 at BASELINE config 3).  The tiled kernel above
// spends a 128-query workgroup and a 64-key tile on 16 tokens; this one packs 32 / SL problems (SL = 8, 16 or 32
// token slots) into ONE 32 x 32 MFMA tile per wave - block-diagonal validity mask - so that all 64 lanes carry a
// token, and is bound by the q/k/v/o bytes (1.06 GB at config 3).  No LDS ring and no barrier: Q and K fragments
// are the lanes' own rows straight from global memory (the A / B operand layouts of v_mfma_f32_32x32x16_bf16 are
// row-per-lane), V goes through 4 KiB of wave-private LDS for the transposing read, and the output tile returns
// through the same 4 KiB so that every store instruction writes whole 128-byte rows.
template <int SL>
__global__ void __launch_bounds__(256, 4)
attn_small_kernel(const AttnParams P) {
    __shared__ __attribute__((aligned(16))) char smem[4 * 4096];
    constexpr int PP = 32 / SL;                      // problems per tile
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;
    char* const sc = smem + wave * 4096;

    // block -> (4 consecutive problem groups, head group); head group fastest: the blocks in flight together read the
    // same token rows
    const uint32_t quad = fdiv(blockIdx.x, P.fd_heads);
    const int hgrp = (int)(blockIdx.x - quad * P.fd_heads.d);
    const int grp = (int)quad * 4 + wave;
    if (grp * PP >= P.n_problems) return;            // wave-uniform; no block-level barrier anywhere below
    const int hpb = P.hpb;
    const int64_t hoff = (int64_t)hgrp * hpb * 64;

    const int slot = l31 / SL, tok = l31 % SL;
    int prob = grp * PP + slot;
    const bool pvalid = prob < P.n_problems;
    if (!pvalid) prob = P.n_problems - 1;
    const bool ok = pvalid && tok < P.L;
    const int64_t row = seg0_row(P.rm, seg0_base(P.rm, prob), tok < P.L ? tok : P.L - 1);
    const bf16_t* const qp = P.q0 + row * P.ld0 + hoff + half * 8;
    const bf16_t* const kp = P.k0 + row * P.ld0 + hoff + half * 8;
    const bf16_t* const vp = P.v0 + row * P.ld0 + hoff + half * 8;
    const int64_t orow = (int64_t)(P.o0 + row * P.ldo0 + hoff);

    // keys this lane's 16 score registers stand for: (r & 3) + 8 (r >> 2) + 4 half; valid = same slot, token < L
    uint32_t kmask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int key = (r & 3) + 8 * (r >> 2) + 4 * half;
        if (key / SL == slot && key % SL < P.L) kmask |= 1u << r;
    }
    // tr-read geometry of the V^T fragments (see attn_fwd_kernel)
    const int tr_u = lane & 15, tr_g = (lane >> 4) & 1;
    int vra[2], vrb[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        const int dcol = dt * 32 + tr_g * 16 + (tr_u & 3) * 4;
        const int keyA = half * 4 + (tr_u >> 2), keyB = keyA + 8;
        vra[dt] = keyA * 128 + (((dcol >> 3) ^ (((keyA >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
        vrb[dt] = keyB * 128 + (((dcol >> 3) ^ (((keyB >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
    }
    const int vswz = ((l31 >> 1) & 1) << 2;
    char* const myrow = sc + l31 * 128;

    for (int hh = 0; hh < hpb; ++hh) {
        bf16x8 qf[4], kf[4];
        uint4 vv[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            qf[ks] = *(const bf16x8*)(qp + hh * 64 + ks * 16);
            kf[ks] = *(const bf16x8*)(kp + hh * 64 + ks * 16);
            vv[ks] = *(const uint4*)(vp + hh * 64 + ks * 16);
        }
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks)
            st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], scale_frag(qf[ks], P.scale_log2), st, 0, 0, 0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) *(uint4*)(myrow + (((2 * ks + half) ^ vswz) << 4)) = vv[ks];

        float mx = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            if (!((kmask >> r) & 1u)) st[r] = -INFINITY;
            mx = fmaxf(mx, st[r]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));       // every slot holds >= 1 valid key: finite
        float pv[16], sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            pv[r] = __builtin_amdgcn_exp2f(st[r] - mx);
            sum += pv[r];
        }
        sum += __shfl_xor(sum, 32, 64);
        bf16x8 pf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint4 pk = pack8(pv + 8 * s);
            pf[s] = *reinterpret_cast<const bf16x8*>(&pk);
        }
        f32x16 ot[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dt][r] = 0.f;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(sc + vra[dt] + s * (16 * 128)));
                const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                    (__attribute__((address_space(3))) s16x4*)(sc + vrb[dt] + s * (16 * 128)));
                const bf16x8 vf = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
                ot[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], ot[dt], 0, 0, 0);
            }
        // normalise; transpose the 32 x 64 output tile through the wave's LDS (same-wave LDS ops complete in order)
        const float inv = __builtin_amdgcn_rcpf(sum);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = ot[dt][rg * 4 + j] * inv;
                *(uint2*)(myrow + (((dt * 4 + rg) ^ (l31 & 7)) << 4) + half * 8) = pack4(v);
            }
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int r = pass * 8 + (lane >> 3), c = lane & 7;
            const uint4 val = *(const uint4*)(sc + r * 128 + ((c ^ (r & 7)) << 4));
            const int64_t rp = __shfl(orow, r, 64);
            const int okr = __shfl((int)ok, r, 64);
            if (okr) *(uint4*)((bf16_t*)rp + hh * 64 + c * 8) = val;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Group-masked attention over short groups: the row-wise cross-view attention (crossview_temporal_dit.py:300-327; every
// problem = one latent row of one frame, L = views x row width, the [B, V, V] view mask expanded to tokens).  When a
// problem is exactly G groups of <= 32 tokens (L = G * group_size), the mask is block structured at the granularity of one
// MFMA tile: a wave owns the queries of ONE group (query-per-lane, as above) and visits only the key groups its mask row
// allows - the ring mask of the 6-camera rigs allows 3 of 6, so half of the tiled kernel's score work is never issued and
// no per-score mask arithmetic remains.  Structure of attn_small_kernel: no LDS ring, no barrier; Q and K fragments are
// the lanes' own rows straight from global memory (a K / V row is read by the waves of the <= G query groups that see it:
// L2 / L1 hits), V passes through 4 KiB of wave-private LDS for the transposing read, online softmax across the visited
// groups, output rows returned through the same 4 KiB as whole 128-byte rows.  HBM-bound: q, k, v read + o written once
// (1.06 GB at BASELINE config 3).
__global__ void __launch_bounds__(256, 3)
attn_group_kernel(const AttnParams P) {
    __shared__ __attribute__((aligned(16))) char smem[4 * 4096];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;
    char* const sc = smem + wave * 4096;

    // block -> (4 consecutive (problem, query group) units, head group); head group fastest
    const uint32_t quad = fdiv(blockIdx.x, P.fd_heads);
    const int hgrp = (int)(blockIdx.x - quad * P.fd_heads.d);
    const uint32_t unit = quad * 4 + (uint32_t)wave;
    const int G = P.mask_G, gs = P.group_size;
    if (unit >= (uint32_t)P.n_problems * (uint32_t)G) return;     // wave-uniform; no block-level barrier below
    const int prob = (int)fdiv(unit, P.fd_G);
    const int gq = (int)(unit - (uint32_t)prob * (uint32_t)G);
    const int hpb = P.hpb;
    const int64_t hoff = (int64_t)hgrp * hpb * 64;
    const int64_t base = seg0_base(P.rm, prob);

    const bool qvalid = l31 < gs;
    const int lclamp = qvalid ? l31 : gs - 1;
    const int64_t qrow = seg0_row(P.rm, base, gq * gs + lclamp);
    const bf16_t* const qp = P.q0 + qrow * P.ld0 + hoff + half * 8;
    const int64_t orow = (int64_t)(P.o0 + qrow * P.ldo0 + hoff);

    // the key groups this wave's queries may attend to (one mask row per (sample, query group): wave-uniform)
    uint32_t bits = 0;
    {
        const uint8_t* mrow = P.mask + ((int64_t)fdiv((uint32_t)prob, P.fd_ppm) * G + gq) * G;
        for (int g = 0; g < G; ++g) bits |= (mrow[g] ? 1u : 0u) << g;
        bits = __builtin_amdgcn_readfirstlane(bits);
    }
    // keys this lane's 16 score registers stand for inside a group: (r & 3) + 8 (r >> 2) + 4 half; valid = key < gs
    uint32_t kmask = 0;
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if ((r & 3) + 8 * (r >> 2) + 4 * half < gs) kmask |= 1u << r;
    // tr-read geometry of the V^T fragments (see attn_fwd_kernel)
    const int tr_u = lane & 15, tr_g = (lane >> 4) & 1;
    int vra[2], vrb[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        const int dcol = dt * 32 + tr_g * 16 + (tr_u & 3) * 4;
        const int keyA = half * 4 + (tr_u >> 2), keyB = keyA + 8;
        vra[dt] = keyA * 128 + (((dcol >> 3) ^ (((keyA >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
        vrb[dt] = keyB * 128 + (((dcol >> 3) ^ (((keyB >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
    }
    const int vswz = ((l31 >> 1) & 1) << 2;
    char* const myrow = sc + l31 * 128;

    for (int hh = 0; hh < hpb; ++hh) {
        bf16x8 qf[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = scale_frag(*(const bf16x8*)(qp + hh * 64 + ks * 16), P.scale_log2);
        f32x16 ot[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dt][r] = 0.f;
        float m_run = -INFINITY, l_run = 0.f;          // l_run: this lane's keys only; the partner's half is added at the end

        for (uint32_t rem = bits; rem != 0; rem &= rem - 1) {
            const int g = __builtin_ctz(rem);
            const int64_t krow = seg0_row(P.rm, base, g * gs + lclamp);      // rows past the group's end: clamped, masked below
            const bf16_t* const kp = P.k0 + krow * P.ld0 + hoff + hh * 64 + half * 8;
            const bf16_t* const vp = P.v0 + krow * P.ld0 + hoff + hh * 64 + half * 8;
            bf16x8 kf[4];
            uint4 vv[4];
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                kf[ks] = *(const bf16x8*)(kp + ks * 16);
                vv[ks] = *(const uint4*)(vp + ks * 16);
            }
            f32x16 st;
#pragma unroll
            for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[ks], qf[ks], st, 0, 0, 0);
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) *(uint4*)(myrow + (((2 * ks + half) ^ vswz) << 4)) = vv[ks];

            float mx = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                if (!((kmask >> r) & 1u)) st[r] = -INFINITY;
                mx = fmaxf(mx, st[r]);
            }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));       // a group holds >= 1 valid key: finite
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);      // 0 for the first group (m_run = -inf)
            m_run = m_new;
            float pv[16], sum = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                pv[r] = __builtin_amdgcn_exp2f(st[r] - m_new);
                sum += pv[r];
            }
            l_run = l_run * alpha + sum;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
            bf16x8 pf[2];
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const uint4 pk = pack8(pv + 8 * s);
                pf[s] = *reinterpret_cast<const bf16x8*>(&pk);
            }
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4*)(sc + vra[dt] + s * (16 * 128)));
                    const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                        (__attribute__((address_space(3))) s16x4*)(sc + vrb[dt] + s * (16 * 128)));
                    const bf16x8 vf = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
                    ot[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[s], ot[dt], 0, 0, 0);
                }
        }
        // normalise; transpose the 32 x 64 output tile through the wave's LDS (same-wave LDS ops complete in order)
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        const float inv = __builtin_amdgcn_rcpf(l_tot);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = ot[dt][rg * 4 + j] * inv;
                *(uint2*)(myrow + (((dt * 4 + rg) ^ (l31 & 7)) << 4) + half * 8) = pack4(v);
            }
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int r = pass * 8 + (lane >> 3), c = lane & 7;
            const uint4 val = *(const uint4*)(sc + r * 128 + ((c ^ (r & 7)) << 4));
            const int64_t rp = __shfl(orow, r, 64);
            if (r < gs) *(uint4*)((bf16_t*)rp + hh * 64 + c * 8) = val;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Group-masked attention, shared form: ONE WORKGROUP = one (problem, head group), ONE WAVE = one query group (view).  The
// per-wave form above lets every wave fetch the K / V rows of the key groups it may see straight from global memory, so a
// row is pulled through L1 / TA once per query group that sees it (3x with the ring mask of the 6-camera rigs) in 32-byte
// pieces: the launch moves its 1.06 GB at 2.7-3.0 TB/s.  Here wave g copies the K and V rows of group g of a head into the
// workgroup's LDS images ONCE, by LDS-DMA (8 lanes per row: whole 128-byte row pieces, no staging registers), and every
// wave reads the fragments of the groups its mask row allows from LDS (K image swizzled for ds_read_b128, V image for
// ds_read_b64_tr_b16, as in attn_fwd_kernel).  The images are double buffered over the heads of the workgroup: the copy of
// head h+2 is requested right after the ONE barrier per head - the one that says "everybody is done reading head h's images
// and everybody's rows of head h+1 have landed" - so a copy has a whole head's compute to arrive; the next head's Q rows are
// requested before the current head's compute; the output tile leaves through 4 KiB of wave-private LDS as whole rows.
// One workgroup per CU (120 KiB at 6 views).  HBM-bound: q, k, v read + o written once.
constexpr int GRP_IMG = 32 * 128;                 // one group's K (or V) image: 32 rows x 128 B
template <int G>
__global__ void __launch_bounds__(G * 64, 1)
attn_group_lds_kernel(const AttnParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int STAGE = 2 * G * GRP_IMG;                    // K images [G][32][128], then V images
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);           // = query group
    const int half = lane >> 5;
    const int l31 = lane & 31;
    char* const sc = smem + 2 * STAGE + wave * 4096;          // this wave's output transpose region

    const uint32_t prob = fdiv(blockIdx.x, P.fd_heads);
    const int hgrp = (int)(blockIdx.x - prob * P.fd_heads.d);
    const int gs = P.group_size, hpb = P.hpb;
    const int64_t hoff = (int64_t)hgrp * hpb * 64;
    const int64_t base = seg0_base(P.rm, (int)prob);

    const bool qvalid = l31 < gs;
    const int lclamp = qvalid ? l31 : gs - 1;
    const int64_t qrow = seg0_row(P.rm, base, wave * gs + lclamp);
    const bf16_t* const qp = P.q0 + qrow * P.ld0 + hoff + half * 8;
    const int64_t orow = (int64_t)(P.o0 + qrow * P.ldo0 + hoff);

    uint32_t bits = 0;                     // key groups this wave's queries may attend to (wave-uniform)
    {
        const uint8_t* mrow = P.mask + ((int64_t)fdiv(prob, P.fd_ppm) * G + wave) * G;
        for (int g = 0; g < G; ++g) bits |= (mrow[g] ? 1u : 0u) << g;
        bits = __builtin_amdgcn_readfirstlane(bits);
    }
    uint32_t kmask = 0;                    // keys of a group this lane's 16 score registers stand for: valid = key < gs
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if ((r & 3) + 8 * (r >> 2) + 4 * half < gs) kmask |= 1u << r;

    // copy geometry: instruction i of this wave fills rows 8 i + (lane >> 3) of ITS group's image, 16 B per lane; the chunk
    // swizzle of the image is applied on the source column (the destination of an LDS-DMA is lane-linear)
    int64_t srow[4];
    int kcol[4], vcol[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = 8 * i + (lane >> 3);
        srow[i] = seg0_row(P.rm, base, wave * gs + (r < gs ? r : gs - 1)) * P.ld0 + hoff;      // rows past the group: clamped, masked
        kcol[i] = ((lane & 7) ^ ((r >> 1) & 7)) << 3;
        vcol[i] = ((lane & 7) ^ (((r >> 1) & 1) << 2)) << 3;
    }
    const int kswz = (lane >> 1) & 7;
    const int tr_u = lane & 15, tr_g = (lane >> 4) & 1;
    int vra[2], vrb[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
        const int dcol = dt * 32 + tr_g * 16 + (tr_u & 3) * 4;
        const int keyA = half * 4 + (tr_u >> 2), keyB = keyA + 8;
        vra[dt] = keyA * 128 + (((dcol >> 3) ^ (((keyA >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
        vrb[dt] = keyB * 128 + (((dcol >> 3) ^ (((keyB >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
    }
    char* const myrow = sc + l31 * 128;

    // copy of head h_'s K / V rows of group `wave` into the images of stage (h_ & 1) (8 LDS-DMA instructions)
    // (requests from inline asm: the compiler treats the builtin as a load that may alias any LDS access and put a vmcnt(0) in
    // front of the output transpose right behind the requests of head h + 2 - the copy was waited for, not overlapped)
    const uint32_t lds0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)smem;
    auto dma16 = [](const void* src, uint32_t lds_addr) {
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(src), "s"(lds_addr) : "memory", "m0");
    };
#define DWM_GRP_COPY(h_)                                                                                          \
    do {                                                                                                          \
        const uint32_t st_ = lds0 + ((h_) & 1) * STAGE + wave * GRP_IMG;                                          \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                           \
            dma16(P.k0 + srow[i] + (h_) * 64 + kcol[i], st_ + i * 1024);                                          \
            dma16(P.v0 + srow[i] + (h_) * 64 + vcol[i], st_ + G * GRP_IMG + i * 1024);                            \
        }                                                                                                         \
    } while (0)
    DWM_GRP_COPY(0);
    if (hpb > 1) DWM_GRP_COPY(1);
    bf16x8 qf[4], qn[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qn[ks] = qf[ks] = *(const bf16x8*)(qp + ks * 16);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                                           // heads 0 and 1 have landed
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = scale_frag(qf[ks], P.scale_log2);

    for (int hh = 0; hh < hpb; ++hh) {
        const char* const kimg = smem + (hh & 1) * STAGE;
        const char* const vimg = kimg + G * GRP_IMG;
        if (hh + 1 < hpb) {                                    // the next head's Q rows travel under this head's compute
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) qn[ks] = *(const bf16x8*)(qp + (hh + 1) * 64 + ks * 16);
        }
        f32x16 ot[2];
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[dt][r] = 0.f;
        float m_run = -INFINITY, l_run = 0.f;
        // the allowed key groups are taken three at a time (the ring mask of the camera rigs allows exactly three): the S
        // MFMAs of a chunk are independent chains, the softmax runs once over the chunk's 48 scores per lane (one rescale
        // per chunk instead of one per group) - a wave alone on its SIMD is latency-bound, this is where its ILP comes from
        for (uint32_t rem = bits; rem != 0;) {
            int gi[3];
            int ng = 0;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                gi[c] = rem ? __builtin_ctz(rem) : 0;
                if (rem) { ++ng; rem &= rem - 1; }
            }
            // all K fragments of the chunk are read first (12 reads in flight, absent groups re-read group gi[c] = 0's rows and
            // are masked below), then the MFMAs follow behind counted waits: as read-then-use pairs the compiler kept ONE
            // fragment register and every MFMA waited for a full LDS round trip
            f32x16 st[3];
            bf16x8 kfr[3][4];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const char* kl = kimg + gi[c] * GRP_IMG;
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) kfr[c][ks] = *(const bf16x8*)(kl + l31 * 128 + (((2 * ks + half) ^ kswz) << 4));
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int r = 0; r < 16; ++r) st[c][r] = 0.f;
            }
#pragma unroll
            for (int ks = 0; ks < 4; ++ks)
#pragma unroll
                for (int c = 0; c < 3; ++c) st[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kfr[c][ks], qf[ks], st[c], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    if (!((kmask >> r) & 1u) || c >= ng) st[c][r] = -INFINITY;
                    mx = fmaxf(mx, st[c][r]);
                }
            mx = fmaxf(mx, __shfl_xor(mx, 32, 64));       // a group holds >= 1 valid key: finite
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);      // 0 for the first chunk (m_run = -inf)
            m_run = m_new;
            float sum = 0.f;
            bf16x8 pf[3][2];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float pv[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    pv[r] = __builtin_amdgcn_exp2f(st[c][r] - m_new);
                    sum += pv[r];
                }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const uint4 pk = pack8(pv + 8 * s2);
                    pf[c][s2] = *reinterpret_cast<const bf16x8*>(&pk);
                }
            }
            l_run = l_run * alpha + sum;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) ot[dt][r] *= alpha;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                if (c < ng) {
                    const char* vl = vimg + gi[c] * GRP_IMG;
#pragma unroll
                    for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                        for (int dt = 0; dt < 2; ++dt) {
                            const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                (__attribute__((address_space(3))) s16x4*)(vl + vra[dt] + s2 * (16 * 128)));
                            const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
                                (__attribute__((address_space(3))) s16x4*)(vl + vrb[dt] + s2 * (16 * 128)));
                            const bf16x8 vf = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
                            ot[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf, pf[c][s2], ot[dt], 0, 0, 0);
                        }
                }
            }
        }
        // ONE barrier per head: own fragment reads of this head done, own rows of the next head landed (everything this
        // wave has requested is at least a head old here: the wait is free) - after it stage hh & 1 may be refilled
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        // the next head's Q rows count as used here (they have landed: see the wait above) - left to their first use below, the
        // compiler's own wait for them would sit behind the copy requests of head hh + 2 and drain those
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(qn[ks]));
        __syncthreads();
        if (hh + 2 < hpb) DWM_GRP_COPY(hh + 2);
        // normalise; transpose the 32 x 64 output tile through the wave's own LDS (same-wave LDS ops complete in order)
        const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
        const float inv = __builtin_amdgcn_rcpf(l_tot);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                float v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = ot[dt][rg * 4 + j] * inv;
                *(uint2*)(myrow + (((dt * 4 + rg) ^ (l31 & 7)) << 4) + half * 8) = pack4(v);
            }
#pragma unroll
        for (int pass = 0; pass < 4; ++pass) {
            const int r = pass * 8 + (lane >> 3), c = lane & 7;
            const uint4 val = *(const uint4*)(sc + r * 128 + ((c ^ (r & 7)) << 4));
            const int64_t rp = __shfl(orow, r, 64);
            if (r < gs) *(uint4*)((bf16_t*)rp + hh * 64 + c * 8) = val;
        }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[ks] = scale_frag(qn[ks], P.scale_log2);
    }
}
#undef DWM_GRP_COPY

// ---------------------------------------------------------------------------------------------------------------
// Resident form (round 3): the K and V rows of ONE head of one problem - all L <= 608 of them, 2 x 76 KiB at the joint
// attention's L = 602 - are copied into LDS ONCE by LDS-DMA and every query tile of the head is walked against them by the
// workgroup's 12 waves (tile = round * 12 + wave).  Against the tiled kernel above (128-query workgroups: every (problem,
// head)'s K / V crosses L2 -> LDS 4-5 times - 3.2 x its bytes in 128-byte requests, profiles/r2_attn_l2_counters.json; 4 LDS-DMA
// instructions + their address arithmetic + one workgroup barrier per 16 MFMAs and wave) this removes the refills
// (amplification 1), the per-tile barrier and the per-tile DMA issue: a wave's tile loop is fragment reads, MFMAs and the
// softmax only, and the waves run it unsynchronised (two barriers per HEAD: "K / V landed", "everybody done with them").
// Workgroups are persistent (one per CU, a fixed share of the (problem, head group) items), the next unit's Q rows are
// requested when a unit's tile loop ends, row offsets of inputs and outputs come from per-item tables in LDS, and the output
// tile leaves the registers as 16-byte pieces after a lane <-> lane + 32 exchange (v_permlane32_swap): the LDS is full.
// What the structure still pays (timeline in profiles/r3_attn_timeline.txt, L = 602: 54.7 k cycles per head): the copy of the
// next head stands between two heads (7 k cycles: 304 one-KiB DMA instructions through one CU's address path), the waves of a
// SIMD finish their tiles far apart (the oldest wave of three gets most issue slots: 15.6 / 19.7 / 34.3 k cycles for the same
// tile loop) and 19 tiles over 12 waves leave 5 waves idle in the second round.  Tried and dropped in this round: L2
// touches of the next head (loads return in order: the touches stall the next wait behind an HBM round trip), a refill point
// inside the last round (its barrier costs the waves' skew), loader waves that copy behind the others' progress words (the
// copy is hidden but the computing waves slow down by more), 8 computing + 4 loading waves, start skew between workgroups.
// Round 4, measured and dropped as well (scripts/experiments/attn_refill_points.patch, profiles/r4a_microbench_refill_stream32.log):
// two barrier-free refill points - the waves without a tile in the last round sleep on two LDS counters that the computing
// waves bump (one atomic each) once they are past n / 2 and 3 n / 4 of their last unit, and copy the next head's rows into
// the dead front of the images: bit-identical results, 3-5 % SLOWER at L = 602 (652-670 vs 693-701 TFLOP/s, same call) and
// 10 % slower at L = 448 (520 vs 575), 627-636 vs 657-665 inside the bench; and a register prefetch of the next head by the
// idle waves (5 x 31 KiB fit a head) - the register allocator puts the buffer in scratch at any size (the kernel sits at its
// 168-register budget with 25 spills already).
//
// Softmax without a running maximum (the fast path): softmax is shift invariant, so P' = 2^s (s = the log2-domain score,
// scale * log2(e) folded into Q) and O = (sum_k P'_k V_k) / (sum_k P'_k) need no maximum at all as long as nothing leaves
// the fp32 / bf16 exponent range - bf16 keeps fp32's exponent, so P' has the same RELATIVE precision as 2^(s - m).  With
// the RMS-normalised q / k of this model |s| is a few units.  Dropping the maximum, the -m accumulator splat and the rescale
// branch takes ~20 % of the vector instructions and 16 registers out of the tile loop - and makes partial results over key
// ranges plain sums.  A unit is accepted if every row sum lies in [2^-64, 2^64] (no P' overflowed, no row underflowed);
// otherwise (never, on this model) it is redone by the textbook online softmax from global memory (res_tile_safe).
// Fragment layouts and swizzles are attn_fwd_kernel's.
// One step of the fast path's software pipeline over the 32-key sub-tiles k of a sequence:
//     S(k+1) = K(k+1) Q^T   (4 MFMAs per query tile; accumulator starts from the inline constant 0)
//  || E(k):  P' = 2^S(k), row sums, bf16 pack   (16 v_exp, 8 v_pk_add, 8 v_cvt_pk per query tile)
//  || PV(k-1): O^T += V(k-1)^T P'(k-1)^T        (4 MFMAs per query tile)
// written as ONE instruction stream in which every MFMA is followed by one slice of E - two exponentials, a packed add and a
// convert: head_dim 64 makes the forward VALU-heavy (a vector instruction per ~50 MFMA flop), and on this chip a wave's own
// vector instructions hide under its own MFMAs (MFMA + 4..6 VALU per 32-cycle slot: 17.8 / 19.6 ns against 17.2 ns for the
// bare MFMA) while another wave's do not (43.8 ns for the same work split over two waves of a SIMD; scripts/probes/
// mfma_valu_probe.hip, profiles/r3_mfma_valu_probe.txt).  The order is pinned with sched_barrier(0) between the chunks; all
// fragment reads of a step are requested in its first chunks (the compiler's counted lgkmcnt waits follow the data).
template <int NT, bool DO_S, bool DO_E, bool DO_PV, bool RAGGED>
DWM_DEVINL void res_step(const char* __restrict__ kl, const char* __restrict__ vl, int key0, int L,
                         const bf16x8 (&qf)[NT][4], f32x16 (&s_out)[NT], f32x16 (&s_in)[NT],
                         bf16x8 (&p_out)[NT][2], const bf16x8 (&p_in)[NT][2],
                         f32x16 (&ot)[NT][2], f32x2 (&lsum)[NT][2],
                         int l31, int half, int kswz, const int (&vra)[2], const int (&vrb)[2]) {
    const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bf16x8 kf[4], vf[2][2];
    uint32_t pk[NT][8];
    // slice j of E: scores 2j, 2j + 1 of every query tile
    auto slice = [&](int j) {
        if (!DO_E) return;
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            float a = s_in[t][2 * j], b = s_in[t][2 * j + 1];
            if (RAGGED) {                                   // keys past the end of the sequence: 2^-inf = 0
                if (key0 + ((2 * j) & 3) + 8 * ((2 * j) >> 2) + 4 * half >= L) a = -INFINITY;
                if (key0 + ((2 * j + 1) & 3) + 8 * ((2 * j + 1) >> 2) + 4 * half >= L) b = -INFINITY;
            }
            const float pa = __builtin_amdgcn_exp2f(a), pb = __builtin_amdgcn_exp2f(b);
            lsum[t][j & 1] += (f32x2){pa, pb};
            // the convert is pinned to its slice by an empty volatile asm on its result (left alone it is sunk to the end of
            // the step, eight in a row behind the last MFMA).  NOT the convert itself as inline asm: the compiler does not
            // see the v_exp -> VALU wait state an asm operand needs and the convert then reads stale registers
            uint32_t w = pack_bf16x2(pa, pb);
            asm volatile("" : "+v"(w));
            pk[t][j] = w;
        }
    };
    auto vread = [&](int s2, int dt) {
        const s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vl + vra[dt] + s2 * (16 * 128)));
        const s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(vl + vrb[dt] + s2 * (16 * 128)));
        vf[s2][dt] = __builtin_shufflevector(a, b, 0, 1, 2, 3, 4, 5, 6, 7);
    };
    // MFMA m of the step (0-3: S with K fragment m; 4-7: PV with V fragment (m-4)/2, (m-4)%2) has its fragment requested PD
    // chunks ahead: everything up front would cost 32 fragment registers (with two query tiles the step then spills)
    constexpr int PD = NT == 1 ? 4 : 2;
    auto request = [&](int m) {
        if (m < 4) { if (DO_S) kf[m] = *(const bf16x8*)(kl + l31 * 128 + (((2 * m + half) ^ kswz) << 4)); }
        else if (m < 8) { if (DO_PV) vread((m - 4) >> 1, (m - 4) & 1); }
    };
    // chunk 0: the first fragment requests, first slice
#pragma unroll
    for (int m = 0; m < PD; ++m) request(m);
    slice(0);
    __builtin_amdgcn_sched_barrier(0);
    // chunks 1-8: one MFMA per query tile, the request PD MFMAs ahead, one slice
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        request(m + PD);
        if (m < 4) {
            if (DO_S) {
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    s_out[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[m], qf[t][m], m == 0 ? zero : s_out[t], 0, 0, 0);
            }
        } else if (DO_PV) {
            const int i = m - 4;
#pragma unroll
            for (int t = 0; t < NT; ++t)
                ot[t][i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vf[i >> 1][i & 1], p_in[t][i >> 1], ot[t][i & 1], 0, 0, 0);
        }
        if (m < 7) slice(m + 1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (DO_E) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            const uint4 lo = {pk[t][0], pk[t][1], pk[t][2], pk[t][3]}, hi = {pk[t][4], pk[t][5], pk[t][6], pk[t][7]};
            p_out[t][0] = *reinterpret_cast<const bf16x8*>(&lo);
            p_out[t][1] = *reinterpret_cast<const bf16x8*>(&hi);
        }
    }
}

// one unit = NT query tiles of one head against the resident K / V images: tile loop, acceptance test of the fast path (or
// the fallback), normalisation, and the stores.  qraw: this lane's raw Q fragments; op[t]: this lane's output row pointer
// (rows past the last query are clamped to it: they then hold the same Q, compute the same output and store the same
// bytes to the same address - unconditional stores keep the loop free of exec-masked blocks).
template <int NT, class Fetch>
DWM_DEVINL void res_unit(const ResCtx& c, const bf16x8 (&qraw)[NT][4], bf16_t* const (&op)[NT], float scale_log2, bool force_safe,
                         const ResGlobal& gm, Fetch&& after_loop, long long* tr = nullptr) {
    bf16x8 qf[NT][4];
    f32x16 ot[NT][2];
    f32x2 lsum[NT][2];
    float l_tot[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qf[t][ks] = scale_log2 == 1.f ? qraw[t][ks] : scale_frag(qraw[t][ks], scale_log2);   // (Q may arrive pre-scaled)
        lsum[t][0] = lsum[t][1] = (f32x2){0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) ot[t][i][r] = 0.f;
    }
    // software pipeline over the 32-key sub-tiles k (res_step); first and last sub-tile peeled, two steps per trip so that
    // the A / B register sets swap roles without copies
    const int n = c.nsub;
    const bool ragged = (n << 5) > c.L;
    const int lastkey = (n - 1) << 5;
    f32x16 sa[NT], sb[NT];
    bf16x8 pa[NT][2], pb[NT][2];
#define DWM_RES_STEP(S_, E_, PV_, RG_, kl_, vl_, so_, si_, po_, pi_) \
    res_step<NT, S_, E_, PV_, RG_>(kl_, vl_, lastkey, c.L, qf, so_, si_, po_, pi_, ot, lsum, c.l31, c.half, c.kswz, c.vra, c.vrb)
    DWM_RES_STEP(true, false, false, false, c.kimg, c.vimg, sa, sa, pa, pa);                          // S(0)
    if (n == 1) {
        if (ragged) DWM_RES_STEP(false, true, false, true, c.kimg, c.vimg, sa, sa, pa, pa);           // E(0)
        else DWM_RES_STEP(false, true, false, false, c.kimg, c.vimg, sa, sa, pa, pa);
        DWM_RES_STEP(false, false, true, false, c.kimg, c.vimg, sa, sa, pa, pa);                      // PV(0)
    } else {
        DWM_RES_STEP(true, true, false, false, c.kimg + 4096, c.vimg, sb, sa, pa, pa);                // S(1) || E(0)
        // invariant at the top of step k: S(k) is in sb, P'(k-1) in pa
        int k = 1;
#ifdef DWM_ATTN_TRACE
        if (tr != nullptr) tr[4] = (long long)__builtin_readcyclecounter();
#endif
        for (; k + 2 < n; k += 2) {
            DWM_RES_STEP(true, true, true, false, c.kimg + (k + 1) * 4096, c.vimg + (k - 1) * 4096, sa, sb, pb, pa);
            DWM_RES_STEP(true, true, true, false, c.kimg + (k + 2) * 4096, c.vimg + k * 4096, sb, sa, pa, pb);
        }
        if (k + 1 < n) {                                                   // step k, then the last sub-tile k + 1
            DWM_RES_STEP(true, true, true, false, c.kimg + (k + 1) * 4096, c.vimg + (k - 1) * 4096, sa, sb, pb, pa);
            if (ragged) DWM_RES_STEP(false, true, true, true, c.kimg, c.vimg + k * 4096, sa, sa, pa, pb);
            else DWM_RES_STEP(false, true, true, false, c.kimg, c.vimg + k * 4096, sa, sa, pa, pb);
            DWM_RES_STEP(false, false, true, false, c.kimg, c.vimg + (k + 1) * 4096, sa, sa, pa, pa);
        } else {                                                           // k is the last sub-tile
            if (ragged) DWM_RES_STEP(false, true, true, true, c.kimg, c.vimg + (k - 1) * 4096, sb, sb, pb, pa);
            else DWM_RES_STEP(false, true, true, false, c.kimg, c.vimg + (k - 1) * 4096, sb, sb, pb, pa);
            DWM_RES_STEP(false, false, true, false, c.kimg, c.vimg + k * 4096, sb, sb, pb, pb);
        }
    }
#undef DWM_RES_STEP
#ifdef DWM_ATTN_TRACE
    if (tr != nullptr) tr[5] = (long long)__builtin_readcyclecounter();
#endif
    after_loop();
    bool ok = !force_safe;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float l_half = (lsum[t][0][0] + lsum[t][0][1]) + (lsum[t][1][0] + lsum[t][1][1]);
        const auto lsw = __builtin_amdgcn_permlane32_swap(__float_as_uint(l_half), __float_as_uint(l_half), false, false);
        l_tot[t] = __uint_as_float(lsw[0]) + __uint_as_float(lsw[1]);
        // the row sum in range: no P' overflowed (an infinite or NaN P' makes the sum infinite or NaN) and the row did not
        // underflow; O' <= sum * max|V| then stays finite for |V| < 2^63
        ok = ok && (l_tot[t] >= 5.421010862e-20f) && (l_tot[t] <= 1.8446744e19f);
    }
    if (!__all(ok)) {                                      // wave-uniform: redo the unit by the online softmax
#pragma unroll                                             // (a runtime t would put qf / ot into scratch)
        for (int t = 0; t < NT; ++t) {
            float m_run = -INFINITY, l_run = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int r = 0; r < 16; ++r) ot[t][i][r] = 0.f;
            for (int k = 0; k < c.nsub; ++k) res_tile_safe(gm, k << 5, c.L, c.L0, qf[t], ot[t], m_run, l_run, c.l31, c.half);
            l_tot[t] = l_run + __shfl_xor(l_run, 32, 64);
        }
    }
    // normalise and store: lane (q, half) holds d = 32 dt + 8 g + 4 half + (0..3) in registers 4 g .. 4 g + 3 of ot[dt];
    // after the exchange of one 8-byte piece with lane ^ 32 per pair of g, the lower lane owns the whole 16-byte chunk of
    // the even g, the upper lane that of the odd g
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const float inv = __builtin_amdgcn_rcpf(l_tot[t]);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int gp = 0; gp < 2; ++gp) {
                float a[4], b[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    a[j] = ot[t][dt][gp * 8 + j] * inv;            // g = 2 gp
                    b[j] = ot[t][dt][gp * 8 + 4 + j] * inv;        // g = 2 gp + 1
                }
                const uint2 pa = pack4(a), pb = pack4(b);
                const auto s0 = __builtin_amdgcn_permlane32_swap(pa.x, pb.x, false, false);
                const auto s1 = __builtin_amdgcn_permlane32_swap(pa.y, pb.y, false, false);
                const uint4 val = {s0[0], s1[0], s0[1], s1[1]};
                *(uint4*)(op[t] + dt * 32 + (2 * gp + c.half) * 8) = val;
            }
    }
}

template <int NW>      // NW waves; one query tile (32 queries) per unit
__global__ void __launch_bounds__(NW * 64, 1)
attn_res_kernel(const AttnParams P) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5;
    const int l31 = lane & 31;

    const int L = P.L, L0 = P.L0;
    const int Lp = (L + 31) & ~31;                        // image rows (32-key granules)
    const int Lt = (L + 3) & ~3;                          // table pitch
    char* const kimg = smem;
    char* const vimg = smem + Lp * 128;
    // tables: input row offsets (see attn_fwd_kernel) of this item and of the next one, output row offsets of this item
    int32_t* const tabs = (int32_t*)(smem + 2 * Lp * 128);
    int32_t* const otab = tabs + 2 * Lt;

    ResCtx c;
    c.kimg = kimg; c.vimg = vimg; c.rowtab = tabs;
    c.L = L; c.L0 = L0; c.nsub = Lp >> 5;
    c.l31 = l31; c.half = half; c.kswz = (lane >> 1) & 7;
    {
        const int tr_u = lane & 15, tr_g = (lane >> 4) & 1;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            const int dcol = dt * 32 + tr_g * 16 + (tr_u & 3) * 4;
            const int keyA = half * 4 + (tr_u >> 2), keyB = keyA + 8;
            c.vra[dt] = keyA * 128 + (((dcol >> 3) ^ (((keyA >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
            c.vrb[dt] = keyB * 128 + (((dcol >> 3) ^ (((keyB >> 1) & 1) << 2)) << 4) + ((dcol & 7) << 1);
        }
    }

    // Work: item = (problem, head group of hpb heads); the workgroups are PERSISTENT (one per CU, items blockIdx.x,
    // blockIdx.x + gridDim.x, ...): only the very first head of a workgroup is loaded cold, the copy pipeline below runs across
    // item seams.  g = running head index of this workgroup.
    const int hpb = P.hpb;
    const int n_items = P.n_problems * (int)P.fd_heads.d;
    const int n_my = ((int)blockIdx.x < n_items) ? (n_items - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;
    const int G = n_my * hpb;
    auto item_of = [&](int g, uint32_t& prob, int64_t& hoff) {       // head g of this workgroup: its problem and column offset
        const int it = g / hpb, hh = g - it * hpb;
        const uint32_t item = blockIdx.x + (uint32_t)it * gridDim.x;
        prob = fdiv(item, P.fd_heads);
        hoff = ((int64_t)(item - prob * P.fd_heads.d) * hpb + hh) * 64;
    };
    auto build_tab = [&](int32_t* tab, int32_t* ot, uint32_t prob) {
        const int64_t base0 = seg0_base(P.rm, (int)prob);
        for (int l = tid; l < L; l += NW * 64) {
            const int64_t r0 = l < L0 ? seg0_row(P.rm, base0, l) : 0;
            if (tab != nullptr) tab[l] = (int32_t)((l < L0 ? r0 * P.ld0 : ((int64_t)prob * P.L1 + (l - L0)) * P.ld1) >> 3);
            if (ot != nullptr)      // offset inside the token's output segment in 16-byte units (segment 1 adds oseg1_delta: the two
                                    // allocations may be > 32 GiB apart)
                ot[l] = (int32_t)((l < L0 ? r0 * P.ldo0 : ((int64_t)prob * P.L1 + (l - L0)) * P.ldo1) >> 3);
        }
    };
    // copy of the 32-key sub-tiles [s0, s1) of one head's K or V rows into its image: instruction i (8 rows x 128 B, 16 B per
    // lane, LDS destination lane-linear) belongs to participant i mod np; the chunk swizzle of the images is applied on the source
    // column (attn_fwd_kernel)
    auto copy_rows = [&](const int32_t* tab, int64_t ho, int s0, int s1, bool is_v, int me, int np) {
        int i = s0 * 4;
        i += (me - i % np + np) % np;
        for (; i < s1 * 4; i += np) {
            const int r = i * 8 + (lane >> 3);
            const int rc = r < L ? r : L - 1;                 // rows past the end: a copy of the last row (finite), masked as keys
            const int64_t off = ((int64_t)tab[rc] << 3) + (rc < L0 ? 0 : P.seg1_delta) + ho;
            if (!is_v) glds16(P.k0 + off + (((lane & 7) ^ ((r >> 1) & 7)) << 3), kimg + i * 1024);
            else glds16(P.v0 + off + (((lane & 7) ^ (((r >> 1) & 1) << 2)) << 3), vimg + i * 1024);
        }
    };

    const int nqt = (P.qend + 31) >> 5;                      // 32-query tiles of a head
    const int nwc = P.nwc;                                   // compute waves (<= NW): tile = round * nwc + wave
    const int rounds = (nqt + nwc - 1) / nwc;
    const bool force_safe = P.safe_softmax != 0;             // dwm_attn_args.variant bit 4: online softmax for every unit
    const int n = c.nsub;

    // development aid (-DDWM_ATTN_TRACE): shader-clock timestamps of wave w of workgroup b < 8 at 8 points of every head,
    // written to the (otherwise unused) lse buffer as int64 [8 workgroups][NW][64 heads][8]
#ifdef DWM_ATTN_TRACE
#define DWM_TR(slot_) do { if (P.lse != nullptr && blockIdx.x < 8 && lane == 0 && g < 64) \
        ((long long*)P.lse)[(((int)blockIdx.x * NW + wave) * 64 + g) * 8 + (slot_)] = (long long)__builtin_readcyclecounter(); } while (0)
#else
#define DWM_TR(slot_) do {} while (0)
#endif
    if (G == 0) return;
    uint32_t prob; int64_t hoff;
    item_of(0, prob, hoff);
    build_tab(tabs, otab, prob);
    __syncthreads();
    copy_rows(tabs, hoff, 0, n, false, wave, NW);            // the first head: nothing to hide it under
    copy_rows(tabs, hoff, 0, n, true, wave, NW);
    bf16x8 qn[4];                                            // raw Q fragments of this wave's next unit
    if (wave < nwc && wave < nqt) {
        int lq = wave * 32 + l31;
        lq = lq < P.qend ? lq : P.qend - 1;
        const bf16_t* qp = P.q0 + ((int64_t)tabs[lq] << 3) + (lq < L0 ? 0 : P.seg1_delta) + hoff + half * 8;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) qn[ks] = *(const bf16x8*)(qp + ks * 16);
    }

    for (int g = 0; g < G; ++g) {
        const int it = g / hpb;
        const int32_t* const tab = tabs + (it & 1) * Lt;
        item_of(g, prob, hoff);
        // the next head (same item: same table; next item: its table is built now, it becomes visible at the barrier below)
        const bool has_next = g + 1 < G;
        uint32_t nprob = prob; int64_t nhoff = hoff;
        const int32_t* ntab = tab;
        const bool new_item_next = has_next && (g + 1) / hpb != it;
        if (has_next) {
            item_of(g + 1, nprob, nhoff);
            if (new_item_next) {
                ntab = tabs + ((it + 1) & 1) * Lt;
                build_tab((int32_t*)ntab, nullptr, nprob);
            }
        }
        DWM_TR(0);
        __builtin_amdgcn_s_waitcnt(0x0F70);                  // vmcnt(0): this wave's share of the head's rows has landed
        DWM_TR(1);
        __syncthreads();                                     // ... and everybody else's
        DWM_TR(2);
        c.rowtab = tab;

        for (int r = 0; r < rounds; ++r) {
            const int qt = r * nwc + wave;
            if (wave < nwc && qt < nqt) {
                bf16x8 q[1][4];
                bf16_t* op[1];
#pragma unroll
                for (int ks = 0; ks < 4; ++ks) q[0][ks] = qn[ks];
                // this wave's NEXT unit (next round of this head, or its first tile of the next head): its Q rows are requested
                // when this unit's tile loop is over (the loop's registers are free then) and travel under the normalisation, the
                // stores and - across a head seam - the barriers
                auto fetch_next_q = [&]() {
                    const bool same = qt + nwc < nqt;
                    if (!same && !(has_next && wave < nqt)) {      // no next unit: still define qn (it must not stay live across the tile loop)
#pragma unroll
                        for (int ks = 0; ks < 4; ++ks) qn[ks] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
                        return;
                    }
                    int lq = (same ? qt + nwc : wave) * 32 + l31;
                    lq = lq < P.qend ? lq : P.qend - 1;
                    const int32_t* const t2 = same ? tab : ntab;
                    const bf16_t* qp = P.q0 + ((int64_t)t2[lq] << 3) + (lq < L0 ? 0 : P.seg1_delta) + (same ? hoff : nhoff) + half * 8;
#pragma unroll
                    for (int ks = 0; ks < 4; ++ks) qn[ks] = *(const bf16x8*)(qp + ks * 16);
                };
                {
                    int lq = qt * 32 + l31;
                    lq = lq < P.qend ? lq : P.qend - 1;
                    op[0] = P.o0 + ((int64_t)otab[lq] << 3) + (lq < L0 ? 0 : P.oseg1_delta) + hoff;
                }
                ResGlobal gm;
                gm.k = P.k0 + hoff; gm.v = P.v0 + hoff; gm.tab = tab; gm.seg1_delta = P.seg1_delta;
#ifdef DWM_ATTN_TRACE
                res_unit<1>(c, q, op, P.scale_log2, force_safe, gm, fetch_next_q,
                            (P.lse != nullptr && blockIdx.x < 8 && lane == 0 && g < 64 && r == 0) ? (long long*)P.lse + (((int)blockIdx.x * NW + wave) * 64 + g) * 8 : nullptr);
#else
                res_unit<1>(c, q, op, P.scale_log2, force_safe, gm, fetch_next_q);
#endif
                if (r == 0) DWM_TR(3);
            }
        }
        DWM_TR(6);
        __syncthreads();                                     // everybody is done with this head's images
        DWM_TR(7);
        if (new_item_next) build_tab(nullptr, otab, nprob);  // the output row table of the next item (this item's is no longer read)
        if (has_next) {
            copy_rows(ntab, nhoff, 0, n, false, wave, NW);
            copy_rows(ntab, nhoff, 0, n, true, wave, NW);
        }
    }
}

// diagnostic: every lane issues one ds_read_b64_tr_b16 at byte offset offs[lane] of an LDS
// image holding lds16[i] = i, and reports its 4 result elements (hardware-semantics probe).
__global__ void __launch_bounds__(64)
tr_probe_kernel(const int* __restrict__ offs, short* __restrict__ out) {
    __shared__ __attribute__((aligned(16))) short img[4096];
    const int lane = threadIdx.x;
    for (int i = lane; i < 4096; i += 64) img[i] = (short)i;
    __syncthreads();
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
        (__attribute__((address_space(3))) s16x4*)((char*)img + offs[lane]));
#pragma unroll
    for (int j = 0; j < 4; ++j) out[lane * 4 + j] = v[j];
}

// ---- host side: plan (which kernel, which geometry, which parameter block), then launch

enum class AttnKernel { SMALL, GROUP_LDS, GROUP, STREAM, RES, TILED };
struct AttnPlan {
    AttnKernel kernel;
    unsigned grid, block;
    size_t lds;                 // dynamic LDS bytes
    int qt, mask;               // TILED: attn_fwd_kernel<qt, mask>
    int sl;                     // SMALL: attn_small_kernel<sl>
    int g;                      // GROUP_LDS: attn_group_lds_kernel<g>
};

// Heads per workgroup: variant bits 8-11 (1..15) when set - the caller checks that they divide `heads` - otherwise the first of the
// kernel's candidates that divides `heads` and leaves at least min_items (problem, head group) items, 1 if none does.
int heads_per_wg(const AttnParams& P, int asked, std::initializer_list<int> candidates, int64_t min_items = 0) {
    if (asked != 0) return asked;
    for (const int h : candidates)
        if (P.heads % h == 0 && (int64_t)P.n_problems * (P.heads / h) >= min_items) return h;
    return 1;
}
bool set_heads_per_wg(AttnParams& P, int h) {
    if (P.heads % h != 0) return false;
    P.hpb = h;
    P.fd_heads = make_fastdiv((uint32_t)(P.heads / h));
    return true;
}

// Kernel selection, in order of precedence (host arithmetic only; `ncu` = CUs of the device).  Completes P for the chosen kernel.
//   0. preconditions of every launch, whichever kernel serves it: the tiled kernel's heads per workgroup must divide `heads`
//      (DWM_EINVAL), its grid must stay below 2^31 workgroups and its K / V ring + row table must fit the LDS window
//      (DWM_EUNSUPPORTED).  Every kernel then checks its own heads per workgroup (DWM_EINVAL) and grid (DWM_EUNSUPPORTED).
//   1. SMALL (attn_small_kernel): L <= 32, one segment, no mask, no LSE - point-wise temporal attention.
//   2. group-masked (mask_mode 1, one segment, no LSE, G whole groups of 8..32 tokens - row-wise cross-view attention):
//      GROUP_LDS for G = 4 / 6 / 8 (one workgroup per (problem, head group), K / V of a head copied to LDS once: 6 views are the
//      camera rigs of every shipped config) unless bit 7; else GROUP (one wave per query group).
//   3. resident (no mask, no LSE, not cross, 64 <= L <= 608: the K / V rows of one head fit the LDS), persistent, one workgroup
//      per CU: STREAM (attention_stream.hip) for 8..20 query tiles (225 <= L <= 608) unless bit 13 or bits 0-3 are set or the
//      launch is one stream_covers() declines; else RES (attn_res_kernel<12>, bits 0-3 = compute waves).
//   4. TILED (attn_fwd_kernel): everything else; 64 queries per wave on request (bits 0-3 = 2) or by the automatic rule below.
// Variant bit 5 skips 1-3 (A/B measurements, tests); bit 4 (online softmax for every unit) is read by the resident kernels only;
// bits 8-11 override the heads per workgroup of whichever kernel runs; bit 12 is accepted and ignored (older callers: "the
// streaming form"); bit 15 is not a kernel choice (fill_params).
int plan_attention(AttnParams& P, int variant, bool cross, int ncu, AttnPlan& plan) {
    const int v_waves = variant & 15;                       // bits 0-3: queries per wave (tiled) / compute waves (resident)
    const bool v_safe_softmax = ((variant >> 4) & 1) != 0;
    const bool v_tiled_only = ((variant >> 5) & 1) != 0;
    const bool v_group_per_wave = ((variant >> 7) & 1) != 0;
    const int v_heads = (variant >> 8) & 15;
    const bool v_keep_res = ((variant >> 13) & 1) != 0;
    const int64_t L = P.L;
    plan = AttnPlan();
    plan.block = 256;

    // tiled kernel: 2 = 64 queries per wave (256 per workgroup); anything else = 32 (3 workgroups per CU: measured faster in the
    // full step).
    // (automatic: 64 queries per wave from L = 1024 on - the UNet's spatial self-attention at L = 1792: 808-843 against 685-715 TFLOP/s;
    //  "full" temporal attention, 19 frames x 448 tokens = 8512 in the shipped UniMLVG example: 628 against 522 TFLOP/s,
    //  profiles/r5y_microbench_attention.log; variant bits 0-3 = 1 keeps 32)
    // (the automatic rule covers what was measured: unmasked inference launches whose 256-query blocks still fill the CUs; masked,
    //  LSE-producing (training) and small-grid launches keep 32 queries per wave unless the caller asks)
    const int64_t blocks64 = (int64_t)P.n_problems * P.heads * ((P.qend + 255) / 256);
    const bool auto64 = v_waves == 0 && L - P.kbeg >= 1024 && P.mask_mode == 0 && P.lse == nullptr && blocks64 >= 512;
    const int qt = v_waves == 2 || auto64 ? 2 : 1;
    P.nqb = (int)((P.qend + qt * 128 - 1) / (qt * 128));
    P.fd_nqb = make_fastdiv((uint32_t)P.nqb);
    P.safe_softmax = v_safe_softmax;
    // heads per workgroup amortise the per-workgroup fixed cost.  Measured on the step's shapes (L = 168 .. 602): 2 ~ 3 > 1;
    // single-tile problems (L <= 64) take more.
    if (!set_heads_per_wg(P, L - P.kbeg <= KT ? heads_per_wg(P, v_heads, {6, 5, 4, 3, 2}) : heads_per_wg(P, v_heads, {2, 3}))) return DWM_EINVAL;
    const int64_t tiled_grid = (int64_t)P.n_problems * (P.heads / P.hpb) * P.nqb;
    if (tiled_grid >= (1ll << 31)) return DWM_EUNSUPPORTED;
    if (NSTAGE * STAGE_BYTES + L * 4 + 16 > MAX_LDS_BYTES) return DWM_EUNSUPPORTED;

    if (!v_tiled_only && L <= 32 && P.L1 == 0 && P.mask_mode == 0 && P.lse == nullptr) {
        if (!set_heads_per_wg(P, heads_per_wg(P, v_heads, {8, 7, 6, 5, 4, 3, 2}))) return DWM_EINVAL;
        plan.kernel = AttnKernel::SMALL;
        plan.sl = L <= 8 ? 8 : L <= 16 ? 16 : 32;
        const int64_t ngrp = ((int64_t)P.n_problems + 32 / plan.sl - 1) / (32 / plan.sl);
        const int64_t nblk = ((ngrp + 3) / 4) * (P.heads / P.hpb);
        if (nblk >= (1ll << 31)) return DWM_EUNSUPPORTED;
        plan.grid = (unsigned)nblk;
        return DWM_OK;
    }
    if (!v_tiled_only && P.mask_mode == 1 && P.L1 == 0 && P.lse == nullptr && P.group_size >= 8 && P.group_size <= 32 &&
        (int64_t)P.mask_G * P.group_size == L) {
        // (GROUP_LDS: the double-buffered copy pipeline runs over the heads of a workgroup)
        if (!set_heads_per_wg(P, heads_per_wg(P, v_heads, {8, 7, 6, 5, 4, 3, 2}))) return DWM_EINVAL;
        const int G = P.mask_G;
        if ((G == 6 || G == 4 || G == 8) && !v_group_per_wave) {
            plan.kernel = AttnKernel::GROUP_LDS;
            plan.g = G;
            const int64_t nblk = (int64_t)P.n_problems * (P.heads / P.hpb);
            if (nblk >= (1ll << 31)) return DWM_EUNSUPPORTED;
            plan.grid = (unsigned)nblk;
            plan.block = (unsigned)G * 64;
            plan.lds = (size_t)4 * G * GRP_IMG + (size_t)G * 4096;        // two stages of K + V images, output regions
            return DWM_OK;
        }
        plan.kernel = AttnKernel::GROUP;
        const int64_t units = (int64_t)P.n_problems * G;
        const int64_t nblk = ((units + 3) / 4) * (P.heads / P.hpb);
        if (nblk >= (1ll << 31) || units >= (1ll << 31)) return DWM_EUNSUPPORTED;
        plan.grid = (unsigned)nblk;
        return DWM_OK;
    }
#ifdef DWM_ATTN_TRACE
    const bool res_lse_ok = true;              // the lse buffer is the trace buffer in this build
#else
    const bool res_lse_ok = P.lse == nullptr;
#endif
    if (!v_tiled_only && P.mask_mode == 0 && res_lse_ok && !cross && L <= 608 && L >= 64) {
        // heads per item: as many as leave >= 3 items per CU
        if (!set_heads_per_wg(P, heads_per_wg(P, v_heads, {6, 5, 4, 3, 2}, 768))) return DWM_EINVAL;
        const int64_t nitems = (int64_t)P.n_problems * (P.heads / P.hpb);
        if (nitems >= (1ll << 31)) return DWM_EUNSUPPORTED;
        plan.grid = (unsigned)(nitems < ncu ? nitems : ncu);               // persistent: one workgroup per CU
        P.nwc = v_waves == 0 ? 12 : v_waves;                               // compute waves (12 = all)
        if (P.nwc > 12) return DWM_EINVAL;
        // the one-wave-per-SIMD streaming form (4 waves, all query tiles of a wave in one pass over the keys, V double-buffered in
        // LDS, K fragments from global memory, Q in AGPRs): 778-808 against 740-755 TFLOP/s at L = 602, 655-690 against 590-610 at
        // L = 448 (profiles/r6g2_*)
        const int nqt = (P.qend + 31) >> 5;
        if (!v_keep_res && v_waves == 0 && nqt >= 8 && nqt <= 20 && stream_covers(P)) {
            plan.kernel = AttnKernel::STREAM;
            plan.lds = stream_lds_bytes(P.L);                              // (what its launcher asks for)
            P.stream_far = stream_far(P);
            return DWM_OK;
        }
        plan.kernel = AttnKernel::RES;
        plan.block = 768;
        plan.lds = (size_t)2 * ((L + 31) & ~31) * 128 + (size_t)3 * ((L + 3) & ~3) * sizeof(int32_t);
        return DWM_OK;
    }
    plan.kernel = AttnKernel::TILED;
    plan.qt = qt;
    plan.mask = P.mask_mode;
    plan.grid = (unsigned)tiled_grid;
    plan.lds = NSTAGE * STAGE_BYTES + (size_t)((P.L + 3) & ~3) * sizeof(int32_t);
    return DWM_OK;
}

int launch_small(const AttnParams& P, const AttnPlan& pl, hipStream_t s) {
    const dim3 grid(pl.grid), block(pl.block);
    if (pl.sl == 8) hipLaunchKernelGGL((attn_small_kernel<8>), grid, block, 0, s, P);
    else if (pl.sl == 16) hipLaunchKernelGGL((attn_small_kernel<16>), grid, block, 0, s, P);
    else hipLaunchKernelGGL((attn_small_kernel<32>), grid, block, 0, s, P);
    return dwm_launch_status();
}

template <int G>
int launch_group_lds_g(const AttnParams& P, const AttnPlan& pl, hipStream_t s) {
    const hipError_t e = dwm_allow_dynamic_lds<attn_group_lds_kernel<G>>(160 * 1024);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((attn_group_lds_kernel<G>), dim3(pl.grid), dim3(pl.block), pl.lds, s, P);
    return dwm_launch_status();
}
int launch_group_lds(const AttnParams& P, const AttnPlan& pl, hipStream_t s) {
    return pl.g == 6 ? launch_group_lds_g<6>(P, pl, s) : pl.g == 4 ? launch_group_lds_g<4>(P, pl, s) : launch_group_lds_g<8>(P, pl, s);
}

int launch_group(const AttnParams& P, const AttnPlan& pl, hipStream_t s) {
    hipLaunchKernelGGL(attn_group_kernel, dim3(pl.grid), dim3(pl.block), 0, s, P);
    return dwm_launch_status();
}

int launch_res(const AttnParams& P, const AttnPlan& pl, hipStream_t s) {
    const hipError_t e = dwm_allow_dynamic_lds<attn_res_kernel<12>>(160 * 1024);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((attn_res_kernel<12>), dim3(pl.grid), dim3(pl.block), pl.lds, s, P);
    return dwm_launch_status();
}

template <int QT, int MASK>
int launch_tiled_qm(const AttnParams& P, const AttnPlan& pl, hipStream_t s) {
    const hipError_t e = dwm_allow_dynamic_lds<attn_fwd_kernel<QT, MASK>>(MAX_LDS_BYTES);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL((attn_fwd_kernel<QT, MASK>), dim3(pl.grid), dim3(pl.block), pl.lds, s, P);
    return dwm_launch_status();
}
int launch_tiled(const AttnParams& P, const AttnPlan& pl, hipStream_t s) {
    if (pl.qt == 1) return pl.mask == 0 ? launch_tiled_qm<1, 0>(P, pl, s) : pl.mask == 1 ? launch_tiled_qm<1, 1>(P, pl, s) : launch_tiled_qm<1, 2>(P, pl, s);
    return pl.mask == 0 ? launch_tiled_qm<2, 0>(P, pl, s) : pl.mask == 1 ? launch_tiled_qm<2, 1>(P, pl, s) : launch_tiled_qm<2, 2>(P, pl, s);
}

}  // namespace

// attention_stream.hip: the STREAM launch (attn_stream_kernel lives in that translation unit)
int dwm_attn_stream_launch(const dwm_attn::AttnParams& P, unsigned nblk, hipStream_t s);

extern "C" int dwm_attention_fwd(const dwm_attn_args* a, void* stream) {
    AttnParams P;
    int rc = fill_params(a, P);
    if (rc != DWM_OK) return rc;
    AttnPlan plan;
    rc = plan_attention(P, a->variant, a->cross != 0, dwm_cu_count(), plan);
    if (rc != DWM_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    switch (plan.kernel) {
        case AttnKernel::SMALL: return launch_small(P, plan, s);
        case AttnKernel::GROUP_LDS: return launch_group_lds(P, plan, s);
        case AttnKernel::GROUP: return launch_group(P, plan, s);
        case AttnKernel::STREAM: return dwm_attn_stream_launch(P, plan.grid, s);
        case AttnKernel::RES: return launch_res(P, plan, s);
        default: return launch_tiled(P, plan, s);
    }
}

extern "C" int dwm_debug_tr_probe(const int32_t* offs, int16_t* out, void* stream) {
    if (offs == nullptr || out == nullptr) return DWM_EINVAL;
    hipLaunchKernelGGL(tr_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)offs, (short*)out);
    return dwm_launch_status();
}
