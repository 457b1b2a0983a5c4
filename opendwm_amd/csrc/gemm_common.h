// Shared between gemm_bf16.hip (8-wave kernels, host entry points) and gemm_bf16_4w.hip (4-wave kernels): the row map on the device,
// the launch decision (GemmPlan) and the host-side pieces both translation units evaluate.
#pragma once
#include "common.h"
#include "dwm_hip.h"

namespace dwm_gemm {

// a dwm_rowmap2d with its divisions prepared
struct DevRowMap {
    FastDiv rw, rh;
    int64_t rpitch, ipitch, origin;
    int enabled, xstep;
};
// (false: not a valid map)
static inline bool make_dev_rowmap(const dwm_rowmap2d& r, DevRowMap& d) {
    d.enabled = r.rw > 0;
    d.xstep = r.xstep > 0 ? (int)r.xstep : 1;
    if (!d.enabled) { d.rw = make_fastdiv(1); d.rh = make_fastdiv(1); d.rpitch = d.ipitch = d.origin = 0; return true; }
    if (r.rh <= 0 || r.rw >= (1ll << 30) || r.rh >= (1ll << 30)) return false;
    d.rw = make_fastdiv((uint32_t)r.rw); d.rh = make_fastdiv((uint32_t)r.rh);
    d.rpitch = r.rpitch; d.ipitch = r.ipitch; d.origin = r.origin;
    return true;
}
DWM_DEVINL int64_t map_row(const DevRowMap& rm, int64_t m) {
    if (!rm.enabled) return m;
    const uint32_t q = fdiv((uint32_t)m, rm.rw), x = (uint32_t)m - q * rm.rw.d;
    const uint32_t i = fdiv(q, rm.rh), y = q - i * rm.rh.d;
    return (int64_t)i * rm.ipitch + (int64_t)y * rm.rpitch + (int64_t)x * rm.xstep + rm.origin;
}

// ---- the launch decision of dwm_gemm_bf16 (plan_gemm in gemm_bf16.hip writes it, the launch functions read it)
enum class GemmFamily {
    W4_FAST,        // gemm4w_kernel<epi, rf32, rs, false>
    W4_GENERAL,     // gemm4w_kernel<epi, rf32, rs, true>
    W8_SPLITK,      // gemm_bf16_kernel<EPI_SPLITK> over `ksplit` K ranges + splitk_finish_kernel
    W8_256,         // gemm_bf16_kernel<epi, fast, false, 0, rs>
    W8_128,         // gemm_bf16_kernel<epi, fast, false, 1, rs>
    W8_C32          // gemm_bf16_kernel<RESID, fast, true, 0, rs>: the fp32 residual stream
};
struct GemmPlan {
    GemmFamily family;
    int epi, rs;                // template coordinates (rs = 0: the RESID operands are read at run time)
    bool fast, rf32;
    int tc;                     // TileCfg of the 8-wave kernels
    int ntm, ntn;               // row / column tiles
    unsigned grid, block;
    int lds;                    // dynamic LDS bytes (with the pad of development builds where reserved bit 10 asks for it)
    int ksplit;                 // K ranges (1: no split)
    int gm;                     // raster group height: row tiles that share a W panel
};

// raster group height: 8 row tiles share a W panel in the XCD's L2 for K ~ 1.5 k; a long K (FF2: 6144) makes the A panel of
// 8 rows (25 MB) stream through it, 4 rows measured 3 % faster there
static inline int raster_group_height(int64_t K) { return K >= 4096 ? 4 : 8; }

static inline int64_t gemm_nout(const dwm_gemm_args& a) { return a.epilogue == DWM_EPI_GEGLU ? a.N / 2 : a.N; }
static inline int gemm_ntaps(const dwm_gemm_args& a) { return a.ntaps > 0 ? a.ntaps : 1; }
static inline int64_t gemm_k_per_tap(const dwm_gemm_args& a) { return a.ntaps > 0 ? a.k_per_tap : a.K; }

// ---- split-K: a tile grid that fills less than half of the 256 CUs and a long K (`nk` steps of 64).  The thresholds live here only.
static inline bool splitk_pays(int64_t tiles, int64_t nk) { return tiles <= 128 && nk >= 16; }
// The automatic rule of dwm_gemm_bf16, as far as its two users agree.  They part here ON PURPOSE (kept as found, the bench's bits
// depend on it): the 4-wave cover predicate declines a launch on this answer alone; the 8-wave planner additionally needs a 16-byte
// aligned workspace and no development knob (reserved bits 0 / 1), and may come back to one range after clamp_ksplit.  A launch
// in that gap runs the UNSPLIT 8-WAVE kernel, not a 4-wave one.
static inline bool auto_splitk(const dwm_gemm_args& a, int64_t tiles) {
    return (a.epilogue == DWM_EPI_PLAIN || a.epilogue == DWM_EPI_RESID) && a.workspace != nullptr && a.split_k == 0 &&
           a.C32 == nullptr && splitk_pays(tiles, a.K / 64);
}
// at least 8 K steps per range, at most `max_ranges`, and no more ranges than `avail` bytes hold (`range_bytes` each); the
// result may be < 1
static inline int clamp_ksplit(int ksplit, int64_t nk, int max_ranges, int64_t range_bytes, int64_t avail) {
    if (ksplit > nk / 8) ksplit = (int)(nk / 8);
    if (ksplit > max_ranges) ksplit = max_ranges;
    if ((int64_t)ksplit * range_bytes > avail) ksplit = (int)(avail / range_bytes);
    return ksplit;
}

}  // namespace dwm_gemm

// gemm_bf16_4w.hip.  dwm_gemm4w_covers: host arithmetic only - whether the 4-wave kernels serve the launch (`fast_only`: their fast
// form only), and if so the plan's family, coordinates and geometry.  dwm_gemm4w_launch: the launch of a plan it accepted.
bool dwm_gemm4w_covers(const dwm_gemm_args& a, bool fast_only, dwm_gemm::GemmPlan& plan);
int dwm_gemm4w_launch(const dwm_gemm_args& a, const dwm_gemm::GemmPlan& plan, hipStream_t s);
