// wanda_k7.h — what the K7 translation units share (wanda.hip, wanda_rows_*.hip, wanda_matrix.hip;
// colsq.hip takes the phase clock from here): the phase clock, the group prefix search, the metric,
// the 256-thread scan, the dtype switch, and the plain host interface between wanda.hip (checks,
// workspace, rows planning) and the per-dtype rows units.  The rows kernels themselves are in
// wanda_rows.h, which only the rows units include.
#pragma once
#include "common.h"

// Phase clock for the K6 / K7 matrix-mode kernels, compiled in only by tools/diag/k7_clock.sh
// (-DECO_K7_CLOCK, its own .so): workgroup 0 stamps the 100 MHz wall clock at its phase boundaries,
// every workgroup folds its entry / exit into a min / max.
#ifdef ECO_K7_CLOCK
__device__ unsigned long long eco_k7_clk[8][16];
#define K7_STAMP(k, i) do { if (threadIdx.x == 0 && blockIdx.x == 0) eco_k7_clk[k][i] = wall_clock64(); } while (0)
#define K7_ENTER(k) do { if (threadIdx.x == 0) atomicMin(&eco_k7_clk[k][14], wall_clock64()); } while (0)
#define K7_EXIT(k) do { if (threadIdx.x == 0) atomicMax(&eco_k7_clk[k][15], wall_clock64()); } while (0)
extern "C" int ecoflap_debug_k7_clock_reset(void) {
    unsigned long long z[8][16];
    for (int k = 0; k < 8; ++k) for (int i = 0; i < 16; ++i) z[k][i] = i == 14 ? ~0ull : 0ull;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(eco_k7_clk), z, sizeof(z));
}
extern "C" int ecoflap_debug_k7_clock_read(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(eco_k7_clk), sizeof(unsigned long long) * 8 * 16);
}
#else
#define K7_STAMP(k, i) do { } while (0)
#define K7_ENTER(k) do { } while (0)
#define K7_EXIT(k) do { } while (0)
#endif

// Block-level launches: every K7 kernel below serves up to ECOFLAP_WANDA_MAX_ITEMS matrices (all
// the Linears of one transformer block) from ONE launch; the item of a workgroup / wave is found
// from a prefix table in the kernel arguments (wave-uniform scalar search).
#define WMAX ECOFLAP_WANDA_MAX_ITEMS

template <typename G>
static __device__ __forceinline__ int group_item(const G& g, int64_t idx) {
    int it = 0;
    while (it + 1 < g.n && idx >= g.start[it + 1]) ++it;
    return it;
}

template <int DT>
static __device__ __forceinline__ uint32_t metric_bits(const void* w, int64_t i, float sq) {
    return __float_as_uint(__builtin_fabsf(Vec<DT>::load1(w, i)) * sq);
}

// inclusive scan of one value per thread over a 256-thread block; returns (inclusive, total)
static __device__ __forceinline__ uint32_t block_scan_256(uint32_t v, uint32_t* lds_wave4,
                                                          uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    __syncthreads();  // protect lds_wave4 reuse
    if (lane == 63) lds_wave4[wave] = x;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < wave) base += lds_wave4[k];
    }
    total = lds_wave4[0] + lds_wave4[1] + lds_wave4[2] + lds_wave4[3];
    return x + base;
}

static inline bool item_vector_ok(const ecoflap_wanda_item& it, const float* sq) {
    const int nvec_elems = it.dtype == ECOFLAP_F32 ? 4 : 8;
    // mask rows are written with 4/8-byte stores: cols % 8 keeps them aligned for 16-bit dtypes
    return it.cols % nvec_elems == 0 && aligned16(it.w) && aligned16(sq) &&
           (!it.mask_out || (((uintptr_t)it.mask_out) & 7u) == 0);
}

#define DT_SWITCH(dt, CALL)                                    \
    do {                                                       \
        if ((dt) == ECOFLAP_F32) { CALL(ECOFLAP_F32); }        \
        else if ((dt) == ECOFLAP_F16) { CALL(ECOFLAP_F16); }   \
        else { CALL(ECOFLAP_BF16); }                           \
    } while (0)

// ---- K7 rows mode: what the host planner (wanda.hip) and the rows units share --------------------
#define WANDA_ROWS_MAX_COLS 15360  // metric bits + histogram stay under 64 KiB of LDS

struct RowsGroup {
    int n;
    int32_t start[WMAX + 1];      // row prefix over the group's matrices
    void* w[WMAX];
    const float* sq[WMAX];
    int64_t cols[WMAX];
    int64_t k[WMAX];
    uint8_t* mask[WMAX];
};

#define ROWS_WAVE_MAX_NVEC 256                           // 4 vectors per lane (2048 bf16 columns)
#define ROWS_FUSE_MAX_NVEC 1024                          // workgroup-form rows that may share a grid: 4 vectors per thread
static inline int rows_wave_class(int64_t nvec) {       // vectors per lane, one wave per row
    const int nv = (int)((nvec + 63) / 64);
    return nv <= 1 ? 1 : (nv <= 2 ? 2 : (nv <= 4 ? 4 : 0));
}
static inline int rows_reg_class(int64_t nvec) {        // vectors per thread, one workgroup per row
    const int nv = (int)((nvec + 255) / 256);
    static const int classes[] = {1, 2, 3, 4, 6, 8, 12, 16};
    for (int c : classes)
        if (nv <= c) return c;
    return 0;
}

// The rows launchers are templates on the dtype (wanda_rows.h); each dtype's instances are compiled
// in a translation unit of their own (wanda_rows_f32.hip, _f16.hip, _bf16.hip) behind these plain
// functions, so that the three compile side by side.  `cls` is the group's register class
// (rows_wave_class / rows_reg_class).  They only launch: the caller checks the launch.
#define K7_ROWS_DECLARE(SUFFIX_)                                                                        \
    void wanda_rows_launch_##SUFFIX_(bool wave, const RowsGroup& g, int cls, hipStream_t s);           \
    void wanda_rows_fused_launch_##SUFFIX_(const RowsGroup& gw, int cls_w, const RowsGroup& gr,        \
                                           int cls_r, hipStream_t s);                                  \
    void wanda_rows_lds_launch_##SUFFIX_(void* w, const float* sq, int64_t rows, int64_t cols,         \
                                         int64_t k, uint8_t* mask_out, hipStream_t s)
K7_ROWS_DECLARE(f32);
K7_ROWS_DECLARE(f16);
K7_ROWS_DECLARE(bf16);
#undef K7_ROWS_DECLARE
