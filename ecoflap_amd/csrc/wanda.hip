// wanda.hip — K6 / K7 / K8: Wanda calibration statistic, metric + selection +
// zeroing, and mask apply, for gfx950.
//
// Replaces
//   K6  WrappedGPT.add_batch           LAVIS/lavis/compression/pruners/wanda_pruner.py:71-84
//   K7  |W| * sqrt(scaler_row), sort, select, zero
//         rows mode   (T5/BERT)         wanda_pruner.py:260, :272-279
//         matrix mode (ViT)             wanda_pruner.py:541, :555-558
//   K8  grad *= mask                    UPop/ecoflap_compression_vqa.py:124-129
//
// All HBM-bound byte/element work: 16-byte coalesced loads, selection by radix
// select on the fp32 metric's bit pattern (metrics are >= +0 so the unsigned
// order of the bits IS the float order; NaN sorts last like torch.sort), LDS
// histograms, no GEMM reshaping.
// Algorithmic bytes: K6 tokens*cols*s_x; K7 2*s per element + 4*cols.
//
// This file: the K7 entries (argument checks, workspace, the sqrt launch, rows planning), the n:m
// kernel and K8.  The kernels of K7 live by family: wanda_rows.h (rows mode, one translation unit
// per dtype), wanda_matrix.hip (matrix mode); K6 is colsq.hip; wanda_k7.h holds what they share.
#include "wanda_matrix_state.h"

// =====================================================================================
// K7 common: sqrt(scaler_row) once per matrix (correctly rounded, = torch.sqrt)
// =====================================================================================
struct SqrtGroup {
    int n;
    int32_t start[WMAX + 1];      // workgroup prefix (256 columns each)
    const float* src[WMAX];
    float* dst[WMAX];
    int64_t cols[WMAX];
    uint32_t* zero[WMAX];         // matrix mode: the item's selection state, cleared here (no memset launch)
    int zero_words;
};
__global__ __launch_bounds__(256) void sqrt_cols_kernel(const SqrtGroup g) {
    const int it = group_item(g, blockIdx.x);
    const int lb = blockIdx.x - g.start[it], nb = g.start[it + 1] - g.start[it];
    const int64_t c = (int64_t)lb * 256 + threadIdx.x;
    if (c < g.cols[it]) g.dst[it][c] = __builtin_sqrtf(g.src[it][c]);
    if (g.zero[it])
        for (int i = lb * 256 + threadIdx.x; i < g.zero_words; i += nb * 256) g.zero[it][i] = 0u;
}

static inline size_t sq_bytes(int64_t cols) { return (((size_t)cols * sizeof(float) + 255) / 256) * 256; }

extern "C" size_t ecoflap_wanda_workspace_bytes(int64_t rows, int64_t cols) {
    (void)rows;
    if (cols <= 0) return 0;
    // sqrt table (padded to 256 B) + matrix-mode selection states
    return sq_bytes(cols) + sizeof(MatrixSelState) + sizeof(BracketState) + WS_PART_BYTES;
}

extern "C" size_t ecoflap_wanda_block_workspace_bytes(const ecoflap_wanda_item* items, int n_items) {
    size_t total = 0;
    if (!items) return 0;
    for (int i = 0; i < n_items; ++i)
        if (items[i].cols > 0)
            total += sq_bytes(items[i].cols) + sizeof(MatrixSelState) + sizeof(BracketState);
    return total ? total + WS_PART_BYTES : 0;
}

// FN_f32 / FN_f16 / FN_bf16 (ARGS): the rows units' entries (wanda_k7.h) by dtype
#define ROWS_DT(dt, FN, ...)                                       \
    do {                                                           \
        if ((dt) == ECOFLAP_F32) FN##_f32(__VA_ARGS__);            \
        else if ((dt) == ECOFLAP_F16) FN##_f16(__VA_ARGS__);       \
        else FN##_bf16(__VA_ARGS__);                               \
    } while (0)

// the argument checks of ecoflap_wanda_prune_block after the item count's; their order and codes are
// part of the C ABI (tests/test_cabi_exports.py), and no HIP call comes before they pass
static int block_check(const ecoflap_wanda_item* items, int n_items, void* workspace, size_t workspace_bytes) {
    if (!items) return ECOFLAP_ENULL;
    for (int i = 0; i < n_items; ++i) {
        const ecoflap_wanda_item& it = items[i];
        if (!dtype_ok(it.dtype)) return ECOFLAP_EDTYPE;
        if (it.mode != ECOFLAP_WANDA_ROWS && it.mode != ECOFLAP_WANDA_MATRIX) return ECOFLAP_EMODE;
        if (it.rows <= 0 || it.cols <= 0 || it.k < 0) return ECOFLAP_ESIZE;
        if (it.mode == ECOFLAP_WANDA_ROWS && it.cols > WANDA_ROWS_MAX_COLS) return ECOFLAP_ESIZE;
        // the reference indexes sorted[k]: k == numel raises IndexError there (W:555)
        if (it.mode == ECOFLAP_WANDA_MATRIX &&
            (it.k >= it.rows * it.cols || it.rows * it.cols >= (int64_t)0xffffffffLL))
            return ECOFLAP_ESIZE;
        if (it.rows > 0x7fffffffLL / 2) return ECOFLAP_ESIZE;
        if (!it.w || !it.scaler_row) return ECOFLAP_ENULL;
    }
    if (!workspace) return ECOFLAP_ENULL;
    if (workspace_bytes < ecoflap_wanda_block_workspace_bytes(items, n_items)) return ECOFLAP_EWORKSPACE;
    return 0;
}

// sqrt(scaler_row) of the items that `want` it, and the cleared selection state of every
// matrix-mode item, in one launch
static int launch_sqrt(const ecoflap_wanda_item* items, int n_items, float* const* sq,
                       MatrixSelState* const* st, const bool* want, hipStream_t s) {
    SqrtGroup g;
    g.n = n_items;
    g.zero_words = (int)(sizeof(MatrixSelState) / sizeof(uint32_t));
    g.start[0] = 0;
    for (int i = 0; i < n_items; ++i) {
        g.src[i] = items[i].scaler_row; g.dst[i] = sq[i]; g.cols[i] = items[i].cols;
        g.zero[i] = items[i].mode == ECOFLAP_WANDA_MATRIX ? (uint32_t*)st[i] : nullptr;
        g.start[i + 1] = g.start[i] + (want[i] ? (int32_t)((items[i].cols + 255) / 256) : 0);
    }
    if (g.start[n_items] == 0) return 0;
    hipLaunchKernelGGL(sqrt_cols_kernel, dim3((unsigned)g.start[n_items]), dim3(256), 0, s, g);
    ECO_CHECK_LAUNCH();
    return 0;
}

// ---- rows mode -------------------------------------------------------------------------
// Groups of one (dtype, form, register class) each; a wave-form group and a workgroup-form
// group of the same dtype share one grid when the long rows fit 4 vectors per thread.
static int rows_plan_and_launch(const ecoflap_wanda_item* items, int n_items, float* const* sq, bool* done,
                                hipStream_t s) {
    struct Pending { RowsGroup g; int dtype, cls; bool wave, used; };
    static thread_local Pending pend[8];
    int n_pend = 0;
    for (int i = 0; i < n_items; ++i) {
        if (done[i] || items[i].mode != ECOFLAP_WANDA_ROWS) continue;
        const ecoflap_wanda_item& a = items[i];
        const int nve = a.dtype == ECOFLAP_F32 ? 4 : 8;
        if (!item_vector_ok(a, sq[i])) {     // odd widths / unaligned views: the LDS form, per matrix
            ROWS_DT(a.dtype, wanda_rows_lds_launch, a.w, sq[i], a.rows, a.cols, a.k, a.mask_out, s);
            ECO_CHECK_LAUNCH();
            done[i] = true;
            continue;
        }
        // measured on MI355X: the wave form wins up to 256 vectors per row (2048 bf16 columns)
        const int64_t nvec = a.cols / nve;
        const bool wave = nvec <= ROWS_WAVE_MAX_NVEC;
        const int cls = wave ? rows_wave_class(nvec) : rows_reg_class(nvec);
        if (n_pend == 8) {                   // more classes than slots: flush what is pending
            for (int q = 0; q < n_pend; ++q) {
                Pending& P = pend[q];
                ROWS_DT(P.dtype, wanda_rows_launch, P.wave, P.g, P.cls, s);
                ECO_CHECK_LAUNCH();
            }
            n_pend = 0;
        }
        Pending& P = pend[n_pend++];
        P.dtype = a.dtype; P.cls = cls; P.wave = wave; P.used = false;
        RowsGroup& g = P.g;
        g.n = 0;
        g.start[0] = 0;
        for (int j = i; j < n_items; ++j) {
            const ecoflap_wanda_item& b = items[j];
            if (done[j] || b.mode != ECOFLAP_WANDA_ROWS || b.dtype != a.dtype || !item_vector_ok(b, sq[j]))
                continue;
            const int64_t nvb = b.cols / nve;
            const bool wb = nvb <= ROWS_WAVE_MAX_NVEC;
            if (wb != wave || (wb ? rows_wave_class(nvb) : rows_reg_class(nvb)) != cls) continue;
            if ((int64_t)g.start[g.n] + b.rows > 0x3fffffffLL) continue;   // next group
            g.w[g.n] = b.w; g.sq[g.n] = sq[j]; g.cols[g.n] = b.cols; g.k[g.n] = b.k; g.mask[g.n] = b.mask_out;
            g.start[g.n + 1] = g.start[g.n] + (int32_t)b.rows;
            ++g.n;
            done[j] = true;
        }
    }
    for (int q = 0; q < n_pend; ++q) {
        Pending& P = pend[q];
        if (P.used) continue;
        P.used = true;
        Pending* mate = nullptr;             // the other form, same dtype, long rows of <= 4 vectors per thread
        for (int r = q + 1; r < n_pend && !mate; ++r) {
            Pending& Q = pend[r];
            if (Q.used || Q.dtype != P.dtype || Q.wave == P.wave) continue;
            const Pending& longer = P.wave ? Q : P;
            if (longer.cls <= 4) mate = &Q;
        }
        if (mate) {
            mate->used = true;
            const Pending& W = P.wave ? P : *mate;
            const Pending& L = P.wave ? *mate : P;
            ROWS_DT(P.dtype, wanda_rows_fused_launch, W.g, W.cls, L.g, L.cls, s);
        } else {
            ROWS_DT(P.dtype, wanda_rows_launch, P.wave, P.g, P.cls, s);
        }
        ECO_CHECK_LAUNCH();
    }
    return 0;
}

// All Linears of one transformer block in one call: one sqrt launch, one selection launch per
// (dtype, register class) of the rows-mode matrices, 3 histogram launches + 1 apply launch for
// ALL matrix-mode matrices of a dtype — instead of 2 (rows) / 6 (matrix) launches per matrix.
// Besides the launch count this is what fills the chip: one T5 matrix has 2048-5120 rows (2-5
// waves per SIMD for the one-wave-per-row kernel), a T5 block has 18-28 thousand.
extern "C" int ecoflap_wanda_prune_block(const ecoflap_wanda_item* items, int n_items,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    if (n_items < 0 || n_items > WMAX) return ECOFLAP_ESIZE;
    if (n_items == 0) return 0;
    int rc = block_check(items, n_items, workspace, workspace_bytes);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)stream;

    // workspace: sqrt tables, then the selection states
    float* sq[WMAX];
    MatrixSelState* st[WMAX];
    char* p = (char*)workspace;
    for (int i = 0; i < n_items; ++i) { sq[i] = (float*)p; p += sq_bytes(items[i].cols); }
    for (int i = 0; i < n_items; ++i) {
        st[i] = (MatrixSelState*)p;      // cleared by the sqrt kernel below (matrix-mode items)
        p += sizeof(MatrixSelState);
    }
    BracketState* bst[WMAX];
    for (int i = 0; i < n_items; ++i) { bst[i] = (BracketState*)p; p += sizeof(BracketState); }
    uint32_t* part = (uint32_t*)p;

    bool sampled_item[WMAX], want[WMAX], done[WMAX];
    wanda_matrix_sampled(items, n_items, sq, sampled_item);
    for (int i = 0; i < n_items; ++i) { want[i] = !sampled_item[i]; done[i] = false; }
    rc = launch_sqrt(items, n_items, sq, st, want, s);
    if (rc) return rc;
    rc = rows_plan_and_launch(items, n_items, sq, done, s);
    if (rc) return rc;
    return wanda_matrix_launch(items, n_items, sq, st, bst, part, sampled_item, done, s);
}

static int wanda_single(void* w, const float* scaler_row, int64_t rows, int64_t cols, int dtype,
                        int64_t k, uint8_t* mask_out, int mode, void* workspace,
                        size_t workspace_bytes, void* stream) {
    ecoflap_wanda_item it;
    it.w = w; it.scaler_row = scaler_row; it.rows = rows; it.cols = cols; it.k = k;
    it.mask_out = mask_out; it.dtype = dtype; it.mode = mode;
    return ecoflap_wanda_prune_block(&it, 1, workspace, workspace_bytes, stream);
}

extern "C" int ecoflap_wanda_prune_rows(void* w, const float* scaler_row, int64_t rows,
                                        int64_t cols, int dtype, int64_t k, uint8_t* mask_out,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return wanda_single(w, scaler_row, rows, cols, dtype, k, mask_out, ECOFLAP_WANDA_ROWS, workspace,
                        workspace_bytes, stream);
}

extern "C" int ecoflap_wanda_prune_matrix(void* w, const float* scaler_row, int64_t rows,
                                          int64_t cols, int dtype, int64_t k, uint8_t* mask_out,
                                          void* workspace, size_t workspace_bytes, void* stream) {
    return wanda_single(w, scaler_row, rows, cols, dtype, k, mask_out, ECOFLAP_WANDA_MATRIX,
                        workspace, workspace_bytes, stream);
}

// =====================================================================================
// K7, structured n:m branch (wanda_pruner.py:265-270 = :546-551): in every group of m consecutive
// columns of a row the n smallest metrics are zeroed (`topk(..., largest=False)`: a NaN counts as
// the largest; equal metrics: the lower column first).  HBM-bound, one pass: 2*s*numel + 4*cols.
// One thread per group: the group's metrics as integer keys (non-negative floats order as their
// bits, NaN -> 0xffffffff), each element's rank by counting.
template <int DT>
__global__ __launch_bounds__(256) void wanda_nm_kernel(void* __restrict__ w, const float* __restrict__ scaler_row,
                                                       int64_t rows, int64_t cols, int n, int m,
                                                       uint8_t* __restrict__ mask_out) {
    const int64_t gpr = (cols + m - 1) / m;                    // groups per row
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= rows * gpr) return;
    const int64_t r = g / gpr, c0 = (g - r * gpr) * m;
    const int len = (int)(cols - c0 < m ? cols - c0 : m);
    uint32_t key[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        key[j] = 0xffffffffu;
        if (j < len) {
            const float v = __builtin_fabsf(Vec<DT>::load1(w, r * cols + c0 + j)) * __builtin_sqrtf(scaler_row[c0 + j]);
            key[j] = v != v ? 0xffffffffu : __float_as_uint(v);
        }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        if (j >= len) break;
        int rank = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i < len && i != j && (key[i] < key[j] || (key[i] == key[j] && i < j))) ++rank;
        const bool z = rank < n;
        if (z) Vec<DT>::store1(w, r * cols + c0 + j, 0.0f);
        if (mask_out) mask_out[r * cols + c0 + j] = z ? 1 : 0;
    }
}

extern "C" int ecoflap_wanda_prune_nm(void* w, const float* scaler_row, int64_t rows, int64_t cols,
                                      int dtype, int n, int m, uint8_t* mask_out, void* stream) {
    if (!dtype_ok(dtype)) return ECOFLAP_EDTYPE;
    if (rows < 0 || cols < 0 || n <= 0 || m < n || m > 16) return ECOFLAP_ESIZE;
    if (cols % m != 0 && cols % m < n) return ECOFLAP_ESIZE;       // (topk raises on the short slice)
    if (rows == 0 || cols == 0) return 0;
    if (!w || !scaler_row) return ECOFLAP_ENULL;
    const int64_t groups = rows * ((cols + m - 1) / m);
    if ((groups + 255) / 256 > 0x7fffffffLL) return ECOFLAP_ESIZE;
    const dim3 grid((unsigned)((groups + 255) / 256));
#define NM_GO(DT_) hipLaunchKernelGGL((wanda_nm_kernel<DT_>), grid, dim3(256), 0, (hipStream_t)stream, w, scaler_row, rows, cols, n, m, mask_out)
    DT_SWITCH(dtype, NM_GO);
#undef NM_GO
    ECO_CHECK_LAUNCH();
    return 0;
}

// =====================================================================================
// K8  grad *= mask
// =====================================================================================
// 16-byte vectors of the gradient, 8 (4) mask bytes per vector; scalar form for unaligned tails
template <int DT>
__global__ __launch_bounds__(256) void mask_mul_kernel(void* g, const uint8_t* __restrict__ keep,
                                                       int64_t n) {
    constexpr int N = Vec<DT>::N;
    const int64_t stride = (int64_t)gridDim.x * 256;
    const bool vec = (((uintptr_t)g) & 15u) == 0 && (((uintptr_t)keep) & (N - 1)) == 0;
    const int64_t nvec = vec ? n / N : 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
        float f[N];
        Vec<DT>::unpack(ld16(g, v), f);
        uint32_t m0 = *(const uint32_t*)(keep + v * N), m1 = 0;
        if (N == 8) m1 = *(const uint32_t*)(keep + v * N + 4);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const uint32_t byte = ((e < 4 ? m0 : m1) >> (8 * (e & 3))) & 0xffu;
            f[e] = Vec<DT>::round(f[e] * (byte ? 1.0f : 0.0f));      // grad * mask, as the reference multiplies
        }
        st16(g, v, Vec<DT>::pack(f));
    }
    for (int64_t i = nvec * N + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float m = keep[i] ? 1.0f : 0.0f;
        Vec<DT>::store1(g, i, Vec<DT>::load1(g, i) * m);
    }
}

extern "C" int ecoflap_mask_mul(void* g, const uint8_t* keep_mask, int64_t n, int dtype,
                                void* stream) {
    if (!dtype_ok(dtype)) return ECOFLAP_EDTYPE;
    if (n < 0) return ECOFLAP_ESIZE;
    if (n == 0) return 0;
    if (!g || !keep_mask) return ECOFLAP_ENULL;
    int64_t b = (n / 8 + 256 * 2 - 1) / (256 * 2);            // ~2 vectors per thread
    if (b > 4096) b = 4096;
    if (b < 1) b = 1;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == ECOFLAP_F32)
        hipLaunchKernelGGL((mask_mul_kernel<ECOFLAP_F32>), dim3((unsigned)b), dim3(256), 0, s, g, keep_mask, n);
    else if (dtype == ECOFLAP_F16)
        hipLaunchKernelGGL((mask_mul_kernel<ECOFLAP_F16>), dim3((unsigned)b), dim3(256), 0, s, g, keep_mask, n);
    else
        hipLaunchKernelGGL((mask_mul_kernel<ECOFLAP_BF16>), dim3((unsigned)b), dim3(256), 0, s, g, keep_mask, n);
    ECO_CHECK_LAUNCH();
    return 0;
}
