// sparsegpt.hip — SparseGPT block step for gfx950.
//
// Replaces the inner part of SparseGPT.fasterprune
//   LAVIS/lavis/compression/pruners/sparsegpt_pruner.py:172-216
// for one block of <= 128 columns [i1, i2):
//   tmp    = W1**2 / diag(Hinv1)**2                               (:186)
//   thresh = sort(tmp.flatten())[int(tmp.numel() * sparsity)]     (:187)
//   mask1  = tmp <= thresh                                        (:188)
//   for i in range(count):  q = w masked; err = (w - q) / d;
//       W1[:, i:] -= err (x) Hinv1[i, i:]                         (:192-210)
//   W[:, i1:i2] = Q1 ;  Err1 kept for  W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:]   (:212-216)
//
// The Hessian accumulation (:71-82), the two Cholesky factorisations (:118-160) and the
// trailing update GEMM are plain library calls on the host side (torch.addmm / rocSOLVER);
// what is fused here is the part torch runs as ~1000 tiny kernels per block:
//   * threshold: k-th order statistic of tmp over rows x count by three histogram passes
//     (same scheme as the Wanda matrix mode: LDS histograms, integer atomics, every
//     workgroup resolves earlier passes itself);
//   * sweep: rows are independent, so ONE 64-lane wave owns a row: its <=128 block values
//     live in two registers per lane, Hinv1 sits in LDS, each of the `count` sequential steps
//     is a lane broadcast + a fully rounded fp32 divide + one multiply and one subtract per
//     lane (two roundings, as torch's outer-product-then-subtract; no fma contraction).
//
// The trailing update W[:, i2:] -= Err1 @ Hinv[i1:i2, i2:] (:216) is `ecoflap_sparsegpt_trailing`
// below, an fp32 MFMA kernel of this file, and `ecoflap_sparsegpt_matrix` queues the whole column
// sweep of one Linear — widen, every block step, every trailing update, round back — from one
// host call (CoOp/trainers/pruners/sparsegpt_pruner.py:176-189, :261-307).
// `ecoflap_sparsegpt_matrix_group` does the same for up to 8 Linears that share Hinv (q / k / v,
// gate / up of a decoder block) with the launches of ONE matrix per column block: the histogram and
// sweep bodies below are shared by the single and the grouped kernels.
#include "common.h"

struct SgptSelState {
    uint32_t hist[3][2048];
};

static __device__ __forceinline__ uint32_t sg_block_scan_256(uint32_t v, uint32_t* lds_wave4,
                                                             uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    __syncthreads();
    if (lane == 63) lds_wave4[wave] = x;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < wave) base += lds_wave4[k];
    total = lds_wave4[0] + lds_wave4[1] + lds_wave4[2] + lds_wave4[3];
    return x + base;
}

static __device__ __forceinline__ void sg_pick(const uint32_t* __restrict__ hist, int bins,
                                               uint32_t remaining, uint32_t* wave4, uint32_t* out2) {
    uint32_t carry = 0;
    for (int base = 0; base < bins; base += 256) {
        const uint32_t cnt = hist[base + threadIdx.x];
        uint32_t total;
        const uint32_t incl = sg_block_scan_256(cnt, wave4, total) + carry;
        const uint32_t excl = incl - cnt;
        if (excl < remaining && remaining <= incl) {
            out2[0] = (uint32_t)(base + threadIdx.x);
            out2[1] = remaining - excl;
        }
        carry += total;
    }
    __syncthreads();
}

static __device__ __forceinline__ void sg_resolve(const SgptSelState* st, int upto, uint32_t rank0,
                                                  uint32_t* wave4, uint32_t* out2, uint32_t& prefix,
                                                  uint32_t& remaining) {
    prefix = 0;
    remaining = rank0;
    if (upto >= 1) { sg_pick(st->hist[0], 2048, remaining, wave4, out2); prefix |= out2[0] << 21; remaining = out2[1]; __syncthreads(); }
    if (upto >= 2) { sg_pick(st->hist[1], 2048, remaining, wave4, out2); prefix |= out2[0] << 10; remaining = out2[1]; __syncthreads(); }
    if (upto >= 3) { sg_pick(st->hist[2], 1024, remaining, wave4, out2); prefix |= out2[0]; remaining = out2[1]; __syncthreads(); }
}

// tmp = w^2 / d^2 with torch's three roundings
static __device__ __forceinline__ uint32_t sg_metric_bits(float w, float d) {
    const float a = w * w;
    const float b = d * d;
    return __float_as_uint(a / b);
}

// one histogram pass over W[rows, i1:i1+count) into st->hist[PASS]; the whole workgroup calls it
template <int PASS>
static __device__ __forceinline__ void sg_hist_pass(const float* __restrict__ W, int64_t rows,
                                                    int64_t ldw, const float* __restrict__ Hinv,
                                                    int64_t ldh, int64_t i1, int count,
                                                    uint32_t rank0, SgptSelState* st) {
    constexpr int SHIFT = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
    constexpr int BITS = PASS == 2 ? 10 : 11;
    constexpr uint32_t HI_MASK = PASS == 0 ? 0u : (PASS == 1 ? 0xffe00000u : 0xfffffc00u);
    __shared__ uint32_t h[2048];
    __shared__ float diag[128];
    __shared__ uint32_t wave4[4];
    __shared__ uint32_t out2[2];
    for (int i = threadIdx.x; i < 2048; i += 256) h[i] = 0;
    if (threadIdx.x < count) diag[threadIdx.x] = Hinv[(i1 + threadIdx.x) * ldh + i1 + threadIdx.x];
    uint32_t prefix, remaining;
    sg_resolve(st, PASS, rank0, wave4, out2, prefix, remaining);
    __syncthreads();
    const int64_t n = rows * count;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
        const int64_t r = e / count;
        const int c = (int)(e - r * count);
        const uint32_t b = sg_metric_bits(W[r * ldw + i1 + c], diag[c]);
        if ((b & HI_MASK) == prefix) atomicAdd(&h[(b >> SHIFT) & ((1u << BITS) - 1u)], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (1 << BITS); i += 256)
        if (h[i]) atomicAdd(&st->hist[PASS][i], h[i]);
}

template <int PASS>
__global__ __launch_bounds__(256) void sgpt_hist_kernel(const float* __restrict__ W, int64_t rows,
                                                        int64_t ldw, const float* __restrict__ Hinv,
                                                        int64_t ldh, int64_t i1, int count,
                                                        uint32_t rank0, SgptSelState* st) {
    sg_hist_pass<PASS>(W, rows, ldw, Hinv, ldh, i1, count, rank0, st);
}

// ---- the members of a grouped sweep (`ecoflap_sparsegpt_matrix_group`) ---------------------------
// Member g owns rows [off[g], off[g] + rows[g]) of the stacked fp32 working copy and of Err; every
// off[g] is a multiple of SGT_WG_ROWS, so a sweep workgroup never holds rows of two members; the
// rows between a member's last row and the next offset are padding (zero in the working copy, never
// counted into a histogram, never written back).  Passed by value; read with constant indices only
// (a dynamic index into kernel arguments would go through scratch).
#define SGPT_MAX_GROUP ECOFLAP_SGPT_MAX_GROUP
#define SGT_WG_ROWS 4
struct SgptGroup {
    int64_t off[SGPT_MAX_GROUP];
    int64_t rows[SGPT_MAX_GROUP];
    uint32_t rank0[SGPT_MAX_GROUP];
    int n;
};

// grid (x, n members): member blockIdx.y's elements are counted into ITS state st[blockIdx.y] only
template <int PASS>
__global__ __launch_bounds__(256) void sgpt_hist_group_kernel(const float* __restrict__ W, int64_t ldw,
                                                              const float* __restrict__ Hinv, int64_t ldh,
                                                              int64_t i1, int count, SgptGroup grp,
                                                              SgptSelState* st) {
    int64_t off = grp.off[0], rows = grp.rows[0];
    uint32_t rank0 = grp.rank0[0];
#pragma unroll
    for (int k = 1; k < SGPT_MAX_GROUP; ++k)
        if (k == (int)blockIdx.y) { off = grp.off[k]; rows = grp.rows[k]; rank0 = grp.rank0[k]; }
    sg_hist_pass<PASS>(W + off * ldw, rows, ldw, Hinv, ldh, i1, count, rank0, st + blockIdx.y);
}

// one wave per row; workgroup = 4 rows sharing Hinv1 in LDS.  The whole workgroup calls this with
// ONE (rank0, st) — it resolves the threshold behind barriers; `row` is the wave's row of W and Err,
// `live` false for a wave without a row (it leaves after the barriers).
static __device__ __forceinline__ void sg_sweep_rows(float* W, int64_t ldw,
                                                     const float* __restrict__ Hinv, int64_t ldh,
                                                     int64_t i1, int count, uint32_t rank0,
                                                     const SgptSelState* st, int use_thresh,
                                                     const uint8_t* __restrict__ mask_in,
                                                     float* __restrict__ Err, uint8_t* mask_out,
                                                     int nm_n, int nm_m, int64_t row, bool live) {
    // upper triangle of Hinv1, packed: row i starts at i*count - i*(i-1)/2, holds j = i..count-1
    extern __shared__ __attribute__((aligned(16))) float Hs[];
    __shared__ uint32_t wave4[4];
    __shared__ uint32_t out2[2];
#define HS(i, j) Hs[(i) * count - (((i) * ((i) - 1)) >> 1) + ((j) - (i))]
    for (int e = threadIdx.x; e < count * count; e += 256) {
        const int i = e / count, j = e - i * count;
        if (j >= i) HS(i, j) = Hinv[(i1 + i) * ldh + i1 + j];
    }
    uint32_t thres_bits = 0, remaining;
    if (use_thresh) sg_resolve(st, 3, rank0, wave4, out2, thres_bits, remaining);
    __syncthreads();
    const float thresh = __uint_as_float(thres_bits);
    const int lane = threadIdx.x & 63;
    if (!live) return;
    float* wrow = W + row * ldw + i1;
    float w[2], q[2] = {0.f, 0.f}, er[2] = {0.f, 0.f};
    bool mk[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = lane + 64 * t;
        w[t] = (j < count) ? wrow[j] : 0.f;
        if (j < count) {
            if (use_thresh) {
                const float d = HS(j, j);
                mk[t] = __uint_as_float(sg_metric_bits(w[t], d)) <= thresh;     // tmp <= thresh (:188)
            } else {
                mk[t] = mask_in ? mask_in[row * count + j] != 0 : false;    // (n:m: filled in during the sweep)
            }
        } else {
            mk[t] = false;
        }
    }
    for (int i = 0; i < count; ++i) {
        if (nm_n != 0 && i % nm_m == 0) {
            // n:m (:196-198): the n smallest W1[:, i:i+m]**2 / diag**2 of this row, on the sweep's
            // current values, join the mask; ranks by counting over the group's lanes
            const int len = count - i < nm_m ? count - i : nm_m;
            uint32_t myk[2];
            bool in[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int j = lane + 64 * t;
                in[t] = j >= i && j < i + len;
                myk[t] = 0xffffffffu;
                if (in[t]) {
                    const uint32_t b = sg_metric_bits(w[t], HS(j, j));
                    myk[t] = (b & 0x7fffffffu) > 0x7f800000u ? 0xffffffffu : b;      // NaN: the largest
                }
            }
            int rank[2] = {0, 0};
            for (int p = 0; p < len; ++p) {
                const int jj = i + p;
                const uint32_t kp = (jj < 64) ? __shfl(myk[0], jj & 63, 64) : __shfl(myk[1], jj & 63, 64);
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const int j = lane + 64 * t;
                    if (in[t] && jj != j && (kp < myk[t] || (kp == myk[t] && jj < j))) ++rank[t];
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (in[t] && rank[t] < nm_n) mk[t] = true;
        }
        const int src = i & 63;
        const float wi = (i < 64) ? __shfl(w[0], src, 64) : __shfl(w[1], src, 64);
        const int mi = (i < 64) ? __shfl((int)mk[0], src, 64) : __shfl((int)mk[1], src, 64);
        const float d = HS(i, i);
        const float qi = mi ? 0.f : wi;               // q[mask1[:, i]] = 0            (:200-201)
        const float err = (wi - qi) / d;              // err1 = (w - q) / d            (:206)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int j = lane + 64 * t;
            if (j >= i && j < count) {
                const float p = err * HS(i, j);   // err1 (x) Hinv1[i, i:]     (:207)
                w[t] = w[t] - p;
            }
            if (j == i) { q[t] = qi; er[t] = err; }
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int j = lane + 64 * t;
        if (j < count) {
            wrow[j] = q[t];                               // W[:, i1:i2] = Q1            (:212)
            Err[row * count + j] = er[t];
            if (mask_out) mask_out[row * count + j] = mk[t] ? 1 : 0;
        }
    }
#undef HS
}

__global__ __launch_bounds__(256) void sgpt_sweep_kernel(float* W, int64_t rows, int64_t ldw,
                                                         const float* __restrict__ Hinv, int64_t ldh,
                                                         int64_t i1, int count, uint32_t rank0,
                                                         const SgptSelState* st, int use_thresh,
                                                         const uint8_t* __restrict__ mask_in,
                                                         float* __restrict__ Err, uint8_t* mask_out,
                                                         int nm_n, int nm_m) {
    const int64_t row = (int64_t)blockIdx.x * SGT_WG_ROWS + (threadIdx.x >> 6);
    sg_sweep_rows(W, ldw, Hinv, ldh, i1, count, rank0, st, use_thresh, mask_in, Err, mask_out, nm_n,
                  nm_m, row, row < rows);
}

// The sweep over the stacked rows of a group: the workgroup's four rows lie in ONE member (offsets
// are multiples of four), whose rank and state it resolves; a padding row gets Err = 0, so the
// trailing update leaves its zeros alone.
__global__ __launch_bounds__(256) void sgpt_sweep_group_kernel(float* W, int64_t ldw,
                                                               const float* __restrict__ Hinv, int64_t ldh,
                                                               int64_t i1, int count, SgptGroup grp,
                                                               const SgptSelState* st, int use_thresh,
                                                               float* __restrict__ Err, int nm_n, int nm_m) {
    const int64_t row0 = (int64_t)blockIdx.x * SGT_WG_ROWS;
    int64_t off = grp.off[0], rows = grp.rows[0];
    uint32_t rank0 = grp.rank0[0];
    int g = 0;
#pragma unroll
    for (int k = 1; k < SGPT_MAX_GROUP; ++k)
        if (k < grp.n && row0 >= grp.off[k]) { g = k; off = grp.off[k]; rows = grp.rows[k]; rank0 = grp.rank0[k]; }
    const int64_t row = row0 + (threadIdx.x >> 6);
    const bool live = row - off < rows;
    sg_sweep_rows(W, ldw, Hinv, ldh, i1, count, rank0, st + g, use_thresh, (const uint8_t*)nullptr, Err,
                  (uint8_t*)nullptr, nm_n, nm_m, row, live);
    if (!live) {
        const int lane = threadIdx.x & 63;
        for (int j = lane; j < count; j += 64) Err[row * count + j] = 0.f;
    }
}

extern "C" size_t ecoflap_sparsegpt_workspace_bytes(void) { return sizeof(SgptSelState); }

// W: float[rows, ldw] (fp32 working copy of the weight), Hinv: float[cols, ldh] upper Cholesky
// factor of the inverse Hessian; block columns [i1, i1+count); k = int(rows*count*sparsity).
// mask_in (optional): uint8[rows*count] mask to use instead of the threshold (not used by the
// reference's unstructured path).  err_out: float[rows*count]; mask_out (optional).
// argument checks of the block step (no HIP call is made before they pass)
static int sgpt_block_check(int64_t rows, int64_t ldw, int64_t ldh, int64_t i1, int count, int64_t k,
                            bool thresholded) {
    if (rows <= 0 || count <= 0 || count > 128 || ldw < i1 + count || ldh < i1 + count || i1 < 0)
        return ECOFLAP_ESIZE;
    const int64_t n = rows * count;
    if (thresholded && (k < 0 || k >= n || n >= (int64_t)0xffffffffLL)) return ECOFLAP_ESIZE;
    return 0;
}

static int sgpt_nm_check(int count, int n, int m) {
    if (n <= 0 || m < n || m > 16 || (count % m != 0 && count % m < n)) return ECOFLAP_ESIZE;
    return 0;
}

// the launches of one thresholded (or given-mask) block step; arguments already checked
static int sgpt_block_launch(float* W, int64_t rows, int64_t ldw, const float* Hinv, int64_t ldh,
                             int64_t i1, int count, int64_t k, const uint8_t* mask_in, float* err_out,
                             uint8_t* mask_out, SgptSelState* st, hipStream_t s) {
    const int64_t n = rows * count;
    const uint32_t rank0 = (uint32_t)(k + 1);
    if (!mask_in) {
        hipError_t e = hipMemsetAsync(st, 0, sizeof(SgptSelState), s);
        if (e != hipSuccess) return (int)e;
        int64_t b = (n + 256 * 8 - 1) / (256 * 8);
        if (b < 1) b = 1;
        if (b > 512) b = 512;
        const dim3 grid((unsigned)b), blk(256);
        hipLaunchKernelGGL((sgpt_hist_kernel<0>), grid, blk, 0, s, W, rows, ldw, Hinv, ldh, i1, count, rank0, st);
        hipLaunchKernelGGL((sgpt_hist_kernel<1>), grid, blk, 0, s, W, rows, ldw, Hinv, ldh, i1, count, rank0, st);
        hipLaunchKernelGGL((sgpt_hist_kernel<2>), grid, blk, 0, s, W, rows, ldw, Hinv, ldh, i1, count, rank0, st);
        ECO_CHECK_LAUNCH();
    }
    const size_t lds = ((size_t)count * (count + 1) / 2) * sizeof(float);   // <= 33 KB
    hipLaunchKernelGGL(sgpt_sweep_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), lds, s, W, rows,
                       ldw, Hinv, ldh, i1, count, rank0, st, mask_in ? 0 : 1, mask_in, err_out,
                       mask_out, 0, 0);
    ECO_CHECK_LAUNCH();
    return 0;
}

static int sgpt_block_nm_launch(float* W, int64_t rows, int64_t ldw, const float* Hinv, int64_t ldh,
                                int64_t i1, int count, int n, int m, float* err_out, uint8_t* mask_out,
                                hipStream_t s) {
    const size_t lds = ((size_t)count * (count + 1) / 2) * sizeof(float);
    hipLaunchKernelGGL(sgpt_sweep_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), lds, s, W, rows,
                       ldw, Hinv, ldh, i1, count, 0u, (const SgptSelState*)nullptr, 0,
                       (const uint8_t*)nullptr, err_out, mask_out, n, m);
    ECO_CHECK_LAUNCH();
    return 0;
}

extern "C" int ecoflap_sparsegpt_block(float* W, int64_t rows, int64_t ldw, const float* Hinv,
                                       int64_t ldh, int64_t i1, int count, int64_t k,
                                       const uint8_t* mask_in, float* err_out, uint8_t* mask_out,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    const int rc = sgpt_block_check(rows, ldw, ldh, i1, count, k, !mask_in);
    if (rc) return rc;
    if (!W || !Hinv || !err_out || !workspace) return ECOFLAP_ENULL;
    if (workspace_bytes < sizeof(SgptSelState)) return ECOFLAP_EWORKSPACE;
    return sgpt_block_launch(W, rows, ldw, Hinv, ldh, i1, count, k, mask_in, err_out, mask_out,
                             (SgptSelState*)workspace, (hipStream_t)stream);
}

// The same block step under n:m (sparsegpt_pruner.py:190, :196-198; dead in the reference's shipped
// configs): no threshold, the mask grows during the sweep.  0 < n <= m <= 16; a group cut short by
// the block's end must hold at least n columns (the reference's topk raises otherwise).
extern "C" int ecoflap_sparsegpt_block_nm(float* W, int64_t rows, int64_t ldw, const float* Hinv,
                                          int64_t ldh, int64_t i1, int count, int n, int m,
                                          float* err_out, uint8_t* mask_out, void* stream) {
    int rc = sgpt_block_check(rows, ldw, ldh, i1, count, 0, false);
    if (rc) return rc;
    if ((rc = sgpt_nm_check(count, n, m)) != 0) return rc;
    if (!W || !Hinv || !err_out) return ECOFLAP_ENULL;
    return sgpt_block_nm_launch(W, rows, ldw, Hinv, ldh, i1, count, n, m, err_out, mask_out,
                                (hipStream_t)stream);
}

// ---- trailing update: W[:, j0:cols] -= Err[rows, count] @ Hinv[i1:i1+count, j0:cols] -------------
// (sparsegpt_pruner.py:302 of the CoOp tree, :216 of the LAVIS one) on v_mfma_f32_32x32x2_f32, in
// the tiling of csrc/gemm_f32.hip: a 64 x 64 tile of W per 256-thread workgroup, one 32 x 32 MFMA
// tile per wave, k in chunks of 32 through LDS.  `count` is at most 128, so a tile is at most four
// chunks: they go through ONE pair of LDS images with two barriers each; the next chunk's global
// loads are issued into registers before this chunk multiplies, and the lane's 16 elements of W are
// fetched before the first chunk, so a workgroup waits for memory once, not once per chunk (the
// update of a CLIP matrix is latency bound: 0.6 GFLOP at most).
//
// Numerics: every output element is ONE fp32 accumulation chain from +0 over k in a FIXED order —
// ascending quads, inside quad q the MFMA steps take the pairs (4q, 4q + 2) then (4q + 1, 4q + 3),
// one rounding per accumulate — followed by one subtraction from W.  k slots past `count` hold
// 0 x 0.  No atomics, no split over k: the same call gives the same bits, whatever the grid.
//
// LDS: Err rows at a pitch of 34 floats (the 8-byte k-pair reads of a half-wave fall on 32
// distinct even banks, as GF_LDK); Hinv rows as they lie, 64 columns wide (a half-wave reads 32
// consecutive floats of one k row: conflict free).  Every global access is bounds checked: rows
// past `rows`, columns past `cols` and k past `count` read as zero and are never stored.
typedef float sg_f32x16 __attribute__((ext_vector_type(16)));
typedef float sg_f32x2 __attribute__((ext_vector_type(2)));

#define SGT_BT 64               // tile edge
#define SGT_BK 32               // k per chunk
#define SGT_LDA (SGT_BK + 2)

__global__ __launch_bounds__(256) void sgpt_trailing_kernel(float* __restrict__ W, int64_t rows,
                                                            int64_t cols, int64_t ldw,
                                                            const float* __restrict__ Err,
                                                            const float* __restrict__ Hinv, int64_t ldh,
                                                            int64_t i1, int count, int64_t j0,
                                                            int tiles_n) {
    __shared__ __attribute__((aligned(16))) float As[SGT_BT * SGT_LDA];      // Err  [row][k]
    __shared__ __attribute__((aligned(16))) float Bs[SGT_BK * SGT_BT];       // Hinv [k][col]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tn = blockIdx.x % tiles_n, tm = blockIdx.x / tiles_n;
    const int64_t m0 = (int64_t)tm * SGT_BT, n0 = j0 + (int64_t)tn * SGT_BT;
    const int wy = wave >> 1, wx = wave & 1;
    const int r32 = lane & 31, kh = lane >> 5;
    sg_f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    // the tile of W this lane will update is on its way before anything else (C/D map of the
    // 32 x 32 shapes: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5))
    const int64_t col = n0 + 32 * wx + r32;
    float wv[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + 32 * wy + (r & 3) + 8 * (r >> 2) + 4 * kh;
        wv[r] = (row < rows && col < cols) ? W[row * ldw + col] : 0.f;
    }
    const int ak = tid & 31, ar = tid >> 5;         // Err: k ak of rows ar + 8 i
    const int bc = tid & 63, bk = tid >> 6;         // Hinv: column bc of k rows bk + 4 i
    float pa[8], pb[8];
    auto load_chunk = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int64_t row = m0 + ar + 8 * i;
            const int k = k0 + ak;
            pa[i] = (row < rows && k < count) ? Err[row * count + k] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int k = k0 + bk + 4 * i;
            const int64_t c = n0 + bc;
            pb[i] = (k < count && c < cols) ? Hinv[(i1 + k) * ldh + c] : 0.f;
        }
    };
    load_chunk(0);
    for (int k0 = 0; k0 < count; k0 += SGT_BK) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            As[(ar + 8 * i) * SGT_LDA + ak] = pa[i];
            Bs[(bk + 4 * i) * SGT_BT + bc] = pb[i];
        }
        __syncthreads();
        if (k0 + SGT_BK < count) load_chunk(k0 + SGT_BK);      // on its way while this chunk multiplies
        const float* A = &As[(32 * wy + r32) * SGT_LDA + 2 * kh];
        const float* B = &Bs[(2 * kh) * SGT_BT + 32 * wx + r32];
#pragma unroll
        for (int q = 0; q < SGT_BK / 4; ++q) {
            const sg_f32x2 av = *(const sg_f32x2*)(A + 4 * q);
            const float b0 = B[(4 * q) * SGT_BT], b1 = B[(4 * q + 1) * SGT_BT];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], b1, acc, 0, 0, 0);
        }
        __syncthreads();
    }
    if (col >= cols) return;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int64_t row = m0 + 32 * wy + (r & 3) + 8 * (r >> 2) + 4 * kh;
        if (row < rows) W[row * ldw + col] = wv[r] - acc[r];
    }
}

static int sgpt_trailing_check(int64_t rows, int64_t cols, int64_t ldw, int64_t ldh, int64_t i1,
                               int count, int64_t j0) {
    if (rows <= 0 || count <= 0 || count > 128 || i1 < 0 || j0 < 0 || cols < j0 || ldw < cols ||
        ldh < cols)
        return ECOFLAP_ESIZE;
    const int64_t tiles = ((rows + SGT_BT - 1) / SGT_BT) * ((cols - j0 + SGT_BT - 1) / SGT_BT);
    if (tiles > 0x7fffffffLL) return ECOFLAP_ESIZE;
    return 0;
}

static int sgpt_trailing_launch(float* W, int64_t rows, int64_t cols, int64_t ldw, const float* Err,
                                const float* Hinv, int64_t ldh, int64_t i1, int count, int64_t j0,
                                hipStream_t s) {
    if (cols == j0) return 0;
    const int64_t tiles_n = (cols - j0 + SGT_BT - 1) / SGT_BT;
    const int64_t tiles = ((rows + SGT_BT - 1) / SGT_BT) * tiles_n;
    hipLaunchKernelGGL(sgpt_trailing_kernel, dim3((unsigned)tiles), dim3(256), 0, s, W, rows, cols, ldw,
                       Err, Hinv, ldh, i1, count, j0, (int)tiles_n);
    ECO_CHECK_LAUNCH();
    return 0;
}

// W: float[rows, ldw]; Err: float[rows, count] as the block step leaves it (pitch `count`); Hinv:
// float[*, ldh], its rows [i1, i1 + count) and columns [j0, cols) are read.
extern "C" int ecoflap_sparsegpt_trailing(float* W, int64_t rows, int64_t cols, int64_t ldw,
                                          const float* Err, const float* Hinv, int64_t ldh,
                                          int64_t i1, int count, int64_t j0, void* stream) {
    const int rc = sgpt_trailing_check(rows, cols, ldw, ldh, i1, count, j0);
    if (rc) return rc;
    if (!W || !Err || !Hinv) return ECOFLAP_ENULL;
    return sgpt_trailing_launch(W, rows, cols, ldw, Err, Hinv, ldh, i1, count, j0, (hipStream_t)stream);
}

// ---- the whole sweep of one Linear from one host call ------------------------------------------
// widen: W32 = float(w), dead columns zeroed (`W = W.float(); W[:, dead] = 0`); narrow: w =
// W32.to(dtype), round to nearest even as torch's cast (v_cvt_pk_f16_f32 / v_cvt_pk_bf16_f32).
// VEC: one 16-byte vector of the storage dtype per thread (cols a multiple of its width, so a
// vector never straddles a row and the dead mask is read at `e % cols`); otherwise one element.
template <int DT, bool VEC>
__global__ __launch_bounds__(256) void sgpt_widen_kernel(const void* __restrict__ w, float* __restrict__ W32,
                                                         int64_t n, int64_t cols,
                                                         const uint8_t* __restrict__ dead) {
    typedef Vec<DT> V;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (t * V::N >= n) return;
        float f[V::N];
        V::unpack(ld16(w, t), f);
        if (dead) {
            const int64_t c0 = (t * V::N) % cols;
#pragma unroll
            for (int i = 0; i < V::N; ++i)
                if (dead[c0 + i]) f[i] = 0.f;
        }
#pragma unroll
        for (int v = 0; v < V::N / 4; ++v) st16(W32, t * (V::N / 4) + v, Vec<ECOFLAP_F32>::pack(f + 4 * v));
    } else {
        if (t >= n) return;
        const float x = V::load1(w, t);
        W32[t] = (dead && dead[t % cols]) ? 0.f : x;
    }
}

template <int DT, bool VEC>
__global__ __launch_bounds__(256) void sgpt_narrow_kernel(const float* __restrict__ W32, void* __restrict__ w,
                                                          int64_t n) {
    typedef Vec<DT> V;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        if (t * V::N >= n) return;
        float f[V::N];
#pragma unroll
        for (int v = 0; v < V::N / 4; ++v) Vec<ECOFLAP_F32>::unpack(ld16(W32, t * (V::N / 4) + v), f + 4 * v);
        st16(w, t, V::pack(f));
    } else {
        if (t >= n) return;
        V::store1(w, t, W32[t]);
    }
}

template <int DT>
static void sgpt_convert_launch(bool widen, void* w, float* W32, int64_t rows, int64_t cols,
                                const uint8_t* dead, hipStream_t s) {
    const int64_t n = rows * cols;
    const bool vec = cols % Vec<DT>::N == 0 && aligned16(w) && aligned16(W32);
    const int64_t threads = vec ? n / Vec<DT>::N : n;
    const dim3 grid((unsigned)((threads + 255) / 256)), blk(256);
    if (widen) {
        if (vec) hipLaunchKernelGGL((sgpt_widen_kernel<DT, true>), grid, blk, 0, s, w, W32, n, cols, dead);
        else hipLaunchKernelGGL((sgpt_widen_kernel<DT, false>), grid, blk, 0, s, w, W32, n, cols, dead);
    } else {
        if (vec) hipLaunchKernelGGL((sgpt_narrow_kernel<DT, true>), grid, blk, 0, s, W32, w, n);
        else hipLaunchKernelGGL((sgpt_narrow_kernel<DT, false>), grid, blk, 0, s, W32, w, n);
    }
}

static int sgpt_convert(bool widen, int dtype, void* w, float* W32, int64_t rows, int64_t cols,
                        const uint8_t* dead, hipStream_t s) {
    if (dtype == ECOFLAP_F32) sgpt_convert_launch<ECOFLAP_F32>(widen, w, W32, rows, cols, dead, s);
    else if (dtype == ECOFLAP_F16) sgpt_convert_launch<ECOFLAP_F16>(widen, w, W32, rows, cols, dead, s);
    else sgpt_convert_launch<ECOFLAP_BF16>(widen, w, W32, rows, cols, dead, s);
    ECO_CHECK_LAUNCH();
    return 0;
}

static inline size_t sg_align256(size_t b) { return (b + 255) & ~(size_t)255; }

// workspace of `ecoflap_sparsegpt_matrix`: the fp32 working copy [rows, cols], Err [rows, 128] and
// the selection state, each on a 256-byte boundary (0 for sizes the entry refuses)
extern "C" size_t ecoflap_sparsegpt_matrix_workspace_bytes(int64_t rows, int64_t cols) {
    if (rows <= 0 || cols <= 0 || rows > ((int64_t)1 << 40) / cols) return 0;
    return sg_align256((size_t)rows * (size_t)cols * 4) + sg_align256((size_t)rows * 128 * 4) +
           sg_align256(sizeof(SgptSelState));
}

// SparseGPT.fasterprune after the factorisation, for one Linear w[rows, cols] (contiguous, storage
// dtype, read and written in place): W = w.float(); W[:, dead] = 0; per block of `blocksize` columns
// the block step at rank ranks_host[block] = int(rows * count * sparsity) (a HOST array, read before
// this call returns; unused under n:m) or the n:m step, then the trailing update where columns
// remain; w = W.to(dtype).  Everything is queued on `stream`; nothing waits for the device.
extern "C" int ecoflap_sparsegpt_matrix(void* w, int dtype, int64_t rows, int64_t cols,
                                        const float* Hinv, int64_t ldh, const uint8_t* dead,
                                        int blocksize, const int64_t* ranks_host, int prune_n,
                                        int prune_m, void* workspace, size_t workspace_bytes,
                                        void* stream) {
    if (!dtype_ok(dtype)) return ECOFLAP_EDTYPE;
    if (rows <= 0 || cols <= 0 || blocksize <= 0 || blocksize > 128 || ldh < cols ||
        rows > ((int64_t)1 << 40) / cols)
        return ECOFLAP_ESIZE;
    if (!w || !Hinv || !workspace || (prune_n == 0 && !ranks_host)) return ECOFLAP_ENULL;
    if (prune_n < 0 || (prune_n == 0 && prune_m != 0)) return ECOFLAP_ESIZE;
    for (int64_t i1 = 0, b = 0; i1 < cols; i1 += blocksize, ++b) {
        const int count = (int)(cols - i1 < blocksize ? cols - i1 : blocksize);
        int rc = sgpt_block_check(rows, cols, ldh, i1, count, prune_n ? 0 : ranks_host[b], prune_n == 0);
        if (rc == 0 && prune_n) rc = sgpt_nm_check(count, prune_n, prune_m);
        if (rc == 0 && i1 + count < cols) rc = sgpt_trailing_check(rows, cols, cols, ldh, i1, count, i1 + count);
        if (rc) return rc;
    }
    if (workspace_bytes < ecoflap_sparsegpt_matrix_workspace_bytes(rows, cols)) return ECOFLAP_EWORKSPACE;
    if (!aligned16(workspace)) return ECOFLAP_EALIGN;
    hipStream_t s = (hipStream_t)stream;
    float* W32 = (float*)workspace;
    float* Err = (float*)((char*)workspace + sg_align256((size_t)rows * (size_t)cols * 4));
    SgptSelState* st = (SgptSelState*)((char*)Err + sg_align256((size_t)rows * 128 * 4));
    int rc = sgpt_convert(true, dtype, w, W32, rows, cols, dead, s);
    if (rc) return rc;
    for (int64_t i1 = 0, b = 0; i1 < cols; i1 += blocksize, ++b) {
        const int count = (int)(cols - i1 < blocksize ? cols - i1 : blocksize);
        if (prune_n)
            rc = sgpt_block_nm_launch(W32, rows, cols, Hinv, ldh, i1, count, prune_n, prune_m, Err, nullptr, s);
        else
            rc = sgpt_block_launch(W32, rows, cols, Hinv, ldh, i1, count, ranks_host[b], nullptr, Err, nullptr, st, s);
        if (rc) return rc;
        if (i1 + count < cols) {
            rc = sgpt_trailing_launch(W32, rows, cols, cols, Err, Hinv, ldh, i1, count, i1 + count, s);
            if (rc) return rc;
        }
    }
    return sgpt_convert(false, dtype, w, W32, rows, cols, nullptr, s);
}

// ---- the whole sweep of up to 8 Linears that share Hinv, from one host call ----------------------
// (q / k / v, gate / up of a decoder block: the same input, so the same H and the same factor.)
// The members' fp32 working copies are stacked into one [R, cols] matrix, member g at row off[g], a
// multiple of SGT_WG_ROWS; Err is stacked the same way.  Rows are independent in every step, and the
// trailing kernel's bits do not depend on where a row lies in the grid, so a column block costs the
// launches of ONE matrix — a clear, three histogram passes with a member dimension in the grid (a
// state, a rank and a histogram per member), one sweep, one trailing update over all R rows —
// however many members there are, and every member ends with the bits of its own
// `ecoflap_sparsegpt_matrix` call.
static int64_t sg_group_pad(int64_t rows) { return (rows + SGT_WG_ROWS - 1) / SGT_WG_ROWS * SGT_WG_ROWS; }

// per-member size checks of the single entry; -> stacked (padded) row count in *total
static int sgpt_group_rows(const ecoflap_sgpt_group_item* items, int n_items, int64_t cols, int64_t* total) {
    if (!items) return ECOFLAP_ENULL;
    if (n_items <= 0 || n_items > SGPT_MAX_GROUP || cols <= 0) return ECOFLAP_ESIZE;
    int64_t R = 0;
    for (int g = 0; g < n_items; ++g) {
        if (items[g].rows <= 0 || items[g].rows > ((int64_t)1 << 40) / cols) return ECOFLAP_ESIZE;
        R += sg_group_pad(items[g].rows);
    }
    *total = R;
    return 0;
}

// workspace of `ecoflap_sparsegpt_matrix_group`: the stacked working copy [R, cols], Err [R, 128] and
// one selection state per member, each on a 256-byte boundary (0 for what the entry refuses)
extern "C" size_t ecoflap_sparsegpt_matrix_group_workspace_bytes(const ecoflap_sgpt_group_item* items,
                                                                 int n_items, int64_t cols) {
    int64_t R;
    if (sgpt_group_rows(items, n_items, cols, &R)) return 0;
    return sg_align256((size_t)R * (size_t)cols * 4) + sg_align256((size_t)R * 128 * 4) +
           sg_align256((size_t)n_items * sizeof(SgptSelState));
}

extern "C" int ecoflap_sparsegpt_matrix_group(const ecoflap_sgpt_group_item* items, int n_items, int dtype,
                                              int64_t cols, const float* Hinv, int64_t ldh,
                                              const uint8_t* dead, int blocksize, int prune_n, int prune_m,
                                              void* workspace, size_t workspace_bytes, void* stream,
                                              int64_t* launches_out) {
    if (!dtype_ok(dtype)) return ECOFLAP_EDTYPE;
    if (!items) return ECOFLAP_ENULL;
    if (n_items <= 0 || n_items > SGPT_MAX_GROUP) return ECOFLAP_ESIZE;
    if (cols <= 0 || blocksize <= 0 || blocksize > 128 || ldh < cols) return ECOFLAP_ESIZE;
    int64_t R;
    int rc = sgpt_group_rows(items, n_items, cols, &R);
    if (rc) return rc;
    if (!Hinv || !workspace) return ECOFLAP_ENULL;
    for (int g = 0; g < n_items; ++g)
        if (!items[g].w || (prune_n == 0 && !items[g].ranks_host)) return ECOFLAP_ENULL;
    if (prune_n < 0 || (prune_n == 0 && prune_m != 0)) return ECOFLAP_ESIZE;
    // every member against the single entry's checks (its own rows, its own ranks), then the grids
    // that span the stack
    for (int g = 0; g < n_items; ++g)
        for (int64_t i1 = 0, b = 0; i1 < cols; i1 += blocksize, ++b) {
            const int count = (int)(cols - i1 < blocksize ? cols - i1 : blocksize);
            rc = sgpt_block_check(items[g].rows, cols, ldh, i1, count, prune_n ? 0 : items[g].ranks_host[b],
                                  prune_n == 0);
            if (rc == 0 && prune_n) rc = sgpt_nm_check(count, prune_n, prune_m);
            if (rc == 0 && i1 + count < cols)
                rc = sgpt_trailing_check(items[g].rows, cols, cols, ldh, i1, count, i1 + count);
            if (rc) return rc;
        }
    if (R / SGT_WG_ROWS > 0x7fffffffLL) return ECOFLAP_ESIZE;
    if (cols > blocksize && (rc = sgpt_trailing_check(R, cols, cols, ldh, 0, blocksize, blocksize)) != 0) return rc;
    if (workspace_bytes < ecoflap_sparsegpt_matrix_group_workspace_bytes(items, n_items, cols))
        return ECOFLAP_EWORKSPACE;
    if (!aligned16(workspace)) return ECOFLAP_EALIGN;

    hipStream_t s = (hipStream_t)stream;
    float* W32 = (float*)workspace;
    float* Err = (float*)((char*)workspace + sg_align256((size_t)R * (size_t)cols * 4));
    SgptSelState* st = (SgptSelState*)((char*)Err + sg_align256((size_t)R * 128 * 4));
    int64_t launches[5] = {0, 0, 0, 0, 0};      // clears, histogram, sweep, trailing, widen + narrow
    SgptGroup grp;
    grp.n = n_items;
    int64_t hist_blocks = 1;
    for (int64_t g = 0, at = 0; g < SGPT_MAX_GROUP; ++g) {
        grp.off[g] = grp.rows[g] = 0;
        grp.rank0[g] = 0;
        if (g >= n_items) continue;
        grp.off[g] = at;
        grp.rows[g] = items[g].rows;
        at += sg_group_pad(items[g].rows);
        // the single entry's histogram grid at a full block, per member: the widest is launched for
        // all (the counts are integer atomics: they do not depend on the grid)
        int64_t b = (items[g].rows * (cols < blocksize ? cols : (int64_t)blocksize) + 256 * 8 - 1) / (256 * 8);
        if (b > 512) b = 512;
        if (b > hist_blocks) hist_blocks = b;
    }
    for (int g = 0; g < n_items; ++g) {
        float* Wg = W32 + grp.off[g] * cols;
        rc = sgpt_convert(true, dtype, items[g].w, Wg, items[g].rows, cols, dead, s);
        if (rc) return rc;
        ++launches[4];
        const int64_t pad = sg_group_pad(items[g].rows) - items[g].rows;
        if (pad) {      // padding rows: zero, and they stay zero (the sweep gives them Err = 0)
            hipError_t e = hipMemsetAsync(Wg + items[g].rows * cols, 0, (size_t)pad * (size_t)cols * 4, s);
            if (e != hipSuccess) return (int)e;
        }
    }
    const dim3 blk(256);
    for (int64_t i1 = 0, b = 0; i1 < cols; i1 += blocksize, ++b) {
        const int count = (int)(cols - i1 < blocksize ? cols - i1 : blocksize);
        if (prune_n == 0) {
            for (int g = 0; g < n_items; ++g) grp.rank0[g] = (uint32_t)(items[g].ranks_host[b] + 1);
            hipError_t e = hipMemsetAsync(st, 0, (size_t)n_items * sizeof(SgptSelState), s);
            if (e != hipSuccess) return (int)e;
            ++launches[0];
            const dim3 grid((unsigned)hist_blocks, (unsigned)n_items);
            hipLaunchKernelGGL((sgpt_hist_group_kernel<0>), grid, blk, 0, s, W32, cols, Hinv, ldh, i1, count, grp, st);
            hipLaunchKernelGGL((sgpt_hist_group_kernel<1>), grid, blk, 0, s, W32, cols, Hinv, ldh, i1, count, grp, st);
            hipLaunchKernelGGL((sgpt_hist_group_kernel<2>), grid, blk, 0, s, W32, cols, Hinv, ldh, i1, count, grp, st);
            ECO_CHECK_LAUNCH();
            launches[1] += 3;
        }
        const size_t lds = ((size_t)count * (count + 1) / 2) * sizeof(float);
        hipLaunchKernelGGL(sgpt_sweep_group_kernel, dim3((unsigned)(R / SGT_WG_ROWS)), blk, lds, s, W32, cols,
                           Hinv, ldh, i1, count, grp, st, prune_n == 0 ? 1 : 0, Err, prune_n, prune_m);
        ECO_CHECK_LAUNCH();
        ++launches[2];
        if (i1 + count < cols) {
            rc = sgpt_trailing_launch(W32, R, cols, cols, Err, Hinv, ldh, i1, count, i1 + count, s);
            if (rc) return rc;
            ++launches[3];
        }
    }
    for (int g = 0; g < n_items; ++g) {
        rc = sgpt_convert(false, dtype, items[g].w, W32 + grp.off[g] * cols, items[g].rows, cols, nullptr, s);
        if (rc) return rc;
        ++launches[4];
    }
    if (launches_out)
        for (int i = 0; i < 5; ++i) launches_out[i] = launches[i];
    return 0;
}
