// colsq.hip — K6: the Wanda calibration statistic (column sum of squares -> running mean), for gfx950.
//
// Replaces
//   K6  WrappedGPT.add_batch           LAVIS/lavis/compression/pruners/wanda_pruner.py:71-84
//
// HBM-bound: 16-byte coalesced loads, no GEMM reshaping.  Algorithmic bytes: tokens*cols*s_x.
// (wanda_k7.h: only the phase clock, whose slot 6 this kernel stamps under -DECO_K7_CLOCK.)
#include "wanda_k7.h"

// =====================================================================================
// K6  column sum of squares -> running mean
// =====================================================================================
// ONE launch per hooked input.  Workgroup (column block, row chunk) writes
// partial[chunk][col] = sum over the chunk's rows of x^2 (fp32); the LAST chunk of a column block
// to finish (ticket counter in the workspace) sums that block's partials in fixed chunk order —
// so the result does not depend on which workgroup came last — and applies the reference's
// update (W:80-84).  Tickets reset themselves: the workspace is zeroed once by its owner.
// FROM_DEV: the sample count lives in device memory (graph-replayable: no launch argument
// changes from call to call); the last workgroup of the whole grid then adds `batch` to it.
struct ColsqArgs {
    const void* x;
    int64_t tokens, cols;
    int rows_per_chunk, nchunks;
    float* partial;          // [nchunks][cols]
    unsigned* tickets;       // [colblocks + 1], zero between launches
    float* scaler_row;
    float decay, n_new;      // host form
    int64_t* n_dev;          // device form (nullptr: host form)
    int64_t batch;
    int colblocks;           // column blocks of this input (= gridDim.x of the one-input launch)
    int first_wg;            // multi-input launch: first workgroup of this input
    int vector;              // 16-byte column vectors usable
    int raw;                 // 1: scaler_row[c] = ||x_c||^2 of THIS input only (no running mean)
    int small;               // 1: few rows — one workgroup per 64 columns reduces ALL rows (colsq_small_body)
};

// the work of workgroup (bx = column block, by = row chunk) of one hooked input
template <int DT, bool VECTOR>
__device__ __forceinline__ void colsq_body(const ColsqArgs& a, const int bx, const int by,
                                           float (*lds)[64 * 8], unsigned* last) {
    constexpr int N = VECTOR ? Vec<DT>::N : 1;
    const void* __restrict__ x = a.x;
    const int64_t tokens = a.tokens, cols = a.cols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cvec = (int64_t)bx * 64 + lane;  // column vector handled by this lane
    const int64_t ncvec = cols / N;
    const int64_t r0 = (int64_t)by * a.rows_per_chunk;
    int64_t r1 = r0 + a.rows_per_chunk;
    if (r1 > tokens) r1 = tokens;
    float acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.f;
    K7_ENTER(5); K7_STAMP(5, 0);
    if (cvec < ncvec) {
        // four independent 16-byte loads in flight per lane before the first use
        int64_t r = r0 + wave;
        for (; r + 12 < r1; r += 16) {
            float f0[N], f1[N], f2[N], f3[N];
            if (VECTOR) {
                const u32x4 va = ld16(x, r * ncvec + cvec), vb = ld16(x, (r + 4) * ncvec + cvec);
                const u32x4 vc = ld16(x, (r + 8) * ncvec + cvec), vd = ld16(x, (r + 12) * ncvec + cvec);
                Vec<DT>::unpack(va, f0); Vec<DT>::unpack(vb, f1);
                Vec<DT>::unpack(vc, f2); Vec<DT>::unpack(vd, f3);
            } else {
                f0[0] = Vec<DT>::load1(x, r * cols + cvec);
                f1[0] = Vec<DT>::load1(x, (r + 4) * cols + cvec);
                f2[0] = Vec<DT>::load1(x, (r + 8) * cols + cvec);
                f3[0] = Vec<DT>::load1(x, (r + 12) * cols + cvec);
            }
#pragma unroll
            for (int i = 0; i < N; ++i) {   // same order as the one-row-at-a-time loop below
                acc[i] += f0[i] * f0[i];
                acc[i] += f1[i] * f1[i];
                acc[i] += f2[i] * f2[i];
                acc[i] += f3[i] * f3[i];
            }
        }
        for (; r < r1; r += 4) {
            float f[N];
            if (VECTOR) {
                Vec<DT>::unpack(ld16(x, r * ncvec + cvec), f);
            } else {
                f[0] = Vec<DT>::load1(x, r * cols + cvec);
            }
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] += f[i] * f[i];
        }
    }
    K7_STAMP(5, 1);
#pragma unroll
    for (int i = 0; i < N; ++i) lds[wave][lane * N + i] = acc[i];
    __syncthreads();
    if (wave == 0 && cvec < ncvec) {
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float s = (lds[0][lane * N + i] + lds[1][lane * N + i]) +
                            (lds[2][lane * N + i] + lds[3][lane * N + i]);
            // device-scope (sc1) store: written through this XCD's L2, so the workgroup that
            // finishes the column block — possibly on another XCD — reads it without anyone
            // having to write back or invalidate a whole L2 (what a release fence would do)
            __hip_atomic_store(&a.partial[(int64_t)by * cols + cvec * N + i], s,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // ---- last chunk of this column block finishes the update ------------------------------
    __builtin_amdgcn_s_waitcnt(0);         // this wave's partial stores have been performed
    __syncthreads();
    K7_STAMP(5, 2);
    if (threadIdx.x == 0)
        *last = (__hip_atomic_fetch_add(&a.tickets[bx], 1u, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_AGENT) == (unsigned)a.nchunks - 1u);
    __syncthreads();
    K7_STAMP(5, 3);
    K7_EXIT(5);
    if (!*last) return;
#ifdef ECO_K7_CLOCK
    if (threadIdx.x == 0) { atomicMin(&eco_k7_clk[6][14], wall_clock64()); }
#endif
    float decay = a.decay, n_new = a.n_new;
    if (a.n_dev) {                         // formed as the host form does (double, then float)
        const int64_t n0 = a.n_dev[0];
        decay = (float)((double)n0 / (double)(n0 + a.batch));
        n_new = (float)(n0 + a.batch);
    }
    const int64_t c0 = (int64_t)bx * 64 * N;
    for (int64_t c = c0 + threadIdx.x; c < c0 + 64 * N && c < cols; c += 256) {
        float s = 0.f;
        int k = 0;
        for (; k + 8 <= a.nchunks; k += 8) {     // eight loads in flight, summed in chunk order
            float t[8];
#pragma unroll
            for (int j = 0; j < 8; ++j)          // device-scope loads: never a stale L2 line
                t[j] = __hip_atomic_load(&a.partial[(int64_t)(k + j) * cols + c], __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += t[j];
        }
        for (; k < a.nchunks; ++k)
            s += __hip_atomic_load(&a.partial[(int64_t)k * cols + c], __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
        const float nrm = __builtin_sqrtf(s);  // torch.norm(...): sqrt of the sum of squares
        const float sq = nrm * nrm;            // ... ** 2
        if (a.raw) {
            a.scaler_row[c] = sq;              // this input's own statistic (data-parallel replay)
        } else {
            const float r = a.scaler_row[c] * decay;  // scaler_row *= n / (n + b)
            a.scaler_row[c] = r + sq / n_new;         // += ... / nsamples
        }
    }
    // every wave of this workgroup has read n_dev (and used it) before thread 0 takes the
    // grid-level ticket: the workgroup that takes the LAST one bumps the count
    __syncthreads();
    K7_EXIT(6);
    if (threadIdx.x == 0) {
        __hip_atomic_store(&a.tickets[bx], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (a.n_dev) {                     // every column block has read n_dev before its ticket
            if (__hip_atomic_fetch_add(&a.tickets[a.colblocks], 1u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT) == (unsigned)a.colblocks - 1u) {
                __hip_atomic_store(&a.tickets[a.colblocks], 0u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
                a.n_dev[0] += a.batch;
            }
        }
    }
}

// Few rows (tokens <= COLSQ_SMALL_TOKENS: one calibration batch of a FlanT5 block is 128-384
// rows of 2048-5120 columns, 0.5-4 MB): the two-stage scheme above is all latency there — partial
// sums to memory, a ticket, the last arriver's reload (12.5 us for a block's 13 MB).  Here a
// workgroup owns 64 columns (8 lanes x 8) and reduces ALL rows itself: lane (row slot, column
// vector) takes rows wave * 8 + slot + 32 p — at most 16 16-byte loads, four in flight at a time —, the wave's 8
// row slots are added by a fixed butterfly, the 4 waves through LDS in a fixed order, and the same
// workgroup applies the update: no partials, no ticket to wait for.  One path per (tokens, cols):
// a given input is always summed in the same order.
#define COLSQ_SMALL_TOKENS 512
template <int DT>
__device__ __forceinline__ void colsq_small_body(const ColsqArgs& a, const int bx, float (*lds)[64 * 8]) {
    constexpr int N = Vec<DT>::N;
    const void* __restrict__ x = a.x;
    const int64_t tokens = a.tokens, cols = a.cols;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int cl = lane & 7, slot = lane >> 3;
    const int64_t ncvec = cols / N;
    const int64_t cvec = (int64_t)bx * 8 + cl;
    float acc[N];
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = 0.f;
    if (cvec < ncvec) {
        int64_t r = wave * 8 + slot;
        for (; r + 96 < tokens; r += 128) {          // four loads in flight (all sixteen at once: slower, measured)
            float f0[N], f1[N], f2[N], f3[N];
            const u32x4 va = ld16(x, r * ncvec + cvec), vb = ld16(x, (r + 32) * ncvec + cvec);
            const u32x4 vc = ld16(x, (r + 64) * ncvec + cvec), vd = ld16(x, (r + 96) * ncvec + cvec);
            Vec<DT>::unpack(va, f0); Vec<DT>::unpack(vb, f1);
            Vec<DT>::unpack(vc, f2); Vec<DT>::unpack(vd, f3);
#pragma unroll
            for (int i = 0; i < N; ++i) {            // same order as the one-row-at-a-time loop below
                acc[i] += f0[i] * f0[i];
                acc[i] += f1[i] * f1[i];
                acc[i] += f2[i] * f2[i];
                acc[i] += f3[i] * f3[i];
            }
        }
        for (; r < tokens; r += 32) {
            float f[N];
            Vec<DT>::unpack(ld16(x, r * ncvec + cvec), f);
#pragma unroll
            for (int i = 0; i < N; ++i) acc[i] += f[i] * f[i];
        }
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float v = acc[i];
        v += __shfl_xor(v, 8, 64);
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (slot == 0) lds[wave][cl * N + i] = v;
    }
    __syncthreads();
    float decay = a.decay, n_new = a.n_new;
    if (a.n_dev) {                         // formed as the host form does (double, then float)
        const int64_t n0 = a.n_dev[0];
        decay = (float)((double)n0 / (double)(n0 + a.batch));
        n_new = (float)(n0 + a.batch);
    }
    const int64_t c = (int64_t)bx * 8 * N + threadIdx.x;
    if (threadIdx.x < 8 * N && c < cols) {
        const float s = (lds[0][threadIdx.x] + lds[1][threadIdx.x]) + (lds[2][threadIdx.x] + lds[3][threadIdx.x]);
        const float nrm = __builtin_sqrtf(s);  // torch.norm(...): sqrt of the sum of squares
        const float sq = nrm * nrm;            // ... ** 2
        if (a.raw) {
            a.scaler_row[c] = sq;
        } else {
            const float r = a.scaler_row[c] * decay;  // scaler_row *= n / (n + b)
            a.scaler_row[c] = r + sq / n_new;         // += ... / nsamples
        }
    }
    if (a.n_dev) {
        // every wave of this workgroup has read n_dev before thread 0 takes the grid-level
        // ticket: the workgroup that takes the LAST one bumps the count
        __syncthreads();
        if (threadIdx.x == 0 &&
            __hip_atomic_fetch_add(&a.tickets[a.colblocks], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                (unsigned)a.colblocks - 1u) {
            __hip_atomic_store(&a.tickets[a.colblocks], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            a.n_dev[0] += a.batch;
        }
    }
}

template <int DT, bool VECTOR>
__global__ __launch_bounds__(256) void colsq_kernel(const ColsqArgs a) {
    __shared__ float lds[4][64 * 8];
    __shared__ unsigned last;
    if (VECTOR && a.small) colsq_small_body<DT>(a, blockIdx.x, lds);
    else colsq_body<DT, VECTOR>(a, blockIdx.x, blockIdx.y, lds, &last);
}

// ALL hooked inputs of a transformer block for one calibration sample in ONE launch (the
// reference calls add_batch from one forward hook per Linear, W:240-252 / :521-533): the
// per-input launches are pure latency (11-17 us for 1.6-25 MB).  Workgroups of the inputs are
// laid out one input after another; same arithmetic per input as the one-input kernel.
struct ColsqMultiArgs {
    ColsqArgs it[ECOFLAP_COLSQ_MAX_ITEMS];
    int first[ECOFLAP_COLSQ_MAX_ITEMS];      // first workgroup of input i (INT_MAX past the last): one
    int n;                                   // vector load, no walk over the 100-byte records
};

template <int DT>
__global__ __launch_bounds__(256) void colsq_multi_kernel(const ColsqMultiArgs m) {
    __shared__ float lds[4][64 * 8];
    __shared__ unsigned last;
    int i = 0;
    const int wg = blockIdx.x;
#pragma unroll
    for (int j = 1; j < ECOFLAP_COLSQ_MAX_ITEMS; ++j) i += wg >= m.first[j] ? 1 : 0;     // (ascending)
    const ColsqArgs& a = m.it[i];
    const int local = wg - a.first_wg;
    const int bx = local % a.colblocks, by = local / a.colblocks;
    if (a.small) colsq_small_body<DT>(a, bx, lds);
    else if (a.vector) colsq_body<DT, true>(a, bx, by, lds, &last);
    else colsq_body<DT, false>(a, bx, by, lds, &last);
}

// The running mean replayed from per-batch statistics (raw rows of the kernels above), in
// global batch order: what the one-process loop computes, bit for bit, when the batches were
// reduced on different ranks.  sq: [J][ld] fp32; batches: int64[J] (device).
__global__ __launch_bounds__(256) void colsq_replay_kernel(float* __restrict__ scaler_row,
                                                           const float* __restrict__ sq,
                                                           const int64_t* __restrict__ batches,
                                                           int J, int64_t cols, int64_t ld,
                                                           int64_t n_before) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float row = scaler_row[c];
    int64_t n0 = n_before;
    for (int j = 0; j < J; ++j) {
        const int64_t b = batches[j];
        const float decay = (float)((double)n0 / (double)(n0 + b));
        const float n_new = (float)(n0 + b);
        const float r = row * decay;
        row = r + sq[(int64_t)j * ld + c] / n_new;
        n0 += b;
    }
    scaler_row[c] = row;
}

static inline int colsq_rows_per_chunk(int64_t tokens, int64_t cols) {
    // ~512 workgroups over the 256 CUs, at least 64 rows (16 per wave) per workgroup so every
    // lane keeps several loads in flight and the second stage sums few partials
    const int64_t colblocks = (cols / 4 + 63) / 64 + 1;
    int64_t want_chunks = 512 / colblocks;
    if (want_chunks < 1) want_chunks = 1;
    int64_t rpc = (tokens + want_chunks - 1) / want_chunks;
    if (rpc < 64) rpc = 64;
    return (int)rpc;
}
static inline int colsq_nchunks(int64_t tokens, int64_t cols) {
    const int rpc = colsq_rows_per_chunk(tokens, cols);
    return (int)((tokens + rpc - 1) / rpc);
}
// ticket area at the head of the workspace: FIXED size, so that calls with different shapes that
// share one workspace never see another call's partial sums where they expect zeroed tickets
#define COLSQ_MAX_COLBLOCKS 4095
static inline size_t colsq_ticket_bytes(int64_t) { return (COLSQ_MAX_COLBLOCKS + 1) * sizeof(unsigned); }

extern "C" size_t ecoflap_colsqnorm_workspace_bytes(int64_t tokens, int64_t cols) {
    if (tokens <= 0 || cols <= 0) return 0;
    return colsq_ticket_bytes(cols) + (size_t)colsq_nchunks(tokens, cols) * (size_t)cols * sizeof(float);
}

static int colsq_accum_impl(float* scaler_row, const void* x, int64_t tokens, int64_t cols,
                            int dtype, int64_t nsamples_before, int64_t* nsamples_dev,
                            int64_t batch, void* workspace, size_t workspace_bytes, void* stream);

extern "C" int ecoflap_colsqnorm_accum(float* scaler_row, const void* x, int64_t tokens,
                                       int64_t cols, int dtype, int64_t nsamples_before,
                                       int64_t batch, void* workspace, size_t workspace_bytes,
                                       void* stream) {
    return colsq_accum_impl(scaler_row, x, tokens, cols, dtype, nsamples_before, nullptr, batch,
                            workspace, workspace_bytes, stream);
}

extern "C" int ecoflap_colsqnorm_accum_dev(float* scaler_row, const void* x, int64_t tokens,
                                           int64_t cols, int dtype, int64_t* nsamples_dev,
                                           int64_t batch, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    if (!nsamples_dev) return ECOFLAP_ENULL;
    return colsq_accum_impl(scaler_row, x, tokens, cols, dtype, 0, nsamples_dev, batch, workspace,
                            workspace_bytes, stream);
}

static int colsq_fill(ColsqArgs& a, float* scaler_row, const void* x, int64_t tokens,
                      int64_t cols, int dtype, int64_t nsamples_before, int64_t* nsamples_dev,
                      int64_t batch, int raw, void* workspace) {
    if (tokens <= 0 || cols <= 0 || nsamples_before < 0 || batch <= 0) return ECOFLAP_ESIZE;
    if (!scaler_row || !x || !workspace) return ECOFLAP_ENULL;
    const int nvec = dtype == ECOFLAP_F32 ? 4 : 8;
    const bool vector = (cols % nvec == 0) && aligned16(x);
    const int64_t ncv = vector ? cols / nvec : cols;
    if ((ncv + 63) / 64 > COLSQ_MAX_COLBLOCKS) return ECOFLAP_ESIZE;
    a.x = x; a.tokens = tokens; a.cols = cols;
    a.rows_per_chunk = colsq_rows_per_chunk(tokens, cols);
    a.nchunks = colsq_nchunks(tokens, cols);
    a.tickets = (unsigned*)workspace;
    a.partial = (float*)((char*)workspace + colsq_ticket_bytes(cols));
    a.scaler_row = scaler_row;
    a.decay = (float)((double)nsamples_before / (double)(nsamples_before + batch));
    a.n_new = (float)(nsamples_before + batch);
    a.n_dev = nsamples_dev;
    a.batch = batch;
    a.colblocks = (int)((ncv + 63) / 64);
    a.first_wg = 0;
    a.vector = vector ? 1 : 0;
    a.raw = raw;
    a.small = 0;
    if (vector && tokens <= COLSQ_SMALL_TOKENS && (ncv + 7) / 8 <= COLSQ_MAX_COLBLOCKS) {
        a.small = 1;                       // one workgroup per 64 (fp32: 32) columns, all rows: colsq_small_body
        a.colblocks = (int)((ncv + 7) / 8);
        a.nchunks = 1;
        a.rows_per_chunk = (int)tokens;
    }
    return 0;
}

static int colsq_accum_impl(float* scaler_row, const void* x, int64_t tokens, int64_t cols,
                            int dtype, int64_t nsamples_before, int64_t* nsamples_dev,
                            int64_t batch, void* workspace, size_t workspace_bytes, void* stream) {
    if (!dtype_ok(dtype)) return ECOFLAP_EDTYPE;
    if (tokens <= 0 || cols <= 0) return ECOFLAP_ESIZE;
    if (workspace_bytes < ecoflap_colsqnorm_workspace_bytes(tokens, cols)) return ECOFLAP_EWORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    ColsqArgs a;
    const int rc = colsq_fill(a, scaler_row, x, tokens, cols, dtype, nsamples_before, nsamples_dev,
                              batch, 0, workspace);
    if (rc) return rc;
    const dim3 grid((unsigned)a.colblocks, (unsigned)a.nchunks);
#define COLSQ(DT_)                                                                                \
    do {                                                                                          \
        if (a.vector) hipLaunchKernelGGL((colsq_kernel<DT_, true>), grid, dim3(256), 0, s, a);    \
        else hipLaunchKernelGGL((colsq_kernel<DT_, false>), grid, dim3(256), 0, s, a);            \
    } while (0)
    if (dtype == ECOFLAP_F32) COLSQ(ECOFLAP_F32);
    else if (dtype == ECOFLAP_F16) COLSQ(ECOFLAP_F16);
    else COLSQ(ECOFLAP_BF16);
#undef COLSQ
    ECO_CHECK_LAUNCH();
    return 0;
}

// Workspace of the multi-input call: ECOFLAP_COLSQ_MAX_ITEMS ticket areas of FIXED size at the
// head (input i always finds its tickets at the same place, whatever the shapes of the call, so
// a zeroed-once workspace can serve calls of different shapes one after another), then the
// inputs' partial sums.
static inline size_t colsq_item_partial_bytes(int64_t tokens, int64_t cols) {
    if (tokens <= 0 || cols <= 0) return 0;
    return ((size_t)colsq_nchunks(tokens, cols) * (size_t)cols * sizeof(float) + 255) & ~(size_t)255;
}

extern "C" size_t ecoflap_colsqnorm_multi_workspace_bytes(const ecoflap_colsq_item* items, int n) {
    if (!items || n <= 0) return 0;
    size_t total = (size_t)ECOFLAP_COLSQ_MAX_ITEMS * colsq_ticket_bytes(0);
    for (int i = 0; i < n; ++i) total += colsq_item_partial_bytes(items[i].tokens, items[i].cols);
    return total;
}

extern "C" int ecoflap_colsqnorm_accum_multi(const ecoflap_colsq_item* items, int n, int dtype,
                                             void* workspace, size_t workspace_bytes,
                                             void* stream) {
    if (!dtype_ok(dtype)) return ECOFLAP_EDTYPE;
    if (!items || !workspace) return ECOFLAP_ENULL;
    if (n <= 0 || n > ECOFLAP_COLSQ_MAX_ITEMS) return ECOFLAP_ESIZE;
    if (workspace_bytes < ecoflap_colsqnorm_multi_workspace_bytes(items, n)) return ECOFLAP_EWORKSPACE;
    ColsqMultiArgs m;
    m.n = n;
    size_t off = (size_t)ECOFLAP_COLSQ_MAX_ITEMS * colsq_ticket_bytes(0);
    int wg = 0;
    for (int i = 0; i < n; ++i) {
        const ecoflap_colsq_item& it = items[i];
        const int rc = colsq_fill(m.it[i], it.scaler_row, it.x, it.tokens, it.cols, dtype,
                                  it.nsamples_dev ? 0 : it.nsamples_before, it.nsamples_dev,
                                  it.batch, it.raw ? 1 : 0, workspace);
        if (rc) return rc;
        m.it[i].tickets = (unsigned*)((char*)workspace + (size_t)i * colsq_ticket_bytes(0));
        m.it[i].partial = (float*)((char*)workspace + off);
        m.it[i].first_wg = wg;
        m.first[i] = wg;
        wg += m.it[i].colblocks * m.it[i].nchunks;
        off += colsq_item_partial_bytes(it.tokens, it.cols);
    }
    for (int i = n; i < ECOFLAP_COLSQ_MAX_ITEMS; ++i) m.first[i] = 0x7fffffff;
    hipStream_t s = (hipStream_t)stream;
    if (dtype == ECOFLAP_F32)
        hipLaunchKernelGGL((colsq_multi_kernel<ECOFLAP_F32>), dim3((unsigned)wg), dim3(256), 0, s, m);
    else if (dtype == ECOFLAP_F16)
        hipLaunchKernelGGL((colsq_multi_kernel<ECOFLAP_F16>), dim3((unsigned)wg), dim3(256), 0, s, m);
    else
        hipLaunchKernelGGL((colsq_multi_kernel<ECOFLAP_BF16>), dim3((unsigned)wg), dim3(256), 0, s, m);
    ECO_CHECK_LAUNCH();
    return 0;
}

extern "C" int ecoflap_colsq_replay(float* scaler_row, const float* sq, const int64_t* batches_dev,
                                    int n_batches, int64_t cols, int64_t ld,
                                    int64_t nsamples_before, void* stream) {
    if (!scaler_row || !sq || !batches_dev) return ECOFLAP_ENULL;
    if (n_batches <= 0 || cols <= 0 || ld < cols || nsamples_before < 0) return ECOFLAP_ESIZE;
    hipLaunchKernelGGL(colsq_replay_kernel, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, scaler_row, sq, batches_dev, n_batches, cols, ld,
                       nsamples_before);
    ECO_CHECK_LAUNCH();
    return 0;
}
