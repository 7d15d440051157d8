// wanda_matrix.hip — K7 matrix mode (ViT, wanda_pruner.py:541, :555-558): the three-histogram
// selection, the sampled bracket with its on-device fallback, and the host half that groups the
// matrix-mode items of a block and launches them.  Selection by radix select on the fp32 metric's
// bit pattern (metrics are >= +0 so the unsigned order of the bits IS the float order; NaN sorts
// last like torch.sort).
#include "wanda_matrix_state.h"

// =====================================================================================
// K7 matrix mode: global (k+1)-th smallest over rows*cols by 3 histogram passes
// (11 + 11 + 10 bits), then zero metric <= threshold.
// =====================================================================================
// (MatrixSelState and the WM_* sizes: wanda_matrix_state.h)

// Workgroup barrier that orders LDS traffic ONLY.  __syncthreads() is a release / acquire fence on
// every address space, which the compiler implements as s_waitcnt vmcnt(0): in a kernel that has
// its share of W in flight in registers, EVERY barrier of the prologue then waits for the whole
// stream (measured: 12 us to the first barrier instead of 2).  Here: lgkmcnt(0) (LDS and scalar
// loads; vmcnt 63 / expcnt 7 = do not wait) and s_barrier; the "memory" clobber keeps the compiler
// from moving accesses across it.  Threads that exchange data through GLOBAL memory inside one
// kernel must not use this.
static __device__ __forceinline__ void lds_barrier() {
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}
template <bool LDS_ONLY>
static __device__ __forceinline__ void wm_barrier() {
    if (LDS_ONLY) lds_barrier();
    else __syncthreads();
}

// sqrt(scaler_row) of the workgroup's matrix into LDS (every vector needs 2 x 16 bytes of it:
// from global memory those were two dependent cache round trips per vector, most of a pass)
static __device__ __forceinline__ const float* stage_sq(const float* __restrict__ sq, int64_t cols,
                                                        float* lds) {
    if (cols > WM_SQ_LDS) return sq;
    for (int64_t c = threadIdx.x; c < cols; c += WM_THREADS) lds[c] = sq[c];
    __syncthreads();
    return lds;
}
// the same, straight from the statistic (sampled-bracket path: no sqrt launch in front of it)
static __device__ __forceinline__ const float* stage_sqrt(const float* __restrict__ sr, int64_t cols,
                                                          float* lds) {
    for (int64_t c = threadIdx.x; c < cols; c += WM_THREADS) lds[c] = __builtin_sqrtf(sr[c]);
    __syncthreads();
    return lds;
}
// the same in two halves, so that the statistic's loads can be issued BEFORE a long run of other
// loads (loads return in order: issued after them, these would wait for all of them) and consumed
// after it: the first WM_SR_PRE * WM_THREADS columns travel through registers
#define WM_SR_PRE 8
struct SqrtPre { float v[WM_SR_PRE]; };
static __device__ __forceinline__ SqrtPre stage_sqrt_issue(const float* __restrict__ sr, int64_t cols) {
    SqrtPre p;
#pragma unroll
    for (int q = 0; q < WM_SR_PRE; ++q) {
        // (index clamped, not predicated: a predicated load becomes a branch, and the compiler
        // then sinks the wait and the sqrt into it — eight serial round trips)
        const int64_t c = threadIdx.x + (int64_t)q * WM_THREADS;
        p.v[q] = sr[c < cols ? c : cols - 1];
    }
    return p;
}
static __device__ __forceinline__ const float* stage_sqrt_finish(const SqrtPre& p, const float* __restrict__ sr,
                                                                 int64_t cols, float* lds) {
#pragma unroll
    for (int q = 0; q < WM_SR_PRE; ++q) {
        const int64_t c = threadIdx.x + (int64_t)q * WM_THREADS;
        if (c < cols) lds[c] = __builtin_sqrtf(p.v[q]);
    }
    for (int64_t c = threadIdx.x + (int64_t)WM_SR_PRE * WM_THREADS; c < cols; c += WM_THREADS)
        lds[c] = __builtin_sqrtf(sr[c]);
    lds_barrier();
    return lds;
}
static __device__ __forceinline__ u32x4 ld_sq4(const float* sq, int64_t i4) {
    return *(const u32x4*)(sq + 4 * i4);      // LDS or global, 16-byte aligned either way
}

// inclusive scan of one value per thread over the 1024-thread block; returns (inclusive, total)
template <bool LDS_ONLY = false>
static __device__ __forceinline__ uint32_t block_scan_wm(uint32_t v, uint32_t* lds_waves,
                                                         uint32_t& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    wm_barrier<LDS_ONLY>();  // protect lds_waves reuse
    if (lane == 63) lds_waves[wave] = x;
    wm_barrier<LDS_ONLY>();
    uint32_t base = 0, t = 0;
#pragma unroll
    for (int k = 0; k < WM_WAVES; ++k) {
        const uint32_t wk = lds_waves[k];
        if (k < wave) base += wk;
        t += wk;
    }
    total = t;
    return x + base;
}

// Every workgroup resolves the LATEST pass itself from its global histogram (8 KB, L2-resident):
// bin = first bin whose inclusive count reaches `remaining`.  Identical in every workgroup, so no
// separate "pick" launch and no inter-workgroup hand-off is needed; the result (prefix, remaining)
// is left in the state by the matrix's first workgroup, so the next pass starts from it instead
// of resolving all earlier passes again.  Two adjacent bins per thread: one block scan per pick.
struct PickLoad {                // the pick's global loads, issued before anything that can wait on memory
    uint32_t c0, c1, prefix, remaining;
};
static __device__ __forceinline__ PickLoad pick_load(const MatrixSelState* st, int upto, uint32_t rank0) {
    PickLoad p;
    p.c0 = p.c1 = 0; p.prefix = 0; p.remaining = rank0;
    if (upto == 0) return p;
    const int bins = upto == 3 ? 1024 : 2048;
    const int b0 = 2 * (int)threadIdx.x;
    if (b0 < bins) {
        const uint2 two = *(const uint2*)(st->hist[upto - 1] + b0);
        p.c0 = two.x; p.c1 = two.y;
    }
    if (upto >= 2) {
        p.prefix = st->resolved[upto - 2][0];
        p.remaining = st->resolved[upto - 2][1];
    }
    return p;
}

// prefix (selected high bits) and remaining rank after `upto` resolved passes
static __device__ __forceinline__ void resolve(MatrixSelState* st, int upto, const PickLoad& p, bool writer,
                                               uint32_t* wave4, uint32_t* out2, uint32_t& prefix,
                                               uint32_t& remaining) {
    prefix = p.prefix;
    remaining = p.remaining;
    if (upto == 0) return;
    uint32_t total;
    const uint32_t incl = block_scan_wm(p.c0 + p.c1, wave4, total);
    const uint32_t excl = incl - (p.c0 + p.c1);
    if (excl < remaining && remaining <= incl) {
        const bool second = remaining > excl + p.c0;
        out2[0] = (uint32_t)(2 * threadIdx.x + (second ? 1 : 0));
        out2[1] = remaining - excl - (second ? p.c0 : 0u);
    }
    __syncthreads();
    const int shift = upto == 1 ? 21 : (upto == 2 ? 10 : 0);
    prefix |= out2[0] << shift;
    remaining = out2[1];
    __syncthreads();
    if (writer && threadIdx.x == 0) {
        st->resolved[upto - 1][0] = prefix;
        st->resolved[upto - 1][1] = remaining;
    }
}

struct MatGroup {
    int n;
    int32_t start[WMAX + 1];      // workgroup prefix over the group's matrices
    void* w[WMAX];
    const float* sq[WMAX];
    int64_t rows[WMAX];
    int64_t cols[WMAX];
    uint32_t rank0[WMAX];
    MatrixSelState* st[WMAX];
    uint8_t* mask[WMAX];
};

template <int DT, int PASS, bool VECTOR, int SUB = 1>
__global__ __launch_bounds__(WM_THREADS) void wanda_matrix_hist_kernel(const MatGroup g) {
    const int it = group_item(g, blockIdx.x);
    const unsigned lb = blockIdx.x - g.start[it], nb = g.start[it + 1] - g.start[it];
    const void* __restrict__ w = g.w[it];
    const float* sq = g.sq[it];
    const int64_t rows = g.rows[it], cols = g.cols[it];
    const uint32_t rank0 = g.rank0[it];
    MatrixSelState* st = g.st[it];
    constexpr int SHIFT = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
    constexpr int BITS = PASS == 2 ? 10 : 11;
    constexpr uint32_t HI_MASK = PASS == 0 ? 0u : (PASS == 1 ? 0xffe00000u : 0xfffffc00u);
    constexpr int N = Vec<DT>::N;
    // SUB > 1: SUB interleaved counters per bin, chosen by the lane — the top digit has few
    // distinct values, and lanes of one LDS atomic that meet at one address are served one by one
    __shared__ uint32_t h[2048 * SUB];
    __shared__ uint32_t wave4[WM_WAVES];
    __shared__ uint32_t out2[2];
    const PickLoad pl = pick_load(st, PASS, rank0);   // in flight while the LDS is set up
    for (int i = threadIdx.x; i < 2048 * SUB; i += WM_THREADS) h[i] = 0;
    const uint32_t sub = SUB > 1 ? (threadIdx.x & (SUB - 1)) : 0u;
    __shared__ __attribute__((aligned(16))) float sq_lds[VECTOR ? WM_SQ_LDS : 4];
    if (VECTOR) sq = stage_sq(sq, cols, sq_lds);
    uint32_t prefix, remaining;
    resolve(st, PASS, pl, lb == 0, wave4, out2, prefix, remaining);
    __syncthreads();
    if (VECTOR) {
        const int64_t vpr = cols / N;                 // vectors per row
        const int64_t nvec = rows * vpr;
        // WM_UNROLL independent 16-byte loads in flight per thread (one per stride of the
        // workgroup set): with a single load per iteration the pass ran at the latency bound
        const int64_t stride = (int64_t)nb * WM_THREADS;
        // column of a vector without a 64-bit modulo per vector (that division was most of the
        // pass's instructions): one 32-bit modulo up front, then add-and-wrap per stride
        const uint32_t vpr32 = (uint32_t)vpr, step32 = (uint32_t)(stride % vpr);
        uint32_t cv = (uint32_t)(((int64_t)lb * WM_THREADS + threadIdx.x) % vpr);
        for (int64_t v0 = (int64_t)lb * WM_THREADS + threadIdx.x; v0 < nvec; v0 += stride * WM_UNROLL) {
            u32x4 wv[WM_UNROLL];
#pragma unroll
            for (int j = 0; j < WM_UNROLL; ++j)
                if (v0 + j * stride < nvec) wv[j] = ld16(w, v0 + j * stride);
#pragma unroll
            for (int j = 0; j < WM_UNROLL; ++j) {
                const int64_t v = v0 + j * stride;
                const int64_t c0 = (int64_t)cv * N;
                cv += step32;
                if (cv >= vpr32) cv -= vpr32;
                if (v >= nvec) continue;
                float f[N];
                Vec<DT>::unpack(wv[j], f);
#pragma unroll
                for (int q = 0; q < N / 4; ++q) {
                    const u32x4 s4 = ld_sq4(sq, c0 / 4 + q);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t b = __float_as_uint(__builtin_fabsf(f[4 * q + i]) * __uint_as_float(s4[i]));
                        if ((b & HI_MASK) == prefix) atomicAdd(&h[((b >> SHIFT) & ((1u << BITS) - 1u)) * SUB + sub], 1u);
                    }
                }
            }
        }
    } else {
        for (int64_t r = lb; r < rows; r += nb)
            for (int64_t c = threadIdx.x; c < cols; c += WM_THREADS) {
                const uint32_t b = metric_bits<DT>(w, r * cols + c, sq[c]);
                if ((b & HI_MASK) == prefix) atomicAdd(&h[((b >> SHIFT) & ((1u << BITS) - 1u)) * SUB + sub], 1u);
            }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (1 << BITS); i += WM_THREADS) {
        uint32_t c = 0;
#pragma unroll
        for (int q = 0; q < SUB; ++q) c += h[i * SUB + q];
        if (c) atomicAdd(&st->hist[PASS][i], c);
    }
}

template <int DT, bool VECTOR>
__global__ __launch_bounds__(WM_THREADS) void wanda_matrix_apply_kernel(const MatGroup g) {
    const int it = group_item(g, blockIdx.x);
    const unsigned lb = blockIdx.x - g.start[it], nb = g.start[it + 1] - g.start[it];
    void* w = g.w[it];
    const float* sq = g.sq[it];
    const int64_t rows = g.rows[it], cols = g.cols[it];
    const uint32_t rank0 = g.rank0[it];
    MatrixSelState* st = g.st[it];
    uint8_t* mask_out = g.mask[it];
    constexpr int N = Vec<DT>::N;
    __shared__ uint32_t wave4[WM_WAVES];
    __shared__ uint32_t out2[2];
    const PickLoad pl = pick_load(st, 3, rank0);
    __shared__ __attribute__((aligned(16))) float sq_lds[VECTOR ? WM_SQ_LDS : 4];
    if (VECTOR) sq = stage_sq(sq, cols, sq_lds);
    uint32_t thres_bits, remaining;
    resolve(st, 3, pl, false, wave4, out2, thres_bits, remaining);
    const float thres = __uint_as_float(thres_bits);
    if (VECTOR) {
        const int64_t vpr = cols / N;
        const int64_t nvec = rows * vpr;
        const int64_t stride = (int64_t)nb * WM_THREADS;
        const uint32_t vpr32 = (uint32_t)vpr, step32 = (uint32_t)(stride % vpr);
        uint32_t cv = (uint32_t)(((int64_t)lb * WM_THREADS + threadIdx.x) % vpr);
        for (int64_t v0 = (int64_t)lb * WM_THREADS + threadIdx.x; v0 < nvec; v0 += stride * WM_UNROLL) {
            u32x4 wv[WM_UNROLL];
#pragma unroll
            for (int j = 0; j < WM_UNROLL; ++j)
                if (v0 + j * stride < nvec) wv[j] = ld16(w, v0 + j * stride);
#pragma unroll
            for (int j = 0; j < WM_UNROLL; ++j) {
                const int64_t v = v0 + j * stride;
                const int64_t c0 = (int64_t)cv * N;
                cv += step32;
                if (cv >= vpr32) cv -= vpr32;
                if (v >= nvec) continue;
                float f[N];
                Vec<DT>::unpack(wv[j], f);
                uint32_t lo = 0, hi = 0;
                bool any = false;
#pragma unroll
                for (int q = 0; q < N / 4; ++q) {
                    const u32x4 s4 = ld_sq4(sq, c0 / 4 + q);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int e = 4 * q + i;
                        // W_metric <= thres (W:556): false for NaN metrics, as in torch
                        const bool prune = (__builtin_fabsf(f[e]) * __uint_as_float(s4[i])) <= thres;
                        if (prune) { f[e] = 0.0f; any = true; }
                        if (e < 4) lo |= (prune ? 1u : 0u) << (8 * e);
                        else hi |= (prune ? 1u : 0u) << (8 * (e - 4));
                    }
                }
                if (any) st16(w, v, Vec<DT>::pack(f));
                if (mask_out) {
                    uint8_t* m = mask_out + v * N;
                    *(uint32_t*)m = lo;
                    if (N == 8) *(uint32_t*)(m + 4) = hi;
                }
            }
        }
    } else {
        for (int64_t r = lb; r < rows; r += nb)
            for (int64_t c = threadIdx.x; c < cols; c += WM_THREADS) {
                const int64_t i = r * cols + c;
                const float mval = __uint_as_float(metric_bits<DT>(w, i, sq[c]));
                const bool prune = mval <= thres;
                if (prune) Vec<DT>::store1(w, i, 0.0f);
                if (mask_out) mask_out[i] = prune ? 1 : 0;
            }
    }
}

// =====================================================================================
// K7 matrix mode, sampled bracket: 2 reads + 1 write of W instead of 4 + 1, in TWO dependent launches
// =====================================================================================
// The three histogram passes above read W three times to find ONE number.  Here a sample of
// WS_SAMPLE_VECS vectors per matrix (pseudo-randomly placed, one per stride) brackets the (k+1)-th
// smallest metric between two sample order statistics 5 sigma either side of its expected rank
// (~4 % of the elements); ONE full pass counts exactly what lies below the bracket and histograms
// what lies inside it (512 bins: an LDS atomic for 4 % of the elements instead of all of them);
// the apply pass then knows the bin that holds the threshold, zeroes everything below that bin,
// keeps everything above it and appends the bin's own few hundred elements (index, metric bits)
// to a list; the last workgroup to finish selects the threshold among them exactly and settles
// them.  Every count is exact, so the result is the reference's (W:555-558) bit for bit; when the
// bracket misses (probability ~1e-6 per matrix), the bin is too crowded for the list (massive
// ties) or the threshold is not finite, every workgroup of the matrix sees that from the counts
// before it has written anything, and the matrix's first workgroup runs the three-histogram
// selection on it by itself (matrix_fallback_body).
//
// Round 5, after a phase clock on the device (tools/diag/k7_clock.py: sample 14.9 us alone on 4
// workgroups, 1.6 us to the next launch, bracket pass 19 us of which 11 streaming, apply pass 21 us
// of which 4.2 before its first load, 5 us of threshold settling at the end): the sample no longer
// has a launch of its own.  EVERY workgroup of the counting pass takes the sample of its matrix
// itself (2048 vectors, L2 hits after the first workgroup; the result is a pure function of W and
// the statistic, so all workgroups hold the same bracket and nobody waits for anybody — no flag,
// no spin, nothing that could deadlock against another process's launch) while the WS_PRE vectors
// per thread that are its share of the matrix are already on their way into registers; counts go
// to a slot per workgroup (no zeroed state, no atomics meeting at the memory side) which the
// apply pass sums in its prologue, again with its share of W already in flight.
// (WS_SAMPLE_VECS ... BracketState: wanda_matrix_state.h)

struct BracketGroup {
    MatGroup m;
    BracketState* bs[WMAX];
    const float* sr[WMAX];          // the raw statistic (sqrt taken while staging it into LDS)
};

// rank (1-based) -> (bin, rank inside the bin) over an LDS histogram of 2048 bins, WM_THREADS threads
static __device__ __forceinline__ void find_rank_wm(const uint32_t* h, uint32_t rank, uint32_t* waves,
                                                    uint32_t* out2) {
    const uint32_t c0 = h[2 * threadIdx.x], c1 = h[2 * threadIdx.x + 1];
    uint32_t total;
    const uint32_t incl = block_scan_wm(c0 + c1, waves, total);
    const uint32_t excl = incl - (c0 + c1);
    if (excl < rank && rank <= incl) {
        const bool second = rank > excl + c0;
        out2[0] = 2 * threadIdx.x + (second ? 1u : 0u);
        out2[1] = rank - excl - (second ? c0 : 0u);
    }
    __syncthreads();
}
// the counting pass: sample -> bracket [lo, hi) (every workgroup, identically), then the exact
// count below the bracket and the WS_BINS-bin histogram inside it over the workgroup's share of W.
// The sample's two order statistics are taken at the resolution of ONE histogram — 4096 bins of
// 1/16 octave (metric bits >> 19): the bracket's edges are bin edges, up to 4 % of the elements wider
// on either side than the exact order statistics would make it, which costs the exact pass a few
// more LDS atomics and saves the prologue a second histogram level (two more scans, five barriers:
// 3.5 us of every workgroup's time by the phase clock).  Nothing about exactness depends on where
// the edges lie.
#define WS_SBINS 4096
#define WS_SSUB 4                      // interleaved counters per sample bin (few dozen live bins)
template <int DT>
__global__ __launch_bounds__(WM_THREADS) void wanda_matrix_sbracket_kernel(const BracketGroup bg,
                                                                           uint32_t* __restrict__ part) {
    const MatGroup& g = bg.m;
    const int it = group_item(g, blockIdx.x);
    const unsigned lb = blockIdx.x - g.start[it], nb = g.start[it + 1] - g.start[it];
    const void* __restrict__ w = g.w[it];
    const int64_t rows = g.rows[it], cols = g.cols[it];
    BracketState* bs = bg.bs[it];
    constexpr int N = Vec<DT>::N;
    constexpr int S = WS_SAMPLE_VECS * N;
    constexpr int VPT = WS_SAMPLE_VECS / WM_THREADS;          // sample vectors per thread
    __shared__ uint32_t h[WS_BINS];
    __shared__ uint32_t red[WM_WAVES];
    __shared__ __attribute__((aligned(16))) float sq_lds[WM_SQ_LDS];
    __shared__ __attribute__((aligned(16))) uint32_t h1s[WS_SBINS * WS_SSUB];
    __shared__ uint32_t waves[WM_WAVES], o_lo[2], o_hi[2], brk[4];
    K7_ENTER(1); K7_STAMP(1, 0);
    const int64_t vpr = cols / N, nvec = rows * vpr;
    const uint32_t vpr32 = (uint32_t)vpr;
    // ---- the prologue's global loads, issued before anything waits --------------------------
    const SqrtPre srp = stage_sqrt_issue(bg.sr[it], cols);
    // the sample: one vector per stride of the matrix, at a pseudo-random place inside its stride
    // (a regular stride can be a multiple of the row length and then sees one column group only)
    const uint32_t step = (uint32_t)(nvec / WS_SAMPLE_VECS);
    u32x4 sv[VPT];
    uint32_t sc0[VPT];
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const uint32_t i = threadIdx.x + WM_THREADS * j;
        const uint32_t jitter = (uint32_t)(((uint64_t)(i * 2654435761u) * (uint64_t)step) >> 32);
        const uint32_t v = i * step + jitter;
        sc0[j] = (v % vpr32) * N;
        sv[j] = ld16(w, (int64_t)v);
    }
    // A compute unit serves its waves' loads in the order they arrive: every wave's prologue loads
    // are queued before any wave's W loads
    lds_barrier();
    // The first WS_PRE vectors per thread of the workgroup's share of W, in registers across the
    // sample.  Not more: a wave cannot run ahead of its own loads by more than the memory pipeline
    // holds — with the whole share (12 vectors) issued up front the waves sat in the ISSUE of those
    // loads until most of the stream had arrived, and the sample waited with them.
    const uint32_t nvec32 = (uint32_t)nvec, stride32 = nb * WM_THREADS;     // (numel < 2^32)
    const uint32_t vfirst32 = lb * WM_THREADS + threadIdx.x;
    u32x4 cur[WS_PRE];
#pragma unroll
    for (int j = 0; j < WS_PRE; ++j) {
        const uint32_t v = vfirst32 + j * stride32;
        cur[j] = ld16(w, (int64_t)(v < nvec32 ? v : nvec32 - 1u));  // (clamped: no branch around a load)
    }
    for (int i = threadIdx.x; i < WS_BINS; i += WM_THREADS) h[i] = 0;
    for (int i = threadIdx.x; i < WS_SBINS * WS_SSUB; i += WM_THREADS) h1s[i] = 0;
    const float* sq = stage_sqrt_finish(srp, bg.sr[it], cols, sq_lds);      // (ends with a barrier)
    K7_STAMP(1, 1);
    // ---- the sample's histogram -------------------------------------------------------------
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        float f[N];
        Vec<DT>::unpack(sv[j], f);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const uint32_t b = __float_as_uint(__builtin_fabsf(f[e]) * sq[sc0[j] + e]);
            const uint32_t top = b >> 19;                       // (sign-bit patterns: the last bin)
            atomicAdd(&h1s[(top < (uint32_t)WS_SBINS ? top : (uint32_t)WS_SBINS - 1u) * WS_SSUB + (threadIdx.x & (WS_SSUB - 1))], 1u);
        }
    }
    lds_barrier();
    K7_STAMP(1, 2);
    // sample ranks 5 sigma either side of the expected one; four bins per thread, one scan
    const double numel = (double)rows * (double)cols;
    const double p = (double)g.rank0[it] / numel;
    const double mid = p * S;
    const double dev = 5.0 * __builtin_sqrt((double)S * p * (1.0 - p)) + 8.0;
    const bool open_lo = mid - dev < 1.0, open_hi = mid + dev > (double)S;
    const uint32_t r_lo = open_lo ? 1u : (uint32_t)(mid - dev);
    const uint32_t r_hi = open_hi ? (uint32_t)S : (uint32_t)(mid + dev);
    {
        uint32_t c4[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const u32x4 x = *(const u32x4*)(h1s + (4 * threadIdx.x + k) * WS_SSUB);
            c4[k] = x[0] + x[1] + x[2] + x[3];
        }
        const uint32_t csum = c4[0] + c4[1] + c4[2] + c4[3];
        uint32_t total;
        const uint32_t incl = block_scan_wm<true>(csum, waves, total);
        const uint32_t excl = incl - csum;
        if (excl < r_lo && r_lo <= incl) {
            uint32_t e = excl; int d = 0; bool on = true;      // first bin whose running count reaches the rank
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                on = on && r_lo > e + c4[k];
                if (on) { e += c4[k]; d = k + 1; }
            }
            o_lo[0] = 4 * threadIdx.x + (uint32_t)d;
        }
        if (excl < r_hi && r_hi <= incl) {
            uint32_t e = excl; int d = 0; bool on = true;      // first bin whose running count reaches the rank
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                on = on && r_hi > e + c4[k];
                if (on) { e += c4[k]; d = k + 1; }
            }
            o_hi[0] = 4 * threadIdx.x + (uint32_t)d;
        }
    }
    lds_barrier();
    if (threadIdx.x == 0) {
        const uint32_t lo = open_lo ? 0u : (o_lo[0] << 19);
        const uint64_t hi64 = open_hi ? 0x100000000ull : ((uint64_t)(o_hi[0] + 1u) << 19);
        const uint32_t hi = hi64 > 0xffffffffull ? 0xffffffffu : (uint32_t)hi64;
        const uint32_t width = hi - lo;
        int shift = 0;
        while (shift < 31 && ((width - 1u) >> shift) >= (uint32_t)WS_BINS) ++shift;
        brk[0] = lo; brk[1] = hi; brk[2] = (uint32_t)shift; brk[3] = hi > lo ? 1u : 0u;
        if (lb == 0) {
            bs->list_count = 0u; bs->ticket = 0u; bs->fallback = 0u;
            bs->lo = lo; bs->hi = hi; bs->shift = (uint32_t)shift; bs->valid = hi > lo ? 1u : 0u;
        }
    }
    lds_barrier();
    K7_STAMP(1, 3);
    const uint32_t lo = brk[0], width = brk[1] - brk[0], shift = brk[2];
    // ---- the exact counts over the share of W: the next WS_PRE loads in flight while the ---------
    // ---- current ones are counted                                                       ---------
    uint32_t below = 0;
    if (brk[3]) {
        const uint32_t step32 = stride32 % vpr32;
        uint32_t cv = vfirst32 % vpr32;
        const uint32_t wg_first = lb * WM_THREADS;              // (uniform: the loop's trip count)
        for (uint32_t base = 0; wg_first + base < nvec32; base += WS_PRE * stride32) {
            u32x4 nxt[WS_PRE];
            const bool more = wg_first + base + WS_PRE * stride32 < nvec32;
            if (more) {
#pragma unroll
                for (int j = 0; j < WS_PRE; ++j) {
                    const uint32_t v = vfirst32 + base + (WS_PRE + j) * stride32;
                    nxt[j] = ld16(w, (int64_t)(v < nvec32 ? v : nvec32 - 1u));
                }
            }
#pragma unroll
            for (int j = 0; j < WS_PRE; ++j) {
                const uint32_t c0 = cv * N;
                cv += step32;
                if (cv >= vpr32) cv -= vpr32;
                if (vfirst32 + base + j * stride32 < nvec32) {
                    float f[N];
                    Vec<DT>::unpack(cur[j], f);
#pragma unroll
                    for (int q = 0; q < N / 4; ++q) {
                        const u32x4 s4 = ld_sq4(sq, c0 / 4 + q);
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const uint32_t b = __float_as_uint(__builtin_fabsf(f[4 * q + i]) * __uint_as_float(s4[i]));
                            const uint32_t rel = b - lo;
                            below += b < lo ? 1u : 0u;
                            if (b >= lo && rel < width) atomicAdd(&h[rel >> shift], 1u);
                        }
                    }
                }
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < WS_PRE; ++j) cur[j] = nxt[j];
            }
        }
    }
    K7_STAMP(1, 4);
    // the workgroup's slot: its histogram and its count below the bracket
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) below += __shfl_xor(below, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = below;
    lds_barrier();
    uint32_t* slot = part + (size_t)blockIdx.x * WS_PART_WORDS;
    if (threadIdx.x < WS_BINS) slot[threadIdx.x] = h[threadIdx.x];
    if (threadIdx.x == WS_BINS) {
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < WM_WAVES; ++k) t += red[k];
        slot[WS_BINS] = t;
    }
    K7_STAMP(1, 5);
    K7_EXIT(1);
}

// The exact finish for a matrix the sampled passes cannot settle (the bracket missed, ~1e-6 per
// matrix; the threshold's bin reaches non-finite bit patterns; the bin is too crowded for the
// list: massive ties), ON THE DEVICE and inside the apply pass: every one of these conditions is
// known from the counts in the prologue, to every workgroup of the matrix alike, BEFORE anything
// of W has been written — so all of them leave, and the matrix's first workgroup runs the whole
// three-histogram selection and the apply pass by itself (LDS histograms, no other workgroup to
// wait for: no grid barrier, nothing that could deadlock with another resident instance, and no
// question of one XCD seeing another's stores).  Slow (one CU streams the matrix four times:
// ~1 ms for 8.6 M elements) and rare.  Rounds 3-4 decided this on the host (a flag read-back and a
// stream round trip per call), round 5 first by a conditional launch of its own (4 us at the end
// of every call for a launch that almost never had anything to do).
// How often it ran, by reason (1: bracket miss / non-finite bin, 2: crowded bin, 3: a list that
// does not match its count — cannot happen, counted so that a test would see it): read and cleared
// by ecoflap_wanda_fallback_counts (tests: ordinary data must not take it).
__device__ unsigned int eco_k7_fallbacks[4];
extern "C" int ecoflap_wanda_fallback_counts(unsigned int* out4, int reset) {
    if (out4) {
        const hipError_t e = hipMemcpyFromSymbol(out4, HIP_SYMBOL(eco_k7_fallbacks), sizeof(unsigned int) * 4);
        if (e != hipSuccess) return (int)e;
    }
    if (reset) {
        const unsigned int z[4] = {0u, 0u, 0u, 0u};
        const hipError_t e = hipMemcpyToSymbol(HIP_SYMBOL(eco_k7_fallbacks), z, sizeof(z));
        if (e != hipSuccess) return (int)e;
    }
    return 0;
}

template <int DT, int PASS>
static __device__ __forceinline__ void fallback_hist_pass(const void* __restrict__ w, const float* sq,
                                                          int64_t nvec, uint32_t vpr32, uint32_t* h,
                                                          uint32_t prefix) {
    constexpr int N = Vec<DT>::N;
    constexpr int SHIFT = PASS == 0 ? 21 : (PASS == 1 ? 10 : 0);
    constexpr uint32_t DMASK = PASS == 2 ? 1023u : 2047u;
    constexpr uint32_t HI_MASK = PASS == 0 ? 0u : (PASS == 1 ? 0xffe00000u : 0xfffffc00u);
    for (int i = threadIdx.x; i < 2048; i += WM_THREADS) h[i] = 0;
    __syncthreads();
    uint32_t cv = threadIdx.x % vpr32;
    const uint32_t step32 = WM_THREADS % vpr32;
    for (int64_t v = threadIdx.x; v < nvec; v += WM_THREADS) {
        const int64_t c0 = (int64_t)cv * N;
        cv += step32;
        if (cv >= vpr32) cv -= vpr32;
        float f[N];
        Vec<DT>::unpack(ld16(w, v), f);
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const uint32_t b = __float_as_uint(__builtin_fabsf(f[e]) * sq[c0 + e]);
            if ((b & HI_MASK) == prefix) atomicAdd(&h[(b >> SHIFT) & DMASK], 1u);
        }
    }
    __syncthreads();
}

// one workgroup, the whole matrix: h = 2048 words of LDS, sq = the staged sqrt table
template <int DT>
static __device__ void matrix_fallback_body(void* w, const float* sq, int64_t rows, int64_t cols, uint32_t rank0,
                                            uint8_t* mask_out, uint32_t* h, uint32_t* wave4, uint32_t* out2,
                                            unsigned reason) {
    if (threadIdx.x == 0) atomicAdd(&eco_k7_fallbacks[reason & 3u], 1u);
    constexpr int N = Vec<DT>::N;
    const int64_t vpr = cols / N, nvec = rows * vpr;
    const uint32_t vpr32 = (uint32_t)vpr;
    uint32_t prefix = 0, remaining = rank0;
    __syncthreads();
    fallback_hist_pass<DT, 0>(w, sq, nvec, vpr32, h, prefix);
    find_rank_wm(h, remaining, wave4, out2);
    prefix |= out2[0] << 21; remaining = out2[1];
    __syncthreads();
    fallback_hist_pass<DT, 1>(w, sq, nvec, vpr32, h, prefix);
    find_rank_wm(h, remaining, wave4, out2);
    prefix |= out2[0] << 10; remaining = out2[1];
    __syncthreads();
    fallback_hist_pass<DT, 2>(w, sq, nvec, vpr32, h, prefix);
    find_rank_wm(h, remaining, wave4, out2);
    prefix |= out2[0];
    __syncthreads();
    const float thres = __uint_as_float(prefix);     // sorted[k]
    uint32_t cv = threadIdx.x % vpr32;
    const uint32_t step32 = WM_THREADS % vpr32;
    for (int64_t v = threadIdx.x; v < nvec; v += WM_THREADS) {
        const int64_t c0 = (int64_t)cv * N;
        cv += step32;
        if (cv >= vpr32) cv -= vpr32;
        float f[N];
        Vec<DT>::unpack(ld16(w, v), f);
        uint32_t lo = 0, hi = 0;
        bool any = false;
#pragma unroll
        for (int e = 0; e < N; ++e) {
            // W_metric <= thres (W:556): false for NaN metrics, as in torch
            const bool prune = (__builtin_fabsf(f[e]) * sq[c0 + e]) <= thres;
            if (prune) { f[e] = 0.0f; any = true; }
            if (e < 4) lo |= (prune ? 1u : 0u) << (8 * e);
            else hi |= (prune ? 1u : 0u) << (8 * (e - 4));
        }
        if (any) st16(w, v, Vec<DT>::pack(f));
        if (mask_out) {
            uint8_t* m = mask_out + v * N;
            *(uint32_t*)m = lo;
            if (N == 8) *(uint32_t*)(m + 4) = hi;
        }
    }
}

template <int DT>
__global__ __launch_bounds__(WM_THREADS) void wanda_matrix_apply2_kernel(const BracketGroup bg,
                                                                         const uint32_t* __restrict__ part) {
    const MatGroup& g = bg.m;
    const int it = group_item(g, blockIdx.x);
    const unsigned lb = blockIdx.x - g.start[it], nb = g.start[it + 1] - g.start[it];
    void* w = g.w[it];
    const int64_t rows = g.rows[it], cols = g.cols[it];
    const uint32_t rank0 = g.rank0[it];
    BracketState* bs = bg.bs[it];
    uint8_t* mask_out = g.mask[it];
    constexpr int N = Vec<DT>::N;
    __shared__ uint32_t wave4[WM_WAVES];
    __shared__ uint32_t out2[2];
    __shared__ uint32_t is_last, below_s, ln, lbase, binc_s;
    __shared__ __attribute__((aligned(16))) uint32_t arr[WS_CAP];   // (first the slots' sums, 8 x 512)
    __shared__ __attribute__((aligned(16))) uint32_t hsel[4096];
    __shared__ __attribute__((aligned(16))) float sq_lds[WM_SQ_LDS];
    K7_ENTER(2); K7_STAMP(2, 0);
    if (!bs->valid) {                          // (an empty bracket: cannot happen, handled all the same)
        if (lb == 0) {
            const float* sq0 = stage_sqrt(bg.sr[it], cols, sq_lds);
            matrix_fallback_body<DT>(w, sq0, rows, cols, rank0, mask_out, hsel, wave4, out2, 1u);
        }
        return;
    }
    const uint32_t lo = bs->lo, hi = bs->hi, shift = bs->shift;
    // Loads return in order, so the prologue's own loads go FIRST and the workgroup's share of W
    // right behind them: the prologue then runs while W streams in.
    // The matrix's counts: the sum of its workgroups' slots (L2-resident, 2 KB each)
    const uint32_t* pp = part + (size_t)g.start[it] * WS_PART_WORDS;
    // eight groups of 128 threads, 4 bins per thread, one slot per group at a time: 12 slots per
    // group in flight, one latency for up to 96 workgroups (more: further rounds, still ahead of
    // the W loads); the groups' sums meet in LDS
    constexpr int PXG = WM_THREADS / (WS_BINS / 4), PXN = 12;
    const unsigned grp = threadIdx.x / (WS_BINS / 4), b4 = (threadIdx.x % (WS_BINS / 4)) * 4u;
    u32x4 px[PXN];
#pragma unroll
    for (int u = 0; u < PXN; ++u) {
        const unsigned q = grp + (unsigned)PXG * u;
        const u32x4 x = *(const u32x4*)(pp + (size_t)(q < nb ? q : nb - 1u) * WS_PART_WORDS + b4);
        px[u] = q < nb ? x : u32x4{0u, 0u, 0u, 0u};
    }
    // one wave: the slots' counts below the bracket
    const bool tb_wave = threadIdx.x >= WS_BINS && threadIdx.x < WS_BINS + 64;
    uint32_t tb0 = 0, tb1 = 0;
    if (tb_wave) {
        const unsigned q0 = threadIdx.x - WS_BINS, q1 = q0 + 64u;
        const uint32_t x0 = pp[(size_t)(q0 < nb ? q0 : nb - 1u) * WS_PART_WORDS + WS_BINS];
        const uint32_t x1 = pp[(size_t)(q1 < nb ? q1 : nb - 1u) * WS_PART_WORDS + WS_BINS];
        tb0 = q0 < nb ? x0 : 0u;
        tb1 = q1 < nb ? x1 : 0u;
    }
    u32x4 acc = {0u, 0u, 0u, 0u};
    if (nb > (unsigned)(PXG * PXN)) {          // (rare: one matrix on more than 96 workgroups)
        for (unsigned q = grp + (unsigned)(PXG * PXN); q < nb; q += PXG)
            acc += *(const u32x4*)(pp + (size_t)q * WS_PART_WORDS + b4);
        if (tb_wave)
            for (unsigned q = threadIdx.x - WS_BINS + 128u; q < nb; q += 64u) tb0 += pp[(size_t)q * WS_PART_WORDS + WS_BINS];
    }
    const SqrtPre srp = stage_sqrt_issue(bg.sr[it], cols);
    if (threadIdx.x == 0) ln = 0u;
    lds_barrier();          // (every wave's prologue loads are queued before any wave's W loads)
    const int64_t vpr = cols / N;
    const int64_t nvec = rows * vpr;
    const uint32_t nvec32 = (uint32_t)nvec, stride32 = nb * WM_THREADS;
    const uint32_t vfirst32 = lb * WM_THREADS + threadIdx.x;
    const int64_t stride = (int64_t)stride32, vfirst = (int64_t)vfirst32;
    u32x4 cur[WS_PRE];
#pragma unroll
    for (int j = 0; j < WS_PRE; ++j) {
        const uint32_t v = vfirst32 + j * stride32;
        cur[j] = ld16(w, (int64_t)(v < nvec32 ? v : nvec32 - 1u));  // (clamped: no branch around a load)
    }
    {
#pragma unroll
        for (int u = 0; u < PXN; ++u) acc += px[u];
        *(u32x4*)(arr + grp * WS_BINS + b4) = acc;
    }
    if (tb_wave) {
        uint32_t tb = tb0 + tb1;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) tb += __shfl_xor(tb, off, 64);
        if (threadIdx.x == WS_BINS) below_s = tb;
    }
    const float* sq = stage_sqrt_finish(srp, bg.sr[it], cols, sq_lds);      // (ends with a barrier)
    uint32_t c = 0;
    if (threadIdx.x < WS_BINS) {
#pragma unroll
        for (int u = 0; u < PXG; ++u) c += arr[u * WS_BINS + threadIdx.x];
    }
    const uint32_t below = below_s;
    uint32_t total;
    const uint32_t incl = block_scan_wm<true>(c, wave4, total);
    const bool miss = rank0 <= below || rank0 - below > total;
    const uint32_t r = rank0 - below;
    if (threadIdx.x == 0) { out2[0] = 0xffffffffu; out2[1] = 0; binc_s = 0; }
    lds_barrier();
    if (!miss && incl - c < r && r <= incl) { out2[0] = threadIdx.x; out2[1] = r - (incl - c); binc_s = c; }
    lds_barrier();
    const uint32_t bin = out2[0], rr = out2[1], binc = binc_s;
    uint64_t binhi64 = (uint64_t)lo + ((uint64_t)(bin + 1u) << shift);
    if (binhi64 > (uint64_t)hi) binhi64 = hi;
    // The cases the two passes cannot settle, known here to every workgroup of the matrix and
    // before any of them has written a byte of W: the bracket missed, the threshold's bin reaches
    // into Inf / NaN bit patterns (`metric <= thres` is not an order on bits there), the bin holds
    // more elements than the list (massive ties).  All leave; the first runs the exact finish.
    const bool unsettled = miss || bin == 0xffffffffu || binhi64 > 0x7f800000ull;
    if (unsettled || binc > (uint32_t)WS_CAP) {
        if (lb == 0) matrix_fallback_body<DT>(w, sq, rows, cols, rank0, mask_out, hsel, wave4, out2, unsettled ? 1u : 2u);
        return;
    }
    const uint32_t binlo = lo + (bin << shift), binw = (uint32_t)binhi64 - binlo;
    K7_STAMP(2, 1);
    {
        const uint32_t vpr32 = (uint32_t)vpr, step32 = stride32 % vpr32;
        uint32_t cv = vfirst32 % vpr32;
        auto apply_vec = [&](const u32x4& x, int64_t v, int64_t c0) {
            float f[N];
            Vec<DT>::unpack(x, f);
            uint32_t lo4 = 0, hi4 = 0;
            bool any = false, open_any = false;
#pragma unroll
            for (int q = 0; q < N / 4; ++q) {
                const u32x4 s4 = ld_sq4(sq, c0 / 4 + q);
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int e = 4 * q + i;
                    const uint32_t b = __float_as_uint(__builtin_fabsf(f[e]) * __uint_as_float(s4[i]));
                    const bool prune = b < binlo;
                    open_any |= (b - binlo) < binw;          // (b < binlo wraps to a huge value)
                    if (prune) { f[e] = 0.0f; any = true; }
                    if (mask_out) {
                        if (e < 4) lo4 |= (prune ? 1u : 0u) << (8 * e);
                        else hi4 |= (prune ? 1u : 0u) << (8 * (e - 4));
                    }
                }
            }
            if (!open_any) {
                if (any) st16(w, v, Vec<DT>::pack(f));
                if (mask_out) {
                    uint8_t* m = mask_out + v * N;
                    *(uint32_t*)m = lo4;
                    if (N == 8) *(uint32_t*)(m + 4) = hi4;
                }
            } else {
                // a vector with an element of the threshold's bin (a few hundred per matrix):
                // element stores only, and never the open element's own bytes (the last
                // workgroup may write them).  Metrics again from the untouched vector.
                float f0[N];
                Vec<DT>::unpack(x, f0);
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    const int64_t idx = v * N + e;
                    const uint32_t b = __float_as_uint(__builtin_fabsf(f0[e]) * sq[c0 + e]);
                    if ((b - binlo) < binw) {
                        // the workgroup's own list first (LDS; `hsel` is free until the settling):
                        // one atomic per WORKGROUP at the memory side instead of one per element —
                        // ~1000 returning atomics on one address were most of this pass's time
                        const uint32_t ls = atomicAdd(&ln, 1u);
                        if (ls < 2048u) { hsel[2 * ls] = (uint32_t)idx; hsel[2 * ls + 1] = b; continue; }
                        const uint32_t slot = atomicAdd(&bs->list_count, 1u);
                        if (slot < (uint32_t)WS_CAP) {
                            __hip_atomic_store(&bs->list_idx[slot], (uint32_t)idx, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                            __hip_atomic_store(&bs->list_bits[slot], b, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
                        }
                    } else {
                        const bool prune = b < binlo;
                        if (prune) Vec<DT>::store1(w, idx, 0.0f);
                        if (mask_out) mask_out[idx] = prune ? 1 : 0;
                    }
                }
            }
        };
        // the next WS_PRE loads in flight while the current vectors are decided and stored
        const uint32_t wg_first = lb * WM_THREADS;              // (uniform: the loop's trip count)
        for (uint32_t base = 0; wg_first + base < nvec32; base += WS_PRE * stride32) {
            u32x4 nxt[WS_PRE];
            const bool more = wg_first + base + WS_PRE * stride32 < nvec32;
            if (more) {
#pragma unroll
                for (int j = 0; j < WS_PRE; ++j) {
                    const uint32_t v = vfirst32 + base + (WS_PRE + j) * stride32;
                    nxt[j] = ld16(w, (int64_t)(v < nvec32 ? v : nvec32 - 1u));
                }
            }
#pragma unroll
            for (int j = 0; j < WS_PRE; ++j) {
                const int64_t c0 = (int64_t)cv * N;
                cv += step32;
                if (cv >= vpr32) cv -= vpr32;
                const uint32_t v = vfirst32 + base + j * stride32;
                if (v < nvec32) apply_vec(cur[j], (int64_t)v, c0);
            }
            if (more) {
#pragma unroll
                for (int j = 0; j < WS_PRE; ++j) cur[j] = nxt[j];
            }
        }
    }
    // ---- the workgroup's list joins the matrix's -------------------------------------------------
    K7_STAMP(2, 2);
    __syncthreads();
    {
        const uint32_t nl = ln < 2048u ? ln : 2048u;
        if (threadIdx.x == 0) lbase = nl ? atomicAdd(&bs->list_count, nl) : 0u;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < nl; i += WM_THREADS) {
            const uint32_t slot = lbase + i;
            if (slot < (uint32_t)WS_CAP) {
                __hip_atomic_store(&bs->list_idx[slot], hsel[2 * i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(&bs->list_bits[slot], hsel[2 * i + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    // ---- the last workgroup of this matrix settles the threshold's bin ----------------------
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    K7_STAMP(2, 3);
    if (threadIdx.x == 0)
        is_last = (__hip_atomic_fetch_add(&bs->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                   == nb - 1u) ? 1u : 0u;
    __syncthreads();
    K7_EXIT(2);
    if (!is_last) return;
#ifdef ECO_K7_CLOCK
    if (threadIdx.x == 0) atomicMin(&eco_k7_clk[3][14], wall_clock64());
#endif
    const uint32_t n = __hip_atomic_load(&bs->list_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (n != binc) {       // every element of the bin is appended exactly once: cannot happen; counted, never silent
        if (threadIdx.x == 0) { bs->fallback = 3u; atomicAdd(&eco_k7_fallbacks[3], 1u); }
        return;
    }
    // the list's metrics relative to the bin's low edge: all below binw <= 2^shift, so the rr-th
    // smallest takes ceil(shift / 12) digit passes (one for the usual bin of <= 4096 bit patterns)
    for (uint32_t i = threadIdx.x; i < n; i += WM_THREADS)
        arr[i] = __hip_atomic_load(&bs->list_bits[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - binlo;
    uint32_t prefix = 0, remaining = rr;
    const int passes = shift <= 12 ? 1 : (shift <= 24 ? 2 : 3);
#pragma unroll 1
    for (int pass = 3 - passes; pass < 3; ++pass) {
        const int sh = pass == 0 ? 24 : (pass == 1 ? 12 : 0);
        const uint32_t himask = pass == 0 ? 0u : (pass == 1 ? 0xff000000u : 0xfffff000u);
        const uint32_t dmask = pass == 0 ? 255u : 4095u;
        for (int i = threadIdx.x; i < 4096; i += WM_THREADS) hsel[i] = 0;
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n; i += WM_THREADS) {
            const uint32_t b = arr[i];
            if ((b & himask) == prefix) atomicAdd(&hsel[(b >> sh) & dmask], 1u);
        }
        __syncthreads();
        const u32x4 c4 = *(const u32x4*)(hsel + 4 * threadIdx.x);
        const uint32_t csum = c4[0] + c4[1] + c4[2] + c4[3];
        uint32_t tot;
        const uint32_t inc = block_scan_wm(csum, wave4, tot);
        uint32_t exc = inc - csum;
        if (exc < remaining && remaining <= inc) {
            int d = 0;
            while (remaining > exc + c4[d]) { exc += c4[d]; ++d; }
            out2[0] = 4 * threadIdx.x + (uint32_t)d;
            out2[1] = remaining - exc;
        }
        __syncthreads();
        prefix |= out2[0] << sh;
        remaining = out2[1];
        __syncthreads();
    }
    const uint32_t thres = prefix;           // sorted[k], relative to the bin's low edge
    for (uint32_t i = threadIdx.x; i < n; i += WM_THREADS) {
        const uint32_t idx = __hip_atomic_load(&bs->list_idx[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool prune = arr[i] <= thres;
        if (prune) Vec<DT>::store1(w, (int64_t)idx, 0.0f);
        if (mask_out) mask_out[idx] = prune ? 1 : 0;
    }
    K7_EXIT(3);
}

// ---- host side -----------------------------------------------------------------------------
// The sampled-bracket path (matrix-mode items big enough to sample one vector per stride; it
// stages sqrt(scaler_row) itself and clears its own state): 2 reads + 1 write of W instead of
// 4 + 1, in two launches.  DEFAULT since round 5 — the matrices it cannot settle are finished
// exactly inside the second launch (`matrix_fallback_body`), no flag crosses to the host and
// the call stays asynchronous.  ECOFLAP_WANDA_SAMPLED=0 (read at every call) selects the
// three-histogram path for every matrix.
void wanda_matrix_sampled(const ecoflap_wanda_item* items, int n_items, float* const* sq, bool* sampled_item) {
    const char* sampled_env = getenv("ECOFLAP_WANDA_SAMPLED");
    const bool force_legacy = sampled_env != nullptr && sampled_env[0] == '0';
    for (int i = 0; i < n_items; ++i) {
        const ecoflap_wanda_item& a = items[i];
        const int64_t nv = a.rows * a.cols / (a.dtype == ECOFLAP_F32 ? 4 : 8);
        sampled_item[i] = a.mode == ECOFLAP_WANDA_MATRIX && !force_legacy && item_vector_ok(a, sq[i]) &&
                          nv >= 8 * WS_SAMPLE_VECS && a.cols <= WM_SQ_LDS && a.rows * a.cols <= WS_MAX_NUMEL &&
                          (((uintptr_t)a.scaler_row) & 15u) == 0;
    }
}

int wanda_matrix_launch(const ecoflap_wanda_item* items, int n_items, float* const* sq,
                        MatrixSelState* const* st, BracketState* const* bst, uint32_t* part,
                        const bool* sampled_item, bool* done, hipStream_t s) {
    for (int i = 0; i < n_items; ++i) {
        if (done[i]) continue;
        const ecoflap_wanda_item& a = items[i];
        const bool vec = item_vector_ok(a, sq[i]);
        MatGroup g;
        g.n = 0;
        g.start[0] = 0;
        // the group's workgroups are shared out in proportion to the matrices' sizes (equal work
        // per workgroup: a ViT-g block's matrices differ 4x), WM_TOTAL_WGS over the launch
        int members[WMAX];
        int64_t total_elems = 0;
        for (int j = i; j < n_items; ++j) {
            const ecoflap_wanda_item& b = items[j];
            if (done[j] || b.dtype != a.dtype || item_vector_ok(b, sq[j]) != vec ||
                sampled_item[j] != sampled_item[i]) continue;
            members[g.n++] = j;
            total_elems += b.rows * b.cols;
            done[j] = true;
        }
        const int budget = WM_TOTAL_WGS;
        for (int q = 0; q < g.n; ++q) {
            const ecoflap_wanda_item& b = items[members[q]];
            const int64_t n = b.rows * b.cols;
            // >= 4 vectors per thread and pass
            int64_t cap = vec ? (n / (b.dtype == ECOFLAP_F32 ? 4 : 8) + 4 * WM_THREADS - 1) / (4 * WM_THREADS)
                              : (b.rows + 3) / 4;
            int64_t nb = (int64_t)((double)budget * (double)n / (double)total_elems + 0.5);
            if (nb > cap) nb = cap;
            if (nb < 1) nb = 1;
            g.w[q] = b.w; g.sq[q] = sq[members[q]]; g.rows[q] = b.rows; g.cols[q] = b.cols;
            g.rank0[q] = (uint32_t)(b.k + 1);     // sorted[k], 0-indexed -> (k+1)-th smallest
            g.st[q] = st[members[q]]; g.mask[q] = b.mask_out;
            g.start[q + 1] = g.start[q] + (int32_t)nb;
        }
        const dim3 grid((unsigned)g.start[g.n]), blk(WM_THREADS);
#define MATRIX_LEGACY(DT_, G_, GRID_)                                                               \
    do {                                                                                            \
        if (vec) {                                                                                  \
            hipLaunchKernelGGL((wanda_matrix_hist_kernel<DT_, 0, true, WM_SUB0>), GRID_, blk, 0, s, G_); \
            hipLaunchKernelGGL((wanda_matrix_hist_kernel<DT_, 1, true>), GRID_, blk, 0, s, G_);     \
            hipLaunchKernelGGL((wanda_matrix_hist_kernel<DT_, 2, true>), GRID_, blk, 0, s, G_);     \
            hipLaunchKernelGGL((wanda_matrix_apply_kernel<DT_, true>), GRID_, blk, 0, s, G_);       \
        } else {                                                                                    \
            hipLaunchKernelGGL((wanda_matrix_hist_kernel<DT_, 0, false>), GRID_, blk, 0, s, G_);    \
            hipLaunchKernelGGL((wanda_matrix_hist_kernel<DT_, 1, false>), GRID_, blk, 0, s, G_);    \
            hipLaunchKernelGGL((wanda_matrix_hist_kernel<DT_, 2, false>), GRID_, blk, 0, s, G_);    \
            hipLaunchKernelGGL((wanda_matrix_apply_kernel<DT_, false>), GRID_, blk, 0, s, G_);      \
        }                                                                                           \
    } while (0)
        // sampled bracket (2 reads + 1 write) when every matrix of the group is big enough to
        // sample one vector per stride; otherwise / on a flagged matrix the three histograms
        const bool sampled = sampled_item[i];
        if (!sampled) {
#define MATRIX_GO(DT_) MATRIX_LEGACY(DT_, g, grid)
            DT_SWITCH(a.dtype, MATRIX_GO);
#undef MATRIX_GO
            ECO_CHECK_LAUNCH();
            continue;
        }
        BracketGroup bg;
        bg.m = g;
        for (int q = 0; q < g.n; ++q) {
            bg.bs[q] = bst[members[q]];
            bg.sr[q] = items[members[q]].scaler_row;
        }
        if ((size_t)g.start[g.n] > (size_t)(WM_TOTAL_WGS + WMAX)) return ECOFLAP_ESIZE;   // (cannot happen: see nb)
#define MATRIX_GO(DT_)                                                                              \
    do {                                                                                            \
        hipLaunchKernelGGL((wanda_matrix_sbracket_kernel<DT_>), grid, blk, 0, s, bg, part);         \
        hipLaunchKernelGGL((wanda_matrix_apply2_kernel<DT_>), grid, blk, 0, s, bg, (const uint32_t*)part); \
    } while (0)
        DT_SWITCH(a.dtype, MATRIX_GO);
#undef MATRIX_GO
        ECO_CHECK_LAUNCH();
#undef MATRIX_LEGACY
    }
    return 0;
}
