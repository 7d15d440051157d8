// wanda_rows.h — K7 rows mode (T5/BERT, wanda_pruner.py:260, :272-279): the LDS form, the wave,
// workgroup and fused register forms with their two searches, and the launchers.  Everything here
// is a template on the dtype; wanda_rows_f32.hip, _f16.hip and _bf16.hip each instantiate one
// dtype's share (62 of the 186 kernels), so that the three compile side by side.  The fused
// instances stay in the unit of the wave and workgroup instances whose bodies they inline: in a
// unit of their own they came out identical, but the wave and workgroup kernels left behind did
// not (profiles/r16_wanda_split/README.md).
#pragma once
#include "wanda_k7.h"

// =====================================================================================
// K7 rows mode: one 256-thread workgroup per row; the row's metric bits live in LDS.
// =====================================================================================

template <int DT>
__global__ __launch_bounds__(256) void wanda_rows_kernel(void* w, const float* __restrict__ sq,
                                                         int64_t cols, int64_t k,
                                                         uint8_t* mask_out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    uint32_t* m = smem;                 // [cols] metric bits
    uint32_t* hist = smem + cols;       // [256]
    uint32_t* wave4 = hist + 256;       // [4]
    uint32_t* sel = wave4 + 4;          // [2] selected digit / remaining rank
    const int64_t row = blockIdx.x;
    void* wrow = (char*)w + row * cols * Vec<DT>::BYTES;
    const int tid = threadIdx.x;

    for (int64_t c = tid; c < cols; c += 256) m[c] = metric_bits<DT>(wrow, c, sq[c]);
    __syncthreads();

    // (k)-th smallest, 1-indexed, by 4 passes of 8-bit MSB-first radix select
    uint32_t prefix = 0, prefix_mask = 0;
    uint32_t remaining = (uint32_t)k;
    if (k > 0 && k < cols) {
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            hist[tid] = 0;
            __syncthreads();
            for (int64_t c = tid; c < cols; c += 256) {
                const uint32_t b = m[c];
                if ((b & prefix_mask) == prefix) atomicAdd(&hist[(b >> shift) & 255u], 1u);
            }
            __syncthreads();
            uint32_t total;
            const uint32_t cnt = hist[tid];
            const uint32_t incl = block_scan_256(cnt, wave4, total);
            const uint32_t excl = incl - cnt;
            if (excl < remaining && remaining <= incl) {  // exactly one thread
                sel[0] = (uint32_t)tid;
                sel[1] = remaining - excl;
            }
            __syncthreads();
            prefix |= sel[0] << shift;
            prefix_mask |= 255u << shift;
            remaining = sel[1];
            __syncthreads();
        }
    }
    // prefix = bits of the k-th smallest metric T; `remaining` of the elements equal to T are
    // pruned, lowest column first (stable sort order, W:272-277).
    if (k <= 0) return;
    const bool all = (k >= cols);
    // count of elements equal to T decides whether column order matters
    uint32_t running = 0;  // equal-to-T elements in columns before this 256-column tile
    for (int64_t c0 = 0; c0 < cols; c0 += 256) {
        const int64_t c = c0 + tid;
        const uint32_t b = (c < cols) ? m[c] : 0xffffffffu;
        const bool eq = !all && (c < cols) && (b == prefix);
        uint32_t total;
        const uint32_t incl = block_scan_256(eq ? 1u : 0u, wave4, total);
        const bool prune = (c < cols) && (all || b < prefix || (eq && (running + incl) <= remaining));
        if (prune) Vec<DT>::store1(wrow, c, 0.0f);
        if (mask_out && c < cols) mask_out[row * cols + c] = prune ? 1 : 0;
        running += total;
    }
}

// -------------------------------------------------------------------------------------
// K7 rows mode, register form (cols a multiple of the 16-byte vector): the row's metric
// bits live in registers (NV vectors per lane), W is read with 16-byte loads and written
// back once; the k-th smallest is found by a bitwise binary search on the bit pattern —
// per bit one compare-count over the lane's registers, a 64-wide shuffle reduction and one
// barrier (LDS only carries the four wave sums).  No atomics, no histogram.
// -------------------------------------------------------------------------------------
static __device__ __forceinline__ uint32_t block_count_256(uint32_t v, uint32_t* lds8, int phase) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    uint32_t* buf = lds8 + 4 * (phase & 1);     // double-buffered: one barrier per call
    if ((threadIdx.x & 63) == 0) buf[threadIdx.x >> 6] = v;
    __syncthreads();
    return buf[0] + buf[1] + buf[2] + buf[3];
}

// ---- helpers shared by the two register forms of the rows mode ----------------------------
// wave-wide inclusive prefix sum on the DPP network (row shifts inside the four 16-lane rows, then
// the two row broadcasts gfx9 has): 6 full-rate adds, no LDS crossbar; `total` = the wave's sum
// (uniform)
static __device__ __forceinline__ uint32_t wave_scan_dpp(uint32_t v, uint32_t& total) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xa, 0xf, true);   // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xc, 0xf, true);   // row_bcast:31
    total = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    return v;
}
// wave-wide sum: the scan's total
static __device__ __forceinline__ uint32_t wave_sum_dpp(uint32_t v) {
    uint32_t total;
    wave_scan_dpp(v, total);
    return total;
}

// pruned elements -> +0 on the stored bits themselves (kept elements are not re-encoded), and the
// row's uint8 mask bytes
template <int DT>
static __device__ __forceinline__ void zero_pruned(u32x4& wv, const bool* prune) {
    if (Vec<DT>::N == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wv[i] = prune[i] ? 0u : wv[i];
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            wv[q] &= (prune[2 * q] ? 0u : 0xffffu) | (prune[2 * q + 1] ? 0u : 0xffff0000u);
    }
}
// `m <= T` goes: the common ending of a row (no mask bytes wanted, no tie cut by column order).
// 16-bit dtypes: one compare and ONE sub-dword select per element — v_cndmask_b32_sdwa writes the
// element's half of the packed register and preserves the other (the compiler's form is compare,
// select, select, or, and per PAIR plus the bool bookkeeping: ~5 per element in the listing).
// Element halves are visited low halves first, high halves second: consecutive writes never
// touch the same register (the 16-bit-destination forwarding hazard of this ISA).
template <int DT>
static __device__ __forceinline__ void zero_le(u32x4& wv, const uint32_t* m, uint32_t T) {
    if constexpr (Vec<DT>::N == 4) {
#pragma unroll
        for (int i = 0; i < 4; ++i) wv[i] = m[i] <= T ? 0u : wv[i];
    } else {
        const uint32_t zero = 0u;
        uint32_t r0 = wv[0], r1 = wv[1], r2 = wv[2], r3 = wv[3];
#define ECO_SEL_LO(R_, M_) asm volatile("v_cmp_lt_u32 vcc, %2, %1\n\tv_cndmask_b32_sdwa %0, %3, %0, vcc dst_sel:WORD_0 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:WORD_0" : "+v"(R_) : "v"(M_), "s"(T), "v"(zero) : "vcc")
#define ECO_SEL_HI(R_, M_) asm volatile("v_cmp_lt_u32 vcc, %2, %1\n\tv_cndmask_b32_sdwa %0, %3, %0, vcc dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD src1_sel:WORD_1" : "+v"(R_) : "v"(M_), "s"(T), "v"(zero) : "vcc")
        ECO_SEL_LO(r0, m[0]); ECO_SEL_LO(r1, m[2]); ECO_SEL_LO(r2, m[4]); ECO_SEL_LO(r3, m[6]);
        ECO_SEL_HI(r0, m[1]); ECO_SEL_HI(r1, m[3]); ECO_SEL_HI(r2, m[5]); ECO_SEL_HI(r3, m[7]);
#undef ECO_SEL_LO
#undef ECO_SEL_HI
        wv[0] = r0; wv[1] = r1; wv[2] = r2; wv[3] = r3;
    }
}

template <int N>
static __device__ __forceinline__ void store_mask_bytes(uint8_t* mrow, const bool* prune) {
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i < 4) lo |= (prune[i] ? 1u : 0u) << (8 * i);
        else hi |= (prune[i] ? 1u : 0u) << (8 * (i - 4));
    }
    *(uint32_t*)mrow = lo;
    if (N == 8) *(uint32_t*)(mrow + 4) = hi;
}

// count of row elements below cand: per-lane compare + add-with-carry, one DPP reduction
template <int NV, int N>
static __device__ __forceinline__ uint32_t wave_count_less(const uint32_t (&m)[NV][N], uint32_t cand) {
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j)
#pragma unroll
        for (int i = 0; i < N; ++i) c += (m[j][i] < cand) ? 1u : 0u;
    return wave_sum_dpp(c);
}

// The rounds on bits 31..16 only look at the HIGH HALVES of the metrics (cand has no low bits
// there), two elements per register: hi16(x) >= c for both halves of a word with ONE subtraction,
//   d = (x | 0x80008000) - (c & 0x7fff) * 0x10001   (no borrow leaves a half; bit 15 / 31 of d is
//   set iff low15(x) >= low15(c));   c < 0x8000: x >= c <=> bit15(x | d);  else bit15(x & d),
// counted with v_bcnt: 3 instructions per two elements instead of 4 (compare + add-with-carry each,
// and the v_cmp -> carry-in hazard of this ISA costs a wait state per compare on top).
template <int NV, int N>
static __device__ __forceinline__ void gather_hi16(const uint32_t (&m)[NV][N], uint32_t (&x)[NV * N / 2]) {
#pragma unroll
    for (int w = 0; w < NV * N / 2; ++w) {
        const int e = 2 * w;
        // bytes [b.3 b.2 a.3 a.2]: element e in the low half, e+1 in the high half
        x[w] = __builtin_amdgcn_perm(m[(e + 1) / N][(e + 1) % N], m[e / N][e % N], 0x07060302u);
    }
}
template <int W, bool KEEP>
static __device__ __forceinline__ uint32_t wave_count_hi16_ge(const uint32_t (&x)[W], const uint32_t (&xg)[KEEP ? W : 1],
                                                              uint32_t c) {
    const uint32_t cl = (c & 0x7fffu) * 0x10001u;
    const uint32_t K = 0x80008000u;
    uint32_t cnt = 0;
    if (c & 0x8000u) {         // wave-uniform
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t d = (KEEP ? xg[KEEP ? w : 0] : (x[w] | K)) - cl;
            const uint32_t f = __builtin_amdgcn_bitop3_b32(d, x[w], K, 0x80);      // d & x & K
            asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(cnt) : "v"(f));
        }
    } else {
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t d = (KEEP ? xg[KEEP ? w : 0] : (x[w] | K)) - cl;
            const uint32_t f = __builtin_amdgcn_bitop3_b32(d, x[w], K, 0xa8);      // (d | x) & K
            asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(cnt) : "v"(f));
        }
    }
    return wave_sum_dpp(cnt);
}

// sum (or max) of one wave-uniform value per wave over the workgroup's four waves, result uniform:
// lane 0 of each wave writes its value, one barrier (double-buffered by call parity), four reads
static __device__ __forceinline__ uint32_t block_sum4(uint32_t wave_value, uint32_t* lds8, int phase,
                                                      int wave, int lane) {
    uint32_t* buf = lds8 + 4 * (phase & 1);
    if (lane == 0) buf[wave] = wave_value;
    __syncthreads();
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(buf[0] + buf[1] + buf[2] + buf[3]));
}
static __device__ __forceinline__ uint32_t block_max4(uint32_t wave_value, uint32_t* lds8, int phase,
                                                      int wave, int lane) {
    uint32_t* buf = lds8 + 4 * (phase & 1);
    if (lane == 0) buf[wave] = wave_value;
    __syncthreads();
    const uint32_t a = buf[0] > buf[1] ? buf[0] : buf[1], b = buf[2] > buf[3] ? buf[2] : buf[3];
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)(a > b ? a : b));
}

// ---- the k-th smallest by ONE histogram pass instead of a bisection (round 4) --------------
// profiles/r04_secondary/k7_rows_phases.md: of the ~41 VALU instructions per element of the
// bisection form, ~21 were the bisection itself (71 per probe and lane, 9-14 probes), 5 the
// compaction, 3 the low bits.  Here the top of the search costs 3 VALU + one LDS atomic per
// element: the metrics' bit patterns are binned RELATIVE TO THE ROW MAXIMUM,
//     bin = sat_sub(m, mx - (2^28 - 1)) >> 18          (1024 bins of 2^18 codes = 1/32 octave,
//                                                        32 octaves below the maximum; what lies
//                                                        further down shares bin 0)
// into an LDS histogram (ds_add_u32), the bin holding the k-th smallest is found by one scan
// (16 bins per lane + a wave prefix), and only that bin's elements (a few dozen of a 2048- or
// 5120-wide row) go on to the 18 low-bit rounds.  Exact: the bins partition the values in
// order, every count is a count of elements.  A bin with more than RH_CAND elements (massive
// ties) or a k-th smallest in the shared bin 0 takes the generic bit-by-bit search over all
// elements.
#define RH_BINS 1024
#define RH_SHIFT 18
#define RH_SPAN ((1u << 28) - 1u)         // RH_BINS << RH_SHIFT, minus one
#define RH_CAND 128                        // candidates one wave finishes (two per lane)

static __device__ __forceinline__ uint32_t rh_lowbound(uint32_t mx) { return mx > RH_SPAN ? mx - RH_SPAN : 0u; }
static __device__ __forceinline__ uint32_t rh_bin(uint32_t m, uint32_t lowbound) {
    return __builtin_elementwise_sub_sat(m, lowbound) >> RH_SHIFT;
}
// One wave scans the RH_BINS counters (lane l: bins [16 l, 16 l + 16)): the bin holding the k-th
// smallest (1-indexed), the number of elements in lower bins, and that bin's population — all
// wave-uniform.  The counters sum to >= k.
static __device__ __forceinline__ void rh_find(const uint32_t* hist, uint32_t k, int lane, uint32_t& bin,
                                               uint32_t& less_below, uint32_t& ncand) {
    constexpr int PER = RH_BINS / 64;
    uint32_t c[PER];
#pragma unroll
    for (int q = 0; q < PER / 4; ++q) {
        const u32x4 v = ((const u32x4*)hist)[lane * (PER / 4) + q];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[4 * q + i] = v[i];
    }
#pragma unroll
    for (int j = 1; j < PER; ++j) c[j] += c[j - 1];               // local inclusive sums
    uint32_t total;
    const uint32_t incl = wave_scan_dpp(c[PER - 1], total);
    const uint32_t P = incl - c[PER - 1];                        // elements in the lanes before
    const int32_t kk = (int32_t)k - (int32_t)P;                  // <= 0: the bin lies in an earlier lane
    uint32_t cnt = 0, below = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const bool lt = (int32_t)c[j] < kk;
        cnt += lt ? 1u : 0u;
        below = lt ? c[j] : below;
    }
    const uint64_t has = __ballot(incl >= k);                    // first lane whose range reaches k
    const int L = __builtin_ctzll(has);
    const uint32_t cntL = (uint32_t)__builtin_amdgcn_readlane((int)cnt, L);
    bin = (uint32_t)L * PER + cntL;
    less_below = (uint32_t)__builtin_amdgcn_readlane((int)(P + below), L);
    ncand = hist[bin];                                           // uniform address: broadcast read
    ncand = (uint32_t)__builtin_amdgcn_readfirstlane((int)ncand);
}

// One 256-thread workgroup per row (rows beyond the wave form's reach, and the long rows of a
// block whose short rows run in the wave form): the same search — bisection over the packed high
// halves, then the compacted bucket — with the per-probe count summed over the four waves through
// LDS (one barrier per probe).
template <int DT, int NV, bool HIST>
static __device__ __forceinline__ void rows_reg_body(const RowsGroup& g, int64_t grow, uint32_t* lds8,
                                                     uint32_t* wave4, uint32_t* cand_lds, uint32_t* res3,
                                                     uint32_t* hist) {
    constexpr int N = Vec<DT>::N;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int it = group_item(g, grow);
    const int64_t row = grow - g.start[it];
    const int64_t cols = g.cols[it], k = g.k[it];
    const float* __restrict__ sq = g.sq[it];
    uint8_t* mask_out = g.mask[it];
    const int64_t nvec = cols / N;
    void* wrow = (char*)g.w[it] + row * cols * Vec<DT>::BYTES;
    u32x4 wv[NV];
    uint32_t m[NV][N];
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (tid + 256 * j < nvec) wv[j] = ld16(wrow, tid + 256 * j);
    if constexpr (HIST) {                      // the row's histogram (+ the candidate counter behind it)
        const u32x4 zero = {0u, 0u, 0u, 0u};
        static_assert(RH_BINS == 1024, "one 16-byte clear per thread");
        ((u32x4*)hist)[tid] = zero;
        if (tid == 0) hist[RH_BINS] = 0u;
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = tid + 256 * j;
        if (v < nvec) {
            float f[N];
            Vec<DT>::unpack(wv[j], f);
#pragma unroll
            for (int q = 0; q < N / 4; ++q) {
                const u32x4 s4 = ld16(sq, v * (N / 4) + q);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    m[j][4 * q + i] = __float_as_uint(__builtin_fabsf(f[4 * q + i]) * __uint_as_float(s4[i]));
            }
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) m[j][i] = 0xffffffffu;   // padding: never among the k smallest
        }
    }
    const bool all = (k >= cols);
    uint32_t T = 0xffffffffu, take_equal = 0, total_equal = 0;
    int phase = 0;
    if (!all) {
        uint32_t mx = 0;
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (tid + 256 * j < nvec) {
#pragma unroll
                for (int i = 0; i < N; ++i) mx = m[j][i] > mx ? m[j][i] : mx;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_xor(mx, off, 64);
            mx = o > mx ? o : mx;
        }
        // (the barrier inside also orders the histogram's clears before the adds below)
        mx = block_max4((uint32_t)__builtin_amdgcn_readfirstlane((int)mx), lds8, phase++, wave, lane);
        uint32_t lo, less_below, ncand;        // the interval [lo, lo + 2^bits) holding the k-th smallest
        int bits;
        bool crowded;
        if constexpr (HIST) {
            const uint32_t lowbound = rh_lowbound(mx);
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (tid + 256 * j < nvec) {
#pragma unroll
                    for (int i = 0; i < N; ++i)
                        __hip_atomic_fetch_add(&hist[rh_bin(m[j][i], lowbound)], 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            __syncthreads();
            // every wave scans the counters for itself: the same uniform result in all four,
            // no second barrier to hand it round
            uint32_t bin;
            rh_find(hist, (uint32_t)k, lane, bin, less_below, ncand);
            if (bin == 0 && lowbound > 0) {
                lo = 0; bits = 32; less_below = 0; crowded = true;
            } else {
                lo = lowbound + (bin << RH_SHIFT); bits = RH_SHIFT; crowded = ncand > RH_CAND;
            }
        } else {
            const int top = mx ? 31 - __builtin_clz(mx) : -1;
            constexpr int WH = NV * N / 2;
            constexpr uint32_t ALL = 256 * NV * N;
            uint32_t xh[WH], xg[WH];
            gather_hi16(m, xh);
#pragma unroll
            for (int w = 0; w < WH; ++w) xg[w] = xh[w] | 0x80008000u;
            const uint32_t mx16 = mx >> 16;
            uint32_t blo = 0, flo = 0, bhi = 65536u, fhi = ALL;
            if (mx16 < 0xffffu) { bhi = mx16 + 1; fhi = (uint32_t)cols; }
            while (bhi - blo > 1) {
                const uint32_t mid = (blo + bhi) >> 1;
                const uint32_t fm = ALL - block_sum4(wave_count_hi16_ge<WH, true>(xh, xg, mid), lds8, phase++, wave, lane);
                if (fm < (uint32_t)k) { blo = mid; flo = fm; } else { bhi = mid; fhi = fm; }
            }
            lo = blo << 16;
            less_below = flo;
            ncand = fhi - flo;
            bits = (top < 15 ? top : 15) + 1;
            crowded = ncand > RH_CAND;
        }
        if (!crowded) {                                   // block-uniform
            // compact the interval's elements; ONE wave finishes the low bits on them with
            // ballots — `bits` rounds without a block barrier or a pass over the registers
            const uint32_t span = 1u << bits;
            if constexpr (HIST) {
                // order among the candidates does not matter: a counter hands out the slots
#pragma unroll
                for (int j = 0; j < NV; ++j)
#pragma unroll
                    for (int i = 0; i < N; ++i) {
                        const uint32_t rel = m[j][i] - lo;
                        if (rel < span) {
                            const uint32_t p_ = __hip_atomic_fetch_add(&hist[RH_BINS], 1u, __ATOMIC_RELAXED,
                                                                       __HIP_MEMORY_SCOPE_WORKGROUP);
                            cand_lds[p_] = rel;
                        }
                    }
            } else {
                uint32_t mine = 0;
#pragma unroll
                for (int j = 0; j < NV; ++j)
#pragma unroll
                    for (int i = 0; i < N; ++i) mine += ((m[j][i] - lo) < span) ? 1u : 0u;
                uint32_t total;
                uint32_t pos = block_scan_256(mine, wave4, total) - mine;
                if (mine) {
#pragma unroll
                    for (int j = 0; j < NV; ++j)
#pragma unroll
                        for (int i = 0; i < N; ++i)
                            if ((m[j][i] - lo) < span) cand_lds[pos++] = m[j][i] - lo;
                }
            }
            __syncthreads();
            if (wave == 0) {
                const bool v0 = (uint32_t)lane < ncand, v1 = (uint32_t)lane + 64 < ncand;
                const uint32_t c0 = v0 ? cand_lds[lane] : 0u, c1 = v1 ? cand_lds[lane + 64] : 0u;
                uint32_t off = 0;
                for (int bit = bits - 1; bit >= 0; --bit) {
                    const uint32_t cand = off | (1u << bit);
                    const uint32_t c = less_below + (uint32_t)__popcll(__ballot(v0 && c0 < cand)) +
                                       (uint32_t)__popcll(__ballot(v1 && c1 < cand));
                    if (c < (uint32_t)k) off = cand;
                }
                const uint32_t less = less_below + (uint32_t)__popcll(__ballot(v0 && c0 < off)) +
                                      (uint32_t)__popcll(__ballot(v1 && c1 < off));
                const uint32_t eq = (uint32_t)__popcll(__ballot(v0 && c0 == off)) +
                                    (uint32_t)__popcll(__ballot(v1 && c1 == off));
                if (lane == 0) { res3[0] = lo + off; res3[1] = less; res3[2] = eq; }
            }
            __syncthreads();
            T = (uint32_t)__builtin_amdgcn_readfirstlane((int)res3[0]);
            total_equal = (uint32_t)__builtin_amdgcn_readfirstlane((int)res3[2]);
            take_equal = (uint32_t)k - (uint32_t)__builtin_amdgcn_readfirstlane((int)res3[1]);
        } else {                                          // crowded interval: all elements, bit by bit
            uint32_t less = less_below, off = 0;
            for (int bit = bits - 1; bit >= 0; --bit) {
                const uint32_t cand = lo + (off | (1u << bit));
                const uint32_t c = block_sum4(wave_count_less(m, cand), lds8, phase++, wave, lane);
                if (c < (uint32_t)k) { off |= 1u << bit; less = c; }
            }
            T = lo + off;
            uint32_t eq = 0;
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int i = 0; i < N; ++i) eq += (m[j][i] == T) ? 1u : 0u;
            total_equal = block_sum4(wave_sum_dpp(eq), lds8, phase++, wave, lane);
            take_equal = (uint32_t)k - less;
        }
    }
    const bool ordered = !all && (take_equal < total_equal);   // ties cut by column order
    if (!ordered) {
        const uint32_t Tq = all ? 0xffffffffu : T;
        if (!mask_out) {                       // block-uniform: the production call
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int64_t v = tid + 256 * j;
                if (v < nvec) {
                    zero_le<DT>(wv[j], m[j], Tq);
                    st16(wrow, v, wv[j]);
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t v = tid + 256 * j;
            if (v < nvec) {
                bool prune[N];
#pragma unroll
                for (int i = 0; i < N; ++i) prune[i] = m[j][i] <= Tq;
                zero_pruned<DT>(wv[j], prune);
                st16(wrow, v, wv[j]);
                store_mask_bytes<N>(mask_out + row * cols + v * N, prune);
            }
        }
        return;
    }
    uint32_t running = 0;
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = tid + 256 * j;
        // block-uniform branch: equal-to-T elements in lower columns come first
        uint32_t mine = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) mine += (m[j][i] == T) ? 1u : 0u;
        uint32_t total;
        const uint32_t incl = block_scan_256(mine, wave4, total);
        const uint32_t rank0 = running + incl - mine;
        running += total;
        if (v < nvec) {
            bool prune[N];
            uint32_t seen = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const bool eqT = (m[j][i] == T);
                prune[i] = (m[j][i] < T) || (eqT && (rank0 + seen) < take_equal);
                seen += eqT ? 1u : 0u;
            }
            zero_pruned<DT>(wv[j], prune);
            st16(wrow, v, wv[j]);
            if (mask_out) store_mask_bytes<N>(mask_out + row * cols + v * N, prune);
        }
    }
}

template <int DT, int NV, bool HIST>
__global__ __launch_bounds__(256) void wanda_rows_reg_kernel(const RowsGroup g) {
    __shared__ uint32_t lds8[8];
    __shared__ uint32_t wave4[4];
    __shared__ uint32_t cand_lds[RH_CAND];
    __shared__ uint32_t res3[3];
    __shared__ __attribute__((aligned(16))) uint32_t hist[HIST ? RH_BINS + 4 : 4];
    rows_reg_body<DT, NV, HIST>(g, blockIdx.x, lds8, wave4, cand_lds, res3, hist);
}

// -------------------------------------------------------------------------------------
// K7 rows mode, wave form (rows of up to 64*12 vectors): ONE 64-lane wave per row, four rows
// per workgroup — the search needs no LDS traffic and no barrier at all.
// -------------------------------------------------------------------------------------
// One 64-lane wave per row, four rows per workgroup.  (Tried and measured slower on MI355X: a
// persistent wave walking a run of rows with the next row's loads in flight during the search —
// all waves then load, search and store in phase and the memory and VALU phases stop overlapping
// across waves; seeding the search from the previous row's threshold through a word in the
// workspace — loads of many waves from one address serialise like atomics, ~30 ns each.)
// FULL: every row of the launch has exactly 64 * NV vectors (FlanT5's 2048-wide rows in bf16):
// no padding values, no bounds tests (the padding's defaults alone were 61 register moves).
template <int DT, int NV, bool HIST, bool FULL = false>
static __device__ __forceinline__ void rows_wave_body(const RowsGroup& g, int64_t first_row,
                                                      uint32_t (*cand_lds_all)[64 * 2],
                                                      uint32_t (*hist_all)[RH_BINS]) {
    constexpr int N = Vec<DT>::N;
    const int lane = threadIdx.x & 63;
    // (the wave index is uniform, which the compiler cannot see through threadIdx: without the
    // readfirstlane every per-row scalar — item, k, cols, the search bounds — lives in VGPRs)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t grow = first_row + wave;
    if (grow >= g.start[g.n]) return;          // whole wave leaves together
    const int it = group_item(g, grow);
    const int64_t row = grow - g.start[it];
    const int64_t cols = g.cols[it], k = g.k[it];
    const float* __restrict__ sq = g.sq[it];
    uint8_t* mask_out = g.mask[it];
    const int64_t nvec = cols / N;
    void* wrow = (char*)g.w[it] + row * cols * Vec<DT>::BYTES;
    uint32_t* cand_lds = cand_lds_all[wave];
    u32x4 wv[NV];
    uint32_t m[NV][N];
#pragma unroll
    for (int j = 0; j < NV; ++j)
        if (FULL || lane + 64 * j < nvec) wv[j] = ld16(wrow, lane + 64 * j);
    if constexpr (HIST) {                      // the wave's histogram, cleared while the loads fly
        const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int q = 0; q < RH_BINS / 256; ++q) ((u32x4*)hist_all[wave])[lane + 64 * q] = zero;
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = lane + 64 * j;
        if (FULL || v < nvec) {
            float f[N];
            Vec<DT>::unpack(wv[j], f);
#pragma unroll
            for (int q = 0; q < N / 4; ++q) {
                const u32x4 s4 = ld16(sq, v * (N / 4) + q);
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    m[j][4 * q + i] = __float_as_uint(__builtin_fabsf(f[4 * q + i]) * __uint_as_float(s4[i]));
            }
        } else {
#pragma unroll
            for (int i = 0; i < N; ++i) m[j][i] = 0xffffffffu;
        }
    }
    const bool all = (k >= cols);
    uint32_t T = 0xffffffffu, take_equal = 0, total_equal = 0;
    if (!all) {
        // k-th smallest (1-indexed) = largest T with #(m < T) < k.  First an interval
        // [lo, lo + 2^bits) that holds it, with the number of elements below it — from the
        // histogram of the metrics relative to the row maximum (HIST) or from a bisection over the
        // packed high halves —; then only the elements inside the interval (typically ~1 % of a
        // row) can still change a count: they are compacted to at most two per lane and the low
        // bits are found bit by bit with 2 ballots per round instead of a pass over the row.
        uint32_t mx = 0;
#pragma unroll
        for (int j = 0; j < NV; ++j)
            if (FULL || lane + 64 * j < nvec) {
#pragma unroll
                for (int i = 0; i < N; ++i) mx = m[j][i] > mx ? m[j][i] : mx;
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t o = __shfl_xor(mx, off, 64);
            mx = o > mx ? o : mx;
        }
        mx = (uint32_t)__builtin_amdgcn_readfirstlane((int)mx);      // uniform: scalar loop control
        uint32_t lo, less_below, ncand;        // less_below = #(m < lo), ncand = population of the interval
        int bits;
        bool crowded;
        if constexpr (HIST) {
            uint32_t* hist = hist_all[wave];
            const uint32_t lowbound = rh_lowbound(mx);
#pragma unroll
            for (int j = 0; j < NV; ++j)
                if (FULL || lane + 64 * j < nvec) {      // (padding must not be binned: it lies above mx)
#pragma unroll
                    for (int i = 0; i < N; ++i)
                        __hip_atomic_fetch_add(&hist[rh_bin(m[j][i], lowbound)], 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            // (one wave's LDS operations are performed in issue order: the clears above, these
            // adds and the reads of the scan need no barrier between them)
            uint32_t bin;
            rh_find(hist, (uint32_t)k, lane, bin, less_below, ncand);
            if (bin == 0 && lowbound > 0) {      // k-th smallest more than 32 octaves below the maximum
                lo = 0; bits = 32; less_below = 0; crowded = true;
            } else {
                lo = lowbound + (bin << RH_SHIFT); bits = RH_SHIFT; crowded = ncand > RH_CAND;
            }
        } else {
            const int top = mx ? 31 - __builtin_clz(mx) : -1;
            constexpr int WH = NV * N / 2;
            constexpr bool KEEPG = NV <= 4;
            constexpr uint32_t ALL = 64 * NV * N;              // padding (0xffff....) is never "less"
            uint32_t xh[WH], xg[KEEPG ? WH : 1];
            gather_hi16(m, xh);
            if (KEEPG) {
#pragma unroll
                for (int w = 0; w < WH; ++w) xg[KEEPG ? w : 0] = xh[w] | 0x80008000u;
            }
            // f(c) = #(hi16(m) < c) is monotone; wanted: p16 = max{c : f(c) < k}.  Bisection on
            // [lo, hi] with f(lo) < k <= f(hi); the last two values give the bucket's population
            const uint32_t mx16 = mx >> 16;
            uint32_t blo = 0, flo = 0, bhi = 65536u, fhi = ALL;
            if (mx16 < 0xffffu) { bhi = mx16 + 1; fhi = (uint32_t)cols; }   // every real element is below
            while (bhi - blo > 1) {
                const uint32_t mid = (blo + bhi) >> 1;
                const uint32_t fm = ALL - wave_count_hi16_ge<WH, KEEPG>(xh, xg, mid);
                if (fm < (uint32_t)k) { blo = mid; flo = fm; } else { bhi = mid; fhi = fm; }
            }
            lo = blo << 16;
            less_below = flo;
            ncand = fhi - flo;
            bits = (top < 15 ? top : 15) + 1;
            crowded = ncand > RH_CAND;
        }
        constexpr uint32_t CMAX = 2;             // candidates per lane (RH_CAND = 64 * CMAX)
        if (!crowded) {                          // wave-uniform
            const uint32_t span = 1u << bits;    // (bits <= 18 here)
            // (tried: a counter handing out the slots, `cand[atomicAdd(counter, 1)] = rel` under the
            // lanes' own branch — the compiler turns it into a wave-aggregated atomic, 11 VALU per
            // element slot with a hit against 6 for the ballot form below, plus an LDS round trip)
            uint32_t pos = 0;
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    const uint32_t rel = m[j][i] - lo;
                    const bool hit = rel < span;
                    const uint64_t mask = __ballot(hit);
                    if (mask) {                  // wave-uniform: a third of the element slots have no candidate
                        if (hit) cand_lds[pos + __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u))] = rel;
                        pos += (uint32_t)__popcll(mask);
                    }
                }
            // (same wave wrote and reads: program order, no barrier needed on one SIMD)
            __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): LDS writes done
            uint32_t cr[CMAX];
            bool cv[CMAX];
#pragma unroll
            for (uint32_t c = 0; c < CMAX; ++c) {
                cv[c] = lane + 64 * c < ncand;
                cr[c] = cv[c] ? cand_lds[lane + 64 * c] : 0u;
            }
            uint32_t off = 0;                    // T = lo + off
            for (int bit = bits - 1; bit >= 0; --bit) {
                const uint32_t cand = off | (1u << bit);
                uint32_t c = less_below;
#pragma unroll
                for (uint32_t q = 0; q < CMAX; ++q) c += (uint32_t)__popcll(__ballot(cv[q] && cr[q] < cand));
                if (c < (uint32_t)k) off = cand;
            }
            T = lo + off;
            uint32_t less = less_below;
#pragma unroll
            for (uint32_t q = 0; q < CMAX; ++q) {
                less += (uint32_t)__popcll(__ballot(cv[q] && cr[q] < off));
                total_equal += (uint32_t)__popcll(__ballot(cv[q] && cr[q] == off));
            }
            take_equal = (uint32_t)k - less;
        } else {                                 // crowded interval (few distinct values): all elements
            uint32_t less = less_below, off = 0;
            for (int bit = bits - 1; bit >= 0; --bit) {
                const uint32_t cand = lo + (off | (1u << bit));
                const uint32_t c = wave_count_less(m, cand);
                if (c < (uint32_t)k) { off |= 1u << bit; less = c; }
            }
            T = lo + off;
#pragma unroll
            for (int j = 0; j < NV; ++j)
#pragma unroll
                for (int i = 0; i < N; ++i)
                    total_equal += (uint32_t)__popcll(__ballot(m[j][i] == T));
            take_equal = (uint32_t)k - less;
        }
    }
    const bool ordered = !all && (take_equal < total_equal);
    if (!ordered) {
        // every element equal to T goes (or, with k >= cols, every element): prune = m <= T
        const uint32_t Tq = all ? 0xffffffffu : T;
        if (!mask_out) {                       // wave-uniform: the production call
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                const int64_t v = lane + 64 * j;
                if (FULL || v < nvec) {
                    zero_le<DT>(wv[j], m[j], Tq);
                    st16(wrow, v, wv[j]);
                }
            }
            return;
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const int64_t v = lane + 64 * j;
            if (FULL || v < nvec) {
                bool prune[N];
#pragma unroll
                for (int i = 0; i < N; ++i) prune[i] = m[j][i] <= Tq;
                zero_pruned<DT>(wv[j], prune);
                st16(wrow, v, wv[j]);
                store_mask_bytes<N>(mask_out + row * cols + v * N, prune);
            }
        }
        return;
    }
    uint32_t running = 0;                      // ties cut by column order
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int64_t v = lane + 64 * j;
        uint32_t mine = 0;
#pragma unroll
        for (int i = 0; i < N; ++i) mine += (m[j][i] == T) ? 1u : 0u;
        uint32_t x = mine;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(x, off, 64);
            if (lane >= off) x += y;
        }
        const uint32_t rank0 = running + x - mine;
        running += __shfl(x, 63, 64);
        if (v < nvec) {
            bool prune[N];
            uint32_t seen = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const bool eqT = (m[j][i] == T);
                prune[i] = (m[j][i] < T) || (eqT && (rank0 + seen) < take_equal);
                seen += eqT ? 1u : 0u;
            }
            zero_pruned<DT>(wv[j], prune);
            st16(wrow, v, wv[j]);
            if (mask_out) store_mask_bytes<N>(mask_out + row * cols + v * N, prune);
        }
    }
}

template <int DT, int NV, bool HIST, bool FULL>
__global__ __launch_bounds__(256, 4) void wanda_rows_wave_kernel(const RowsGroup g) {
    __shared__ uint32_t cand_lds_all[4][64 * 2];
    __shared__ __attribute__((aligned(16))) uint32_t hist_all[HIST ? 4 : 1][RH_BINS];
    rows_wave_body<DT, NV, HIST, FULL>(g, (int64_t)blockIdx.x * 4, cand_lds_all, hist_all);
}

// A block's short rows (wave form) and long rows (workgroup form) in ONE grid: the long rows of a
// T5 block (2048 rows of 5120 columns) are too few to fill the chip in a launch of their own
// (measured: 33 us for 22 % of the block's bytes, after the 58 us of the other 78 %), and launches
// on one stream do not overlap; side streams joined by events cost more than they gave.  The
// long-row workgroups come first in the grid so that they are not the tail.
template <int DT, int NVW, int NVR, bool HIST, bool FULL>
__global__ __launch_bounds__(256, 4) void wanda_rows_fused_kernel(const RowsGroup gw, const RowsGroup gr) {
    __shared__ uint32_t cand_lds_all[4][64 * 2];      // wave form: 2 candidates per lane and wave
    __shared__ uint32_t lds8[8];
    __shared__ uint32_t wave4[4];
    __shared__ uint32_t res3[4];
    // wave form: one histogram per wave; workgroup form: the first one (+ its counter in res3's
    // neighbour would alias: the counter lives behind the LAST histogram instead)
    __shared__ __attribute__((aligned(16))) uint32_t hist_all[HIST ? 4 : 1][RH_BINS];
    const int64_t n_long = gr.start[gr.n];
    if ((int64_t)blockIdx.x < n_long)
        rows_reg_body<DT, NVR, HIST>(gr, blockIdx.x, lds8, wave4, &cand_lds_all[0][0], res3, &hist_all[0][0]);
    else
        rows_wave_body<DT, NVW, HIST, FULL>(gw, ((int64_t)blockIdx.x - n_long) * 4, cand_lds_all, hist_all);
}

// Which search the rows kernels run: the histogram form (default) or the bisection form of
// rounds 2-3 (ECOFLAP_WANDA_ROWS_SEARCH=bisect: A/B measurements and the parity tests, which run
// both against the oracle).  Read per call: cheap, and a test can flip it inside one process.
static inline bool rows_search_hist() {
    const char* e = getenv("ECOFLAP_WANDA_ROWS_SEARCH");
    return !(e && e[0] == 'b');
}

// every row of the group exactly 64 * nv vectors wide (no padding lanes)?
template <int DT>
static inline bool rows_group_full(const RowsGroup& g, int nv) {
    for (int i = 0; i < g.n; ++i)
        if (g.cols[i] != (int64_t)64 * nv * Vec<DT>::N) return false;
    return true;
}

template <int DT, bool HIST, bool FULL>
static void launch_rows_wave_t(const RowsGroup& g, int nv, hipStream_t s) {
    const dim3 grid((unsigned)((g.start[g.n] + 3) / 4)), blk(256);
    if (nv == 1) hipLaunchKernelGGL((wanda_rows_wave_kernel<DT, 1, HIST, FULL>), grid, blk, 0, s, g);
    else if (nv == 2) hipLaunchKernelGGL((wanda_rows_wave_kernel<DT, 2, HIST, FULL>), grid, blk, 0, s, g);
    else hipLaunchKernelGGL((wanda_rows_wave_kernel<DT, 4, HIST, FULL>), grid, blk, 0, s, g);
}
template <int DT>
static void launch_rows_wave(const RowsGroup& g, int nv, hipStream_t s) {
    const bool full = rows_group_full<DT>(g, nv);
    if (rows_search_hist()) {
        if (full) launch_rows_wave_t<DT, true, true>(g, nv, s);
        else launch_rows_wave_t<DT, true, false>(g, nv, s);
    } else {
        launch_rows_wave_t<DT, false, false>(g, nv, s);
    }
}

template <int DT, bool HIST, bool FULL>
static void launch_rows_fused_t(const RowsGroup& gw, int nvw, const RowsGroup& gr, int nvr, hipStream_t s) {
    const dim3 grid((unsigned)(gr.start[gr.n] + (gw.start[gw.n] + 3) / 4)), blk(256);
#define FUSED(W_, R_) hipLaunchKernelGGL((wanda_rows_fused_kernel<DT, W_, R_, HIST, FULL>), grid, blk, 0, s, gw, gr)
#define FUSED_R(W_)                                                          \
    do {                                                                     \
        if (nvr == 1) FUSED(W_, 1); else if (nvr == 2) FUSED(W_, 2);         \
        else if (nvr == 3) FUSED(W_, 3); else FUSED(W_, 4);                  \
    } while (0)
    if (nvw == 1) FUSED_R(1); else if (nvw == 2) FUSED_R(2); else FUSED_R(4);
#undef FUSED_R
#undef FUSED
}
template <int DT>
static void launch_rows_fused(const RowsGroup& gw, int nvw, const RowsGroup& gr, int nvr, hipStream_t s) {
    const bool full = rows_group_full<DT>(gw, nvw);
    if (rows_search_hist()) {
        if (full) launch_rows_fused_t<DT, true, true>(gw, nvw, gr, nvr, s);
        else launch_rows_fused_t<DT, true, false>(gw, nvw, gr, nvr, s);
    } else {
        launch_rows_fused_t<DT, false, false>(gw, nvw, gr, nvr, s);
    }
}

template <int DT, bool HIST>
static void launch_rows_reg_t(const RowsGroup& g, int nv, hipStream_t s) {
    const dim3 grid((unsigned)g.start[g.n]), blk(256);
#define ROWS_REG(NV_) hipLaunchKernelGGL((wanda_rows_reg_kernel<DT, NV_, HIST>), grid, blk, 0, s, g)
    switch (nv) {
        case 1: ROWS_REG(1); break;
        case 2: ROWS_REG(2); break;
        case 3: ROWS_REG(3); break;
        case 4: ROWS_REG(4); break;
        case 6: ROWS_REG(6); break;
        case 8: ROWS_REG(8); break;
        case 12: ROWS_REG(12); break;
        default: ROWS_REG(16); break;
    }
#undef ROWS_REG
}
template <int DT>
static void launch_rows_reg(const RowsGroup& g, int nv, hipStream_t s) {
    if (rows_search_hist()) launch_rows_reg_t<DT, true>(g, nv, s);
    else launch_rows_reg_t<DT, false>(g, nv, s);
}

// ---- one dtype's instances behind the plain interface of wanda_k7.h ------------------------------
// (the LDS form: odd widths / unaligned views, per matrix)
#define WANDA_ROWS_UNIT(DT_, SUFFIX_)                                                                   \
    void wanda_rows_launch_##SUFFIX_(bool wave, const RowsGroup& g, int cls, hipStream_t s) {          \
        if (wave) launch_rows_wave<DT_>(g, cls, s);                                                    \
        else launch_rows_reg<DT_>(g, cls, s);                                                          \
    }                                                                                                   \
    void wanda_rows_lds_launch_##SUFFIX_(void* w, const float* sq, int64_t rows, int64_t cols,         \
                                         int64_t k, uint8_t* mask_out, hipStream_t s) {                \
        const size_t lds = ((size_t)cols + 256 + 4 + 4) * sizeof(uint32_t);                            \
        hipLaunchKernelGGL((wanda_rows_kernel<DT_>), dim3((unsigned)rows), dim3(256), lds, s, w, sq,   \
                           cols, k, mask_out);                                                         \
    }                                                                                                   \
    void wanda_rows_fused_launch_##SUFFIX_(const RowsGroup& gw, int cls_w, const RowsGroup& gr,        \
                                           int cls_r, hipStream_t s) {                                 \
        launch_rows_fused<DT_>(gw, cls_w, gr, cls_r, s);                                               \
    }
