// attention.hip — multi-head self-attention of the EVA ViT-g blocks for gfx950 (plumbing for the
// build's shape modules, include/ecoflap_shape_ops.h; not part of the pruner ABI).
//
// The zeroth-order loop is forward-bound, and the library's fused attention runs the ViT-g shape
// (257 tokens, 16 heads of 88) at 67 TFLOP/s: 0.7 ms per block at 16 concatenated evaluations, a
// sixth of a ViT-g matrix's step.  This kernel serves exactly that shape family (N <= 288 tokens,
// head width <= 96, fp16, no mask, no dropout):
//
//   * one persistent workgroup per CU walks the (image, head) items; the head's K [N, D] and V
//     [N, D] live in LDS for the whole workgroup (K rows at a 16*odd-byte pitch: every
//     ds_read_b128 of 16 consecutive rows covers all 64 banks once; V rows at 192 bytes);
//   * production schedule (vit_attention_kernel, below): 8 waves, two per SIMD, one query tile
//     each; the waves done with their tile fetch the next item; small batches split an item's
//     tiles over several workgroups; one XCD runs whole images.  The previous schedule (4 waves,
//     vit_attention_v1_kernel) stays as the reference of the bitwise tests;
//   * a wave takes 32 queries at a time; the tile's arithmetic is attention_tile.h's (one routine
//     for this file and mha_attention.hip), here with 9 key tiles, 6 head-dimension chunks, a
//     run-time head width and K pitch, and double-buffered V fragments: S^T = K Q^T by
//     v_mfma_f32_32x32x16_f16 (queries on the lanes, keys in the registers: a query's softmax
//     is a per-lane loop plus one exchange with lane ^ 32), all N scores of the tile in
//     registers, exact two-pass softmax in fp32, O^T = V^T P^T with the P tile straight from
//     those registers and V^T fragments by ds_read_b64_tr_b16 from the row-major V image;
//   * reads qkv as the qkv Linear wrote it ([B, N, 3, H, D]) and writes [B, N, H*D]: no permute /
//     contiguous copies around it.
// Per (image, head) independent: batch invariant by construction.
#include <stdlib.h>

#include "attention_tile.h"
#include "../../include/ecoflap_shape_ops.h"

#define AT_NT 9                 // tiles of 32 keys / queries (N <= 288)
#define AT_ROWS (AT_NT * 32)
#define AT_DC 6                 // 16-wide chunks of the head dimension (D <= 96)
#define AT_DT 3                 // 32-wide tiles of the head dimension
#define AT_KPITCH_MAX 208       // bytes per K row in LDS: 2*D rounded up to 16 * odd
#define AT_KBYTES 46080         // one K image: N * kpitch (257 * 176 = 45232)
#define AT_PF 15                // 16-byte vectors of K and of V a prefetching thread holds (v1)

struct AttnArgs {
    const _Float16* qkv;        // [B, N, 3, H, D]
    _Float16* out;              // [B, N, H * D]
    int B, N, H, D;
    int kpitch;                 // bytes
    float scale_log2e;          // softmax scale * log2(e)
    int debug;                  // ablation switches for tools/attention_launches.py (0 in production)
};

// One 32-query tile of one (image, head); `base`: q of (b, token 0, h).  The V fragments are
// double-buffered (attention_tile.h: PREFETCH_V).
static __device__ __forceinline__ void attn_tile(const AttnArgs& a, const unsigned char* Ks,
                                                 const unsigned char* Vs, const _Float16* base,
                                                 int64_t row_stride, int b, int h, int qt, int lane) {
    attention_tile<AT_NT, AT_DC, AT_DT, false, true>(
        Ks, Vs, a.kpitch, base, row_stride, a.out + ((int64_t)b * a.N * a.H + h) * a.D,
        (int64_t)a.H * a.D, a.N, a.D, a.scale_log2e, a.debug, qt, lane);
}

// vectors fi, fi + step, ... of one head's K or V rows (`off`: H*D for K, 2*H*D for V), clamped
template <int NV>
static __device__ __forceinline__ void at_gather(u32x4 (&r)[NV], const _Float16* nb, int64_t row_stride,
                                                 int64_t off, int fi, int step, int total, int vpr) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int v0 = fi + step * j;
        const int v = v0 < total ? v0 : total - 1;
        const int key = v / vpr, c = v - key * vpr;
        r[j] = *(const u32x4*)(nb + (int64_t)key * row_stride + 8 * c + off);
    }
}

template <int NV>
static __device__ __forceinline__ void at_scatter(const u32x4 (&r)[NV], unsigned char* dst, int pitch,
                                                  int fi, int step, int total, int vpr) {
#pragma unroll
    for (int j = 0; j < NV; ++j) {
        const int v = fi + step * j;
        if (v < total) {
            const int key = v / vpr, c = v - key * vpr;
            *(u32x4*)(dst + key * pitch + 16 * c) = r[j];
        }
    }
}

// K by LDS DMA straight into the idle buffer `Kn`, no registers: a K image without row padding is
// contiguous (vector v of the head lives at byte 16 v), so a wave's 64 consecutive vectors are
// one 1-KiB piece at a wave-uniform LDS address.  This wave moves pieces blk0, blk0 + step, ...
static __device__ __forceinline__ void at_dma_k(unsigned char* Kn, const _Float16* nb, int64_t row_stride,
                                                int64_t off, int blk0, int step, int lane, int total, int vpr) {
    for (int blk = blk0; 64 * blk < total; blk += step) {
        const int v0 = 64 * blk + lane;
        const int v = v0 < total ? v0 : total - 1;
        const int key = v / vpr, c = v - key * vpr;
        const _Float16* src = nb + (int64_t)key * row_stride + 8 * c + off;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)(Kn + 1024 * blk), 16, 0, 0);
    }
}

// The previous schedule, kept as the reference of the bitwise tests.  PERSISTENT workgroups (one
// per CU: the LDS image allows no second one) walk the (image, head) items.  A head has
// ceil(N / 32) query tiles for 4 waves; in the last round of tiles the waves WITHOUT a tile (three
// of four at N = 257) fetch the NEXT item while the others finish: its K goes straight into the
// second K buffer in LDS (nobody reads that one), its V waits in registers until everybody is
// done with the current V image.  The fill's memory latency hides under the last tile instead of
// standing alone in front of every item.
__global__ __launch_bounds__(256) void vit_attention_v1_kernel(const AttnArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char Kb[2 * AT_KBYTES];
    __shared__ __attribute__((aligned(16))) unsigned char Vs[AT_ROWS * AT_VPITCH];
    const int N = a.N, D = a.D, H = a.H, kpitch = a.kpitch;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branches on it are uniform
    const int64_t row_stride = (int64_t)3 * H * D;
    const int nt = (N + 31) >> 5;
    const int nitems = a.B * H;
    const int vpr = D >> 3, total = N * vpr;
    const int rounds = (nt + 3) >> 2;
    const int busy_last = nt - 4 * (rounds - 1);               // waves with a tile in the last round
    const int nfree = 4 - busy_last;
    const bool overlap = nfree > 0 && (total + 64 * nfree - 1) / (64 * nfree) <= AT_PF;
    const bool dma = kpitch == 2 * D && ((total + 63) >> 6) * 1024 <= AT_KBYTES;
    at_zero_v_tail(Vs, N, AT_ROWS, tid, 256);                  // N is the same for every item: once
    auto head_base = [&](int item) {
        return a.qkv + (int64_t)(item / H) * N * row_stride + (int64_t)(item % H) * D;
    };
    // all threads: K and V of `item` into LDS (the loads of a round in flight together)
    auto fill_all = [&](int item, unsigned char* kdst) {
        const _Float16* nb = head_base(item);
        for (int f0 = tid; f0 < total; f0 += 256 * 6) {
            u32x4 kk[6], vv[6];
            at_gather(kk, nb, row_stride, (int64_t)H * D, f0, 256, total, vpr);
            at_gather(vv, nb, row_stride, (int64_t)2 * H * D, f0, 256, total, vpr);
            at_scatter(kk, kdst, kpitch, f0, 256, total, vpr);
            at_scatter(vv, Vs, AT_VPITCH, f0, 256, total, vpr);
        }
    };
    if ((int)blockIdx.x < nitems && !(a.debug & 1)) fill_all((int)blockIdx.x, Kb);
    __syncthreads();
    int cur = 0;
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        const int b = item / H, h = item % H;
        const _Float16* base = head_base(item);
        const unsigned char* Ks = Kb + cur * AT_KBYTES;
        unsigned char* Kn = Kb + (cur ^ 1) * AT_KBYTES;
        const int next = item + (int)gridDim.x;
        const bool has_next = next < nitems && !(a.debug & 1);
        u32x4 pv[AT_PF];
        const int fi = (wave - busy_last) * 64 + lane;         // index among the prefetching threads
        const int fstep = 64 * nfree;
        for (int rd = 0; rd + 1 < rounds; ++rd)                // rounds in which every wave has a tile
            attn_tile(a, Ks, Vs, base, row_stride, b, h, 4 * rd + wave, lane);
        {
            const int qt = 4 * (rounds - 1) + wave;
            if (qt < nt) {
                attn_tile(a, Ks, Vs, base, row_stride, b, h, qt, lane);
            } else if (overlap && has_next) {
                const _Float16* nb = head_base(next);
                at_gather(pv, nb, row_stride, (int64_t)2 * H * D, fi, fstep, total, vpr);   // V: requested first, kept in registers
                if (dma) {
                    at_dma_k(Kn, nb, row_stride, (int64_t)H * D, wave - busy_last, nfree, lane, total, vpr);
                } else {
#pragma unroll
                    for (int j0 = 0; j0 < AT_PF; j0 += 5) {    // K: through registers into the idle buffer, five in flight
                        u32x4 kk[5];
                        at_gather(kk, nb, row_stride, (int64_t)H * D, fi + fstep * j0, fstep, total, vpr);
                        at_scatter(kk, Kn, kpitch, fi + fstep * j0, fstep, total, vpr);
                    }
                }
                __builtin_amdgcn_s_waitcnt(0);       // the DMA pieces have landed before the barrier
            }
        }
        __syncthreads();                     // every wave is done with this item's LDS image
        if (has_next) {
            if (overlap) {
                if (wave >= busy_last) at_scatter(pv, Vs, AT_VPITCH, fi, fstep, total, vpr);
            } else {
                fill_all(next, Kn);
            }
        }
        __syncthreads();
        cur ^= 1;
    }
}

// The production schedule: 8 waves per workgroup, two per SIMD, so that one wave's softmax (VALU)
// and LDS waits run beside its partner's MFMAs.  The LDS image of one item (the same buffers as
// above: K double-buffered, V single) still allows one workgroup per CU, so the work is cut
// into UNITS: an (image, head) item, or, when the items are fewer than the CUs, a part of an
// item's query tiles (each part's workgroup fills its own copy of K and V, from L2).  A unit of
// k <= 9 tiles runs in at most two rounds: wave w takes tile w, and wave 0 also tile 8 (k = 9);
// every other wave fetches the next unit as soon as its own tile is done - V into registers, kept
// until the barrier, K by LDS DMA into the idle buffer (through registers when its rows are
// padded).  Units go to workgroups so that one XCD runs whole images (all heads of an image
// side by side): a qkv row's K and V bytes, which neighbouring heads share cache lines of,
// reach one L2 once.  attn_tile is the same code in both schedules: each query's arithmetic is
// unchanged, whichever wave and workgroup run its tile.
#define AT_WAVES 8
#define AT_PF2 8                // 16-byte vectors of V (and of padded K) a fetching thread holds
static_assert(AT_ROWS * 2 * AT_DC <= 64 * (AT_WAVES - 1) * AT_PF2,
              "seven fetching waves hold the largest image's V in registers");

struct AttnSched {
    int parts;                  // units per item (1 unless the items are fewer than the CUs)
    int tpp;                    // query tiles per unit (the last part of an item may have fewer)
    int units;                  // items * parts
};

__global__ __launch_bounds__(64 * AT_WAVES) void vit_attention_kernel(const AttnArgs a, const AttnSched sc) {
    __shared__ __attribute__((aligned(16))) unsigned char Kb[2 * AT_KBYTES];
    __shared__ __attribute__((aligned(16))) unsigned char Vs[AT_ROWS * AT_VPITCH];
    const int N = a.N, D = a.D, H = a.H, kpitch = a.kpitch;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branches on it are uniform
    const int64_t row_stride = (int64_t)3 * H * D;
    const int nt = (N + 31) >> 5;
    const int vpr = D >> 3, total = N * vpr;
    const bool dma = kpitch == 2 * D && ((total + 63) >> 6) * 1024 <= AT_KBYTES;
    const bool loads = !(a.debug & 1);
    // workgroups g and g + 8 share an XCD: give each XCD a contiguous run of units
    const int G = gridDim.x, g = blockIdx.x;
    const int first = (G & 7) == 0 ? (g & 7) * (G >> 3) + (g >> 3) : g;
    at_zero_v_tail(Vs, N, AT_ROWS, tid, 64 * AT_WAVES);        // N is the same for every unit: once
    auto head_base = [&](int unit) {
        const int item = unit / sc.parts;
        return a.qkv + (int64_t)(item / H) * N * row_stride + (int64_t)(item % H) * D;
    };
    if (first < sc.units && loads) {                 // the first unit: every thread, through registers
        const _Float16* nb = head_base(first);
        for (int f0 = tid; f0 < total; f0 += 64 * AT_WAVES * AT_PF2) {
            u32x4 kk[AT_PF2], vv[AT_PF2];
            at_gather(kk, nb, row_stride, (int64_t)H * D, f0, 64 * AT_WAVES, total, vpr);
            at_gather(vv, nb, row_stride, (int64_t)2 * H * D, f0, 64 * AT_WAVES, total, vpr);
            at_scatter(kk, Kb, kpitch, f0, 64 * AT_WAVES, total, vpr);
            at_scatter(vv, Vs, AT_VPITCH, f0, 64 * AT_WAVES, total, vpr);
        }
    }
    __syncthreads();
    int cur = 0;
    for (int unit = first; unit < sc.units; unit += G) {
        const int item = unit / sc.parts, part = unit - item * sc.parts;
        const int b = item / H, h = item % H;
        const int t0 = part * sc.tpp;
        const int k = nt - t0 < sc.tpp ? nt - t0 : sc.tpp;            // tiles of this unit
        const int busy = k > AT_WAVES ? k - AT_WAVES : 0;             // waves with a second tile (0 or 1)
        const int nfree = AT_WAVES - busy;
        const _Float16* base = head_base(unit);
        const unsigned char* Ks = Kb + cur * AT_KBYTES;
        unsigned char* Kn = Kb + (cur ^ 1) * AT_KBYTES;
        const int next = unit + G;
        const bool has_next = next < sc.units && loads;
        const int fi = (wave - busy) * 64 + lane;                     // index among the fetching threads
        u32x4 pv[AT_PF2];
        for (int qt = t0 + wave; qt < t0 + k; qt += AT_WAVES)
            attn_tile(a, Ks, Vs, base, row_stride, b, h, qt, lane);
        if (wave >= busy && has_next) {
            const _Float16* nb = head_base(next);
            at_gather(pv, nb, row_stride, (int64_t)2 * H * D, fi, 64 * nfree, total, vpr);
            if (dma) {
                at_dma_k(Kn, nb, row_stride, (int64_t)H * D, wave - busy, nfree, lane, total, vpr);
            } else {
                u32x4 kk[AT_PF2];               // K: through registers into the idle buffer
                at_gather(kk, nb, row_stride, (int64_t)H * D, fi, 64 * nfree, total, vpr);
                at_scatter(kk, Kn, kpitch, fi, 64 * nfree, total, vpr);
            }
            __builtin_amdgcn_s_waitcnt(0);       // the DMA pieces have landed before the barrier
        }
        __syncthreads();                         // every wave is done with this unit's LDS image
        if (has_next && wave >= busy) at_scatter(pv, Vs, AT_VPITCH, fi, 64 * nfree, total, vpr);
        __syncthreads();
        cur ^= 1;
    }
}

// shapes both entry points accept (the same: a shape that moves between this kernel and the
// caller's fallback would change its output)
static int attn_setup(AttnArgs& a, const void* qkv, void* out, int64_t batch, int64_t tokens,
                      int64_t heads, int64_t head_dim, float scale, int dtype) {
    if (dtype != ECOFLAP_F16) return ECOFLAP_EDTYPE;
    if (batch <= 0 || tokens <= 0 || tokens > AT_ROWS || heads <= 0 || head_dim < 8 ||
        head_dim > 16 * AT_DC || (head_dim % 8) != 0 || batch * heads > 0x7fffffffLL)
        return ECOFLAP_ESIZE;
    int kp = 2 * (int)head_dim;                    // 16-byte vectors per K row in LDS must be odd
    if (((kp / 16) & 1) == 0) kp += 16;
    if (tokens * kp > AT_KBYTES) return ECOFLAP_ESIZE;     // one K image of the double buffer
    if (!qkv || !out) return ECOFLAP_ENULL;
    if (!aligned16(qkv) || (((uintptr_t)out) & 7u)) return ECOFLAP_EALIGN;
    a.qkv = (const _Float16*)qkv;
    a.out = (_Float16*)out;
    a.B = (int)batch; a.N = (int)tokens; a.H = (int)heads; a.D = (int)head_dim;
    a.kpitch = kp;
    a.scale_log2e = scale * 1.4426950408889634f;
    {
        // phase-ablation switches of tools/attention_launches.py (read once; 0 in production)
        static const int debug = [] { const char* d = getenv("ECOFLAP_ATTN_DEBUG"); return d ? atoi(d) : 0; }();
        a.debug = debug;
    }
    return 0;
}

extern "C" int ecoflap_vit_attention(const void* qkv, void* out, int64_t batch, int64_t tokens,
                                     int64_t heads, int64_t head_dim, float scale, int dtype,
                                     void* stream) {
    AttnArgs a;
    const int rc = attn_setup(a, qkv, out, batch, tokens, heads, head_dim, scale, dtype);
    if (rc) return rc;
    // one persistent workgroup per CU (its LDS image allows no second one); fewer items than CUs:
    // split each item's query tiles over several workgroups
    const int64_t cus = 256, items = batch * heads, nt = (tokens + 31) / 32;
    AttnSched sc;
    int64_t parts = items < cus ? cus / items : 1;
    if (parts > nt) parts = nt;
    sc.tpp = (int)((nt + parts - 1) / parts);
    sc.parts = (int)((nt + sc.tpp - 1) / sc.tpp);
    if (items * sc.parts > 0x7fffffffLL) return ECOFLAP_ESIZE;
    sc.units = (int)(items * sc.parts);
    const int grid = sc.units < cus ? sc.units : (int)cus;
    hipLaunchKernelGGL(vit_attention_kernel, dim3((unsigned)grid), dim3(64 * AT_WAVES), 0, (hipStream_t)stream, a, sc);
    ECO_CHECK_LAUNCH();
    return 0;
}

// The previous schedule (one workgroup of 4 waves per CU, the free waves of the last round
// fetching the next item): the reference the bitwise tests and tools/attention_launches.py
// compare the production kernel with.
extern "C" int ecoflap_vit_attention_v1(const void* qkv, void* out, int64_t batch, int64_t tokens,
                                        int64_t heads, int64_t head_dim, float scale, int dtype,
                                        void* stream) {
    AttnArgs a;
    const int rc = attn_setup(a, qkv, out, batch, tokens, heads, head_dim, scale, dtype);
    if (rc) return rc;
    // one persistent workgroup per CU (its LDS image allows no second one) walking the items
    int64_t grid = batch * heads;
    if (grid > 256) grid = 256;
    hipLaunchKernelGGL(vit_attention_v1_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    ECO_CHECK_LAUNCH();
    return 0;
}
