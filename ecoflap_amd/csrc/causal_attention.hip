// causal_attention.hip — causal self-attention of a LLaMA decoder block for gfx950, rotary embedding
// included: out = softmax(rot(q) rot(k)^T * scale + causal mask) v per (sample, head), head width
// 128, up to 4096 tokens, no KV cache; grouped-query attention (kv_heads < heads: query head h reads
// KV head h / (heads / kv_heads), transformers' repeat_kv order) included.  Plumbing of the build's
// shape modules (include/ecoflap_shape_ops.h, shapes/llama.py), not part of the pruner ABI.
//
// attention.hip and mha_attention.hip hold all of K and V of a head in LDS and run an exact
// two-pass softmax; a 2048 x 128 head is 512 KB of K alone.  Here (attention_stream.h):
//
//   * a workgroup of 8 waves owns 256 consecutive queries of one (sample, head), a wave 32 of
//     them; key / value blocks of 64 stream through LDS, double-buffered (2 x 37 KB), one barrier
//     per block.  The next block's rows travel from memory into registers while the current block
//     is multiplied, and are written to the other buffer after.  One workgroup per CU, two waves
//     per SIMD, 247 VGPRs and no scratch: with 4 waves per workgroup a thread stages twice as
//     many rows and the kernel spills (profiles/r13_llama);
//   * q, k and v are three pointers with one token stride and one batch stride: the three Linears'
//     outputs are read in place (three tensors or three slices of one), the merged heads are
//     written where o_proj reads them;
//   * the rotation is transformers' rotate_half form (element d pairs with d + 64) from a caller's
//     fp32 table [tokens, 64]: K is rotated as its block is written to LDS, Q as it is loaded into
//     registers, in fp32, rounded once to f16; no rotated copy exists in memory;
//   * key blocks wholly above a workgroup's diagonal are never loaded; key tiles above a wave's
//     diagonal are neither multiplied nor exponentiated; the diagonal tile is masked in registers;
//   * the workgroups of the late (long) query blocks come first in grid order;
//   * grouped-query attention (template parameter P, heads per workgroup): a wave's result depends
//     only on its own (sample, head, 32-query tile) and on the K / V blocks it reads, so the 8 waves
//     need not belong to one head.  With P in {2, 4, 8} they are P query heads of one KV group
//     times 8 / P query tiles: the workgroup owns 256 / P consecutive queries, a K / V block is
//     fetched, rotated and staged once for P heads, and the key-block count follows the shorter
//     query span.  P == 1 is the mapping above and the default: the kernel is bound by the chain
//     of key blocks of its longest workgroups, not by the K / V fetch, and no larger P measured
//     faster beyond the spread (profiles/r17_llama_gqa).  Every (sample, head, 32-query tile) gets
//     the bits it gets at P == 1 on K / V expanded to all heads.
// Online softmax with a rescale on every block (no deferred-rescale threshold), no atomics; every
// (sample, head, query block) is computed by itself: batch invariant bit for bit.
#include "attention_stream.h"
#include "../../include/ecoflap_shape_ops.h"

#define CA_WAVES 8
#define CA_THREADS (64 * CA_WAVES)
#define CA_QROWS (32 * CA_WAVES) // queries per workgroup
#define CA_MAX_TOKENS 4096
#define CA_KTASKS (AS_KEYS * 8 / CA_THREADS)     // per thread: pairs of 16-byte chunks of K
#define CA_VTASKS (AS_KEYS * 16 / CA_THREADS)    // per thread: 16-byte chunks of V

struct CausalArgs {
    const _Float16 *q, *k, *v;  // q row (b, n): q + b * q_bs + n * q_ts, laid out [H, 128];
                                // k / v row (b, n): ptr + b * kv_bs + n * kv_ts, laid out [KVH, 128]
    _Float16* out;              // row (b, n): out + b * out_bs + n * out_ts, laid out [H, 128]
    const float *cos, *sin;     // [N, 64] (ROPE only)
    int64_t q_ts, q_bs, kv_ts, kv_bs, out_ts, out_bs;   // elements
    int B, N, KVH, G, nqb;      // G = H / KVH query heads per KV head; nqb: query blocks of
                                // CA_QROWS / P per (sample, head)
    float scale_log2e;          // softmax scale * log2(e)
};

// x_lo' = x_lo cos - x_hi sin, x_hi' = x_hi cos + x_lo sin on 8 pairs (d, d + 64), every product
// and sum rounded to fp32 on its own
static __device__ __forceinline__ void rotate8(float* lo, float* hi, const float4 (&c)[2], const float4 (&s)[2]) {
    const float cs[8] = {c[0].x, c[0].y, c[0].z, c[0].w, c[1].x, c[1].y, c[1].z, c[1].w};
    const float sn[8] = {s[0].x, s[0].y, s[0].z, s[0].w, s[1].x, s[1].y, s[1].z, s[1].w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float a = lo[i], b = hi[i];
        lo[i] = a * cs[i] - b * sn[i];
        hi[i] = b * cs[i] + a * sn[i];
    }
}

// P: query heads per workgroup, one of 1, 2, 4, 8 and a divisor of G.  Wave w serves query head
// kvh * G + P * gi + w % P and query tile (8 / P) * qb + w / P.
template <bool ROPE, int P>
__global__ __launch_bounds__(CA_THREADS) void causal_attention_kernel(const CausalArgs a) {
    constexpr int TILES = CA_WAVES / P;             // query tiles of 32 per workgroup
    constexpr int QROWS = 32 * TILES;               // queries per workgroup
    __shared__ __attribute__((aligned(16))) unsigned char Kb[2 * AS_KBYTES];
    __shared__ __attribute__((aligned(16))) unsigned char Vb[2 * AS_VBYTES];
    const int N = a.N;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branches on it are uniform
    const int per = a.G / P;                        // workgroups per (sample, KV head, query block)
    const unsigned nitems = (unsigned)(a.B * a.KVH * per);
    const int qb = a.nqb - 1 - (int)(blockIdx.x / nitems);          // late (long) query blocks first
    const int item = (int)(blockIdx.x % nitems);
    const int b = item / (a.KVH * per), kvg = item - b * (a.KVH * per);
    const int kvh = kvg / per, gi = kvg - kvh * per;
    const int h = kvh * a.G + P * gi + wave % P;    // this wave's query head
    const int64_t in0 = (int64_t)b * a.q_bs + (int64_t)h * AS_D;
    const int64_t kv0 = (int64_t)b * a.kv_bs + (int64_t)kvh * AS_D;
    const _Float16 *kbase = a.k + kv0, *vbase = a.v + kv0;
    const int qt = TILES * qb + wave / P;           // this wave's query tile of 32
    const bool active = 32 * qt < N;                // (uniform) a tile wholly past N only helps to fill
    int lastq = QROWS * qb + QROWS - 1;
    if (lastq > N - 1) lastq = N - 1;
    const int nkb = lastq / AS_KEYS + 1;            // key blocks at or below the workgroup's diagonal

    // Q^T fragments, rotated: chunk c of lane (r, hh) is columns 16 c + 8 hh .. + 7 of its query,
    // so chunks c and c + 4 hold the pairs (d, d + 64)
    const int r = lane & 31, hh = lane >> 5;
    const int q = 32 * qt + r, qc = q < N ? q : N - 1;
    f16x8 qf[AS_DC];
    if (active) {
        const _Float16* qrow = a.q + in0 + (int64_t)qc * a.q_ts + 8 * hh;
        u32x4 raw[AS_DC];
#pragma unroll
        for (int c = 0; c < AS_DC; ++c) raw[c] = *(const u32x4*)(qrow + 16 * c);
        if constexpr (ROPE) {
#pragma unroll
            for (int c = 0; c < AS_DC / 2; ++c) {
                const int64_t t0 = (int64_t)qc * 64 + 16 * c + 8 * hh;
                const float4 cs[2] = {*(const float4*)(a.cos + t0), *(const float4*)(a.cos + t0 + 4)};
                const float4 sn[2] = {*(const float4*)(a.sin + t0), *(const float4*)(a.sin + t0 + 4)};
                float lo[8], hi[8];
                Vec<ECOFLAP_F16>::unpack(raw[c], lo);
                Vec<ECOFLAP_F16>::unpack(raw[c + 4], hi);
                rotate8(lo, hi, cs, sn);
                raw[c] = Vec<ECOFLAP_F16>::pack(lo);
                raw[c + 4] = Vec<ECOFLAP_F16>::pack(hi);
            }
        }
#pragma unroll
        for (int c = 0; c < AS_DC; ++c) qf[c] = __builtin_bit_cast(f16x8, raw[c]);
    }

    // A block's rows on their way to LDS.  K: 64 rows x 8 pair tasks (the 16-byte chunks pc and
    // pc + 8 of a row; their 8 cos and 8 sin are read when the pair is written), one per thread;
    // V: 64 rows x 16 chunks, two per thread.  Rows past the last token are read from the last
    // token's address and written as zeros.
    u32x4 kst[CA_KTASKS][2], vst[CA_VTASKS];
    auto fetch = [&](int kb) {
#pragma unroll
        for (int j = 0; j < CA_KTASKS; ++j) {
            const int id = tid + CA_THREADS * j, row = id >> 3, pc = id & 7;
            const int n = AS_KEYS * kb + row, nc = n < N ? n : N - 1;
            const _Float16* src = kbase + (int64_t)nc * a.kv_ts + 8 * pc;
            kst[j][0] = *(const u32x4*)src;
            kst[j][1] = *(const u32x4*)(src + 64);
        }
#pragma unroll
        for (int j = 0; j < CA_VTASKS; ++j) {
            const int id = tid + CA_THREADS * j, row = id >> 4, c = id & 15;
            const int n = AS_KEYS * kb + row, nc = n < N ? n : N - 1;
            vst[j] = *(const u32x4*)(vbase + (int64_t)nc * a.kv_ts + 8 * c);
        }
    };
    auto stash = [&](int kb, int buf) {
        const u32x4 z = {0u, 0u, 0u, 0u};
        unsigned char* Ks = Kb + buf * AS_KBYTES;
        unsigned char* Vs = Vb + buf * AS_VBYTES;
#pragma unroll
        for (int j = 0; j < CA_KTASKS; ++j) {
            const int id = tid + CA_THREADS * j, row = id >> 3, pc = id & 7;
            const bool live = AS_KEYS * kb + row < N;
            u32x4 lo4 = kst[j][0], hi4 = kst[j][1];
            if constexpr (ROPE) {
                const int n = AS_KEYS * kb + row;
                const int64_t t0 = (int64_t)(live ? n : N - 1) * 64 + 8 * pc;
                const float4 cs[2] = {*(const float4*)(a.cos + t0), *(const float4*)(a.cos + t0 + 4)};
                const float4 sn[2] = {*(const float4*)(a.sin + t0), *(const float4*)(a.sin + t0 + 4)};
                float lo[8], hi[8];
                Vec<ECOFLAP_F16>::unpack(lo4, lo);
                Vec<ECOFLAP_F16>::unpack(hi4, hi);
                rotate8(lo, hi, cs, sn);
                lo4 = Vec<ECOFLAP_F16>::pack(lo);
                hi4 = Vec<ECOFLAP_F16>::pack(hi);
            }
            *(u32x4*)(Ks + row * AS_KPITCH + 16 * pc) = live ? lo4 : z;
            *(u32x4*)(Ks + row * AS_KPITCH + 16 * pc + 128) = live ? hi4 : z;
        }
#pragma unroll
        for (int j = 0; j < CA_VTASKS; ++j) {
            const int id = tid + CA_THREADS * j, row = id >> 4, c = id & 15;
            const bool live = AS_KEYS * kb + row < N;
            *(u32x4*)(Vs + row * AS_VPITCH + 16 * c) = live ? vst[j] : z;
        }
    };

    fetch(0);
    stash(0, 0);
    __syncthreads();
    StreamState st;
    stream_init(st);
    for (int kb = 0; kb < nkb; ++kb) {
        const int buf = kb & 1;
        const bool more = kb + 1 < nkb;             // (uniform over the workgroup)
        if (more) fetch(kb + 1);
        __builtin_amdgcn_sched_barrier(0);
        if (active && 2 * kb <= qt) {
            const unsigned char* Ks = Kb + buf * AS_KBYTES;
            const unsigned char* Vs = Vb + buf * AS_VBYTES;
            if (2 * kb + 1 < qt) stream_block<2, false>(Ks, Vs, qf, st, a.scale_log2e, lane);
            else if (2 * kb + 1 == qt) stream_block<2, true>(Ks, Vs, qf, st, a.scale_log2e, lane);
            else stream_block<1, true>(Ks, Vs, qf, st, a.scale_log2e, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
        // everybody finished with the other buffer before the barrier that ended the last round
        if (more) stash(kb + 1, buf ^ 1);
        __syncthreads();
    }
    if (active && q < N)
        stream_store(st, a.out + (int64_t)b * a.out_bs + (int64_t)q * a.out_ts + (int64_t)h * AS_D, lane);
}

template <int P>
static void launch_causal(const CausalArgs& a, unsigned grid, bool rope, hipStream_t st) {
    if (rope)
        hipLaunchKernelGGL((causal_attention_kernel<true, P>), dim3(grid), dim3(CA_THREADS), 0, st, a);
    else
        hipLaunchKernelGGL((causal_attention_kernel<false, P>), dim3(grid), dim3(CA_THREADS), 0, st, a);
}

// heads_per_workgroup == 0.  Measured at G = 4 and G = 8 (32 / 8 and 64 / 8 heads, 2048 and 512
// tokens, profiles/r17_llama_gqa): no P > 1 is below P = 1's median by more than P = 1's own
// max - min at both token counts, so one head per workgroup stays the default for every G.
extern "C" int ecoflap_causal_attention_gqa_default_p(int64_t group) { return group < 1 ? 0 : 1; }

extern "C" int ecoflap_causal_attention_gqa(const void* q, const void* k, const void* v, void* out,
                                            const float* rope_cos, const float* rope_sin, int64_t batch,
                                            int64_t tokens, int64_t heads, int64_t kv_heads,
                                            int64_t head_dim, int64_t q_token_stride,
                                            int64_t q_batch_stride, int64_t kv_token_stride,
                                            int64_t kv_batch_stride, int64_t out_token_stride,
                                            int64_t out_batch_stride, float scale,
                                            int heads_per_workgroup, int dtype, void* stream) {
    if (dtype != ECOFLAP_F16) return ECOFLAP_EDTYPE;
    if (batch <= 0 || batch > 0x7fffffffLL || heads <= 0 || heads > 0x7fffffffLL || tokens < 1 ||
        tokens > CA_MAX_TOKENS || head_dim != AS_D || !(scale > 0.f) || !(scale < __builtin_inff()))
        return ECOFLAP_ESIZE;
    if (batch * heads > 0x7fffffffLL || batch * heads * ((tokens + 31) / 32) > 0x7fffffffLL) return ECOFLAP_ESIZE;
    if (kv_heads < 1 || heads % kv_heads != 0) return ECOFLAP_ESIZE;
    const int64_t group = heads / kv_heads;
    int P = heads_per_workgroup;
    if (P == 0) P = ecoflap_causal_attention_gqa_default_p(group);
    if ((P != 1 && P != 2 && P != 4 && P != 8) || group % P != 0) return ECOFLAP_ESIZE;
    // a q / out row holds [heads, 128], a k / v row [kv_heads, 128]; rows may not overlap
    if (q_token_stride < heads * AS_D || kv_token_stride < kv_heads * AS_D ||
        out_token_stride < heads * AS_D || q_batch_stride < 0 || kv_batch_stride < 0 || out_batch_stride < 0)
        return ECOFLAP_ESIZE;
    if (!q || !k || !v || !out || (!rope_cos != !rope_sin)) return ECOFLAP_ENULL;
    if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(out) || !aligned16(rope_cos) ||
        !aligned16(rope_sin) || (q_token_stride & 7) || (q_batch_stride & 7) || (kv_token_stride & 7) ||
        (kv_batch_stride & 7) || (out_token_stride & 7) || (out_batch_stride & 7))
        return ECOFLAP_EALIGN;
    CausalArgs a;
    a.q = (const _Float16*)q; a.k = (const _Float16*)k; a.v = (const _Float16*)v;
    a.out = (_Float16*)out;
    a.cos = rope_cos; a.sin = rope_sin;
    a.q_ts = q_token_stride; a.q_bs = q_batch_stride;
    a.kv_ts = kv_token_stride; a.kv_bs = kv_batch_stride;
    a.out_ts = out_token_stride; a.out_bs = out_batch_stride;
    a.B = (int)batch; a.N = (int)tokens; a.KVH = (int)kv_heads; a.G = (int)group;
    const int64_t qrows = CA_QROWS / P;
    a.nqb = (int)((tokens + qrows - 1) / qrows);
    a.scale_log2e = scale * 1.4426950408889634f;
    // batch * heads / P workgroups per query block: at most batch * heads * ceil(tokens / 32) < 2^31
    const unsigned grid = (unsigned)(batch * kv_heads * (group / P) * a.nqb);
    hipStream_t st = (hipStream_t)stream;
    switch (P) {
    case 1: launch_causal<1>(a, grid, rope_cos != nullptr, st); break;
    case 2: launch_causal<2>(a, grid, rope_cos != nullptr, st); break;
    case 4: launch_causal<4>(a, grid, rope_cos != nullptr, st); break;
    default: launch_causal<8>(a, grid, rope_cos != nullptr, st); break;
    }
    ECO_CHECK_LAUNCH();
    return 0;
}

extern "C" int ecoflap_causal_attention(const void* q, const void* k, const void* v, void* out,
                                        const float* rope_cos, const float* rope_sin, int64_t batch,
                                        int64_t tokens, int64_t heads, int64_t head_dim,
                                        int64_t qkv_token_stride, int64_t qkv_batch_stride,
                                        int64_t out_token_stride, int64_t out_batch_stride,
                                        float scale, int dtype, void* stream) {
    return ecoflap_causal_attention_gqa(q, k, v, out, rope_cos, rope_sin, batch, tokens, heads, heads, head_dim,
                                        qkv_token_stride, qkv_batch_stride, qkv_token_stride, qkv_batch_stride,
                                        out_token_stride, out_batch_stride, scale, 1, dtype, stream);
}
