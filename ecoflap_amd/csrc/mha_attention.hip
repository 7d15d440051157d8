// mha_attention.hip — multi-head self-attention of the OpenAI-CLIP towers (and of every tower of
// that shape family: head width 64, <= 224 tokens, optional causal mask) for gfx950.  Plumbing of
// the build's shape modules (include/ecoflap_shape_ops.h), not part of the pruner ABI.
//
// attention.hip serves ViT-g (257 tokens, 16 heads of 88, batch-first, no mask) and pays for 9 key
// tiles and 6 head-dimension chunks whatever the shape is.  A CLIP text head is 77 x 64 and causal,
// a visual head 197 x 64, and nn.MultiheadAttention keeps its activations sequence-first.  Here:
//
//   * the key / query tile count NT is a template parameter (1 .. 7), the head width is 64 (4
//     chunks of 16, 2 output tiles of 32): the work is proportional to the shape;
//   * rows are addressed by a token stride and a batch stride, so the in-projection's output is
//     read in place whether it is [L, N, 3D] or [N, L, 3D], and the merged heads are written where
//     out_proj reads them;
//   * one wave owns one 32-query tile of one (sample, head).  A workgroup holds K and V of IPW
//     heads in LDS and has IPW * NT waves (77 tokens: 2 heads, 6 waves; 197 tokens: 1 head, 7
//     waves).  LDS admits 2-3 workgroups per CU (43-75 KB each), registers 3-4 waves per SIMD
//     (at 197 tokens: 160 VGPRs, so one 7-wave workgroup per CU); a workgroup does not overlap
//     its own fill with its products.  Measured in profiles/r10_clip: 38-47 % of the HBM rate at
//     batch 256-512, 1.6-7.4 x the library's attention at the two towers' shapes;
//   * causal: key tiles wholly above the diagonal are neither multiplied nor exponentiated, the
//     diagonal tile is masked in registers; a masked entry's probability is exp2(-inf) = 0 exactly;
//   * the arithmetic is attention_tile.h's, instantiated per tile count with the constants 64
//     (head width), 144 (K pitch) and no ablation word: S^T = K Q^T on v_mfma_f32_32x32x16_f16,
//     fp32 scores, exact two-pass softmax, O^T = V^T P^T with V^T fragments by ds_read_b64_tr_b16
//     from a row-major V image.
// Per (sample, head) independent and free of atomics: batch invariant by construction.
//
// ecoflap_mha_attention_colsq (below) is the non-causal kernel with attention_tile.h's COLSQ
// epilogue: besides (or instead of) the merged heads it leaves sq[c] = sum over all (sample, token)
// rows of the squared f16 output in column c — the Wanda statistic of out_proj's input — without
// reading the output back.  Wave partial (32 queries, butterfly) -> workgroup partial (a head's
// query tiles, in tile order, through LDS) -> workspace row per (sample, head) -> a second small
// launch adds the samples in sample order.  No atomics: the sums' order is fixed by the shape.
#include "attention_tile.h"
#include "../../include/ecoflap_shape_ops.h"

#define MH_D 64                 // head width
#define MH_DC 4                 // 16-wide chunks of the head dimension
#define MH_DT 2                 // 32-wide tiles of the head dimension
#define MH_VPR 8                // 16-byte vectors per K / V row
#define MH_KPITCH 144           // bytes per K row in LDS: 16 * 9 (odd: a ds_read_b128 of 16 rows covers all banks once)
#define MH_MAX_NT 7             // tokens <= 224

struct MhaArgs {
    const _Float16* qkv;        // row (b, n): qkv + b * qkv_bs + n * qkv_ts, laid out [3, H, 64]
    _Float16* out;              // row (b, n): out + b * out_bs + n * out_ts, laid out [H, 64]
    float* part;                // colsq only: [B * H, 64] per-(sample, head) sums; out may be null
    int64_t qkv_ts, qkv_bs, out_ts, out_bs;     // elements
    int B, N, H;
    float scale_log2e;          // softmax scale * log2(e)
};

// heads per workgroup: a workgroup has IPW * NT waves, at least 4 and at most 7
template <int NT> struct MhaCfg {
    static constexpr int IPW = NT >= 4 ? 1 : (NT == 3 ? 2 : 4 / NT);
    static constexpr int WAVES = IPW * NT;
    static constexpr int ROWS = 32 * NT;
};

// Workgroup g: heads (items) g * IPW .. g * IPW + IPW - 1 of the B * H; wave w: item w / NT of
// them, query tile w % NT.  One barrier: after the fill.
template <int NT, bool CAUSAL, bool COLSQ>
__global__ __launch_bounds__(64 * MhaCfg<NT>::WAVES) void mha_attention_kernel(const MhaArgs a) {
    constexpr int IPW = MhaCfg<NT>::IPW, WAVES = MhaCfg<NT>::WAVES, ROWS = MhaCfg<NT>::ROWS;
    constexpr int THREADS = 64 * WAVES;
    __shared__ __attribute__((aligned(16))) unsigned char Kb[IPW * ROWS * MH_KPITCH];
    __shared__ __attribute__((aligned(16))) unsigned char Vb[IPW * ROWS * AT_VPITCH];
    __shared__ __attribute__((aligned(16))) float Sq[COLSQ ? WAVES * MH_D : 4];     // colsq: a row per wave
    const int N = a.N, H = a.H;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branches on it are uniform
    const int nitems = a.B * H;
    const int item0 = (int)blockIdx.x * IPW;
    const int64_t HD = (int64_t)H * MH_D;
#pragma unroll
    for (int li = 0; li < IPW; ++li) at_zero_v_tail(Vb + li * ROWS * AT_VPITCH, N, ROWS, tid, THREADS);
    // K and V of the workgroup's heads into LDS: 4 vectors of each per thread in flight
    {
        const int per = N * MH_VPR;
        int live = nitems - item0;
        if (live > IPW) live = IPW;
        const int total = live * per;
        for (int v0 = tid; v0 < total; v0 += 4 * THREADS) {
            u32x4 kk[4], vv[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v1 = v0 + j * THREADS;
                const int v = v1 < total ? v1 : total - 1;
                const int li = v / per, rem = v - li * per;
                const int key = rem >> 3, c = rem & 7;
                const int item = item0 + li;
                const _Float16* src = a.qkv + (int64_t)(item / H) * a.qkv_bs + (int64_t)key * a.qkv_ts +
                                      (int64_t)(item % H) * MH_D + 8 * c;
                kk[j] = *(const u32x4*)(src + HD);
                vv[j] = *(const u32x4*)(src + 2 * HD);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int v = v0 + j * THREADS;
                if (v < total) {
                    const int li = v / per, rem = v - li * per;
                    const int key = rem >> 3, c = rem & 7;
                    *(u32x4*)(Kb + (li * ROWS + key) * MH_KPITCH + 16 * c) = kk[j];
                    *(u32x4*)(Vb + (li * ROWS + key) * AT_VPITCH + 16 * c) = vv[j];
                }
            }
        }
    }
    __syncthreads();
    const int li = wave / NT, qt = wave - li * NT;
    const int item = item0 + li;
    if (item < nitems && 32 * qt < N) {
        const int b = item / H, h = item - b * H;
        // constants for the head width, the K pitch and the ablation word: their selects fold away
        if constexpr (COLSQ)
            attention_tile<NT, MH_DC, MH_DT, CAUSAL, false, true>(
                Kb + li * ROWS * MH_KPITCH, Vb + li * ROWS * AT_VPITCH, MH_KPITCH,
                a.qkv + (int64_t)b * a.qkv_bs + (int64_t)h * MH_D, a.qkv_ts,
                a.out ? a.out + (int64_t)b * a.out_bs + (int64_t)h * MH_D : nullptr, a.out_ts, N, MH_D,
                a.scale_log2e, 0, qt, lane, Sq + wave * MH_D);
        else
            attention_tile<NT, MH_DC, MH_DT, CAUSAL, false>(
                Kb + li * ROWS * MH_KPITCH, Vb + li * ROWS * AT_VPITCH, MH_KPITCH,
                a.qkv + (int64_t)b * a.qkv_bs + (int64_t)h * MH_D, a.qkv_ts,
                a.out + (int64_t)b * a.out_bs + (int64_t)h * MH_D, a.out_ts, N, MH_D, a.scale_log2e, 0, qt, lane);
    } else if constexpr (COLSQ) {
        Sq[wave * MH_D + lane] = 0.f;       // a query tile wholly past N (or past the last head): nothing
    }
    if constexpr (COLSQ) {
        // a head's query tiles in tile order -> its row of the workspace (every wave arrives here)
        __syncthreads();
        if (tid < IPW * MH_D) {
            const int hl = tid >> 6, c = tid & 63;
            if (item0 + hl < nitems) {
                float acc = Sq[(hl * NT) * MH_D + c];
#pragma unroll
                for (int t = 1; t < NT; ++t) acc += Sq[(hl * NT + t) * MH_D + c];
                a.part[(int64_t)(item0 + hl) * MH_D + c] = acc;
            }
        }
    }
}

// sq[h * 64 + c] = part[(0, h), c] + part[(1, h), c] + ... in sample order
__global__ __launch_bounds__(256) void mha_colsq_finish_kernel(const float* __restrict__ part,
                                                               float* __restrict__ sq, int B, int H) {
    const int i = (int)blockIdx.x * 256 + (int)threadIdx.x;
    const int HD = H * MH_D;
    if (i >= HD) return;
    float acc = part[i];
    for (int b = 1; b < B; ++b) acc += part[(int64_t)b * HD + i];
    sq[i] = acc;
}

template <int NT>
static int mha_launch(const MhaArgs& a, int causal, hipStream_t stream) {
    constexpr int IPW = MhaCfg<NT>::IPW, WAVES = MhaCfg<NT>::WAVES;
    const int nitems = a.B * a.H;
    const unsigned grid = (unsigned)((nitems + IPW - 1) / IPW);
    if (causal)
        hipLaunchKernelGGL((mha_attention_kernel<NT, true, false>), dim3(grid), dim3(64 * WAVES), 0, stream, a);
    else
        hipLaunchKernelGGL((mha_attention_kernel<NT, false, false>), dim3(grid), dim3(64 * WAVES), 0, stream, a);
    ECO_CHECK_LAUNCH();
    return 0;
}

template <int NT>
static int mha_colsq_launch(const MhaArgs& a, float* sq, hipStream_t stream) {
    constexpr int IPW = MhaCfg<NT>::IPW, WAVES = MhaCfg<NT>::WAVES;
    const int nitems = a.B * a.H;
    const unsigned grid = (unsigned)((nitems + IPW - 1) / IPW);
    hipLaunchKernelGGL((mha_attention_kernel<NT, false, true>), dim3(grid), dim3(64 * WAVES), 0, stream, a);
    ECO_CHECK_LAUNCH();
    hipLaunchKernelGGL(mha_colsq_finish_kernel, dim3((unsigned)((a.H * MH_D + 255) / 256)), dim3(256), 0,
                       stream, (const float*)a.part, sq, a.B, a.H);
    ECO_CHECK_LAUNCH();
    return 0;
}

extern "C" int ecoflap_mha_attention(const void* qkv, void* out, int64_t batch, int64_t tokens,
                                     int64_t heads, int64_t head_dim, int64_t qkv_token_stride,
                                     int64_t qkv_batch_stride, int64_t out_token_stride,
                                     int64_t out_batch_stride, int causal, float scale, int dtype,
                                     void* stream) {
    if (dtype != ECOFLAP_F16) return ECOFLAP_EDTYPE;
    if (batch <= 0 || tokens <= 0 || tokens > 32 * MH_MAX_NT || heads <= 0 || head_dim != MH_D ||
        batch * heads > 0x7fffffffLL || !(scale > 0.f) || !(scale < __builtin_inff()))
        return ECOFLAP_ESIZE;
    // a row holds [3, heads, 64] / [heads, 64]; rows may not overlap
    if (qkv_token_stride < 3 * heads * MH_D || out_token_stride < heads * MH_D ||
        qkv_batch_stride < 0 || out_batch_stride < 0)
        return ECOFLAP_ESIZE;
    if (!qkv || !out) return ECOFLAP_ENULL;
    if (!aligned16(qkv) || !aligned16(out) || (qkv_token_stride & 7) || (qkv_batch_stride & 7) ||
        (out_token_stride & 7) || (out_batch_stride & 7))
        return ECOFLAP_EALIGN;
    MhaArgs a;
    a.qkv = (const _Float16*)qkv;
    a.out = (_Float16*)out;
    a.part = nullptr;
    a.qkv_ts = qkv_token_stride; a.qkv_bs = qkv_batch_stride;
    a.out_ts = out_token_stride; a.out_bs = out_batch_stride;
    a.B = (int)batch; a.N = (int)tokens; a.H = (int)heads;
    a.scale_log2e = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    switch ((int)((tokens + 31) / 32)) {
        case 1: return mha_launch<1>(a, causal, st);
        case 2: return mha_launch<2>(a, causal, st);
        case 3: return mha_launch<3>(a, causal, st);
        case 4: return mha_launch<4>(a, causal, st);
        case 5: return mha_launch<5>(a, causal, st);
        case 6: return mha_launch<6>(a, causal, st);
        default: return mha_launch<7>(a, causal, st);
    }
}

extern "C" size_t ecoflap_mha_attention_colsq_workspace_bytes(int64_t batch, int64_t heads) {
    if (batch <= 0 || heads <= 0 || batch * heads > 0x7fffffffLL) return 0;
    return (size_t)(batch * heads) * MH_D * sizeof(float);
}

extern "C" int ecoflap_mha_attention_colsq(const void* qkv, void* out, float* sq, void* workspace,
                                           size_t workspace_bytes, int64_t batch, int64_t tokens,
                                           int64_t heads, int64_t head_dim, int64_t qkv_token_stride,
                                           int64_t qkv_batch_stride, int64_t out_token_stride,
                                           int64_t out_batch_stride, float scale, int dtype,
                                           void* stream) {
    if (dtype != ECOFLAP_F16) return ECOFLAP_EDTYPE;
    if (batch <= 0 || tokens <= 0 || tokens > 32 * MH_MAX_NT || heads <= 0 || head_dim != MH_D ||
        batch * heads > 0x7fffffffLL || heads * MH_D > 0x7fffffffLL || !(scale > 0.f) ||
        !(scale < __builtin_inff()))
        return ECOFLAP_ESIZE;
    if (qkv_token_stride < 3 * heads * MH_D || qkv_batch_stride < 0) return ECOFLAP_ESIZE;
    if (out && (out_token_stride < heads * MH_D || out_batch_stride < 0)) return ECOFLAP_ESIZE;
    if (workspace_bytes < ecoflap_mha_attention_colsq_workspace_bytes(batch, heads)) return ECOFLAP_ESIZE;
    if (!qkv || !sq || !workspace) return ECOFLAP_ENULL;
    if (!aligned16(qkv) || !aligned16(sq) || !aligned16(workspace) || (qkv_token_stride & 7) ||
        (qkv_batch_stride & 7))
        return ECOFLAP_EALIGN;
    if (out && (!aligned16(out) || (out_token_stride & 7) || (out_batch_stride & 7))) return ECOFLAP_EALIGN;
    MhaArgs a;
    a.qkv = (const _Float16*)qkv;
    a.out = (_Float16*)out;
    a.part = (float*)workspace;
    a.qkv_ts = qkv_token_stride; a.qkv_bs = qkv_batch_stride;
    a.out_ts = out ? out_token_stride : 0; a.out_bs = out ? out_batch_stride : 0;
    a.B = (int)batch; a.N = (int)tokens; a.H = (int)heads;
    a.scale_log2e = scale * 1.4426950408889634f;
    hipStream_t st = (hipStream_t)stream;
    switch ((int)((tokens + 31) / 32)) {
        case 1: return mha_colsq_launch<1>(a, sq, st);
        case 2: return mha_colsq_launch<2>(a, sq, st);
        case 3: return mha_colsq_launch<3>(a, sq, st);
        case 4: return mha_colsq_launch<4>(a, sq, st);
        case 5: return mha_colsq_launch<5>(a, sq, st);
        case 6: return mha_colsq_launch<6>(a, sq, st);
        default: return mha_colsq_launch<7>(a, sq, st);
    }
}
