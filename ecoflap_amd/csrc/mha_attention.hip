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
//   * the arithmetic of attention.hip's attn_tile: S^T = K Q^T on v_mfma_f32_32x32x16_f16 (queries
//     on the lanes, keys in the registers), fp32 scores, exact two-pass softmax with four
//     independent chains, probabilities rounded to f16 and fed to O^T = V^T P^T straight from
//     their registers, V^T fragments by ds_read_b64_tr_b16 from a row-major V image.
// Per (sample, head) independent and free of atomics: batch invariant by construction.
#include "common.h"
#include "../../include/ecoflap_shape_ops.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define MH_D 64                 // head width
#define MH_DC 4                 // 16-wide chunks of the head dimension
#define MH_DT 2                 // 32-wide tiles of the head dimension
#define MH_VPR 8                // 16-byte vectors per K / V row
#define MH_KPITCH 144           // bytes per K row in LDS: 16 * 9 (odd: a ds_read_b128 of 16 rows covers all banks once)
#define MH_VPITCH 192           // bytes per V row in LDS: 64 * 3 (4 consecutive rows x 64 B cover all banks once)
#define MH_MAX_NT 7             // tokens <= 224

struct MhaArgs {
    const _Float16* qkv;        // row (b, n): qkv + b * qkv_bs + n * qkv_ts, laid out [3, H, 64]
    _Float16* out;              // row (b, n): out + b * out_bs + n * out_ts, laid out [H, 64]
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

static __device__ __forceinline__ f32x16 mh_mfma(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// One 32-query tile of one (sample, head): S^T = K Q^T, exact softmax, O^T = V^T P^T, store.
// qbase: q of (b, token 0, h); obase: out of (b, token 0, h).  `qt` is wave-uniform.
template <int NT, bool CAUSAL>
static __device__ __forceinline__ void mha_tile(const MhaArgs& a, const unsigned char* Ks,
                                                const unsigned char* Vs, const _Float16* qbase,
                                                _Float16* obase, int qt, int lane) {
    const int N = a.N;
    const int r = lane & 31, hh = lane >> 5;
    const int q = 32 * qt + r;
    const int qc = q < N ? q : N - 1;
    const int tmax = CAUSAL ? qt : NT - 1;          // last key tile this query tile attends to
    // Q^T fragments (B operand: k = d on the half-lanes, column = query on the lanes)
    f16x8 qf[MH_DC];
#pragma unroll
    for (int c = 0; c < MH_DC; ++c) qf[c] = *(const f16x8*)(qbase + (int64_t)qc * a.qkv_ts + 16 * c + 8 * hh);
    // S^T = K Q^T: tile t holds keys 32t .. 32t+31 (rows, in the registers) x 32 queries (lanes).
    // d-chunk outermost: independent accumulators per step; a K fragment's register is reloaded
    // for the next chunk as soon as its product has issued.
    f32x16 s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[t][i] = 0.f;
    {
        const unsigned char* krow = Ks + r * MH_KPITCH + 16 * hh;
        f16x8 kf[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t <= tmax) kf[t] = *(const f16x8*)(krow + 32 * t * MH_KPITCH);
#pragma unroll
        for (int c = 0; c < MH_DC; ++c) {
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t <= tmax) {
                    s[t] = mh_mfma(kf[t], qf[c], s[t]);
                    if (c + 1 < MH_DC) kf[t] = *(const f16x8*)(krow + 32 * t * MH_KPITCH + 32 * (c + 1));
                }
            }
            // (keeps the scheduler from hoisting every later chunk's loads up here: they spill)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // exact softmax over the keys of this lane's query: own registers, then lane ^ 32.  Four
    // independent chains for the maximum and for the sum.  Key 0 is never masked: m is finite.
    float mx[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t <= tmax) {
            if (32 * t + 32 > N || (CAUSAL && t == qt)) {      // uniform: the tile past N, the diagonal tile
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const int key = 32 * t + (i & 3) + 8 * (i >> 2) + 4 * hh;
                    const bool keep = key < N && (!CAUSAL || key <= q);
                    s[t][i] = keep ? s[t][i] : -__builtin_inff();
                }
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) mx[i & 3] = __builtin_fmaxf(mx[i & 3], s[t][i]);
        }
    }
    float m = __builtin_fmaxf(__builtin_fmaxf(mx[0], mx[1]), __builtin_fmaxf(mx[2], mx[3]));
    m = __builtin_fmaxf(m, __shfl_xor(m, 32, 64));
    const float c2 = a.scale_log2e, mc = m * c2;
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        if (t <= tmax) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = __builtin_amdgcn_exp2f(s[t][i] * c2 - mc);     // masked: exp2(-inf) = 0
                s[t][i] = p;
                ls[i & 3] += p;
            }
        }
    }
    float l = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    l += __shfl_xor(l, 32, 64);
    // O^T = V^T P^T: P tile t, k-step st = registers 8 st .. 8 st + 7 of s[t], as they stand.  V
    // stays row-major in LDS; its transposed A fragments come from ds_read_b64_tr_b16: lane 4q+p
    // of a 16-lane group addresses row q, columns 4p..4p+3 of a 4-key x 16-column block and
    // receives column (lane & 15) of the 4 keys - the MFMA's k order (keys 4h..4h+3 and
    // 8+4h..8+4h+3 of the step).  Every branch here is wave-uniform: EXEC stays all ones.
    f32x16 o[MH_DT];
#pragma unroll
    for (int dt = 0; dt < MH_DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
    {
        typedef short s16x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
        const int grp = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
        const unsigned char* vb = Vs + (4 * hh + qq) * MH_VPITCH + 2 * (16 * (grp & 1) + 4 * pp);
#define MH_TR(KS_, DT_, HALF_) __builtin_amdgcn_ds_read_tr16_b64_v4i16(                          \
        (lds_s16x4)(vb + (16 * (KS_) + 8 * (HALF_)) * MH_VPITCH + 64 * (DT_)))
#pragma unroll
        for (int ks = 0; ks < 2 * NT; ++ks) {             // ks = 2 t + st: 16 keys per step
            const int t = ks >> 1, st = ks & 1;
            if (t <= tmax) {
                u32x4 vf[MH_DT];
#pragma unroll
                for (int dt = 0; dt < MH_DT; ++dt) {
                    const s16x4 x0 = MH_TR(ks, dt, 0), x1 = MH_TR(ks, dt, 1);
                    const uint2 u0 = __builtin_bit_cast(uint2, x0), u1 = __builtin_bit_cast(uint2, x1);
                    vf[dt] = u32x4{u0.x, u0.y, u1.x, u1.y};
                }
                u32x4 pk;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    pk[j] = Vec<ECOFLAP_F16>::f2h_pk(s[t][8 * st + 2 * j], s[t][8 * st + 2 * j + 1]);
                const f16x8 pf = __builtin_bit_cast(f16x8, pk);
#pragma unroll
                for (int dt = 0; dt < MH_DT; ++dt)
                    o[dt] = mh_mfma(__builtin_bit_cast(f16x8, vf[dt]), pf, o[dt]);
            }
        }
#undef MH_TR
    }
    if (q < N) {
        const float inv = 1.0f / l;
        _Float16* orow = obase + (int64_t)q * a.out_ts;
#pragma unroll
        for (int dt = 0; dt < MH_DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * dt + 8 * g + 4 * hh;
                uint2 w2;
                w2.x = Vec<ECOFLAP_F16>::f2h_pk(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv);
                w2.y = Vec<ECOFLAP_F16>::f2h_pk(o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
                *(uint2*)(orow + d) = w2;
            }
    }
}

// Workgroup g: heads (items) g * IPW .. g * IPW + IPW - 1 of the B * H; wave w: item w / NT of
// them, query tile w % NT.  One barrier: after the fill.
template <int NT, bool CAUSAL>
__global__ __launch_bounds__(64 * MhaCfg<NT>::WAVES) void mha_attention_kernel(const MhaArgs a) {
    constexpr int IPW = MhaCfg<NT>::IPW, WAVES = MhaCfg<NT>::WAVES, ROWS = MhaCfg<NT>::ROWS;
    constexpr int THREADS = 64 * WAVES;
    __shared__ __attribute__((aligned(16))) unsigned char Kb[IPW * ROWS * MH_KPITCH];
    __shared__ __attribute__((aligned(16))) unsigned char Vb[IPW * ROWS * MH_VPITCH];
    const int N = a.N, H = a.H;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // scalar: the branches on it are uniform
    const int nitems = a.B * H;
    const int item0 = (int)blockIdx.x * IPW;
    const int64_t HD = (int64_t)H * MH_D;
    // Rows past N: V's must be zero (their probabilities are, and 0 * garbage must stay 0); K's may
    // hold anything (those keys are masked by a select, not by arithmetic).
    {
        const u32x4 z = {0u, 0u, 0u, 0u};
        constexpr int VV = MH_VPITCH / 16;
#pragma unroll
        for (int li = 0; li < IPW; ++li)
            for (int i = N * VV + tid; i < ROWS * VV; i += THREADS) ((u32x4*)(Vb + li * ROWS * MH_VPITCH))[i] = z;
    }
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
                    *(u32x4*)(Vb + (li * ROWS + key) * MH_VPITCH + 16 * c) = vv[j];
                }
            }
        }
    }
    __syncthreads();
    const int li = wave / NT, qt = wave - li * NT;
    const int item = item0 + li;
    if (item < nitems && 32 * qt < N) {
        const int b = item / H, h = item - b * H;
        mha_tile<NT, CAUSAL>(a, Kb + li * ROWS * MH_KPITCH, Vb + li * ROWS * MH_VPITCH,
                             a.qkv + (int64_t)b * a.qkv_bs + (int64_t)h * MH_D,
                             a.out + (int64_t)b * a.out_bs + (int64_t)h * MH_D, qt, lane);
    }
}

template <int NT>
static int mha_launch(const MhaArgs& a, int causal, hipStream_t stream) {
    constexpr int IPW = MhaCfg<NT>::IPW, WAVES = MhaCfg<NT>::WAVES;
    const int nitems = a.B * a.H;
    const unsigned grid = (unsigned)((nitems + IPW - 1) / IPW);
    if (causal)
        hipLaunchKernelGGL((mha_attention_kernel<NT, true>), dim3(grid), dim3(64 * WAVES), 0, stream, a);
    else
        hipLaunchKernelGGL((mha_attention_kernel<NT, false>), dim3(grid), dim3(64 * WAVES), 0, stream, a);
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
