// attention_stream.h — the streaming (flash-style) sibling of attention_tile.h for heads whose K and
// V do not fit LDS: one wave owns a 32-query tile, key / value blocks of 64 pass through LDS, and
// the wave keeps a running maximum m, a running sum l and an un-normalised O per query.
// causal_attention.hip is its one user (head width 128).  attention_tile.h's instantiations do not
// pass through here: their sums and roundings are what they were.
//
// Orientation and fragments are attention_tile.h's: S^T = K Q^T on v_mfma_f32_32x32x16_f16 (a
// lane holds 16 keys of ONE query per tile, so a row reduction is in-lane plus one exchange with
// lane ^ 32), O^T = V^T P^T with V^T fragments by ds_read_b64_tr_b16 from a row-major V image,
// fp32 scores and sums, probabilities rounded to f16 for the second product.
//
// Per block, in this order (the textbook order: a block's probabilities are exponentiated only
// after the maximum that covers them is known, and O and l are rescaled on EVERY block, no
// deferred-rescale threshold):
//   m' = max(m, max of the block's scores);  alpha = exp2((m - m') c);  p = exp2((s - m') c)
//   l = l alpha + sum p;  O = O alpha + V^T f16(p)
// m starts at -inf and l, O at 0; a wave's first block always holds key 0, which no query masks,
// so m' is finite from the first block on and alpha = exp2(-inf) = 0 there, exactly.
#pragma once
#include "attention_tile.h"

#define AS_D 128                // head width
#define AS_DC 8                 // 16-wide chunks of the head dimension
#define AS_DT 4                 // 32-wide output tiles of the head dimension
#define AS_KEYS 64              // keys per block: two tiles of 32
#define AS_KPITCH 272           // bytes per K row in LDS: 16 * 17 (odd: a ds_read_b128 of 16 rows covers all banks once)
#define AS_VPITCH 320           // bytes per V row in LDS: 256 + 64 (4 consecutive rows x 64 B cover all banks once)
#define AS_KBYTES (AS_KEYS * AS_KPITCH)
#define AS_VBYTES (AS_KEYS * AS_VPITCH)

struct StreamState {
    float m, l;                 // running maximum (raw score) and sum of this lane's query
    f32x16 o[AS_DT];            // O^T, un-normalised: rows d = 32 dt + 8 g + 4 hh .. + 3, column = query
};

static __device__ __forceinline__ void stream_init(StreamState& st) {
    st.m = -__builtin_inff();
    st.l = 0.f;
#pragma unroll
    for (int dt = 0; dt < AS_DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) st.o[dt][i] = 0.f;
}

// One 64-key block for one wave.  TILES: how many of the block's two key tiles lie at or below
// the wave's diagonal (the others are neither multiplied nor exponentiated); DIAG: the last of
// them IS the diagonal tile and is masked in registers (key > query -> -inf, probability exactly
// 0).  Every branch is wave-uniform: EXEC stays all ones for the transposed reads.
//   Ks, Vs    the block's K image (rotated already, AS_KPITCH) and V image (AS_VPITCH); V rows
//             past the last token must be zero (0 * garbage must stay 0), K's may hold anything
//   qf        Q^T fragments of the wave's tile: chunk c = columns 16 c + 8 hh .. + 7 of query lane & 31
template <int TILES, bool DIAG>
static __device__ __forceinline__ void stream_block(const unsigned char* Ks, const unsigned char* Vs,
                                                    const f16x8 (&qf)[AS_DC], StreamState& st,
                                                    float scale_log2e, int lane) {
    const int r = lane & 31, hh = lane >> 5;
    f32x16 s[TILES];
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[t][i] = 0.f;
    {
        const unsigned char* krow = Ks + r * AS_KPITCH + 16 * hh;
        f16x8 kf[TILES];
#pragma unroll
        for (int t = 0; t < TILES; ++t) kf[t] = *(const f16x8*)(krow + 32 * t * AS_KPITCH);
#pragma unroll
        for (int c = 0; c < AS_DC; ++c) {
#pragma unroll
            for (int t = 0; t < TILES; ++t) {
                s[t] = mfma16(kf[t], qf[c], s[t]);
                if (c + 1 < AS_DC) kf[t] = *(const f16x8*)(krow + 32 * t * AS_KPITCH + 32 * (c + 1));
            }
            // (keeps the scheduler from hoisting every later chunk's loads up here: they spill)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // register i of a tile is key (i & 3) + 8 (i >> 2) + 4 hh of the tile; the query is r
    if constexpr (DIAG) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int key = (i & 3) + 8 * (i >> 2) + 4 * hh;
            s[TILES - 1][i] = key <= r ? s[TILES - 1][i] : -__builtin_inff();
        }
    }
    float mx[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) mx[i & 3] = __builtin_fmaxf(mx[i & 3], s[t][i]);
    float mb = __builtin_fmaxf(__builtin_fmaxf(mx[0], mx[1]), __builtin_fmaxf(mx[2], mx[3]));
    mb = __builtin_fmaxf(mb, __shfl_xor(mb, 32, 64));
    const float c2 = scale_log2e;
    const float mn = __builtin_fmaxf(st.m, mb), mc = mn * c2;
    const float alpha = __builtin_amdgcn_exp2f(st.m * c2 - mc);
    st.m = mn;
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < TILES; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float p = __builtin_amdgcn_exp2f(s[t][i] * c2 - mc);
            s[t][i] = p;
            ls[i & 3] += p;
        }
    float lb = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    lb += __shfl_xor(lb, 32, 64);
    st.l = st.l * alpha + lb;
#pragma unroll
    for (int dt = 0; dt < AS_DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) st.o[dt][i] *= alpha;
    // O^T += V^T P^T: 16-key steps, AS_DT independent accumulators each (attention_tile.h's
    // operand maps with this file's V pitch)
    typedef short s16x4 __attribute__((ext_vector_type(4)));
    typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
    const int grp = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
    const unsigned char* vb = Vs + (4 * hh + qq) * AS_VPITCH + 2 * (16 * (grp & 1) + 4 * pp);
#pragma unroll
    for (int ks = 0; ks < 2 * TILES; ++ks) {
        u32x4 vf[AS_DT];
#pragma unroll
        for (int dt = 0; dt < AS_DT; ++dt) {
            const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vb + 16 * ks * AS_VPITCH + 64 * dt));
            const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vb + (16 * ks + 8) * AS_VPITCH + 64 * dt));
            const uint2 u0 = __builtin_bit_cast(uint2, x0), u1 = __builtin_bit_cast(uint2, x1);
            vf[dt] = u32x4{u0.x, u0.y, u1.x, u1.y};
        }
        const int t = ks >> 1, h8 = 8 * (ks & 1);
        u32x4 pk;
#pragma unroll
        for (int j = 0; j < 4; ++j) pk[j] = Vec<ECOFLAP_F16>::f2h_pk(s[t][h8 + 2 * j], s[t][h8 + 2 * j + 1]);
        const f16x8 pf = __builtin_bit_cast(f16x8, pk);
#pragma unroll
        for (int dt = 0; dt < AS_DT; ++dt) st.o[dt] = mfma16(__builtin_bit_cast(f16x8, vf[dt]), pf, st.o[dt]);
        __builtin_amdgcn_sched_barrier(0);          // (the same for the V fragments of the later steps)
    }
}

// O / l, rounded once to f16, into the query's output row (four halves per store)
static __device__ __forceinline__ void stream_store(const StreamState& st, _Float16* orow, int lane) {
    const int hh = lane >> 5;
    const float inv = 1.0f / st.l;
#pragma unroll
    for (int dt = 0; dt < AS_DT; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            uint2 w2;
            w2.x = Vec<ECOFLAP_F16>::f2h_pk(st.o[dt][4 * g] * inv, st.o[dt][4 * g + 1] * inv);
            w2.y = Vec<ECOFLAP_F16>::f2h_pk(st.o[dt][4 * g + 2] * inv, st.o[dt][4 * g + 3] * inv);
            *(uint2*)(orow + 32 * dt + 8 * g + 4 * hh) = w2;
        }
}
