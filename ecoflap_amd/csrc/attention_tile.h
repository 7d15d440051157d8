// attention_tile.h — one 32-query tile of softmax(Q K^T * scale) V on gfx950: the arithmetic both
// attention kernels of the build run (attention.hip: ViT-g; mha_attention.hip: the CLIP towers).
// The kernels differ in what they put into LDS and in who runs which tile; a tile's sums, their
// order and its rounding are this file's alone.
#pragma once
#include "common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define AT_VPITCH 192           // bytes per V row in LDS (96 halves: 4 consecutive rows x 64 B cover all banks once)

static __device__ __forceinline__ f32x16 mfma16(f16x8 a, f16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// Rows N .. rows - 1 of a V image: V's must be zero (their probabilities are, and 0 * garbage must
// stay 0); K's may hold anything readable (those keys are masked by a select, not by arithmetic).
static __device__ __forceinline__ void at_zero_v_tail(unsigned char* Vs, int N, int rows, int tid, int threads) {
    const u32x4 z = {0u, 0u, 0u, 0u};
    for (int i = N * (AT_VPITCH / 16) + tid; i < rows * (AT_VPITCH / 16); i += threads) ((u32x4*)Vs)[i] = z;
}

// One 32-query tile (`qt`, wave-uniform) of one (sample, head): S^T = K Q^T, mask, exact softmax,
// O^T = V^T P^T, store.
//   NT                key / query tiles of 32 (the images hold 32 * NT rows); DC: 16-wide chunks,
//                     DT: 32-wide output tiles of the head dimension; CAUSAL: keys <= query only
//   Ks, kpitch        K image in LDS, row pitch in bytes (16 * odd: a ds_read_b128 of 16
//                     consecutive rows covers all 64 banks once); Vs: V image, AT_VPITCH
//   qbase, q_ts       q of (sample, token 0, head) and the token stride in elements; obase, o_ts:
//                     the same for the output row
//   N, D              tokens, head width (D % 8 == 0, D <= 16 * DC)
//   debug             phase-ablation word of tools/attention_launches.py (2: no QK^T, 4: no
//                     softmax, 8: no PV, 16: no store)
//   sqw               COLSQ only: 32 * DT floats (LDS) that receive, per column d of the head, the
//                     sum over this tile's queries < N of (float)(f16-rounded O[q, d])^2 — the
//                     sum of squares of exactly the values the store writes; obase may then be
//                     null (wave-uniform): nothing is stored
// A caller that passes constants for D, kpitch and debug pays for none of their selects.
// PREFETCH_V picks the schedule of the V fragment loads (below), not the arithmetic.  COLSQ adds
// an epilogue and changes nothing before it: the instantiations without it are what they were.
template <int NT, int DC, int DT, bool CAUSAL, bool PREFETCH_V, bool COLSQ = false>
static __device__ __forceinline__ void attention_tile(const unsigned char* Ks, const unsigned char* Vs,
                                                      int kpitch, const _Float16* qbase, int64_t q_ts,
                                                      _Float16* obase, int64_t o_ts, int N, int D,
                                                      float scale_log2e, int debug, int qt, int lane,
                                                      float* sqw = nullptr) {
    const int r = lane & 31, hh = lane >> 5;
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const int q = 32 * qt + r;
    const int qc = q < N ? q : N - 1;
    const int tmax = CAUSAL ? qt : NT - 1;          // last key tile this query tile attends to
    // Q^T fragments (B operand: k = d on the half-lanes, column = query on the lanes)
    f16x8 qf[DC];
#pragma unroll
    for (int c = 0; c < DC; ++c) {
        const int d0 = 16 * c + 8 * hh;
        qf[c] = d0 < D ? *(const f16x8*)(qbase + (int64_t)qc * q_ts + d0) : zero8;
    }
    // S^T = K Q^T: tile t holds keys 32t .. 32t+31 (rows, in the registers) x 32 queries (lanes).
    // d-chunk outermost: up to NT INDEPENDENT accumulators per step (no MFMA waits for the one
    // before it); a K fragment's register is reloaded for the next chunk as soon as its product
    // has issued (with one or two waves per SIMD nobody else hides the LDS latency).  Every tile
    // up to tmax is computed whatever N is (keys past N are masked below); causal: the tiles
    // wholly above the diagonal are neither multiplied nor exponentiated.
    f32x16 s[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int i = 0; i < 16; ++i) s[t][i] = 0.f;
    if (!(debug & 2)) {
        const unsigned char* krow = Ks + r * kpitch + 16 * hh;
        f16x8 kf[NT];
#pragma unroll
        for (int t = 0; t < NT; ++t)
            if (t <= tmax) kf[t] = *(const f16x8*)(krow + 32 * t * kpitch);
#pragma unroll
        for (int c = 0; c < DC; ++c) {
            const bool live = 16 * c + 8 * hh < D;      // (a row's last chunk may be half padding)
#pragma unroll
            for (int t = 0; t < NT; ++t) {
                if (t <= tmax) {
                    s[t] = mfma16(live ? kf[t] : zero8, qf[c], s[t]);
                    if (c + 1 < DC) kf[t] = *(const f16x8*)(krow + 32 * t * kpitch + 32 * (c + 1));
                }
            }
            // (keeps the scheduler from hoisting every later chunk's loads up here: they spill)
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // exact softmax over the keys of this lane's query: own registers, then lane ^ 32.  Four
    // independent chains for the maximum and for the sum (a serial chain of 16 * NT dependent ops
    // would expose every VALU latency).  Register i of tile t is key 32 t + (i & 3) + 8 (i >> 2) +
    // 4 hh.  A masked entry's probability is exp2(-inf) = 0 exactly; key 0 is never masked, so m
    // is finite.
    float mx[4] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    if (!(debug & 4)) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t <= tmax) {
                if (32 * t + 32 > N || (CAUSAL && t == qt)) {      // uniform: the tile(s) reaching past N, the diagonal tile
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
    }
    float m = __builtin_fmaxf(__builtin_fmaxf(mx[0], mx[1]), __builtin_fmaxf(mx[2], mx[3]));
    m = __builtin_fmaxf(m, __shfl_xor(m, 32, 64));
    const float c2 = scale_log2e, mc = m * c2;
    float ls[4] = {0.f, 0.f, 0.f, 0.f};
    if (!(debug & 4)) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
            if (t <= tmax) {
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float p = __builtin_amdgcn_exp2f(s[t][i] * c2 - mc);
                    s[t][i] = p;
                    ls[i & 3] += p;
                }
            }
        }
    }
    float l = (ls[0] + ls[1]) + (ls[2] + ls[3]);
    l += __shfl_xor(l, 32, 64);
    // O^T = V^T P^T, DT independent accumulators per 16-key step ks = 2 t + st.  The B operand is
    // P tile t, registers 8 st .. 8 st + 7 of s[t], as they stand (rounded to f16).  V stays
    // row-major in LDS; its transposed A fragments come from ds_read_b64_tr_b16: lane 4q+p of a
    // 16-lane group addresses row q, columns 4p..4p+3 of a 4-key x 16-column block and receives
    // column (lane & 15) of the 4 keys - exactly the MFMA's k order (keys 4h..4h+3 and
    // 8+4h..8+4h+3 of the step).  Every branch here is wave-uniform: EXEC stays all ones.
    f32x16 o[DT];
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.f;
    if (!(debug & 8)) {
        typedef short s16x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
        const int grp = lane >> 4, qq = (lane & 15) >> 2, pp = lane & 3;
        const unsigned char* vb = Vs + (4 * hh + qq) * AT_VPITCH + 2 * (16 * (grp & 1) + 4 * pp);
        auto load_v = [&](u32x4 (&vf)[DT], int ks) {
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) {
                const s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vb + 16 * ks * AT_VPITCH + 64 * dt));
                const s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(vb + (16 * ks + 8) * AT_VPITCH + 64 * dt));
                const uint2 u0 = __builtin_bit_cast(uint2, x0), u1 = __builtin_bit_cast(uint2, x1);
                vf[dt] = u32x4{u0.x, u0.y, u1.x, u1.y};
            }
        };
        auto step = [&](const u32x4 (&vf)[DT], int ks) {
            const int t = ks >> 1, st = ks & 1;
            u32x4 pk;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                pk[j] = Vec<ECOFLAP_F16>::f2h_pk(s[t][8 * st + 2 * j], s[t][8 * st + 2 * j + 1]);
            const f16x8 pf = __builtin_bit_cast(f16x8, pk);
#pragma unroll
            for (int dt = 0; dt < DT; ++dt) o[dt] = mfma16(__builtin_bit_cast(f16x8, vf[dt]), pf, o[dt]);
        };
        // Two schedules of the same loads and products.  ViT-g double-buffers the fragments (the
        // loads of step ks + 1 issue before the products of step ks).  The CLIP instances load
        // inside the step: double-buffered, <4, causal> goes from 156 to 172 VGPRs (3 -> 2 waves
        // per SIMD) and <3, causal> from 85 to 130.  Merging the two is a performance question.
        if constexpr (PREFETCH_V) {
            u32x4 vf[2][DT];
            load_v(vf[0], 0);
#pragma unroll
            for (int ks = 0; ks < 2 * NT; ++ks) {
                if (ks + 1 < 2 * NT && ((ks + 1) >> 1) <= tmax) load_v(vf[(ks + 1) & 1], ks + 1);
                if ((ks >> 1) <= tmax) step(vf[ks & 1], ks);
                if ((ks & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        } else {
#pragma unroll
            for (int ks = 0; ks < 2 * NT; ++ks) {
                if ((ks >> 1) <= tmax) {
                    u32x4 vf[DT];
                    load_v(vf, ks);
                    step(vf, ks);
                }
            }
        }
    }
    if constexpr (COLSQ) {
        // The store's own packed halves, squared in fp32 and summed over the tile's 32 queries:
        // a butterfly over lane bits 0 .. 4 (the half-lanes hold different columns and stay
        // apart) — every lane ends with the same sum, added in an order that depends on nothing
        // but the lane numbers.  Queries >= N contribute +0.  All 64 lanes take part (the
        // exchanges sit outside the q < N branch).
        typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
        const bool liveq = q < N;
        const bool store = obase != nullptr;
        const float inv = 1.0f / l;
        _Float16* orow = obase + (int64_t)q * o_ts;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * dt + 8 * g + 4 * hh;
                uint2 w2;
                w2.x = Vec<ECOFLAP_F16>::f2h_pk(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv);
                w2.y = Vec<ECOFLAP_F16>::f2h_pk(o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
                if (store && liveq && d < D) *(uint2*)(orow + d) = w2;
                const h2_t a = __builtin_bit_cast(h2_t, w2.x), b = __builtin_bit_cast(h2_t, w2.y);
                float v[4] = {(float)a[0], (float)a[1], (float)b[0], (float)b[1]};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    v[j] = (liveq && d < D) ? v[j] * v[j] : 0.f;
#pragma unroll
                    for (int m_ = 1; m_ < 32; m_ <<= 1) v[j] += __shfl_xor(v[j], m_, 64);
                }
                if (r == 0) *(float4*)(sqw + d) = float4{v[0], v[1], v[2], v[3]};
            }
        return;
    }
    // lane (r, hh) holds O^T rows d = 32 dt + 8 g + 4 hh .. + 3 of its query: four halves per store
    if (q < N && !(debug & 16)) {
        const float inv = 1.0f / l;
        _Float16* orow = obase + (int64_t)q * o_ts;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int d = 32 * dt + 8 * g + 4 * hh;
                if (d < D) {
                    uint2 w2;
                    w2.x = Vec<ECOFLAP_F16>::f2h_pk(o[dt][4 * g] * inv, o[dt][4 * g + 1] * inv);
                    w2.y = Vec<ECOFLAP_F16>::f2h_pk(o[dt][4 * g + 2] * inv, o[dt][4 * g + 3] * inv);
                    *(uint2*)(orow + d) = w2;
                }
            }
    }
}
