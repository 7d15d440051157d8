// lm_loss.hip — the causal language-model loss of a decoder (transformers' ForCausalLMLoss: labels
// padded by one ignore_index and shifted, flat cross entropy, mean) for gfx950, straight from the
// 16-bit logits the lm_head wrote.  Plumbing of the build's shape modules
// (include/ecoflap_shape_ops.h, shapes/llama.py), not part of the pruner ABI.
//
// The torch chain copies the logits to fp32 (read 2 B, write 4 B per logit) and runs log_softmax on
// the copy (read 4 B, write 4 B): 14 bytes of traffic per logit and a handful of launches for one
// scalar.  Here:
//
//   * one workgroup of 4 waves owns one row; every logit is read once, in 16-byte vectors, four
//     vectors in flight per lane; the shift is an index into `labels`, so no padded, sliced or
//     copied label tensor exists; a row without a target is not read at all;
//   * a lane keeps a running maximum m and s = sum(exp(x - m)) in fp32 and rescales s when a group
//     of up to 32 values raises m (online softmax: a 128256-wide row does not fit a lane's
//     registers, and a second pass would read the row twice); exp(d) is v_exp_f32 on d * log2(e);
//   * the target's logit is taken from the vector that holds it as it goes by;
//   * (m, s) pairs are merged over the wave by shuffles and over the four waves through LDS in a
//     fixed order; nll = log(s) + m - x_target;
//   * the ragged tail (vocab % 8 elements) is read element by element: nothing outside [0, vocab)
//     of a row is touched;
//   * a second launch of one workgroup adds row_loss over the rows that have a target, in fp64, in
//     an order that depends on the row count alone, and divides by their number (0 / 0 = NaN).
// No atomics, no host synchronisation, no allocation: capturable, repeatable bit for bit, and a
// row's loss does not depend on the rows that travel with it.
#include "common.h"
#include "../../include/ecoflap_shape_ops.h"

#define LM_THREADS 256
#define LM_WAVES (LM_THREADS / 64)
#define LM_UNROLL 4
#define LM_RED_THREADS 1024
#define LM_LOG2E 1.4426950408889634f

struct LmLossArgs {
    const void* logits;
    const int64_t* labels;
    float* row_loss;
    float* loss_out;
    int64_t tokens, vocab, stride, ignore_index, rows;
    int shift;
};

// 0: no target (last token under shift, or ignore_index), 1: target in [0, vocab), 2: out of range
static __device__ __forceinline__ int lm_target(const LmLossArgs& a, int64_t row, int64_t& target) {
    int64_t idx = row;
    if (a.shift) {
        const int64_t t = row % a.tokens;
        if (t + 1 >= a.tokens) return 0;
        idx = row + 1;
    }
    target = a.labels[idx];
    if (target == a.ignore_index) return 0;
    return (target >= 0 && target < a.vocab) ? 1 : 2;
}

// (m, s) <- (m, s) merged with (m2, s2); m, m2 finite or -FLT_MAX
static __device__ __forceinline__ void lm_merge(float& m, float& s, float m2, float s2) {
    const float mn = fmaxf(m, m2);
    s = s * __builtin_amdgcn_exp2f((m - mn) * LM_LOG2E) + s2 * __builtin_amdgcn_exp2f((m2 - mn) * LM_LOG2E);
    m = mn;
}

// element `sub` of a 16-byte vector of DT as fp32 (on the packed words: no indexed register array)
template <int DT>
static __device__ __forceinline__ float lm_pick(const u32x4& v, int sub) {
    const int w = sub >> 1;
    uint32_t x = v[0];
    x = w == 1 ? v[1] : x;
    x = w == 2 ? v[2] : x;
    x = w == 3 ? v[3] : x;
    x = (sub & 1) ? x >> 16 : x & 0xffffu;
    if constexpr (DT == ECOFLAP_F16) return Vec<ECOFLAP_F16>::h2f(x);
    else return __uint_as_float(x << 16);
}

template <int DT>
__global__ __launch_bounds__(LM_THREADS) void lm_row_loss_kernel(const LmLossArgs a) {
    __shared__ float ms[LM_WAVES], ss[LM_WAVES];
    __shared__ float xt_s;
    const int tid = threadIdx.x;
    const int64_t row = blockIdx.x;
    int64_t target = 0;
    const int kind = lm_target(a, row, target);     // uniform over the workgroup
    if (kind != 1) {
        if (tid == 0) a.row_loss[row] = kind == 0 ? 0.f : __builtin_nanf("");
        return;
    }
    const unsigned char* base = (const unsigned char*)a.logits + row * a.stride * 2;
    const int64_t nvec = a.vocab >> 3;
    const int64_t tvec = target >> 3;
    const int tsub = (int)(target & 7);

    float m = -__FLT_MAX__, s = 0.f;
    int64_t v = tid;
    for (; v + (LM_UNROLL - 1) * LM_THREADS < nvec; v += LM_UNROLL * LM_THREADS) {
        u32x4 raw[LM_UNROLL];
#pragma unroll
        for (int j = 0; j < LM_UNROLL; ++j) raw[j] = ld16(base, v + j * LM_THREADS);
        float f[LM_UNROLL][8];
        float vmax = m;
#pragma unroll
        for (int j = 0; j < LM_UNROLL; ++j) {
            Vec<DT>::unpack(raw[j], f[j]);
#pragma unroll
            for (int i = 0; i < 8; ++i) vmax = fmaxf(vmax, f[j][i]);
        }
        s *= __builtin_amdgcn_exp2f((m - vmax) * LM_LOG2E);
        m = vmax;
#pragma unroll
        for (int j = 0; j < LM_UNROLL; ++j) {
#pragma unroll
            for (int i = 0; i < 8; ++i) s += __builtin_amdgcn_exp2f((f[j][i] - m) * LM_LOG2E);
            if (v + j * LM_THREADS == tvec) xt_s = lm_pick<DT>(raw[j], tsub);
        }
    }
    for (; v < nvec; v += LM_THREADS) {
        const u32x4 raw = ld16(base, v);
        float f[8];
        Vec<DT>::unpack(raw, f);
        float vmax = m;
#pragma unroll
        for (int i = 0; i < 8; ++i) vmax = fmaxf(vmax, f[i]);
        s *= __builtin_amdgcn_exp2f((m - vmax) * LM_LOG2E);
        m = vmax;
#pragma unroll
        for (int i = 0; i < 8; ++i) s += __builtin_amdgcn_exp2f((f[i] - m) * LM_LOG2E);
        if (v == tvec) xt_s = lm_pick<DT>(raw, tsub);
    }
    // the ragged tail: one lane, element by element
    const int ntail = (int)(a.vocab & 7);
    if (ntail && tid == (int)(nvec % LM_THREADS)) {
        for (int i = 0; i < ntail; ++i) {
            const float x = Vec<DT>::load1(base, nvec * 8 + i);
            const float mn = fmaxf(m, x);
            s = s * __builtin_amdgcn_exp2f((m - mn) * LM_LOG2E) + __builtin_amdgcn_exp2f((x - mn) * LM_LOG2E);
            m = mn;
            if (nvec * 8 + i == target) xt_s = x;
        }
    }

#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const float m2 = __shfl_down(m, off, 64), s2 = __shfl_down(s, off, 64);
        lm_merge(m, s, m2, s2);
    }
    if ((tid & 63) == 0) {
        ms[tid >> 6] = m;
        ss[tid >> 6] = s;
    }
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < LM_WAVES; ++w) lm_merge(m, s, ms[w], ss[w]);
        a.row_loss[row] = logf(s) + m - xt_s;
    }
}

// loss_out[0] = sum(row_loss over rows with a target) / their number, one workgroup
__global__ __launch_bounds__(LM_RED_THREADS) void lm_mean_kernel(const LmLossArgs a) {
    __shared__ double sum_s[LM_RED_THREADS / 64];
    __shared__ long long cnt_s[LM_RED_THREADS / 64];
    const int tid = threadIdx.x;
    double sum = 0.0;
    long long cnt = 0;
    for (int64_t r = tid; r < a.rows; r += LM_RED_THREADS) {
        int64_t target;
        if (lm_target(a, r, target) != 0) {
            sum += (double)a.row_loss[r];
            ++cnt;
        }
    }
    sum = wave_sum(sum);
    cnt = wave_sum(cnt);
    if ((tid & 63) == 0) {
        sum_s[tid >> 6] = sum;
        cnt_s[tid >> 6] = cnt;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < LM_RED_THREADS / 64; ++w) {
            sum += sum_s[w];
            cnt += cnt_s[w];
        }
        a.loss_out[0] = (float)(sum / (double)cnt);
    }
}

extern "C" int ecoflap_causal_lm_loss(const void* logits, const int64_t* labels, float* row_loss,
                                      float* loss_out, int64_t batch, int64_t tokens, int64_t vocab,
                                      int64_t logits_row_stride, int64_t ignore_index, int shift,
                                      int dtype, void* stream) {
    if (!logits || !labels || !row_loss || !loss_out) return ECOFLAP_ENULL;
    if (dtype != ECOFLAP_F16 && dtype != ECOFLAP_BF16) return ECOFLAP_EDTYPE;
    if (batch < 0 || tokens < 0 || vocab < 0 || batch > 0x7fffffffLL || tokens > 0x7fffffffLL) return ECOFLAP_ESIZE;
    const int64_t rows = batch * tokens;
    if (rows > 0x7fffffffLL || (rows > 0 && vocab == 0) || logits_row_stride < vocab) return ECOFLAP_ESIZE;
    if (shift != 0 && shift != 1) return ECOFLAP_EMODE;
    if (!aligned16(logits) || (logits_row_stride & 7) || ((uintptr_t)labels & 7u) || ((uintptr_t)row_loss & 3u) ||
        ((uintptr_t)loss_out & 3u))
        return ECOFLAP_EALIGN;
    LmLossArgs a;
    a.logits = logits; a.labels = labels; a.row_loss = row_loss; a.loss_out = loss_out;
    a.tokens = tokens; a.vocab = vocab; a.stride = logits_row_stride; a.ignore_index = ignore_index;
    a.rows = rows; a.shift = shift;
    hipStream_t st = (hipStream_t)stream;
    if (rows > 0) {
        if (dtype == ECOFLAP_F16)
            hipLaunchKernelGGL((lm_row_loss_kernel<ECOFLAP_F16>), dim3((unsigned)rows), dim3(LM_THREADS), 0, st, a);
        else
            hipLaunchKernelGGL((lm_row_loss_kernel<ECOFLAP_BF16>), dim3((unsigned)rows), dim3(LM_THREADS), 0, st, a);
        ECO_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(lm_mean_kernel, dim3(1), dim3(LM_RED_THREADS), 0, st, a);    // rows == 0: writes NaN
    ECO_CHECK_LAUNCH();
    return 0;
}
