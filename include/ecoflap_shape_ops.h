/*
 * ecoflap_shape_ops.h — fused forward ops of the synthetic shape modules (plumbing).
 *
 * NOT part of the pruner drop-in boundary (that is ecoflap_hip.h).  The scoring loop is
 * forward-bound, and a third of a BLIP-2-shaped forward's GPU time was eight-kernel
 * RMSNorm chains and other element-wise glue; these entry points fuse them for the
 * build's own shape modules (ecoflap_amd/shapes/).  Same conventions as ecoflap_hip.h.
 */
#ifndef ECOFLAP_SHAPE_OPS_H
#define ECOFLAP_SHAPE_OPS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* T5LayerNorm (LAVIS/lavis/models/blip2_models/modeling_t5.py:239-262):
 *   var = mean(float(x)^2); h = bf16/f16(x * rsqrt(var + eps)); y = w * h
 * x, y: [rows, d] of `dtype` (F16/BF16), w: [d] of `dtype`; d % 8 == 0. */
int ecoflap_t5_rmsnorm(const void* x, const void* w, void* y, int64_t rows, int64_t d,
                       float eps, int dtype, void* stream);
/* The same preceded by the residual add that produces its input (T5 block: h = x + sublayer(x),
 * then the NEXT sublayer's norm of h): sum_out = dtype(x + residual), y = rmsnorm(sum_out) * w —
 * the bits of the separate add and norm, one pass instead of two. */
int ecoflap_t5_add_rmsnorm(const void* x, const void* residual, const void* w, void* sum_out, void* y,
                           int64_t rows, int64_t d, float eps, int dtype, void* stream);

/* gated GELU of T5DenseGatedActDense (modeling_t5.py:296-330): y = gelu(a) * b
 * (erf GELU in fp32, rounded to dtype, then the product rounded to dtype). n % 8 == 0. */
int ecoflap_gelu_mul(const void* a, const void* b, void* y, int64_t n, int dtype, void* stream);

/* SwiGLU of the LLaMA MLP (transformers' LlamaMLP: act_fn(gate_proj(x)) * up_proj(x)):
 * y = dtype(dtype(silu(a)) * b), silu(a) = a / (1 + exp(-a)) in fp32 (a * exp(a / 2) * exp(a / 2)
 * where exp(-a) overflows, a < -88.7).  F16 / BF16; n % 8 == 0. */
int ecoflap_silu_mul(const void* a, const void* b, void* y, int64_t n, int dtype, void* stream);

/* nn.LayerNorm on a 16-bit activation under autocast (EVA ViT blocks,
 * LAVIS/lavis/models/eva_vit.py:160-184): fp32 statistics and fp32 affine parameters, 16-bit
 * in and out; with `residual` the block's residual add is fused in front:
 *   s = dtype(x + residual) -> sum_out;  y = dtype((float(s) - mean) * rstd * w + b)
 * x, residual, sum_out, y: [rows, d] of `dtype` (F16/BF16); w, b: [d] float; d % 8 == 0.
 * residual == NULL: plain LayerNorm of x (sum_out unused).  Every pointer, w and b included, is
 * read or written in 16-byte vectors: ECOFLAP_EALIGN otherwise (ecoflap_add_bias_layernorm and
 * ecoflap_qkv_bias_add below too). */
int ecoflap_add_layernorm(const void* x, const void* residual, const float* w, const float* b,
                          void* sum_out, void* y, int64_t rows, int64_t d, float eps, int dtype,
                          void* stream);

/* The consumers of a Linear output that arrives WITHOUT its bias (the pinned GEMM solutions of
 * libecoflap_gemm.so have no bias epilogue on gfx950: every bias-epilogue solution of the library
 * there is a Stream-K kernel).  `bias` is the Linear's own bias, [d] of `dtype`; the first step is
 * always dtype(out + bias), the value the Linear would have returned from a rounded accumulator:
 *   ecoflap_add_bias_layernorm: ecoflap_add_layernorm with residual' = dtype(residual + bias)
 *   ecoflap_bias_gelu:          y = dtype(gelu(dtype(a + bias)))        (erf GELU, EVA Mlp)
 *   ecoflap_bias_add_residual:  y = dtype(x + dtype(m + bias))          (EVA Block's MLP residual) */
int ecoflap_add_bias_layernorm(const void* x, const void* residual, const void* residual_bias,
                               const float* w, const float* b, void* sum_out, void* y,
                               int64_t rows, int64_t d, float eps, int dtype, void* stream);
int ecoflap_bias_gelu(const void* a, const void* bias, void* y, int64_t rows, int64_t d, int dtype,
                      void* stream);
int ecoflap_bias_add_residual(const void* x, const void* m, const void* bias, void* y, int64_t rows,
                              int64_t d, int dtype, void* stream);

/* EVA attention bias (eva_vit.py:123-128): qkv += cat(q_bias, zeros, v_bias).to(dtype), in
 * place; qkv: [rows, 3*dim] of `dtype` (F16/BF16), q_bias / v_bias: [dim] float; dim % 8 == 0.
 * (The pinned-forward qkv Linear of shapes/eva_vit.py adds this bias in its GEMM's epilogue
 * instead; this pass serves the other cases.) */
int ecoflap_qkv_bias_add(void* qkv, const float* q_bias, const float* v_bias, int64_t rows,
                         int64_t dim, int dtype, void* stream);

/* Multi-head self-attention of the EVA ViT blocks (LAVIS/lavis/models/eva_vit.py:119-141 without
 * the relative position bias BLIP-2's tower does not use): out = softmax(q k^T * scale) v per
 * (image, head).  qkv: [batch, tokens, 3, heads, head_dim] of F16 as the qkv Linear wrote it;
 * out: [batch, tokens, heads * head_dim].  tokens <= 288, head_dim <= 96 and a multiple of 8.
 * fp32 scores / softmax, probabilities rounded to f16 for the second product. */
int ecoflap_vit_attention(const void* qkv, void* out, int64_t batch, int64_t tokens,
                          int64_t heads, int64_t head_dim, float scale, int dtype, void* stream);

/* ecoflap_vit_attention on the kernel's previous schedule (one 4-wave workgroup per CU): the
 * same shapes and the same output bits; kept as the reference of the bitwise tests. */
int ecoflap_vit_attention_v1(const void* qkv, void* out, int64_t batch, int64_t tokens,
                             int64_t heads, int64_t head_dim, float scale, int dtype, void* stream);

/* Multi-head self-attention of the OpenAI-CLIP towers (CoOp/clip/model.py:167-188: the
 * nn.MultiheadAttention of a ResidualAttentionBlock between its in- and out-projection), and of
 * any tower of that shape family: out = softmax(q k^T * scale [+ causal mask]) v per (sample, head)
 * (csrc/mha_attention.hip).  qkv is the in-projection's output read in place: the row of (sample b,
 * token n) starts at qkv + b * qkv_batch_stride + n * qkv_token_stride (elements) and holds
 * [3, heads, head_dim]; out's row of (b, n) starts at out + b * out_batch_stride + n *
 * out_token_stride and receives the merged heads [heads, head_dim] — so [L, N, 3D] (sequence
 * first) and [N, L, 3D] both work without a copy.  causal != 0: key j > query i is masked
 * (probability exactly 0).  F16 only (else ECOFLAP_EDTYPE); head_dim == 64, 1 <= tokens <= 224,
 * finite scale > 0, token strides at least a row (else ECOFLAP_ESIZE); pointers 16-byte aligned
 * and every stride a multiple of 8 elements (else ECOFLAP_EALIGN).  fp32 scores / exact two-pass
 * softmax, probabilities rounded to f16 for the second product; each (sample, head) is computed
 * independently of the others (batch invariant bit for bit).  Nothing is launched on an error. */
int ecoflap_mha_attention(const void* qkv, void* out, int64_t batch, int64_t tokens, int64_t heads,
                          int64_t head_dim, int64_t qkv_token_stride, int64_t qkv_batch_stride,
                          int64_t out_token_stride, int64_t out_batch_stride, int causal,
                          float scale, int dtype, void* stream);

/* The NON-causal ecoflap_mha_attention with the Wanda column statistic of its output as an epilogue
 * (CoOp/trainers/pruners/wanda_pruner.py:69-104 + :159-172 + :311-313 + :334-341: the side copy
 * `hacky_attn` of a CLIP block, which has no mask in either tower, hooked at its `proj`, whose
 * input goes through WrappedGPT's `torch.norm(inp.float(), p=2, dim=1) ** 2`):
 *   sq[h * 64 + d] = sum over all batch * tokens rows of (float)(f16-rounded out[row, h, d])^2
 * sq: [heads * 64] fp32 on the device, overwritten.  out MAY be null: the output is then never
 * stored (the text tower, whose real forward is causal: the unmasked output exists only to be
 * reduced); given, it receives the bits ecoflap_mha_attention(causal = 0) writes (the out strides
 * are ignored when out is null).  workspace: caller-owned, at least
 * ecoflap_mha_attention_colsq_workspace_bytes(batch, heads) bytes, 16-byte aligned, overwritten; it
 * needs no initialisation and carries nothing between calls.  No atomics: per-wave, per-workgroup
 * and per-sample partial sums are added in an order fixed by the shape, so sq is bitwise
 * repeatable and does not depend on the launch schedule; query rows >= tokens contribute nothing.
 * Launches only (no synchronisation, no allocation): usable inside a captured graph.  Shape limits
 * and error codes of ecoflap_mha_attention; a short workspace is ECOFLAP_ESIZE.  Nothing is launched
 * on an error. */
size_t ecoflap_mha_attention_colsq_workspace_bytes(int64_t batch, int64_t heads);
int ecoflap_mha_attention_colsq(const void* qkv, void* out, float* sq, void* workspace,
                                size_t workspace_bytes, int64_t batch, int64_t tokens, int64_t heads,
                                int64_t head_dim, int64_t qkv_token_stride, int64_t qkv_batch_stride,
                                int64_t out_token_stride, int64_t out_batch_stride, float scale,
                                int dtype, void* stream);

/* Causal self-attention of a LLaMA decoder block (transformers' LlamaAttention, eager path, between
 * the q / k / v projections and o_proj), rotary embedding included (csrc/causal_attention.hip):
 *   out = softmax(rot(q) rot(k)^T * scale + causal mask) v   per (sample, head)
 * Key j > query i has probability exactly 0.  The row of (sample b, token n) of q, k and v starts at
 * ptr + b * qkv_batch_stride + n * qkv_token_stride (elements) and holds [heads, 128]: the three
 * Linears' outputs are read in place, as three tensors or as three slices of one; out's row of
 * (b, n) starts at out + b * out_batch_stride + n * out_token_stride and receives the merged heads
 * [heads, 128].  rot is the rotate_half form (element d pairs with d + 64, NOT the interleaved form):
 *   rot(x)[d] = x[d] cos[n, d] - x[d + 64] sin[n, d],  rot(x)[d + 64] = x[d + 64] cos[n, d] + x[d] sin[n, d]
 * with token n's row of rope_cos / rope_sin, [tokens, 64] fp32 on the device (positions 0 ..
 * tokens - 1, no KV cache; rope_theta and scaling variants are the caller's); multiplied in fp32,
 * rotated q and k rounded once to f16, no rotated copy in memory.  Both table pointers NULL: no
 * rotation; one alone: ECOFLAP_ENULL.  Grouped-query attention (kv_heads != heads) is served by
 * ecoflap_causal_attention_gqa below; this entry is that one with kv_heads = heads, one head per
 * workgroup and q's strides for k / v.
 * F16 only (else ECOFLAP_EDTYPE); head_dim == 128, 1 <= tokens <= 4096, batch, heads > 0, batch *
 * heads * ceil(tokens / 32) < 2^31, finite scale > 0, token strides at least a row, batch strides
 * >= 0 (else ECOFLAP_ESIZE); pointers 16-byte aligned and every stride a multiple of 8 elements
 * (else ECOFLAP_EALIGN).  Flash-style: key / value blocks of 64 stream through LDS, running
 * maximum and sum per query with a rescale on every block (no deferred-rescale threshold), fp32
 * scores and sums, probabilities rounded to f16 for the second product; key blocks above the
 * diagonal are skipped.  No atomics; every (sample, head, 256-query block) is computed
 * independently (batch invariant bit for bit).  Nothing is launched on an error. */
int ecoflap_causal_attention(const void* q, const void* k, const void* v, void* out,
                             const float* rope_cos, const float* rope_sin, int64_t batch,
                             int64_t tokens, int64_t heads, int64_t head_dim,
                             int64_t qkv_token_stride, int64_t qkv_batch_stride,
                             int64_t out_token_stride, int64_t out_batch_stride, float scale,
                             int dtype, void* stream);

/* ecoflap_causal_attention with grouped-query attention (Llama-2-70B, Llama-3, Mistral: fewer key /
 * value heads than query heads).  A q / out row holds [heads, 128] as above; a k / v row holds
 * [kv_heads, 128] and starts at ptr + b * kv_batch_stride + n * kv_token_stride (strides of their
 * own: the k / v projections are narrower tensors, or slices of one fused buffer).  Query head h
 * reads KV head h / (heads / kv_heads): transformers' repeat_kv order.  No expanded copy of K / V
 * exists anywhere.
 * heads_per_workgroup (P), with G = heads / kv_heads: one of 1, 2, 4, 8 and a divisor of G; 0 means
 * the build's choice, ecoflap_causal_attention_gqa_default_p(G): 1 for every G, by measurement
 * (profiles/r17_llama_gqa: no larger P was faster beyond the run-to-run spread).  A workgroup of 8 waves serves P
 * query heads of one KV group times 8 / P query tiles of 32 (256 / P consecutive queries): a K / V
 * block is fetched, rotated and staged in LDS once for P heads.  P changes the schedule only: the
 * output of every (sample, head, 32-query tile) is bit for bit what ecoflap_causal_attention writes
 * for that head on K / V expanded to `heads` heads in memory, for every valid P.
 * Everything else is ecoflap_causal_attention's contract (F16 only, head_dim == 128, 1 <= tokens <=
 * 4096, both rope pointers or neither, 16-byte pointers, every stride a multiple of 8 elements, no
 * atomics, batch invariant bit for bit) and its error codes in its order; in addition ECOFLAP_ESIZE
 * for kv_heads < 1, heads % kv_heads != 0, an invalid heads_per_workgroup and a kv token stride
 * below kv_heads * 128 (the grid is at most batch * heads * ceil(tokens / 32) < 2^31 workgroups).
 * Nothing is launched on an error. */
int ecoflap_causal_attention_gqa(const void* q, const void* k, const void* v, void* out,
                                 const float* rope_cos, const float* rope_sin, int64_t batch,
                                 int64_t tokens, int64_t heads, int64_t kv_heads, int64_t head_dim,
                                 int64_t q_token_stride, int64_t q_batch_stride,
                                 int64_t kv_token_stride, int64_t kv_batch_stride,
                                 int64_t out_token_stride, int64_t out_batch_stride, float scale,
                                 int heads_per_workgroup, int dtype, void* stream);

/* What heads_per_workgroup == 0 stands for at group size G = heads / kv_heads (0 for G < 1). */
int ecoflap_causal_attention_gqa_default_p(int64_t group);

/* The causal language-model loss of a decoder, from the 16-bit logits its lm_head wrote
 * (transformers' ForCausalLMLoss: labels padded by one ignore_index and shifted, flat fp32 cross
 * entropy, mean; csrc/lm_loss.hip).  logits: [batch * tokens, vocab] of F16 / BF16, row r at
 * logits + r * logits_row_stride elements (the lm_head output, or a column slice of a wider buffer,
 * read in place); labels: [batch, tokens] int64, contiguous.  shift = 1: the target of row (b, t) is
 * labels[b, t + 1] and the last token of every sample has none; shift = 0: labels[b, t].
 *   row_loss[r] = -log_softmax(float(logits[r]))[target] in fp32 (maximum, sum(exp(x - max)) and
 *     the target's logit in fp32, nll = log(sum) + max - x_target); exactly 0 where the row has no
 *     target or the target equals ignore_index (such a row is not read).  [batch * tokens], caller-owned.
 *   loss_out[0] = (sum of row_loss over the rows with a target) / (their number); NaN when there is
 *     none, as F.cross_entropy(reduction="mean") answers.
 * A target that is neither ignore_index nor in [0, vocab) makes its row's loss and the mean NaN
 * (torch raises a device-side assert there); nothing outside [0, vocab) of any row is ever read,
 * whatever the labels hold.  Every logit is read once, in 16-byte vectors (a ragged tail of vocab % 8
 * elements one by one); any vocab >= 1.  The mean is a second one-workgroup launch adding row_loss in
 * fp64 in an order fixed by batch * tokens alone: no atomics, the same bits on every call, and a
 * row's loss does not depend on the other rows (batch invariant bit for bit).  Launches only (no
 * synchronisation, no allocation, no host read of labels): usable inside a captured graph.
 * ECOFLAP_ENULL: a null logits, labels, row_loss or loss_out; ECOFLAP_EDTYPE: not F16 / BF16;
 * ECOFLAP_ESIZE: batch, tokens or vocab < 0, vocab == 0 with rows, logits_row_stride < vocab, or
 * batch * tokens >= 2^31; ECOFLAP_EMODE: shift not 0 or 1; ECOFLAP_EALIGN: logits not 16-byte
 * aligned, logits_row_stride % 8 != 0, or labels / row_loss / loss_out not aligned to their element.
 * Nothing is launched on an error.  batch * tokens == 0: returns 0, loss_out[0] = NaN, nothing read. */
int ecoflap_causal_lm_loss(const void* logits, const int64_t* labels, float* row_loss, float* loss_out,
                           int64_t batch, int64_t tokens, int64_t vocab, int64_t logits_row_stride,
                           int64_t ignore_index, int shift, int dtype, void* stream);

/* Up to ECOFLAP_COPY_MAX_ITEMS device-to-device copies (non-overlapping, any alignment) in
 * one launch: the loop's state hand-overs between static graph buffers. */
#define ECOFLAP_COPY_MAX_ITEMS 32
typedef struct {
    void* dst;
    const void* src;
    int64_t bytes;
} ecoflap_copy_item;
int ecoflap_multi_copy(const ecoflap_copy_item* items, int n, void* stream);
/* Bitwise comparison of up to ECOFLAP_COPY_MAX_ITEMS pairs (dst vs src of each item) in one
 * launch: *mismatch_flag |= 1 when any byte differs (the caller zeroes it). */
int ecoflap_multi_compare(const ecoflap_copy_item* items, int n, int* mismatch_flag, void* stream);

/* y[M,N] = x[M,K] W[N,K]^T (+ bias[N]) in fp32 on v_mfma_f32_32x32x2_f32 (csrc/gemm_f32.hip): the
 * forward's fp32 Linears (BLIP-2's Q-Former), for which hipBLASLt has only Stream-K solutions on
 * gfx950.  Every output element is one fp32 accumulation chain in a fixed k order, the bias added
 * last: a row's result does not depend on the rows that travel with it, nor on M.  N % 128 == 0, K % 32 == 0 (else
 * ECOFLAP_ESIZE: the caller keeps the framework's GEMM); x, w 16-byte aligned. */
int ecoflap_linear_f32(const float* x, const float* w, const float* bias, float* y, int64_t M,
                       int64_t N, int64_t K, void* stream);

/* ---- libecoflap_gemm.so (csrc/gemm_pinned.hip) ------------------------------------------------
 * y[M,N] = x[M,K] W[N,K]^T (+ bias[N]) for F16 / BF16 (fp32 accumulation) through hipBLASLt with
 * the SOLUTION PINNED per (N, K, dtype, bias): chosen once, among the library's own candidates
 * for the weight shape, by name (no Stream-K, no K split over workgroups) and by measurement
 * (same bits on a repeated call; the probe problem alone == its first and its last slot of a
 * 16-slot problem), then used for every M.  One macro tile and one K order for every row count:
 * a row's result does not depend on how many rows travel with it (batch invariance by
 * construction) nor on an environment variable of the library.
 *
 * ecoflap_linear_pinned_plan: choose (or look up) the plan; allocates and synchronises, so call
 *   it OUTSIDE stream capture, before the first ecoflap_linear_pinned of that weight shape.
 *   m_probe = a row count the loop uses (the check runs at m_probe and 16 * m_probe).
 *   -> 0 and the solution's index / name (the lowest index among the survivors: no timing enters
 *   the choice), its time on the 16-slot problem (best_us)
 *   and, for the record, the time of the library's own first choice on the same data
 *   (default_us), or ECOFLAP_ESIZE when no candidate survived.
 *   Bias: gfx950's bias-epilogue solutions are all Stream-K kernels, so the solution is a
 *   no-bias one; ecoflap_linear_pinned with a bias prefills the output with the bias rows and runs
 *   beta = 1 (one extra write + read of the output); the shape modules instead leave the bias to
 *   the op that consumes the output (ecoflap_add_bias_layernorm / _bias_gelu / _bias_add_residual).
 * ecoflap_linear_pinned: the product; launches only (safe under capture once planned and once
 *   called with this M).  bias_dtype: dtype code of `bias` (the Linear's own dtype, or F32).
 *   workspace: >= 64 MiB recommended (the pinned solutions take none or little).
 *   ECOFLAP_EMODE: no plan for this weight shape. */
int ecoflap_linear_pinned_plan(int64_t m_probe, int64_t N, int64_t K, int dtype, int has_bias,
                               int bias_dtype, int* solution_index, int* tried, int* passed,
                               float* best_us, float* default_us, char* name_out, int name_len);
int ecoflap_linear_pinned(const void* x, const void* w, const void* bias, void* y, int64_t M,
                          int64_t N, int64_t K, int dtype, int bias_dtype, void* workspace,
                          size_t workspace_bytes, void* stream);
/* Measurement only (tools/tune_gemm.py): every solution of the library that supports the problem
 * at m_probe and 16 * m_probe rows (heuristic list + all algorithms, no name filter; bias in the
 * GEMM's epilogue when has_bias), each timed on both, the `top` fastest by t(16 m) + t(m) checked
 * bit for bit for repeatability (flag 1) and batch invariance (flag 2); flag 4 = the heuristic's
 * first choice (always listed).  Rows fastest first; names packed at name_len bytes each. */
int ecoflap_linear_tune(int64_t m_probe, int64_t N, int64_t K, int dtype, int has_bias, int bias_dtype,
                        int top, int* index_out, float* us_big_out, float* us_small_out, int* flags_out,
                        char* names_out, int name_len, int* n_out, int* n_candidates);
/* "<hipblasLtGetVersion>-<git revision>" of the hipBLASLt serving this process: a solution index
 * means something only together with it (recorded by the run summaries). */
int ecoflap_linear_library_version(char* out, int len);

#ifdef __cplusplus
}
#endif
#endif
