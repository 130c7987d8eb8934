/*
 * tgis_hip.h — C ABI of libtgis_hip.so, the MI355X (gfx950) native-kernel library that sits
 * where the reference's CUDA extension modules sit on the batched-decode hot path.
 *
 * Boundary: SURVEY.md §8(b) row #5.  The reference calls pybind/torch-extension functions with
 * at::Tensor arguments (flash_attn_2_cuda, dropout_layer_norm, rotary_emb, exllamav2_kernels);
 * this library exposes the same operations behind a plain C ABI: raw device pointers, int64
 * sizes/strides, float scalars and a hipStream_t passed as void*.  No torch types, no allocation
 * inside any call (callers pass workspaces; *_workspace_bytes queries say how large), no implicit
 * synchronisation.  Every function returns 0 on success or a negative TGIS_E* code;
 * tgis_last_error() returns a thread-local message for the last failure.
 *
 * dtype codes: TGIS_F16 (IEEE half) and TGIS_BF16.  All "T*" pointers below are 2-byte elements
 * of that dtype.  All pointers are device pointers unless the comment says host.
 *
 * Reference citations are relative to /root/reference/server/text_generation_server/.
 */
#ifndef TGIS_HIP_H
#define TGIS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TGIS_OK 0
#define TGIS_EINVAL (-1)   /* bad argument (shape, alignment, dtype) */
#define TGIS_EHIP (-2)     /* a HIP runtime call failed */
#define TGIS_EUNSUPPORTED (-3)
#define TGIS_ENOMEM (-4)

#define TGIS_F16 0
#define TGIS_BF16 1

/* KV page geometry: 32 tokens per page; per (page, k|v, kv_head) one
 * 32*head_dim element block in an MFMA-fragment-ready order. */
#define TGIS_KV_PAGE_TOKENS 32

/* KV cache element codes of the *_kv8 entry points (csrc/kv_layout.h).  TGIS_KV_MODEL: the pools hold the
 * model dtype (the entry point then behaves exactly like the one it extends; the scales are ignored).  TGIS_KV_FP8_E4M3:
 * the pools hold one byte per element, OCP float8_e4m3fn, in the same page layout: stored = e4m3(sat(x / s)) with sat the
 * clamp to +-448 and round-to-nearest-even, s = k_scale for k and v_scale for v (one positive float each per layer).  The
 * NaN codes 0x7F / 0xFF are never written. */
#define TGIS_KV_MODEL 0
#define TGIS_KV_FP8_E4M3 1

/* ---- library info ------------------------------------------------------------------------- */
const char* tgis_version(void);          /* "tgis_hip x.y (gfx950)" */
const char* tgis_arch(void);             /* offload arch the kernels were compiled for */
const char* tgis_last_error(void);       /* thread-local, never NULL */
/* Forget the last failure, including the HIP runtime's sticky per-thread error: every launch in this library ends with
 * hipGetLastError(), so an error left behind by someone else's aborted stream capture would otherwise be reported by
 * the next, unrelated call. */
void tgis_clear_error(void);
int tgis_device_info(int device, int* num_cus, int64_t* hbm_bytes, char* name, int name_len);

/* Optional per-op device timing with HIP events recorded on the op's own stream.
 * tgis_timing_enable(1) makes every timed op (see TGIS_OP_*) bracket its kernel launch(es) with an
 * event pair; tgis_timing_read() synchronises those events and returns count and total
 * milliseconds since the last tgis_timing_reset().  Disabled by default (no events, no cost). */
#define TGIS_OP_GPTQ_GEMM 0
#define TGIS_OP_ATTN 1
#define TGIS_OP_DENSE_GEMM 2
#define TGIS_OP_NORM 3
#define TGIS_OP_ROPE_KV 4
#define TGIS_OP_ACT 5
#define TGIS_OP_SAMPLE 6
#define TGIS_OP_DECODE_TAIL 7
#define TGIS_OP_COUNT 8
int tgis_timing_enable(int on);
int tgis_timing_reset(void);
int tgis_timing_read(int op, int64_t* count, double* total_ms);

/* ---- GPTQ int4 linear (replaces exllamav2_kernels.make_q_matrix / gemm_half_q_half,
 *      utils/gptq/exllamav2.py:14-62,100-144; normative arithmetic utils/gptq/quant_linear.py:130-192) */

/* Bytes of the prepared (repacked) weight image for a [K,N] 4-bit matrix with `groups` groups. */
int64_t tgis_gptq_prepared_bytes(int64_t K, int64_t N, int64_t groups);

/* Repack GPTQ tensors into the kernel layout.  One-time, at load
 * (the reference does this in Ex4bitLinearV2.post_init, exllamav2.py:124-137).
 *   qweight [K/8, N] int32, qzeros [groups, N/8] int32, scales [groups, N] f16,
 *   g_idx [K] int32 or NULL (NULL = trivial k / groupsize), perm_out [K] int32 or NULL:
 *   when g_idx is not the trivial map (act-order) perm_out receives the row permutation that the
 *   activation must be gathered with (x'[:,k'] = x[:,perm[k']]); groupsize = K / groups.
 *   prepared: caller-owned buffer of tgis_gptq_prepared_bytes().  Requires K%32==0, N%32==0
 *   (same asserts as exllamav2.py:118-119) and (K/groups)%8==0.
 *   flags bit 0 (TGIS_GPTQ_GATE_UP): the matrix is a fused [gate | up] projection (N = 2 I); columns are
 *   interleaved in the image so that tgis_gptq_gemm_f16(act=2) can apply SiLU(gate)*up in its epilogue. */
#define TGIS_GPTQ_GATE_UP 1
int tgis_gptq_prepare(const int32_t* qweight, const int32_t* qzeros, const void* scales,
                      const int32_t* g_idx_host, int32_t* perm_out, int64_t K, int64_t N,
                      int64_t groups, int flags, void* prepared, void* stream);

/* Workspace for split-K partial sums + arrival counters of one gemm call. The counter region
 * (first 4096 bytes) must be zero before the first call; the kernel leaves it zero. */
/* Largest M for which tgis_gptq_gemm_f16 is a fused dequantise + MFMA kernel worth calling (above it the caller
 * dequantises once with tgis_gptq_dequant_f16 and uses a library GEMM, exllamav2.py:87 "M > 50"): M <= 64 streams the
 * weights once per pass, 64 < M <= 256 in 64-row passes, and — for K % 64 == 0, group size 64 * 2^n, no act-order, act != 1 —
 * a tall kernel (one dequantisation per 128 rows, 700-900 TFLOP/s, no scratch copy of W) takes over up to a few thousand
 * rows. */
int64_t tgis_gptq_gemm_fused_rows(int64_t K, int64_t groups, int act_order, int act);
int64_t tgis_gptq_gemm_workspace_bytes(int64_t M, int64_t K, int64_t N);

/* Activation layout between the decode step's own kernels (round 4).  A leading dimension of TGIS_LD_FRAGMENTS says that a
 * [M <= 64, K] f16 activation (K % 64 == 0; the buffer holds ceil(M / 32) * 32 * K elements) is stored in the order the MFMA
 * reads it — [row block m/32][k64-step][i = k/8 % 4][lane = 32 (k/32 % 2) + m % 32][k % 8], i.e. element (m, k) at
 * (m/32) * 32 K + ((k/64 * 4 + k/8 % 4) * 64 + 32 (k/32 % 2) + m % 32) * 8 + k % 8 — instead of row-major.  Producers that can write it:
 * tgis_rmsnorm_residual[_partial] (ldy), tgis_attn_paged (ld_out), tgis_gptq_gemm_f16 with act = 2 (ldo).  Consumers:
 * tgis_gptq_gemm_f16, tgis_gptq_gemm_f16_partial, tgis_gptq_gemm_rope_f16 (ldx), which then run the kernel of
 * csrc/gptq_wide_body.h: each k64-step of the activation is four contiguous KiB straight into the A operand, no LDS staging
 * (7B shapes, 32 rows: qkv + rope 16.9 -> 12 us, o 6.0 -> 5.3, gate_up 16.8 -> 14.4, down 10.5 -> 9.2).  Same arithmetic as
 * the row-major path ((q - z) * s rounded to f16 once, fp32 accumulation); only the summation order over k differs.
 * tgis_gptq_fragments_ok: 1 if the GEMM (act 0, 2, or 3 = the rope epilogue) takes such an activation and is expected to be
 * faster with it (1 <= M <= 64, no act-order, groups of 64 * 2^n rows; act 2 / 3 additionally >= 128 workgroups). */
#define TGIS_LD_FRAGMENTS ((int64_t)-32)
int tgis_gptq_fragments_ok(int64_t M, int64_t K, int64_t N, int64_t groups, int act_order, int act);

/* out[M,N] f16 = x[M,K] f16 @ dequant(W)[K,N] (+ bias[N] f16 if non-NULL); fp32 accumulate.
 * Fused int4-dequant MFMA kernel for any M (rows are processed in slabs of 32).
 * x row stride ldx, out row stride ldo (elements).  perm (int32 [K] or NULL) gathers x columns
 * for act-order matrices.  act: 0 = none; 1 = x is [M,2K] and the kernel consumes silu(x[:, :K]) * x[:, K:]
 * while staging it; 2 = the image was prepared with TGIS_GPTQ_GATE_UP and out is [M, N/2] =
 * silu(gate) * up applied in the epilogue (both fuse LlamaMLP's activation, flash_llama_modeling.py:332-335).
 * act 4 / 5 (M <= 256, row-major x and out, not a TGIS_GPTQ_GATE_UP image): out = f16(gelu(f16(x @ W + bias))), exact erf
 * form / tanh approximation — the `self.act(...)` behind an int4 `c_fc` (flash_santacoder_modeling.py:284-306).  The plan is
 * the one of act 0 and the activation is applied where that plan finishes the sum (the epilogue of an unsplit plan, the
 * split-K reduce otherwise): bit-identical to tgis_gptq_gemm_f16(act 0) followed by tgis_gelu.
 * tgis_gptq_gemm_fused_rows(act 4 | 5) is 256: above, the caller runs act 0 (or its library path) and tgis_gelu. */
int tgis_gptq_gemm_f16(const void* x, int64_t ldx, const void* prepared, const void* bias,
                       const int32_t* perm, void* out, int64_t ldo, int64_t M, int64_t K, int64_t N,
                       int64_t groups, int act, void* workspace, int64_t workspace_bytes, void* stream);

/* Deferred-reduce variant: instead of the f16 result, the S split-K partial sums are left in
 * `slabs` as fp32 [ceil(M/32)][S][32][ld] (ld = N rounded up to 32, returned in *slab_ld; S in *num_slabs, >= 1) for a
 * consumer that sums them in its prologue (tgis_rmsnorm_residual_partial / tgis_rope_kv_write_partial), which
 * removes the reduce launch.  The consumer rounds the sum (+bias) to f16 first, so results are bit-identical to
 * tgis_gptq_gemm_f16 followed by the plain consumer.  slabs must hold tgis_gptq_gemm_partial_bytes(M,K,N) bytes. */
int64_t tgis_gptq_gemm_partial_bytes(int64_t M, int64_t K, int64_t N);
int tgis_gptq_gemm_f16_partial(const void* x, int64_t ldx, const void* prepared, const int32_t* perm, int64_t M,
                               int64_t K, int64_t N, int64_t groups, int act, float* slabs, int64_t slabs_bytes,
                               int* num_slabs, int64_t* slab_ld, void* stream);

/* ---- fused qkv projection + rotary embedding + cache write (decode, round 3) ------------------------------------------
 * One launch for `qkv = query_key_value(x)`, `rotary_emb(q, k, cos, sin)` and `layer_past[slot] = (k, v)`
 * (flash_llama_modeling.py:251-268,282) at decode sizes: the GEMM keeps the whole k range in a block (no split-K slabs)
 * and its epilogue rounds the sum (+ bias) to f16, rotates q / k heads in fp32 (the arithmetic of tgis_rope_kv_write) and
 * stores q to q_out[M, ldq] and k / v into the cache pages of slots[m] (page layouts of tgis_rope_kv_write).
 * `prepared` is a SECOND image of the qkv weight made with flags = TGIS_GPTQ_ROPE_IMAGE(D, H + Hkv): inside each rotated
 * head a 32-column tile holds 16 dims and their 16 rotation partners, so every wave owns complete rotation pairs.
 * Full rotary span only (rot_dim == D).  tgis_gptq_rope_ok: whether the launch exists for the shape (1 <= M <= 64, groups
 * of 64 * 2^n rows, no act-order, D % 32 == 0) AND is expected to beat the two launches it replaces (its unsplit plan
 * still covers the chip: >= 128 workgroups); the entry point itself only checks the former. */
#define TGIS_GPTQ_ROPE_IMAGE(D, rotated_heads) (2 | ((int)(D) << 8) | ((int)(rotated_heads) << 20))
int tgis_gptq_rope_ok(int64_t M, int64_t K, int64_t N, int64_t groups, int act_order, int64_t D);
int tgis_gptq_gemm_rope_f16(const void* x, int64_t ldx, const void* prepared, const void* bias, const int32_t* positions,
                            const int32_t* slots, const void* cos, const void* sin, void* q_out, int64_t ldq,
                            void* k_pool, void* v_pool, int64_t M, int64_t K, int64_t N, int64_t groups, int64_t H,
                            int64_t Hkv, int64_t D, void* stream);
/* tgis_gptq_gemm_rope_f16 with a KV cache of element kv_dtype (TGIS_KV_*): k / v go into their pages quantised with
 * k_scale / v_scale; q_out is as above.  Same call site (flash_llama_modeling.py:251-268,282). */
int tgis_gptq_gemm_rope_f16_kv8(const void* x, int64_t ldx, const void* prepared, const void* bias,
                                const int32_t* positions, const int32_t* slots, const void* cos, const void* sin, void* q_out,
                                int64_t ldq, void* k_pool, void* v_pool, int64_t M, int64_t K, int64_t N, int64_t groups,
                                int64_t H, int64_t Hkv, int64_t D, void* stream, int kv_dtype, float k_scale, float v_scale);

/* The same launch for dense (f16 / bf16) qkv weights: `prepared` from tgis_dense_prepare with
 * flags = TGIS_GPTQ_ROPE_IMAGE(D, H + Hkv); cos / sin in the model dtype; 1 <= M <= 64. */
int tgis_dense_rope_ok(int64_t M, int64_t K, int64_t N, int64_t D);
int tgis_dense_gemm_rope(const void* x, int64_t ldx, const void* prepared, const void* bias, const int32_t* positions,
                         const int32_t* slots, const void* cos, const void* sin, void* q_out, int64_t ldq, void* k_pool,
                         void* v_pool, int64_t M, int64_t K, int64_t N, int64_t H, int64_t Hkv, int64_t D, int dtype,
                         void* stream);
/* tgis_dense_gemm_rope with a KV cache of element kv_dtype (TGIS_KV_*) and its per-layer scales (as
 * tgis_gptq_gemm_rope_f16_kv8; flash_llama_modeling.py:251-268,282). */
int tgis_dense_gemm_rope_kv8(const void* x, int64_t ldx, const void* prepared, const void* bias, const int32_t* positions,
                             const int32_t* slots, const void* cos, const void* sin, void* q_out, int64_t ldq, void* k_pool,
                             void* v_pool, int64_t M, int64_t K, int64_t N, int64_t H, int64_t Hkv, int64_t D, int dtype,
                             void* stream, int kv_dtype, float k_scale, float v_scale);

/* Full dequantisation to a dense f16 [K,N] matrix (row-major), the "temp_dq" path the reference
 * uses for M > 50 before a library GEMM (exllamav2.py:65-66,87). */
int tgis_gptq_dequant_f16(const void* prepared, void* w_out, int64_t K, int64_t N, int64_t groups,
                          int flags, void* stream);

/* ---- GPTQ 8-bit linear (replaces the Triton QuantLinear that get_linear gives every GPTQ width but 4,
 *      utils/layers.py:184-199; normative arithmetic utils/gptq/quant_linear.py:130-192,259) -------------------------------
 * W[k,n] = f16((q[k,n] - (z[g(k),n] + 1)) * s[g(k),n]), q and z unsigned bytes, z + 1 not masked back to a byte (a stored
 * 255 is a zero point of 256); the weight is rounded to f16 once, accumulation is fp32, the output f16 (+ bias).
 * Every entry point requires K % 32 == 0, N % 32 == 0 and (K / groups) % 16 == 0 and refuses anything else. */

/* Bytes of the prepared image of a [K,N] 8-bit matrix with `groups` groups (w8 [N/32][K/64 + 1][2][64][16 B]
 * + sz [N/32][groups][32]).  Call site: QuantLinear.__init__ / pack, utils/gptq/quant_linear.py:130-192,259. */
int64_t tgis_gptq8_prepared_bytes(int64_t K, int64_t N, int64_t groups);

/* Repack qweight [K/4, N] int32, qzeros [groups, N/4] int32, scales [groups, N] f16 into the image; g_idx_host / perm_out as
 * tgis_gptq_prepare (act-order rows are sorted by group, perm_out receives the gather the activation needs).  flags must
 * be 0.  One-time, at load: replaces the buffers QuantLinear keeps (utils/gptq/quant_linear.py:130-192,259). */
int tgis_gptq8_prepare(const int32_t* qweight, const int32_t* qzeros, const void* scales, const int32_t* g_idx_host,
                       int32_t* perm_out, int64_t K, int64_t N, int64_t groups, int flags, void* prepared, void* stream);

/* Workspace of one tgis_gptq8_gemm_f16 call: the 4096-byte counter region of the int4 convention (zero before and after
 * the call; this launch does not touch it) followed by the fp32 split-K slabs (utils/gptq/quant_linear.py:130-192,259). */
int64_t tgis_gptq8_gemm_workspace_bytes(int64_t M, int64_t K, int64_t N);

/* out[M,N] f16 = x[M,K] f16 @ dequant(W) (+ bias), 1 <= M <= 64 (a larger M is an argument error: the caller dequantises
 * with tgis_gptq8_dequant_f16 and uses a library GEMM).  ldx / ldo: row strides in elements (ldx % 8 == 0, x 16-byte
 * aligned).  perm (int32 [K] or NULL) gathers x columns, -1 reads a zero.  act 0, or 1: x is [M, 2K] and the operand is
 * silu(x[:, :K]) * x[:, K:].  Deterministic: k-parts and split-K slabs are summed in fixed order.  No allocation, no
 * synchronisation.  Replaces QuantLinear.forward, utils/gptq/quant_linear.py:130-192,259. */
int tgis_gptq8_gemm_f16(const void* x, int64_t ldx, const void* prepared, const void* bias, const int32_t* perm, void* out,
                        int64_t ldo, int64_t M, int64_t K, int64_t N, int64_t groups, int act, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* Dense f16 [K,N] (row-major, rows in image order) of a prepared 8-bit matrix, for the large-M library GEMM; bit-equal to
 * ((q - z - 1).float() * s.float()).half().  Replaces the dequantisation inside QuantLinear.forward,
 * utils/gptq/quant_linear.py:130-192,259. */
int tgis_gptq8_dequant_f16(const void* prepared, void* w_out, int64_t K, int64_t N, int64_t groups, void* stream);

/* ---- dense skinny GEMM (replaces F.linear / torch.mm at decode sizes, utils/layers.py:110-111,
 *      lm_head utils/layers.py:261) -------------------------------------------------------------- */
int64_t tgis_dense_prepared_bytes(int64_t N, int64_t K);
/* Repack a torch-Linear weight W[N,K] (row-major, dtype) into 32-column MFMA tiles.
 * flags bit 0: W is the Llama MLP's [gate rows | up rows] (N = 2 I, I a multiple of 16): tile t then holds gate rows
 * 16 t .. 16 t + 15 and the matching up rows, for the act = 2 epilogue of tgis_dense_gemm. */
int tgis_dense_prepare(const void* w, int64_t N, int64_t K, int dtype, int flags, void* prepared, void* stream);
int64_t tgis_dense_gemm_workspace_bytes(int64_t M, int64_t K, int64_t N);
/* out[M,N] = x[M,K] @ W^T (+bias).  out_f32 != 0 writes float32 output (logits).
 * act 0: plain.  act 1: x is [M, 2K] (gate | up) and the operand is silu(gate) * up, formed while it is staged
 * (down_proj after an un-fused gate_up).  act 2: the image has flags bit 0 and out is [M, N/2] =
 * silu(x @ Wgate^T) * (x @ Wup^T), each factor rounded to the model dtype as the reference's eager ops do
 * (flash_llama_modeling.py:332-335); the down projection then runs with act 0.
 * act 4 / 5: out = gelu(T(x @ W^T + bias)) in the model dtype, exact erf form / tanh approximation — the `self.act(...)`
 * behind `c_fc` (flash_santacoder_modeling.py:284-306) applied to the rounded output where it is finished (the epilogue of an
 * unsplit plan, the split-K reduce otherwise): bit-identical to tgis_dense_gemm(act 0) followed by tgis_gelu. */
int tgis_dense_gemm(const void* x, int64_t ldx, const void* prepared, const void* bias, void* out,
                    int64_t ldo, int64_t M, int64_t K, int64_t N, int dtype, int out_f32, int act,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* Deferred split-K, as tgis_gptq_gemm_f16_partial: the fp32 partial sums [ceil(M/32)][num_slabs][32][slab_ld] are
 * left for the consumer kernel (tgis_rmsnorm_residual_partial / tgis_rope_kv_write_partial), which adds the bias. */
int64_t tgis_dense_gemm_partial_bytes(int64_t M, int64_t K, int64_t N);
int tgis_dense_gemm_partial(const void* x, int64_t ldx, const void* prepared, int64_t M, int64_t K, int64_t N,
                            int dtype, int act, float* slabs, int64_t slabs_bytes, int* num_slabs,
                            int64_t* slab_ld, void* stream);

/* ---- routed expert MLP (Mixtral: transformers' MixtralTopKRouter + MixtralExperts; the reference has no such model) ----
 * A slot is (token t, choice k) = t * top_k + k.  Nothing below reads the routing on the host, so the four launches of a
 * block (router GEMM by tgis_dense_gemm with out_f32, route, up, down) can be captured.  Deterministic: integer work for
 * the lists, k-parts and the top_k addends summed in fixed order, no float atomics. */
/* logits: fp32 [T, E] (row stride ld), the router GEMM's output.  Per token: softmax over all E, the top_k largest (ties
 * to the lower expert index), those renormalised to sum 1.  Writes expert_ids int32 [T, top_k], expert_w f32 [T, top_k],
 * counts int32 [E], offsets int32 [E + 1] (exclusive prefix sum of counts) and slot_rows int32 [T * top_k]: the slots
 * grouped by expert, ascending inside each expert.  2 <= E <= 64, 1 <= top_k <= min(E, 8), T >= 0 (T * top_k < 2^31);
 * anything else is TGIS_EINVAL before the device is touched. */
int tgis_moe_route(const float* logits, int64_t ld, int64_t T, int E, int top_k, int32_t* expert_ids, float* expert_w,
                   int32_t* counts, int32_t* offsets, int32_t* slot_rows, void* stream);
/* h[slot, :] = silu(x[t] @ Wgate[e]^T) * (x[t] @ Wup[e]^T) for every slot, e = the slot's expert, each factor rounded to
 * the model dtype as act 2 of tgis_dense_gemm does.  images: E gate|up images (tgis_dense_prepare with flags bit 0, N =
 * 2 I rows, I a multiple of 16) expert_stride bytes apart; x [T, K] (row stride ldx, K % 8 == 0); h [T * top_k, N / 2]
 * (row stride ldh).  The grid is (N / 32, E) whatever the routing; a block whose expert nobody chose reads no weights. */
int tgis_moe_gemm_up(const void* x, int64_t ldx, const void* images, int64_t expert_stride, const int32_t* offsets,
                     const int32_t* slot_rows, void* h, int64_t ldh, int64_t T, int64_t K, int64_t N, int E, int top_k,
                     int dtype, void* stream);
/* y[slot, :] = (h[slot] @ Wdown[e]^T) * expert_w[slot], the product in fp32.  images: E plain images of W2 [N, K].
 * form 0 (decode): scratch receives the slabs [ceil(T/32)][top_k][32][ceil(N/32)*32] of a deferred sum — slab k, row t holds
 * token t's k-th expert, every (t, k) written exactly once — for tgis_rmsnorm_residual_partial with num_slabs = top_k;
 * out is not used.  form 1: scratch holds y as fp32 [T * top_k, N] and a second launch writes
 * out[t] = T(sum_k y[t * top_k + k]) in the order k = 0 .. top_k - 1 (N % 4 == 0; row stride ldo).
 * tgis_moe_gemm_down_bytes: the size of scratch. */
int64_t tgis_moe_gemm_down_bytes(int64_t T, int64_t N, int top_k, int form);
int tgis_moe_gemm_down(const void* h, int64_t ldh, const void* images, int64_t expert_stride, const int32_t* offsets,
                       const int32_t* slot_rows, const float* expert_w, int64_t T, int64_t K, int64_t N, int E, int top_k,
                       int dtype, int form, float* scratch, int64_t scratch_bytes, void* out, int64_t ldo, void* stream);
/* The two expert GEMMs over int4 GPTQ weights: the contracts of tgis_moe_gemm_up / tgis_moe_gemm_down (same grid, same
 * early return for an unchosen expert — neither its nibbles nor its scale table are read — same epilogues, same slabs and
 * tgis_moe_gemm_down_bytes, same run-to-run bytes) with images = E images of tgis_gptq_prepare for (K, N, groups),
 * expert_stride >= tgis_gptq_prepared_bytes(K, N, groups) bytes apart (a multiple of 16); gate|up images are prepared with
 * flags bit 0.  The weight a product sees is f16((q - z - 1) * scale), one rounding, as tgis_gptq_gemm_f16's.
 * Served: dtype TGIS_F16, K % 64 == 0, N % 32 == 0, one group or groups of 64 * 2^n rows that divide K, no act-order
 * permutation; anything else (groups of 32 rows, bf16, a stride below one image) is TGIS_EINVAL before any launch. */
int tgis_moe_gptq_gemm_up(const void* x, int64_t ldx, const void* images, int64_t expert_stride, const int32_t* offsets,
                          const int32_t* slot_rows, void* h, int64_t ldh, int64_t T, int64_t K, int64_t N, int64_t groups,
                          int E, int top_k, int dtype, void* stream);
int tgis_moe_gptq_gemm_down(const void* h, int64_t ldh, const void* images, int64_t expert_stride, const int32_t* offsets,
                            const int32_t* slot_rows, const float* expert_w, int64_t T, int64_t K, int64_t N, int64_t groups,
                            int E, int top_k, int dtype, int form, float* scratch, int64_t scratch_bytes, void* out,
                            int64_t ldo, void* stream);

/* ---- per-request LoRA adapters (csrc/lora.hip) ----
 * A wrapped linear computes y[t] = W x[t] + scale_s B_s (A_s x[t]) with s = slot[t]; a row with slot[t] = -1 keeps W x[t].
 * Shared limits: 0 <= T <= 64 rows, 1 <= S <= 32 slots, 1 <= P <= 3 projections fused into the base linear, max_rank a
 * multiple of 16 up to 64, dtype TGIS_F16 / TGIS_BF16, K % 8 == 0, N % 8 == 0; anything else is TGIS_EINVAL with a message,
 * before the device is touched.  Nothing is read on the host, no float atomics: the same input gives the same bytes.
 *
 * Slot images of one linear (S of each, a fixed byte stride apart, at fixed addresses; an adapter is loaded by a
 * stream-ordered copy), with ranks int32 [S] (0: the slot holds nothing for this linear) and scales f32 [S] (alpha / r):
 *   A  [P][max_rank][K] row-major in the model dtype (tgis_lora_a_bytes), rows rank .. round_up(rank, 16) - 1 zero;
 *   B  [max_rank / 16][N][16] in the model dtype (tgis_lora_b_bytes): granule g holds columns 16 g .. 16 g + 15 of
 *      B [N, r], zero from column rank on.
 * A step reads round_up(rank, 16) rows of A and as many columns of B of a slot that some row names, and nothing else. */
int64_t tgis_lora_a_bytes(int64_t K, int P, int max_rank);
int64_t tgis_lora_b_bytes(int64_t N, int max_rank);
/* slot int32 [T] with values -1 .. S-1 -> counts int32 [S], offsets int32 [S + 1] (exclusive prefix sum) and rows int32 [T]:
 * the rows that name a slot, grouped by slot and ascending inside each (offsets[S] of them).  Once per forward. */
int tgis_lora_group(const int32_t* slot, int64_t T, int S, int32_t* counts, int32_t* offsets, int32_t* rows, void* stream);
/* v[t, p, 0 .. round_up(rank_s, 16)) = A_s[p] x[t] in fp32 for every row t of the lists; v is fp32 [T, P, max_rank] and the
 * rest of it is left alone.  x [T, K] in the model dtype, row stride ldx (a multiple of 8), 16-byte aligned. */
int tgis_lora_shrink(const void* x, int64_t ldx, const void* a_images, int64_t a_stride, const int32_t* ranks,
                     const int32_t* offsets, const int32_t* rows, float* v, int64_t T, int64_t K, int P, int S, int max_rank,
                     int dtype, void* stream);
/* y[t, n] = T(float(y[t, n]) + scale_s * sum_r v[t, p(n), r] B_s[n, r]) in place for every row t of the lists, r ascending
 * in fp32; p(n) is the segment of n under the P + 1 column bounds (a host array: bounds[0] = 0 < ... < bounds[P] = N, all
 * multiples of 8).  y [T, N] in the model dtype, row stride ldy.  Rows outside the lists are not touched. */
int tgis_lora_expand(const float* v, const void* b_images, int64_t b_stride, const int32_t* ranks, const float* scales,
                     const int32_t* offsets, const int32_t* rows, const int64_t* bounds, void* y, int64_t ldy, int64_t T,
                     int64_t N, int P, int S, int max_rank, int dtype, void* stream);

/* ---- fused residual-add + RMSNorm / LayerNorm (replaces dropout_layer_norm.dropout_add_ln_fwd,
 *      custom_modeling/flash_llama_modeling.py:132-152, utils/layers.py:376-396) ---------------- */
/* res_out = x (+ residual); y = res_out * rsqrt(mean(res_out^2) + eps) * weight.
 * residual may be NULL (first layer).  res_out may alias residual or x.  fp32 statistics.
 * ldy: 0 or hidden (y row-major), or TGIS_LD_FRAGMENTS (rows <= 64, hidden % 64 == 0: y feeds an int4 GEMM of the decode
 * step, see TGIS_LD_FRAGMENTS above). */
int tgis_rmsnorm_residual(const void* x, const void* residual, const void* weight, void* y, int64_t ldy,
                          void* res_out, int64_t rows, int64_t hidden, float eps, int dtype,
                          void* stream);
/* Same as tgis_rmsnorm_residual with x given as split-K partial sums: x = f16(sum_s slabs[s][row][:] (+ bias)).
 * rows <= 32. */
int tgis_rmsnorm_residual_partial(const float* slabs, int num_slabs, int64_t slab_ld, const void* bias,
                                  const void* residual, const void* weight, void* y, int64_t ldy, void* res_out,
                                  int64_t rows, int64_t hidden, float eps, int dtype, void* stream);
int tgis_layernorm_residual(const void* x, const void* residual, const void* weight, const void* bias,
                            void* y, void* res_out, int64_t rows, int64_t hidden, float eps,
                            int dtype, void* stream);
/* tgis_layernorm_residual with x given as split-K partial sums (see tgis_rmsnorm_residual_partial): x = model-dtype
 * rounding of sum_s slabs[s][row][:] (+ xbias, the producing linear's bias).  Removes the reduce launch after the
 * c_proj linears of flash_santacoder_modeling.py:255-307. */
int tgis_layernorm_residual_partial(const float* slabs, int num_slabs, int64_t slab_ld, const void* xbias,
                                    const void* residual, const void* weight, const void* bias, void* y,
                                    void* res_out, int64_t rows, int64_t hidden, float eps, int dtype,
                                    void* stream);

/* Parallel-residual boundary of a GPT-NeoX layer (flash_neox_modeling.py:238-259): res_out = h' = residual + A + B, with
 * A = a (+ a_bias) and B = b (+ b_bias) summed in fp32 in that order and rounded to the model dtype once;
 * y1 = LayerNorm(h'; w1, b1) and y2 = LayerNorm(h'; w2, b2) from ONE set of fp32 statistics of the unrounded h'.
 * a / b / biases may be NULL (absent); y2 == NULL (w2, b2 ignored) is a single LayerNorm (final_layer_norm).
 * res_out may alias residual; NULL skips the store. */
int tgis_layernorm2_residual(const void* residual, const void* a, const void* a_bias, const void* b, const void* b_bias,
                             const void* w1, const void* b1, const void* w2, const void* b2, void* y1, void* y2,
                             void* res_out, int64_t rows, int64_t hidden, float eps, int dtype, void* stream);
/* The same with either addend given as split-K partial sums (a_slabs [ceil(rows/32)][a_num_slabs][32][a_slab_ld] fp32 of
 * tgis_dense_gemm_partial / tgis_gptq_gemm_f16_partial; the two may have different numbers of slabs) or as a tensor: per
 * addend at most one of (tensor, slabs) is non-NULL.  A slab sum is NOT rounded before it joins h' (h' is rounded once). */
int tgis_layernorm2_residual_partial(const void* residual, const void* a, const float* a_slabs, int a_num_slabs,
                                     int64_t a_slab_ld, const void* a_bias, const void* b, const float* b_slabs,
                                     int b_num_slabs, int64_t b_slab_ld, const void* b_bias, const void* w1, const void* b1,
                                     const void* w2, const void* b2, void* y1, void* y2, void* res_out, int64_t rows,
                                     int64_t hidden, float eps, int dtype, void* stream);

/* ---- RoPE + KV-cache write (replaces rotary_emb.apply_rotary + the index_put at
 *      flash_llama_modeling.py:262-268,282; utils/layers.py:466-472) ---------------------------- */
/* qkv [T, (H + 2*Hkv)*D] (row stride ld_qkv): rotates q heads and k heads in place with the
 * half-split (NeoX) rotation using cos/sin tables [max_pos, rot_dim/2] of the model dtype gathered by
 * positions[T] (int32) — dims [0, rot_dim) of each head, rot_dim even and <= D (partial rotary: gpt-neox-20b 24 of 96), then writes k and v of token t into KV page slot slots[t]
 * (= page_id*32 + offset).  cos == NULL skips the rotation (learned-position models).
 * k_pool / v_pool: this layer's K and V page pools, [num_pages][Hkv][32*D] each.  Inside a (page, kv head) block of
 * 32 tokens x D: K as [token >> 4][D / 8][16 tokens][8], V as [4 column groups][D][8] with token t in column
 * (i >> 2) * 8 + (t >> 4) * 4 + (i & 3), i = t & 15 (csrc/kv_layout.h, DESIGN.md section 3: the orders in which the
 * attention kernels' MFMA fragments are whole cache lines).  The pools are opaque to callers; oracle/ops_ref.py's
 * kv_page_unpack reads them back for tests. */
int tgis_rope_kv_write(void* qkv, int64_t ld_qkv, const void* cos, const void* sin,
                       const int32_t* positions, const int32_t* slots, void* k_pool, void* v_pool,
                       int64_t T, int H, int Hkv, int D, int rot_dim, int dtype, void* stream);

/* Same with the qkv activation given as split-K partial sums: qkv_out[T, ld_qkv] receives
 * f16(sum_s slabs[s] (+ bias)) with q,k rotated; k,v go to the cache. */
int tgis_rope_kv_write_partial(const float* slabs, int num_slabs, int64_t slab_ld, const void* bias, void* qkv_out,
                               int64_t ld_qkv, const void* cos, const void* sin, const int32_t* positions,
                               const int32_t* slots, void* k_pool, void* v_pool, int64_t T, int H, int Hkv, int D,
                               int rot_dim, int dtype, void* stream);

/* Prefill form of tgis_rope_kv_write for fresh sequences (token i of sequence b is cache position i): q is rotated in
 * place; k (rotated) and v go to the cache page by page — full 16-byte runs of the page layouts instead of the
 * per-token scatter — with the slots of a last partial page zeroed.  k/v inside `qkv` are left as they came.
 *   cu_seqlens [B+1]: token offsets; block_tables [B, max_pages]; T = total tokens; max_len = longest sequence. */
int tgis_rope_kv_write_prefill(void* qkv, int64_t ld_qkv, const void* cos, const void* sin, const int32_t* positions,
                               const int32_t* cu_seqlens, const int32_t* block_tables, int64_t max_pages, void* k_pool,
                               void* v_pool, int64_t B, int64_t T, int64_t max_len, int H, int Hkv, int D, int rot_dim,
                               int dtype, void* stream);

/* The three cache writers above for a KV cache of element kv_dtype (TGIS_KV_*): k and v are stored as
 * e4m3(sat(x / k_scale)) / e4m3(sat(x / v_scale)) of the value the 16-bit pool would receive (k after rotary, rounded to
 * the model dtype); q, qkv_out and the unrotated dims are exactly those of the 16-bit call; the prefill form zeroes the
 * slots of a last partial page as well.  Same call sites (flash_llama_modeling.py:262-268,282). */
int tgis_rope_kv_write_kv8(void* qkv, int64_t ld_qkv, const void* cos, const void* sin, const int32_t* positions,
                           const int32_t* slots, void* k_pool, void* v_pool, int64_t T, int H, int Hkv, int D, int rot_dim,
                           int dtype, void* stream, int kv_dtype, float k_scale, float v_scale);
int tgis_rope_kv_write_partial_kv8(const float* slabs, int num_slabs, int64_t slab_ld, const void* bias, void* qkv_out,
                                   int64_t ld_qkv, const void* cos, const void* sin, const int32_t* positions,
                                   const int32_t* slots, void* k_pool, void* v_pool, int64_t T, int H, int Hkv, int D,
                                   int rot_dim, int dtype, void* stream, int kv_dtype, float k_scale, float v_scale);
int tgis_rope_kv_write_prefill_kv8(void* qkv, int64_t ld_qkv, const void* cos, const void* sin, const int32_t* positions,
                                   const int32_t* cu_seqlens, const int32_t* block_tables, int64_t max_pages, void* k_pool,
                                   void* v_pool, int64_t B, int64_t T, int64_t max_len, int H, int Hkv, int D, int rot_dim,
                                   int dtype, void* stream, int kv_dtype, float k_scale, float v_scale);

/* tgis_rope_kv_write_prefill / _kv8 behind a reused prefix (KV prefix reuse: the first past_lens[b] tokens of sequence b
 * are already in the cache, on pages it shares with the request that wrote them; the reference recomputes them,
 * flash_llama_modeling.py:262-268,282 over the whole prompt): token i of sequence b in `qkv` is cache position
 * past_lens[b] + i and goes to table entry past_lens[b] / 32 + i / 32.
 *   past_lens [B] int32 (device): every entry a multiple of 32 (precondition; the caller builds it from host ints),
 *   and past_lens[b] / 32 + ceil(len_b / 32) <= max_pages.  cu_seqlens, T and max_len describe the SUFFIX tokens only.
 * Everything else is the fresh form; no page in front of past_lens[b] / 32 is stored to.  All-zero past_lens is
 * tgis_rope_kv_write_prefill bit for bit.  A null past_lens is TGIS_EINVAL. */
int tgis_rope_kv_write_prefill_at(void* qkv, int64_t ld_qkv, const void* cos, const void* sin, const int32_t* positions,
                                  const int32_t* cu_seqlens, const int32_t* block_tables, int64_t max_pages, void* k_pool,
                                  void* v_pool, int64_t B, int64_t T, int64_t max_len, int H, int Hkv, int D, int rot_dim,
                                  int dtype, void* stream, const int32_t* past_lens);
int tgis_rope_kv_write_prefill_at_kv8(void* qkv, int64_t ld_qkv, const void* cos, const void* sin, const int32_t* positions,
                                      const int32_t* cu_seqlens, const int32_t* block_tables, int64_t max_pages,
                                      void* k_pool, void* v_pool, int64_t B, int64_t T, int64_t max_len, int H, int Hkv,
                                      int D, int rot_dim, int dtype, void* stream, int kv_dtype, float k_scale,
                                      float v_scale, const int32_t* past_lens);

/* The cache writers for models with a per-head RMSNorm of q and k between the qkv projection and the rotation (Qwen3's
 * self_attn.q_norm / k_norm; transformers' Qwen3Attention.forward): every q head and every k head is normalised over its D
 * elements in fp32, rstd = rsqrt(mean_d(x^2) + eps), y = x rstd w[d] with w = q_norm_w / k_norm_w [D] of the model dtype,
 * then rotated in fp32 over dims [0, rot_dim) and rounded to the model dtype once, at the store; dims in [rot_dim, D) are
 * normalised and not rotated, v heads are copied.  x is the model-dtype activation (for slabs: the rounded sum + bias of
 * tgis_rope_kv_write_partial).  Each entry point carries every option of the plain writers in one signature:
 *   tgis_rope_kv_write_qknorm: per token (decode and verify steps, any forward that is not page-wise).  slabs == NULL: in
 *     place on qkv; else qkv receives the reduced, normalised, rotated activation (num_slabs, slab_ld, bias as in
 *     tgis_rope_kv_write_partial; a bias needs slabs).  Hkv = 0 with null pools: q heads only.
 *   tgis_rope_kv_write_prefill_qknorm: page-wise (tgis_rope_kv_write_prefill; past_lens non-null:
 *     tgis_rope_kv_write_prefill_at).  k / v inside `qkv` are left as they came.
 *   kv_dtype, k_scale, v_scale: TGIS_KV_MODEL (scales ignored) or TGIS_KV_FP8_E4M3, as in the _kv8 writers.
 * D must be 64, 96 or 128; rot_dim a positive multiple of 16 <= D; both norm weights, cos, sin and positions non-null;
 * eps > 0.  T == 0 (B == 0) is TGIS_OK and touches nothing.  Both forms write the same bits for the same token. */
int tgis_rope_kv_write_qknorm(void* qkv, int64_t ld_qkv, const float* slabs, int num_slabs, int64_t slab_ld,
                              const void* bias, const void* q_norm_w, const void* k_norm_w, float eps, const void* cos,
                              const void* sin, const int32_t* positions, const int32_t* slots, void* k_pool, void* v_pool,
                              int64_t T, int H, int Hkv, int D, int rot_dim, int dtype, int kv_dtype, float k_scale,
                              float v_scale, void* stream);
int tgis_rope_kv_write_prefill_qknorm(void* qkv, int64_t ld_qkv, const void* q_norm_w, const void* k_norm_w, float eps,
                                      const void* cos, const void* sin, const int32_t* positions,
                                      const int32_t* cu_seqlens, const int32_t* past_lens, const int32_t* block_tables,
                                      int64_t max_pages, void* k_pool, void* v_pool, int64_t B, int64_t T, int64_t max_len,
                                      int H, int Hkv, int D, int rot_dim, int dtype, int kv_dtype, float k_scale,
                                      float v_scale, void* stream);

/* ---- paged attention, prefill and decode (replaces flash_attn_2_cuda.varlen_fwd,
 *      utils/flash_attn.py:43-78) ---------------------------------------------------------------- */
/* Number of key-range splits the launcher will use for this shape (so callers can size workspace). */
int tgis_attn_num_splits(int64_t B, int Hkv, int H, int64_t max_q_len, int64_t max_ctx);
/* Key splits for a launch of up to max_q_len q tokens per sequence over a long cached context: the verify step of
 * speculative decoding (K + 1 rows per request, models/decode_graph.py _VerifyGraph) and the suffix prefill behind reused
 * prefix pages (models/flash_causal_lm.py _prefill_suffix_forward), both through the attention() call site of
 * utils/flash_attn.py:43-78.  max_q_len == 1: exactly
 * tgis_attn_num_splits; the prefill form (max_q_len * next_pow2(min(H / Hkv, 16)) > 64): 1; max_ctx < 1024
 * (so anything below 32 pages): 1.  Host only. */
int tgis_attn_num_splits_q(int64_t B, int Hkv, int H, int64_t max_q_len, int64_t max_ctx);
/* Bytes of split workspace for total_q_tokens = B * max_q_len q rows (covers ragged cu_seqlens_q below that).  head_dim D of tgis_attn_paged: 64, 96 or 128. */
int64_t tgis_attn_workspace_bytes(int64_t total_q_tokens, int H, int Hkv, int D, int num_splits);
/* Causal softmax(q k^T * scale) v over the paged cache.
 *   q: [total_q, H, D] with token stride ld_q (elements); out: [total_q, H*D] contiguous (ld_out = 0 or
 *   H*D), or — decode, B <= 64 — in fragment order for the o_proj GEMM (ld_out = TGIS_LD_FRAGMENTS).
 *   cu_seqlens_q [B+1] int32: q token offsets per sequence (decode: arange).
 *   ctx_lens [B] int32: tokens of each sequence present in the cache INCLUDING the q tokens.
 *   block_tables [B, max_pages] int32: page ids.  q token i of sequence b sits at position
 *   ctx_lens[b] - q_len_b + i and attends to cache positions <= its own.
 *   max_q_len / max_ctx are launch-shape bounds (host ints). */
int tgis_attn_paged(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                    const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                    const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv, int D,
                    int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* tgis_attn_paged over pools of element kv_dtype (TGIS_KV_*; utils/flash_attn.py:43-78).  A one-byte cache is read as
 * k_scale * e4m3(k) and v_scale * e4m3(v): k_scale is folded into the softmax scale and 1 / v_scale into its normaliser
 * (no per-element multiply).  Same launch forms, splits and workspace as tgis_attn_paged. */
int tgis_attn_paged_kv8(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool, const int32_t* block_tables,
                        int64_t max_pages, const int32_t* ctx_lens, const int32_t* cu_seqlens_q, void* out, int64_t ld_out,
                        int64_t B, int H, int Hkv, int D, int64_t max_q_len, int64_t max_ctx, float scale, int dtype,
                        int num_splits, void* workspace, int64_t workspace_bytes, void* stream, int kv_dtype,
                        float k_scale, float v_scale);
/* tgis_attn_paged with a mask over each sequence's own q rows: the verify step of speculative decoding over several
 * candidates per request, which the reference flattens into one forward (utils/paged.py:162-330; its attention call is
 * utils/flash_attn.py:43-78).  q_mask [total_q] uint64, one word per q row: bit j of q_mask[i] is set when q row i of a
 * sequence attends to that sequence's q row j, whose key sits at cache position ctx_lens[b] - q_len_b + j.  Keys below
 * ctx_lens[b] - q_len_b are always visible.  The mask is ANDed with the causal bound: a set bit above the row's own index is
 * ignored; a row with no visible key at all gives zeros.  Any per-row bitmask is served, not only trees.
 * Only the decode form (max_q_len * next_pow2(min(H / Hkv, 16)) <= 64, so q_len <= 64: one word per row); anything else, or a
 * NULL q_mask, is TGIS_EINVAL before any launch.  Key splits (callers take num_splits from tgis_attn_num_splits_q), workspace
 * (tgis_attn_workspace_bytes), both merges and `out` are those of tgis_attn_paged.  The mask changes scores only: every load
 * the launch issues is one tgis_attn_paged issues for the same ctx_lens and cu_seqlens_q. */
int tgis_attn_paged_tree(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool, const int32_t* block_tables,
                         int64_t max_pages, const int32_t* ctx_lens, const int32_t* cu_seqlens_q, void* out, int64_t ld_out,
                         int64_t B, int H, int Hkv, int D, int64_t max_q_len, int64_t max_ctx, float scale, int dtype,
                         int num_splits, void* workspace, int64_t workspace_bytes, void* stream, const uint64_t* q_mask);
/* tgis_attn_paged_tree over pools of element kv_dtype, as tgis_attn_paged_kv8 is to tgis_attn_paged (utils/flash_attn.py:43-78). */
int tgis_attn_paged_tree_kv8(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                             const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                             const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv, int D,
                             int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits, void* workspace,
                             int64_t workspace_bytes, void* stream, int kv_dtype, float k_scale, float v_scale,
                             const uint64_t* q_mask);

/* tgis_attn_paged under a sliding window (Mistral's config.sliding_window; the reference has no such model, the semantics
 * are those of transformers' MistralForCausalLM; call site utils/flash_attn.py:43-78): the q row at cache position p attends
 * to the `window` positions p - window < j <= p, its own among them.  window >= 1.  A window that no row of the launch
 * reaches (max_ctx <= window) is the tgis_attn_paged launch, bit for bit.
 * max_q_len == 1: the decode kernel's window variant.  Pages wholly below a sequence's window are not loaded and their
 * block_tables entries are not read; key splits divide the visible pages (callers take num_splits from
 * tgis_attn_num_splits(B, Hkv, H, 1, min(max_ctx, window + 31))), workspace (tgis_attn_workspace_bytes), both merges, `out`
 * and ld_out = TGIS_LD_FRAGMENTS are those of tgis_attn_paged.
 * max_q_len > 1: always the prefill kernel's window variant, whatever the group size; num_splits must be 1.
 * window < 1, num_splits > 1 with max_q_len > 1, or a missing / short workspace with splits is TGIS_EINVAL before any launch. */
int tgis_attn_paged_window(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool, const int32_t* block_tables,
                           int64_t max_pages, const int32_t* ctx_lens, const int32_t* cu_seqlens_q, void* out, int64_t ld_out,
                           int64_t B, int H, int Hkv, int D, int64_t max_q_len, int64_t max_ctx, float scale, int dtype,
                           int num_splits, void* workspace, int64_t workspace_bytes, void* stream, int64_t window);
/* tgis_attn_paged_window over pools of element kv_dtype, as tgis_attn_paged_kv8 is to tgis_attn_paged (utils/flash_attn.py:43-78). */
int tgis_attn_paged_window_kv8(const void* q, int64_t ld_q, const void* k_pool, const void* v_pool,
                               const int32_t* block_tables, int64_t max_pages, const int32_t* ctx_lens,
                               const int32_t* cu_seqlens_q, void* out, int64_t ld_out, int64_t B, int H, int Hkv, int D,
                               int64_t max_q_len, int64_t max_ctx, float scale, int dtype, int num_splits, void* workspace,
                               int64_t workspace_bytes, void* stream, int kv_dtype, float k_scale, float v_scale,
                               int64_t window);

/* ---- KV-cache statistics (replaces nothing in the reference, which has no quantised cache: the calibration pass of the
 *      one-byte cache, utils/kv_cache.py) -------------------------------------------------------------- */
/* Max |x| per kv head over the tokens that B sequences hold in ONE layer's 16-bit pools (dtype TGIS_F16 / TGIS_BF16; D 64,
 * 96 or 128), max-merged into out [2][Hkv] fp32: row 0 = k (as cached: after rotary), row 1 = v.  The caller zeroes `out`
 * once; calls accumulate (a max is exact in any order: the result is bit-identical to a host restatement).
 *   block_tables [B, max_pages] int32, ctx_lens [B] int32: only tokens < ctx_lens[b] count — the slots past the last token
 *   of a partly filled page are ignored, table entries past a sequence's last page are never dereferenced, ctx_lens[b] = 0
 *   contributes nothing.  No allocation, no sync; B = 0 returns TGIS_OK. */
int tgis_kv_absmax(const void* k_pool, const void* v_pool, const int32_t* block_tables, int64_t max_pages,
                   const int32_t* ctx_lens, int64_t B, int Hkv, int D, int dtype, float* out, void* stream);

/* ---- elementwise --------------------------------------------------------------------------------- */
/* out[T,I] = act(gate_up[T,0:I]) * gate_up[T,I:2I]; act 1 = SiLU (flash_llama_modeling.py:332-335). */
int tgis_act_mul(const void* gate_up, void* out, int64_t T, int64_t I, int act, int dtype, void* stream);
/* out[T,I] = gelu(x) ; approx 1 = tanh (flash_santacoder_modeling.py:303-307). */
int tgis_gelu(const void* x, void* out, int64_t n, int tanh_approx, int dtype, void* stream);
/* out[T,E] = table[ids[T]] (+ pos_table[positions[T]] if non-NULL); ids int64. Out-of-range id -> 0 row
 * (TensorParallelEmbedding's null row, utils/layers.py:325-357); ids are offset by -id_offset first. */
int tgis_embedding(const int64_t* ids, const void* table, const int32_t* positions,
                   const void* pos_table, void* out, int64_t T, int64_t E, int64_t vocab_rows,
                   int64_t id_offset, int dtype, void* stream);
/* Decode-step bookkeeping in one launch (flash_causal_lm.py:457-458,499 on device):
 * positions[b] (int32) -> slots[b] = block_tables[b][pos/32]*32 + pos%32 ; ctx_lens[b] = pos+1. */
int tgis_decode_slots(const int32_t* positions, const int32_t* block_tables, int64_t max_pages,
                      int32_t* slots, int32_t* ctx_lens, int64_t B, void* stream);
/* What follows a decode step on the device, in one launch (flash_causal_lm.py:457 `cu_seqlens.add_(cu_seqlens_q)`, :499
 * `position_ids += 1`, :533-535 `all_input_ids_tensor.scatter_(1, position_ids, next ids)`): position_ids int64 [B] += 1;
 * all_input_ids[b][position_ids[b]] = ids[b] (row stride ld_all, NULL: skip); ids_copy [B] = ids (NULL: skip; the caller's
 * next `input_ids`, since `ids` is a buffer the next step overwrites); cu_seqlens int32 [B + 1] += cu_seqlens_q (NULL:
 * skip); stage_ids int64 [B] / stage_positions int32 [B]: the same new ids / positions once more, e.g. into the static
 * input buffers of a captured decode step (NULL: skip). */
int tgis_decode_advance(const int64_t* ids, int64_t* ids_copy, int64_t* position_ids, int64_t* all_input_ids,
                        int64_t ld_all, int32_t* cu_seqlens, const int32_t* cu_seqlens_q, int64_t* stage_ids,
                        int32_t* stage_positions, int64_t B, void* stream);

/* ---- prompt-lookup speculative decoding (greedy requests) -----------------------------------------
 * The reference verifies several drafted tokens per forward (models/paged_causal_lm.py:481-562 the step, :630-657 when it
 * is taken, utils/paged.py the flattened inputs and the acceptance); its drafter is a trained MLP speculator, here the
 * drafts are looked up in the request's own context.  K drafts per request, 0 <= K <= 7; a verify forward has K + 1 rows
 * per request: its latest token, then its drafts.  No allocation, no sync; B = 0 returns TGIS_OK. */
/* The K + 1-row form of tgis_decode_slots (utils/paged.py prepare_inputs_with_speculation: input ids, positions and slot
 * mapping of the flattened candidates).  positions [B] int32: position of each request's latest token; latest_ids [B]
 * int64; drafts [B, K] int64 (K = 0: may be NULL).  Row r = b (K + 1) + j: input_ids[r] = j ? drafts[b][j - 1] :
 * latest_ids[b]; positions_out[r] = positions[b] + j; slots[r] = block_tables[b][pos / 32] * 32 + pos % 32 of that
 * position (a table index past max_pages - 1 is clamped to it); ctx_lens[b] = positions[b] + K + 1. */
int tgis_spec_stage(const int32_t* positions, const int64_t* latest_ids, const int64_t* drafts, int64_t K,
                    const int32_t* block_tables, int64_t max_pages, int64_t* input_ids, int32_t* positions_out,
                    int32_t* slots, int32_t* ctx_lens, int64_t B, void* stream);
/* The K + 1-token form of tgis_decode_advance (utils/paged.py process_outputs_with_speculation: the longest correct
 * candidate prefix; paged_causal_lm.py:530-562 what is emitted and the new inputs).  argmax_ids int64 / argmax_logprobs f32
 * [B, K + 1]: the greedy choice behind every verify row; drafts [B, K].  With a = the longest prefix of argmax_ids[b][j] ==
 * drafts[b][j], request b emits the a + 1 tokens argmax_ids[b][0 .. a]:
 *   n_emit [B] int32 = a + 1;  out_ids int64 / out_logprobs f32 [B, K + 1] (NULL: skip): the emitted entries, then -1 / 0;
 *   all_input_ids[b][position_ids[b] + 1 + j] = emitted id j (row stride ld_all, NULL: skip; columns >= ld_all are not
 *   written);  position_ids int64 [B] += n_emit;  latest_ids [B] (NULL: skip) = the last emitted id;  cu_seqlens int32
 *   [B + 1] (NULL: skip): entry b += sum of n_emit[i], i < b;  stage_ids int64 [B] / stage_positions int32 [B] (NULL:
 *   skip): the new latest ids / positions once more, e.g. into the static inputs of a captured step.
 * One workgroup serves the batch.  K = 0 is tgis_decode_advance (cu_seqlens_q = arange) bit for bit. */
int tgis_spec_accept(const int64_t* argmax_ids, const float* argmax_logprobs, const int64_t* drafts, int64_t K,
                     int32_t* n_emit, int64_t* out_ids, float* out_logprobs, int64_t* latest_ids, int64_t* position_ids,
                     int64_t* all_input_ids, int64_t ld_all, int32_t* cu_seqlens, int64_t* stage_ids,
                     int32_t* stage_positions, int64_t B, void* stream);
/* tgis_spec_accept behind a verify step whose rows were chosen by tgis_warp_sample_verify instead of the argmax
 * (paged_causal_lm.py:630-641 is where the reference leaves sampled requests out of speculation; here they are verified).
 * chosen_ids / chosen_logprobs [B, K + 1] stand where argmax_ids / argmax_logprobs stand above and every output is computed
 * the same way by the same kernel.  In addition, do_sample int [B] (NULL: nothing more, the call equals tgis_spec_accept
 * bit for bit) and rng [B, 2] uint64 (seed, offset), the streams of tgis_warp_sample: a request with do_sample[b] != 0 has
 * rng[b].offset += n_emit[b], one draw per emitted token (utils/tokens.py:32-41 a Sampling draws once per token). */
int tgis_spec_accept_sampled(const int64_t* chosen_ids, const float* chosen_logprobs, const int64_t* drafts, int64_t K,
                             int32_t* n_emit, int64_t* out_ids, float* out_logprobs, int64_t* latest_ids,
                             int64_t* position_ids, int64_t* all_input_ids, int64_t ld_all, int32_t* cu_seqlens,
                             int64_t* stage_ids, int32_t* stage_positions, const int* do_sample, uint64_t* rng, int64_t B,
                             void* stream);
/* The drafter (stands where the reference calls its speculator, utils/paged.py prepare_inputs_with_speculation): prompt
 * lookup.  The context of request b is all_input_ids[b][0 .. len), len = position_ids[b] + 1 (clamped to [0, ld_all]).  For
 * n = N .. 1 (1 <= N <= 4): the largest j with j + n < len and tokens[j .. j + n) == tokens[len - n .. len); the first n
 * that has one wins.  drafts[b] [K] int64 (1 <= K <= 7) = tokens[j + n .. j + n + K), id 0 where the context ends;
 * hits[b] int32 = n, or 0 with all-zero drafts when nothing matched; hits_copy [B] (NULL: skip) receives hits once more
 * (the buffer that travels to the host).  One workgroup per request. */
int tgis_spec_propose(const int64_t* all_input_ids, int64_t ld_all, const int64_t* position_ids, int64_t K, int64_t N,
                      int64_t* drafts, int32_t* hits, int32_t* hits_copy, int64_t B, void* stream);

/* ---- several candidates per request: the verify step as a token tree ------------------------------
 * The reference verifies top_k candidates of n_predict tokens per request in one forward and keeps the one with the longest
 * correct prefix (utils/paged.py:162-330, `best_guess = n_correct.argmax(1)`).  Here: C candidates (1 <= C <= 8) of K drafts
 * (0 <= K <= 7; C > 1 needs K >= 1), R = 1 + C K <= 64 rows per request.  With pos the position of the latest token, row 0 is
 * that token (rotary position pos, cache position pos) and row 1 + c K + j is draft j of candidate c: rotary position
 * pos + 1 + j (its depth), cache position pos + 1 + c K + j (its row).  A row attends to the cache below pos, to row 0 and to
 * its own candidate's rows up to itself (tgis_attn_paged_tree).  No allocation, no sync; B = 0 returns TGIS_OK. */
/* The R-row form of tgis_spec_stage (utils/paged.py prepare_inputs_with_speculation).  drafts [B, C, K] int64.  Row
 * r = b R + i: input_ids[r] = the row's token; positions_out[r] = its rotary position (by depth); slots[r] = the slot of its
 * cache position (by row), the table index clamped as tgis_spec_stage clamps it; ctx_lens[b] = positions[b] + R.  C = 1 is
 * tgis_spec_stage bit for bit.  (C is an argument tgis_spec_stage does not have.) */
int tgis_spec_tree_stage(const int32_t* positions, const int64_t* latest_ids, const int64_t* drafts, int64_t C, int64_t K,
                         const int32_t* block_tables, int64_t max_pages, int64_t* input_ids, int32_t* positions_out,
                         int32_t* slots, int32_t* ctx_lens, int64_t B, void* stream);
/* tgis_spec_accept over C candidates (utils/paged.py process_outputs_with_speculation: the first maximum of n_correct).
 * argmax_ids int64 / argmax_logprobs f32 [B, R]; drafts [B, C, K].  a_c = the longest j such that for every draft i < j of
 * candidate c the choice behind its parent row equals it; the parent of draft 0 is row 0, of draft i > 0 row 1 + c K + i - 1.
 * best [B] int32 = the lowest c with the largest a_c.  With a = a_best, request b emits the a + 1 choices along that path:
 * argmax_ids[b][0], then those behind drafts 0 .. a - 1 of candidate best.  n_emit, out_ids / out_logprobs [B, K + 1],
 * latest_ids, position_ids, all_input_ids, cu_seqlens, stage_ids and stage_positions are those of tgis_spec_accept, NULL
 * where it allows NULL.  One workgroup serves the batch.  C = 1 is tgis_spec_accept bit for bit (best = 0). */
int tgis_spec_tree_accept(const int64_t* argmax_ids, const float* argmax_logprobs, const int64_t* drafts, int64_t C, int64_t K,
                          int32_t* n_emit, int32_t* best, int64_t* out_ids, float* out_logprobs, int64_t* latest_ids,
                          int64_t* position_ids, int64_t* all_input_ids, int64_t ld_all, int32_t* cu_seqlens,
                          int64_t* stage_ids, int32_t* stage_positions, int64_t B, void* stream);
/* Behind tgis_spec_tree_accept: the cache as if the best candidate alone had been verified (the reference keeps the best
 * candidate's cache entries and frees the others', utils/paged.py:303-315).  For every request with best > 0 and n_emit > 1, the keys and values at
 * cache position pos + 1 + best K + j move to pos + 1 + j, j < n_emit - 1, in every layer and kv head, in ONE launch.
 *   k_pool / v_pool: layer 0's pools, [num_pages, Hkv, 32 D] elements of elem_bytes (2: f16 / bf16, 1: e4m3 codes) in the
 *   orders of the KV page layout (K moves as 8-element runs, V element by element); layer l's pools start layer_stride
 *   ELEMENTS behind layer l - 1's (16-byte aligned).  Bytes are copied, nothing is requantised.
 *   new_positions [B] int32: the positions tgis_spec_tree_accept left (its stage_positions): pos = new_positions[b] - n_emit[b].
 *   best / n_emit [B] int32 as tgis_spec_tree_accept wrote them, read on the device (the call needs no host value).
 * Source and destination positions never overlap: at most K positions move (n_emit - 1 <= K), the destinations lie in
 * [pos + 1, pos + K] and, with best >= 1, every source lies at pos + 1 + K or beyond (best K >= K positions behind its
 * destination), so no ordering between the copies is needed.  best is clamped to [0, C - 1], n_emit to [1, K + 1], table indices to
 * [0, max_pages - 1] and page ids to [0, num_pages - 1]: a wrong value can never address past a request's table or the pool. */
int tgis_spec_tree_commit(void* k_pool, void* v_pool, int64_t layer_stride, int64_t num_layers, int64_t num_pages,
                          const int32_t* block_tables, int64_t max_pages, const int32_t* new_positions, const int32_t* best,
                          const int32_t* n_emit, int64_t C, int64_t K, int64_t B, int Hkv, int D, int elem_bytes,
                          void* stream);
/* tgis_spec_propose for C candidates (stands where the reference asks its speculator for top_k candidates, utils/paged.py
 * prepare_inputs_with_speculation).  Match sites are visited with n from N down to 1 and, within one n, from the latest site
 * to the earliest; a site becomes the next candidate if the first token of its continuation differs from the first token of
 * every candidate already taken, so candidates part at depth 1.  drafts [B, C, K] int64, zeros for candidates that were not
 * found (and where the context ends); hits[b] = the n of the first candidate, 0 if there is none; hits_copy as in
 * tgis_spec_propose.  One workgroup per request.  C = 1 is tgis_spec_propose bit for bit. */
int tgis_spec_propose_multi(const int64_t* all_input_ids, int64_t ld_all, const int64_t* position_ids, int64_t C, int64_t K,
                            int64_t N, int64_t* drafts, int32_t* hits, int32_t* hits_copy, int64_t B, void* stream);

/* ---- MLP speculator, the reference's drafter (models/paged_causal_lm.py:481-562, utils/paged.py:20-38,208) ------------
 * Head i of K <= n_predict:  s = proj_i x + alpha emb_i[t];  x = gelu_erf(rmsln_i(s));  t = argmax(head_i x), starting from
 * x = the post-final-norm hidden state behind a request's latest token t.  proj_i and head_i are tgis_dense_gemm on
 * prepared images (head_i with out_f32 = 1), the argmax is tgis_argmax_logprob; these three entry points are the rest of
 * the chain.  No allocation, no sync; B = 0 returns TGIS_OK. */
/* The chain's input (paged_causal_lm.py:192,261 batch.embeds; :500-520 the rows kept behind a verify step).  hidden
 * [B K1, E] model dtype, 1 <= K1 <= 8; request b takes row b K1 + clamp(n_emit[b], 1, K1) - 1 (n_emit int32 [B], NULL: row
 * b K1).  out [B, E] and out_copy [B, E] (NULL: skip) receive the row, bit for bit, or with scale_input != 0 the row times
 * rsqrt(mean(x^2) + eps) / sqrt(2) (fp32 statistics, one rounding).  E % 8 == 0. */
int tgis_spec_mlp_input(const void* hidden, const int32_t* n_emit, int64_t K1, void* out, void* out_copy, int64_t B,
                        int64_t E, int scale_input, float eps, int dtype, void* stream);
/* Between the two GEMMs of a head (the speculator's emb + LayerNormParameterized + GELU).  proj_out [B, I] model dtype,
 * tok int64 [B] (clamped to [0, V)), emb [V, I], ln_weight / ln_bias [I]:
 *   s = proj_out[b] + alpha emb[tok[b]];  x_out[b] = gelu_erf(s rsqrt(mean(s^2) + eps) ln_weight + ln_bias)
 * in fp32 with one rounding; no mean is subtracted.  One workgroup per row; I % 8 == 0, I <= 16384. */
int tgis_spec_mlp_state(const void* proj_out, const int64_t* tok, const void* emb, int64_t V, const void* ln_weight,
                        const void* ln_bias, float alpha, float eps, void* x_out, int64_t B, int64_t I, int dtype,
                        void* stream);
/* Behind the chain (utils/paged.py prepare_inputs_with_speculation takes the candidates request-major): toks [K, B] int64,
 * row i written by the argmax of head i, into drafts [B, K] int64, 1 <= K <= 7; hits [B] int32 and hits_copy [B] (NULL:
 * skip) are set to 1, the tgis_spec_propose convention for "this request has drafts". */
int tgis_spec_mlp_drafts(const int64_t* toks, int64_t K, int64_t* drafts, int32_t* hits, int32_t* hits_copy, int64_t B,
                         void* stream);

/* ---- greedy sampling (Greedy + log_softmax + gather, utils/tokens.py:44-46,238-271,388-397) ------ */
/* Per row: token = argmax (lowest id on ties), logprob = logit[token] - logsumexp(row).
 * logits [B,V] f32 (logits_f32 != 0) or model dtype. ids_out int64 [B], logprob_out f32 [B].
 * scratch (may be NULL): tgis_argmax_scratch_bytes(B) bytes of device memory the call may use until it completes; with it
 * a small batch's rows are split over several workgroups each (two launches; same ids, logprobs within summation order). */
int64_t tgis_argmax_scratch_bytes(int64_t B);
int tgis_argmax_logprob(const void* logits, int64_t ld, int64_t B, int64_t V, int logits_f32, int dtype,
                        int64_t* ids_out, float* logprob_out, void* scratch, int64_t scratch_bytes, void* stream);

/* ---- next-token chooser for a heterogeneous batch -------------------------------------------------
 * One launch for what HeterogeneousNextTokenChooser.__call__ (utils/tokens.py:242-270) does with the
 * Heterogeneous* processors (utils/logits_process.py:93-402) and Sampling / HeterogeneousSampling
 * (utils/tokens.py:32-41,336-385), in the reference's order: EOS mask or length penalty, repetition
 * penalty, temperature, top-k, top-p, typical-p, then argmax (greedy rows) or a categorical draw.
 *   logits  [B,V] f32 (read only);  scores [B,V] f32 out: the warped scores, -inf where filtered — the
 *           tensor get_token_info (utils/tokens.py:388-425) takes top-n tokens and ranks from.
 *   Per-row parameter arrays, each may be NULL (= processor not instantiated): temperature; top_k
 *   (0 = off); top_p_cut = 1 - top_p as the host rounded it (<= 0 = off); typical_p (>= 1 = off);
 *   rep_penalty (1 = off) with input_ids [B,L] int64 (row stride ld_ids; padding included, as the
 *   reference passes it) and exclude_id (the id the penalty leaves alone, -1 = none);
 *   eos_adjust [B,2] = (mode, factor): mode 1 sets scores[eos_id] = -inf (min_new_tokens), mode 2
 *   scores[eos_id] += |scores[eos_id]| * factor (length penalty); do_sample [B] (NULL = all greedy).
 *   rng [B,2] uint64 (seed, offset): the request's Philox4x32-10 stream; offset += 1 per draw.
 * Outputs: next_ids int64 [B]; next_logprob f32 [B] = log_softmax(scores)[id]; lse f32 [B] =
 * logsumexp(scores) (log_softmax of a row = scores - lse). */
int tgis_warp_sample(const float* logits, int64_t ld_logits, float* scores, int64_t ld_scores, int64_t B,
                     int64_t V, const float* temperature, const int* top_k, const float* top_p_cut,
                     const float* typical_p, const float* rep_penalty, const int64_t* input_ids,
                     int64_t ld_ids, int64_t L, int64_t exclude_id, const float* eos_adjust, int64_t eos_id,
                     const int* do_sample, uint64_t* rng, int64_t* next_ids, float* next_logprob, float* lse,
                     void* stream);
/* The verify form of tgis_warp_sample: the chooser behind every row of a verify forward of speculative decoding
 * (models/paged_causal_lm.py:481-562 the step; :630-641 the reference speculates for greedy requests only, this entry
 * lets sampled and warped ones be verified by the draw their plain step would have made).  B requests, K drafts each,
 * 0 <= K <= 7; logits / scores hold B (K + 1) rows, row r = b (K + 1) + j being request b's j-th verify row.
 *   Row r takes request b's parameters from the same [B] arrays as above (temperature, top_k, top_p_cut, typical_p,
 *   rep_penalty, do_sample): nothing is expanded on the host.
 *   Repetition-penalty context of row (b, j): input_ids[b][0 .. L) as above (padding and exclude_id included), then
 *   drafts[b][0 .. j) (drafts [B, K] int64; K = 0: may be NULL); out-of-range ids are skipped, duplicates penalised once.
 *   eos_adjust [B, K + 1, 2]: (mode, factor) per row (utils/tokens.py:242-256 stepped once per row by the host).
 *   A sampled row draws with (seed, offset + j) of rng[b]; rng [B, 2] is READ ONLY here (tgis_spec_accept_sampled
 *   advances it by the tokens emitted).
 * Outputs: next_ids int64, next_logprob f32, lse f32 [B, K + 1]; scores [B (K + 1), V].  Row (b, j) is, bit for bit, what
 * tgis_warp_sample gives for a row with b's parameters, that context and the stream state (seed, offset + j); K = 0 is
 * tgis_warp_sample except for the untouched rng.  No allocation, no sync; B = 0 returns TGIS_OK. */
int tgis_warp_sample_verify(const float* logits, int64_t ld_logits, float* scores, int64_t ld_scores, int64_t B,
                            int64_t K, int64_t V, const float* temperature, const int* top_k, const float* top_p_cut,
                            const float* typical_p, const float* rep_penalty, const int64_t* input_ids, int64_t ld_ids,
                            int64_t L, int64_t exclude_id, const int64_t* drafts, const float* eos_adjust, int64_t eos_id,
                            const int* do_sample, const uint64_t* rng, int64_t* next_ids, float* next_logprob, float* lse,
                            void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TGIS_HIP_H */
