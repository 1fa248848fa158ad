/* vqs_debug.h -- test hooks and lab switches of libvqs_hip.so.  NOT part of the drop-in boundary (include/vqs.h): nothing the
 * reference-side binding of INTEGRATION.md needs is declared here.  The parity tests (tests/test_gpu_stage_locked.py,
 * tests/test_gpu_bench_config.py, tests/test_properties.py) and the lab tools (tools/lab_call.py) are the only callers.
 * vqs_debug_gemm_launch: single launches of the GEMM's Qwen2.5-VL epilogues (tests/test_gpu_gemm_epilogues.py, profiles/gemm_epilogue_kernels.md). */
#ifndef VQS_DEBUG_H
#define VQS_DEBUG_H
#include "vqs.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Stage tap (parity tests): register a caller-owned device buffer for a named intermediate of the NEXT passes; when a
 * pass produces it, it is copied there on the pass's stream (device to device, no synchronisation).  The workspace
 * buffers are reused layer after layer, so this is how a test reads EVERY layer's tensors and checks each launch
 * against the oracle on the engine's own inputs (tests/test_gpu_stage_locked.py).  Names: "<stack>.<layer>.<what>" or
 * "<stack>.<what>": vit.{patch_out,h0,feat_in,pmid}; vit.<i>.{xn0,q,k,v,attn,d_attn,xn1,mid,d_mlp};
 * enc.emb; enc.<i>.{xn0,q,k,v,attn,d_attn,xn1,ff,d_ff}; dec.emb; dec.<i>.{xn0,qkv,sattn,d_self,xn1,cq,cqk,cscores,cprobs,cctx,
 * cattn,d_cross,xn2,ff,d_ff}.  bytes = capacity of d_dst (a pass fails with VQS_ERR_WORKSPACE if it is too small);
 * name == NULL clears every tap, d_dst == NULL removes one.  With no tap registered a pass pays one empty() test. */
int vqs_debug_tap(vqs_handle* h, const char* name, void* d_dst, size_t bytes);
/* Host-side test hook, no device access: the element offsets into a head-major [B, hx, S, hdim] tensor that the GEMM's
 * head-major epilogue (EPI_HEADS, the QKV projections' scatter -- HF modeling_t5.py:311-323 view/transpose) uses for the
 * rows row0 + 8k, k = 0..n-1, computed by the SAME inline functions as the kernel (one division, then steps).  S >= 8. */
int vqs_debug_heads_rows(int32_t row0, int32_t S, int32_t hx, int32_t hdim, int32_t n, int64_t* off_out);
/* Host-side test hook, no device access: the tile every workgroup slot of a persistent GEMM launch (grid workgroups, a multiple
 * of 8) computes under tile order (gm, ns), by the SAME inline functions as the launcher and the kernels: out[4*i .. 4*i+3] =
 * (slot, m0, n0, batch entry) for the M x N x K x batch problem, i < number of tiles.  gm = ns = 0 asks for the library's choice
 * by shape (the Infinity-Cache working-set rule, vqs_kernels.h resolve_tile_order).  Returns the resolved gm | ns << 8 (an
 * illegal ns falls back to 1) or a negative error. */
int vqs_debug_tile_order(int32_t M, int32_t N, int32_t K, int32_t batch, int32_t gm, int32_t ns, int32_t grid, int32_t* out);
/* Host-side test hook, no device access: the kernel family a vqs_gemm launch of this shape resolves to, by the launcher's own
 * function (gemm.hip gemm_plan, read through vqs_debug_gemm_plan below; bias-free, ldc = N): 10 = the quad form (four waves, 16x16x32 MFMAs; operand offsets relative to the output tile, no
 * size limit), 3 = an 8-wave persistent kernel (32-bit byte offsets into a batch entry's operands), 12 = the stream form (<= 128 rows
 * per batch entry, W streamed from HBM; bitwise the results of 3: one family), 13 = a quad call site's few-row launch in the slim form
 * (gemm_slim.inc, round 6: 128 x 128 tiles for launches whose 256 x 256 tiles leave most CUs idle; bitwise the results of 10: one family),
 * 0 = one tile per workgroup (64-bit pointers), -1 = not launchable (the launcher's argument checks included: a refused variant, K not a multiple of 64, ...).  Two properties the tests pin: the form of a bf16-result launch is a function of the
 * epilogue and the WEIGHT's shape only, never of M (a pair's bits must not depend on its batch), and an operand of 4 GiB or more
 * per batch entry never reaches a 32-bit kernel (it falls back to family 0 where that computes the same function, else -1). */
int vqs_debug_gemm_form(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t epilogue, int32_t batch, int32_t variant,
                        int32_t S, int32_t inner, int32_t inner_kv);
/* Host-side test hook, no device access: the whole plan of a GEMM launch, by the launcher's own function (gemm.hip gemm_plan, where the rule
 * is stated).  launch[VQS_GEMM_PLAN_FIELDS] describes the launch by integers only (unused fields 0):
 *   0 M, 1 N, 2 K, 3 lda, 4 ldw, 5 ldc, 6 epilogue, 7 batch, 8 variant (bits 0-7 as vqs_gemm), 9 S, 10 inner, 11 inner_kv, 12 hd, 13 hd_src, 14 Hkv, 15 operand type (GemmParams::f16, 0-4),
 *   16 l2_touch override (0 by shape, 1 on, 2 off), 17 split_off (elements; 0 = no split result), 18 flags, 19 gate_act, 20 rowss_parts, 21 ldh;
 *   flags: 1 bias present, 2 row scale (rowss_in) present, 4 no_stream, 8 rope cos table, 16 rope sin table, 32 the fused residual +
 *   RMSNorm operands (hres, lnw, rowss_out) present, 64 a launch of an engine handle (its batched launches follow the library rule).
 * Returns 1 and plan[0..4] = kernel family (0 tile, 1 tile ping-pong, 2 persistent, 3 persistent ping-pong, 4 stream, 5 quad, 6 slim:
 * vqs_kernels.h GemmKernel), the persistent kernel's L2 touch (0 / 2), the operand type the kernel is instantiated for, workgroups,
 * threads per workgroup; 0 where the launcher refuses the launch (hipErrorInvalidValue); VQS_ERR_INVALID for a bad call of the hook. */
#define VQS_GEMM_PLAN_FIELDS 22
int vqs_debug_gemm_plan(const int32_t* launch, int32_t n, int32_t* plan);
/* Device-side test hook: ONE launch of the GEMM with every field of its parameter block in the caller's hands (the Qwen2.5-VL row's epilogues: 128-lane
 * heads, narrow heads in wide slots, the grouped-query scatter, the SiLU gate and the gated bias, the scaled fp16 families, the rotary embedding inside the
 * head-major epilogue -- tests/test_gpu_gemm_epilogues.py).  It fills the block by the function vqs_debug_gemm_plan fills it with and calls launch_gemm,
 * nothing else: no copy, no synchronisation.
 *   launch[VQS_GEMM_LAUNCH_FIELDS]: the VQS_GEMM_PLAN_FIELDS integers above, then 22 H (heads of the q tensor: EPI_HEADS, > 0 there).  The first 22 given to
 *     vqs_debug_gemm_plan name the kernel this launch runs.  A flag that is set requires its pointer below, and a pointer without its flag is an error.
 *   ptrs[VQS_GEMM_LAUNCH_PTRS]: 0 A, 1 W, 2 C (every epilogue but EPI_HEADS), 3 bias (bf16 [N]; gated: packed column order), 4-6 heads_out[0..2] (EPI_HEADS:
 *     q [B, H, S, hd], k and v [B, Hkv, S, hd]), 7 rope_cos, 8 rope_sin (fp32 [M, 64]), 9 rowss_in (fp32 [rowss_parts][M]); unused ones NULL.
 *   scales[VQS_GEMM_LAUNCH_SCALES]: 0 acc_scale, 1 out_scale (operand types 3 and 4; 1 otherwise), 2 rs_invd, 3 rs_eps (row scale).
 * A launch the launcher refuses returns VQS_ERR_INVALID and nothing is launched; so does a bad call of the hook.  Batched launches (batch > 1), EPI_RESID_RMS,
 * EPI_F32_RESID, split results and the handle flag stay with vqs_debug_gemm_batched / vqs_gemm_rms / vqs_gemm: VQS_ERR_INVALID here. */
#define VQS_GEMM_LAUNCH_FIELDS 23
#define VQS_GEMM_LAUNCH_PTRS 10
#define VQS_GEMM_LAUNCH_SCALES 4
int vqs_debug_gemm_launch(const int32_t* launch, int32_t n, const void* const* ptrs, int32_t nptrs, const float* scales, int32_t nscales, void* stream);
/* Device-side test hook: the batched form of vqs_gemm that the engine's decoder launches (entry z reads A + z*sA, W + z*sW and
 * writes C + z*sC, strides in elements; EPI_F32 or EPI_BF16 only), with the split-bf16 result store (split_off != 0: the lo plane
 * bf16(acc - hi) goes to C + split_off) and no_stream = 1 keeping the launch off the stream form (csrc/gemm_stream.inc).  The
 * per-kernel tests hold the stream form against the persistent kernel and against per-entry one-tile launches, bitwise. */
int vqs_debug_gemm_batched(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldc,
                           int32_t epilogue, int32_t batch, int64_t sA, int64_t sW, int64_t sC, int64_t split_off, int32_t no_stream,
                           int32_t variant, void* stream);
/* Device-side test hooks for the fp16 instantiations (options vit_fp16 / enc_fp16): the single-kernel entry points of vqs.h name bf16
 * tensors; these run the same launches on IEEE fp16 ones so that the per-kernel tests cover the fp16 kernels at shapes of their own
 * (edge tiles, ragged key lengths), not only at the tower's / encoder's shapes through whole passes.
 *   vqs_debug_attention_f16: vqs_attention with q / k / v / out in fp16 (d_bias_table NULL: the vision tower's kernel; non-NULL: the T5
 *     encoder's, with the per-head position-bias table and the key-length mask).
 *   vqs_debug_norm16: vqs_norm_deferred's forms with 16-bit types by `types`: 1 = RMSNorm, bf16 deltas in, fp16 operand out (T5 encoder),
 *     3 = LayerNorm, fp16 deltas in, fp16 operand out (vision tower); d_delta may be NULL (plain norm).  Other combinations: VQS_ERR_INVALID.
 * The fp16 GEMMs are reached through vqs_gemm's variant word (bits 27-28, vqs.h). */
int vqs_debug_attention_f16(const void* d_q, const void* d_k, const void* d_v, void* d_out, const float* d_bias_table, const int32_t* d_key_len,
                            int32_t B, int32_t H, int32_t S, float scale, void* stream);
int vqs_debug_norm16(int32_t kind, float* d_x, const void* d_delta, const void* d_delta2, int32_t store_x, const void* d_w, const void* d_b,
                     void* d_out, int32_t M, int32_t D, float eps, int32_t types, void* stream);
/* Single-launch test hooks of the Qwen2.5-VL row's shared prompt prefix (include/vqs_qwen.h vqs_qwen_score_suffix), on caller tensors;
 * f16 = 1: IEEE fp16 tensors (the range-safe fp16 forms), 0: bf16.
 *   vqs_debug_qwen_attention: the prefill's causal GQA attention (attn_fwd_hd_kernel): q [B, H, S, 128], k / v [B, Hkv, S, 128], out [B*S, H*128]
 *   vqs_debug_qwen_attention_suffix: attn_suffix_hd_kernel, query rows [q0, S) only: q [B, H, Sq, 128] (row r = position q0 + r, Sq >= S - q0),
 *     k / v [B, Hkv, S, 128], out [B*Sq, H*128]; q0 a multiple of 32
 *   vqs_debug_qwen_kv_assemble: qwen_kv_assemble_kernel: dk / dv [B, Hkv, Lp + Ls, 128] from pk / pv [U, Hkv, Lp, 128] (medium media_idx[b];
 *     outside [0, U): zero rows) and sk / sv [B, Hkv, Ls, 128]
 *   vqs_debug_attention_hd: every form of attn_fwd_hd_kernel<128, CAUSAL, F16>: fills the launch's parameter block (head width 128) and calls
 *     launch_attention, nothing else.  causal = 0: the vision tower's form; out_hd (0 = 128, else a multiple of 4 up to 128): the lanes of a head
 *     that leave, out is then [B*S, H*out_hd] (the tower's 80-lane compact output); d_key_len may be NULL (every sample has S keys); Hkv = 0
 *     means H.  A shape the launcher refuses comes back as VQS_ERR_INVALID and nothing is launched. */
int vqs_debug_qwen_attention(const void* d_q, const void* d_k, const void* d_v, void* d_out, const int32_t* d_key_len, int32_t B, int32_t H, int32_t Hkv,
                             int32_t S, float scale, int32_t f16, void* stream);
int vqs_debug_qwen_attention_suffix(const void* d_q, const void* d_k, const void* d_v, void* d_out, const int32_t* d_key_len, int32_t B, int32_t H,
                                    int32_t Hkv, int32_t S, int32_t Sq, int32_t q0, float scale, int32_t f16, void* stream);
int vqs_debug_attention_hd(const void* d_q, const void* d_k, const void* d_v, void* d_out, const int32_t* d_key_len, int32_t B, int32_t H, int32_t Hkv,
                           int32_t S, float scale, int32_t causal, int32_t f16, int32_t out_hd, void* stream);
int vqs_debug_qwen_kv_assemble(const void* d_pk, const void* d_pv, const void* d_sk, const void* d_sv, const int32_t* d_media_idx, void* d_dk, void* d_dv,
                               int32_t B, int32_t U, int32_t Hkv, int32_t Lp, int32_t Ls, void* stream);
/* Single-launch test hooks of the Qwen2.5-VL decode-step kernels (csrc/qwen_decode.hip), on caller tensors; head width 128.
 *   vqs_debug_qwen_decode_attention: launch_qwen_decode_attn (mode 0) / launch_qwen_tail_attn (modes 1, 2) and nothing else.  kc / vc
 *     [B, Hkv, Lmax, 128].  mode 0, the decode step: q bf16 [B, Hq * 128], len[b] = the position just appended (keys [0, len[b]]), out bf16
 *     [B, Hq * 128].  mode 1, the precise tail: q fp32, len[b] = the COUNT of keys, out split-bf16 (hi plane at out, lo plane out_plane elements
 *     further).  mode 2: mode 1 over IEEE fp16 K / V (the key scale folded into `scale`, the output multiplied by vscale).  A length outside
 *     the cache is clamped by the kernels (mode 0: to [0, Lmax - 1]; modes 1, 2: to [1, Lmax]).
 *   vqs_debug_qwen_decode_rope_append: launch_qwen_decode_rope_append: qkv bf16 [B, (Hq + 2 Hkv) * hd], cos / sin fp32 [B, half], q_out
 *     [B, Hq * hd], kc / vc [B, Hkv, Lmax, hd]; a sample whose len[b] is outside [0, Lmax) writes nothing.
 *   vqs_debug_qwen_decode_attention_form: host-side, no device access: the kernel the launcher picks for this geometry, by the launcher's own
 *     function (vqs_kernels.h qwen_decode_attn_form): 1 = the grouped-query kernel, 0 = the per-query-head kernel, -1 = not launchable;
 *     *lds_bytes (may be NULL) = the launch's dynamic LDS bytes (0 when not launchable). */
int vqs_debug_qwen_decode_attention(const void* d_q, const void* d_kc, const void* d_vc, const int32_t* d_len, void* d_out, int64_t out_plane, int32_t B,
                                    int32_t Hq, int32_t Hkv, int32_t Lmax, float scale, float vscale, int32_t mode, void* stream);
/* vqs_debug_qwen_rows_attention: launch_qwen_rows_attn and nothing else -- the precise tail's attention over a row list (vqs_qwen_score_rows).
 * q fp32 [Q, Hq * 128], k / v [R, Hkv, L, 128] (bf16, or IEEE fp16 with kv_f16 != 0: key scale folded into `scale`, output multiplied by vscale),
 * row_sample / row_keys int32 [Q], out split-bf16 [Q, Hq * 128] with the lo plane out_plane (>= Q * Hq * 128) elements further.  Row r attends over
 * sample row_sample[r] (outside [0, R): a zero row) with min(max(row_keys[r], 1), L) keys; the kernel form is vqs_debug_qwen_decode_attention_form's. */
int vqs_debug_qwen_rows_attention(const void* d_q, const void* d_k, const void* d_v, const int32_t* d_row_sample, const int32_t* d_row_keys, void* d_out,
                                  int64_t out_plane, int32_t Q, int32_t R, int32_t Hq, int32_t Hkv, int32_t L, float scale, int32_t kv_f16, float vscale,
                                  void* stream);
int vqs_debug_qwen_decode_rope_append(const void* d_qkv, const float* d_cos, const float* d_sin, const int32_t* d_len, void* d_q_out, void* d_kc, void* d_vc,
                                      int32_t B, int32_t Hq, int32_t Hkv, int32_t hd, int32_t half, int32_t Lmax, void* stream);
int vqs_debug_qwen_decode_attention_form(int32_t Hq, int32_t Hkv, int32_t Lmax, int64_t* lds_bytes);
/* Single-launch test hooks of the precise decoder's glue, the split-K reductions and the greedy / score tail (csrc/elementwise.hip,
 * csrc/attn.hip), on caller tensors: each calls ONE launcher with the caller's arguments and nothing else (no copy, no synchronisation); a
 * launcher's refusal (a shape or an alignment it does not take) comes back as VQS_ERR_INVALID and nothing is launched.
 *   vqs_debug_rmsnorm_split: launch_rmsnorm_split: x fp32 [M, D] (+= delta fp32 [M, D] when not NULL, written back), w bf16 [D], out split-bf16:
 *     hi plane [M, D] at out, lo plane out_plane elements further.  D % 4 == 0, out_plane % 4 == 0.
 *   vqs_debug_sum_planes: launch_sum_planes: part fp32 [nslices][2 rows][ldp] (slice k at part + k slice_stride; hi rows, then lo rows),
 *     mode 0: out fp32 [rows, ld_out]; 1: split-bf16 planes [rows, ld_out] at out and out + out_plane; 2: cols = 2 F packed gate | linear
 *     columns (blocks of 64 = 32 | 32) -> split(act(gate) * linear), F columns; 3: IEEE fp16 [rows, ld_out].  bias (bf16 [cols], may be NULL)
 *     and silu != 0 select the Qwen2.5-VL tail's forms (bias added to the sums; the gate's activation is SiLU instead of gelu_new); mode 3
 *     has no such form.
 *   vqs_debug_reduce_slices: launch_reduce_slices: out bf16 [n] = sum over slices of part fp32 [nslices][n], in index order; n % 4 == 0.
 *   vqs_debug_reduce_slices_act: launch_reduce_slices_act: out bf16 [rows, ld_out] = f(sum over slices of part [nslices][rows][ldp] (+ bias));
 *     gated != 0: packed gate | up columns -> SiLU(gate) * up, cols / 2 columns.
 *   vqs_debug_masked_softmax: launch_masked_softmax: scores fp32 [B * rows, S_pad] -> probs [B * rows, S_pad] (bf16, or IEEE fp16 when
 *     out_f16 != 0), 0 for keys >= min(key_len[b], S_pad).
 *   vqs_debug_transpose_pad: launch_transpose_pad: in bf16 [B, S, D] -> out [B, D, S_pad], columns >= S zero.  D % 64 == 0, S_pad % 64 == 0.
 *   vqs_debug_argmax_append: launch_argmax_append: tokens[b, dst_col] (dst_col < 0: T - 1) = argmax of logits row b T + T - 1 over [0, V), the
 *     lowest index on ties; flags (may be NULL): bit 1 is set when a scanned logit is not finite.
 *   vqs_debug_decoder_attention: launch_decoder_attention with every field of its parameter block: vqs_decoder_attention plus the cached
 *     self form (qpos0 = decoder position of query row 0, S = qpos0 + T keys, kv_stride_b elements between the samples' K / V rows, bias_ld =
 *     row length of the bias table; 0 = the teacher-forced defaults) and the precise self form (precise != 0: q / k / v fp32 [B T, ldq], the
 *     output split-bf16 with the lo plane out_plane elements after the hi plane).  Cross form: keys at positions >= key_len[b] are masked
 *     whatever they hold; value rows there are multiplied by a probability of exactly 0 and must be finite (vqs_decoder_attention, vqs.h).
 *   vqs_debug_score_head: launch_score_head (vqs_score_head of vqs.h) with the pass's status word: flags (may be NULL) bit 1 is set when a
 *     sample's summed label log-probs are not finite. */
int vqs_debug_rmsnorm_split(float* d_x, const float* d_delta, const void* d_w, void* d_out, int64_t out_plane, int32_t M, int32_t D, float eps,
                            void* stream);
int vqs_debug_sum_planes(const float* d_part, int32_t nslices, int64_t slice_stride, int32_t rows, int32_t cols, int32_t ldp, int32_t mode, void* d_out,
                         int32_t ld_out, int64_t out_plane, const void* d_bias, int32_t silu, void* stream);
int vqs_debug_reduce_slices(const float* d_part, int32_t nslices, int64_t n, void* d_out, void* stream);
int vqs_debug_reduce_slices_act(const float* d_part, int32_t nslices, int64_t slice_stride, int32_t rows, int32_t cols, int32_t ldp, const void* d_bias,
                                int32_t gated, void* d_out, int32_t ld_out, void* stream);
int vqs_debug_masked_softmax(const float* d_scores, void* d_probs, const int32_t* d_key_len, int32_t B, int32_t rows, int32_t S_pad, int32_t out_f16,
                             void* stream);
int vqs_debug_transpose_pad(const void* d_in, void* d_out, int32_t B, int32_t S, int32_t D, int32_t S_pad, void* stream);
int vqs_debug_argmax_append(const float* d_logits, int32_t ldl, int32_t V, int32_t* d_tokens, int32_t ld_tokens, int32_t B, int32_t T, int32_t dst_col,
                            int32_t* d_flags, void* stream);
int vqs_debug_decoder_attention(const void* d_q, const void* d_k, const void* d_v, void* d_out, const float* d_bias_table, const int32_t* d_key_len,
                                int32_t B, int32_t H, int32_t T, int32_t S, int32_t ldq, int32_t ldk, int32_t cross, int64_t kv_stride_b, int32_t qpos0,
                                int32_t bias_ld, int32_t precise, int64_t out_plane, void* stream);
int vqs_debug_score_head(const float* d_logits, int32_t ldl, int32_t V, const int32_t* d_labels, float* d_lp, float* d_scores, int32_t B, int32_t T,
                         int32_t* d_flags, void* stream);
/* Single-launch test hooks of the Qwen2.5-VL prefill's glue and of the bind-time range proof (csrc/elementwise.hip, csrc/qwen_decode.hip), on caller
 * tensors (tests/test_gpu_qwen_glue_kernels.py, profiles/qwen_glue_kernels.md): each calls ONE launcher with the caller's arguments and nothing else (no
 * copy, no synchronisation); a launcher's refusal comes back as VQS_ERR_INVALID and nothing is launched, and so does a NULL required pointer or a
 * non-positive size.  No kernel of this family defines an out-of-range index map: every map entry must name a row / column that exists.
 *   vqs_debug_rmsnorm_f16s: launch_rmsnorm_f16s: x fp32 [M, D] += fp16 delta * d1 (+ fp16 delta2 * d2), written back unless store_x == 0 (one delta only);
 *     out [M, out_ld] (out_ld = 0: D; >= D, a multiple of 4) = w * x * rsqrt(mean x^2 + eps) * osc as IEEE fp16, or bf16 with out_bf16 != 0 (the final
 *     norm; store_x == 0 has no such form).  w bf16 [D]; D % 4 == 0.
 *   vqs_debug_rope_qk: launch_rope_qk: q [B, Hq, S, hd] and k [B, Hk, S, hd] rotated in place in one launch (rotate-half, lanes [0, 2 half); the others
 *     keep their bits); cos / sin fp32 [B S, half]; f16 != 0: IEEE fp16 tensors (half % 8 == 0, hd % 8 == 0, half <= 64 only), else bf16, where any
 *     other even half takes two launches of vqs_rope's kernel.
 *   vqs_debug_qwen_embed: launch_qwen_embed: out fp32 [rows, D] = merged row vis_slot[r] where that is >= 0 (bf16, or IEEE fp16 times unscale with
 *     merged_f16 != 0), else embed row min(max(ids[r], 0), vocab - 1) (bf16 [vocab, D]).
 *   vqs_debug_gather_rows_bf16: launch_gather_rows_bf16: dst [rows, dst_ld] = row map[r] of src0 (map[r] >= 0), row -map[r] - 2 of src1 (map[r] <= -2; src1
 *     required then) or zeros (-1), columns [cols, dst_ld) zero; source rows src_ld apart; map NULL: identity.  The hook refuses rows <= 0, cols <= 0,
 *     src_ld < cols and dst_ld < cols on the host (the launcher checks nothing).
 *   vqs_debug_gather_cols_bf16: launch_gather_cols_bf16: dst [rows, dst_cols] = src [rows, src_ld] column cmap[c], 0 where cmap[c] < 0.
 *   vqs_debug_gather_rows_f32: form 0: elementwise.hip's launcher (window permutation: dst [rows, cols] = src row map[r], a zero row for -1; dense rows,
 *     src_ld must be 0 or cols), form 1: qwen_decode.hip's (the tail's embedding rows: source rows src_ld >= cols apart, no zero rows).  cols % 4 == 0.
 *   vqs_debug_f16_to_bf16_rows: launch_f16_to_bf16_rows: dst[r][0 : cols) = bf16(fp16 src[r][0 : cols) * unscale), rows src_ld / dst_ld elements apart;
 *     cols % 8 == 0, rows <= 65535.
 *   vqs_debug_qwen_tail_rope_q: launch_qwen_tail_rope_q: q_out fp32 [B, Hq hd] = the first Hq hd columns of qkv fp32 [B, ld], each head rotated by table
 *     row row[b] of cos / sin fp32 [*, half]; lanes [2 half, hd) copied.  half <= 64; the hook also refuses ld < Hq hd.
 *   vqs_debug_rowbound: launch_rowbound: mode 0: out[j] = R sqrt(sum_k (W[j, k] g[k % g_len])^2) + |bias[j]|; mode 1: out[j] = sum_k |W[j, k]| u[k] + |bias[j]|
 *     (u NULL: the constant *uconst).  W bf16 [N, ldw >= K], g / bias bf16, u fp32 [K]; bias and out may be NULL; *slot = max(*slot, max_j out[j]) on
 *     the bit pattern, 0x7fc00000 once a row's bound is NaN.
 *   vqs_debug_absmax_bf16: launch_absmax_bf16: *slot = max(*slot, R max |x[i]|) over n bf16 elements, NaN as above.
 *   vqs_debug_gate_pair_bound: launch_gate_pair_bound: u_act[j] = rb[gate(j)] rb[up(j)] over the packed 32 | 32 blocks for j < mlp_p, 0 for [mlp_p, ld);
 *     *slot as above.  mlp_p % 32 == 0, ld >= mlp_p. */
int vqs_debug_rmsnorm_f16s(float* d_x, const void* d_delta, const void* d_delta2, int32_t store_x, const void* d_w, void* d_out, int32_t out_ld, int32_t M,
                           int32_t D, float eps, float d1, float d2, float osc, int32_t out_bf16, void* stream);
int vqs_debug_rope_qk(void* d_q, void* d_k, const float* d_cos, const float* d_sin, int32_t B, int32_t Hq, int32_t Hk, int32_t S, int32_t hd, int32_t half,
                      int32_t f16, void* stream);
int vqs_debug_qwen_embed(const int32_t* d_ids, const int32_t* d_vis_slot, const void* d_embed, const void* d_merged, float* d_out, int32_t rows, int32_t D,
                         int32_t vocab, int32_t merged_f16, float unscale, void* stream);
int vqs_debug_gather_rows_bf16(const void* d_src0, const void* d_src1, const int32_t* d_map, void* d_dst, int32_t rows, int32_t cols, int32_t src_ld,
                               int32_t dst_ld, void* stream);
int vqs_debug_gather_cols_bf16(const void* d_src, const int32_t* d_cmap, void* d_dst, int32_t rows, int32_t src_ld, int32_t dst_cols, void* stream);
int vqs_debug_gather_rows_f32(const float* d_src, const int32_t* d_map, float* d_dst, int32_t rows, int32_t cols, int32_t src_ld, int32_t form, void* stream);
int vqs_debug_f16_to_bf16_rows(const void* d_src, void* d_dst, int32_t rows, int64_t cols, int64_t src_ld, int64_t dst_ld, float unscale, void* stream);
int vqs_debug_qwen_tail_rope_q(const float* d_qkv, int32_t ld, const float* d_cos, const float* d_sin, const int32_t* d_row, float* d_q_out, int32_t B,
                               int32_t Hq, int32_t hd, int32_t half, void* stream);
int vqs_debug_rowbound(const void* d_w, int64_t ldw, int32_t N, int32_t K, int32_t mode, const void* d_g, int32_t g_len, float R, const float* d_u,
                       const float* d_uconst, const void* d_bias, float* d_out, float* d_slot, void* stream);
int vqs_debug_absmax_bf16(const void* d_x, int64_t n, float R, float* d_slot, void* stream);
int vqs_debug_gate_pair_bound(const float* d_rb, int32_t mlp_p, int32_t ld, float* d_u_act, float* d_slot, void* stream);
/* Tap window: taps copy only the rows of `count` consecutive outer entries starting at `first` -- pairs for the T5 stacks
 * (rows [first*S, (first+count)*S) of an [B*S, W] tensor, the same fraction of a head-major [B, H, S, 64] or a [B*T, W] one),
 * images for the vision tower (so the window's pairs must reference images first .. first+count-1 in order, as the bench
 * batch does).  Every intermediate is laid out outer-entry-major, so the window is ONE contiguous byte range of each
 * tensor and the tap buffers shrink by B / count: this is how a stage-locked check runs on the BENCHMARKED configuration
 * (XXL, 256 pairs: full taps would need ~290 GB) for a few sampled pairs.  count == 0 restores whole-tensor taps. */
int vqs_debug_tap_window(vqs_handle* h, int32_t first, int32_t count);

/* Lab switches of vqs_set_option (cache-policy hints, bitwise-neutral; the library's rule by shape is the product setting):
 *   "tile_order:<N>x<K>"  value = gm | ns << 8: tile order (see vqs_gemm) of every GEMM of a pass whose weight is [N, K];
 *                  0 removes the entry (back to the library's choice for that shape).  Bitwise-neutral.
 *   "l2_touch:<N>x<K>"    1: the lock-step GEMM prefetches the A panel two K-tiles ahead into L2 for the big launches whose weight is
 *                  [N, K], 2: it does not, 0: the library's rule by shape.  A hint: bitwise-neutral.
 *   "nt_store:<N>x<K>"    1: the results of every GEMM of a pass whose weight is [N, K] are stored with the non-temporal hint,
 *                  2: plain stores, 0: the library's choice for the call site.  A cache-policy hint: bitwise-neutral.
 */

#ifdef __cplusplus
}
#endif
#endif /* VQS_DEBUG_H */
