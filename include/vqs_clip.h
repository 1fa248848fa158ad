/* libvqs_hip -- CLIPScore row: OpenAI CLIP ViT-L/14 (336 px / 224 px) image and text towers, projection heads and the
 * cosine grid on gfx950.  C ABI, exported from libvqs_hip.so next to include/vqs.h; same conventions (device pointers
 * named d_*, raw bf16 bits, `stream` = hipStream_t as void*, no allocation, no stream synchronisation, 0 = success,
 * negative = VQS_ERR_* of include/vqs.h, no CPU fallback).
 *
 * What it stands in for: HF `CLIPModel.get_image_features` / `get_text_features` (models/clip/modeling_clip.py) followed
 * by the L2 normalisation and the dot product the v3.0 CLIPScore model takes (the plain cosine; `logit_scale` is not applied).
 * The vision tower is the launch sequence of vqs_encode_images (include/vqs.h) run through ALL of its layers; the text tower
 * runs the same GEMM / LayerNorm launches at its own width behind a causal attention kernel of its own (csrc/clip.hip).
 */
#ifndef VQS_CLIP_H
#define VQS_CLIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vqs_clip_handle vqs_clip_handle;

/* HF CLIPConfig (models/clip/configuration_clip.py): vision_config, text_config, projection_dim. */
typedef struct vqs_clip_config {
    int32_t vis_hidden;   /* 1024 */
    int32_t vis_layers;   /* 24: every layer is run (the pooled output reads the last one) */
    int32_t vis_heads;    /* 16 (head dim must be 64) */
    int32_t vis_mlp;      /* 4096 */
    int32_t vis_patch;    /* 14 */
    int32_t vis_image;    /* 336 / 224 */
    float vis_eps;        /* 1e-5 */
    int32_t txt_hidden;   /* 768 */
    int32_t txt_layers;   /* 12 */
    int32_t txt_heads;    /* 12 (head dim must be 64) */
    int32_t txt_mlp;      /* 3072 */
    int32_t txt_vocab;    /* 49408 */
    int32_t txt_context;  /* 77 (<= 128) */
    float txt_eps;        /* 1e-5 */
    int32_t embed_dim;    /* 768 (projection_dim) */
} vqs_clip_config;

/* One named bf16 device tensor (same layout as vqs_weight_desc of include/vqs.h).  Names are the HF CLIPModel state_dict
 * keys: vision_model.*, text_model.*, visual_projection.weight, text_projection.weight (logit_scale is not read). */
typedef struct vqs_clip_weight_desc {
    const char* name;
    const void* d_data;
    int64_t numel;
} vqs_clip_weight_desc;

int vqs_clip_create(const vqs_clip_config* cfg, vqs_clip_handle** out);
void vqs_clip_destroy(vqs_clip_handle* h);
const char* vqs_clip_last_error(const vqs_clip_handle* h);

/* The caller keeps every bound tensor alive; fused q|k|v weights / biases, the zero-padded patch kernel and the fp16 copies
 * of both towers' linear weights are written into d_packed (vqs_clip_packed_bytes() bytes, caller-owned). */
size_t vqs_clip_packed_bytes(const vqs_clip_handle* h);
int vqs_clip_bind_weights(vqs_clip_handle* h, const vqs_clip_weight_desc* weights, int32_t n_weights, void* d_packed,
                          size_t packed_bytes, void* stream);

/* CLIPModel.get_image_features + L2 normalisation.
 *   d_pixels  bf16 [n, 3, image, image]  (CLIP-normalised)
 *   d_embed   fp32 [n, embed_dim]  (output) unit vectors */
size_t vqs_clip_image_workspace_bytes(const vqs_clip_handle* h, int32_t n);
int vqs_clip_encode_images(vqs_clip_handle* h, const void* d_pixels, int32_t n, float* d_embed, void* d_ws, size_t ws_bytes,
                           void* stream);

/* CLIPModel.get_text_features + L2 normalisation.
 *   d_ids      int32 [n, L]   token ids, 8 <= L <= txt_context; rows are right-padded with any valid id
 *   d_eot_pos  int32 [n]      position of each row's EOT token (the pooled row); computed on the host
 *   d_embed    fp32  [n, embed_dim]  (output) unit vectors
 * No padding mask (CLIP's text tower has none): the causal mask keeps the pooled row from seeing anything behind it. */
size_t vqs_clip_text_workspace_bytes(const vqs_clip_handle* h, int32_t n, int32_t L);
int vqs_clip_encode_texts(vqs_clip_handle* h, const int32_t* d_ids, const int32_t* d_eot_pos, int32_t n, int32_t L,
                          float* d_embed, void* d_ws, size_t ws_bytes, void* stream);

/* d_out fp32 [M, N] = d_img [M, E] . d_txt [N, E]^T in fp32 FMA (one ascending chain per element). */
int vqs_clip_similarity(const float* d_img, const float* d_txt, int32_t M, int32_t N, int32_t E, float* d_out, void* stream);
/* d_out[k] = <d_img[d_idx_i[k]], d_txt[d_idx_t[k]]>, the same chain: bitwise the grid's element.  Indices outside
 * [0, M) x [0, N) yield NaN. */
int vqs_clip_similarity_pairs(const float* d_img, const float* d_txt, const int32_t* d_idx_i, const int32_t* d_idx_t, int32_t M,
                              int32_t N, int32_t K, int32_t E, float* d_out, void* stream);

/* "fp16": 1 (default) both towers hold their 16-bit tensors in IEEE fp16 (fp16 copies of the linear weights made at bind time,
 *         fp32 accumulation / residual stream / statistics) as option vit_fp16 of include/vqs.h does; 0 = bf16 operands.
 *         The library does not look at weights: the Python binding checks their range at bind time.
 * "norm_defer": 1 (default) deferred store of the fp32 stream in the norm kernels (bitwise equal), 0 = store in every norm. */
int vqs_clip_set_option(vqs_clip_handle* h, const char* name, int32_t value);
int vqs_clip_get_option(const vqs_clip_handle* h, const char* name, int32_t* value);

/* ---- single-kernel entry points (parity tests call the new kernels through these) ---- */
/* Causal attention of the text tower, head dim 64: q / k / v [B, H, S, 64] head-major (bf16, or IEEE fp16 with f16 = 1),
 * out [B*S, H*64] token-major, 1 <= S <= 128; mask = key <= query only; fp32 scores and softmax. */
int vqs_clip_causal_attention(const void* d_q, const void* d_k, const void* d_v, void* d_out, int32_t B, int32_t H, int32_t S,
                              float scale, int32_t f16, void* stream);
/* d_out fp32 [n, L, D] = token_embedding[ids] + position_embedding[0..L) (both bf16).  An id outside [0, vocab) yields NaN rows. */
int vqs_clip_embed(const int32_t* d_ids, const void* d_tok, const void* d_pos, float* d_out, int32_t n, int32_t L, int32_t D,
                   int32_t vocab, void* stream);
/* Pool + head: per sample b the row d_rows[b] (NULL: row 0) of the fp32 stream d_x [n, S, D], plus the pending 16-bit
 * sub-layer output d_delta (same shape; NULL = none; delta_f16: it is IEEE fp16, else bf16), LayerNorm (w, b bf16; fp32
 * statistics), projection by d_proj bf16 [E, D] without bias in fp32, L2 normalisation -> d_out fp32 [n, E].
 * D <= 4096, D % 8 == 0. */
int vqs_clip_pool_head(const float* d_x, const void* d_delta, int32_t delta_f16, const int32_t* d_rows, const void* d_ln_w,
                       const void* d_ln_b, const void* d_proj, float* d_out, int32_t n, int32_t S, int32_t D, int32_t E, float eps,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VQS_CLIP_H */
