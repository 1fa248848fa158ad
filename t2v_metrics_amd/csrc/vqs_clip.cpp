// Host side of the CLIPScore row: the C ABI of include/vqs_clip.h.  The launch sequences restate what HF executes for
// CLIPModel.get_image_features / get_text_features (models/clip/modeling_clip.py):
//   CLIPVisionTransformer: embeddings -> pre_layrnorm -> encoder (all layers) -> post_layernorm(CLS) -> visual_projection
//   CLIPTextTransformer:   embeddings -> encoder (causal mask) -> final_layer_norm -> row of the EOT token -> text_projection
// followed by x / ||x||.  The towers' blocks are the loop vqs_encode_images runs (vqs_blocks.h).  No device allocation, no
// stream synchronisation, no CPU fallback.
#include "../../include/vqs.h"
#include "../../include/vqs_clip.h"
#include "vqs_blocks.h"

#include <hip/hip_runtime.h>

#include <string>
#include <unordered_map>
#include <vector>

using vqs::bf16_t;
using vqs::GemmCall;
using vqs::Carver;
using vqs::ClipTower;
using vqs::fail;

namespace vqs {
hipError_t launch_clip_causal_attention(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, int B, int H, int S, float scale,
                                        bool f16, hipStream_t s);
hipError_t launch_clip_embed(const int* ids, const bf16_t* tok, const bf16_t* pos, float* out, int n, int L, int D, int vocab, hipStream_t s);
hipError_t launch_clip_pool_head(const float* x, const bf16_t* delta, bool delta_f16, const int* rows, const bf16_t* lnw, const bf16_t* lnb,
                                 const bf16_t* proj, float* out, int n, int S, int D, int E, float eps, hipStream_t s);
hipError_t launch_clip_similarity(const float* img, const float* txt, int M, int N, int E, float* out, hipStream_t s);
hipError_t launch_clip_similarity_pairs(const float* img, const float* txt, const int* ii, const int* tt, int M, int N, int K, int E, float* out,
                                        hipStream_t s);
}  // namespace vqs

struct vqs_clip_handle : vqs::HostBase {
    vqs_clip_config c;
    int fp16 = 1;
    int norm_defer = 1;
    int P = 0, Sv = 0, kpatch = 0, kpad = 0;
    const bf16_t* patch_w = nullptr;
    ClipTower vis, txt;
};

namespace {

struct TowerWs {
    bf16_t* im2col = nullptr;      // vision only
    float* patch_out = nullptr;
    float* pre = nullptr;
    vqs::ClipBlockBufs b;
    size_t total;
};

TowerWs carve_tower(const vqs_clip_handle* h, char* base, bool vision, int n, int S) {
    const vqs_clip_config& c = h->c;
    Carver cv{base};
    TowerWs w;
    const int hid = vision ? c.vis_hidden : c.txt_hidden, mlp = vision ? c.vis_mlp : c.txt_mlp;
    const size_t NS = (size_t)n * S;
    if (vision) {
        const size_t NP = (size_t)n * h->P;
        w.im2col = cv.take<bf16_t>(NP * h->kpad);
        w.patch_out = cv.take<float>(NP * hid);
        w.pre = cv.take<float>(NS * hid);
    }
    w.b.hidden = cv.take<float>(NS * hid);
    w.b.delta = cv.take<bf16_t>(NS * hid);
    w.b.delta2 = cv.take<bf16_t>(NS * hid);
    w.b.xn = cv.take<bf16_t>(NS * hid);
    w.b.q = cv.take<bf16_t>(NS * hid);
    w.b.k = cv.take<bf16_t>(NS * hid);
    w.b.v = cv.take<bf16_t>(NS * hid);
    w.b.attn = cv.take<bf16_t>(NS * hid);
    w.b.mid = cv.take<bf16_t>(NS * mlp);
    w.total = cv.total();
    return w;
}

struct ClipPacked {
    size_t patch_w;
    struct T { std::vector<size_t> qkv_w, qkv_b, qkv_w16, out_w16, fc1_w16, fc2_w16; } vis, txt;
    size_t total;
};

ClipPacked clip_packed_layout(const vqs_clip_handle* h) {
    const vqs_clip_config& c = h->c;
    ClipPacked pl;
    Carver cv{nullptr};
    auto take = [&](size_t elems) { return cv.mark(elems * sizeof(bf16_t)); };
    pl.patch_w = take((size_t)c.vis_hidden * h->kpad);
    auto tower = [&](ClipPacked::T& t, int layers, size_t hid, size_t mlp) {
        for (int i = 0; i < layers; ++i) {
            t.qkv_w.push_back(take(3 * hid * hid));
            t.qkv_b.push_back(take(3 * hid));
            t.qkv_w16.push_back(take(3 * hid * hid));
            t.out_w16.push_back(take(hid * hid));
            t.fc1_w16.push_back(take(mlp * hid));
            t.fc2_w16.push_back(take(mlp * hid));
        }
    };
    tower(pl.vis, c.vis_layers, c.vis_hidden, c.vis_mlp);
    tower(pl.txt, c.txt_layers, c.txt_hidden, c.txt_mlp);
    pl.total = cv.total();
    return pl;
}

// The CLIPScore handle's side of the shared block loop: HF CLIPModel names under `prefix`, no taps, no profiling.
struct ClipBlocksCtx {
    vqs_clip_handle* h;
    hipStream_t st;
    const ClipTower* t;
    std::string prefix;      // "vision_model." / "text_model."
    int hid, mlp;
    bool causal;             // the text tower's mask
    int weights(int i, vqs::ClipBlockWeights& lw) { return vqs::clip_block_weights(h, prefix, i, hid, mlp, h->fp16 != 0, *t, lw); }
    vqs::GemmOpts gemm_opts(const GemmCall&) const { return {}; }
    hipError_t attention(const vqs::ClipBlockShape& s, const vqs::ClipBlockBufs& w) {
        if (causal) return vqs::launch_clip_causal_attention(w.q, w.k, w.v, w.attn, s.n, s.heads, s.S, 0.125f, s.f16, st);
        vqs::AttnParams a{w.q, w.k, w.v, w.attn, nullptr, nullptr, s.n, s.heads, s.S, 0.125f};
        a.f16 = s.f16;
        return vqs::launch_attention(a, st);
    }
    int tap(int, const char*, const void*, size_t) { return VQS_OK; }
};

int pack_tower(vqs_clip_handle* h, const std::string& prefix, int layers, int hid, int mlp, const ClipPacked::T& pl, ClipTower& t, char* pk,
               hipStream_t st) {
    auto at = [&](size_t off) { return reinterpret_cast<bf16_t*>(pk + off); };
    t = ClipTower();
    for (int i = 0; i < layers; ++i) {
        const std::string p = prefix + "encoder.layers." + std::to_string(i) + ".";
        const char* nm[3] = {"q_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 3; ++j) {
            VQS_W(ww, p + "self_attn." + nm[j] + ".weight", (int64_t)hid * hid);
            VQS_W(bb, p + "self_attn." + nm[j] + ".bias", hid);
            VQS_HIP(h, vqs::launch_copy_rows(ww, at(pl.qkv_w[i]), hid, hid, hid, hid, j * hid, st), "pack qkv");
            VQS_HIP(h, vqs::launch_copy_rows(bb, at(pl.qkv_b[i]), 1, hid, hid, hid, j, st), "pack qkv bias");
        }
        VQS_W(ow, p + "self_attn.out_proj.weight", (int64_t)hid * hid);
        VQS_W(f1w, p + "mlp.fc1.weight", (int64_t)mlp * hid);
        VQS_W(f2w, p + "mlp.fc2.weight", (int64_t)hid * mlp);
        // fp16 copies (option fp16): bf16 -> fp16 is exact for 2^-14 <= |w| < 65 520
        VQS_HIP(h, vqs::launch_cast16(at(pl.qkv_w[i]), at(pl.qkv_w16[i]), (size_t)3 * hid * hid, true, st), "fp16 qkv");
        VQS_HIP(h, vqs::launch_cast16(ow, at(pl.out_w16[i]), (size_t)hid * hid, true, st), "fp16 out_proj");
        VQS_HIP(h, vqs::launch_cast16(f1w, at(pl.fc1_w16[i]), (size_t)mlp * hid, true, st), "fp16 fc1");
        VQS_HIP(h, vqs::launch_cast16(f2w, at(pl.fc2_w16[i]), (size_t)mlp * hid, true, st), "fp16 fc2");
        t.qkv_w.push_back(at(pl.qkv_w[i]));
        t.qkv_b.push_back(at(pl.qkv_b[i]));
        t.qkv_w16.push_back(at(pl.qkv_w16[i]));
        t.out_w16.push_back(at(pl.out_w16[i]));
        t.fc1_w16.push_back(at(pl.fc1_w16[i]));
        t.fc2_w16.push_back(at(pl.fc2_w16[i]));
    }
    return VQS_OK;
}

}  // namespace

extern "C" {

int vqs_clip_create(const vqs_clip_config* cfg, vqs_clip_handle** out) {
    if (!cfg || !out) return VQS_ERR_INVALID;
    vqs_clip_handle* h = new vqs_clip_handle();
    h->c = *cfg;
    const vqs_clip_config& c = h->c;
    *out = h;
    auto bad = [&](const char* m) { return fail(h, VQS_ERR_INVALID, m); };
    if (c.vis_layers < 1 || c.txt_layers < 1) return bad("layer counts must be positive");
    if (c.vis_hidden <= 0 || c.vis_heads <= 0 || c.vis_hidden != c.vis_heads * 64) return bad("vision head dim must be 64");
    if (c.txt_hidden <= 0 || c.txt_heads <= 0 || c.txt_hidden != c.txt_heads * 64) return bad("text head dim must be 64");
    // the q|k|v GEMM's head-major epilogue hands a wave 128 columns of ONE of q / k / v; every linear contracts over >= 128
    if (c.vis_hidden % 128 || c.txt_hidden % 128) return bad("hidden sizes must be multiples of 128");
    if (c.vis_mlp < 128 || c.txt_mlp < 128 || c.vis_mlp % 64 || c.txt_mlp % 64) return bad("mlp sizes must be multiples of 64, at least 128");
    if (c.vis_hidden > 4096 || c.txt_hidden > 4096) return bad("hidden sizes above 4096 are not supported");
    if (c.vis_patch <= 0 || c.vis_image <= 0 || c.vis_image % c.vis_patch) return bad("image size must be a multiple of the patch size");
    if (c.txt_context < 8 || c.txt_context > 128) return bad("txt_context must be in [8, 128]");
    if (c.txt_vocab <= 0) return bad("txt_vocab must be positive");
    if (c.embed_dim <= 0 || c.embed_dim > 4096 || c.embed_dim % 4) return bad("embed_dim must be a multiple of 4, at most 4096");
    const int g = c.vis_image / c.vis_patch;
    if (g * g + 1 < 8) return bad("the image needs at least 7 patches");
    h->P = g * g;          // P > 0 marks an accepted configuration
    h->Sv = h->P + 1;
    h->kpatch = 3 * c.vis_patch * c.vis_patch;
    h->kpad = (h->kpatch + 63) / 64 * 64;
    return VQS_OK;
}

void vqs_clip_destroy(vqs_clip_handle* h) { delete h; }

const char* vqs_clip_last_error(const vqs_clip_handle* h) { return h ? h->err.c_str() : "null handle"; }

int vqs_clip_set_option(vqs_clip_handle* h, const char* name, int32_t value) {
    if (!h || !name) return VQS_ERR_INVALID;
    const std::string n(name);
    if (n == "fp16" && (value == 0 || value == 1)) h->fp16 = value;
    else if (n == "norm_defer" && (value == 0 || value == 1)) h->norm_defer = value;
    else return fail(h, VQS_ERR_INVALID, "set_option: unknown option or value: " + n + "=" + std::to_string(value));
    return VQS_OK;
}

int vqs_clip_get_option(const vqs_clip_handle* h, const char* name, int32_t* value) {
    if (!h || !name || !value) return VQS_ERR_INVALID;
    const std::string n(name);
    if (n == "fp16") *value = h->fp16;
    else if (n == "norm_defer") *value = h->norm_defer;
    else return VQS_ERR_INVALID;
    return VQS_OK;
}

size_t vqs_clip_packed_bytes(const vqs_clip_handle* h) { return (h && h->P > 0) ? clip_packed_layout(h).total : 0; }

int vqs_clip_bind_weights(vqs_clip_handle* h, const vqs_clip_weight_desc* weights, int32_t n, void* d_packed, size_t packed_bytes,
                          void* stream) {
    if (!h) return VQS_ERR_INVALID;
    if (h->P <= 0) return fail(h, VQS_ERR_STATE, "bind_weights: the handle's configuration was refused");
    if (!weights || n <= 0 || !d_packed) return fail(h, VQS_ERR_INVALID, "bind_weights: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const vqs_clip_config& c = h->c;
    const ClipPacked pl = clip_packed_layout(h);
    if (packed_bytes < pl.total) return fail(h, VQS_ERR_WORKSPACE, "bind_weights: packed buffer too small");
    h->bound = false;
    VQS_RUN(vqs::set_weights(h, weights, n));
    char* pk = (char*)d_packed;
    {   // conv kernel [hid, 3*p*p] -> [hid, kpad] zero padded (K must be a multiple of 64)
        VQS_W(pw, "vision_model.embeddings.patch_embedding.weight", (int64_t)c.vis_hidden * h->kpatch);
        bf16_t* dst = reinterpret_cast<bf16_t*>(pk + pl.patch_w);
        VQS_HIP(h, vqs::launch_copy_rows(pw, dst, c.vis_hidden, h->kpatch, h->kpatch, h->kpad, 0, st), "pack patch");
        h->patch_w = dst;
    }
    VQS_RUN(pack_tower(h, "vision_model.", c.vis_layers, c.vis_hidden, c.vis_mlp, pl.vis, h->vis, pk, st));
    VQS_RUN(pack_tower(h, "text_model.", c.txt_layers, c.txt_hidden, c.txt_mlp, pl.txt, h->txt, pk, st));
    {   // everything the passes look up by name later must be there now
        const int vh = c.vis_hidden, th = c.txt_hidden;
        VQS_W(a0, "vision_model.embeddings.class_embedding", vh);
        VQS_W(a1, "vision_model.embeddings.position_embedding.weight", (int64_t)h->Sv * vh);
        VQS_W(a2, "vision_model.pre_layrnorm.weight", vh);
        VQS_W(a3, "vision_model.pre_layrnorm.bias", vh);
        VQS_W(a4, "vision_model.post_layernorm.weight", vh);
        VQS_W(a5, "vision_model.post_layernorm.bias", vh);
        VQS_W(a6, "visual_projection.weight", (int64_t)c.embed_dim * vh);
        VQS_W(b0, "text_model.embeddings.token_embedding.weight", (int64_t)c.txt_vocab * th);
        VQS_W(b1, "text_model.embeddings.position_embedding.weight", (int64_t)c.txt_context * th);
        VQS_W(b2, "text_model.final_layer_norm.weight", th);
        VQS_W(b3, "text_model.final_layer_norm.bias", th);
        VQS_W(b4, "text_projection.weight", (int64_t)c.embed_dim * th);
        (void)a0; (void)a1; (void)a2; (void)a3; (void)a4; (void)a5; (void)a6; (void)b0; (void)b1; (void)b2; (void)b3; (void)b4;
        vqs::ClipBlockWeights lw;
        for (int i = 0; i < c.vis_layers; ++i) {
            ClipBlocksCtx cx{h, st, &h->vis, "vision_model.", c.vis_hidden, c.vis_mlp, false};
            VQS_RUN(cx.weights(i, lw));
        }
        for (int i = 0; i < c.txt_layers; ++i) {
            ClipBlocksCtx cx{h, st, &h->txt, "text_model.", c.txt_hidden, c.txt_mlp, true};
            VQS_RUN(cx.weights(i, lw));
        }
    }
    h->bound = true;
    return VQS_OK;
}

size_t vqs_clip_image_workspace_bytes(const vqs_clip_handle* h, int32_t n) {
    if (!h || h->P <= 0 || n <= 0) return 0;
    return carve_tower(h, nullptr, true, n, h->Sv).total;
}

int vqs_clip_encode_images(vqs_clip_handle* h, const void* d_pixels, int32_t N, float* d_embed, void* d_ws, size_t ws_bytes, void* stream) {
    if (!h) return VQS_ERR_INVALID;
    if (!h->bound) return fail(h, VQS_ERR_STATE, "encode_images: weights not bound");
    if (!d_pixels || !d_embed || !d_ws || N <= 0) return fail(h, VQS_ERR_INVALID, "encode_images: bad arguments");
    const vqs_clip_config& c = h->c;
    const TowerWs w = carve_tower(h, (char*)d_ws, true, N, h->Sv);
    if (ws_bytes < w.total) return fail(h, VQS_ERR_WORKSPACE, "encode_images: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int hid = c.vis_hidden, P = h->P, Sv = h->Sv;
    const int NP = N * P, NS = N * Sv;
    const bool f16 = h->fp16 != 0;

    VQS_W(cls, "vision_model.embeddings.class_embedding", hid);
    VQS_W(pos, "vision_model.embeddings.position_embedding.weight", (int64_t)Sv * hid);
    VQS_W(pre_w, "vision_model.pre_layrnorm.weight", hid);
    VQS_W(pre_b, "vision_model.pre_layrnorm.bias", hid);
    VQS_W(post_w, "vision_model.post_layernorm.weight", hid);
    VQS_W(post_b, "vision_model.post_layernorm.bias", hid);
    VQS_W(proj, "visual_projection.weight", (int64_t)c.embed_dim * hid);

    // embeddings: the launches of vqs_encode_images (the patch embedding keeps its bf16 operands, fp32 result)
    VQS_HIP(h, vqs::launch_im2col((const bf16_t*)d_pixels, w.im2col, N, c.vis_image, c.vis_patch, h->kpad, st), "im2col");
    {
        GemmCall g{w.im2col, h->patch_w, w.patch_out};
        g.M = NP; g.N = hid; g.K = h->kpad; g.lda = h->kpad; g.ldw = h->kpad; g.ldc = hid; g.epi = vqs::EPI_F32;
        VQS_RUN(vqs::run_gemm(h, g, {}, st, "patch_embed"));
    }
    VQS_HIP(h, vqs::launch_vit_assemble(w.patch_out, cls, pos, w.pre, N, P, hid, st), "vit_assemble");
    VQS_HIP(h, vqs::launch_layernorm(w.pre, nullptr, pre_w, pre_b, w.b.hidden, 1, NS, hid, c.vis_eps, st), "pre_layrnorm");
    const bf16_t* pend = nullptr;
    {
        ClipBlocksCtx cx{h, st, &h->vis, "vision_model.", hid, c.vis_mlp, false};
        vqs::ClipBlockShape bs{N, Sv, hid, c.vis_heads, c.vis_mlp, c.vis_layers, c.vis_eps, f16, h->norm_defer != 0, "vit"};
        VQS_RUN(vqs::run_clip_blocks(cx, bs, w.b, st, &pend));
    }
    // pooled_output = post_layernorm(last_hidden_state[:, 0]); image_embeds = visual_projection(pooled_output); x / ||x||
    VQS_HIP(h, vqs::launch_clip_pool_head(w.b.hidden, pend, f16, nullptr, post_w, post_b, proj, d_embed, N, Sv, hid, c.embed_dim, c.vis_eps, st),
            "image pool + head");
    return VQS_OK;
}

size_t vqs_clip_text_workspace_bytes(const vqs_clip_handle* h, int32_t n, int32_t L) {
    if (!h || h->P <= 0 || n <= 0 || L < 8 || L > h->c.txt_context) return 0;
    return carve_tower(h, nullptr, false, n, L).total;
}

int vqs_clip_encode_texts(vqs_clip_handle* h, const int32_t* d_ids, const int32_t* d_eot_pos, int32_t N, int32_t L, float* d_embed,
                          void* d_ws, size_t ws_bytes, void* stream) {
    if (!h) return VQS_ERR_INVALID;
    if (!h->bound) return fail(h, VQS_ERR_STATE, "encode_texts: weights not bound");
    const vqs_clip_config& c = h->c;
    if (!d_ids || !d_eot_pos || !d_embed || !d_ws || N <= 0) return fail(h, VQS_ERR_INVALID, "encode_texts: bad arguments");
    if (L < 8 || L > c.txt_context) return fail(h, VQS_ERR_INVALID, "encode_texts: L must be in [8, txt_context] (pad shorter rows: padding is never read)");
    const TowerWs w = carve_tower(h, (char*)d_ws, false, N, L);
    if (ws_bytes < w.total) return fail(h, VQS_ERR_WORKSPACE, "encode_texts: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int hid = c.txt_hidden;
    const bool f16 = h->fp16 != 0;

    VQS_W(tok, "text_model.embeddings.token_embedding.weight", (int64_t)c.txt_vocab * hid);
    VQS_W(pos, "text_model.embeddings.position_embedding.weight", (int64_t)c.txt_context * hid);
    VQS_W(fin_w, "text_model.final_layer_norm.weight", hid);
    VQS_W(fin_b, "text_model.final_layer_norm.bias", hid);
    VQS_W(proj, "text_projection.weight", (int64_t)c.embed_dim * hid);

    VQS_HIP(h, vqs::launch_clip_embed(d_ids, tok, pos, w.b.hidden, N, L, hid, c.txt_vocab, st), "text embed");
    const bf16_t* pend = nullptr;
    {
        ClipBlocksCtx cx{h, st, &h->txt, "text_model.", hid, c.txt_mlp, true};
        vqs::ClipBlockShape bs{N, L, hid, c.txt_heads, c.txt_mlp, c.txt_layers, c.txt_eps, f16, h->norm_defer != 0, "txt"};
        VQS_RUN(vqs::run_clip_blocks(cx, bs, w.b, st, &pend));
    }
    // final_layer_norm is per row, so norming the pooled row alone is what HF computes: pooled = final_layer_norm(h)[eot]; text_projection; x / ||x||
    VQS_HIP(h, vqs::launch_clip_pool_head(w.b.hidden, pend, f16, d_eot_pos, fin_w, fin_b, proj, d_embed, N, L, hid, c.embed_dim, c.txt_eps, st),
            "text pool + head");
    return VQS_OK;
}

int vqs_clip_similarity(const float* d_img, const float* d_txt, int32_t M, int32_t N, int32_t E, float* d_out, void* stream) {
    return vqs::abi_code(vqs::launch_clip_similarity(d_img, d_txt, M, N, E, d_out, (hipStream_t)stream));
}

int vqs_clip_similarity_pairs(const float* d_img, const float* d_txt, const int32_t* d_idx_i, const int32_t* d_idx_t, int32_t M, int32_t N,
                              int32_t K, int32_t E, float* d_out, void* stream) {
    return vqs::abi_code(vqs::launch_clip_similarity_pairs(d_img, d_txt, d_idx_i, d_idx_t, M, N, K, E, d_out, (hipStream_t)stream));
}

int vqs_clip_causal_attention(const void* q, const void* k, const void* v, void* out, int32_t B, int32_t H, int32_t S, float scale, int32_t f16,
                              void* stream) {
    return vqs::abi_code(vqs::launch_clip_causal_attention((const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, B, H, S, scale, f16 != 0,
                                                    (hipStream_t)stream));
}

int vqs_clip_embed(const int32_t* d_ids, const void* d_tok, const void* d_pos, float* d_out, int32_t n, int32_t L, int32_t D, int32_t vocab,
                   void* stream) {
    return vqs::abi_code(vqs::launch_clip_embed(d_ids, (const bf16_t*)d_tok, (const bf16_t*)d_pos, d_out, n, L, D, vocab, (hipStream_t)stream));
}

int vqs_clip_pool_head(const float* d_x, const void* d_delta, int32_t delta_f16, const int32_t* d_rows, const void* d_ln_w, const void* d_ln_b,
                       const void* d_proj, float* d_out, int32_t n, int32_t S, int32_t D, int32_t E, float eps, void* stream) {
    return vqs::abi_code(vqs::launch_clip_pool_head(d_x, (const bf16_t*)d_delta, delta_f16 != 0, d_rows, (const bf16_t*)d_ln_w, (const bf16_t*)d_ln_b,
                                             (const bf16_t*)d_proj, d_out, n, S, D, E, eps, (hipStream_t)stream));
}

}  // extern "C"
