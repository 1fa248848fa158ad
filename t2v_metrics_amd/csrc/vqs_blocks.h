// The pre-LayerNorm transformer block loop of a CLIP tower (HF CLIPEncoderLayer, modeling_clip.py), shared by the two handles
// that run one: vqs_encode_images (vqs_api.cpp; the CLIP-FlanT5 row's vision tower) and the CLIPScore row (vqs_clip.cpp; its
// vision AND text towers).  One launch sequence, so a tower computes the same bits whichever handle runs it.
//
// Residual stream protocol: a sub-layer's output GEMM writes its 16-bit result into `delta`; the NEXT norm kernel performs
// hidden += delta (written back) and normalises in the same pass.  Deferred store (norm_defer, every layer but the last):
// layer_norm2 normalises hidden + delta_attn WITHOUT writing the stream and the next layer_norm1 stores
// (hidden + delta_attn) + delta_mlp -- the same fp32 additions in the same order, 22 instead of 24 bytes per element and layer.
// On return *pend_out is the last fc2 output, NOT yet added to `hidden`: the caller's next kernel adds it.
#pragma once
#include "vqs_host.h"

#include <string>
#include <vector>

namespace vqs {

struct ClipBlockWeights {       // one layer; the linear weights in the operand type the tower runs (bf16, or the fp16 copies), biases / norms bf16
    const bf16_t *ln1w, *ln1b, *ln2w, *ln2b;
    const bf16_t *qkv_w, *qkv_b, *out_w, *out_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};

struct ClipBlockBufs {
    float* hidden;              // fp32 stream [n * S, hid]
    bf16_t *delta, *delta2, *xn, *q, *k, *v, *attn;   // [n * S, hid] each
    bf16_t* mid;                // [n * S, mlp]
};

struct ClipBlockShape {
    int n, S, hid, heads, mlp, layers;
    float eps;
    bool f16;                   // 16-bit tensors are IEEE fp16
    bool norm_defer;
    const char* stack;          // tap / label prefix: "vit" (the names vqs_encode_images has always used) or "txt"
};

// The packed (device) per-layer tensors of one tower: q|k|v fused, and the fp16 copies of the four linear weights.
struct ClipTower {
    std::vector<const bf16_t*> qkv_w, qkv_b, qkv_w16, out_w16, fc1_w16, fc2_w16;
};

// Layer i's tensors: norms, biases and (bf16 towers) the unfused linears by their HF names under `prefix`, the rest from `t`.
inline int clip_block_weights(HostBase* h, const std::string& prefix, int i, int hid, int mlp, bool f16, const ClipTower& t, ClipBlockWeights& lw) {
    const std::string p = prefix + "encoder.layers." + std::to_string(i) + ".";
    VQS_W(ln1w, p + "layer_norm1.weight", hid);
    VQS_W(ln1b, p + "layer_norm1.bias", hid);
    VQS_W(ln2w, p + "layer_norm2.weight", hid);
    VQS_W(ln2b, p + "layer_norm2.bias", hid);
    VQS_W(ow, p + "self_attn.out_proj.weight", (int64_t)hid * hid);
    VQS_W(ob, p + "self_attn.out_proj.bias", hid);
    VQS_W(f1w, p + "mlp.fc1.weight", (int64_t)mlp * hid);
    VQS_W(f1b, p + "mlp.fc1.bias", mlp);
    VQS_W(f2w, p + "mlp.fc2.weight", (int64_t)hid * mlp);
    VQS_W(f2b, p + "mlp.fc2.bias", hid);
    lw = ClipBlockWeights{ln1w, ln1b, ln2w, ln2b, f16 ? t.qkv_w16[i] : t.qkv_w[i], t.qkv_b[i], f16 ? t.out_w16[i] : ow, ob,
                          f16 ? t.fc1_w16[i] : f1w, f1b, f16 ? t.fc2_w16[i] : f2w, f2b};
    return VQS_OK;
}

// Ctx supplies the handle-specific parts:
//   HostBase* h                                                          the handle (errors, profile)
//   int weights(int layer, ClipBlockWeights& w)                          look the layer's tensors up (VQS_OK or an error code)
//   GemmOpts gemm_opts(const GemmCall& g)                                the handle's per-launch choices (tile orders ...)
//   hipError_t attention(const ClipBlockShape& s, const ClipBlockBufs& w)   q / k / v [n, heads, S, 64] -> attn [n * S, hid], scale 1/8: the vision
//                                                                        tower's full attention or the text tower's causal kernel
//   int tap(int layer, const char* what, const void* p, size_t bytes)    stage tap (no-op where the handle has none)
template <class Ctx>
int run_clip_blocks(Ctx& cx, const ClipBlockShape& s, const ClipBlockBufs& w, hipStream_t st, const bf16_t** pend_out) {
    const int NS = s.n * s.S, hid = s.hid, mlp = s.mlp;
    const bool f16 = s.f16;
    const std::string stack(s.stack);
    const std::string n_qkv = stack + " qkv", n_out = stack + " out_proj", n_fc1 = stack + " fc1", n_fc2 = stack + " fc2", n_attn = stack + " attention";
    const bf16_t* pend = nullptr;
    const bf16_t* pend_attn = nullptr;
    for (int i = 0; i < s.layers; ++i) {
        const bool defer = s.norm_defer && i + 1 < s.layers;
        ClipBlockWeights lw;
        VQS_RUN(cx.weights(i, lw));
        if (pend_attn)
            VQS_HIP(cx.h, launch_layernorm(w.hidden, pend_attn, lw.ln1w, lw.ln1b, w.xn, 0, NS, hid, s.eps, st, pend, true, f16), "layer_norm1");
        else
            VQS_HIP(cx.h, launch_layernorm(w.hidden, pend, lw.ln1w, lw.ln1b, w.xn, 0, NS, hid, s.eps, st, nullptr, true, f16), "layer_norm1");
        pend = nullptr;
        pend_attn = nullptr;
        VQS_RUN(cx.tap(i, "xn0", w.xn, (size_t)NS * hid * sizeof(bf16_t)));
        {
            GemmCall g{w.xn, lw.qkv_w, nullptr};
            g.bias = lw.qkv_b;
            g.f16 = f16;
            g.M = NS; g.N = 3 * hid; g.K = hid; g.lda = hid; g.ldw = hid; g.ldc = 0; g.epi = EPI_HEADS;
            g.S = s.S; g.H = s.heads; g.inner = hid;
            g.heads[0] = w.q; g.heads[1] = w.k; g.heads[2] = w.v;
            VQS_RUN(run_gemm(cx.h, g, cx.gemm_opts(g), st, n_qkv.c_str()));
        }
        {
            VQS_RUN(cx.tap(i, "q", w.q, (size_t)NS * hid * sizeof(bf16_t)));
            VQS_RUN(cx.tap(i, "k", w.k, (size_t)NS * hid * sizeof(bf16_t)));
            VQS_RUN(cx.tap(i, "v", w.v, (size_t)NS * hid * sizeof(bf16_t)));
            VQS_HIP(cx.h, cx.attention(s, w), n_attn);
            VQS_RUN(cx.tap(i, "attn", w.attn, (size_t)NS * hid * sizeof(bf16_t)));
        }
        {
            GemmCall g{w.attn, lw.out_w, w.delta};
            g.bias = lw.out_b;
            g.f16 = f16;
            g.M = NS; g.N = hid; g.K = hid; g.lda = hid; g.ldw = hid; g.ldc = hid; g.epi = EPI_BF16;
            VQS_RUN(run_gemm(cx.h, g, cx.gemm_opts(g), st, n_out.c_str()));
            VQS_RUN(cx.tap(i, "d_attn", w.delta, (size_t)NS * hid * sizeof(bf16_t)));
        }
        VQS_HIP(cx.h, launch_layernorm(w.hidden, w.delta, lw.ln2w, lw.ln2b, w.xn, 0, NS, hid, s.eps, st, nullptr, !defer, f16), "layer_norm2");
        if (defer) pend_attn = w.delta;
        VQS_RUN(cx.tap(i, "xn1", w.xn, (size_t)NS * hid * sizeof(bf16_t)));
        {
            GemmCall g{w.xn, lw.fc1_w, w.mid};
            g.bias = lw.fc1_b;
            g.f16 = f16;
            g.M = NS; g.N = mlp; g.K = hid; g.lda = hid; g.ldw = hid; g.ldc = mlp; g.epi = EPI_BF16_QGELU;
            VQS_RUN(run_gemm(cx.h, g, cx.gemm_opts(g), st, n_fc1.c_str()));
            VQS_RUN(cx.tap(i, "mid", w.mid, (size_t)NS * mlp * sizeof(bf16_t)));
        }
        {
            bf16_t* dst = defer ? w.delta2 : w.delta;
            GemmCall g{w.mid, lw.fc2_w, dst};
            g.bias = lw.fc2_b;
            g.f16 = f16;
            g.M = NS; g.N = hid; g.K = mlp; g.lda = mlp; g.ldw = mlp; g.ldc = hid; g.epi = EPI_BF16;
            VQS_RUN(run_gemm(cx.h, g, cx.gemm_opts(g), st, n_fc2.c_str()));
            VQS_RUN(cx.tap(i, "d_mlp", dst, (size_t)NS * hid * sizeof(bf16_t)));
            pend = dst;
        }
    }
    *pend_out = pend;
    return VQS_OK;
}

}  // namespace vqs
