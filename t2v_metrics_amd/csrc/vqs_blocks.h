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
#include "vqs_kernels.h"

#include <string>

namespace vqs {

struct GemmCall {
    const bf16_t* A;
    const bf16_t* W;
    void* C;
    const bf16_t* bias = nullptr;
    const float* resid = nullptr;
    int M, N, K;
    int lda, ldw, ldc;
    int epi;
    int S = 0, H = 0, inner = 0;
    bf16_t* heads[3] = {nullptr, nullptr, nullptr};
    int batch = 1;
    long long sA = 0, sW = 0, sC = 0;
    // fused residual + RMSNorm (see vqs_kernels.h)
    float* hres = nullptr;
    int ldh = 0;
    const bf16_t* lnw = nullptr;
    float* rowss_out = nullptr;
    const float* rowss_in = nullptr;
    int rowss_parts = 0;
    float rs_invd = 0.0f, rs_eps = 0.0f;
    int nt_store = 0;          // result rows leave with the non-temporal hint (call sites whose multi-GB output is streamed once)
    long long split_off = 0;   // EPI_BF16: also store the lo plane of a split-bf16 result at C + split_off (vqs_kernels.h)
    float acc_scale = 1.0f, out_scale = 1.0f;   // f16 = 3 / 4: the scaled quad families (vqs_kernels.h)
    int no_stream = 0;         // 1: keep this launch off the stream form (same bits either way)
    int f16 = 0;               // A, W and the 16-bit result are IEEE fp16 (the fp16 vision tower; quad form only)
};

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

// Ctx supplies the handle-specific parts:
//   int weights(int layer, ClipBlockWeights& w)                          look the layer's tensors up (VQS_OK or an error code)
//   int gemm(const GemmCall& g, const char* what)                        launch (profiling, tile orders ... are the handle's business)
//   hipError_t attention(const ClipBlockShape& s, const ClipBlockBufs& w)   q / k / v [n, heads, S, 64] -> attn [n * S, hid], scale 1/8: the vision
//                                                                        tower's full attention or the text tower's causal kernel
//   int hip(hipError_t e, const char* what)                              VQS_OK, or record the message and return VQS_ERR_HIP
//   int tap(int layer, const char* what, const void* p, size_t bytes)    stage tap (no-op where the handle has none)
template <class Ctx>
int run_clip_blocks(Ctx& cx, const ClipBlockShape& s, const ClipBlockBufs& w, hipStream_t st, const bf16_t** pend_out) {
#define VQS_BLK(expr)              \
    do {                           \
        int _r = (expr);           \
        if (_r != 0) return _r;    \
    } while (0)
    const int NS = s.n * s.S, hid = s.hid, mlp = s.mlp;
    const bool f16 = s.f16;
    const std::string stack(s.stack);
    const std::string n_qkv = stack + " qkv", n_out = stack + " out_proj", n_fc1 = stack + " fc1", n_fc2 = stack + " fc2", n_attn = stack + " attention";
    const bf16_t* pend = nullptr;
    const bf16_t* pend_attn = nullptr;
    for (int i = 0; i < s.layers; ++i) {
        const bool defer = s.norm_defer && i + 1 < s.layers;
        ClipBlockWeights lw;
        VQS_BLK(cx.weights(i, lw));
        if (pend_attn)
            VQS_BLK(cx.hip(launch_layernorm(w.hidden, pend_attn, lw.ln1w, lw.ln1b, w.xn, 0, NS, hid, s.eps, st, pend, true, f16), "layer_norm1"));
        else
            VQS_BLK(cx.hip(launch_layernorm(w.hidden, pend, lw.ln1w, lw.ln1b, w.xn, 0, NS, hid, s.eps, st, nullptr, true, f16), "layer_norm1"));
        pend = nullptr;
        pend_attn = nullptr;
        VQS_BLK(cx.tap(i, "xn0", w.xn, (size_t)NS * hid * sizeof(bf16_t)));
        {
            GemmCall g{w.xn, lw.qkv_w, nullptr};
            g.bias = lw.qkv_b;
            g.f16 = f16;
            g.M = NS; g.N = 3 * hid; g.K = hid; g.lda = hid; g.ldw = hid; g.ldc = 0; g.epi = EPI_HEADS;
            g.S = s.S; g.H = s.heads; g.inner = hid;
            g.heads[0] = w.q; g.heads[1] = w.k; g.heads[2] = w.v;
            VQS_BLK(cx.gemm(g, n_qkv.c_str()));
        }
        {
            VQS_BLK(cx.tap(i, "q", w.q, (size_t)NS * hid * sizeof(bf16_t)));
            VQS_BLK(cx.tap(i, "k", w.k, (size_t)NS * hid * sizeof(bf16_t)));
            VQS_BLK(cx.tap(i, "v", w.v, (size_t)NS * hid * sizeof(bf16_t)));
            VQS_BLK(cx.hip(cx.attention(s, w), n_attn.c_str()));
            VQS_BLK(cx.tap(i, "attn", w.attn, (size_t)NS * hid * sizeof(bf16_t)));
        }
        {
            GemmCall g{w.attn, lw.out_w, w.delta};
            g.bias = lw.out_b;
            g.f16 = f16;
            g.M = NS; g.N = hid; g.K = hid; g.lda = hid; g.ldw = hid; g.ldc = hid; g.epi = EPI_BF16;
            VQS_BLK(cx.gemm(g, n_out.c_str()));
            VQS_BLK(cx.tap(i, "d_attn", w.delta, (size_t)NS * hid * sizeof(bf16_t)));
        }
        VQS_BLK(cx.hip(launch_layernorm(w.hidden, w.delta, lw.ln2w, lw.ln2b, w.xn, 0, NS, hid, s.eps, st, nullptr, !defer, f16), "layer_norm2"));
        if (defer) pend_attn = w.delta;
        VQS_BLK(cx.tap(i, "xn1", w.xn, (size_t)NS * hid * sizeof(bf16_t)));
        {
            GemmCall g{w.xn, lw.fc1_w, w.mid};
            g.bias = lw.fc1_b;
            g.f16 = f16;
            g.M = NS; g.N = mlp; g.K = hid; g.lda = hid; g.ldw = hid; g.ldc = mlp; g.epi = EPI_BF16_QGELU;
            VQS_BLK(cx.gemm(g, n_fc1.c_str()));
            VQS_BLK(cx.tap(i, "mid", w.mid, (size_t)NS * mlp * sizeof(bf16_t)));
        }
        {
            bf16_t* dst = defer ? w.delta2 : w.delta;
            GemmCall g{w.mid, lw.fc2_w, dst};
            g.bias = lw.fc2_b;
            g.f16 = f16;
            g.M = NS; g.N = hid; g.K = mlp; g.lda = mlp; g.ldw = mlp; g.ldc = hid; g.epi = EPI_BF16;
            VQS_BLK(cx.gemm(g, n_fc2.c_str()));
            VQS_BLK(cx.tap(i, "d_mlp", dst, (size_t)NS * hid * sizeof(bf16_t)));
            pend = dst;
        }
    }
    *pend_out = pend;
    return 0;
#undef VQS_BLK
}

}  // namespace vqs
