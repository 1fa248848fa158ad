// Host side of libvqs_hip: the C ABI of include/vqs.h and the launch sequence of the CLIP-FlanT5
// scoring pass.  The sequence restates what HF executes for the reference:
//   CLIPVisionModel.forward   HF models/clip/modeling_clip.py:613-656  -> encode_images()
//   T5Stack encoder           HF models/t5/modeling_t5.py:663-750      -> score(): encoder loop
//   T5Stack decoder + lm_head HF models/t5/modeling_t5.py:1026-1047    -> score(): decoder loop
// No device allocation, no stream synchronisation, no CPU fallback: if a launch fails the call
// returns VQS_ERR_HIP and the message says which one.
#include "../../include/vqs.h"
#include "../../include/vqs_debug.h"
#include "vqs_blocks.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

using vqs::bf16_t;
using vqs::align_up;
using vqs::Carver;
using vqs::fail;
using vqs::GemmCall;

#if defined(VQS_ATTN_TIMING) && VQS_ATTN_TIMING
namespace vqs { hipError_t lab_set_attn_timing(unsigned long long* d_buf); }   // attn.hip, timing build only
#endif

struct vqs_handle : vqs::HostBase {
    vqs_config c;
    int gemm_variant = 0;
    // derived
    int P = 0, Sv = 0, kpatch = 0, kpad = 0, I = 0;
    // packed (device) weights
    const bf16_t* patch_w = nullptr;
    vqs::ClipTower vit;       // q|k|v fused; the fp16 copies serve option vit_fp16
    std::vector<const bf16_t*> enc_qkv, enc_wi, dec_qkv, dec_ckv, dec_wi, dec_ckT;
    int cross_mode = 1;   // 1 = reassociated cross-attention (default), 0 = per-layer K|V projection of the encoder output
    int stream_gemm = 1;  // 1 = skinny batched launches (M <= 128 rows per entry) take the HBM-streaming GEMM form (gemm_stream.inc; bitwise the 8-wave forms), 0 = never
    int vit_fp16 = 1;     // 1 (default) = the vision tower and the projector run on IEEE fp16 operands (11 significant bits instead of bf16's 8, same MFMA rate and
                          // bytes): fp16 copies of their weights (made at bind time), fp16 activations, fp32 accumulation / residual stream / statistics
                          // as before; the image features leave as bf16 (the C ABI's type).  CLIP was trained in fp16; the T5 stack is NOT fp16-safe
                          // and stays bf16.  0 = the bf16 tower of rounds 1-3 (what the reference's dtype would give)
    const bf16_t* proj0_w16 = nullptr;
    const bf16_t* proj2_w16 = nullptr;
    int dec_precise = 1;  // 1 = the scoring decoder holds its activations as split-bf16 / fp32 (decoder_pass_precise), 0 = bf16 (rounds 1-3)
    int proj_fp16 = 1;    // 1 (default) = with vit_fp16 the selected features (hidden_states[-2], the residual STREAM itself cast to 16 bits) and the projector's
                          // hidden tensor are fp16 too; 0 = they stay bf16 while the tower's blocks run fp16.  Round 6: the stream is a sum over all
                          // blocks' outputs -- the one site of the tower whose bind-time range proof (engine.py fp16_range_proof) fails first
    int proj_fs_shift = 0, proj_mid_shift = 0;   // with proj_fp16: the selected features are held as fp16(x * 2^-fs), the projector's hidden tensor as
                          // fp16(x * 2^-mid) -- the scales the bind-time range proof asks for (engine.py; 0 = none: the unscaled kernels, bit for bit round 5)
    int enc_fp16 = 1;     // 1 (default, round 5) = the ATTENTION SIDE of the T5 encoder runs on IEEE fp16 tensors: both norm outputs, q / k / v, the
                          // softmax probabilities and the attention output are fp16, and q|k|v, o and the gated wi read fp16 copies of their weights
                          // (made at bind time) -- what HF's own fp16 T5 path holds in fp16.  The sub-layer outputs (o / wo results), the gated FFN
                          // product and the wo GEMM stay bf16: those are where Flan-T5 leaves the fp16 range (HF keeps `wo` in fp32 for it,
                          // modeling_t5.py _keep_in_fp32_modules); the residual stream is fp32 here anyway.  Same MFMA rate, same bytes, three more
                          // significant bits on five of the encoder's seven 16-bit tensor classes (profiles/r5_error_attribution_xxl.md).  0 = bf16
    std::vector<const bf16_t*> enc_qkv16, enc_o16, enc_wi16;   // the fp16 copies (packed buffer)
    int dec_fp16 = 1;     // 1 (default, round 5; effective with dec_precise = 1 and cross_mode = 1) = the precise decoder's cross-attention SCORE path
                          // and the tensor it attends over are IEEE fp16: the encoder's output E (its final norm writes fp16), the cross q (from BOTH
                          // planes of the split norm output, rounded once to fp16), q.Wk (fp16 copy of Wk^T), the probabilities; the three products
                          // q.Wk, (q.Wk).E^T and P.E run on fp16 MFMAs (the batched 8-wave and stream kernels' fp16 instantiations), P.E still leaves as
                          // a split-bf16 tensor.  The reassociated cross-attention makes the rounding of q.Wk and of P COHERENT over all ~600 keys,
                          // which is why these three bf16 roundings were most of the precise decoder's floor (profiles/r5_error_attribution_xxl.md).
                          // 0 = bf16 there (round 4's precise decoder).  vqs_generate and dec_precise = 0 / cross_mode = 0 always run bf16.
    std::vector<const bf16_t*> dec_ckT16;                      // fp16 copies of Wk^T (packed buffer)
    const int* lut_bidir = nullptr;
    const int* lut_causal = nullptr;
    int lut_len = 0;
    std::vector<int> h_lut_bidir, h_lut_causal;
    int norm_defer = 1;        // VQS_NORM_DEFER=0: every norm stores the updated fp32 stream (24 instead of 22 B/elem per layer)
    int fused_norm = 0;        // VQS_FUSED_NORM=1: residual update + RMSNorm operand in the o / wo GEMM epilogues (lab; +1 %)
    int splitk = 1;            // VQS_SPLITK=0 disables split-K in the decoder's skinny GEMMs (lab A/B)
    // per-shape tile order of the big GEMMs (option "tile_order:<N>x<K>"): a permutation of the tile list, results unchanged
    struct TileOrder { int N, K, gm, ns; };
    std::vector<TileOrder> tile_orders;
    // per-shape non-temporal result stores (option "nt_store:<N>x<K>" = 1 on, 2 off; absent = the library's choice)
    struct NtStore { int N, K, on; };
    std::vector<NtStore> nt_stores, l2_touches;      // l2_touches: option "l2_touch:<N>x<K>" = 1 on, 2 off
};

namespace {

struct EncodeWs {
    bf16_t* im2col;
    float* patch_out;
    float* pre;
    float* hidden;
    bf16_t *delta, *delta2;
    bf16_t *xn, *q, *k, *v, *attn, *mid, *feat_in, *pmid;
    size_t total;
};

EncodeWs carve_encode(const vqs_handle* h, char* base, int N, std::unordered_map<std::string, size_t>* names = nullptr) {
    const vqs_config& c = h->c;
    Carver cv{base, 0, names};
    EncodeWs w;
    const size_t NP = (size_t)N * h->P, NS = (size_t)N * h->Sv;
    w.im2col = cv.take<bf16_t>(NP * h->kpad);
    w.patch_out = cv.take<float>(NP * c.vis_hidden);
    w.pre = cv.take<float>(NS * c.vis_hidden);
    w.hidden = cv.take<float>(NS * c.vis_hidden, "vit_hidden");
    w.delta = cv.take<bf16_t>(NS * c.vis_hidden);
    w.delta2 = cv.take<bf16_t>(NS * c.vis_hidden);
    w.xn = cv.take<bf16_t>(NS * c.vis_hidden);
    w.q = cv.take<bf16_t>(NS * c.vis_hidden);
    w.k = cv.take<bf16_t>(NS * c.vis_hidden);
    w.v = cv.take<bf16_t>(NS * c.vis_hidden);
    w.attn = cv.take<bf16_t>(NS * c.vis_hidden);
    w.mid = cv.take<bf16_t>(NS * c.vis_mlp);
    w.feat_in = cv.take<bf16_t>(NP * c.vis_hidden);
    w.pmid = cv.take<bf16_t>(NP * c.d_model);
    w.total = cv.total();
    return w;
}

struct ScoreWs {
    int *sent_pos, *enc_len, *flags;
    float *enc_table, *dec_table, *hidden;
    bf16_t *delta, *delta2, *ddelta;
    float* rowss;             // [ceil(D/256)][B*S] partial row sums of squares (fused residual + RMSNorm)
    float* rs;                // [B*S] 1/rms per row, derived from rowss
    bf16_t *xn, *q, *k, *v, *attn, *ff, *enc_out, *ck, *cv;
    float* dhid;
    bf16_t *dxn, *dqkv, *dattn, *dq, *dff;     // dxn, dattn, dff, cctx hold TWO planes [2][rows][width] (split-bf16; plane 0 = the bf16 tensor of rounds 1-3)
    float *dqkv32, *ddelta32, *dscratch;       // precise decoder: fp32 q|k|v, fp32 sub-layer output, GEMM partials
    size_t dscratch_bytes;
    bf16_t *enc_outT, *cqk, *cprobs, *cctx;
    float* cscores;
    int S_pad;
    float* logits;
    int ldl;
    bf16_t* kvcache;          // incremental decoding: [dec_layers][B][Tc][2I] (k | v of every decoded position), else nullptr
    int Tc;
    size_t total;
};

// T = decoder rows per pair held at once; Tc > 0 additionally carves the self-attention K/V cache of vqs_generate for Tc
// positions (the decoder buffers are then sized for T rows per step -- 1 -- and the bias table for Tc distances).
ScoreWs carve_score(const vqs_handle* h, char* base, int B, int L, int T,
                    std::unordered_map<std::string, size_t>* names = nullptr, int Tc = 0) {
    const vqs_config& c = h->c;
    Carver cv{base, 0, names};
    ScoreWs w;
    const int S = L - 1 + h->P;
    const size_t M = (size_t)B * S, MT = (size_t)B * T;
    const int D = c.d_model, I = h->I, F = c.d_ff, H = c.n_heads;
    w.sent_pos = cv.take<int>(B);
    w.enc_len = cv.take<int>(B, "enc_len");
    w.flags = cv.take<int>(4, "flags");
    w.enc_table = cv.take<float>((size_t)H * (2 * S - 1));
    w.dec_table = cv.take<float>((size_t)H * (T > Tc ? T : Tc));
    w.hidden = cv.take<float>(M * D, "enc_in");   // the fp32 residual stream; holds enc_in until layer 0 runs
    w.delta = cv.take<bf16_t>(M * D);            // bf16 sub-layer output waiting to be added by the next norm
    w.delta2 = cv.take<bf16_t>(M * D);           // second pending delta (deferred stream store, VQS_NORM_DEFER)
    w.xn = cv.take<bf16_t>(M * D);
    w.rowss = cv.take<float>((size_t)((D + 255) / 256) * M);
    w.rs = cv.take<float>(M);
    w.q = cv.take<bf16_t>(M * I);
    w.k = cv.take<bf16_t>(M * I);
    w.v = cv.take<bf16_t>(M * I);
    w.attn = cv.take<bf16_t>(M * I);
    w.ff = cv.take<bf16_t>(M * F);
    w.enc_out = cv.take<bf16_t>(M * D, "enc_out");
    w.ck = cv.take<bf16_t>(M * I);
    w.cv = cv.take<bf16_t>(M * I);
    w.dhid = cv.take<float>(MT * D);
    w.ddelta = cv.take<bf16_t>(MT * D);
    w.dxn = cv.take<bf16_t>(2 * MT * D, "dec_out");   // after a pass: the final-norm output (lm_head operand); hi plane, then lo plane
    w.dqkv = cv.take<bf16_t>(MT * 3 * I);
    w.dattn = cv.take<bf16_t>(2 * MT * I);
    w.dq = cv.take<bf16_t>(MT * I);
    w.dff = cv.take<bf16_t>(2 * MT * F);
    w.dqkv32 = cv.take<float>(MT * 3 * I);
    w.ddelta32 = cv.take<float>(MT * D);
    {   // fp32 partials of one decoder GEMM: [slices][2 * MT stacked rows][N] with slices * N <= 16 384 when split (dec_slices) or
        // one slice of the widest N -- a function of the architecture, so no launch ever has to fall back for lack of scratch
        size_t widest = 16384;
        for (size_t n : {(size_t)3 * I, (size_t)2 * F, (size_t)c.vocab, (size_t)D}) widest = n > widest ? n : widest;
        w.dscratch_bytes = 2 * MT * widest * sizeof(float);
        w.dscratch = cv.take<float>(2 * MT * widest);
    }
    w.S_pad = (S + 63) / 64 * 64;
    w.enc_outT = cv.take<bf16_t>((size_t)B * D * w.S_pad);
    w.cqk = cv.take<bf16_t>(MT * H * D);
    w.cscores = cv.take<float>(MT * H * w.S_pad);
    w.cprobs = cv.take<bf16_t>(MT * H * w.S_pad);
    w.cctx = cv.take<bf16_t>(2 * MT * H * D);
    w.ldl = c.vocab;
    w.logits = cv.take<float>(MT * w.ldl, "logits");
    w.Tc = Tc;
    w.kvcache = Tc > 0 ? cv.take<bf16_t>((size_t)c.dec_layers * B * Tc * 2 * I) : nullptr;
    w.total = cv.total();
    return w;
}

struct PackedLayout {
    size_t patch_w;
    std::vector<size_t> vit_qkv_w, vit_qkv_b, enc_qkv, enc_wi, dec_qkv, dec_ckv, dec_wi, dec_ckT;
    std::vector<size_t> vit_qkv_w16, vit_out_w16, vit_fc1_w16, vit_fc2_w16;    // fp16 copies for option vit_fp16 (always laid out: 0.45 GB for ViT-L)
    size_t proj0_w16, proj2_w16;
    std::vector<size_t> enc_qkv16, enc_o16, enc_wi16;                          // fp16 copies for option enc_fp16 (always laid out: 7.2 GB at XXL, 1.9 GB at XL)
    std::vector<size_t> dec_ckT16;                                             // fp16 copies of Wk^T for option dec_fp16 (0.8 GB at XXL)
    size_t lut_bidir, lut_causal;
    size_t total;
};

PackedLayout packed_layout(const vqs_handle* h) {
    const vqs_config& c = h->c;
    Carver cv{nullptr};
    PackedLayout pl;
    auto take = [&](size_t elems) { return cv.mark(elems * sizeof(bf16_t)); };
    const size_t hid = c.vis_hidden, D = c.d_model, I = h->I, F = c.d_ff;
    pl.patch_w = take(hid * h->kpad);
    for (int i = 0; i < c.vis_layers_run; ++i) {
        pl.vit_qkv_w.push_back(take(3 * hid * hid));
        pl.vit_qkv_b.push_back(take(3 * hid));
    }
    for (int i = 0; i < c.enc_layers; ++i) {
        pl.enc_qkv.push_back(take(3 * I * D));
        pl.enc_wi.push_back(take(2 * F * D));
    }
    for (int i = 0; i < c.dec_layers; ++i) {
        pl.dec_qkv.push_back(take(3 * I * D));
        pl.dec_ckv.push_back(take(2 * I * D));
        pl.dec_ckT.push_back(take(I * D));
        pl.dec_wi.push_back(take(2 * F * D));
    }
    for (int i = 0; i < c.vis_layers_run; ++i) {
        pl.vit_qkv_w16.push_back(take(3 * hid * hid));
        pl.vit_out_w16.push_back(take(hid * hid));
        pl.vit_fc1_w16.push_back(take((size_t)c.vis_mlp * hid));
        pl.vit_fc2_w16.push_back(take((size_t)c.vis_mlp * hid));
    }
    pl.proj0_w16 = take(D * hid);
    pl.proj2_w16 = take(D * D);
    for (int i = 0; i < c.enc_layers; ++i) {
        pl.enc_qkv16.push_back(take(3 * I * D));
        pl.enc_o16.push_back(take(D * I));
        pl.enc_wi16.push_back(take(2 * F * D));
    }
    for (int i = 0; i < c.dec_layers; ++i) pl.dec_ckT16.push_back(take(I * D));
    pl.lut_bidir = take(2 * (size_t)(c.rel_max_distance + 1));   // int32 = 2 bf16 slots each
    pl.lut_causal = take(2 * (size_t)(c.rel_max_distance + 1));
    pl.total = cv.total();
    return pl;
}

// The handle's say in a launch: option gemm_variant / stream_gemm and the per-shape cache-policy options ("tile_order:", "l2_touch:",
// "nt_store:"; the latter two for the big launches only -- the decoder shares (N, K)).
vqs::GemmOpts gemm_opts(const vqs_handle* h, const GemmCall& g) {
    vqs::GemmOpts o;
    o.variant = h->gemm_variant;
    o.stream = h->stream_gemm != 0;
    for (const vqs_handle::TileOrder& t : h->tile_orders)
        if (t.N == g.N && t.K == g.K) { o.tile_gm = t.gm; o.tile_ns = t.ns; }
    for (const vqs_handle::NtStore& t : h->l2_touches)
        if (t.N == g.N && t.K == g.K && g.M >= 4096) o.l2_touch = t.on;
    for (const vqs_handle::NtStore& t : h->nt_stores)
        if (t.N == g.N && t.K == g.K && g.M >= 4096) o.nt_store = t.on == 1;
    return o;
}
int run_gemm(vqs_handle* h, const GemmCall& g, hipStream_t st, const char* what) { return vqs::run_gemm(h, g, gemm_opts(h, g), st, what); }

#define TAP2(stack, layer, what, ptr, plane_elems) VQS_RUN(vqs::tap_split(h, stack, layer, what, ptr, (size_t)(plane_elems), st))

// vqs_encode_images' side of the shared tower block loop (vqs_blocks.h): weights by their HF names, launches through run_gemm
// (per-shape cache-policy options), stage taps under "vit.<layer>.<what>".
struct VitBlocksCtx {
    vqs_handle* h;
    hipStream_t st;
    int weights(int i, vqs::ClipBlockWeights& lw) {
        return vqs::clip_block_weights(h, "vision.", i, h->c.vis_hidden, h->c.vis_mlp, h->vit_fp16 != 0, h->vit, lw);
    }
    vqs::GemmOpts gemm_opts(const GemmCall& g) const { return ::gemm_opts(h, g); }
    hipError_t attention(const vqs::ClipBlockShape& s, const vqs::ClipBlockBufs& w) {
        vqs::AttnParams a{w.q, w.k, w.v, w.attn, nullptr, nullptr, s.n, s.heads, s.S, 0.125f};
        a.f16 = s.f16;
        return vqs::launch_attention(a, st);
    }
    int tap(int layer, const char* what, const void* p, size_t bytes) { return vqs::tap(h, "vit", layer, what, p, bytes, st); }
};

// The integers of a GEMM launch (include/vqs_debug.h, VQS_GEMM_PLAN_FIELDS) as the launcher's parameter block: the ONE place both GEMM hooks fill it, so that
// vqs_debug_gemm_plan describes exactly what vqs_debug_gemm_launch launches.  An operand whose flag is set is taken from `ops`; everything else stays null.
enum { GL_BIAS = 1, GL_ROWSS = 2, GL_NO_STREAM = 4, GL_ROPE_COS = 8, GL_ROPE_SIN = 16, GL_RMS = 32, GL_HANDLE = 64 };
struct GemmLaunchOperands {
    const void* bias;
    const float *rowss_in, *rope_cos, *rope_sin;
    float* hres;
    const bf16_t* lnw;
    float* rowss_out;
};
void gemm_params_of(const int32_t* launch, const GemmLaunchOperands& ops, vqs::GemmParams& p) {
    const int32_t flags = launch[18];
    p.M = launch[0]; p.N = launch[1]; p.K = launch[2]; p.lda = launch[3]; p.ldw = launch[4]; p.ldc = launch[5]; p.batch = launch[7];
    p.S = launch[9]; p.inner = launch[10]; p.inner_kv = launch[11]; p.hd = launch[12]; p.hd_src = launch[13]; p.Hkv = launch[14];
    p.f16 = launch[15]; p.l2_touch = launch[16]; p.split_off = launch[17];
    p.gate_act = launch[19]; p.rowss_parts = launch[20]; p.ldh = launch[21];
    if (flags & GL_BIAS) p.bias = (const bf16_t*)ops.bias;
    if (flags & GL_ROWSS) p.rowss_in = ops.rowss_in;
    if (flags & GL_NO_STREAM) p.no_stream = 1;
    if (flags & GL_ROPE_COS) p.rope_cos = ops.rope_cos;
    if (flags & GL_ROPE_SIN) p.rope_sin = ops.rope_sin;
    if (flags & GL_RMS) { p.hres = ops.hres; p.lnw = ops.lnw; p.rowss_out = ops.rowss_out; }
}

}  // namespace

extern "C" {

int vqs_debug_tap(vqs_handle* h, const char* name, void* d_dst, size_t bytes) {
    if (!h) return VQS_ERR_INVALID;
    h->taps.set(name, d_dst, bytes);
    return VQS_OK;
}

int vqs_debug_tap_window(vqs_handle* h, int32_t first, int32_t count) {
    if (!h || first < 0 || count < 0) return VQS_ERR_INVALID;
    h->taps.first = count > 0 ? first : 0;
    h->taps.count = count;
    return VQS_OK;
}

int vqs_debug_gemm_form(int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t epilogue, int32_t batch, int32_t variant,
                        int32_t S, int32_t inner, int32_t inner_kv) {
    const int32_t launch[VQS_GEMM_PLAN_FIELDS] = {M, N, K, lda, ldw, N, epilogue, batch > 0 ? batch : 1, variant & 0xff, S, inner, inner_kv};
    int32_t plan[5];
    if (vqs_debug_gemm_plan(launch, VQS_GEMM_PLAN_FIELDS, plan) != 1) return -1;
    static const int form_of[] = {0, 0, 3, 3, 12, 10, 13};      // by vqs::GemmKernel: tile, tile ping-pong, persistent, ping-pong, stream, quad, slim
    return form_of[plan[0]];
}

int vqs_debug_gemm_plan(const int32_t* launch, int32_t n, int32_t* plan) {
    if (!launch || n != VQS_GEMM_PLAN_FIELDS || !plan) return VQS_ERR_INVALID;
    static const float present = 0.0f;      // stands for an operand that is there: the plan is host arithmetic and reads no operand
    float* const there = const_cast<float*>(&present);
    const GemmLaunchOperands ops{there, there, there, there, there, (const bf16_t*)there, there};
    vqs::GemmParams p{};
    gemm_params_of(launch, ops, p);
    vqs::GemmPlan g;
    if (!vqs::gemm_plan(p, launch[6], launch[8] & 0xff, &g, (launch[18] & GL_HANDLE) != 0)) return 0;
    plan[0] = g.kernel; plan[1] = g.touch; plan[2] = g.type; plan[3] = g.grid; plan[4] = g.block;
    return 1;
}

int vqs_debug_gemm_launch(const int32_t* launch, int32_t n, const void* const* ptrs, int32_t nptrs, const float* scales, int32_t nscales, void* stream) {
    if (!launch || n != VQS_GEMM_LAUNCH_FIELDS || !ptrs || nptrs != VQS_GEMM_LAUNCH_PTRS || !scales || nscales != VQS_GEMM_LAUNCH_SCALES) return VQS_ERR_INVALID;
    enum { P_A, P_W, P_C, P_BIAS, P_HEADS0, P_HEADS1, P_HEADS2, P_ROPE_COS, P_ROPE_SIN, P_ROWSS };
    const int32_t flags = launch[18], epilogue = launch[6];
    // batched launches, the fused residual + RMSNorm, split results and a handle's launches have hooks of their own (vqs_debug_gemm_batched, vqs_gemm_rms);
    // EPI_F32_RESID's residual is not among ptrs
    if (launch[7] > 1 || epilogue == vqs::EPI_RESID_RMS || epilogue == vqs::EPI_F32_RESID || launch[17] != 0 || (flags & ~(GL_BIAS | GL_ROWSS | GL_NO_STREAM | GL_ROPE_COS | GL_ROPE_SIN)) != 0)
        return VQS_ERR_INVALID;
    // a flag requires its pointer and a pointer its flag: the plan hook, which sees the flags only, then describes this very launch
    const struct { int flag, ptr; } pairs[] = {{GL_BIAS, P_BIAS}, {GL_ROWSS, P_ROWSS}, {GL_ROPE_COS, P_ROPE_COS}, {GL_ROPE_SIN, P_ROPE_SIN}};
    for (const auto& pr : pairs)
        if (((flags & pr.flag) != 0) != (ptrs[pr.ptr] != nullptr)) return VQS_ERR_INVALID;
    if (!ptrs[P_A] || !ptrs[P_W]) return VQS_ERR_INVALID;
    if (epilogue == vqs::EPI_HEADS ? (!ptrs[P_HEADS0] || !ptrs[P_HEADS1] || !ptrs[P_HEADS2] || launch[22] <= 0 || launch[9] <= 0) : !ptrs[P_C]) return VQS_ERR_INVALID;
    const GemmLaunchOperands ops{ptrs[P_BIAS], (const float*)ptrs[P_ROWSS], (const float*)ptrs[P_ROPE_COS], (const float*)ptrs[P_ROPE_SIN], nullptr, nullptr, nullptr};
    vqs::GemmParams p{};
    gemm_params_of(launch, ops, p);
    p.A = (const bf16_t*)ptrs[P_A]; p.W = (const bf16_t*)ptrs[P_W]; p.C = const_cast<void*>(ptrs[P_C]);
    for (int t = 0; t < 3; ++t) p.heads_out[t] = (bf16_t*)const_cast<void*>(ptrs[P_HEADS0 + t]);
    p.H = launch[22];
    p.acc_scale = scales[0]; p.out_scale = scales[1]; p.rs_invd = scales[2]; p.rs_eps = scales[3];
    return vqs::abi_code(vqs::launch_gemm(p, epilogue, launch[8] & 0xff, (hipStream_t)stream));
}

int vqs_debug_gemm_batched(const void* A, const void* W, void* C, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw, int32_t ldc,
                           int32_t epilogue, int32_t batch, int64_t sA, int64_t sW, int64_t sC, int64_t split_off, int32_t no_stream,
                           int32_t variant, void* stream) {
    if (!A || !W || !C || (epilogue != vqs::EPI_F32 && epilogue != vqs::EPI_BF16) || batch < 1) return VQS_ERR_INVALID;
    vqs::GemmParams p{};
    p.A = (const bf16_t*)A; p.W = (const bf16_t*)W; p.C = C; p.bias = nullptr; p.resid = nullptr;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = ldc;
    p.S = 1; p.H = 0; p.inner = 1;
    p.batch = batch; p.sA = sA; p.sW = sW; p.sC = sC;
    p.split_off = split_off; p.no_stream = no_stream;
    p.f16 = (variant >> 27) & 3;           // bits 27-28 of `variant`, as in vqs_gemm: 0 bf16, 1 fp16 operands and result, 2 fp16 operands / bf16 (split) result
    if (p.f16 == 3) return VQS_ERR_INVALID;
    return vqs::launch_gemm(p, epilogue, variant & 0xff, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_debug_heads_rows(int32_t row0, int32_t S, int32_t hx, int32_t hdim, int32_t n, int64_t* off_out) {
    if (row0 < 0 || S < 8 || hx <= 0 || hdim <= 0 || n <= 0 || !off_out) return VQS_ERR_INVALID;
    int hs;
    long long off;
    vqs::heads_off_first(row0, S, hx, hdim, hs, off);
    const long long wrap = (long long)(hx - 1) * S * hdim;
    for (int k = 0; k < n; ++k) {          // exactly the use-then-step order of the GEMM epilogue
        off_out[k] = off;
        vqs::heads_off_step8(S, hdim, wrap, hs, off);
    }
    return VQS_OK;
}

int vqs_debug_tile_order(int32_t M, int32_t N, int32_t K, int32_t batch, int32_t gm, int32_t ns, int32_t grid, int32_t* out) {
    if (M <= 0 || N <= 0 || K < 0 || batch <= 0 || grid <= 0 || (grid & 7) != 0 || !out) return VQS_ERR_INVALID;
    vqs::GemmParams p{};
    p.M = M; p.N = N; p.K = K; p.batch = batch; p.tile_gm = gm; p.tile_ns = ns;
    vqs::resolve_tile_order(p, grid);
    const int tiles_m = (M + vqs::GEMM_BM - 1) / vqs::GEMM_BM, tiles_n = (N + vqs::GEMM_BN - 1) / vqs::GEMM_BN;
    const int nwg = tiles_m * tiles_n * batch;
    // the persistent kernels' walk: workgroup b takes slots b, b + grid, b + 2 grid, ... while slot < nwg
    int k = 0;
    for (int b = 0; b < grid; ++b)
        for (int pid = b; pid < nwg; pid += grid) {
            int m0, n0, bz;
            vqs::tile_of_slot(pid, nwg, tiles_m, tiles_n, p.tile_gm, p.tile_ns, m0, n0, bz);
            out[4 * k + 0] = pid; out[4 * k + 1] = m0; out[4 * k + 2] = n0; out[4 * k + 3] = bz;
            ++k;
        }
    return k == nwg ? (p.tile_gm | (p.tile_ns << 8)) : VQS_ERR_INVALID;
}

#if defined(VQS_ATTN_TIMING) && VQS_ATTN_TIMING
// lab builds only (make variant NAME=attn_timing VFLAGS=-DVQS_ATTN_TIMING=1): d_buf = 8 x uint64 on the device, zeroed by the caller
int vqs_lab_set_attn_timing(void* d_buf) { return vqs::lab_set_attn_timing((unsigned long long*)d_buf) == hipSuccess ? VQS_OK : VQS_ERR_HIP; }
#endif


int64_t vqs_attention_lds_bytes(int32_t S, int32_t has_bias, int32_t hd) {
    if (S <= 0 || (hd != 0 && hd != 64 && hd != 128)) return -1;
    return (int64_t)vqs::attention_lds_bytes(S, has_bias != 0, hd);
}

int32_t vqs_relpos_bucket(int32_t relative_position, int32_t bidirectional, int32_t num_buckets, int32_t max_distance) {
    // HF models/t5/modeling_t5.py:238-262, same fp32 operation order as torch.
    int32_t bucket = 0, nb = num_buckets, rp = relative_position;
    if (bidirectional) {
        nb /= 2;
        if (rp > 0) bucket += nb;
        if (rp < 0) rp = -rp;
    } else {
        rp = rp < 0 ? -rp : 0;
    }
    const int32_t max_exact = nb / 2;
    if (rp < max_exact) return bucket + rp;
    float v = logf((float)rp / (float)max_exact) / (float)std::log((double)max_distance / (double)max_exact);
    v = v * (float)(nb - max_exact);
    int32_t large = max_exact + (int32_t)v;
    if (large > nb - 1) large = nb - 1;
    return bucket + large;
}

int vqs_create(const vqs_config* cfg, vqs_handle** out) {
    if (!cfg || !out) return VQS_ERR_INVALID;
    vqs_handle* h = new vqs_handle();
    h->c = *cfg;
    const vqs_config& c = h->c;
    *out = h;
    auto bad = [&](const char* m) { return fail(h, VQS_ERR_INVALID, m); };
    if (c.d_kv != 64) return bad("d_kv must be 64");
    if (c.vis_hidden <= 0 || c.vis_heads <= 0 || c.vis_hidden != c.vis_heads * 64) return bad("vision head dim must be 64");
    if (c.vis_patch <= 0 || c.vis_image % c.vis_patch) return bad("image size must be a multiple of the patch size");
    if (c.vis_hidden % 64 || c.vis_mlp % 64 || c.d_model % 64 || c.d_ff % 64) return bad("hidden sizes must be multiples of 64");
    if (c.vocab % 8) return bad("vocab must be a multiple of 8");
    if (c.vis_layers_run < 1 || c.enc_layers < 1 || c.dec_layers < 1) return bad("layer counts must be positive");
    const int g = c.vis_image / c.vis_patch;
    h->P = g * g;
    h->Sv = h->P + 1;
    h->kpatch = 3 * c.vis_patch * c.vis_patch;
    h->kpad = (h->kpatch + 63) / 64 * 64;
    h->I = c.n_heads * c.d_kv;
    h->lut_len = c.rel_max_distance + 1;
    for (int n = 0; n < h->lut_len; ++n) {
        // index = |relative position|; bidirectional: the +nb/2 for rel>0 is added on the device
        h->h_lut_bidir.push_back(vqs_relpos_bucket(-n, 1, c.rel_buckets, c.rel_max_distance));
        h->h_lut_causal.push_back(vqs_relpos_bucket(-n, 0, c.rel_buckets, c.rel_max_distance));
    }
    h->gemm_variant = 3;   // persistent kernel, schedule chosen by shape (gemm.hip)
    return VQS_OK;
}

int vqs_set_option(vqs_handle* h, const char* name, int32_t value) {
    if (!h || !name) return VQS_ERR_INVALID;
    const std::string n(name);
    if (n == "cross_mode" && (value == 0 || value == 1)) h->cross_mode = value;
    else if (n == "splitk" && (value == 0 || value == 1)) h->splitk = value;
    else if (n == "fused_norm" && (value == 0 || value == 1)) h->fused_norm = value;
    else if (n == "norm_defer" && (value == 0 || value == 1)) h->norm_defer = value;
    else if (n == "dec_precise" && (value == 0 || value == 1)) h->dec_precise = value;
    else if (n == "vit_fp16" && (value == 0 || value == 1)) h->vit_fp16 = value;
    else if (n == "enc_fp16" && value >= 0 && value <= 3) h->enc_fp16 = value;      // 2 / 3: attention sub-block only / FFN input side only (A/B)
    else if (n == "proj_fp16" && (value == 0 || value == 1)) h->proj_fp16 = value;
    else if (n == "proj_fs_shift" && value >= 0 && value <= 60) h->proj_fs_shift = value;
    else if (n == "proj_mid_shift" && value >= 0 && value <= 60) h->proj_mid_shift = value;
    else if (n == "dec_fp16" && (value == 0 || value == 1)) h->dec_fp16 = value;
    else if (n == "stream_gemm" && (value == 0 || value == 1)) h->stream_gemm = value;
    else if (n == "gemm_variant" && (value == 0 || value == 2 || value == 3 || value == 5 || value == 11)) h->gemm_variant = value;
    else if (n.rfind("l2_touch:", 0) == 0 || n.rfind("nt_store:", 0) == 0 || n.rfind("tile_order:", 0) == 0) {
        // per weight shape [N, K], for the big launches of a pass; 0 removes the entry = the library's choice.  All three are
        // bitwise-neutral cache-policy knobs:
        //   "l2_touch:<N>x<K>"   1: A-panel L2 prefetch in the lock-step GEMM, 2: off
        //   "nt_store:<N>x<K>"   1: non-temporal result stores, 2: plain stores
        //   "tile_order:<N>x<K>" gm | ns << 8
        const bool order = n[0] == 't';
        const size_t colon = n.find(':');
        int N = 0, K = 0;
        const int gm = value & 0xff, ns = (value >> 8) & 0xff;
        const bool value_ok = order ? (value >= 0 && (value >> 16) == 0 && (value == 0 || (gm >= 1 && gm <= 64 && ns <= 8))) : (value >= 0 && value <= 2);
        if (std::sscanf(n.c_str() + colon + 1, "%dx%d", &N, &K) != 2 || N <= 0 || K <= 0 || !value_ok)
            return fail(h, VQS_ERR_INVALID, "set_option: bad " + n.substr(0, colon) + ": " + n + "=" + std::to_string(value));
        if (order) {
            auto& v = h->tile_orders;
            for (size_t i = 0; i < v.size(); ++i)
                if (v[i].N == N && v[i].K == K) { v.erase(v.begin() + i); break; }
            if (value != 0) v.push_back(vqs_handle::TileOrder{N, K, gm, ns});
        } else {
            auto& v = n[0] == 'l' ? h->l2_touches : h->nt_stores;
            for (size_t i = 0; i < v.size(); ++i)
                if (v[i].N == N && v[i].K == K) { v.erase(v.begin() + i); break; }
            if (value != 0) v.push_back(vqs_handle::NtStore{N, K, value});
        }
    }
    else return fail(h, VQS_ERR_INVALID, "set_option: unknown option or value: " + n + "=" + std::to_string(value));
    return VQS_OK;
}

int vqs_get_option(const vqs_handle* h, const char* name, int32_t* value) {
    if (!h || !name || !value) return VQS_ERR_INVALID;
    const std::string n(name);
    if (n == "cross_mode") *value = h->cross_mode;
    else if (n == "splitk") *value = h->splitk;
    else if (n == "fused_norm") *value = h->fused_norm;
    else if (n == "norm_defer") *value = h->norm_defer;
    else if (n == "dec_precise") *value = h->dec_precise;
    else if (n == "vit_fp16") *value = h->vit_fp16;
    else if (n == "enc_fp16") *value = h->enc_fp16;
    else if (n == "proj_fp16") *value = h->proj_fp16;
    else if (n == "proj_fs_shift") *value = h->proj_fs_shift;
    else if (n == "proj_mid_shift") *value = h->proj_mid_shift;
    else if (n == "dec_fp16") *value = h->dec_fp16;
    else if (n == "stream_gemm") *value = h->stream_gemm;
    else if (n == "gemm_variant") *value = h->gemm_variant;
    else return VQS_ERR_INVALID;
    return VQS_OK;
}

void vqs_destroy(vqs_handle* h) { delete h; }      // ~GemmProfile destroys the profile's events

const char* vqs_last_error(const vqs_handle* h) { return h ? h->err.c_str() : "null handle"; }

size_t vqs_packed_bytes(const vqs_handle* h) { return h ? packed_layout(h).total : 0; }

int vqs_bind_weights(vqs_handle* h, const vqs_weight_desc* weights, int32_t n, void* d_packed, size_t packed_bytes,
                     void* stream) {
    if (!h || !weights || n <= 0 || !d_packed) return fail(h, VQS_ERR_INVALID, "bind_weights: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    const vqs_config& c = h->c;
    const PackedLayout pl = packed_layout(h);
    if (packed_bytes < pl.total) return fail(h, VQS_ERR_WORKSPACE, "bind_weights: packed buffer too small");
    h->bound = false;
    VQS_RUN(vqs::set_weights(h, weights, n));
    char* pk = (char*)d_packed;
    auto at = [&](size_t off) { return reinterpret_cast<bf16_t*>(pk + off); };
    const int hid = c.vis_hidden, D = c.d_model, I = h->I, F = c.d_ff;

    // conv kernel [hid, 3*p*p] -> [hid, kpad] zero padded (K must be a multiple of 64)
    {
        VQS_W(pw, "vision.embeddings.patch_embedding.weight", (int64_t)hid * h->kpatch);
        VQS_HIP(h, vqs::launch_copy_rows(pw, at(pl.patch_w), hid, h->kpatch, h->kpatch, h->kpad, 0, st), "pack patch");
        h->patch_w = at(pl.patch_w);
    }
    h->vit.qkv_w.clear(); h->vit.qkv_b.clear();
    for (int i = 0; i < c.vis_layers_run; ++i) {
        const std::string p = "vision.encoder.layers." + std::to_string(i) + ".self_attn.";
        const char* nm[3] = {"q_proj", "k_proj", "v_proj"};
        for (int j = 0; j < 3; ++j) {
            VQS_W(ww, p + nm[j] + ".weight", (int64_t)hid * hid);
            VQS_W(bb, p + nm[j] + ".bias", hid);
            VQS_HIP(h, vqs::launch_copy_rows(ww, at(pl.vit_qkv_w[i]), hid, hid, hid, hid, j * hid, st), "pack vit qkv");
            VQS_HIP(h, vqs::launch_copy_rows(bb, at(pl.vit_qkv_b[i]), 1, hid, hid, hid, j, st), "pack vit qkv bias");
        }
        h->vit.qkv_w.push_back(at(pl.vit_qkv_w[i]));
        h->vit.qkv_b.push_back(at(pl.vit_qkv_b[i]));
    }
    // fp16 copies of the tower's and the projector's linear weights (option vit_fp16): bf16 -> fp16 is exact for 2^-14 <= |w| < 65 520
    h->vit.qkv_w16.clear(); h->vit.out_w16.clear(); h->vit.fc1_w16.clear(); h->vit.fc2_w16.clear();
    for (int i = 0; i < c.vis_layers_run; ++i) {
        const std::string p = "vision.encoder.layers." + std::to_string(i) + ".";
        const size_t mlp = (size_t)c.vis_mlp;
        VQS_W(ow, p + "self_attn.out_proj.weight", (int64_t)hid * hid);
        VQS_W(f1w, p + "mlp.fc1.weight", (int64_t)mlp * hid);
        VQS_W(f2w, p + "mlp.fc2.weight", (int64_t)hid * mlp);
        VQS_HIP(h, vqs::launch_cast16(at(pl.vit_qkv_w[i]), at(pl.vit_qkv_w16[i]), (size_t)3 * hid * hid, true, st), "fp16 vit qkv");
        VQS_HIP(h, vqs::launch_cast16(ow, at(pl.vit_out_w16[i]), (size_t)hid * hid, true, st), "fp16 vit out_proj");
        VQS_HIP(h, vqs::launch_cast16(f1w, at(pl.vit_fc1_w16[i]), mlp * hid, true, st), "fp16 vit fc1");
        VQS_HIP(h, vqs::launch_cast16(f2w, at(pl.vit_fc2_w16[i]), mlp * hid, true, st), "fp16 vit fc2");
        h->vit.qkv_w16.push_back(at(pl.vit_qkv_w16[i]));
        h->vit.out_w16.push_back(at(pl.vit_out_w16[i]));
        h->vit.fc1_w16.push_back(at(pl.vit_fc1_w16[i]));
        h->vit.fc2_w16.push_back(at(pl.vit_fc2_w16[i]));
    }
    {
        VQS_W(p0w, "mm_projector.0.weight", (int64_t)D * hid);
        VQS_W(p2w, "mm_projector.2.weight", (int64_t)D * D);
        VQS_HIP(h, vqs::launch_cast16(p0w, at(pl.proj0_w16), (size_t)D * hid, true, st), "fp16 mm_projector.0");
        VQS_HIP(h, vqs::launch_cast16(p2w, at(pl.proj2_w16), (size_t)D * D, true, st), "fp16 mm_projector.2");
        h->proj0_w16 = at(pl.proj0_w16);
        h->proj2_w16 = at(pl.proj2_w16);
    }
    auto pack_qkv = [&](const std::string& prefix, bf16_t* dst, int first, int count) -> int {
        const char* nm[3] = {"q", "k", "v"};
        for (int j = 0; j < count; ++j) {
            VQS_W(ww, prefix + nm[first + j] + ".weight", (int64_t)I * D);
            VQS_HIP(h, vqs::launch_copy_rows(ww, dst, I, D, D, D, j * I, st), "pack t5 qkv");
        }
        return VQS_OK;
    };
    auto pack_wi = [&](const std::string& prefix, bf16_t* dst) -> int {
        VQS_W(w0, prefix + "wi_0.weight", (int64_t)F * D);
        VQS_W(w1, prefix + "wi_1.weight", (int64_t)F * D);
        VQS_HIP(h, vqs::launch_interleave_gate(w0, w1, dst, F, D, st), "pack wi");
        return VQS_OK;
    };
    h->enc_qkv16.clear(); h->enc_o16.clear(); h->enc_wi16.clear(); h->dec_ckT16.clear();
    h->enc_qkv.clear(); h->enc_wi.clear(); h->dec_qkv.clear(); h->dec_ckv.clear(); h->dec_wi.clear(); h->dec_ckT.clear();
    for (int i = 0; i < c.enc_layers; ++i) {
        const std::string p = "encoder.block." + std::to_string(i) + ".";
        VQS_RUN(pack_qkv(p + "layer.0.SelfAttention.", at(pl.enc_qkv[i]), 0, 3));
        VQS_RUN(pack_wi(p + "layer.1.DenseReluDense.", at(pl.enc_wi[i])));
        h->enc_qkv.push_back(at(pl.enc_qkv[i]));
        h->enc_wi.push_back(at(pl.enc_wi[i]));
        // fp16 copies for option enc_fp16 (of the PACKED q|k|v and interleaved wi_0|wi_1, and of o): exact for 2^-14 <= |w| < 65 520
        VQS_W(ow, p + "layer.0.SelfAttention.o.weight", (int64_t)D * I);
        VQS_HIP(h, vqs::launch_cast16(at(pl.enc_qkv[i]), at(pl.enc_qkv16[i]), (size_t)3 * I * D, true, st), "fp16 enc qkv");
        VQS_HIP(h, vqs::launch_cast16(ow, at(pl.enc_o16[i]), (size_t)D * I, true, st), "fp16 enc o");
        VQS_HIP(h, vqs::launch_cast16(at(pl.enc_wi[i]), at(pl.enc_wi16[i]), (size_t)2 * F * D, true, st), "fp16 enc wi");
        h->enc_qkv16.push_back(at(pl.enc_qkv16[i]));
        h->enc_o16.push_back(at(pl.enc_o16[i]));
        h->enc_wi16.push_back(at(pl.enc_wi16[i]));
    }
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string p = "decoder.block." + std::to_string(i) + ".";
        VQS_RUN(pack_qkv(p + "layer.0.SelfAttention.", at(pl.dec_qkv[i]), 0, 3));
        VQS_RUN(pack_qkv(p + "layer.1.EncDecAttention.", at(pl.dec_ckv[i]), 1, 2));
        VQS_RUN(pack_wi(p + "layer.2.DenseReluDense.", at(pl.dec_wi[i])));
        h->dec_qkv.push_back(at(pl.dec_qkv[i]));
        h->dec_ckv.push_back(at(pl.dec_ckv[i]));
        {   // Wk^T [D, I] for the reassociated cross-attention: q'_h = q_h . Wk_h needs Wk_h^T K-contiguous
            VQS_W(wk, p + "layer.1.EncDecAttention.k.weight", (int64_t)I * D);
            VQS_HIP(h, vqs::launch_transpose(wk, at(pl.dec_ckT[i]), I, D, st), "pack cross k^T");
            h->dec_ckT.push_back(at(pl.dec_ckT[i]));
            VQS_HIP(h, vqs::launch_cast16(at(pl.dec_ckT[i]), at(pl.dec_ckT16[i]), (size_t)I * D, true, st), "fp16 cross k^T");
            h->dec_ckT16.push_back(at(pl.dec_ckT16[i]));
        }
        h->dec_wi.push_back(at(pl.dec_wi[i]));
    }
    VQS_HIP(h, hipMemcpyAsync(pk + pl.lut_bidir, h->h_lut_bidir.data(), h->lut_len * sizeof(int), hipMemcpyHostToDevice, st),
           "upload bucket lut");
    VQS_HIP(h, hipMemcpyAsync(pk + pl.lut_causal, h->h_lut_causal.data(), h->lut_len * sizeof(int), hipMemcpyHostToDevice, st),
           "upload bucket lut");
    h->lut_bidir = reinterpret_cast<const int*>(pk + pl.lut_bidir);
    h->lut_causal = reinterpret_cast<const int*>(pk + pl.lut_causal);
    h->bound = true;
    return VQS_OK;
}

size_t vqs_encode_workspace_bytes(const vqs_handle* h, int32_t n_img) {
    if (!h || n_img <= 0) return 0;
    return carve_encode(h, nullptr, n_img).total;
}

int vqs_encode_images(vqs_handle* h, const void* d_pixels, int32_t N, void* d_feats, void* d_ws, size_t ws_bytes,
                      void* stream) {
    if (!h) return VQS_ERR_INVALID;
    if (!h->bound) return fail(h, VQS_ERR_STATE, "encode_images: weights not bound");
    if (!d_pixels || !d_feats || !d_ws || N <= 0) return fail(h, VQS_ERR_INVALID, "encode_images: bad arguments");
    const vqs_config& c = h->c;
    const EncodeWs w = carve_encode(h, (char*)d_ws, N);
    if (ws_bytes < w.total) return fail(h, VQS_ERR_WORKSPACE, "encode_images: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int hid = c.vis_hidden, P = h->P, Sv = h->Sv, mlp = c.vis_mlp, D = c.d_model;
    const int NP = N * P, NS = N * Sv;
    h->taps.outer = N;
    // option vit_fp16: every 16-bit tensor of the tower and the projector (norm outputs, q / k / v, attention output, deltas, FFN
    // product, selected features, projector hidden) is IEEE fp16 and every linear reads the fp16 copy of its weight; the fp32 residual
    // stream, the norm statistics, the softmax and all accumulation are what they were.  The patch embedding (fp32 result) keeps its
    // bf16 operands.
    const bool f16 = h->vit_fp16 != 0;
    if (f16 && h->gemm_variant != 3)
        return fail(h, VQS_ERR_STATE, "encode_images: the fp16 vision tower (option vit_fp16, default 1) needs gemm_variant 3 -- its linears exist in the quad form only; set vit_fp16=0 to A/B other GEMM forms");

    VQS_W(cls, "vision.embeddings.class_embedding", hid);
    VQS_W(pos, "vision.embeddings.position_embedding.weight", (int64_t)Sv * hid);
    VQS_W(pre_w, "vision.pre_layrnorm.weight", hid);
    VQS_W(pre_b, "vision.pre_layrnorm.bias", hid);

    VQS_HIP(h, vqs::launch_im2col((const bf16_t*)d_pixels, w.im2col, N, c.vis_image, c.vis_patch, h->kpad, st), "im2col");
    {
        GemmCall g{w.im2col, h->patch_w, w.patch_out};
        g.M = NP; g.N = hid; g.K = h->kpad; g.lda = h->kpad; g.ldw = h->kpad; g.ldc = hid; g.epi = vqs::EPI_F32;
        VQS_RUN(run_gemm(h, g, st, "patch_embed"));
    }
    VQS_HIP(h, vqs::launch_vit_assemble(w.patch_out, cls, pos, w.pre, N, P, hid, st), "vit_assemble");
    VQS_HIP(h, vqs::launch_layernorm(w.pre, nullptr, pre_w, pre_b, w.hidden, 1, NS, hid, c.vis_ln_eps, st), "pre_layrnorm");
    VQS_TAP("vit", -1, "patch_out", w.patch_out, (size_t)NP * hid);
    VQS_TAP("vit", -1, "h0", w.hidden, (size_t)NS * hid);

    // The block loop (residual stream protocol, deferred stores: vqs_blocks.h) is shared with the CLIPScore row's towers.
    const bf16_t* pend = nullptr;
    {
        VitBlocksCtx cx{h, st};
        vqs::ClipBlockShape bs{N, Sv, hid, c.vis_heads, mlp, c.vis_layers_run, c.vis_ln_eps, f16, h->norm_defer != 0, "vit"};
        vqs::ClipBlockBufs bb{w.hidden, w.delta, w.delta2, w.xn, w.q, w.k, w.v, w.attn, w.mid};
        VQS_RUN(vqs::run_clip_blocks(cx, bs, bb, st, &pend));
    }
    // hidden_states[-2][:, 1:] = hidden + pending fc2 output, CLS dropped, cast to the projector's operand type
    const bool p16 = f16 && h->proj_fp16 != 0;       // operand type of the selected features and the projector
    const bool psc = p16 && (h->proj_fs_shift != 0 || h->proj_mid_shift != 0);      // scaled forms only where the proof asked for a scale
    const float s_fs = psc ? std::ldexp(1.0f, -h->proj_fs_shift) : 1.0f, s_mid = psc ? std::ldexp(1.0f, -h->proj_mid_shift) : 1.0f;
    VQS_HIP(h, vqs::launch_drop_cls_cast(w.hidden, pend, w.feat_in, N, P, hid, st, f16, p16 ? 1 : 0, s_fs), "feature select");
    VQS_TAP("vit", -1, "feat_in", w.feat_in, (size_t)NP * hid);
    VQS_W(p0w, "mm_projector.0.weight", (int64_t)D * hid);
    VQS_W(p0b, "mm_projector.0.bias", D);
    VQS_W(p2w, "mm_projector.2.weight", (int64_t)D * D);
    VQS_W(p2b, "mm_projector.2.bias", D);
    {
        GemmCall g{w.feat_in, p16 ? h->proj0_w16 : p0w, w.pmid};
        g.bias = p0b;
        g.f16 = psc ? 3 : (p16 ? 1 : 0);
        g.acc_scale = 1.0f / s_fs; g.out_scale = s_mid;
        g.M = NP; g.N = D; g.K = hid; g.lda = hid; g.ldw = hid; g.ldc = D; g.epi = vqs::EPI_BF16_GELU;
        VQS_RUN(run_gemm(h, g, st, "mm_projector.0"));
        VQS_TAP("vit", -1, "pmid", w.pmid, (size_t)NP * D);
    }
    {
        // the image features are a bf16 tensor of the C ABI (vqs_score reads them as such).  Round 4 wrote the fp16 result and cast it
        // (two roundings, one more pass over 2.4 GB); the fp16-operand / bf16-result instantiation of the quad kernel (round 5,
        // gemm_f16b_quad) rounds the fp32 accumulator to bf16 ONCE and writes the feature tensor itself
        GemmCall g{w.pmid, p16 ? h->proj2_w16 : p2w, d_feats};
        g.bias = p2b;
        g.f16 = psc ? 4 : (p16 ? 2 : 0);
        g.acc_scale = 1.0f / s_mid;
        g.M = NP; g.N = D; g.K = D; g.lda = D; g.ldw = D; g.ldc = D; g.epi = vqs::EPI_BF16;
        VQS_RUN(run_gemm(h, g, st, "mm_projector.2"));
    }
    return VQS_OK;
}

size_t vqs_score_workspace_bytes(const vqs_handle* h, int32_t B, int32_t L, int32_t T) {
    if (!h || B <= 0 || L < 1 || T <= 0) return 0;
    return carve_score(h, nullptr, B, L, T).total;
}

// Encoder half of the scoring pass: prompt scan, bias table, embed + splice, 24 encoder blocks, final norm
// (+ the transposed copy the reassociated cross-attention reads).  Leaves enc_out / enc_outT / enc_len in the workspace.
// e_out_f16: the encoder's output (enc_out / enc_outT) leaves as IEEE fp16 instead of bf16 -- what the precise decoder of option dec_fp16 reads
static int encoder_pass(vqs_handle* h, const ScoreWs& w, const void* d_feats, const int32_t* d_img_index,
                        const int32_t* d_input_ids, int B, int L, hipStream_t st, bool e_out_f16 = false) {
    const int T = 1;
    const vqs_config& c = h->c;
    const int P = h->P, S = L - 1 + P;
    const int D = c.d_model, I = h->I, F = c.d_ff, H = c.n_heads, V = c.vocab;
    const int M = B * S, MT = B * T;
    (void)P; (void)M; (void)MT; (void)F; (void)I; (void)V;
    h->taps.outer = B;
    VQS_W(shared, "shared.weight", (int64_t)V * D);
    VQS_W(enc_rel, "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", (int64_t)c.rel_buckets * H);

    VQS_HIP(h, hipMemsetAsync(w.flags, 0, 4 * sizeof(int), st), "memset flags");
    VQS_HIP(h, vqs::launch_prompt_scan(d_input_ids, B, L, P, w.sent_pos, w.enc_len, w.flags, st), "prompt_scan");
    VQS_HIP(h, vqs::launch_relpos_table(enc_rel, h->lut_bidir, h->lut_causal, h->lut_len, c.rel_buckets, w.enc_table, H, S,
                                       nullptr, 1, st), "encoder bias table");
    VQS_HIP(h, vqs::launch_embed_splice(d_input_ids, w.sent_pos, w.enc_len, d_img_index, shared, (const bf16_t*)d_feats,
                                       w.hidden, B, L, P, D, V, st), "embed_splice");
    VQS_TAP("enc", -1, "emb", w.hidden, (size_t)M * D);

    // ---------------- encoder (same pending-delta protocol as the vision tower)
    // Fused residual + RMSNorm (VQS_FUSED_NORM=1, off by default): the o / wo GEMM epilogue updates the fp32 stream in
    // place, writes the NEXT norm's operand x*ln_w (without the per-row 1/rms) and per-tile partial row sums of squares;
    // the consuming qkv / wi GEMM scales its accumulator rows by 1/rms.  Bit-exact repeatable and parity-tested, but the
    // read-modify-write epilogue costs the producer GEMMs +0.55 ms per launch against 0.64 ms for the norm kernel it
    // removes (+1 % end to end, and it lowers the GEMM's own roofline fraction): kept as a lab path.
    const bool fused = h->fused_norm != 0 && (h->gemm_variant == 3 || h->gemm_variant == 11 || h->gemm_variant == 5);   // the fused epilogue's launches are not quad-eligible: they run the 8-wave forms
    const int parts = (D + 255) / 256;
    bool scaled = false;          // w.xn holds an un-normalised operand whose row sums are in w.rowss
    const bf16_t* pend = nullptr;
    const bf16_t* pend_attn = nullptr;   // deferred store (see the vision tower): the attention delta the stream has not absorbed yet
    const bool defer = h->norm_defer != 0 && !fused;
    // option enc_fp16: the attention side on IEEE fp16 tensors (see the option's comment in vqs_handle): xn (both norms), q / k / v, P, the
    // attention output are fp16 and q|k|v, o, wi read their fp16 weight copies; o's and wo's results (the deltas) and the gated product stay
    // bf16, wo runs as before.  The final norm's output (the tensor the decoder reads) stays bf16.
    // Values 2 / 3 (round 6, the per-call-site A/B of VERDICT r5 item 4): only the attention sub-block (norm0 output, q / k / v, P, attention
    // output; q|k|v and o weights) / only the FFN's input side (norm1 output; wi weights) on fp16, the other on bf16.
    const bool e16 = h->enc_fp16 != 0;
    const bool e16a = h->enc_fp16 == 1 || h->enc_fp16 == 2, e16f = h->enc_fp16 == 1 || h->enc_fp16 == 3;
    if (e16 && (h->gemm_variant != 3 || fused))
        return fail(h, VQS_ERR_STATE, "score: the fp16 encoder attention side (option enc_fp16, default 1) needs gemm_variant 3 and fused_norm 0 -- its linears "
                                      "exist in the quad form only; set enc_fp16=0 to A/B other GEMM forms");
    auto consume = [&](GemmCall& g) {
        if (scaled) {
            g.rowss_in = w.rs; g.rowss_parts = 0;
        }
    };
    auto produce = [&](GemmCall& g, const bf16_t* next_ln) {
        g.epi = vqs::EPI_RESID_RMS; g.C = w.xn; g.ldc = D; g.hres = w.hidden; g.ldh = D; g.lnw = next_ln; g.rowss_out = w.rowss;
    };
    for (int i = 0; i < c.enc_layers; ++i) {
        const std::string p = "encoder.block." + std::to_string(i) + ".";
        VQS_W(ln0, p + "layer.0.layer_norm.weight", D);
        VQS_W(ow, p + "layer.0.SelfAttention.o.weight", (int64_t)D * I);
        VQS_W(ln1, p + "layer.1.layer_norm.weight", D);
        VQS_W(wo, p + "layer.1.DenseReluDense.wo.weight", (int64_t)D * F);
        if (!scaled) {
            if (pend_attn)
                VQS_HIP(h, vqs::launch_rmsnorm(w.hidden, pend_attn, ln0, w.xn, M, D, c.t5_ln_eps, st, pend, true, 0, e16a), "enc rmsnorm0");
            else
                VQS_HIP(h, vqs::launch_rmsnorm(w.hidden, pend, ln0, w.xn, M, D, c.t5_ln_eps, st, nullptr, true, 0, e16a), "enc rmsnorm0");
            pend = nullptr;
            pend_attn = nullptr;
        }
        VQS_TAP("enc", i, "xn0", w.xn, (size_t)M * D);
        {
            GemmCall g{w.xn, e16a ? h->enc_qkv16[i] : h->enc_qkv[i], nullptr};
            g.M = M; g.N = 3 * I; g.K = D; g.lda = D; g.ldw = D; g.ldc = 0; g.epi = vqs::EPI_HEADS;
            g.S = S; g.H = H; g.inner = I;
            g.heads[0] = w.q; g.heads[1] = w.k; g.heads[2] = w.v;
            g.f16 = e16a ? 1 : 0;
            consume(g);
            VQS_RUN(run_gemm(h, g, st, "enc qkv"));
        }
        {
            vqs::AttnParams a{w.q, w.k, w.v, w.attn, w.enc_table, w.enc_len, B, H, S, 1.0f};
            a.f16 = e16a ? 1 : 0;
            VQS_TAP("enc", i, "q", w.q, (size_t)M * I);
            VQS_TAP("enc", i, "k", w.k, (size_t)M * I);
            VQS_TAP("enc", i, "v", w.v, (size_t)M * I);
            VQS_HIP(h, vqs::launch_attention(a, st), "enc attention");
            VQS_TAP("enc", i, "attn", w.attn, (size_t)M * I);
        }
        {
            GemmCall g{w.attn, e16a ? h->enc_o16[i] : ow, w.delta};
            g.M = M; g.N = D; g.K = I; g.lda = I; g.ldw = I; g.ldc = D; g.epi = vqs::EPI_BF16;
            g.f16 = e16a ? 2 : 0;                // fp16 operands, bf16 delta
            if (fused) produce(g, ln1);
            VQS_RUN(run_gemm(h, g, st, "enc o"));
            if (!fused) VQS_TAP("enc", i, "d_attn", w.delta, (size_t)M * D);
            if (fused) VQS_HIP(h, vqs::launch_rowss_to_rs(w.rowss, parts, M, 1.0f / (float)D, c.t5_ln_eps, w.rs, st), "row 1/rms");
        }
        if (fused) {
            scaled = true;
        } else {
            VQS_HIP(h, vqs::launch_rmsnorm(w.hidden, w.delta, ln1, w.xn, M, D, c.t5_ln_eps, st, nullptr, !defer, 0, e16f), "enc rmsnorm1");
            if (defer) pend_attn = w.delta;
            scaled = false;
            VQS_TAP("enc", i, "xn1", w.xn, (size_t)M * D);
        }
        {
            GemmCall g{w.xn, e16f ? h->enc_wi16[i] : h->enc_wi[i], w.ff};
            g.M = M; g.N = 2 * F; g.K = D; g.lda = D; g.ldw = D; g.ldc = F; g.epi = vqs::EPI_GATED;
            g.f16 = e16f ? 2 : 0;                // fp16 operands, bf16 gated product
            consume(g);
            VQS_RUN(run_gemm(h, g, st, "enc wi"));
            VQS_TAP("enc", i, "ff", w.ff, (size_t)M * F);
        }
        {
            bf16_t* dst = defer ? w.delta2 : w.delta;
            GemmCall g{w.ff, wo, dst};
            g.M = M; g.N = D; g.K = F; g.lda = F; g.ldw = F; g.ldc = D; g.epi = vqs::EPI_BF16;
            if (fused && i + 1 < c.enc_layers) {
                VQS_W(ln0_next, "encoder.block." + std::to_string(i + 1) + ".layer.0.layer_norm.weight", D);
                produce(g, ln0_next);
                VQS_RUN(run_gemm(h, g, st, "enc wo"));
                VQS_HIP(h, vqs::launch_rowss_to_rs(w.rowss, parts, M, 1.0f / (float)D, c.t5_ln_eps, w.rs, st), "row 1/rms");
                scaled = true;
                pend = nullptr;
            } else {
                VQS_RUN(run_gemm(h, g, st, "enc wo"));
                VQS_TAP("enc", i, "d_ff", dst, (size_t)M * D);
                scaled = false;
                pend = dst;
            }
        }
    }
    {
        VQS_W(fin, "encoder.final_layer_norm.weight", D);
        if (pend_attn)
            VQS_HIP(h, vqs::launch_rmsnorm(w.hidden, pend_attn, fin, w.enc_out, M, D, c.t5_ln_eps, st, pend, true, 0, e_out_f16), "enc final norm");
        else
            VQS_HIP(h, vqs::launch_rmsnorm(w.hidden, pend, fin, w.enc_out, M, D, c.t5_ln_eps, st, nullptr, true, 0, e_out_f16), "enc final norm");
        if (h->cross_mode != 0)
            VQS_HIP(h, vqs::launch_transpose_pad(w.enc_out, w.enc_outT, B, S, D, w.S_pad, st), "enc_out transpose");
    }

    return VQS_OK;
}

// Split-K factor of a decoder nn.Linear: K-slices run as batch entries of the persistent kernel (operand pointers advance by
// K/s columns, fp32 partial tiles go to scratch), one pass then sums the slices in a fixed order -- deterministic, no atomics.
// s = the largest divisor of K/64 in 2..16 with tiles * s <= 256 CUs and >= 4 K-tiles per slice, where `tiles` counts `m_tiles`
// M-tiles per N-tile: a function of the WEIGHT's shape only.  The slicing fixes the order in which a row's fp32 partial sums
// are added, so it must not depend on how many rows the launch has -- a pair's score in a 256-pair batch has to be bit-equal to
// its score in a 4-pair batch (reference contract: independent cells, score.py:104-106).  Round 2 derived s from the launch's tile
// count (bits depended on ceil(MT / 256)); round 3 kept an MT <= 1024 cap and a scratch-size fallback that were M-dependent
// switches of the same kind: both are gone -- the partials have their own workspace region sized by the architecture.
static int dec_slices(const vqs_handle* h, int N, int K, int m_tiles) {
    const int tiles = m_tiles * ((N + 255) / 256);
    const int nt = K / 64;
    int sk = 1;
    if (h->splitk && (K % 64) == 0 && (N % 8) == 0)
        for (int s2 = 2; s2 <= 16; ++s2)
            if (nt % s2 == 0 && tiles * s2 <= 256 && nt / s2 >= 4) sk = s2;
    return sk;
}

// A decoder nn.Linear of the bf16 decoder (rounds 1-3; vqs_generate and option dec_precise=0): out[MT, N] (bf16) = A[MT, K] . W[N, K]^T.
// Two M-tiles are assumed for the slice count because that is the bench batch (MT = 512).
static int dec_linear(vqs_handle* h, const bf16_t* A, const bf16_t* W, bf16_t* out, int MT, int N, int K, float* scratch,
                      size_t scratch_bytes, hipStream_t st, const char* what) {
    const int sk = dec_slices(h, N, K, 2);
    if (sk > 1) {
        if ((size_t)sk * MT * N * sizeof(float) > scratch_bytes) return fail(h, VQS_ERR_WORKSPACE, std::string(what) + ": decoder scratch too small");
        GemmCall g{A, W, scratch};
        g.M = MT; g.N = N; g.K = K / sk; g.lda = K; g.ldw = K; g.ldc = N; g.epi = vqs::EPI_F32;
        g.batch = sk; g.sA = K / sk; g.sW = K / sk; g.sC = (long long)MT * N;
        VQS_RUN(run_gemm(h, g, st, what));
        VQS_HIP(h, vqs::launch_reduce_slices(scratch, sk, (size_t)MT * N, out, st), "split-K reduce");
        return VQS_OK;
    }
    GemmCall g{A, W, out};
    g.M = MT; g.N = N; g.K = K; g.lda = K; g.ldw = K; g.ldc = N; g.epi = vqs::EPI_BF16;
    return run_gemm(h, g, st, what);
}

// A decoder nn.Linear of the PRECISE decoder: A2 is a split-bf16 tensor, planes [2][MT][K]; the two planes run as 2*MT stacked
// rows of ONE GEMM over the same weights (and split-K slices as batch entries) into fp32 partials [slices][2*MT][N], which
// launch_sum_planes adds -- hi rows first, slices in index order -- into `out` in the form `mode` names (fp32 / split / gated split).
// The activation thus enters the bf16 MFMA with 16 significant bits and the result is never rounded to bf16.
static int dec_linear_split(vqs_handle* h, const bf16_t* A2, const bf16_t* W, int MT, int N, int K, float* scratch, size_t scratch_bytes,
                            int mode, void* out, int ld_out, long long out_plane, hipStream_t st, const char* what) {
    const int sk = dec_slices(h, N, K, 4);
    if ((size_t)sk * 2 * MT * N * sizeof(float) > scratch_bytes) return fail(h, VQS_ERR_WORKSPACE, std::string(what) + ": decoder scratch too small");
    GemmCall g{A2, W, scratch};
    g.M = 2 * MT; g.N = N; g.K = K / sk; g.lda = K; g.ldw = K; g.ldc = N; g.epi = vqs::EPI_F32;
    g.batch = sk; g.sA = K / sk; g.sW = K / sk; g.sC = (long long)2 * MT * N;
    VQS_RUN(run_gemm(h, g, st, what));
    VQS_HIP(h, vqs::launch_sum_planes(scratch, sk, (long long)2 * MT * N, MT, N, N, mode, out, ld_out, out_plane, st), "sum of stacked partials");
    return VQS_OK;
}

// Decoder half: T teacher-forced rows per pair over the encoder output already in the workspace -> fp32 logits
// [B*T, ldl].  d_labels[b*ld_labels + t] are the target ids (decoder input = shift_right, HF modeling_t5.py:618-637).
// pos0 / cached (vqs_generate): the T rows are decoder positions pos0 .. pos0+T-1 of an incremental decode; their self
// attention K/V rows are appended to w.kvcache and the queries attend to positions 0 .. pos0+T-1 of it (T = 1 per step).
static int decoder_pass(vqs_handle* h, const ScoreWs& w, const int32_t* d_labels, int ld_labels, int B, int L, int T,
                        hipStream_t st, int pos0 = 0, bool cached = false) {
    const vqs_config& c = h->c;
    const int P = h->P, S = L - 1 + P;
    const int D = c.d_model, I = h->I, F = c.d_ff, H = c.n_heads, V = c.vocab;
    const int M = B * S, MT = B * T;
    (void)P; (void)M; (void)MT; (void)F; (void)I; (void)V;
    h->taps.outer = B;
    // ---------------- decoder (teacher forced, T rows per pair)
    VQS_W(shared, "shared.weight", (int64_t)V * D);
    float* scratch = w.dscratch;
    const size_t scratch_bytes = w.dscratch_bytes;
    VQS_W(dec_rel, "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", (int64_t)c.rel_buckets * H);
    const int TB = cached ? w.Tc : T;                          // row length of the decoder bias table
    if (!cached || pos0 == 0)
        VQS_HIP(h, vqs::launch_relpos_table(dec_rel, h->lut_bidir, h->lut_causal, h->lut_len, c.rel_buckets, nullptr, H, S,
                                           w.dec_table, TB, st), "decoder bias table");
    VQS_HIP(h, vqs::launch_decoder_embed(d_labels, ld_labels, shared, w.dhid, B, T, D, V, st, pos0), "decoder embed");
    VQS_TAP("dec", -1, "emb", w.dhid, (size_t)MT * D);
    const bf16_t* dpend = nullptr;
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string p = "decoder.block." + std::to_string(i) + ".";
        VQS_W(ln0, p + "layer.0.layer_norm.weight", D);
        VQS_W(so, p + "layer.0.SelfAttention.o.weight", (int64_t)D * I);
        VQS_W(ln1, p + "layer.1.layer_norm.weight", D);
        VQS_W(cq, p + "layer.1.EncDecAttention.q.weight", (int64_t)I * D);
        VQS_W(co, p + "layer.1.EncDecAttention.o.weight", (int64_t)D * I);
        VQS_W(ln2, p + "layer.2.layer_norm.weight", D);
        VQS_W(wo, p + "layer.2.DenseReluDense.wo.weight", (int64_t)D * F);

        VQS_HIP(h, vqs::launch_rmsnorm(w.dhid, dpend, ln0, w.dxn, MT, D, c.t5_ln_eps, st), "dec rmsnorm0");
        dpend = nullptr;
        VQS_TAP("dec", i, "xn0", w.dxn, (size_t)MT * D);
        VQS_RUN(dec_linear(h, w.dxn, h->dec_qkv[i], w.dqkv, MT, 3 * I, D, scratch, scratch_bytes, st, "dec self qkv"));
        VQS_TAP("dec", i, "qkv", w.dqkv, (size_t)MT * 3 * I);
        if (cached) {
            // append this step's k | v rows (columns I .. 3I of dqkv) to layer i's cache at position pos0, then attend over
            // positions 0 .. pos0+T-1 of the cache
            bf16_t* cl = w.kvcache + (size_t)i * B * w.Tc * 2 * I;
            VQS_HIP(h, hipMemcpy2DAsync(cl + (size_t)pos0 * 2 * I, (size_t)w.Tc * 2 * I * sizeof(bf16_t), w.dqkv + I,
                                       (size_t)3 * I * sizeof(bf16_t), (size_t)2 * I * sizeof(bf16_t) * T, B,
                                       hipMemcpyDeviceToDevice, st), "kv cache append");
            vqs::DecAttnParams a{w.dqkv, cl, cl + I, w.dattn, w.dec_table, nullptr, B, H, T, pos0 + T, 3 * I, 2 * I, 0};
            a.kv_stride_b = (long long)w.Tc * 2 * I;
            a.qpos0 = pos0;
            a.bias_ld = TB;
            VQS_HIP(h, vqs::launch_decoder_attention(a, st), "dec self attention (cached)");
            VQS_TAP("dec", i, "sattn", w.dattn, (size_t)MT * I);
        } else {
            vqs::DecAttnParams a{w.dqkv, w.dqkv + I, w.dqkv + 2 * I, w.dattn, w.dec_table, nullptr, B, H, T, T, 3 * I, 3 * I, 0};
            VQS_HIP(h, vqs::launch_decoder_attention(a, st), "dec self attention");
            VQS_TAP("dec", i, "sattn", w.dattn, (size_t)MT * I);
        }
        VQS_RUN(dec_linear(h, w.dattn, so, w.ddelta, MT, D, I, scratch, scratch_bytes, st, "dec self o"));
        VQS_TAP("dec", i, "d_self", w.ddelta, (size_t)MT * D);
        VQS_HIP(h, vqs::launch_rmsnorm(w.dhid, w.ddelta, ln1, w.dxn, MT, D, c.t5_ln_eps, st), "dec rmsnorm1");
        VQS_TAP("dec", i, "xn1", w.dxn, (size_t)MT * D);
        VQS_RUN(dec_linear(h, w.dxn, cq, w.dq, MT, I, D, scratch, scratch_bytes, st, "dec cross q"));
        VQS_TAP("dec", i, "cq", w.dq, (size_t)MT * I);
        if (h->cross_mode == 0) {
            // direct form (what HF executes): K|V projection of the whole encoder output for this layer
            {
                GemmCall g{w.enc_out, h->dec_ckv[i], nullptr};
                g.M = M; g.N = 2 * I; g.K = D; g.lda = D; g.ldw = D; g.ldc = 0; g.epi = vqs::EPI_HEADS;
                g.S = S; g.H = H; g.inner = I;
                g.heads[0] = w.ck; g.heads[1] = w.cv; g.heads[2] = nullptr;
                VQS_RUN(run_gemm(h, g, st, "dec cross kv"));
            }
            vqs::DecAttnParams a{w.dq, w.ck, w.cv, w.dattn, nullptr, w.enc_len, B, H, T, S, I, 0, 1};
            VQS_HIP(h, vqs::launch_decoder_attention(a, st), "dec cross attention");
        } else {
            // Reassociated cross-attention.  With E = encoder output [S,D] and T (<=16) decoder rows per pair,
            //   scores_h = q_h (E Wk_h^T)^T = (q_h Wk_h) E^T          and       out_h = P_h (E Wv_h^T) = (P_h E) Wv_h^T,
            // so the per-layer [B*S, D] x [D, 2I] projection (4*S*D*I FLOPs per pair and layer, 98 % of the decoder)
            // becomes five small batched GEMMs over E itself (~30x fewer FLOPs); same function, fp32 accumulation.
            VQS_W(cv_w, p + "layer.1.EncDecAttention.v.weight", (int64_t)I * D);
            const int R = T * H;        // rows per pair, ordered (t, h)
            {   // q'[(b,t), h, :] = q[(b,t), h*64:(h+1)*64] . Wk_h            batched over heads
                GemmCall g{w.dq, h->dec_ckT[i], w.cqk};
                g.M = MT; g.N = D; g.K = 64; g.lda = I; g.ldw = I; g.ldc = H * D; g.epi = vqs::EPI_BF16;
                g.batch = H; g.sA = 64; g.sW = 64; g.sC = D;
                VQS_RUN(run_gemm(h, g, st, "cross q.Wk"));
                VQS_TAP("dec", i, "cqk", w.cqk, (size_t)MT * H * D);
            }
            {   // scores[b] [R, S] = q'[b] [R, D] . E[b]^T                      batched over pairs
                GemmCall g{w.cqk, w.enc_out, w.cscores};
                g.M = R; g.N = S; g.K = D; g.lda = D; g.ldw = D; g.ldc = w.S_pad; g.epi = vqs::EPI_F32;
                g.batch = B; g.sA = (long long)R * D; g.sW = (long long)S * D; g.sC = (long long)R * w.S_pad;
                VQS_RUN(run_gemm(h, g, st, "cross scores"));
                VQS_TAP("dec", i, "cscores", w.cscores, (size_t)MT * H * w.S_pad);
            }
            VQS_HIP(h, vqs::launch_masked_softmax(w.cscores, w.cprobs, w.enc_len, B, R, w.S_pad, st), "cross softmax");
            VQS_TAP("dec", i, "cprobs", w.cprobs, (size_t)MT * H * w.S_pad);
            {   // ctx[b] [R, D] = P[b] [R, S_pad] . E[b]  (E^T is K-contiguous)   batched over pairs
                GemmCall g{w.cprobs, w.enc_outT, w.cctx};
                g.M = R; g.N = D; g.K = w.S_pad; g.lda = w.S_pad; g.ldw = w.S_pad; g.ldc = D; g.epi = vqs::EPI_BF16;
                g.batch = B; g.sA = (long long)R * w.S_pad; g.sW = (long long)D * w.S_pad; g.sC = (long long)R * D;
                g.no_stream = 1;      // K = S_pad = 640: ten slabs per item -- the stream form's pipeline fill per item costs more than its
                                  // deeper ring gains (0.50 vs 0.41 ms per launch, profiles/r4_call4_*); the scores launch (K = D) streams
            VQS_RUN(run_gemm(h, g, st, "cross P.E"));
                VQS_TAP("dec", i, "cctx", w.cctx, (size_t)MT * H * D);
            }
            {   // out[(b,t), h*64:(h+1)*64] = ctx[(b,t), h, :] . Wv_h^T          batched over heads
                GemmCall g{w.cctx, cv_w, w.dattn};
                g.M = MT; g.N = 64; g.K = D; g.lda = H * D; g.ldw = D; g.ldc = I; g.epi = vqs::EPI_BF16;
                g.batch = H; g.sA = D; g.sW = (long long)64 * D; g.sC = 64;
                VQS_RUN(run_gemm(h, g, st, "cross ctx.Wv"));
            }
        }
        VQS_TAP("dec", i, "cattn", w.dattn, (size_t)MT * I);
        VQS_RUN(dec_linear(h, w.dattn, co, w.ddelta, MT, D, I, scratch, scratch_bytes, st, "dec cross o"));
        VQS_TAP("dec", i, "d_cross", w.ddelta, (size_t)MT * D);
        VQS_HIP(h, vqs::launch_rmsnorm(w.dhid, w.ddelta, ln2, w.dxn, MT, D, c.t5_ln_eps, st), "dec rmsnorm2");
        VQS_TAP("dec", i, "xn2", w.dxn, (size_t)MT * D);
        {
            GemmCall g{w.dxn, h->dec_wi[i], w.dff};
            g.M = MT; g.N = 2 * F; g.K = D; g.lda = D; g.ldw = D; g.ldc = F; g.epi = vqs::EPI_GATED;
            VQS_RUN(run_gemm(h, g, st, "dec wi"));
            VQS_TAP("dec", i, "ff", w.dff, (size_t)MT * F);
        }
        VQS_RUN(dec_linear(h, w.dff, wo, w.ddelta, MT, D, F, scratch, scratch_bytes, st, "dec wo"));
        VQS_TAP("dec", i, "d_ff", w.ddelta, (size_t)MT * D);
        dpend = w.ddelta;
    }
    {
        VQS_W(fin, "decoder.final_layer_norm.weight", D);
        VQS_W(head, "lm_head.weight", (int64_t)V * D);
        VQS_HIP(h, vqs::launch_rmsnorm(w.dhid, dpend, fin, w.dxn, MT, D, c.t5_ln_eps, st), "dec final norm");
        GemmCall g{w.dxn, head, w.logits};
        g.M = MT; g.N = V; g.K = D; g.lda = D; g.ldw = D; g.ldc = w.ldl; g.epi = vqs::EPI_F32;
        VQS_RUN(run_gemm(h, g, st, "lm_head"));
    }
    return VQS_OK;
}

// The scoring decoder of round 4 (option dec_precise, default 1): the same T teacher-forced rows per pair, but every activation the
// error attribution (profiles/r4_error_attribution.md) shows to matter is held with 16 significant bits or in fp32:
//   split-bf16 (planes hi | lo, consumed as 2*MT stacked rows of one GEMM): norm outputs, self-attention output, P.E context,
//     ctx.Wv output, gated FFN product, final norm output (the lm_head operand);
//   fp32, never rounded: q|k|v of the self-attention and the three sub-layer outputs added into the fp32 stream;
//   bf16 as before: the cross-attention SCORE path (q, q.Wk, probabilities: <= 2e-4 of |delta log P| together), which reads the hi
//     plane of the norm output -- bit for bit what rounds 1-3 computed there.
// Same function as decoder_pass (HF modeling_t5.py:404-509), same launch sequence; the reference rounds every one of these
// tensors to bf16 (mm_utils.py:228), so this is a deviation TOWARDS fp32 arithmetic, like the fp32 residual stream.
static int decoder_pass_precise(vqs_handle* h, const ScoreWs& w, const int32_t* d_labels, int ld_labels, int B, int L, int T, hipStream_t st) {
    const vqs_config& c = h->c;
    const bool x16 = h->dec_fp16 != 0;      // the encoder pass before this call wrote enc_out / enc_outT as fp16 tensors (vqs_score)
    const int P = h->P, S = L - 1 + P;
    const int D = c.d_model, I = h->I, F = c.d_ff, H = c.n_heads, V = c.vocab;
    const int MT = B * T;
    h->taps.outer = B;
    VQS_W(shared, "shared.weight", (int64_t)V * D);
    VQS_W(dec_rel, "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", (int64_t)c.rel_buckets * H);
    float* scratch = w.dscratch;
    const size_t sb = w.dscratch_bytes;
    const long long pD = (long long)MT * D, pI = (long long)MT * I, pF = (long long)MT * F, pC = (long long)MT * H * D;   // plane sizes
    VQS_HIP(h, vqs::launch_relpos_table(dec_rel, h->lut_bidir, h->lut_causal, h->lut_len, c.rel_buckets, nullptr, H, S, w.dec_table, T, st),
           "decoder bias table");
    VQS_HIP(h, vqs::launch_decoder_embed(d_labels, ld_labels, shared, w.dhid, B, T, D, V, st, 0), "decoder embed");
    VQS_TAP("dec", -1, "emb", w.dhid, (size_t)MT * D);
    const float* dpend = nullptr;
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string p = "decoder.block." + std::to_string(i) + ".";
        VQS_W(ln0, p + "layer.0.layer_norm.weight", D);
        VQS_W(so, p + "layer.0.SelfAttention.o.weight", (int64_t)D * I);
        VQS_W(ln1, p + "layer.1.layer_norm.weight", D);
        VQS_W(cq, p + "layer.1.EncDecAttention.q.weight", (int64_t)I * D);
        VQS_W(cv_w, p + "layer.1.EncDecAttention.v.weight", (int64_t)I * D);
        VQS_W(co, p + "layer.1.EncDecAttention.o.weight", (int64_t)D * I);
        VQS_W(ln2, p + "layer.2.layer_norm.weight", D);
        VQS_W(wo, p + "layer.2.DenseReluDense.wo.weight", (int64_t)D * F);

        // ---- causal self-attention
        VQS_HIP(h, vqs::launch_rmsnorm_split(w.dhid, dpend, ln0, w.dxn, pD, MT, D, c.t5_ln_eps, st), "dec rmsnorm0");
        dpend = nullptr;
        TAP2("dec", i, "xn0", w.dxn, pD);
        VQS_RUN(dec_linear_split(h, w.dxn, h->dec_qkv[i], MT, 3 * I, D, scratch, sb, vqs::SUM_F32, w.dqkv32, 3 * I, 0, st, "dec self qkv"));
        VQS_TAP("dec", i, "qkv", w.dqkv32, (size_t)MT * 3 * I);
        {
            vqs::DecAttnParams a{reinterpret_cast<const bf16_t*>(w.dqkv32), reinterpret_cast<const bf16_t*>(w.dqkv32 + I),
                                 reinterpret_cast<const bf16_t*>(w.dqkv32 + 2 * I), w.dattn, w.dec_table, nullptr, B, H, T, T, 3 * I, 3 * I, 0};
            a.precise = 1;
            a.out_plane = pI;
            VQS_HIP(h, vqs::launch_decoder_attention(a, st), "dec self attention");
        }
        TAP2("dec", i, "sattn", w.dattn, pI);
        VQS_RUN(dec_linear_split(h, w.dattn, so, MT, D, I, scratch, sb, vqs::SUM_F32, w.ddelta32, D, 0, st, "dec self o"));
        VQS_TAP("dec", i, "d_self", w.ddelta32, (size_t)MT * D);
        // ---- cross-attention (reassociated, vqs_api.cpp decoder_pass): score path in bf16 off the hi plane, value path precise
        VQS_HIP(h, vqs::launch_rmsnorm_split(w.dhid, w.ddelta32, ln1, w.dxn, pD, MT, D, c.t5_ln_eps, st), "dec rmsnorm1");
        TAP2("dec", i, "xn1", w.dxn, pD);
        // option dec_fp16 (x16): q from BOTH planes of the split norm output, rounded once to fp16; q.Wk, the probabilities and E are fp16 tensors
        if (x16)
            VQS_RUN(dec_linear_split(h, w.dxn, cq, MT, I, D, scratch, sb, vqs::SUM_F16, w.dq, I, 0, st, "dec cross q"));
        else
            VQS_RUN(dec_linear(h, w.dxn, cq, w.dq, MT, I, D, scratch, sb, st, "dec cross q"));
        VQS_TAP("dec", i, "cq", w.dq, (size_t)MT * I);
        const int R = T * H;        // rows per pair, ordered (t, h)
        {   // q'[(b,t), h, :] = q[(b,t), h*64:(h+1)*64] . Wk_h            batched over heads
            GemmCall g{w.dq, x16 ? h->dec_ckT16[i] : h->dec_ckT[i], w.cqk};
            g.M = MT; g.N = D; g.K = 64; g.lda = I; g.ldw = I; g.ldc = H * D; g.epi = vqs::EPI_BF16;
            g.batch = H; g.sA = 64; g.sW = 64; g.sC = D;
            g.f16 = x16 ? 1 : 0;
            VQS_RUN(run_gemm(h, g, st, "cross q.Wk"));
            VQS_TAP("dec", i, "cqk", w.cqk, (size_t)MT * H * D);
        }
        {   // scores[b] [R, S] = q'[b] [R, D] . E[b]^T                      batched over pairs
            GemmCall g{w.cqk, w.enc_out, w.cscores};
            g.M = R; g.N = S; g.K = D; g.lda = D; g.ldw = D; g.ldc = w.S_pad; g.epi = vqs::EPI_F32;
            g.batch = B; g.sA = (long long)R * D; g.sW = (long long)S * D; g.sC = (long long)R * w.S_pad;
            g.f16 = x16 ? 1 : 0;
            VQS_RUN(run_gemm(h, g, st, "cross scores"));
            VQS_TAP("dec", i, "cscores", w.cscores, (size_t)MT * H * w.S_pad);
        }
        VQS_HIP(h, vqs::launch_masked_softmax(w.cscores, w.cprobs, w.enc_len, B, R, w.S_pad, st, x16), "cross softmax");
        VQS_TAP("dec", i, "cprobs", w.cprobs, (size_t)MT * H * w.S_pad);
        {   // ctx[b] [R, D] = P[b] [R, S_pad] . E[b]   -> split-bf16: hi plane = the tensor of rounds 1-3, lo plane behind it
            GemmCall g{w.cprobs, w.enc_outT, w.cctx};
            g.M = R; g.N = D; g.K = w.S_pad; g.lda = w.S_pad; g.ldw = w.S_pad; g.ldc = D; g.epi = vqs::EPI_BF16;
            g.batch = B; g.sA = (long long)R * w.S_pad; g.sW = (long long)D * w.S_pad; g.sC = (long long)R * D;
            g.split_off = pC;
            g.f16 = x16 ? 2 : 0;          // fp16 operands (P, E^T), split-bf16 result
            g.no_stream = 1;      // K = S_pad = 640: ten slabs per item -- the stream form's pipeline fill per item costs more than its
                                  // deeper ring gains (0.50 vs 0.41 ms per launch, profiles/r4_call4_*); the scores launch (K = D) streams
            VQS_RUN(run_gemm(h, g, st, "cross P.E"));
            TAP2("dec", i, "cctx", w.cctx, pC);
        }
        {   // out[(b,t), h*64:(h+1)*64] = ctx[(b,t), h, :] . Wv_h^T          batched over heads; both planes as 2*MT stacked rows
            GemmCall g{w.cctx, cv_w, scratch};
            g.M = 2 * MT; g.N = 64; g.K = D; g.lda = H * D; g.ldw = D; g.ldc = I; g.epi = vqs::EPI_F32;
            g.batch = H; g.sA = D; g.sW = (long long)64 * D; g.sC = 64;
            if ((size_t)2 * MT * I * sizeof(float) > sb) return fail(h, VQS_ERR_WORKSPACE, "cross ctx.Wv: decoder scratch too small");
            VQS_RUN(run_gemm(h, g, st, "cross ctx.Wv"));
            VQS_HIP(h, vqs::launch_sum_planes(scratch, 1, 0, MT, I, I, vqs::SUM_SPLIT, w.dattn, I, pI, st), "cross ctx.Wv planes");
        }
        TAP2("dec", i, "cattn", w.dattn, pI);
        VQS_RUN(dec_linear_split(h, w.dattn, co, MT, D, I, scratch, sb, vqs::SUM_F32, w.ddelta32, D, 0, st, "dec cross o"));
        VQS_TAP("dec", i, "d_cross", w.ddelta32, (size_t)MT * D);
        // ---- gated FFN
        VQS_HIP(h, vqs::launch_rmsnorm_split(w.dhid, w.ddelta32, ln2, w.dxn, pD, MT, D, c.t5_ln_eps, st), "dec rmsnorm2");
        TAP2("dec", i, "xn2", w.dxn, pD);
        VQS_RUN(dec_linear_split(h, w.dxn, h->dec_wi[i], MT, 2 * F, D, scratch, sb, vqs::SUM_GATED_SPLIT, w.dff, F, pF, st, "dec wi"));
        TAP2("dec", i, "ff", w.dff, pF);
        VQS_RUN(dec_linear_split(h, w.dff, wo, MT, D, F, scratch, sb, vqs::SUM_F32, w.ddelta32, D, 0, st, "dec wo"));
        VQS_TAP("dec", i, "d_ff", w.ddelta32, (size_t)MT * D);
        dpend = w.ddelta32;
    }
    {
        VQS_W(fin, "decoder.final_layer_norm.weight", D);
        VQS_W(head, "lm_head.weight", (int64_t)V * D);
        VQS_HIP(h, vqs::launch_rmsnorm_split(w.dhid, dpend, fin, w.dxn, pD, MT, D, c.t5_ln_eps, st), "dec final norm");
        if ((w.ldl % 4) != 0 || (V % 4) != 0) return fail(h, VQS_ERR_INVALID, "precise decoder: vocabulary must be a multiple of 4");
        VQS_RUN(dec_linear_split(h, w.dxn, head, MT, V, D, scratch, sb, vqs::SUM_F32, w.logits, w.ldl, 0, st, "lm_head"));
    }
    return VQS_OK;
}

int vqs_score(vqs_handle* h, const void* d_feats, const int32_t* d_img_index, const int32_t* d_input_ids,
              const int32_t* d_labels, int32_t B, int32_t L, int32_t T, float* d_lp, float* d_scores, void* d_ws,
              size_t ws_bytes, void* stream) {
    if (!h) return VQS_ERR_INVALID;
    if (!h->bound) return fail(h, VQS_ERR_STATE, "score: weights not bound");
    if (!d_feats || !d_img_index || !d_input_ids || !d_labels || !d_lp || !d_scores || !d_ws)
        return fail(h, VQS_ERR_INVALID, "score: null argument");
    if (B <= 0 || L < 1 || T <= 0 || T > 16) return fail(h, VQS_ERR_INVALID, "score: need B>0, L>=1, 1<=T<=16");
    const vqs_config& c = h->c;
    const int P = h->P, S = L - 1 + P;
    if (L - 1 > 2048) return fail(h, VQS_ERR_INVALID, "score: prompt longer than CONTEXT_LEN (2048)");
    if ((size_t)(2 * S + 96) * 16 + 32768 > 160 * 1024) return fail(h, VQS_ERR_INVALID, "score: encoder length too large for the attention kernel's bias tables");
    const ScoreWs w = carve_score(h, (char*)d_ws, B, L, T);
    if (ws_bytes < w.total) return fail(h, VQS_ERR_WORKSPACE, "score: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int V = c.vocab;

    const bool precise = h->dec_precise && h->cross_mode != 0;
    if (precise && h->dec_fp16 && h->gemm_variant != 3)
        return fail(h, VQS_ERR_STATE, "score: the fp16 cross-attention score path (option dec_fp16, default 1) needs gemm_variant 3; set dec_fp16=0 to A/B other GEMM forms");
    VQS_RUN(encoder_pass(h, w, d_feats, d_img_index, d_input_ids, B, L, st, precise && h->dec_fp16 != 0));
    if (precise)
        VQS_RUN(decoder_pass_precise(h, w, d_labels, T, B, L, T, st));
    else                                             // bf16 decoder of rounds 1-3 (option dec_precise=0, or the direct cross-attention form)
        VQS_RUN(decoder_pass(h, w, d_labels, T, B, L, T, st));
    VQS_HIP(h, vqs::launch_score_head(w.logits, w.ldl, V, d_labels, d_lp, d_scores, B, T, st, w.flags), "score head");
    return VQS_OK;
}


// Greedy decoding (the reference's `model.generate`, V_3.0_README.md:316-325; HF GenerationMixin greedy search with
// T5's decoder_start_token_id = pad = 0): the encoder runs once, then step t decodes ONE new row per pair -- its
// self-attention K/V are appended to a per-layer cache in the workspace and it attends to positions 0..t of it (the
// cross-attention is the reassociated form over the encoder output, which needs no cache) -- and appends
// argmax(logits).  No host synchronisation; all max_new steps are executed, the caller truncates at the first EOS.
// d_tokens: int32 [B, max_new].
size_t vqs_generate_workspace_bytes(const vqs_handle* h, int32_t B, int32_t L, int32_t max_new) {
    if (!h || B <= 0 || L < 1 || max_new <= 0 || max_new > VQS_MAX_NEW_TOKENS) return 0;
    return carve_score(h, nullptr, B, L, 1, nullptr, max_new).total;
}

int vqs_generate(vqs_handle* h, const void* d_feats, const int32_t* d_img_index, const int32_t* d_input_ids, int32_t B,
                 int32_t L, int32_t max_new, int32_t* d_tokens, void* d_ws, size_t ws_bytes, void* stream) {
    if (!h) return VQS_ERR_INVALID;
    if (!h->bound) return fail(h, VQS_ERR_STATE, "generate: weights not bound");
    if (!d_feats || !d_img_index || !d_input_ids || !d_tokens || !d_ws) return fail(h, VQS_ERR_INVALID, "generate: null argument");
    if (B <= 0 || L < 1 || max_new <= 0 || max_new > VQS_MAX_NEW_TOKENS)
        return fail(h, VQS_ERR_INVALID, "generate: need B>0, L>=1, 1<=max_new<=" + std::to_string(VQS_MAX_NEW_TOKENS));
    if (L - 1 > 2048) return fail(h, VQS_ERR_INVALID, "generate: prompt longer than CONTEXT_LEN (2048)");
    if (h->cross_mode == 0) return fail(h, VQS_ERR_STATE, "generate: needs the reassociated cross-attention (option cross_mode=1)");
    const ScoreWs w = carve_score(h, (char*)d_ws, B, L, 1, nullptr, max_new);
    if (ws_bytes < w.total) return fail(h, VQS_ERR_WORKSPACE, "generate: workspace too small (size it with vqs_generate_workspace_bytes(B, L, max_new))");
    hipStream_t st = (hipStream_t)stream;
    VQS_HIP(h, hipMemsetAsync(d_tokens, 0, (size_t)B * max_new * sizeof(int32_t), st), "memset tokens");
    VQS_RUN(encoder_pass(h, w, d_feats, d_img_index, d_input_ids, B, L, st));
    for (int t = 0; t < max_new; ++t) {
        // one new decoder row per pair: position t, input = token t-1 (start token for t = 0), self-attention over the cache
        VQS_RUN(decoder_pass(h, w, d_tokens, max_new, B, L, 1, st, t, true));
        VQS_HIP(h, vqs::launch_argmax_append(w.logits, w.ldl, h->c.vocab, d_tokens, max_new, B, 1, st, t, w.flags), "argmax");   // + status bit 1 on a non-finite logit
    }
    return VQS_OK;
}

int64_t vqs_workspace_offset(const vqs_handle* h, const char* name, int32_t B, int32_t L, int32_t T, int64_t* ld_out) {
    if (!h || !name) return -1;
    std::unordered_map<std::string, size_t> names;
    int64_t ld = 0;
    const std::string n(name);
    if (n == "vit_hidden") {
        if (B <= 0) return -1;
        carve_encode(h, nullptr, B, &names);
        ld = h->c.vis_hidden;
    } else {
        if (B <= 0 || L < 1 || T <= 0) return -1;
        const ScoreWs w = carve_score(h, nullptr, B, L, T, &names);
        if (n == "logits") ld = w.ldl;
        else if (n == "enc_in" || n == "enc_out" || n == "dec_out") ld = h->c.d_model;
        else ld = 1;
    }
    auto it = names.find(n);
    if (it == names.end()) return -1;
    if (ld_out) *ld_out = ld;
    return (int64_t)it->second;
}

int vqs_profile_enable(vqs_handle* h, int32_t on) {
    if (!h) return VQS_ERR_INVALID;
    h->prof.on = on != 0;
    return VQS_OK;
}

int vqs_profile_read(vqs_handle* h, double* gemm_ms, double* gemm_flops, int32_t reset) {
    return h ? vqs::profile_read(h, gemm_ms, gemm_flops, nullptr, reset != 0) : VQS_ERR_INVALID;
}

const char* vqs_profile_report(vqs_handle* h) { return h ? h->prof.report.c_str() : ""; }

int vqs_profile_bytes(vqs_handle* h, double* gemm_bytes) {
    if (!h || !gemm_bytes) return VQS_ERR_INVALID;
    *gemm_bytes = h->prof.bytes;
    return VQS_OK;
}

// ---------------------------------------------------------------------------- single-kernel entry points
// GEMM with the fused residual + RMSNorm pieces (tests): epilogue 7 (producer: hres/lnw/rowss_out) and/or a consumer row
// scale (rowss_in/rowss_parts/rs_invd/rs_eps) in front of epilogues 0, 3, 5, 6.  Variants 3, 5, 10 and 11 only.
int vqs_gemm_rms(const void* A, const void* W, void* C, float* hres, const void* lnw, float* rowss_out, const float* rowss_in,
                 int32_t rowss_parts, float rs_invd, float rs_eps, int32_t M, int32_t N, int32_t K, int32_t lda, int32_t ldw,
                 int32_t ldc, int32_t epilogue, int32_t S, int32_t H, int32_t variant, void* stream) {
    vqs::GemmParams p;
    p.A = (const bf16_t*)A; p.W = (const bf16_t*)W; p.C = C; p.bias = nullptr; p.resid = nullptr;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = ldc;
    p.S = S > 0 ? S : 1; p.H = H; p.inner = H * 64 > 0 ? H * 64 : 1;
    const size_t per = (size_t)(S > 0 ? M / S : 0) * H * S * 64;
    p.heads_out[0] = (bf16_t*)C;
    p.heads_out[1] = (bf16_t*)C + per;
    p.heads_out[2] = (bf16_t*)C + 2 * per;
    p.hres = hres; p.ldh = N; p.lnw = (const bf16_t*)lnw; p.rowss_out = rowss_out;
    p.rowss_in = rowss_in; p.rowss_parts = rowss_parts; p.rs_invd = rs_invd; p.rs_eps = rs_eps;
    p.tile_gm = (variant >> 8) & 0xff;     // same layout of the variant word as vqs_gemm
    p.tile_ns = (variant >> 16) & 0xff;
    return vqs::launch_gemm(p, epilogue, variant & 0xff, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_gemm(const void* A, const void* W, void* C, const void* bias, const float* resid, int32_t M, int32_t N, int32_t K,
             int32_t lda, int32_t ldw, int32_t ldc, int32_t epilogue, int32_t S, int32_t H, int32_t variant, void* stream) {
    vqs::GemmParams p;
    p.A = (const bf16_t*)A; p.W = (const bf16_t*)W; p.C = C; p.bias = (const bf16_t*)bias; p.resid = resid;
    p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldw = ldw; p.ldc = ldc;
    p.S = S > 0 ? S : 1; p.H = H; p.inner = H * 64 > 0 ? H * 64 : 1;
    const size_t per = (size_t)(S > 0 ? M / S : 0) * H * S * 64;   // elements per head-major tensor
    p.heads_out[0] = (bf16_t*)C;
    p.heads_out[1] = (bf16_t*)C + per;
    p.heads_out[2] = (bf16_t*)C + 2 * per;
    p.tile_gm = (variant >> 8) & 0xff;     // bits 8-15 / 16-23 of `variant`: tile order (0 = default), see vqs.h
    p.tile_ns = (variant >> 16) & 0xff;
    p.nt_store = (variant >> 24) & 1;      // bit 24: non-temporal result stores; bits 25-26: A-panel L2 touch (0 by shape, 1 on, 2 off)
    p.l2_touch = (variant >> 25) & 3;
    p.f16 = (variant >> 27) & 3;           // bits 27-28: 0 bf16 operands and result, 1 IEEE fp16 operands and result, 2 fp16 operands / bf16 result
    if (p.f16 == 3) return VQS_ERR_INVALID;
    return vqs::launch_gemm(p, epilogue, variant & 0xff, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_attention(const void* q, const void* k, const void* v, void* out, const float* bias_table, const int32_t* key_len,
                  int32_t B, int32_t H, int32_t S, float scale, void* stream) {
    vqs::AttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, bias_table, key_len, B, H, S, scale};
    return vqs::launch_attention(a, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_debug_attention_f16(const void* q, const void* k, const void* v, void* out, const float* bias_table, const int32_t* key_len,
                            int32_t B, int32_t H, int32_t S, float scale, void* stream) {
    vqs::AttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, bias_table, key_len, B, H, S, scale};
    a.f16 = 1;
    return vqs::launch_attention(a, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_debug_qwen_attention(const void* q, const void* k, const void* v, void* out, const int32_t* key_len, int32_t B, int32_t H, int32_t Hkv,
                             int32_t S, float scale, int32_t f16, void* stream) {
    if (!q || !k || !v || !out || !key_len) return VQS_ERR_INVALID;
    vqs::AttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, nullptr, key_len, B, H, S, scale};
    a.hd = 128; a.Hkv = Hkv; a.causal = 1; a.f16 = f16 ? 1 : 0;
    return vqs::abi_code(vqs::launch_attention(a, (hipStream_t)stream));
}

int vqs_debug_attention_hd(const void* q, const void* k, const void* v, void* out, const int32_t* key_len, int32_t B, int32_t H, int32_t Hkv,
                           int32_t S, float scale, int32_t causal, int32_t f16, int32_t out_hd, void* stream) {
    if (!q || !k || !v || !out) return VQS_ERR_INVALID;
    vqs::AttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, nullptr, key_len, B, H, S, scale};
    a.hd = 128; a.Hkv = Hkv; a.causal = causal ? 1 : 0; a.out_hd = out_hd; a.f16 = f16 ? 1 : 0;
    return vqs::abi_code(vqs::launch_attention(a, (hipStream_t)stream));
}

int vqs_debug_qwen_attention_suffix(const void* q, const void* k, const void* v, void* out, const int32_t* key_len, int32_t B, int32_t H,
                                    int32_t Hkv, int32_t S, int32_t Sq, int32_t q0, float scale, int32_t f16, void* stream) {
    if (!q || !k || !v || !out || !key_len) return VQS_ERR_INVALID;
    vqs::AttnSuffixParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, key_len, B, H, Hkv, S, Sq, q0, scale};
    a.f16 = f16 ? 1 : 0;
    return vqs::abi_code(vqs::launch_attention_suffix(a, (hipStream_t)stream));
}

int vqs_debug_qwen_kv_assemble(const void* pk, const void* pv, const void* sk, const void* sv, const int32_t* media_idx, void* dk, void* dv,
                               int32_t B, int32_t U, int32_t Hkv, int32_t Lp, int32_t Ls, void* stream) {
    if (!pk || !pv || !sk || !sv || !media_idx || !dk || !dv) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_qwen_kv_assemble((const bf16_t*)pk, (const bf16_t*)pv, (const bf16_t*)sk, (const bf16_t*)sv, media_idx, (bf16_t*)dk,
                                                 (bf16_t*)dv, B, U, Hkv, Lp, Ls, (hipStream_t)stream));
}

int vqs_debug_qwen_decode_attention(const void* q, const void* kc, const void* vc, const int32_t* len, void* out, int64_t out_plane, int32_t B, int32_t Hq,
                                    int32_t Hkv, int32_t Lmax, float scale, float vscale, int32_t mode, void* stream) {
    if (!q || !kc || !vc || !len || !out || mode < 0 || mode > 2) return VQS_ERR_INVALID;
    if (mode == 0)
        return vqs::abi_code(vqs::launch_qwen_decode_attn((const bf16_t*)q, (const bf16_t*)kc, (const bf16_t*)vc, len, (bf16_t*)out, B, Hq, Hkv, Lmax, scale,
                                                          (hipStream_t)stream));
    return vqs::abi_code(vqs::launch_qwen_tail_attn((const float*)q, (const bf16_t*)kc, (const bf16_t*)vc, len, (bf16_t*)out, (long long)out_plane, B, Hq, Hkv, Lmax,
                                                    scale, (hipStream_t)stream, mode == 2, mode == 2 ? vscale : 1.0f));
}

int vqs_debug_qwen_rows_attention(const void* q, const void* k, const void* v, const int32_t* row_sample, const int32_t* row_keys, void* out, int64_t out_plane,
                                  int32_t Q, int32_t R, int32_t Hq, int32_t Hkv, int32_t L, float scale, int32_t kv_f16, float vscale, void* stream) {
    if (!q || !k || !v || !row_sample || !row_keys || !out) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_qwen_rows_attn((const float*)q, (const bf16_t*)k, (const bf16_t*)v, row_sample, row_keys, (bf16_t*)out, (long long)out_plane, Q, R,
                                                    Hq, Hkv, L, scale, (hipStream_t)stream, kv_f16 != 0, kv_f16 ? vscale : 1.0f));
}

int vqs_debug_qwen_decode_rope_append(const void* qkv, const float* cs, const float* sn, const int32_t* len, void* q_out, void* kc, void* vc, int32_t B,
                                      int32_t Hq, int32_t Hkv, int32_t hd, int32_t half, int32_t Lmax, void* stream) {
    if (!qkv || !cs || !sn || !len || !q_out || !kc || !vc) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_qwen_decode_rope_append((const bf16_t*)qkv, cs, sn, len, (bf16_t*)q_out, (bf16_t*)kc, (bf16_t*)vc, B, Hq, Hkv, hd, half, Lmax,
                                                             (hipStream_t)stream));
}

int vqs_debug_qwen_decode_attention_form(int32_t Hq, int32_t Hkv, int32_t Lmax, int64_t* lds_bytes) {
    size_t lds = 0;
    const int form = vqs::qwen_decode_attn_form(Hq, Hkv, Lmax, &lds);
    if (lds_bytes) *lds_bytes = (int64_t)lds;
    return form;
}

// ---- single-launch hooks of the precise decoder's glue, the split-K reductions and the greedy / score tail (include/vqs_debug.h)
int vqs_debug_rmsnorm_split(float* x, const float* delta, const void* w, void* out, int64_t out_plane, int32_t M, int32_t D, float eps, void* stream) {
    if (!x || !w || !out) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_rmsnorm_split(x, delta, (const bf16_t*)w, (bf16_t*)out, (long long)out_plane, M, D, eps, (hipStream_t)stream));
}

int vqs_debug_sum_planes(const float* part, int32_t nslices, int64_t slice_stride, int32_t rows, int32_t cols, int32_t ldp, int32_t mode, void* out,
                         int32_t ld_out, int64_t out_plane, const void* bias, int32_t silu, void* stream) {
    if (!part || !out) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_sum_planes(part, nslices, (long long)slice_stride, rows, cols, ldp, mode, out, ld_out, (long long)out_plane,
                                                (hipStream_t)stream, (const bf16_t*)bias, silu));
}

int vqs_debug_reduce_slices(const float* part, int32_t nslices, int64_t n, void* out, void* stream) {
    if (!part || !out || nslices <= 0 || n <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_reduce_slices(part, nslices, (size_t)n, (bf16_t*)out, (hipStream_t)stream));
}

int vqs_debug_reduce_slices_act(const float* part, int32_t nslices, int64_t slice_stride, int32_t rows, int32_t cols, int32_t ldp, const void* bias,
                                int32_t gated, void* out, int32_t ld_out, void* stream) {
    if (!part || !out) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_reduce_slices_act(part, nslices, (long long)slice_stride, rows, cols, ldp, (const bf16_t*)bias, gated, (bf16_t*)out,
                                                       ld_out, (hipStream_t)stream));
}

int vqs_debug_masked_softmax(const float* scores, void* probs, const int32_t* key_len, int32_t B, int32_t rows, int32_t S_pad, int32_t out_f16,
                             void* stream) {
    if (!scores || !probs || !key_len || B <= 0 || rows <= 0 || S_pad <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_masked_softmax(scores, (bf16_t*)probs, key_len, B, rows, S_pad, (hipStream_t)stream, out_f16 != 0));
}

int vqs_debug_transpose_pad(const void* in, void* out, int32_t B, int32_t S, int32_t D, int32_t S_pad, void* stream) {
    if (!in || !out || B <= 0 || S <= 0 || D <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_transpose_pad((const bf16_t*)in, (bf16_t*)out, B, S, D, S_pad, (hipStream_t)stream));
}

int vqs_debug_argmax_append(const float* logits, int32_t ldl, int32_t V, int32_t* tokens, int32_t ld_tokens, int32_t B, int32_t T, int32_t dst_col,
                            int32_t* flags, void* stream) {
    if (!logits || !tokens || B <= 0 || T <= 0 || V <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_argmax_append(logits, ldl, V, tokens, ld_tokens, B, T, (hipStream_t)stream, dst_col, flags));
}

int vqs_debug_decoder_attention(const void* q, const void* k, const void* v, void* out, const float* bias_table, const int32_t* key_len, int32_t B,
                                int32_t H, int32_t T, int32_t S, int32_t ldq, int32_t ldk, int32_t cross, int64_t kv_stride_b, int32_t qpos0,
                                int32_t bias_ld, int32_t precise, int64_t out_plane, void* stream) {
    if (!q || !k || !v || !out || B <= 0 || H <= 0) return VQS_ERR_INVALID;
    vqs::DecAttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, bias_table, key_len, B, H, T, S, ldq, ldk, cross};
    a.kv_stride_b = (long long)kv_stride_b; a.qpos0 = qpos0; a.bias_ld = bias_ld; a.precise = precise; a.out_plane = (long long)out_plane;
    return vqs::abi_code(vqs::launch_decoder_attention(a, (hipStream_t)stream));
}

int vqs_debug_score_head(const float* logits, int32_t ldl, int32_t V, const int32_t* labels, float* lp, float* scores, int32_t B, int32_t T,
                         int32_t* flags, void* stream) {
    if (!logits || !labels || !lp || !scores || B <= 0 || T <= 0 || V <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_score_head(logits, ldl, V, labels, lp, scores, B, T, (hipStream_t)stream, flags));
}

int vqs_debug_norm16(int32_t kind, float* x, const void* delta, const void* delta2, int32_t store_x, const void* w, const void* b,
                     void* out, int32_t M, int32_t D, float eps, int32_t types, void* stream) {
    if (!x || !w || !out || (kind == 1 && !b) || (kind != 0 && kind != 1)) return VQS_ERR_INVALID;
    hipError_t e;
    if (kind == 0 && types == 1)          // RMSNorm, bf16 deltas in, fp16 operand out: the T5 encoder of option enc_fp16
        e = vqs::launch_rmsnorm(x, (const bf16_t*)delta, (const bf16_t*)w, (bf16_t*)out, M, D, eps, (hipStream_t)stream, (const bf16_t*)delta2,
                                store_x != 0, 0, true);
    else if (kind == 1 && types == 3)     // LayerNorm, fp16 deltas in, fp16 operand out: the vision tower of option vit_fp16
        e = vqs::launch_layernorm(x, (const bf16_t*)delta, (const bf16_t*)w, (const bf16_t*)b, out, 0, M, D, eps, (hipStream_t)stream,
                                  (const bf16_t*)delta2, store_x != 0, true);
    else
        return VQS_ERR_INVALID;
    return vqs::abi_code(e);
}

// ---- single-launch hooks of the Qwen2.5-VL prefill's glue and of the bind-time range proof (include/vqs_debug.h)
int vqs_debug_rmsnorm_f16s(float* x, const void* delta, const void* delta2, int32_t store_x, const void* w, void* out, int32_t out_ld, int32_t M, int32_t D,
                           float eps, float d1, float d2, float osc, int32_t out_bf16, void* stream) {
    if (!x || !w || !out || M <= 0 || D <= 0 || out_ld < 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_rmsnorm_f16s(x, (const bf16_t*)delta, (const bf16_t*)w, (bf16_t*)out, M, D, eps, (hipStream_t)stream, (const bf16_t*)delta2,
                                                  store_x != 0, out_ld, d1, d2, osc, out_bf16 != 0));
}

int vqs_debug_rope_qk(void* q, void* k, const float* cs, const float* sn, int32_t B, int32_t Hq, int32_t Hk, int32_t S, int32_t hd, int32_t half, int32_t f16,
                      void* stream) {
    if (!q || !k || !cs || !sn || B <= 0 || Hq <= 0 || Hk <= 0 || S <= 0 || hd <= 0 || half <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_rope_qk((bf16_t*)q, (bf16_t*)k, cs, sn, B, Hq, Hk, S, hd, half, (hipStream_t)stream, f16 != 0));
}

int vqs_debug_qwen_embed(const int32_t* ids, const int32_t* vis_slot, const void* embed, const void* merged, float* out, int32_t rows, int32_t D, int32_t vocab,
                         int32_t merged_f16, float unscale, void* stream) {
    if (!ids || !vis_slot || !embed || !merged || !out || rows <= 0 || D <= 0 || vocab <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_qwen_embed(ids, vis_slot, (const bf16_t*)embed, (const bf16_t*)merged, out, rows, D, vocab, (hipStream_t)stream,
                                                merged_f16 != 0, unscale));
}

int vqs_debug_gather_rows_bf16(const void* src0, const void* src1, const int32_t* map, void* dst, int32_t rows, int32_t cols, int32_t src_ld, int32_t dst_ld,
                               void* stream) {
    if (!src0 || !dst || rows <= 0 || cols <= 0 || src_ld < cols || dst_ld < cols) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_gather_rows_bf16((const bf16_t*)src0, (const bf16_t*)src1, map, (bf16_t*)dst, rows, cols, src_ld, dst_ld, (hipStream_t)stream));
}

int vqs_debug_gather_cols_bf16(const void* src, const int32_t* cmap, void* dst, int32_t rows, int32_t src_ld, int32_t dst_cols, void* stream) {
    if (!src || !cmap || !dst || rows <= 0 || src_ld <= 0 || dst_cols <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_gather_cols_bf16((const bf16_t*)src, cmap, (bf16_t*)dst, rows, src_ld, dst_cols, (hipStream_t)stream));
}

int vqs_debug_gather_rows_f32(const float* src, const int32_t* map, float* dst, int32_t rows, int32_t cols, int32_t src_ld, int32_t form, void* stream) {
    if (!src || !map || !dst || rows <= 0 || cols <= 0) return VQS_ERR_INVALID;
    if (form == 0) {        // elementwise.hip: dense rows, -1 = a zero row
        if (src_ld != 0 && src_ld != cols) return VQS_ERR_INVALID;
        return vqs::abi_code(vqs::launch_gather_rows_f32(src, map, dst, rows, cols, (hipStream_t)stream));
    }
    if (form != 1 || src_ld < cols) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_gather_rows_f32(src, map, dst, rows, cols, src_ld, (hipStream_t)stream));      // qwen_decode.hip
}

int vqs_debug_f16_to_bf16_rows(const void* src, void* dst, int32_t rows, int64_t cols, int64_t src_ld, int64_t dst_ld, float unscale, void* stream) {
    if (!src || !dst || src_ld < cols || dst_ld < cols) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_f16_to_bf16_rows((const bf16_t*)src, (bf16_t*)dst, rows, (long long)cols, (long long)src_ld, (long long)dst_ld, unscale,
                                                      (hipStream_t)stream));
}

int vqs_debug_qwen_tail_rope_q(const float* qkv, int32_t ld, const float* cs, const float* sn, const int32_t* row, float* q_out, int32_t B, int32_t Hq, int32_t hd,
                               int32_t half, void* stream) {
    if (!qkv || !cs || !sn || !row || !q_out || hd <= 0 || Hq <= 0 || (int64_t)ld < (int64_t)Hq * hd) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_qwen_tail_rope_q(qkv, ld, cs, sn, row, q_out, B, Hq, hd, half, (hipStream_t)stream));
}

int vqs_debug_rowbound(const void* W, int64_t ldw, int32_t N, int32_t K, int32_t mode, const void* g, int32_t g_len, float R, const float* u, const float* uconst,
                       const void* bias, float* out, float* slot, void* stream) {
    if (!W || ldw < K || (mode != 0 && mode != 1)) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_rowbound((const bf16_t*)W, (long long)ldw, N, K, mode, (const bf16_t*)g, g_len, R, u, uconst, (const bf16_t*)bias, out, slot,
                                              (hipStream_t)stream));
}

int vqs_debug_absmax_bf16(const void* x, int64_t n, float R, float* slot, void* stream) {
    if (n <= 0) return VQS_ERR_INVALID;
    return vqs::abi_code(vqs::launch_absmax_bf16((const bf16_t*)x, (size_t)n, R, slot, (hipStream_t)stream));
}

int vqs_debug_gate_pair_bound(const float* rb, int32_t mlp_p, int32_t ld, float* u_act, float* slot, void* stream) {
    return vqs::abi_code(vqs::launch_gate_pair_bound(rb, mlp_p, ld, u_act, slot, (hipStream_t)stream));
}

int vqs_normalize_u8(const void* d_u8, void* d_out, int32_t N, int32_t H, int32_t W, const float* mean3, const float* std3,
                     void* stream) {
    if (!d_u8 || !d_out || !mean3 || !std3) return VQS_ERR_INVALID;
    return vqs::launch_u8_to_norm_bf16((const unsigned char*)d_u8, (bf16_t*)d_out, N, H, W, mean3, std3, (hipStream_t)stream) == hipSuccess
               ? VQS_OK : VQS_ERR_HIP;
}

size_t vqs_images_workspace_bytes(int32_t n, int32_t rows, int32_t S) {
    if (n <= 0 || rows < 0 || S <= 0) return 0;
    const size_t need = (size_t)n * (size_t)rows * (size_t)S * 3;
    return std::max<size_t>((need + 255) & ~(size_t)255, 256);
}

int vqs_images_u8(const void* d_src, const vqs_image_geometry* g, const int32_t* d_first_h, const int32_t* d_weights_h, const int32_t* d_first_v,
                  const int32_t* d_weights_v, const void* d_lut, void* d_out, void* d_ws, size_t ws_bytes, void* stream) {
    if (!d_src || !g || !d_lut || !d_out) return VQS_ERR_INVALID;
    if (g->n <= 0 || g->n > 65535 || g->H <= 0 || g->W <= 0 || g->Hc <= 0 || g->Wc <= 0 || g->S <= 0 || g->resized_h <= 0 || g->resized_w <= 0)
        return VQS_ERR_INVALID;
    const int32_t rgb[3] = {g->color_r, g->color_g, g->color_b};
    for (int32_t v : rgb)
        if (v < 0 || v > 255) return VQS_ERR_INVALID;
    // the source rectangle lies inside the canvas, the crop window inside the resized axis (sums in 64 bits: no wrap-around)
    if (g->oy < 0 || g->ox < 0 || (long long)g->oy + g->H > g->Hc || (long long)g->ox + g->W > g->Wc) return VQS_ERR_INVALID;
    if (g->crop_y < 0 || g->crop_x < 0 || (long long)g->crop_y + g->S > g->resized_h || (long long)g->crop_x + g->S > g->resized_w)
        return VQS_ERR_INVALID;
    const bool horiz = g->resized_w != g->Wc, vert = g->resized_h != g->Hc;
    if (horiz && (!d_first_h || !d_weights_h || g->taps_h <= 0)) return VQS_ERR_INVALID;
    if (vert && (!d_first_v || !d_weights_v || g->taps_v <= 0)) return VQS_ERR_INVALID;
    if ((long long)g->n * g->H * g->W > (1LL << 40) / 3 || (long long)g->n * g->S * g->S > (1LL << 40) / 3) return VQS_ERR_INVALID;
    if (horiz) {
        if (g->Wc > 16384 || !vqs::images_u8_lds_bytes(g->Wc, nullptr)) return VQS_ERR_INVALID;
        if (g->row0 < 0 || g->rows <= 0 || (long long)g->row0 + g->rows > g->Hc) return VQS_ERR_INVALID;
        if (!vert && (g->row0 > g->crop_y || g->crop_y + g->S > g->row0 + g->rows)) return VQS_ERR_INVALID;
        if (!d_ws || ws_bytes < (size_t)g->n * (size_t)g->rows * (size_t)g->S * 3) return VQS_ERR_WORKSPACE;
    }
    vqs::ImagesU8 p{};
    p.src = (const unsigned char*)d_src;
    p.n = g->n; p.H = g->H; p.W = g->W;
    p.Hc = g->Hc; p.Wc = g->Wc; p.oy = g->oy; p.ox = g->ox;
    p.color = rgb[0] | (rgb[1] << 8) | (rgb[2] << 16);
    p.S = g->S;
    p.x0h = horiz ? d_first_h : nullptr; p.kh = horiz ? d_weights_h : nullptr; p.taps_h = horiz ? g->taps_h : 0; p.crop_x = g->crop_x;
    p.y0v = vert ? d_first_v : nullptr; p.kv = vert ? d_weights_v : nullptr; p.taps_v = vert ? g->taps_v : 0; p.crop_y = g->crop_y;
    p.row0 = horiz ? g->row0 : 0; p.nrows = horiz ? g->rows : 0;
    p.mid = horiz ? (unsigned char*)d_ws : nullptr;
    p.lut = (const bf16_t*)d_lut;
    p.out = (bf16_t*)d_out;
    return vqs::launch_images_u8(p, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_rope(void* x, const float* cos_t, const float* sin_t, int32_t B, int32_t H, int32_t S, int32_t hd, int32_t half,
             void* stream) {
    return vqs::launch_rope((bf16_t*)x, cos_t, sin_t, B, H, S, hd, half, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

// Attention with head_dim 128, grouped-query heads and an optional causal mask (the Qwen2.5-VL row)
int vqs_attention_hd(const void* q, const void* k, const void* v, void* out, const int32_t* key_len, int32_t B, int32_t H,
                     int32_t Hkv, int32_t S, int32_t hd, float scale, int32_t causal, void* stream) {
    vqs::AttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, nullptr, key_len, B, H, S, scale};
    a.hd = hd; a.Hkv = Hkv; a.causal = causal;
    return vqs::launch_attention(a, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_decoder_attention(const void* q, const void* k, const void* v, void* out, const float* bias_table,
                          const int32_t* key_len, int32_t B, int32_t H, int32_t T, int32_t S, int32_t ldq, int32_t ldk,
                          int32_t cross, void* stream) {
    vqs::DecAttnParams a{(const bf16_t*)q, (const bf16_t*)k, (const bf16_t*)v, (bf16_t*)out, bias_table, key_len,
                         B, H, T, S, ldq, ldk, cross};
    return vqs::launch_decoder_attention(a, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_rmsnorm(float* x, const void* delta, const void* w, void* out, int32_t M, int32_t D, float eps, void* stream) {
    return vqs::launch_rmsnorm(x, (const bf16_t*)delta, (const bf16_t*)w, (bf16_t*)out, M, D, eps, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

int vqs_norm_deferred(int32_t kind, float* x, const void* delta, const void* delta2, int32_t store_x, const void* w, const void* b,
                      void* out, int32_t M, int32_t D, float eps, void* stream) {
    if (!x || !delta || !w || !out || (kind == 1 && !b) || (kind != 0 && kind != 1)) return VQS_ERR_INVALID;
    const hipError_t e = kind == 0
        ? vqs::launch_rmsnorm(x, (const bf16_t*)delta, (const bf16_t*)w, (bf16_t*)out, M, D, eps, (hipStream_t)stream,
                              (const bf16_t*)delta2, store_x != 0)
        : vqs::launch_layernorm(x, (const bf16_t*)delta, (const bf16_t*)w, (const bf16_t*)b, out, 0, M, D, eps, (hipStream_t)stream,
                                (const bf16_t*)delta2, store_x != 0);
    return vqs::abi_code(e);
}

int vqs_layernorm(float* x, const void* delta, const void* w, const void* b, void* out, int32_t out_f32, int32_t M, int32_t D,
                  float eps, void* stream) {
    return vqs::launch_layernorm(x, (const bf16_t*)delta, (const bf16_t*)w, (const bf16_t*)b, out, out_f32, M, D, eps, (hipStream_t)stream) == hipSuccess
               ? VQS_OK : VQS_ERR_HIP;
}

int vqs_score_head(const float* logits, int32_t ldl, int32_t V, const int32_t* labels, float* lp, float* scores, int32_t B,
                   int32_t T, void* stream) {
    return vqs::launch_score_head(logits, ldl, V, labels, lp, scores, B, T, (hipStream_t)stream) == hipSuccess ? VQS_OK : VQS_ERR_HIP;
}

}  // extern "C"
