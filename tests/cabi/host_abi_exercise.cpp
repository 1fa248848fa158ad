// Host-side exercise of the C ABI under AddressSanitizer + UBSan: everything that runs without touching a device
// (creation, sizing, options, taps registration, error paths, integer helpers).  No GPU needed.
#include "vqs.h"
#include "vqs_debug.h"
#include "vqs_qwen.h"
#include "vqs_clip.h"
#include <cassert>
#include <cstdio>
#include <cstring>
#include <vector>
int main() {
    vqs_config c;
    memset(&c, 0, sizeof c);
    c.vis_hidden = 1024; c.vis_layers_run = 23; c.vis_heads = 16; c.vis_mlp = 4096; c.vis_patch = 14; c.vis_image = 336; c.vis_ln_eps = 1e-5f;
    c.d_model = 4096; c.n_heads = 64; c.d_kv = 64; c.d_ff = 10240; c.enc_layers = 24; c.dec_layers = 24; c.vocab = 32128;
    c.rel_buckets = 32; c.rel_max_distance = 128; c.t5_ln_eps = 1e-6f;
    vqs_handle* h = nullptr;
    assert(vqs_create(&c, &h) == 0 && h);
    assert(vqs_packed_bytes(h) > 0);
    assert(vqs_encode_workspace_bytes(h, 256) > 0 && vqs_encode_workspace_bytes(h, 0) == 0);
    assert(vqs_score_workspace_bytes(h, 256, 33, 2) > 0 && vqs_score_workspace_bytes(h, 0, 33, 2) == 0);
    assert(vqs_generate_workspace_bytes(h, 4, 33, 64) > 0 && vqs_generate_workspace_bytes(h, 4, 33, 100000) == 0);
    assert(vqs_set_option(h, "cross_mode", 0) == 0 && vqs_set_option(h, "cross_mode", 1) == 0);
    assert(vqs_set_option(h, "cross_mode", 7) != 0 && vqs_set_option(h, "nonsense", 1) != 0 && vqs_set_option(h, nullptr, 1) != 0);
    {
        int32_t v = -1;                                   // defaults are readable, a set is read back, unknown names and null arguments are refused
        assert(vqs_get_option(h, "vit_fp16", &v) == 0 && v == 1 && vqs_get_option(h, "dec_precise", &v) == 0 && v == 1);
        assert(vqs_get_option(h, "gemm_variant", &v) == 0 && v == 3 && vqs_get_option(h, "cross_mode", &v) == 0 && v == 1);
        assert(vqs_set_option(h, "vit_fp16", 0) == 0 && vqs_get_option(h, "vit_fp16", &v) == 0 && v == 0 && vqs_set_option(h, "vit_fp16", 1) == 0);
        assert(vqs_set_option(h, "vit_fp16", 2) != 0 && vqs_get_option(h, "nonsense", &v) != 0 && vqs_get_option(h, "vit_fp16", nullptr) != 0);
        assert(vqs_get_option(nullptr, "vit_fp16", &v) != 0 && vqs_get_option(h, nullptr, &v) != 0 && vqs_get_option(h, "tile_order:64x64", &v) != 0);
    }
    assert(strlen(vqs_last_error(h)) > 0);
    int dummy = 0;
    assert(vqs_debug_tap(h, "enc.3.xn0", &dummy, 4) == 0 && vqs_debug_tap(h, "enc.3.xn0", nullptr, 0) == 0 && vqs_debug_tap(h, nullptr, nullptr, 0) == 0);
    assert(vqs_debug_tap_window(h, 3, 2) == 0 && vqs_debug_tap_window(h, 0, 0) == 0 && vqs_debug_tap_window(h, -1, 2) != 0);
    // GEMM form resolution (host arithmetic): the quad form for bf16 results whatever M, the 32-bit kernels refuse >= 4 GiB operands
    // (13 = the quad family's few-row launch shape, gemm_slim.inc, round 6: same bits; variant 10 = the quad kernel whatever the shape)
    assert(vqs_debug_gemm_form(155648, 20480, 4096, 4096, 4096, 5, 1, 3, 0, 0, 0) == 10 && vqs_debug_gemm_form(2, 20480, 4096, 4096, 4096, 5, 1, 3, 0, 0, 0) == 13 &&
           vqs_debug_gemm_form(2, 20480, 4096, 4096, 4096, 5, 1, 10, 0, 0, 0) == 10);
    // round 4: the stream form's rule (<= 128 rows per entry, >= 4 items since round 6 (192 before), not a quad call site) and the batched debug launch's argument checks
    assert(vqs_debug_gemm_form(128, 608, 4096, 4096, 4096, 3, 256, 3, 0, 0, 0) == 12 && vqs_debug_gemm_form(128, 608, 4096, 4096, 4096, 3, 16, 3, 0, 0, 0) == 12 &&
           vqs_debug_gemm_form(64, 384, 4096, 4096, 4096, 3, 1, 3, 0, 0, 0) == 3);
    assert(vqs_debug_gemm_form(64, 32768, 4096, 4096, 4096, 0, 1, 3, 0, 0, 0) == 13 && vqs_debug_gemm_form(64, 32768, 4096, 4096, 4096, 0, 1, 10, 0, 0, 0) == 10);
    {   // the whole plan behind those numbers (gemm.hip gemm_plan): kernel family, touch, operand type, workgroups, workgroup size
        int32_t l[VQS_GEMM_PLAN_FIELDS] = {8192, 2048, 256, 256, 256, 2048, 3, 1, 3, 1, 1}, g[5] = {-1, -1, -1, -1, -1};
        assert(vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS, g) == 1 && g[0] == 2 && g[1] == 2 && g[2] == 0 && g[3] == 256 && g[4] == 512);   // lock-step with the L2 touch
        l[16] = 2;                                                                                                                            // touch off: ping-pong
        assert(vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS, g) == 1 && g[0] == 3 && g[1] == 0 && g[3] == 256 && g[4] == 512);
        l[8] = 7;                                                                                                                             // a lab variant: refused
        assert(vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS, g) == 0);
        l[8] = 3; l[6] = 7;                                                                                                                   // epilogue 7 without / with its operands
        assert(vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS, g) == 0);
        l[18] = 32; l[21] = 2048;
        assert(vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS, g) == 1 && g[0] == 2 && g[1] == 0 && g[3] == 256);
        assert(vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS - 1, g) == VQS_ERR_INVALID && vqs_debug_gemm_plan(nullptr, VQS_GEMM_PLAN_FIELDS, g) == VQS_ERR_INVALID &&
               vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS, nullptr) == VQS_ERR_INVALID);
    }
    {   // the single-launch hook behind the same integers (+ H): everything it refuses, it refuses in host code, before any device call
        int32_t l[VQS_GEMM_LAUNCH_FIELDS] = {136, 640, 128, 128, 128, 0, 6, 1, 10, 8, 384, 128, 128, 0, 1, 0}, g[5];
        l[22] = 3;                                                                                                                            // gqa 3 : 1, 128-lane heads
        int d = 0;
        const void* ptrs[VQS_GEMM_LAUNCH_PTRS] = {&d, &d, nullptr, nullptr, &d, &d, &d, nullptr, nullptr, nullptr};
        const float sc[VQS_GEMM_LAUNCH_SCALES] = {1.0f, 1.0f, 0.0f, 0.0f};
        assert(vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS, g) == 1 && g[0] == 5 && g[3] == 3);                                                // the quad kernel, three tiles
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_PLAN_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        assert(vqs_debug_gemm_launch(nullptr, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, nullptr, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS - 1, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, nullptr, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES + 1, nullptr) == VQS_ERR_INVALID);
        l[18] = 1;                                                                                                                            // bias flag without the vector
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        l[18] = 0; ptrs[7] = &d;                                                                                                              // a rope table without its flag
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        ptrs[7] = nullptr; l[22] = 0;                                                                                                         // no q heads
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        l[22] = 3; l[7] = 2;                                                                                                                  // batched launches, epilogue 7, split results: other hooks
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        l[7] = 1; l[17] = 4096;
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        l[17] = 0; l[6] = 7;
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        l[6] = 6; l[8] = 0;                                                                                                                   // the launcher's refusal: 128-lane heads under variant 0
        assert(vqs_debug_gemm_plan(l, VQS_GEMM_PLAN_FIELDS, g) == 0);
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
        l[8] = 10; l[9] = 7;                                                                                                                  // S = 7 with 128-lane heads
        assert(vqs_debug_gemm_launch(l, VQS_GEMM_LAUNCH_FIELDS, ptrs, VQS_GEMM_LAUNCH_PTRS, sc, VQS_GEMM_LAUNCH_SCALES, nullptr) == VQS_ERR_INVALID);
    }
    assert(vqs_debug_gemm_batched(nullptr, nullptr, nullptr, 128, 608, 4096, 4096, 4096, 640, 3, 256, 0, 0, 0, 0, 0, 3, nullptr) == VQS_ERR_INVALID);
    {
        int dummy2 = 0;
        assert(vqs_debug_gemm_batched(&dummy2, &dummy2, &dummy2, 128, 608, 4096, 4096, 4096, 640, 5, 256, 0, 0, 0, 0, 0, 3, nullptr) == VQS_ERR_INVALID);   // gated: not a batched debug epilogue
        assert(vqs_debug_gemm_batched(&dummy2, &dummy2, &dummy2, 128, 608, 4096, 4096, 4096, 640, 3, 0, 0, 0, 0, 0, 0, 3, nullptr) == VQS_ERR_INVALID);     // batch < 1
    }
    {   // the single-launch hooks of the Qwen2.5-VL prefill's glue and of the range proof: every refusal is host code, before any device call
        int d = 0;
        float f = 0.f;
        const int I = VQS_ERR_INVALID;
        // scaled RMSNorm: null operands, D % 4, a pitch below D or off the 4-element grid, the unstored form with a bf16 operand, delta2 without delta
        assert(vqs_debug_rmsnorm_f16s(nullptr, nullptr, nullptr, 1, &d, &d, 0, 4, 1280, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, nullptr, nullptr, 1, nullptr, &d, 0, 4, 1280, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, nullptr, nullptr, 1, &d, nullptr, 0, 4, 1280, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, nullptr, nullptr, 1, &d, &d, 0, 0, 1280, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, nullptr, nullptr, 1, &d, &d, 0, 4, 1282, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, nullptr, nullptr, 1, &d, &d, 1276, 4, 1280, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, nullptr, nullptr, 1, &d, &d, 1282, 4, 1280, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, &d, nullptr, 0, &d, &d, 0, 4, 1280, 1e-6f, 1.f, 1.f, 1.f, 1, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, nullptr, &d, 1, &d, &d, 0, 4, 1280, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        assert(vqs_debug_rmsnorm_f16s(&f, &d, &d, 0, &d, &d, 0, 4, 1280, 1e-6f, 1.f, 1.f, 1.f, 0, nullptr) == I);
        // rope_qk: an fp16 half off the 16-byte grid, an odd half, a rotation wider than the head
        assert(vqs_debug_rope_qk(nullptr, &d, &f, &f, 2, 4, 2, 33, 128, 64, 0, nullptr) == I && vqs_debug_rope_qk(&d, &d, nullptr, &f, 2, 4, 2, 33, 128, 64, 0, nullptr) == I);
        assert(vqs_debug_rope_qk(&d, &d, &f, &f, 2, 4, 2, 33, 128, 36, 1, nullptr) == I && vqs_debug_rope_qk(&d, &d, &f, &f, 2, 4, 2, 33, 128, 41, 0, nullptr) == I);
        assert(vqs_debug_rope_qk(&d, &d, &f, &f, 2, 4, 2, 33, 128, 72, 0, nullptr) == I && vqs_debug_rope_qk(&d, &d, &f, &f, 2, 4, 0, 33, 128, 64, 0, nullptr) == I);
        assert(vqs_debug_qwen_embed(nullptr, &d, &d, &d, &f, 4, 128, 16, 0, 1.f, nullptr) == I && vqs_debug_qwen_embed(&d, nullptr, &d, &d, &f, 4, 128, 16, 0, 1.f, nullptr) == I);
        assert(vqs_debug_qwen_embed(&d, &d, &d, &d, &f, 0, 128, 16, 0, 1.f, nullptr) == I && vqs_debug_qwen_embed(&d, &d, &d, &d, &f, 4, 128, 0, 0, 1.f, nullptr) == I);
        // the gathers check nothing themselves: the hook refuses null tensors, empty shapes and a pitch narrower than the row
        assert(vqs_debug_gather_rows_bf16(nullptr, nullptr, nullptr, &d, 4, 64, 64, 64, nullptr) == I && vqs_debug_gather_rows_bf16(&d, nullptr, nullptr, nullptr, 4, 64, 64, 64, nullptr) == I);
        assert(vqs_debug_gather_rows_bf16(&d, nullptr, nullptr, &d, 0, 64, 64, 64, nullptr) == I && vqs_debug_gather_rows_bf16(&d, nullptr, nullptr, &d, 4, 0, 64, 64, nullptr) == I);
        assert(vqs_debug_gather_rows_bf16(&d, nullptr, nullptr, &d, 4, 64, 64, 63, nullptr) == I && vqs_debug_gather_rows_bf16(&d, nullptr, nullptr, &d, 4, 64, 63, 64, nullptr) == I);
        assert(vqs_debug_gather_cols_bf16(nullptr, &d, &d, 4, 64, 32, nullptr) == I && vqs_debug_gather_cols_bf16(&d, nullptr, &d, 4, 64, 32, nullptr) == I &&
               vqs_debug_gather_cols_bf16(&d, &d, nullptr, 4, 64, 32, nullptr) == I);
        assert(vqs_debug_gather_cols_bf16(&d, &d, &d, 0, 64, 32, nullptr) == I && vqs_debug_gather_cols_bf16(&d, &d, &d, 4, 64, 0, nullptr) == I);
        assert(vqs_debug_gather_rows_f32(nullptr, &d, &f, 4, 64, 64, 0, nullptr) == I && vqs_debug_gather_rows_f32(&f, nullptr, &f, 4, 64, 64, 1, nullptr) == I);
        assert(vqs_debug_gather_rows_f32(&f, &d, &f, 0, 64, 64, 0, nullptr) == I && vqs_debug_gather_rows_f32(&f, &d, &f, 4, 0, 64, 1, nullptr) == I);
        assert(vqs_debug_gather_rows_f32(&f, &d, &f, 4, 64, 64, 2, nullptr) == I && vqs_debug_gather_rows_f32(&f, &d, &f, 4, 64, 68, 0, nullptr) == I);     // no such form; form 0 is dense
        assert(vqs_debug_gather_rows_f32(&f, &d, &f, 4, 66, 66, 0, nullptr) == I && vqs_debug_gather_rows_f32(&f, &d, &f, 4, 66, 68, 1, nullptr) == I);     // cols % 4
        assert(vqs_debug_gather_rows_f32(&f, &d, &f, 4, 64, 60, 1, nullptr) == I && vqs_debug_gather_rows_f32(&f, &d, &f, 4, 64, 66, 1, nullptr) == I);     // src_ld < cols, src_ld % 4
        assert(vqs_debug_f16_to_bf16_rows(nullptr, &d, 4, 128, 128, 256, 1.f, nullptr) == I && vqs_debug_f16_to_bf16_rows(&d, nullptr, 4, 128, 128, 256, 1.f, nullptr) == I);
        assert(vqs_debug_f16_to_bf16_rows(&d, &d, 4, 124, 128, 256, 1.f, nullptr) == I && vqs_debug_f16_to_bf16_rows(&d, &d, 65536, 128, 128, 256, 1.f, nullptr) == I);
        assert(vqs_debug_f16_to_bf16_rows(&d, &d, 0, 128, 128, 256, 1.f, nullptr) == I && vqs_debug_f16_to_bf16_rows(&d, &d, 4, 128, 128, 120, 1.f, nullptr) == I);
        assert(vqs_debug_qwen_tail_rope_q(nullptr, 1024, &f, &f, &d, &f, 2, 4, 128, 64, nullptr) == I && vqs_debug_qwen_tail_rope_q(&f, 1024, &f, &f, nullptr, &f, 2, 4, 128, 64, nullptr) == I);
        assert(vqs_debug_qwen_tail_rope_q(&f, 1024, &f, &f, &d, &f, 2, 4, 256, 72, nullptr) == I && vqs_debug_qwen_tail_rope_q(&f, 1024, &f, &f, &d, &f, 2, 4, 64, 40, nullptr) == I);
        assert(vqs_debug_qwen_tail_rope_q(&f, 1024, &f, &f, &d, &f, 0, 4, 128, 64, nullptr) == I && vqs_debug_qwen_tail_rope_q(&f, 500, &f, &f, &d, &f, 2, 4, 128, 64, nullptr) == I);
        // range proof: empty shapes, a mode without its operands, no slot, a pitch below K
        assert(vqs_debug_rowbound(nullptr, 64, 4, 64, 0, &d, 64, 1.f, nullptr, nullptr, nullptr, &f, &f, nullptr) == I && vqs_debug_rowbound(&d, 64, 0, 64, 0, &d, 64, 1.f, nullptr, nullptr, nullptr, &f, &f, nullptr) == I);
        assert(vqs_debug_rowbound(&d, 64, 4, 0, 0, &d, 64, 1.f, nullptr, nullptr, nullptr, &f, &f, nullptr) == I && vqs_debug_rowbound(&d, 64, 4, 64, 0, nullptr, 64, 1.f, nullptr, nullptr, nullptr, &f, &f, nullptr) == I);
        assert(vqs_debug_rowbound(&d, 64, 4, 64, 0, &d, 0, 1.f, nullptr, nullptr, nullptr, &f, &f, nullptr) == I && vqs_debug_rowbound(&d, 64, 4, 64, 1, nullptr, 0, 0.f, nullptr, nullptr, nullptr, &f, &f, nullptr) == I);
        assert(vqs_debug_rowbound(&d, 64, 4, 64, 1, nullptr, 0, 0.f, &f, nullptr, nullptr, &f, nullptr, nullptr) == I && vqs_debug_rowbound(&d, 60, 4, 64, 1, nullptr, 0, 0.f, &f, nullptr, nullptr, &f, &f, nullptr) == I);
        assert(vqs_debug_rowbound(&d, 64, 4, 64, 2, &d, 64, 1.f, &f, nullptr, nullptr, &f, &f, nullptr) == I);
        assert(vqs_debug_absmax_bf16(nullptr, 64, 1.f, &f, nullptr) == I && vqs_debug_absmax_bf16(&d, 0, 1.f, &f, nullptr) == I && vqs_debug_absmax_bf16(&d, 64, 1.f, nullptr, nullptr) == I);
        assert(vqs_debug_gate_pair_bound(nullptr, 32, 32, &f, &f, nullptr) == I && vqs_debug_gate_pair_bound(&f, 48, 64, &f, &f, nullptr) == I && vqs_debug_gate_pair_bound(&f, 64, 32, &f, &f, nullptr) == I);
        assert(vqs_debug_gate_pair_bound(&f, 0, 32, &f, &f, nullptr) == I && vqs_debug_gate_pair_bound(&f, 32, 32, nullptr, &f, nullptr) == I && vqs_debug_gate_pair_bound(&f, 32, 32, &f, nullptr, nullptr) == I);
    }
    assert(vqs_debug_gemm_form(400000, 4096, 10240, 10240, 10240, 3, 1, 3, 0, 0, 0) == 0 && vqs_debug_gemm_form(400000, 4096, 10240, 10240, 10240, 3, 2, 3, 0, 0, 0) == -1);
    int64_t ld = 0;
    assert(vqs_workspace_offset(h, "logits", 4, 33, 2, &ld) >= 0 && ld == 32128);
    assert(vqs_workspace_offset(h, "dec_out", 4, 33, 2, &ld) >= 0 && vqs_workspace_offset(h, "nope", 4, 33, 2, &ld) < 0);
    assert(vqs_workspace_offset(h, "vit_hidden", 4, 0, 0, &ld) >= 0);
    // calls that must fail cleanly before any device access
    assert(vqs_score(h, &dummy, nullptr, nullptr, nullptr, 1, 33, 2, nullptr, nullptr, nullptr, 0, nullptr) != 0);
    assert(vqs_encode_images(h, &dummy, 1, &dummy, &dummy, 16, nullptr) != 0);      // weights not bound
    assert(vqs_bind_weights(h, nullptr, 0, nullptr, 0, nullptr) != 0);
    for (int rel = -700; rel <= 700; ++rel) {
        const int b = vqs_relpos_bucket(rel, 1, 32, 128), u = vqs_relpos_bucket(rel, 0, 32, 128);
        assert(b >= 0 && b < 32 && u >= 0 && u < 32);
    }
    std::vector<int64_t> off(64);
    assert(vqs_debug_heads_rows(5, 608, 64, 64, 64, off.data()) == 0 && vqs_debug_heads_rows(5, 7, 64, 64, 4, off.data()) != 0);
    assert(vqs_attention_lds_bytes(608, 1, 64) > 0 && vqs_attention_lds_bytes(608, 1, 77) < 0);
    // tile order: option parsing (per-shape table, removal, malformed names / values) and the host walk of the tile map
    assert(vqs_set_option(h, "tile_order:20480x4096", 4 | 2 << 8) == 0 && vqs_set_option(h, "tile_order:20480x4096", 2) == 0);
    assert(vqs_set_option(h, "tile_order:20480x4096", 0) == 0 && vqs_set_option(h, "tile_order:4096x10240", 0) == 0);
    assert(vqs_set_option(h, "tile_order:", 8) != 0 && vqs_set_option(h, "tile_order:12x", 8) != 0 && vqs_set_option(h, "tile_order:-4x64", 8) != 0);
    assert(vqs_set_option(h, "tile_order:64x64", 65) != 0 && vqs_set_option(h, "tile_order:64x64", 1 << 16) != 0 && vqs_set_option(h, "tile_order:64x64", 8 | 9 << 8) != 0);
    assert(vqs_set_option(h, "nt_store:4096x10240", 1) == 0 && vqs_set_option(h, "nt_store:4096x10240", 2) == 0 && vqs_set_option(h, "nt_store:4096x10240", 0) == 0);
    assert(vqs_set_option(h, "nt_store:4096x10240", 3) != 0 && vqs_set_option(h, "nt_store:x", 1) != 0);
    assert(vqs_set_option(h, "l2_touch:12288x4096", 1) == 0 && vqs_set_option(h, "l2_touch:12288x4096", 0) == 0 && vqs_set_option(h, "l2_touch:12288x4096", 5) != 0);
    assert(vqs_set_option(h, "gemm_variant", 11) == 0 && vqs_set_option(h, "gemm_variant", 3) == 0 && vqs_set_option(h, "gemm_variant", 6) != 0 && vqs_set_option(h, "gemm_variant", 8) != 0);
    {
        const int M = 155648, N = 20480, nwg = (M / 256) * (N / 256);
        std::vector<int32_t> tiles(4 * (size_t)nwg);
        assert(vqs_debug_tile_order(M, N, 4096, 1, 4, 2, 256, tiles.data()) == (4 | 2 << 8));
        assert(vqs_debug_tile_order(M, N, 4096, 1, 0, 0, 256, tiles.data()) == (4 | 2 << 8));
        assert(vqs_debug_tile_order(577 * 256, 1024, 1024, 1, 8, 2, 256, tiles.data()) == (8 | 1 << 8));     // 577 x 2 tiles per range: remainders -> ns = 1
        assert(vqs_debug_tile_order(M, N, 4096, 1, 4, 2, 250, tiles.data()) < 0 && vqs_debug_tile_order(0, N, 4096, 1, 4, 2, 256, tiles.data()) < 0);
    }
    vqs_destroy(h);
    vqs_config bad = c;
    bad.d_kv = 32;
    vqs_handle* hb = nullptr;
    assert(vqs_create(&bad, &hb) != 0);
    vqs_destroy(hb);
    assert(vqs_create(nullptr, &hb) != 0);
    {   // Qwen2.5-VL row: sizes, options and the calls that must fail cleanly before any device access
        vqs_qwen_config q;
        memset(&q, 0, sizeof q);
        q.v_depth = 32; q.v_hidden = 1280; q.v_heads = 16; q.v_mlp = 3420; q.v_patch_dim = 1176; q.v_merge_unit = 4; q.v_out_hidden = 3584;
        q.v_fullatt_mask = (1 << 7) | (1 << 15) | (1 << 23) | (int32_t)(1u << 31); q.v_eps = 1e-6f;
        q.t_vocab = 152064; q.t_hidden = 3584; q.t_layers = 28; q.t_heads = 28; q.t_kv_heads = 4; q.t_mlp = 18944; q.t_eps = 1e-6f;
        vqs_qwen_handle* qh = nullptr;
        assert(vqs_qwen_create(&q, &qh) == 0 && qh);
        assert(vqs_qwen_packed_bytes(qh) > 0);
        assert(vqs_qwen_vision_workspace_bytes(qh, 3072, 3072) > 0 && vqs_qwen_vision_workspace_bytes(qh, 3071, 3072) == 0);
        assert(vqs_qwen_score_workspace_bytes(qh, 64, 808) > 0 && vqs_qwen_score_workspace_bytes(qh, 0, 808) == 0);
        // KV cache: 28 layers x (K, V) x [B, 4, Lmax, 128] bf16
        assert(vqs_qwen_kv_bytes(qh, 64, 816) == (size_t)2 * 28 * 64 * 4 * 816 * 128 * 2 && vqs_qwen_kv_bytes(qh, 0, 816) == 0);
        assert(vqs_qwen_decode_workspace_bytes(qh, 64) > 0 && vqs_qwen_decode_workspace_bytes(qh, 0) == 0);
        assert(vqs_qwen_debug_option(qh, "x_pitch", 4096) == 0 && vqs_qwen_debug_option(qh, "x_pitch", 3584) == 0);
        assert(vqs_qwen_debug_option(qh, "x_pitch", 3000) != 0 && vqs_qwen_debug_option(qh, "x_pitch", 3600) != 0 && vqs_qwen_debug_option(qh, "nope", 1) != 0);
        assert(strlen(vqs_qwen_last_error(qh)) > 0);
        assert(vqs_qwen_debug_tap(qh, "txt.3.xn0", &dummy, 4) == 0 && vqs_qwen_debug_tap(qh, nullptr, nullptr, 0) == 0);
        assert(vqs_qwen_decode(qh, &dummy, &dummy, nullptr, nullptr, 1, 16, &dummy, 1 << 20, nullptr, &dummy, 1 << 20, nullptr) != 0);   // not bound
        assert(vqs_qwen_prefill(qh, &dummy, &dummy, &dummy, &dummy, &dummy, nullptr, nullptr, 1, 16, nullptr, &dummy, 16, nullptr, 0, 16, nullptr) != 0);
        assert(vqs_qwen_prefill(qh, &dummy, &dummy, &dummy, &dummy, &dummy, nullptr, nullptr, 1, 16, nullptr, &dummy, 16, &dummy, 16, 8, nullptr) != 0);   // Lmax < L
        // a cache longer than the decode kernel can address is refused by the prefill itself, before anything is launched
        assert(vqs_qwen_prefill(qh, &dummy, &dummy, &dummy, &dummy, &dummy, nullptr, nullptr, 1, 16, nullptr, &dummy, 16, &dummy, (size_t)-1,
                                VQS_QWEN_MAX_CACHE_POSITIONS + 1, nullptr) == VQS_ERR_INVALID);
        assert(strstr(vqs_qwen_last_error(qh), "cache positions") != nullptr);
        assert(vqs_qwen_score(qh, &dummy, &dummy, &dummy, &dummy, &dummy, nullptr, nullptr, 1, 16, nullptr, &dummy, 16, nullptr) != 0);
        vqs_qwen_destroy(qh);
        q.t_heads = 27;        // hidden not divisible by heads
        assert(vqs_qwen_create(&q, &qh) != 0);
    }
    {   // CLIPScore row (ViT-L/14-336): sizes, options, refused configurations and the passes that must fail cleanly before any device access
        vqs_clip_config k;
        memset(&k, 0, sizeof k);
        k.vis_hidden = 1024; k.vis_layers = 24; k.vis_heads = 16; k.vis_mlp = 4096; k.vis_patch = 14; k.vis_image = 336; k.vis_eps = 1e-5f;
        k.txt_hidden = 768; k.txt_layers = 12; k.txt_heads = 12; k.txt_mlp = 3072; k.txt_vocab = 49408; k.txt_context = 77; k.txt_eps = 1e-5f;
        k.embed_dim = 768;
        vqs_clip_handle* kh = nullptr;
        assert(vqs_clip_create(&k, &kh) == 0 && kh);
        assert(vqs_clip_packed_bytes(kh) > 0 && vqs_clip_packed_bytes(nullptr) == 0);
        assert(vqs_clip_image_workspace_bytes(kh, 256) > 0 && vqs_clip_image_workspace_bytes(kh, 0) == 0);
        assert(vqs_clip_text_workspace_bytes(kh, 256, 77) > 0 && vqs_clip_text_workspace_bytes(kh, 4, 8) > 0);
        assert(vqs_clip_text_workspace_bytes(kh, 4, 78) == 0 && vqs_clip_text_workspace_bytes(kh, 4, 7) == 0 && vqs_clip_text_workspace_bytes(kh, 0, 77) == 0);
        {
            int32_t v = -1;
            assert(vqs_clip_get_option(kh, "fp16", &v) == 0 && v == 1 && vqs_clip_get_option(kh, "norm_defer", &v) == 0 && v == 1);
            assert(vqs_clip_set_option(kh, "fp16", 0) == 0 && vqs_clip_get_option(kh, "fp16", &v) == 0 && v == 0 && vqs_clip_set_option(kh, "fp16", 1) == 0);
            assert(vqs_clip_set_option(kh, "fp16", 2) != 0 && strlen(vqs_clip_last_error(kh)) > 0);
            assert(vqs_clip_set_option(kh, "vit_fp16", 1) != 0 && vqs_clip_set_option(kh, nullptr, 1) != 0 && vqs_clip_set_option(nullptr, "fp16", 1) != 0);
            assert(vqs_clip_get_option(kh, "nonsense", &v) != 0 && vqs_clip_get_option(kh, "fp16", nullptr) != 0 && vqs_clip_get_option(nullptr, "fp16", &v) != 0);
        }
        float emb = 0.f;
        assert(vqs_clip_encode_images(kh, &dummy, 1, &emb, &dummy, (size_t)1 << 40, nullptr) == VQS_ERR_STATE);      // weights not bound
        assert(strstr(vqs_clip_last_error(kh), "not bound") != nullptr);
        assert(vqs_clip_encode_texts(kh, &dummy, &dummy, 1, 77, &emb, &dummy, (size_t)1 << 40, nullptr) == VQS_ERR_STATE);
        assert(strstr(vqs_clip_last_error(kh), "encode_texts") != nullptr && strstr(vqs_clip_last_error(kh), "not bound") != nullptr);
        assert(vqs_clip_encode_images(nullptr, &dummy, 1, &emb, &dummy, 16, nullptr) == VQS_ERR_INVALID);
        assert(vqs_clip_bind_weights(kh, nullptr, 0, nullptr, 0, nullptr) == VQS_ERR_INVALID && strlen(vqs_clip_last_error(kh)) > 0);
        vqs_clip_destroy(kh);
        // refused configurations: the handle comes back (for its message), sizes as 0, and binds to nothing
        struct { int32_t vqs_clip_config::*field; int32_t value; const char* word; } bad_cfg[] = {
            {&vqs_clip_config::txt_heads, 16, "text head dim"}, {&vqs_clip_config::vis_heads, 8, "vision head dim"},
            {&vqs_clip_config::txt_context, 129, "txt_context"}, {&vqs_clip_config::vis_image, 330, "multiple of the patch"},
            {&vqs_clip_config::embed_dim, 770, "embed_dim"}, {&vqs_clip_config::txt_layers, 0, "layer counts"}};
        for (const auto& b : bad_cfg) {
            vqs_clip_config kb = k;
            kb.*(b.field) = b.value;
            vqs_clip_handle* hb2 = nullptr;
            assert(vqs_clip_create(&kb, &hb2) == VQS_ERR_INVALID && hb2 && strstr(vqs_clip_last_error(hb2), b.word) != nullptr);
            assert(vqs_clip_packed_bytes(hb2) == 0 && vqs_clip_image_workspace_bytes(hb2, 1) == 0 && vqs_clip_text_workspace_bytes(hb2, 1, 77) == 0);
            assert(vqs_clip_bind_weights(hb2, nullptr, 0, nullptr, 0, nullptr) == VQS_ERR_STATE);
            vqs_clip_destroy(hb2);
        }
        assert(vqs_clip_create(nullptr, &kh) != 0 && strcmp(vqs_clip_last_error(nullptr), "null handle") == 0);
        vqs_clip_destroy(nullptr);
    }
    printf("host ABI exercise under ASan/UBSan: ok\n");
    return 0;
}
