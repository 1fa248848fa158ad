// Host support shared by the three engine handles of libvqs_hip (vqs_handle in vqs_api.cpp, vqs_qwen_handle in vqs_qwen.cpp,
// vqs_clip_handle in vqs_clip.cpp) and by the tower block loop of vqs_blocks.h: one handle base (error string, weight table,
// stage taps, GEMM profile), one set of error macros, one workspace carver, one GEMM call path, one tap set, one profile state.
// What a handle owns itself -- configuration, layouts, packing, launch sequences, options -- stays in its .cpp.
// No device allocation; the stream is synchronised nowhere but in profile_read (behind the *_profile_read entry points).
#pragma once
#include "../../include/vqs.h"
#include "vqs_kernels.h"

#include <hip/hip_runtime.h>

#include <array>
#include <cstdio>
#include <map>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

namespace vqs {

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Carves regions out of a caller buffer, every region 256-byte aligned; with base == nullptr it only measures (sizing queries,
// packed layouts).  `names` (optional) receives the offsets of the named regions (vqs_workspace_offset).
struct Carver {
    char* base;
    size_t off = 0;
    std::unordered_map<std::string, size_t>* names = nullptr;
    size_t mark(size_t bytes, const char* name = nullptr) {      // -> the region's offset
        off = align_up(off);
        const size_t o = off;
        if (names && name) (*names)[name] = o;
        off += bytes;
        return o;
    }
    template <typename T>
    T* take(size_t n, const char* name = nullptr) {
        const size_t o = mark(n * sizeof(T), name);
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
    size_t total() const { return align_up(off); }
};

// Stage taps (vqs_debug_tap / vqs_qwen_debug_tap): point name -> caller buffer; a pass copies the named intermediate there.
struct TapSet {
    struct Tap { void* dst; size_t cap; };
    std::unordered_map<std::string, Tap> map;
    // window (vqs_debug_tap_window): taps copy outer entries [first, first + count) of `outer` (pairs of the running T5 pass /
    // images of the running vision pass; set by the pass); count == 0: whole tensors
    int first = 0, count = 0, outer = 0;
    void set(const char* name, void* dst, size_t bytes) {        // register; no buffer: erase; no name: clear
        if (!name) map.clear();
        else if (!dst || bytes == 0) map.erase(name);
        else map[name] = Tap{dst, bytes};
    }
};

// GEMM launch timing behind the bench's roofline numbers: HIP events on the launch stream around every profiled launch, the
// launches' FLOPs and algorithmic bytes, the per-call-site labels of vqs_profile_report.
struct GemmProfile {
    bool on = false;
    std::vector<hipEvent_t> ev;
    size_t used = 0;
    std::vector<std::pair<std::string, double>> what;      // per profiled launch: call-site label, FLOPs
    double flops = 0.0, bytes = 0.0;
    std::string report;
    GemmProfile() = default;
    GemmProfile(const GemmProfile&) = delete;
    GemmProfile& operator=(const GemmProfile&) = delete;
    ~GemmProfile() { for (hipEvent_t e : ev) (void)hipEventDestroy(e); }      // the one place events die: every *_destroy deletes its handle
};

struct HostBase {
    struct Weight { const bf16_t* p; int64_t numel; };
    std::string err;
    std::unordered_map<std::string, Weight> w;
    bool bound = false;
    // what get_w answers to a wrong element count.  The Qwen handle has always said VQS_ERR_MISSING_WEIGHT there and callers may
    // depend on it; a deliberate quirk kept as it is, not a choice to copy
    int numel_code = VQS_ERR_INVALID;
    TapSet taps;
    GemmProfile prof;
};

inline int fail(HostBase* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

// hipError_t -> ABI code of the single-kernel entry points whose launchers validate their arguments
inline int abi_code(hipError_t e) { return e == hipSuccess ? VQS_OK : e == hipErrorInvalidValue ? VQS_ERR_INVALID : VQS_ERR_HIP; }

#define VQS_HIP(h, expr, what)                                                                                       \
    do {                                                                                                             \
        hipError_t _e = (expr);                                                                                      \
        if (_e != hipSuccess) return vqs::fail((h), VQS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(_e));  \
    } while (0)
#define VQS_RUN(expr)                \
    do {                             \
        int _r = (expr);             \
        if (_r != VQS_OK) return _r; \
    } while (0)

// (Re)fill the weight table from the descriptors of a *_bind_weights call (vqs_weight_desc / vqs_clip_weight_desc: same layout).
template <class Desc>
int set_weights(HostBase* h, const Desc* d, int n) {
    h->w.clear();
    for (int i = 0; i < n; ++i) {
        if (!d[i].name || !d[i].d_data) return fail(h, VQS_ERR_INVALID, "bind_weights: null entry");
        h->w[d[i].name] = HostBase::Weight{(const bf16_t*)d[i].d_data, d[i].numel};
    }
    return VQS_OK;
}

inline int get_w(HostBase* h, const std::string& name, int64_t numel, const bf16_t** out) {
    auto it = h->w.find(name);
    if (it == h->w.end()) return fail(h, VQS_ERR_MISSING_WEIGHT, "missing weight: " + name);
    if (it->second.numel != numel)
        return fail(h, h->numel_code, "weight " + name + ": numel " + std::to_string(it->second.numel) + " != expected " + std::to_string(numel));
    *out = it->second.p;
    return VQS_OK;
}
// declares `var`; uses the `h` in scope
#define VQS_W(var, name, numel)  \
    const vqs::bf16_t* var = nullptr; \
    VQS_RUN(vqs::get_w(h, (name), (int64_t)(numel), &var))

// ------------------------------------------------------------------------------------------------------------------ GEMM
// One launch as the launch sequences describe it; the fields are those of GemmParams (vqs_kernels.h) under the same names.
struct GemmCall {
    const bf16_t* A;
    const bf16_t* W;
    void* C;
    const bf16_t* bias = nullptr;
    const float* resid = nullptr;
    int M = 0, N = 0, K = 0;
    int lda = 0, ldw = 0, ldc = 0;
    int epi = 0;
    int S = 0, H = 0, inner = 0;
    int hd = 0, hd_src = 0, inner_kv = 0, Hkv = 0, gate_act = 0;
    bf16_t* heads[3] = {nullptr, nullptr, nullptr};
    int batch = 1;
    long long sA = 0, sW = 0, sC = 0;
    // fused residual + RMSNorm
    float* hres = nullptr;
    int ldh = 0;
    const bf16_t* lnw = nullptr;
    float* rowss_out = nullptr;
    const float* rowss_in = nullptr;
    int rowss_parts = 0;
    float rs_invd = 0.0f, rs_eps = 0.0f;
    int nt_store = 0;          // result rows leave with the non-temporal hint (call sites whose multi-GB output is streamed once)
    long long split_off = 0;   // EPI_BF16: also store the lo plane of a split-bf16 result at C + split_off
    float acc_scale = 1.0f, out_scale = 1.0f;                 // f16 = 3 / 4: the scaled quad families
    const float *rope_cos = nullptr, *rope_sin = nullptr;     // f16 = 3, EPI_HEADS: rotary embedding in the epilogue
    int no_stream = 0;         // 1: keep this launch off the stream form (same bits either way)
    int f16 = 0;               // operand / result types, as GemmParams::f16
};

// What the handle decides about a launch (all but `variant` bitwise-neutral): the defaults are what the Qwen and CLIPScore handles run.
struct GemmOpts {
    int variant = 3;           // option gemm_variant (GemmVariant; what it selects: gemm.hip gemm_plan)
    bool stream = true;        // option stream_gemm
    int tile_gm = 0, tile_ns = 0, l2_touch = 0;
    int nt_store = -1;         // -1: the call site's choice
};

inline GemmParams gemm_params(const GemmCall& g, const GemmOpts& o) {
    GemmParams p{};
    p.A = g.A; p.W = g.W; p.C = g.C; p.bias = g.bias; p.resid = g.resid;
    p.M = g.M; p.N = g.N; p.K = g.K; p.lda = g.lda; p.ldw = g.ldw; p.ldc = g.ldc;
    p.S = g.S > 0 ? g.S : 1; p.H = g.H; p.inner = g.inner > 0 ? g.inner : 1;
    p.heads_out[0] = g.heads[0]; p.heads_out[1] = g.heads[1]; p.heads_out[2] = g.heads[2];
    p.hd = g.hd; p.hd_src = g.hd_src; p.inner_kv = g.inner_kv; p.Hkv = g.Hkv; p.gate_act = g.gate_act;
    p.batch = g.batch; p.sA = g.sA; p.sW = g.sW; p.sC = g.sC;
    p.hres = g.hres; p.ldh = g.ldh; p.lnw = g.lnw; p.rowss_out = g.rowss_out;
    p.rowss_in = g.rowss_in; p.rowss_parts = g.rowss_parts; p.rs_invd = g.rs_invd; p.rs_eps = g.rs_eps;
    p.split_off = g.split_off;
    p.f16 = g.f16; p.acc_scale = g.acc_scale; p.out_scale = g.out_scale;
    p.rope_cos = g.rope_cos; p.rope_sin = g.rope_sin;
    p.tile_gm = o.tile_gm; p.tile_ns = o.tile_ns; p.l2_touch = o.l2_touch;
    p.nt_store = o.nt_store >= 0 ? o.nt_store : g.nt_store;
    p.no_stream = (o.stream && !g.no_stream) ? 0 : 1;
    return p;
}

// Launch; with the profile on, an event pair around the launch and its FLOPs / bytes (every operand read once, every result
// written once) on the counters.
inline int run_gemm(HostBase* h, const GemmCall& g, const GemmOpts& o, hipStream_t st, const char* what) {
    const GemmParams p = gemm_params(g, o);
    GemmProfile& pr = h->prof;
    if (pr.on) {
        while (pr.ev.size() < pr.used + 2) {
            hipEvent_t e;
            VQS_HIP(h, hipEventCreate(&e), "hipEventCreate");
            pr.ev.push_back(e);
        }
        VQS_HIP(h, hipEventRecord(pr.ev[pr.used], st), "hipEventRecord");
    }
    VQS_HIP(h, launch_gemm(p, g.epi, o.variant, st, true), std::string("gemm ") + what);
    if (pr.on) {
        VQS_HIP(h, hipEventRecord(pr.ev[pr.used + 1], st), "hipEventRecord");
        pr.used += 2;
        const double flops = 2.0 * (double)g.M * (double)g.N * (double)g.K * (double)g.batch;
        const double out_b = (g.epi == EPI_F32 || g.epi == EPI_F32_RESID) ? 4.0 : (g.epi == EPI_RESID_RMS ? 10.0 : 2.0);
        const double out_n = (g.epi == EPI_GATED) ? 0.5 * (double)g.N : (double)g.N;
        pr.what.emplace_back(what, flops);
        pr.flops += flops;
        pr.bytes += (double)g.batch * (2.0 * ((double)g.M + (double)g.N) * (double)g.K + out_b * (double)g.M * out_n);
    }
    return VQS_OK;
}

// The one place the stream's events are waited for.  -> number of profiled launches (or an error code); also rebuilds the
// per-label report.  Any of the three outputs may be nullptr.
inline int profile_read(HostBase* h, double* gemm_ms, double* gemm_flops, double* gemm_bytes, bool reset) {
    GemmProfile& pr = h->prof;
    double ms = 0.0;
    std::map<std::string, std::array<double, 3>> by;      // label -> {launches, ms, flops}
    for (size_t i = 0; i + 1 < pr.used; i += 2) {
        VQS_HIP(h, hipEventSynchronize(pr.ev[i + 1]), "hipEventSynchronize");
        float t = 0.f;
        VQS_HIP(h, hipEventElapsedTime(&t, pr.ev[i], pr.ev[i + 1]), "hipEventElapsedTime");
        ms += t;
        if (i / 2 < pr.what.size()) {
            auto& a = by[pr.what[i / 2].first];
            a[0] += 1.0; a[1] += t; a[2] += pr.what[i / 2].second;
        }
    }
    pr.report.clear();
    for (const auto& kv : by) {
        char line[256];
        snprintf(line, sizeof line, "%-20s launches %6.0f  ms %10.3f  TFLOP/s %8.1f\n", kv.first.c_str(), kv.second[0], kv.second[1],
                 kv.second[1] > 0 ? kv.second[2] / kv.second[1] / 1e9 : 0.0);
        pr.report += line;
    }
    if (gemm_ms) *gemm_ms = ms;
    if (gemm_flops) *gemm_flops = pr.flops;
    if (gemm_bytes) *gemm_bytes = pr.bytes;
    const int n = (int)(pr.used / 2);
    if (reset) {
        pr.used = 0;
        pr.what.clear();
        pr.flops = 0.0;
        pr.bytes = 0.0;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------------------------ taps
// Copy an intermediate to a caller buffer registered as "<stack>[.<layer>].<what>" (in-stream, device to device).  The workspace
// buffers are reused layer after layer, so the tests that check EVERY launch of a pass against the oracle on the engine's own
// inputs (tests/test_gpu_stage_locked.py, tests/test_gpu_qwen.py) read them through this.  With nothing registered each of the
// three costs one empty() test.
inline const TapSet::Tap* find_tap(HostBase* h, const char* stack, int layer, const char* what, std::string& name) {
    name = layer >= 0 ? std::string(stack) + "." + std::to_string(layer) + "." + what : std::string(stack) + "." + what;
    auto it = h->taps.map.find(name);
    return it == h->taps.map.end() ? nullptr : &it->second;
}
// every intermediate is outer-entry-major: the window is one contiguous byte range [first, first + bytes) of its `bytes`
inline int tap_window(HostBase* h, const std::string& name, size_t& first, size_t& bytes) {
    const TapSet& t = h->taps;
    first = 0;
    if (t.count == 0) return VQS_OK;
    if (t.outer <= 0 || t.first + t.count > t.outer || bytes % (size_t)t.outer != 0)
        return fail(h, VQS_ERR_INVALID, "tap " + name + ": window [" + std::to_string(t.first) + ", +" + std::to_string(t.count) +
                                        ") does not fit " + std::to_string(t.outer) + " outer entries");
    const size_t per = bytes / (size_t)t.outer;
    first = per * (size_t)t.first;
    bytes = per * (size_t)t.count;
    return VQS_OK;
}
inline int tap_fits(HostBase* h, const std::string& name, const TapSet::Tap& t, size_t bytes) {
    return t.cap >= bytes ? VQS_OK : fail(h, VQS_ERR_WORKSPACE, "tap " + name + ": buffer too small (" + std::to_string(bytes) + " bytes needed)");
}

// dense tensor (or its window)
inline int tap(HostBase* h, const char* stack, int layer, const char* what, const void* src, size_t bytes, hipStream_t st) {
    if (h->taps.map.empty()) return VQS_OK;
    std::string name;
    const TapSet::Tap* t = find_tap(h, stack, layer, what, name);
    if (!t) return VQS_OK;
    size_t first;
    VQS_RUN(tap_window(h, name, first, bytes));
    VQS_RUN(tap_fits(h, name, *t, bytes));
    VQS_HIP(h, hipMemcpyAsync(t->dst, static_cast<const char*>(src) + first, bytes, hipMemcpyDeviceToDevice, st), "tap copy");
    return VQS_OK;
}
// A split-bf16 tensor (planes [2][rows][width], `plane` elements apart) goes to its tap buffer as two planes of the tapped rows:
// [2][window rows][width] bf16; the reader adds them (tests/gpu_util.py).
inline int tap_split(HostBase* h, const char* stack, int layer, const char* what, const bf16_t* src, size_t plane, hipStream_t st) {
    if (h->taps.map.empty()) return VQS_OK;
    std::string name;
    const TapSet::Tap* t = find_tap(h, stack, layer, what, name);
    if (!t) return VQS_OK;
    size_t bytes = plane * sizeof(bf16_t), first;
    VQS_RUN(tap_window(h, name, first, bytes));
    VQS_RUN(tap_fits(h, name, *t, 2 * bytes));
    for (int pl = 0; pl < 2; ++pl)
        VQS_HIP(h, hipMemcpyAsync(static_cast<char*>(t->dst) + pl * bytes, reinterpret_cast<const char*>(src + pl * plane) + first, bytes,
                                  hipMemcpyDeviceToDevice, st), "tap copy");
    return VQS_OK;
}
// a tensor whose rows sit at a pitch: the tap receives the dense [rows, width] tensor (whole tensors only: no handle windows these)
inline int tap2d(HostBase* h, const char* stack, int layer, const char* what, const bf16_t* src, int width, int rows, int pitch, hipStream_t st) {
    if (h->taps.map.empty()) return VQS_OK;
    const size_t bytes = (size_t)rows * width * sizeof(bf16_t);
    if (pitch == width) return tap(h, stack, layer, what, src, bytes, st);
    std::string name;
    const TapSet::Tap* t = find_tap(h, stack, layer, what, name);
    if (!t) return VQS_OK;
    VQS_RUN(tap_fits(h, name, *t, bytes));
    VQS_HIP(h, hipMemcpy2DAsync(t->dst, (size_t)width * sizeof(bf16_t), src, (size_t)pitch * sizeof(bf16_t), (size_t)width * sizeof(bf16_t),
                                (size_t)rows, hipMemcpyDeviceToDevice, st), "tap copy");
    return VQS_OK;
}
// uses the `h` and `st` in scope
#define VQS_TAP(stack, layer, what, ptr, elems) VQS_RUN(vqs::tap(h, stack, layer, what, ptr, (size_t)(elems) * sizeof(*(ptr)), st))

}  // namespace vqs
