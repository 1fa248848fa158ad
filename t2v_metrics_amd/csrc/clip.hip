// Kernels of the CLIPScore row (include/vqs_clip.h) that the CLIP-FlanT5 row does not have: the text tower's causal
// attention, the token + position embedding, pool + projection head, and the cosine grid.  gfx950 only.
//
// Causal attention (HF CLIPAttention with the causal mask of CLIPTextTransformer, modeling_clip.py): head dim 64, S <= 128, so
// one workgroup holds the whole K and V of one (text, head) in LDS and every wave owns 16-query tiles.  Both products run
// TRANSPOSED on v_mfma_f32_16x16x32_{f16,bf16} (operand maps: lane l holds A[row l&15][k = 8(l>>4) + j] and
// B[k = 8(l>>4) + j][col l&15], result col = l&15, row = 4(l>>4) + i):
//   S^T = K . Q^T   A = K tile (a lane reads 16 contiguous bytes of one K row), B = Q^T (16 contiguous bytes of one Q row);
//                   the result has the QUERY on the lane (l&15) and four keys 4(l>>4) + i in its registers, so a query's
//                   softmax statistics are a reduction over a lane's own registers plus the three lanes 16 / 32 / 48 apart;
//   O^T = V^T . P^T B = P^T: a lane needs, for its query, the probabilities of 8 keys of a 32-key step.  An MFMA sums over k
//                   whatever key a k slot stands for, as long as A and B agree: slot j < 4 of lane group g is key
//                   32c + 4g + j (score tile 2c), slot j >= 4 is key 32c + 16 + 4g + (j - 4) (score tile 2c + 1) -- exactly
//                   the registers the lane already holds.  A = V^T read from a transposed LDS image with the same slot map
//                   (two 8-byte reads).  No probability ever moves between lanes or through LDS.
// Scores, mask, softmax and the final 1 / sum are fp32; probabilities enter the second product in the operand type.
#include "vqs_kernels.h"

namespace vqs {

typedef __attribute__((ext_vector_type(8))) __bf16 c_bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 c_f16x8;
typedef __attribute__((ext_vector_type(4))) float c_f32x4;

__device__ __forceinline__ float c_bf2f(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
template <bool F16>
__device__ __forceinline__ uint16_t c_to16(float f) {
    if constexpr (F16) return __builtin_bit_cast(uint16_t, (_Float16)f);
    else return __builtin_bit_cast(uint16_t, (__bf16)f);
}
__device__ __forceinline__ float c_h2f(uint16_t v) { return (float)__builtin_bit_cast(_Float16, v); }

template <bool F16>
__device__ __forceinline__ c_f32x4 c_mfma(uint4 a, uint4 b, c_f32x4 acc) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(c_f16x8, a), __builtin_bit_cast(c_f16x8, b), acc, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(c_bf16x8, a), __builtin_bit_cast(c_bf16x8, b), acc, 0, 0, 0);
}

static constexpr int CA_MAX_S = 128;
static constexpr int CA_KP = 72;     // K row pitch in 16-bit elements: 144 B keeps the 16-byte reads aligned and staggers the rows' banks
static constexpr int CA_VP = 136;    // V^T row pitch: 128 keys + 8

template <bool F16>
__global__ __launch_bounds__(256) void clip_causal_attn_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                               const bf16_t* __restrict__ v, bf16_t* __restrict__ out, int H, int S,
                                                               float scale) {
    __shared__ __attribute__((aligned(16))) uint16_t Ks[CA_MAX_S * CA_KP];
    __shared__ __attribute__((aligned(16))) uint16_t Vt[64 * CA_VP];
    const int bh = blockIdx.x;
    const int b = bh / H, h = bh - b * H;
    const size_t base = (size_t)bh * S * 64;
    const int S32 = (S + 31) & ~31;                     // keys staged (rows >= S are zero: a masked probability times them stays 0)
    for (int idx = threadIdx.x; idx < S32 * 8; idx += 256) {
        const int row = idx >> 3, c = idx & 7;
        uint4 kv = make_uint4(0, 0, 0, 0), vv = make_uint4(0, 0, 0, 0);
        if (row < S) {
            kv = *reinterpret_cast<const uint4*>(k + base + (size_t)row * 64 + c * 8);
            vv = *reinterpret_cast<const uint4*>(v + base + (size_t)row * 64 + c * 8);
        }
        *reinterpret_cast<uint4*>(Ks + row * CA_KP + c * 8) = kv;
        const uint32_t w4[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) Vt[(c * 8 + j) * CA_VP + row] = (uint16_t)(w4[j >> 1] >> ((j & 1) * 16));
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = lane & 15, g = lane >> 4;
    for (int qt = wave; qt * 16 < S; qt += 4) {
        const int qrow = qt * 16 + r;
        uint4 qf[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
            qf[ks] = qrow < S ? *reinterpret_cast<const uint4*>(q + base + (size_t)qrow * 64 + ks * 32 + g * 8) : make_uint4(0, 0, 0, 0);
        const int nkt = 2 * (qt / 2 + 1);               // key tiles up to the 32-key step that holds the diagonal; 16 * nkt <= S32
        c_f32x4 sc[8];
        float m = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt) {
            sc[kt] = c_f32x4{0.f, 0.f, 0.f, 0.f};
            if (kt < nkt) {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const uint4 kf = *reinterpret_cast<const uint4*>(Ks + (kt * 16 + r) * CA_KP + ks * 32 + g * 8);
                    sc[kt] = c_mfma<F16>(kf, qf[ks], sc[kt]);
                }
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int key = kt * 16 + g * 4 + i;
                    const float s = key <= qrow ? sc[kt][i] * scale : -INFINITY;
                    sc[kt][i] = s;
                    m = fmaxf(m, s);
                }
            }
        }
        m = fmaxf(m, __shfl_xor(m, 16));
        m = fmaxf(m, __shfl_xor(m, 32));               // key 0 is visible to every query: m is finite
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < 8; ++kt)
            if (kt < nkt) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float p = __expf(sc[kt][i] - m);
                    sc[kt][i] = p;
                    l += p;
                }
            }
        l += __shfl_xor(l, 16);
        l += __shfl_xor(l, 32);
        c_f32x4 o[4];
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] = c_f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (2 * c < nkt) {
                uint4 pf;
                pf.x = (uint32_t)c_to16<F16>(sc[2 * c][0]) | ((uint32_t)c_to16<F16>(sc[2 * c][1]) << 16);
                pf.y = (uint32_t)c_to16<F16>(sc[2 * c][2]) | ((uint32_t)c_to16<F16>(sc[2 * c][3]) << 16);
                pf.z = (uint32_t)c_to16<F16>(sc[2 * c + 1][0]) | ((uint32_t)c_to16<F16>(sc[2 * c + 1][1]) << 16);
                pf.w = (uint32_t)c_to16<F16>(sc[2 * c + 1][2]) | ((uint32_t)c_to16<F16>(sc[2 * c + 1][3]) << 16);
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    const uint16_t* vrow = Vt + (dt * 16 + r) * CA_VP + c * 32 + g * 4;
                    const uint2 lo = *reinterpret_cast<const uint2*>(vrow);
                    const uint2 hi = *reinterpret_cast<const uint2*>(vrow + 16);
                    o[dt] = c_mfma<F16>(make_uint4(lo.x, lo.y, hi.x, hi.y), pf, o[dt]);
                }
            }
        if (qrow < S) {
            const float inv = 1.0f / l;
            bf16_t* dst = out + ((size_t)b * S + qrow) * ((size_t)H * 64) + h * 64 + g * 4;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                uint2 w2;
                w2.x = (uint32_t)c_to16<F16>(o[dt][0] * inv) | ((uint32_t)c_to16<F16>(o[dt][1] * inv) << 16);
                w2.y = (uint32_t)c_to16<F16>(o[dt][2] * inv) | ((uint32_t)c_to16<F16>(o[dt][3] * inv) << 16);
                *reinterpret_cast<uint2*>(dst + dt * 16) = w2;
            }
        }
    }
}

hipError_t launch_clip_causal_attention(const bf16_t* q, const bf16_t* k, const bf16_t* v, bf16_t* out, int B, int H, int S, float scale,
                                        bool f16, hipStream_t s) {
    if (!q || !k || !v || !out || B <= 0 || H <= 0 || S <= 0 || S > CA_MAX_S || (long long)B * H > 0x7fffffffLL) return hipErrorInvalidValue;
    if (f16) hipLaunchKernelGGL((clip_causal_attn_kernel<true>), dim3(B * H), dim3(256), 0, s, q, k, v, out, H, S, scale);
    else hipLaunchKernelGGL((clip_causal_attn_kernel<false>), dim3(B * H), dim3(256), 0, s, q, k, v, out, H, S, scale);
    return hipGetLastError();
}

// ---------------------------------------------------------------- token + position embedding
// HF CLIPTextEmbeddings: inputs_embeds = token_embedding(ids) + position_embedding(arange(L)); fp32 stream out.
__global__ __launch_bounds__(128) void clip_embed_kernel(const int* __restrict__ ids, const bf16_t* __restrict__ tok, const bf16_t* __restrict__ pos,
                                                         float* __restrict__ out, int L, int D, int vocab) {
    const int row = blockIdx.x;
    const int s = row % L;
    const int id = ids[row];
    const bool ok = id >= 0 && id < vocab;
    const bf16_t* t = tok + (size_t)(ok ? id : 0) * D;
    const bf16_t* p = pos + (size_t)s * D;
    float* o = out + (size_t)row * D;
    for (int d = threadIdx.x * 8; d < D; d += 128 * 8) {
        const uint4 a = *reinterpret_cast<const uint4*>(t + d), c = *reinterpret_cast<const uint4*>(p + d);
        const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, cw[4] = {c.x, c.y, c.z, c.w};
        float r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = c_bf2f((bf16_t)(aw[j >> 1] >> ((j & 1) * 16))), y = c_bf2f((bf16_t)(cw[j >> 1] >> ((j & 1) * 16)));
            r[j] = ok ? x + y : __builtin_nanf("");
        }
        *reinterpret_cast<float4*>(o + d) = make_float4(r[0], r[1], r[2], r[3]);
        *reinterpret_cast<float4*>(o + d + 4) = make_float4(r[4], r[5], r[6], r[7]);
    }
}

hipError_t launch_clip_embed(const int* ids, const bf16_t* tok, const bf16_t* pos, float* out, int n, int L, int D, int vocab, hipStream_t s) {
    if (!ids || !tok || !pos || !out || n <= 0 || L <= 0 || D <= 0 || (D % 8) != 0 || vocab <= 0 || (long long)n * L > 0x7fffffffLL)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_embed_kernel, dim3(n * L), dim3(128), 0, s, ids, tok, pos, out, L, D, vocab);
    return hipGetLastError();
}

// ---------------------------------------------------------------- pool + head
// One workgroup per sample: the pooled row of the fp32 stream (+ the sub-layer output still pending on it), LayerNorm with fp32
// statistics (HF final_layer_norm / post_layernorm), the bias-free projection (text_projection / visual_projection, bf16 weights,
// fp32 FMA: a wave per output, lanes stride the row in 16-byte pieces), L2 normalisation.  Nothing is rounded to 16 bits.
static constexpr int PH_MAX = 4096;

__device__ __forceinline__ float ph_block_sum(float v, float* red) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();                                   // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(256) void clip_pool_head_kernel(const float* __restrict__ x, const bf16_t* __restrict__ delta, int delta_f16,
                                                             const int* __restrict__ rows, const bf16_t* __restrict__ lnw,
                                                             const bf16_t* __restrict__ lnb, const bf16_t* __restrict__ proj,
                                                             float* __restrict__ out, int S, int D, int E, float eps) {
    __shared__ float xs[PH_MAX];
    __shared__ float es[PH_MAX];
    __shared__ float red[4];
    const int b = blockIdx.x;
    int row = rows ? rows[b] : 0;
    const bool ok = row >= 0 && row < S;
    if (!ok) row = 0;
    const size_t off = ((size_t)b * S + row) * D;
    float part = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        float t = x[off + d];
        if (delta) t += delta_f16 ? c_h2f(delta[off + d]) : c_bf2f(delta[off + d]);
        xs[d] = t;
        part += t;
    }
    const float mean = ph_block_sum(part, red) / (float)D;
    part = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float c = xs[d] - mean;
        part += c * c;
    }
    const float rstd = rsqrtf(ph_block_sum(part, red) / (float)D + eps);
    for (int d = threadIdx.x; d < D; d += 256) xs[d] = (xs[d] - mean) * rstd * c_bf2f(lnw[d]) + c_bf2f(lnb[d]);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int e = wave; e < E; e += 4) {
        const bf16_t* wr = proj + (size_t)e * D;
        float acc = 0.f;
        for (int d = lane * 8; d < D; d += 64 * 8) {
            const uint4 w = *reinterpret_cast<const uint4*>(wr + d);
            const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) acc = fmaf(c_bf2f((bf16_t)(ww[j >> 1] >> ((j & 1) * 16))), xs[d + j], acc);
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o);
        if (lane == 0) es[e] = acc;
    }
    __syncthreads();
    part = 0.f;
    for (int e = threadIdx.x; e < E; e += 256) part += es[e] * es[e];
    const float nrm = sqrtf(ph_block_sum(part, red));
    for (int e = threadIdx.x; e < E; e += 256) out[(size_t)b * E + e] = ok ? es[e] / nrm : __builtin_nanf("");
}

hipError_t launch_clip_pool_head(const float* x, const bf16_t* delta, bool delta_f16, const int* rows, const bf16_t* lnw, const bf16_t* lnb,
                                 const bf16_t* proj, float* out, int n, int S, int D, int E, float eps, hipStream_t s) {
    if (!x || !lnw || !lnb || !proj || !out || n <= 0 || S <= 0 || D <= 0 || D > PH_MAX || (D % 8) != 0 || E <= 0 || E > PH_MAX)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_pool_head_kernel, dim3(n), dim3(256), 0, s, x, delta, delta_f16 ? 1 : 0, rows, lnw, lnb, proj, out, S, D, E, eps);
    return hipGetLastError();
}

// ---------------------------------------------------------------- cosine grid / pairs
// One ascending fp32 FMA chain per element, the same function in both kernels: a pair's score is bitwise its grid element.
__device__ __forceinline__ float clip_dot(const float* __restrict__ a, const float* __restrict__ b, int E) {
    float acc = 0.f;
    for (int e = 0; e < E; e += 4) {
        const float4 x = *reinterpret_cast<const float4*>(a + e), y = *reinterpret_cast<const float4*>(b + e);
        acc = fmaf(x.x, y.x, acc);
        acc = fmaf(x.y, y.y, acc);
        acc = fmaf(x.z, y.z, acc);
        acc = fmaf(x.w, y.w, acc);
    }
    return acc;
}

__global__ __launch_bounds__(256) void clip_sim_grid_kernel(const float* __restrict__ img, const float* __restrict__ txt, int M, int N, int E,
                                                            float* __restrict__ out) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i < M && j < N) out[(size_t)i * N + j] = clip_dot(img + (size_t)i * E, txt + (size_t)j * E, E);
}

__global__ __launch_bounds__(256) void clip_sim_pairs_kernel(const float* __restrict__ img, const float* __restrict__ txt, const int* __restrict__ ii,
                                                             const int* __restrict__ tt, int M, int N, int K, int E, float* __restrict__ out) {
    const int kk = blockIdx.x * 256 + threadIdx.x;
    if (kk >= K) return;
    const int i = ii[kk], j = tt[kk];
    out[kk] = (i >= 0 && i < M && j >= 0 && j < N) ? clip_dot(img + (size_t)i * E, txt + (size_t)j * E, E) : __builtin_nanf("");
}

hipError_t launch_clip_similarity(const float* img, const float* txt, int M, int N, int E, float* out, hipStream_t s) {
    if (!img || !txt || !out || M <= 0 || N <= 0 || E <= 0 || (E % 4) != 0 || (M + 3) / 4 > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_sim_grid_kernel, dim3((N + 63) / 64, (M + 3) / 4), dim3(256), 0, s, img, txt, M, N, E, out);
    return hipGetLastError();
}

hipError_t launch_clip_similarity_pairs(const float* img, const float* txt, const int* ii, const int* tt, int M, int N, int K, int E, float* out,
                                        hipStream_t s) {
    if (!img || !txt || !ii || !tt || !out || M <= 0 || N <= 0 || K <= 0 || E <= 0 || (E % 4) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(clip_sim_pairs_kernel, dim3((K + 255) / 256), dim3(256), 0, s, img, txt, ii, tt, M, N, K, E, out);
    return hipGetLastError();
}

}  // namespace vqs
