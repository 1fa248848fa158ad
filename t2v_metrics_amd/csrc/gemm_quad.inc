// =====================================================================================================
// QUAD form (the default of every bf16-result nn.Linear of the path since round 3): four waves of 128x128 (one per SIMD),
// v_mfma_f32_16x16x32_bf16, 256 fp32 accumulators per lane in hand-named AGPRs, over a K-tile pipeline whose LDS image
// is only a LANDING ZONE and whose prefetch distance is TWO K-tiles.
//
// Why this shape (round 3; profiles/r3_call3_*, r3_call5_* ... r3_call10_*):
//   * PMC of one 155 648 x 4 096 x 4 096 launch: hipBLASLt's kernel for these shapes (MT256x256x64, four waves of 128x128,
//     direct-to-LDS loads, prefetch two K-tiles ahead) keeps the matrix pipes 89 % busy at the power-limited clock, the
//     8-wave forms here 73 %, the first wide / ring forms 53-60 % -- at identical L2 hit rates and fabric bytes.  The
//     difference is what a wave issues between its MFMAs and how often it waits: the vendor loop has at most ONE other
//     instruction between two MFMAs and counted waits that never block.
//   * With that discipline (this file's schedule, still on 32x32x16 MFMAs; git history) the form ran 1 310-1 360 TFLOP/s
//     against the 8-wave forms' 1 210-1 290 and the vendor library's 1 480-1 550 -- and 2 150 with the LDS-DMA issued
//     through null descriptors (zeros in LDS): the instruction stream is not the limit any more, the power-limited clock is.
//   * The same stream with every 32x32x16 MFMA replaced by two 16x16x32 MFMAs (same FLOPs, same operands, same memory
//     traffic): 1 750-1 820 TFLOP/s.  A 16x16x32 MFMA moves half the accumulator bytes per FLOP through the register file
//     (4 instead of 16 fp32 per lane and 8 192 MACs instead of 16 384); on a chip that clocks to its power budget that is
//     worth a third.  So: 16x16x32, like the vendor's kernel ("MI16x16x1").
//
// Schedule of one K-tile of 64 (two k-steps of 32; 128 MFMAs per wave = 128 gaps of 16 matrix-pipe cycles):
//   gaps   0.. 30  read the fragments of THIS K-tile's second k-step (set 1: freed by the previous K-tile's last 64 MFMAs),
//                  one read per two gaps = 128 B/clk for the CU's four waves, half the LDS's rate (one per gap saturated it
//                  next to the landing LDS-DMA and the wait of B1 blocked)
//   gaps  32.. 35  toggle the four fragment-address registers to the other buffer (v_xor)
//   -- B1 (gap 40) lgkmcnt(0) + barrier: every wave has read everything it needs from this K-tile's buffer
//   gaps  40..102  the sixteen LDS-DMA pieces of the K-tile TWO ahead go into the buffer just freed, one piece per four
//                  gaps (64 cycles: the rate the CU's vector-memory front end takes 1-KiB wave-instructions from four waves):
//                  M0 write in gap 40 + 4 d, `buffer_load ... lds` in gap 42 + 4 d -- never in the same gap: an M0 write
//                  straight behind an LDS-DMA waits for the memory path to take the instruction (60-180 cycles under load)
//   -- B2 (gap 96) counted vmcnt + barrier: the NEXT K-tile has landed (its pieces were issued 120-180 gaps = 1 900-2 900
//                  matrix-pipe cycles ago, against a measured ~1 850-cycle staging latency under the GEMM's own traffic)
//   gaps  96..126  read the next K-tile's first k-step into set 0 (free since gap 63), one read per two gaps
// Two barriers per K-tile, neither preceded by a wait that blocks in steady state (round 6's ablations: every counted wait removed = no gain; both
// barriers removed = +2 ... 11 %: what costs is keeping the four waves in step, profiles/r6_gemm_vendor_kernel.md).  128 KiB of LDS for the two K-tile
// buffers (rows of 128 B = whole cache lines; the A image keeps the 8-wave forms' swizzle, the W image has its own: gemm_quad_kernel.inc); the epilogue
// goes straight from the registers (no scratch since round 6), so the stream runs on across output tiles (and past the last one through null
// descriptors: no "stream ended" variant of the loop, one set of vmcnt counts).
//
// Addressing: the 16 per-lane LDS-DMA offsets are TILE-RELATIVE and loop-invariant; an output tile's first row goes into
// the base of the SGPR buffer descriptor (64-bit) and its remaining bytes into num_records, so rows beyond M / N read as
// zeros (hardware range check) instead of being clamped -- and no operand offset is ever truncated to 32 bits.
//
// Numerics: one k-order per output element (k ascending in steps of 32, the MFMA's internal order inside a step), whatever
// M, N, the tile order or the position of the row in the batch: a pair's bits do not depend on the batch it is scored in
// (tests/test_gpu_bench_config.py).  A 16x16x32 MFMA adds a k-step's 32 products in the order two 32x32x16 MFMAs do, so the
// 8-wave forms produce the SAME bits (test_gemm_quad_form_is_bitwise_the_other_forms: torch.equal against variant 0 and 11 on
// every epilogue); every bf16-result call site still runs THIS form for every M (gemm_plan) -- the guarantee then does not
// rest on that hardware property -- and the others keep the fp32-result / batched / tiny-K launches.
// =====================================================================================================
#ifndef VQS_QUAD_ORDER
#define VQS_QUAD_ORDER 0
#endif
#ifndef VQS_QUAD_ABL
#define VQS_QUAD_ABL 0      // timing ablations (1, 2, 4, 128: garbage results): 1 = no LDS-DMA in the K loop, 2 = the K loop's LDS-DMA goes
                            // through null descriptors, 4 = B2 does not wait for the staged data, 8 = B1 does not wait for its LDS reads, 16 = no barrier at
                            // B1 / B2 (64 / 512: at B1 / at B2 only), 32 = no wait at the top of a tile, 128 = no epilogue, 256 = the epilogue without its global stores
#endif
static constexpr int QD_BUF = 65536;                    // one K-tile: A 32 KiB + W 32 KiB
// (rounds 3-5 kept 4 x 8 KiB of wave-private epilogue scratch behind the two buffers; the register-direct epilogue of round 6 needs none)

__device__ __forceinline__ v4i_t make_rsrc_n(const void* base, uint64_t bytes) {
    const uint64_t b = (uint64_t)base;
    v4i_t r;
    r.x = __builtin_amdgcn_readfirstlane((uint32_t)b);
    r.y = __builtin_amdgcn_readfirstlane((uint32_t)(b >> 32) & 0xffffu);
    r.z = __builtin_amdgcn_readfirstlane((uint32_t)(bytes > 0xffffffffull ? 0xffffffffull : bytes));
    r.w = 0x00020000;
    return r;
}

typedef uint32_t q_frag_t __attribute__((ext_vector_type(4)));
// accumulator block Q = 8 m + n (rows 16 m .., columns 16 n .. of the wave's 128 x 128) lives in a[4 Q : 4 Q + 3].  The MFMA /
// read-back statements below are the only code that touches AGPRs; tests/test_build_invariants.py checks on the ISA that the
// compiler keeps nothing of its own there (no AGPR operand outside v_mfma / v_accvgpr_read, no scratch).
// F16: the operands are IEEE fp16 instead of bf16 (same fragment layout, same rate, 11 instead of 8 significant bits): the vision tower's
// option `vit_fp16` (vqs.h).  Everything else of the kernel is shared; only this instruction and the epilogue's pack differ.
template <int Q, bool ZERO, bool F16 = false>
__device__ __forceinline__ void mfma16(const uint4& a, const uint4& b) {
    const q_frag_t av = {a.x, a.y, a.z, a.w}, bv = {b.x, b.y, b.z, b.w};
    if constexpr (F16) {
        if constexpr (ZERO) asm volatile("v_mfma_f32_16x16x32_f16 a[%2:%3], %0, %1, 0" ::"v"(av), "v"(bv), "i"(4 * Q), "i"(4 * Q + 3));
        else asm volatile("v_mfma_f32_16x16x32_f16 a[%2:%3], %0, %1, a[%2:%3]" ::"v"(av), "v"(bv), "i"(4 * Q), "i"(4 * Q + 3));
    } else {
        if constexpr (ZERO) asm volatile("v_mfma_f32_16x16x32_bf16 a[%2:%3], %0, %1, 0" ::"v"(av), "v"(bv), "i"(4 * Q), "i"(4 * Q + 3));
        else asm volatile("v_mfma_f32_16x16x32_bf16 a[%2:%3], %0, %1, a[%2:%3]" ::"v"(av), "v"(bv), "i"(4 * Q), "i"(4 * Q + 3));
    }
}
template <bool F16>
__device__ __forceinline__ uint32_t quad_pack2(float a, float b) {
    if constexpr (F16) return pack2h(a, b);
    else return pack2(a, b);
}
template <int Q>
__device__ __forceinline__ void acc4_read(float (&o)[4]) {
    asm volatile("v_accvgpr_read_b32 %0, a[%4]\n\tv_accvgpr_read_b32 %1, a[%5]\n\tv_accvgpr_read_b32 %2, a[%6]\n\tv_accvgpr_read_b32 %3, a[%7]"
                 : "=v"(o[0]), "=v"(o[1]), "=v"(o[2]), "=v"(o[3])
                 : "i"(4 * Q), "i"(4 * Q + 1), "i"(4 * Q + 2), "i"(4 * Q + 3));
}
// the kernel descriptor must allocate all 256 AGPRs although no statement above carries a clobber list
__device__ __forceinline__ void quad_claim_agprs() {
    asm volatile("" ::: "a0", "a15", "a31", "a47", "a63", "a79", "a95", "a111", "a127", "a143", "a159", "a175", "a191", "a207", "a223", "a239", "a255");
}

// ----------------------------------------------------------------------------------------------------
// Epilogue of one wave's 128 x 128 block, STRAIGHT FROM THE REGISTERS (round 6; rounds 3-5 staged it through 32 KiB of wave-private LDS).
// The wave's accumulators are 8 x 8 blocks of 16 x 16; block (m, n) register r of lane l holds activation row 16 m + (l & 15) and the output
// column whose WEIGHT ROW the MFMA's A operand carried in its row 4 (l >> 4) + r.  The K loop reads the weight fragments so that row i of block n
// is weight row 32 (n >> 1) + 4 (n & 1) + 8 (i >> 2) + (i & 3) of the wave's 128 (gemm_quad_kernel.inc): blocks 2 t and 2 t + 1 then give lane l the
// EIGHT CONSECUTIVE output columns 32 t + 8 (l >> 4) + 0 .. 7 of its row -- one 16-byte store per (m, t), a wave instruction = 16 rows x 64 B whole
// sectors, 32 stores per wave and tile as before (gated: 16), no LDS round trip and none of its waits.  Every output element is the same dot product in
// the same k order as before: bitwise neutral (tests/test_gpu_kernels.py: torch.equal against the one-tile and the 8-wave forms on every epilogue).
//   plain / activation : C[row][col_w + 32 t + 8 q + e] = f(acc * acc_scale + bias) * out_scale            (the scales: SC families only)
//   gated              : W rows interleaved in blocks of 32 (gate | linear): t = 2 j is the gate, t = 2 j + 1 the linear column of output
//                        columns 32 j + 8 q + e of the wave's 64 -- both in this lane
//   heads              : the 8 columns are 8 consecutive lanes of one head (hd_src % 8 == 0); rows step by 16 through (sample, position)
//   heads + rope (SC)  : lanes d < 64 of a 128-lane head are t = 0, 1, their partners d + 64 are t + 2 in the same lane
// BIAS false: the launch has no bias vector (every T5 linear): no additions of zero.
// ----------------------------------------------------------------------------------------------------
template <int EPI, int M8, bool F16, bool SC, bool BIAS, bool ROPE>
__device__ __forceinline__ void quad_epilogue_rows(const GemmParams& p, int row, bool row_ok, int col_w, int lq, bool full, const float (&bia)[4][8],
                                                   bf16_t* const (&hdst)[4], long long hoff) {
    const bool nt = p.nt_store != 0;
    float c[8][4];                                                     // blocks n = 0 .. 7 of row block M8
#define QE_RD(N) acc4_read<8 * M8 + N>(c[N])
    QE_RD(0); QE_RD(1); QE_RD(2); QE_RD(3); QE_RD(4); QE_RD(5); QE_RD(6); QE_RD(7);
#undef QE_RD
    float t8[4][8];                                                    // [t][e]: the lane's eight consecutive columns of pair t
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float a = c[2 * t + (e >> 2)][e & 3];
            t8[t][e] = SC ? fmaf(a, p.acc_scale, bia[t][e]) : BIAS ? a + bia[t][e] : a;
        }
    if constexpr (EPI == EPI_GATED) {
        const bool silu = p.gate_act == 1;
        const int NO = p.N >> 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float gv = t8[2 * j][e];
                const float a = silu ? gv * fast_rcp(1.0f + __expf(-gv)) : act_gelu_new(gv);
                o[e] = a * t8[2 * j + 1][e];
                if constexpr (SC) o[e] *= p.out_scale;
            }
            uint4 v;
            v.x = quad_pack2<F16>(o[0], o[1]); v.y = quad_pack2<F16>(o[2], o[3]); v.z = quad_pack2<F16>(o[4], o[5]); v.w = quad_pack2<F16>(o[6], o[7]);
            const int oc = (col_w >> 1) + 32 * j + 8 * lq;
            if constexpr (VQS_QUAD_ABL & 256) asm volatile("" ::"v"(v.x), "v"(v.w));
            else if (full || (row_ok && oc < NO)) st_row16(reinterpret_cast<bf16_t*>(p.C) + (size_t)row * p.ldc + oc, v, nt);
        }
    } else {
        if constexpr (ROPE) {
            // x'[d] = x[d] c[d] - x[d + 64] s[d], x'[d + 64] = x[d + 64] c[d] + x[d] s[d] (rope_qk_kernel's expressions) on the unrounded projection
            const int rr = row_ok ? row : p.M - 1;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float4* cr = reinterpret_cast<const float4*>(p.rope_cos + (size_t)rr * 64 + 32 * t + 8 * lq);
                const float4* sr = reinterpret_cast<const float4*>(p.rope_sin + (size_t)rr * 64 + 32 * t + 8 * lq);
                const float4 c0 = cr[0], c1 = cr[1], s0 = sr[0], s1 = sr[1];
                const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w}, ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float a = t8[t][e], b = t8[t + 2][e];
                    t8[t][e] = a * cc[e] - b * ss[e];
                    t8[t + 2][e] = b * cc[e] + a * ss[e];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            float o[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                o[e] = t8[t][e];
                if constexpr (EPI == EPI_BF16_QGELU) o[e] = act_quick_gelu(o[e]);
                if constexpr (EPI == EPI_BF16_GELU) o[e] = act_gelu_erf(o[e]);
                if constexpr (SC) o[e] *= p.out_scale;
            }
            uint4 v;
            v.x = quad_pack2<F16>(o[0], o[1]); v.y = quad_pack2<F16>(o[2], o[3]); v.z = quad_pack2<F16>(o[4], o[5]); v.w = quad_pack2<F16>(o[6], o[7]);
            const int col = col_w + 32 * t + 8 * lq;
            if constexpr (VQS_QUAD_ABL & 256) asm volatile("" ::"v"(v.x), "v"(v.w));
            else if (full || (row_ok && col < p.N)) {
                bf16_t* dst;
                if constexpr (EPI == EPI_HEADS) dst = hdst[t] + hoff;
                else dst = reinterpret_cast<bf16_t*>(p.C) + (size_t)row * p.ldc + col;
                st_row16(dst, v, nt);
            }
        }
    }
}

template <int EPI, bool F16, bool SC, bool BIAS, bool ROPE>
__device__ __forceinline__ void quad_epilogue_all(const GemmParams& p, int row_w, int col_w, int lane, bool full, const float (&bia)[4][8]) {
    const int lr = lane & 15, lq = lane >> 4;
    // EPI_HEADS: columns [0, inner) -> q heads, [inner, inner + inner_kv) -> k heads, rest -> v heads; a head is hd_src columns of the product and lands in
    // the first hd_src lanes of an hd-lane slot.  All 128 columns of a wave's block belong to tensors with one head count (the launcher's rule); the lane's
    // four 8-column chunks may sit in different heads (hd_src = 64 or 80): one destination base per chunk, computed once per tile.
    bf16_t* hdst[4] = {nullptr, nullptr, nullptr, nullptr};
    int hdim = 64, hx = 1, hs = 0;
    long long hoff = 0, hwrap = 0;
    if constexpr (EPI == EPI_HEADS) {
        hdim = p.hd > 0 ? p.hd : 64;
        const int hsrc = p.hd_src > 0 ? p.hd_src : hdim;
        const int ikv = p.inner_kv > 0 ? p.inner_kv : p.inner;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int cl = col_w + 32 * t + 8 * lq;
            const int which = cl < p.inner ? 0 : (cl < p.inner + ikv ? 1 : 2);
            const int base = which == 0 ? 0 : (which == 1 ? p.inner : p.inner + ikv);
            bf16_t* hp = which == 0 ? p.heads_out[0] : (which == 1 ? p.heads_out[1] : p.heads_out[2]);
            const int head = (cl - base) / hsrc;
            hdst[t] = hp + (size_t)head * p.S * hdim + ((cl - base) - head * hsrc);
        }
        hx = min(col_w, p.N - 64) < p.inner ? p.H : (p.Hkv > 0 ? p.Hkv : p.H);
        heads_off_first(row_w + lr, p.S, hx, hdim, hs, hoff);          // row 16 m + lr: m = 0 here, + 16 per row block below
        hwrap = (long long)(hx - 1) * p.S * hdim;
    }
#define QE_ROWS(M8)                                                                                                                        \
    {                                                                                                                                      \
        const int row = row_w + 16 * M8 + lr;                                                                                              \
        quad_epilogue_rows<EPI, M8, F16, SC, BIAS, ROPE>(p, row, row < p.M, col_w, lq, full, bia, hdst, hoff);                              \
        if constexpr (EPI == EPI_HEADS) {                              /* next row block: + 16 positions (S >= 16: at most one sample boundary) */ \
            if (p.S >= 16) {                                                                                                               \
                hs += 16;                                                                                                                  \
                hoff += 16 * hdim;                                                                                                         \
                if (hs >= p.S) { hs -= p.S; hoff += hwrap; }                                                                               \
            } else {                                                                                                                       \
                heads_off_first(row + 16, p.S, hx, hdim, hs, hoff);                                                                        \
            }                                                                                                                              \
        }                                                                                                                                  \
    }
    QE_ROWS(0) QE_ROWS(1) QE_ROWS(2) QE_ROWS(3) QE_ROWS(4) QE_ROWS(5) QE_ROWS(6) QE_ROWS(7)
#undef QE_ROWS
}

#ifndef VQS_QUAD_ALWAYS_BIAS
#define VQS_QUAD_ALWAYS_BIAS 0      // lab flavour 1: round 5's arithmetic (the additions of zero are executed)
#endif
template <int EPI, bool F16 = false, bool SC = false>
__device__ __forceinline__ void quad_epilogue(const GemmParams& p, int m0, int n0, int wr, int wc, int lane, bool full) {
    const int lq = lane >> 4;
    const int row_w = m0 + wr * 128, col_w = n0 + wc * 128;
    float bia[4][8];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int e = 0; e < 8; ++e) bia[t][e] = 0.0f;
        if (p.bias != nullptr) {                                       // wave-uniform: no T5 linear has a bias
            const int cidx = col_w + 32 * t + 8 * lq;
            if (cidx < p.N) {
                const uint4 bv = *reinterpret_cast<const uint4*>(p.bias + cidx);
                const uint32_t bw[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    bia[t][2 * k] = bf2f((bf16_t)(bw[k] & 0xffff));
                    bia[t][2 * k + 1] = bf2f((bf16_t)(bw[k] >> 16));
                }
            }
        }
    }
    if constexpr (SC && EPI == EPI_HEADS) {
        // rotary embedding in the epilogue: this wave's 128 columns are one q or k head (wave-uniform: the launcher's head-alignment rule)
        const int ikv_r = p.inner_kv > 0 ? p.inner_kv : p.inner;
        if (p.rope_cos != nullptr && col_w < p.inner + ikv_r) {
            quad_epilogue_all<EPI, F16, SC, true, true>(p, row_w, col_w, lane, full, bia);
            return;
        }
    }
    if (SC || p.bias != nullptr || VQS_QUAD_ALWAYS_BIAS) quad_epilogue_all<EPI, F16, SC, true, false>(p, row_w, col_w, lane, full, bia);     // wave-uniform
    else quad_epilogue_all<EPI, F16, SC, false, false>(p, row_w, col_w, lane, full, bia);
}

template <class F, int... G>
__device__ __forceinline__ void quad_for_gaps(F&& f, std::integer_sequence<int, G...>) {
    (f(std::integral_constant<int, G>{}), ...);
}

template <int EPI>
struct QuadStores {   // VMEM store instructions per wave for a full tile
    static constexpr int value = (EPI == EPI_GATED) ? 16 : 32;
};

#define QUAD_SCALED false
#define QUAD_KERNEL gemm_bf16_quad
#define QUAD_F16 false
#define QUAD_OUT_F16 false
#include "gemm_quad_kernel.inc"
#undef QUAD_KERNEL
#undef QUAD_F16
#undef QUAD_OUT_F16
// the same kernel on fp16 operands with an fp16 result (bias still bf16, accumulation and epilogue arithmetic fp32); never instantiated
// with the gated epilogue (no fp16 tensor leaves a gated FFN: T5 is not fp16-safe there)
#define QUAD_KERNEL gemm_f16_quad
#define QUAD_F16 true
#define QUAD_OUT_F16 true
#include "gemm_quad_kernel.inc"
#undef QUAD_KERNEL
#undef QUAD_F16
#undef QUAD_OUT_F16
// fp16 operands, bf16 result: the T5 encoder's o projection (its bf16 delta) and gated wi (its bf16 FFN product) when the encoder's
// attention side runs on fp16 tensors (option enc_fp16; GemmParams::f16 = 2)
#define QUAD_KERNEL gemm_f16b_quad
#define QUAD_F16 true
#define QUAD_OUT_F16 false
#include "gemm_quad_kernel.inc"
#undef QUAD_KERNEL
#undef QUAD_F16
#undef QUAD_OUT_F16
// fp16 operands, fp16 result, SCALED epilogue (GemmParams::f16 = 3): the range-safe fp16 forms of the Qwen2.5-VL row -- every epilogue incl.
// the gated one (its fp16 product sits behind a bind-time scale that a proven bound of |SiLU(g) u| fits into)
#undef QUAD_SCALED
#define QUAD_SCALED true
#define QUAD_KERNEL gemm_f16s_quad
#define QUAD_F16 true
#define QUAD_OUT_F16 true
#include "gemm_quad_kernel.inc"
#undef QUAD_KERNEL
#undef QUAD_F16
#undef QUAD_OUT_F16
#undef QUAD_SCALED
// fp16 operands, bf16 result, SCALED epilogue (GemmParams::f16 = 4; plain epilogue only): the CLIP-FlanT5 projector's last GEMM when its fp16 input
// sits behind a scale (options proj_fs_shift / proj_mid_shift, vqs_api.cpp): the bf16 feature tensor leaves in true units
#define QUAD_SCALED true
#define QUAD_KERNEL gemm_f16bs_quad
#define QUAD_F16 true
#define QUAD_OUT_F16 false
#include "gemm_quad_kernel.inc"
#undef QUAD_KERNEL
#undef QUAD_F16
#undef QUAD_OUT_F16
#undef QUAD_SCALED
