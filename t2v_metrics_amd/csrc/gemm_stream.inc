// =====================================================================================================
// STREAM form (round 4): C[M <= 128, N] = A[M, K] . W[N, K]^T per batch entry, for launches whose W operand is streamed from
// HBM exactly once and whose A operand is a few rows -- the reassociated decoder cross-attention (vqs_api.cpp): per pair
// scores = q'[T*H <= 128, D] . E[S, D]^T and ctx = P[T*H, S] . E^T[D, S]^T, where E (1.27 GB at XXL, B = 256) is read twice per
// decoder layer: 61 GB per step, the decoder's HBM floor.  The 256 x 256 persistent kernel runs these with 64-128 of a tile's
// 256 rows valid and a two-stage staging ring sized for operands that sit in L2 / Infinity Cache: 3.5 TB/s.
//
// Here: one 256-thread workgroup per CU takes 128 columns of N (each wave 32 W rows) of one batch entry and walks the whole K
// in slabs of 64 through a FIVE-stage LDS ring (5 x (16 KiB of A + 4 x 4 KiB of W) = all 160 KiB): four slabs = 64 KiB of W per
// CU are in flight ahead of the one being computed (the chip needs ~12 MB in flight for 6 TB/s at ~2 us: 47 KiB per CU).  Both
// operands arrive by LDS-DMA as whole 128-byte rows (A from L2, where the batch entry's few rows stay; W from HBM), swizzled like
// every other GEMM image of this file (16-B chunk index XOR (row >> 1) & 7: conflict-free ds_read_b128 fragments).  A wave's W
// slabs are its own (no other wave reads them); the A slab is shared, hence one barrier per slab.  vmcnt is counted: a wave waits
// for its pieces of slab t with the pieces of the (up to) three younger slabs still in flight.
//
// Numerics: v_mfma_f32_32x32x16_bf16 with the W fragment as the A operand, k ascending in steps of 16, one accumulator chain per
// output element -- operand roles, k-slot mapping and order of gemm_bf16_kernel / gemm_bf16_persistent: results are BITWISE those
// of the 8-wave forms (tests/test_gpu_kernels.py holds it against variant 0), so which launches take this form (a function of M,
// N and the batch count, gemm_plan) never shows in a pair's bits.
// =====================================================================================================
static constexpr int ST_STAGES = 5;
static constexpr int ST_PD = ST_STAGES - 1;                 // slabs issued ahead of the one computed
static constexpr int ST_A_BYTES = 128 * 128;                // A slab: 128 rows x 64 k
static constexpr int ST_WW_BYTES = 32 * 128;                // one wave's W slab: 32 rows x 64 k
static constexpr int ST_STAGE_BYTES = ST_A_BYTES + 4 * ST_WW_BYTES;   // 32 KiB

// FT (round 5, GemmParams::f16): 0 = bf16 operands; 1 = IEEE fp16 operands and (EPI_BF16) an fp16 result; 2 = fp16 operands, bf16 result
// (incl. the split-bf16 form) -- the decoder's cross-attention score path of option dec_fp16 (q.Wk rows x the fp16 encoder output).
template <int EPI, int FT = 0>
__global__ void __launch_bounds__(256) gemm_bf16_stream(const GemmParams p) {
    static_assert(EPI == EPI_F32 || EPI == EPI_BF16, "plain results only");
    __shared__ __attribute__((aligned(16))) char lds[ST_STAGES * ST_STAGE_BYTES];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t lds_base = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)LDS_PTR(lds));

    // ---- work item: (batch entry, block of 128 columns).  Workgroup slot b runs on XCD b % 8: every XCD gets a contiguous run
    // of the item list, so the N blocks of one batch entry (which share its A rows) run on one XCD and find them in its L2.
    const int nblk = (p.N + 127) >> 7;
    const int total = nblk * (p.batch > 0 ? p.batch : 1);
    int item;
    {
        const int pid = blockIdx.x, xcd = pid & 7, local = pid >> 3;
        const int q = total >> 3, r = total & 7;
        item = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    }
    if (item >= total) return;
    const int bz = item / nblk;
    const int n0 = (item - bz * nblk) << 7;
    const int MB = (p.M + 31) >> 5;                         // 32-row blocks of A (1..4)
    const int nslab = p.K >> 6;

    // ---- staging: per slab this wave moves rows [32 w, 32 w + 32) of the A slab and its own 32 W rows, four 1-KiB pieces each
    // (piece i = rows 8 i .. 8 i + 7; lane l: row 8 i + (l >> 3), 16-B chunk (l & 7) ^ ((row >> 1) & 7) of the source row)
    const v4i_t rsA = make_rsrc_n(p.A + (size_t)bz * p.sA, (uint64_t)p.M * p.lda * 2u);
    const v4i_t rsW = make_rsrc_n(p.W + (size_t)bz * p.sW, (uint64_t)p.N * p.ldw * 2u);
    uint32_t pa[4], pw[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rl = 8 * i + (lane >> 3);                 // row within the wave's 32
        const uint32_t ch = (uint32_t)(((lane & 7) ^ ((rl >> 1) & 7)) << 4);
        pa[i] = (uint32_t)(32 * w + rl) * ((uint32_t)p.lda * 2u) + ch;
        pw[i] = (uint32_t)(n0 + 32 * w + rl) * ((uint32_t)p.ldw * 2u) + ch;
    }
    // piece j = 0..7 of slab t (0..3: A rows 8 j .., 4..7: W rows 8 (j - 4) ..) -> stage t % ST_STAGES
    auto issue_piece = [&](int t, int j) {
        const uint32_t sb = lds_base + (uint32_t)(t % ST_STAGES) * ST_STAGE_BYTES;
        const uint32_t koff = (uint32_t)t * 128u;
        if (j < 4) bglds16(rsA, pa[j], koff, sb + (uint32_t)(32 * w + 8 * j) * 128u);
        else bglds16(rsW, pw[j - 4], koff, sb + ST_A_BYTES + (uint32_t)w * ST_WW_BYTES + (uint32_t)(8 * (j - 4)) * 128u);
    };

    // ---- fragment offsets within a stage: row (lane & 31) of a 32-row block, k-step ks: chunk 2 ks + (lane >> 5)
    const int swr = (lane >> 1) & 7;
    int koff4[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) koff4[ks] = (((ks * 2 + (lane >> 5)) ^ swr) << 4);
    const int a_row = (lane & 31) * 128;
    const int w_row = ST_A_BYTES + w * ST_WW_BYTES + (lane & 31) * 128;

    f32x16 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[m][r] = 0.0f;

    for (int t = 0; t < ST_PD && t < nslab; ++t)
#pragma unroll
        for (int j = 0; j < 8; ++j) issue_piece(t, j);
    for (int t = 0; t < nslab; ++t) {
        // this wave's 8 pieces of slab t have landed: all but the pieces of the (at most ST_PD - 1) younger slabs
        const int younger = min(ST_PD - 1, nslab - 1 - t);
        if (younger >= 3) asm volatile("s_waitcnt vmcnt(24)" ::: "memory");
        else if (younger == 2) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
        else if (younger == 1) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                       // everybody's pieces of slab t; everybody is done with slab t - 1
        __builtin_amdgcn_sched_barrier(0);
        const bool more = t + ST_PD < nslab;                // slab t + ST_PD goes into the stage slab t - 1 occupied
        const char* sb = lds + (t % ST_STAGES) * ST_STAGE_BYTES;
        // Per k-step: the NEXT k-step's five fragment reads are issued first, then this k-step's MFMAs, then two of the eight
        // LDS-DMA pieces of the slab four ahead.  One wave per SIMD: nothing else covers an LDS round trip (~130 cycles x 4 per slab
        // when the reads sat in front of their own MFMAs) or the M0 write of an LDS-DMA, which waits 60-180 cycles for the memory
        // path to take the previous piece (gemm_quad.inc) -- eight back to back per slab made the consumer, not HBM, the bound:
        // 2 200 cycles per slab = 3.6 TB/s on the cross scores (profiles/r4_call3_*).
        uint4 wf[2], af[2][4];
        wf[0] = *reinterpret_cast<const uint4*>(sb + w_row + koff4[0]);
#pragma unroll
        for (int m = 0; m < 4; ++m)
            if (m < MB) af[0][m] = *reinterpret_cast<const uint4*>(sb + a_row + m * 4096 + koff4[0]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int cur = ks & 1, nxt = cur ^ 1;
            if (ks < 3) {
                wf[nxt] = *reinterpret_cast<const uint4*>(sb + w_row + koff4[ks + 1]);
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (m < MB) af[nxt][m] = *reinterpret_cast<const uint4*>(sb + a_row + m * 4096 + koff4[ks + 1]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int m = 0; m < 4; ++m)
                if (m < MB) {
                    if constexpr (FT != 0) acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, wf[cur]), __builtin_bit_cast(f16x8_t, af[cur][m]), acc[m], 0, 0, 0);
                    else acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, wf[cur]), __builtin_bit_cast(bf16x8, af[cur][m]), acc[m], 0, 0, 0);
                }
            __builtin_amdgcn_sched_barrier(0);
            if (more) {
                issue_piece(t + ST_PD, 2 * ks);
                issue_piece(t + ST_PD, 2 * ks + 1);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- epilogue.  acc[m][r]: row = 32 m + (lane & 31), col = n0 + 32 w + 8 (r >> 2) + 4 (lane >> 5) + (r & 3)
    const int colb = n0 + 32 * w + 4 * (lane >> 5);
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int row = 32 * m + (lane & 31);
        if (m < MB && row < p.M) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int col = colb + 8 * g;
                if (col < p.N) {
                    const size_t off = (size_t)bz * p.sC + (size_t)row * p.ldc + col;
                    if constexpr (EPI == EPI_F32) {
                        st16(reinterpret_cast<float*>(p.C) + off, make_float4(acc[m][4 * g + 0], acc[m][4 * g + 1], acc[m][4 * g + 2], acc[m][4 * g + 3]));
                    } else {
                        const float o0 = acc[m][4 * g + 0], o1 = acc[m][4 * g + 1], o2 = acc[m][4 * g + 2], o3 = acc[m][4 * g + 3];
                        uint2 v;
                        v.x = FT == 1 ? pack2h(o0, o1) : pack2(o0, o1);
                        v.y = FT == 1 ? pack2h(o2, o3) : pack2(o2, o3);
                        st8(reinterpret_cast<bf16_t*>(p.C) + off, v);
                        if (FT != 1 && p.split_off != 0) {                   // split-bf16 result: lo = bf16(acc - hi) to the lo plane (vqs_kernels.h)
                            uint2 l;
                            l.x = pack2(o0 - __uint_as_float(v.x << 16), o1 - __uint_as_float(v.x & 0xffff0000u));
                            l.y = pack2(o2 - __uint_as_float(v.y << 16), o3 - __uint_as_float(v.y & 0xffff0000u));
                            st8(reinterpret_cast<bf16_t*>(p.C) + p.split_off + off, l);
                        }
                    }
                }
            }
        }
    }
}

// Which launches take the stream form: few rows per batch entry, no bias / row scale, enough (batch entry, 128-column) items to
// put a workgroup on most CUs, operands addressable with 32-bit byte offsets.  Bitwise the 8-wave forms' results, so the rule may
// depend on M and the batch count.
// Fewest work items (128-column blocks x batch entries) for which a launch of <= 128 rows takes this form.  Rounds 4-5: 192 (a full chip: the form was built for
// the bench batch's cross-attention products).  Round 6: 4 -- at B <= 32 EVERY decoder linear has <= 128 stacked rows, streams its weight from HBM exactly once
// and, as a 256 x 256 persistent launch, occupied 48-80 CUs with 2-4 of a tile's 256 rows valid (B = 1: 44-96 us per launch against 16-41 here; the whole pass
// 30.2 -> 23.9 ms, every B <= 32 about 5.5 ms less; profiles/r6_call21/22_*).  Same bits (header), so the rule stays a function of the launch's shape only and
// never shows in a pair's score: digests of the scores at B = 1 .. 32 are the old rule's (same records).  Larger batches have more than 128 rows: unchanged.
#ifndef VQS_STREAM_MIN_ITEMS
#define VQS_STREAM_MIN_ITEMS 4
#endif
static bool stream_eligible(const GemmParams& p, int epi) {
    if (!(epi == EPI_F32 || epi == EPI_BF16) || p.no_stream) return false;
    if (p.M > 128 || p.bias != nullptr || p.rowss_in != nullptr || (p.K % 64) != 0 || (p.N % 4) != 0) return false;
    if ((p.lda % 8) != 0 || (p.ldw % 8) != 0 || (p.ldc % 4) != 0 || (p.split_off % 4) != 0) return false;
    const long long items = (long long)((p.N + 127) / 128) * (p.batch > 0 ? p.batch : 1);
    if (items < VQS_STREAM_MIN_ITEMS) return false;
    return (uint64_t)p.M * (uint64_t)p.lda * 2ull < (1ull << 31) && (uint64_t)p.N * (uint64_t)p.ldw * 2ull < (1ull << 31);
}
