"""Cases, references and expectations of the single-launch tests of the Qwen2.5-VL prefill's glue and of the bind-time range proof
(tests/test_gpu_qwen_glue_kernels.py; proven without a GPU by tests/test_qwen_glue_inputs.py).  Kernels: norm_rows_reg_kernel / norm_rows_loop_kernel
with scales, rope_qk_kernel, qwen_embed_kernel, the bf16 / fp32 gathers (csrc/elementwise.hip), f16_to_bf16_rows_kernel, qwen_tail_rope_q_kernel,
rowbound_kernel, absmax_bf16_kernel, gate_pair_bound_kernel (csrc/qwen_decode.hip).

Three kinds of expectation:
  exact       copies, and arithmetic on inputs chosen so that every fp32 expression is exact in any contraction (small integers, tables from
              {0, +-1/4, ..., +-1}, power-of-two scales): the expected BUFFER -- guards, pad columns and untouched lanes included -- is compared bit for bit
  criterion   random inputs against a float64 reference with one rounding to the 16-bit type, under compare_tap's per-launch criterion
              (oracle/clip_t5_engine_rounding.py: one own ulp; 0.5 % of a bf16 / 2 % of an fp16 tensor different at all)
  bound       fp32 results against float64 under a bound derived from the operation count (tail rope, row bounds), stated where it is used
Every reference takes `mistake`: the planted errors of MISTAKES, each of which must change the expectation of every case it applies to.

Every index map of every case is in range: the kernels define nothing else (qwen_embed's token ids excepted: the kernel clamps them)."""
import functools
import math
import zlib

import torch

SENT16 = 0x7FC1                   # 16-bit pattern of every element a launch must not write: a quiet NaN in bf16 and in fp16
SENT32 = 0x7FC12345               # the same for fp32 / int32 tensors
GUARD = 2048                      # guard elements in front of and behind every tensor a launch writes
MAX_OWN_ULPS = 1.001              # _stage_locked_impl's conditions (tests/test_gpu_qwen.py)
MAX_FRAC_DIFF = {7: 5e-3, 10: 2e-2}
MANT = {torch.bfloat16: 7, torch.float16: 10}
BITS = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32, torch.int32: torch.int32}

MISTAKES = ("d_swapped", "out_on_stream", "mean_over_out_ld",                                         # scaled RMSNorm
            "partner_hd_half", "k_heads_by_hq", "table_row_by_s", "rotate_pad_lanes",                 # rope_qk / tail_rope_q
            "src1_row_off_by_one", "no_zero_fill", "pair_blocks_of_32", "g_clamped", "unscale_after_rounding")


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def criterion(ref16, out16):
    """compare_tap's per-launch criterion on two tensors of one 16-bit type -> (ok, report)"""
    from oracle.clip_t5_engine_rounding import compare_tap
    m = MANT[out16.dtype]
    r = compare_tap(ref16.float(), out16.float(), mant_bits=m)
    return r["max_own_ulps"] <= MAX_OWN_ULPS and r["frac_diff"] <= MAX_FRAC_DIFF[m], r


# ---------------------------------------------------------------------------------------------------- guarded buffers
class Buf:
    """A [rows, ld] tensor between two guards of GUARD elements; every element holds the sentinel pattern until something is written."""

    def __init__(self, rows, ld, dtype, device="cpu"):
        bits = BITS[dtype]
        pat = SENT16 if bits == torch.int16 else SENT32
        self.rows, self.ld, self.dtype = rows, ld, dtype
        self.flat = torch.full((2 * GUARD + rows * ld,), pat, dtype=bits, device=device).view(dtype)
        self.body = self.flat[GUARD:GUARD + rows * ld].view(rows, ld)

    @classmethod
    def of(cls, t, ld=None, device="cpu"):
        """t [rows, cols] in columns [0, cols) of a buffer of pitch ld (default cols)"""
        t = t.reshape(t.shape[0], -1) if t.dim() != 2 else t
        b = cls(t.shape[0], ld or t.shape[1], t.dtype, device)
        b.body[:, :t.shape[1]] = t.to(device)
        return b

    def ptr(self):
        return self.body.data_ptr()

    def bits(self):
        return self.flat.view(BITS[self.dtype]).cpu()

    def outside(self, cols):
        """True when everything but columns [0, cols) of the body still holds the sentinel"""
        f = self.flat.view(BITS[self.dtype]).clone()
        pat = SENT16 if f.dtype == torch.int16 else SENT32
        f[GUARD:GUARD + self.rows * self.ld].view(self.rows, self.ld)[:, :cols] = pat
        return bool((f == pat).all())


def first_difference(got, want):
    i = int(torch.nonzero(got != want)[0])
    return f"element {i - GUARD} of the body (guards: {GUARD} in front): {int(got[i]):#x} != {int(want[i]):#x}; {int((got != want).sum())} differ"


# ---------------------------------------------------------------------------------------------------- scaled RMSNorm
NORM_EPS = float(torch.tensor(1e-6, dtype=torch.float32))
NORM_M = (1, 7, 70)                                   # one row; two workgroups with a ragged second; 17.5 workgroups
NORM_D = (200, 1024, 1280, 3584)                      # the loop kernel; the register forms NV = 4, 5 (vision tower), 14 (7B language model)
NORM_SCALES = ((1.0, 1.0, 1.0), (4.0, 0.5, 0.25), (2.0 ** -3, 2.0 ** 6, 2.0 ** -6))        # (d1, d2, out)
NORM_MODES = {torch.float16: (0, 1, 2, 3), torch.bfloat16: (0, 1, 3)}                      # the unstored form has no bf16 instantiation


def norm_pitches(D):
    return (D, (D // 512 + 1) * 512)                  # dense; the next multiple of 512 above D (3584 -> 4096: the engine's own x pitch)


@functools.lru_cache(maxsize=None)
def norm_inputs(M, D):
    """x = 3 randn + 0.5 (a mean the RMS norm must not remove), two unit normal fields the deltas are cut from, w bf16 around 1"""
    g = _gen("norm", M, D)
    x = 3.0 * torch.randn(M, D, generator=g) + 0.5
    r1, r2 = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    w = (1.0 + 0.25 * torch.randn(D, generator=g)).to(torch.bfloat16)
    return x, r1, r2, w


def norm_deltas(M, D, sc):
    """the stored fp16 deltas: deviation 0.5 / d, so that the true deltas d * delta have deviation 0.5 under every scale"""
    _, r1, r2, _ = norm_inputs(M, D)
    return (r1 * (0.5 / sc[0])).to(torch.float16), (r2 * (0.5 / sc[1])).to(torch.float16)


def norm_expected(x, dl1, dl2, w, mode, sc, out_dtype, acc=torch.float64, out_ld=None, mistake=None):
    """-> (what x holds after the launch, fp32 bit for bit; the operand [M, D] in out_dtype: norm in `acc`, one rounding).
    The stream is (x + d1 delta1) + d2 delta2 in fp32 in that order; the products are exact (power-of-two scales), so a contraction changes nothing."""
    d1, d2, so = sc
    if mistake == "d_swapped":
        d1, d2 = d2, d1
    v = x
    if mode in (1, 2, 3):
        v = v + dl1.float() * d1
    if mode == 3:
        v = v + dl2.float() * d2
    if mistake == "out_on_stream":
        v, so = v * so, 1.0
    stored = v if mode in (1, 3) else x
    div = out_ld if (mistake == "mean_over_out_ld" and out_ld) else x.shape[1]
    va = v.to(acc)
    rs = torch.rsqrt((va * va).sum(-1, keepdim=True) / div + NORM_EPS)
    return stored, (va * rs * w.to(acc) * so).to(out_dtype)


def norm_mistake_applies(mistake, mode, sc, D, out_ld):
    return {"d_swapped": mode != 0 and sc[0] != sc[1], "out_on_stream": sc[2] != 1.0, "mean_over_out_ld": out_ld != D}[mistake]


# ---------------------------------------------------------------------------------------------------- rope_qk, tail_rope_q
ROPE_HEADS = ((4, 4), (4, 2), (7, 1))                 # (Hq, Hk): no grouping, 2 : 1, 7 : 1 (the 7B model's ratio) with an odd head count
ROPE_B = 2
ROPE_S = (1, 31, 32, 33, 70)                          # one row; either side of the 32-row block; three blocks with a ragged last
ROPE_LANES = ((128, 64), (128, 40), (64, 32), (128, 8))      # (hd, half): the language model; the vision tower's 80-lane heads in 128-lane slots; a narrow head; one chunk
ROPE_TABLE_VALUES = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, -0.25, -0.5, -0.75, -1.0])


def rope_inputs(Hq, Hk, S, hd, half, dtype, exact, B=ROPE_B, scale=1.0):
    """q [B, Hq, S, hd], k [B, Hk, S, hd] in dtype, cos / sin fp32 [B S, half].  exact: integers in [-7, 7] against tables from ROPE_TABLE_VALUES --
    every product is a multiple of 1/4 below 8 and every sum below 16: exact in fp32, in bf16 and in fp16 whatever is contracted.  Otherwise unit
    normal values times `scale` against the cosine and sine of random angles."""
    g = _gen("rope", Hq, Hk, S, hd, half, exact)
    if exact:
        q = torch.randint(-7, 8, (B, Hq, S, hd), generator=g).to(dtype)
        k = torch.randint(-7, 8, (B, Hk, S, hd), generator=g).to(dtype)
        cos = ROPE_TABLE_VALUES[torch.randint(0, 9, (B * S, half), generator=g)]
        sin = ROPE_TABLE_VALUES[torch.randint(0, 9, (B * S, half), generator=g)]
    else:
        q = (torch.randn(B, Hq, S, hd, generator=g) * scale).to(dtype)
        k = (torch.randn(B, Hk, S, hd, generator=g) * scale).to(dtype)
        ang = torch.rand(B * S, half, generator=g, dtype=torch.float64) * (2.0 * math.pi)
        cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
    return q, k, cos.contiguous(), sin.contiguous()


def rope_expected(x, cos, sin, half, acc=torch.float64, walk_heads=None, mistake=None):
    """x [B, H, S, hd] rotated (rotate-half over lanes [0, 2 half), table row b S + s), arithmetic in `acc`, one rounding to x's type; the other lanes
    keep their bits.  walk_heads: the head count the row index is taken apart with (mistake k_heads_by_hq: Hq for the k tensor)."""
    B, H, S, hd = x.shape
    rows = x.reshape(B * H * S, hd).to(acc)
    r = torch.arange(B * H * S)
    b, s = r // ((walk_heads or H) * S), r % S
    tok = s if mistake == "table_row_by_s" else b * S + s
    c, sn = cos[tok].to(acc), sin[tok].to(acc)
    p = hd // 2 if mistake == "partner_hd_half" else half
    a, bb = rows[:, :half], rows[:, p:p + half]
    out = rows.clone()
    if mistake == "rotate_pad_lanes" and 2 * half < hd:
        lanes = torch.arange(2 * half, hd)
        out[:, lanes] = rows[:, lanes] * c[:, lanes % half] - rows[:, lanes] * sn[:, lanes % half]
    out[:, :half] = a * c - bb * sn
    out[:, p:p + half] = bb * c + a * sn
    return out.to(x.dtype).reshape(B, H, S, hd)


def rope_qk_expected(q, k, cos, sin, half, acc=torch.float64, mistake=None):
    Hq = q.shape[1]
    return (rope_expected(q, cos, sin, half, acc, None, mistake),
            rope_expected(k, cos, sin, half, acc, Hq if mistake == "k_heads_by_hq" else None, mistake))


def rope_mistake_applies(mistake, Hq, Hk, hd, half, B=ROPE_B):
    return {"partner_hd_half": 2 * half != hd, "k_heads_by_hq": Hq != Hk and B > 1, "table_row_by_s": B > 1, "rotate_pad_lanes": 2 * half < hd}[mistake]


TAIL_B = 3


def tail_rope_inputs(Hq, hd, half, exact, B=TAIL_B, pad=24, table_rows=11):
    """qkv fp32 [B, ld] with ld = Hq hd + pad (the k | v columns stand behind the q columns), cos / sin fp32 [table_rows, half], row int32 [B]: different
    table rows per sample, the last one included"""
    g = _gen("tail_rope", Hq, hd, half, exact)
    ld = Hq * hd + pad
    if exact:
        qkv = torch.randint(-7, 8, (B, ld), generator=g).float()
        cos = ROPE_TABLE_VALUES[torch.randint(0, 9, (table_rows, half), generator=g)].contiguous()
        sin = ROPE_TABLE_VALUES[torch.randint(0, 9, (table_rows, half), generator=g)].contiguous()
    else:
        qkv = torch.randn(B, ld, generator=g)
        ang = torch.rand(table_rows, half, generator=g, dtype=torch.float64) * (2.0 * math.pi)
        cos, sin = torch.cos(ang).float(), torch.sin(ang).float()
    row = torch.tensor([table_rows - 1, 4, 0][:B], dtype=torch.int32)
    return qkv, ld, cos, sin, row


def tail_rope_expected(qkv, cos, sin, row, Hq, hd, half, acc=torch.float64, mistake=None):
    """-> (q_out [B, Hq hd] in acc, |a c| + |b s| of every element: 0 for the lanes that are copied)"""
    B = qkv.shape[0]
    x = qkv[:, :Hq * hd].reshape(B, Hq, hd).to(acc)
    tr = torch.arange(B) if mistake == "table_row_by_s" else row.long()
    c, sn = cos[tr].to(acc)[:, None, :], sin[tr].to(acc)[:, None, :]
    p = hd // 2 if mistake == "partner_hd_half" else half
    a, bb = x[..., :half], x[..., p:p + half]
    out, mag = x.clone(), torch.zeros_like(x)
    if mistake == "rotate_pad_lanes" and 2 * half < hd:
        lanes = torch.arange(2 * half, hd)
        out[..., lanes] = x[..., lanes] * c[..., lanes % half] - x[..., lanes] * sn[..., lanes % half]
    out[..., :half], out[..., p:p + half] = a * c - bb * sn, bb * c + a * sn
    mag[..., :half], mag[..., p:p + half] = (a * c).abs() + (bb * sn).abs(), (bb * c).abs() + (a * sn).abs()
    return out.reshape(B, Hq * hd), mag.reshape(B, Hq * hd)


TAIL_ROPE_BOUND = 3.0 * 2.0 ** -24        # two products and one sum, each within half an fp32 ulp (2^-24 relative) of terms no larger than |a c| + |b s|


# ---------------------------------------------------------------------------------------------------- gathers, embed, fp16 -> bf16
def rand_bf16(shape, g):
    """random finite bf16 bit patterns: every exponent but the top one, both signs (a copy must keep subnormals and negative zeros too)"""
    bits = torch.randint(0, 1 << 16, shape, generator=g, dtype=torch.int32)
    bits = torch.where((bits & 0x7F80) == 0x7F80, bits & ~0x4000, bits)
    return bits.to(torch.int16).view(torch.bfloat16)


def gather_rows_expected(src0, src1, rmap, cols, dst_ld, mistake=None):
    """torch indexing restatement -> [rows, dst_ld] bf16: map >= 0 row of src0, <= -2 row -m-2 of src1, -1 zeros; columns >= cols zero"""
    n = len(rmap) if rmap is not None else src0.shape[0]
    m = torch.arange(n) if rmap is None else rmap.long()
    out = torch.zeros(n, dst_ld, dtype=torch.bfloat16)
    if mistake == "no_zero_fill":
        out = torch.full((n, dst_ld), SENT16, dtype=torch.int16).view(torch.bfloat16)
        out[:, :cols] = 0
    out[m >= 0, :cols] = src0[m[m >= 0], :cols]
    if bool((m <= -2).any()):
        r1 = -m[m <= -2] - 2
        if mistake == "src1_row_off_by_one":              # row -m-1 (wrapped, so that the restatement itself stays in range)
            r1 = (r1 + 1) % src1.shape[0]
        out[m <= -2, :cols] = src1[r1, :cols]
    return out


def gate_up_map(mlp_p):
    """the packed gate | up row map of vqs_qwen.cpp: blocks of 64 rows = 32 gate rows (src0) | 32 up rows (src1, coded -r-2)"""
    j = torch.arange(2 * mlp_p)
    blk, within = j // 64, j % 64
    r = blk * 32 + within % 32
    return torch.where(within < 32, r, -r - 2).to(torch.int32)


# (name, rows of dst, cols, src_ld, dst_ld, kind of map): the engine's uses and the edges of the one-workgroup-per-row loop
GATHER_ROWS_CASES = (
    ("identity-1row", 1, 64, 64, 64, "identity"),
    ("identity-pad-1176-1216", 5, 1176, 1176, 1216, "identity"),          # patch rows padded to the GEMM's K (src_ld != dst_ld, zero fill)
    ("identity-wide-src", 9, 300, 320, 300, "identity"),                  # the last-position rows out of a wider pitch; dst_ld no multiple of 256
    ("perm-257", 257, 128, 128, 128, "perm"),
    ("perm-zero-rows", 70, 1280, 1280, 1280, "perm-1"),                   # window permutation with the -1 padding slots of a partial window
    ("heads-pad", 96, 200, 200, 264, "perm-1"),
    ("gate-up-64", 128, 200, 200, 256, "gateup"),                         # 32 | 32 rows of two sources
    ("gate-up-bias", 192, 1, 1, 1, "gateup"),                             # bias vectors: one column, pitch 1
    ("perm-bias", 130, 1, 1, 1, "perm-1"),
)


def gather_rows_inputs(name):
    _, rows, cols, src_ld, dst_ld, kind = next(c for c in GATHER_ROWS_CASES if c[0] == name)
    g = _gen("gather_rows", name)
    if kind == "identity":
        nsrc, rmap = rows, None
    elif kind == "gateup":
        nsrc, rmap = rows // 2, gate_up_map(rows // 2)
    else:
        nsrc = rows + 3
        rmap = torch.randperm(nsrc, generator=g)[:rows].to(torch.int32)
        if kind == "perm-1":
            rmap[torch.randperm(rows, generator=g)[:max(rows // 8, 1)]] = -1
    src0 = rand_bf16((nsrc, src_ld), g)
    src1 = rand_bf16((nsrc, src_ld), g) if kind == "gateup" else None
    return src0, src1, rmap, rows, cols, src_ld, dst_ld


def gather_cols_inputs(direction):
    """the o / proj weight's column map between 80-lane heads and 128-lane slots: 'spread' 3 heads x 80 columns -> 3 x 128 (pad lanes -1),
    'compact' the inverse selection 3 x 128 -> 3 x 80"""
    g = _gen("gather_cols", direction)
    c = torch.arange(384)
    if direction == "spread":
        src_ld, cmap = 240, torch.where(c % 128 < 80, (c // 128) * 80 + c % 128, -1)
    else:
        c = torch.arange(240)
        src_ld, cmap = 384, (c // 80) * 128 + c % 80
    rows = 37
    return rand_bf16((rows, src_ld), g), cmap.to(torch.int32), rows, src_ld, len(cmap)


def gather_cols_expected(src, cmap):
    m = cmap.long()
    out = src[:, m.clamp_min(0)].clone()
    out[:, m < 0] = 0
    return out


GATHER_F32_D = (4, 320, 1280)             # one float4; more than one pass of 256 threads only at 1280 (320 float4)


def gather_f32_inputs(D, form):
    """form 0 (elementwise.hip): dense rows, -1 = zero row; form 1 (qwen_decode.hip): source pitch D + 8, no zero rows"""
    g = _gen("gather_f32", D, form)
    rows, nsrc = 19, 23
    src_ld = D if form == 0 else D + 8
    src = torch.randint(-(1 << 31), (1 << 31) - 1, (nsrc, src_ld), generator=g, dtype=torch.int64).to(torch.int32)
    src = torch.where((src & 0x7F800000) == 0x7F800000, src & ~0x40000000, src).view(torch.float32)
    rmap = torch.randperm(nsrc, generator=g)[:rows].to(torch.int32)
    if form == 0:
        rmap[[2, 11]] = -1
    return src, rmap, rows, src_ld


def gather_f32_expected(src, rmap, D):
    m = rmap.long()
    out = src[m.clamp_min(0), :D].clone()
    out[m < 0] = 0
    return out


EMBED_D = (128, 3584)                     # half a pass of 256 threads; 14 passes
EMBED_VOCAB, EMBED_SLOTS = 41, 9


def embed_inputs(D, merged_f16):
    """ids with tokens below 0 and at / above the vocabulary (clamped by the kernel), vision rows interleaved with text rows"""
    g = _gen("embed", D, merged_f16)
    rows = 29
    ids = torch.randint(0, EMBED_VOCAB, (rows,), generator=g).to(torch.int32)
    ids[1], ids[5], ids[8], ids[rows - 1] = -3, EMBED_VOCAB, EMBED_VOCAB + 1000, -(1 << 31)
    vis = torch.full((rows,), -1, dtype=torch.int32)
    where = torch.tensor([2, 3, 4, 9, 10, 20, 27])
    vis[where] = torch.tensor([0, 1, 2, 8, 7, 3, 5], dtype=torch.int32)
    embed = rand_bf16((EMBED_VOCAB, D), g)
    merged = (torch.randn(EMBED_SLOTS, D, generator=g) * 8).to(torch.float16) if merged_f16 else rand_bf16((EMBED_SLOTS, D), g)
    return ids, vis, embed, merged, rows


def embed_expected(ids, vis, embed, merged, unscale):
    """fp32 [rows, D]; an fp16 vision row times a power of two is exact in fp32"""
    tok = embed[ids.long().clamp(0, embed.shape[0] - 1)].float()
    v = merged[vis.long().clamp_min(0)].float()
    if merged.dtype == torch.float16:
        v = v * unscale
    return torch.where((vis >= 0)[:, None], v, tok)


F16_COLS = (8, 2040, 8 * 256 * 3 + 8)     # one 16-byte chunk; 255 chunks (a ragged workgroup); 769 chunks (four workgroups, the last with one chunk)
F16_COLS_STRIDE = 8 * (1024 * 256 + 1)    # one chunk more than the largest grid covers in one pass: the only size at which the grid-stride loop takes a second step


def f16_rows_inputs(cols, rows=5):
    """random finite fp16 bit patterns (subnormals, both zeros, every exponent) with the edge values planted in row 0: the fp16 maximum, the smallest
    subnormal, exact bf16 midpoints that tie to even downwards and upwards, and their neighbours above and below"""
    g = _gen("f16_rows", cols)
    src_ld = cols + 24
    bits = torch.randint(0, 1 << 16, (rows, src_ld), generator=g, dtype=torch.int32)
    bits = torch.where((bits & 0x7C00) == 0x7C00, bits & ~0x4000, bits)
    # 1 + m 2^-10: bf16 keeps 7 bits, so m = 4 (tie, down to even), 12 (tie, up to even), 5 and 3 (either side of the midpoint), 0x3FF (carries into the exponent)
    edge = [0x7BFF, 0xFBFF, 0x0001, 0x8001, 0x03FF, 0x0400, 0x3C04, 0x3C0C, 0x3C05, 0x3C03, 0x3FFF, 0xBC04, 0xBC0C, 0x0000, 0x8000, 0x3C00]
    for i, e in enumerate(edge[:min(len(edge), cols)]):
        bits[0, i] = e
    return bits.to(torch.int16).view(torch.float16), src_ld


def f16_rows_expected(src, cols, unscale, mistake=None):
    """bf16(fp16 * unscale): the fp32 product of an 11-bit significand with a power of two (or with 3) is exact, so this is ONE rounding to nearest even"""
    x = src[:, :cols].float()
    if mistake == "unscale_after_rounding":
        return (x.to(torch.bfloat16).float() * unscale).to(torch.bfloat16)
    return (x * unscale).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------- range proof
ABSMAX_N = (1, 255, 256, 257, 2048 * 256 + 3)         # one element; around one workgroup; three elements past one full pass of the largest grid
ABSMAX_R = float(torch.tensor(1280.0, dtype=torch.float32).sqrt())


def absmax_inputs(n):
    """bf16 values below 4 in magnitude with the maximum, negative, in the LAST element"""
    g = _gen("absmax", n)
    x = (torch.rand(n, generator=g) * 4.0 - 2.0).to(torch.bfloat16)
    x[n - 1] = -5.5
    return x


def absmax_expected(x, R, seed=0.0):
    return torch.maximum(torch.tensor(seed, dtype=torch.float32), torch.tensor(R, dtype=torch.float32) * x.float().abs().max())


def gate_pair_inputs(mlp_p):
    g = _gen("gate_pair", mlp_p)
    return torch.rand(2 * mlp_p, generator=g) * 3.0 + 0.125


def gate_pair_expected(rb, mlp_p, ld, mistake=None):
    """u_act fp32 [ld]: the fp32 product of gate row and up row of the packed 32 | 32 blocks, 0 behind mlp_p"""
    j = torch.arange(mlp_p)
    blk = 32 if mistake == "pair_blocks_of_32" else 64
    u = torch.zeros(ld)
    u[:mlp_p] = rb[(j // 32) * blk + j % 32] * rb[(j // 32) * blk + 32 + j % 32]
    return u


ROWBOUND_N = (1, 4, 5, 130)               # one row; one full workgroup; one row into the second; 32.5 workgroups
ROWBOUND_K = (8, 64, 100, 320)            # fewer columns than lanes; one pass; a ragged second pass; five passes
ROWBOUND_R_EXACT = 2.0                    # a power of two: R sqrt(.) is exact, so the bias add rounds once whether it is contracted or not


def rowbound_inputs(N, K, exact, pad=8):
    """W bf16 [N, K + pad], g bf16 [K] (read as [K / 4] for the merger's wrap), u fp32 [K], bias bf16 [N].  exact: non-zero integers in [-3, 3], g cycling
    through {1/2, 1, 2} (so that a wrapped and a clamped index read different values), u from the same set: every term is a multiple of 1/4 and every
    sum stays far below 2^24 such units -- exact in any order."""
    gen = _gen("rowbound", N, K, exact)
    if exact:
        W = (torch.randint(1, 4, (N, K + pad), generator=gen) * (2 * torch.randint(0, 2, (N, K + pad), generator=gen) - 1)).to(torch.bfloat16)
        pick = torch.tensor([0.5, 1.0, 2.0])
        g = pick[torch.arange(K) % 3].to(torch.bfloat16)
        u = pick[torch.randint(0, 3, (K,), generator=gen)]
        bias = torch.randint(-4, 5, (N,), generator=gen).to(torch.bfloat16)
    else:
        W = (torch.randn(N, K + pad, generator=gen) * K ** -0.5).to(torch.bfloat16)
        g = (1.0 + 0.5 * torch.randn(K, generator=gen)).to(torch.bfloat16)
        u = torch.rand(K, generator=gen) * 4.0
        bias = torch.randn(N, generator=gen).to(torch.bfloat16)
    return W, g, u, bias


def rowbound_expected(W, K, mode, g, g_len, R, u, uconst, bias, acc=torch.float64, mistake=None):
    """[N] in acc: mode 0 R sqrt(sum_k (W[j, k] g[k % g_len])^2) + |bias[j]|, mode 1 sum_k |W[j, k]| u[k] + |bias[j]| (u None: the constant uconst)"""
    w = W[:, :K].to(acc)
    if mode == 0:
        k = torch.arange(K)
        gi = k.clamp_max(g_len - 1) if mistake == "g_clamped" else k % g_len
        t = w * g[gi].to(acc)
        b = torch.sqrt((t * t).sum(1)) * R
    else:
        b = (w.abs() * (u.to(acc) if u is not None else torch.full((K,), uconst, dtype=acc))).sum(1)
    return b + bias.to(acc).abs() if bias is not None else b


def rowbound_expected_exact(W, K, mode, g, g_len, R, u, uconst, bias):
    """[N] fp32, the bits an exact case must produce: the sums are exact, so the kernel rounds at the square root (correctly rounded; taken here in
    float64 and rounded to fp32, which gives the correctly rounded fp32 root -- fp32 square roots of the host differ between machines) and at the bias
    add (R is a power of two, so R sqrt(.) is exact and the add rounds once, contracted or not)."""
    b = rowbound_expected(W, K, mode, g, g_len, 1.0, u, uconst, None)
    if mode == 0:
        b = b.float().double() * R
    return (b + bias.double().abs() if bias is not None else b).float()


def rowbound_bound(K):
    """relative: a K-term fp32 sum of non-negative terms (each addition and each product within 2^-24), the square root, the product by R, the bias add"""
    return (K + 16) * 2.0 ** -24


ROWBOUND_HEADROOM = 32768.0 / 32767.0     # the host's head room over a device bound (vqs_qwen.cpp): the device must stay inside it
ROWBOUND_ARITH_K = (100, 1280, 5120)
ROWBOUND_ARITH_N = 130
