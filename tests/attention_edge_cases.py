"""Inputs and expectations of the exact-selection attention tests (tests/test_gpu_attention_edges.py runs them on the kernels,
tests/test_attention_edge_inputs.py proves on the CPU that the expectations are properties of the operation).  Everything here is plain
torch on the CPU.

The construction.  Key rows are +-1 codes, query i of head h is c * K[pi_h(i)] with c a power of two, V is random in the tensor type.  The
needle's score is c * hd * scale; with G = (needle - second largest visible score) * log2 e >= 200 every other probability and every rescale
factor 2^-G is below the smallest fp32 denormal (2^-149), i.e. exactly 0, the needle's probability is 2^(rounding error of one product) = 1.0
once packed to 8 or 11 significant bits, the row sum is exactly 1 and the output row is V[pi_h(i)] bit for bit -- in any correct fp32 softmax,
tiled or not.  A key dropped, duplicated or swapped, a diagonal hidden, a key too many at a ragged end then changes whole rows."""
import math

import torch

LOG2E = 1.4426950408889634
G_MIN = 200.0
SENTINEL = 0x5A5A                 # 16-bit pattern of the guard rows: finite in bf16 (1.5e13) and in fp16 (203.25)
GUARD = 16                        # guard rows in front of and behind every output

NONCAUSAL_MAPS = ("perm", "anti", "last", "first")
CAUSAL_MAPS = ("diag", "prev", "tile_first", "prev_tile_last", "rand_le")


def dtype_of(f16):
    return torch.float16 if f16 else torch.bfloat16


def ragged_key_lens(S):
    """One sample per length: both sides of the 64-key tile boundaries, one key, the last key cut, whole, and past the end (clamped)."""
    return [1, 63, 64, 65, 127, 128, 129, S - 1, S, S + 5]


def key_map(name, S, klen, gen):
    """pi [S]: the key query i selects, always < klen; the causal maps also keep pi(i) <= i."""
    i = torch.arange(S)
    if name == "perm":                              # a permutation when klen == S
        return torch.randperm(klen, generator=gen)[i % klen]
    if name == "anti":
        return (klen - 1 - i) % klen
    if name == "last":
        return torch.full((S,), klen - 1, dtype=torch.long)
    if name == "first":
        return torch.zeros(S, dtype=torch.long)
    if name == "diag":                              # the diagonal must be visible
        pi = i
    elif name == "prev":
        pi = (i - 1).clamp(min=0)
    elif name == "tile_first":
        pi = 64 * (i // 64)
    elif name == "prev_tile_last":                  # the last key of the previous 64-key tile
        pi = (64 * (i // 64) - 1).clamp(min=0)
    elif name == "rand_le":
        pi = (torch.rand(S, generator=gen) * (i + 1).float()).long().clamp(max=i)
    else:
        raise ValueError(name)
    return pi.clamp(max=klen - 1)


class Case:
    """q [B,H,S,hd], k / v [B,Hkv,S,hd] (tensor type), table fp32 [H, 2S-1] or None, key_len list or None, pi [B,H,S] long,
    rows bool [B,S] = the query rows that are compared."""

    def __init__(self, **kw):
        self.table = self.key_len = None
        self.causal = False
        self.out_hd = 0
        self.__dict__.update(kw)

    @property
    def klens(self):
        B, S = self.q.shape[0], self.q.shape[2]
        return [S] * B if self.key_len is None else [min(x, S) for x in self.key_len]

    def key_len_tensor(self, device="cpu"):
        return None if self.key_len is None else torch.tensor(self.key_len, dtype=torch.int32, device=device)


def build_selection(B, H, Hkv, S, hd, maps, dtype, c, seed, key_len=None, live=None, poison=False):
    """The construction of the module docstring.  Head h of sample b takes maps[(b * H + h) % len(maps)].  live < hd: lanes >= live of q, k, v
    are zero (the vision tower's 80-lane heads).  poison: key rows at positions >= key_len hold twice the code of key key_len - 1 and value
    rows there hold 1000 -- masked keys that would win every row of the 'last' map, and change it, if one of them were visible.  A sample
    with key_len 0 has no key to select (pi = 0, q = 0)."""
    g = torch.Generator().manual_seed(seed)
    live = hd if live is None else live
    rep = H // Hkv
    k = (torch.randint(0, 2, (B, Hkv, S, hd), generator=g) * 2 - 1).float()
    v = torch.randn(B, Hkv, S, hd, generator=g).to(dtype)
    v[v == 0] = 1.0                                  # no signed-zero question in the bitwise comparison
    k[..., live:] = 0
    v[..., live:] = 0
    q = torch.zeros(B, H, S, hd)
    pi = torch.zeros(B, H, S, dtype=torch.long)
    klens = [S] * B if key_len is None else [min(x, S) for x in key_len]
    for b in range(B):
        if klens[b] == 0:
            continue
        for h in range(H):
            pi[b, h] = key_map(maps[(b * H + h) % len(maps)], S, klens[b], g)
            q[b, h] = c * k[b, h // rep, pi[b, h]]
    if poison:
        for b in range(B):
            if 0 < klens[b] < S:
                k[b, :, klens[b]:] = 2 * k[b, :, klens[b] - 1: klens[b]]
                v[b, :, klens[b]:, :live] = 1000.0
    rows = torch.arange(S)[None, :] < torch.tensor(klens)[:, None]
    return Case(q=q.to(dtype), k=k.to(dtype), v=v, pi=pi, rows=rows, key_len=key_len, live=live)


def scores_fp32(q, k, scale, table=None, key_len=None, causal=False):
    """[B,H,S,S] fp32 scores of the operation (grouped-query heads, bias[h, key - query], key-length and causal masks as -inf)."""
    B, H, S, _ = q.shape
    rep = H // k.shape[1]
    s = torch.einsum("bhqd,bhkd->bhqk", q.float(), k.float().repeat_interleave(rep, 1)) * scale
    ar = torch.arange(S)
    if table is not None:
        s = s + table.float()[:, ar[None, :] - ar[:, None] + S - 1][None]
    if key_len is not None:
        dead = ar[None, :] >= torch.tensor(key_len)[:, None]
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    if causal:
        s = s.masked_fill((ar[None, :] > ar[:, None])[None, None], float("-inf"))
    return s


def attention_fp32(q, k, v, scale, table=None, key_len=None, causal=False):
    """[B*S, H*hd] fp32: softmax(scores_fp32) . V"""
    B, H, S, hd = q.shape
    p = torch.softmax(scores_fp32(q, k, scale, table, key_len, causal), dim=-1)
    o = torch.einsum("bhqk,bhkd->bqhd", p, v.float().repeat_interleave(H // k.shape[1], 1))
    return o.reshape(B * S, H * hd)


def selection_margin(case, return_scores=False):
    """G of the case: the smallest distance, in log2 units, from a compared row's needle to its second-largest visible score (inf when the
    needle is the only visible key).  Asserts that the needle IS the largest score of every compared row and that the visible code rows of
    every key head are distinct."""
    S = case.q.shape[2]
    for b, klen in enumerate(case.klens):
        for hk in range(case.k.shape[1]):
            assert torch.unique(case.k[b, hk, :klen].float(), dim=0).shape[0] == klen, f"code rows of sample {b} head {hk} repeat"
    s = scores_fp32(case.q, case.k, case.scale, case.table, case.key_len, case.causal)
    rows = case.rows[:, None, :].expand(-1, s.shape[1], -1)
    assert torch.equal(s.argmax(-1)[rows], case.pi[rows]), "the needle is not the largest score"
    if S > 1:
        top = s.topk(2, dim=-1).values
        gap = ((top[..., 0] - top[..., 1]) * LOG2E)[rows]
    else:
        gap = torch.full((1,), float("inf"))
    G = float(gap.min()) if gap.numel() else float("inf")
    return (G, s) if return_scores else G


def expected_rows(case):
    """[B*S, H*w] in the tensor type: row i of head h is V[pi_h(i)] (w = out_hd or hd lanes of it)."""
    B, H, S, hd = case.q.shape
    w = case.out_hd if case.out_hd > 0 else hd
    vr = case.v.repeat_interleave(H // case.v.shape[1], 1)
    e = torch.gather(vr, 2, case.pi[..., None].expand(-1, -1, -1, hd))
    return e.permute(0, 2, 1, 3)[..., :w].reshape(B * S, H * w).contiguous()


def row_mask(case):
    """bool [B*S]: the compared rows of the token-major output."""
    return case.rows.reshape(-1)


# ---- hd 64: attn_fwd_dma_kernel / attn_fwd_dma_f16_kernel <HAS_BIAS>.  c * scale = 8 >= 5 in every mode (36 of 64 was the largest
# non-needle raw score measured: G >= 8 * 28 * log2 e = 323 before the bias, whose spread takes a few units off)
HD64_MODES = {"nobias": (0.125, 64.0, False), "bias_s1": (1.0, 8.0, True), "bias_s8": (0.125, 64.0, True)}
HD64_S = (1, 17, 63, 64, 65, 129, 577, 608)
HD64_SELECT = [(S, f16, mode, 2, 4) for S in HD64_S for f16 in (False, True) for mode in HD64_MODES]
HD64_SELECT += [(577, f16, mode, 1, 9) for f16 in (False, True) for mode in ("nobias", "bias_s1")]      # B.H = 9: not a multiple of 8, 5 query blocks


def hd64_case(S, f16, mode, B, H, key_len=None, maps=NONCAUSAL_MAPS, poison=False):
    scale, c, has_bias = HD64_MODES[mode]
    case = build_selection(B, H, H, S, 64, maps, dtype_of(f16), c, seed=S * 13 + B, key_len=key_len, poison=poison)
    case.scale = scale
    if has_bias:
        case.table = torch.randn(H, 2 * S - 1, generator=torch.Generator().manual_seed(S + 5))
    return case


# ---- hd 128: attn_fwd_hd_kernel<128, CAUSAL, F16>.  c * scale = 64 / sqrt(128) = 5.7: with the 80 live lanes of the tower's heads the needle's
# raw score is 80, not 128, and c = 32 would leave G near 160
HD128_SCALE, HD128_C = 128 ** -0.5, 64.0
HD128_S = (1, 64, 65, 200, 333)
HD128_SELECT = [(S, f16, causal, H, Hkv, out_hd, 2) for S in HD128_S for f16 in (False, True) for causal in (False, True)
                for H, Hkv in ((4, 4), (4, 2), (7, 1)) for out_hd in (0, 80)]
HD128_SELECT += [(333, f16, causal, 3, 1, 0, 3) for f16 in (False, True) for causal in (False, True)]    # B.H = 9, 3 query blocks


def hd128_case(S, f16, causal, H, Hkv, out_hd, B, key_len=None, maps=None, poison=False):
    maps = maps or (CAUSAL_MAPS if causal else NONCAUSAL_MAPS)
    case = build_selection(B, H, Hkv, S, 128, maps, dtype_of(f16), HD128_C, seed=S * 17 + H + B, key_len=key_len,
                           live=out_hd if out_hd > 0 else None, poison=poison)
    case.scale, case.causal, case.out_hd = HD128_SCALE, causal, out_hd
    return case


# ---- attn_suffix_hd_kernel<F16>: the causal kernel for the query rows [q0, S) only (key_len is mandatory there)
SUFFIX_SELECT = [(S, q0, f16) for S, q0 in ((333, 64), (200, 192)) for f16 in (False, True)]


def suffix_case(S, q0, f16, B=2, H=4, Hkv=2, key_len=None, maps=CAUSAL_MAPS, poison=False):
    case = hd128_case(S, f16, True, H, Hkv, 0, B, key_len=key_len if key_len is not None else [S] * B, maps=maps, poison=poison)
    case.q0 = q0
    case.rows = case.rows & (torch.arange(S)[None, :] >= q0)
    return case


# ---- ragged ends: one launch per map, one sample per key length
RAGGED_S, RAGGED_Q0 = 200, 64
HD64_RAGGED = [(m, f16, mode) for m in NONCAUSAL_MAPS for f16 in (False, True) for mode in HD64_MODES]
HD128_RAGGED = [(m, f16, causal, out_hd) for causal in (False, True) for m in (CAUSAL_MAPS if causal else NONCAUSAL_MAPS)
                for f16 in (False, True) for out_hd in (0, 80)]
SUFFIX_RAGGED = [(m, f16) for m in CAUSAL_MAPS for f16 in (False, True)]


def hd64_ragged_case(m, f16, mode):
    kl = ragged_key_lens(RAGGED_S)
    return hd64_case(RAGGED_S, f16, mode, len(kl), 1, key_len=kl, maps=(m,), poison=True)


def hd128_ragged_case(m, f16, causal, out_hd):
    kl = ragged_key_lens(RAGGED_S)
    return hd128_case(RAGGED_S, f16, causal, 1, 1, out_hd, len(kl), key_len=kl, maps=(m,), poison=True)


def suffix_ragged_case(m, f16):
    kl = ragged_key_lens(RAGGED_S)
    return suffix_case(RAGGED_S, RAGGED_Q0, f16, B=len(kl), H=1, Hkv=1, key_len=kl, maps=(m,), poison=True)


# ---- selection through the position-bias table alone (hd 64, HAS_BIAS)
BIAS_SELECT = [(S, f16, scale) for S in (64, 129, 608, 1100) for f16 in (False, True) for scale in (1.0, 0.125)]
BIAS_PEAK = 300.0                 # natural-log units: 433 log2 units above the zeros of the rest of the table


def bias_offsets(S):
    """key - query offsets of the peaks, one head each: every one of the four shifted LDS copies of the table (offset mod 4), both signs,
    the 64-key tile step and the two ends of the table."""
    seen = []
    for d in (0, 1, -1, 2, -2, 3, -3, 63, -63, 64, -64, S - 1, -(S - 1)):
        if abs(d) <= S - 1 and d not in seen:
            seen.append(d)
    return seen


def bias_select_case(S, f16, scale, key_len=None):
    """q = 0: the table is the only selector.  Row i of head h selects key i + d_h where that key exists and is visible; every other row is
    the uniform mean over the visible keys (the mask wins over the bias).  V holds integers of magnitude <= 8: every fp32 partial sum is an
    integer below 2^24, exact in any order."""
    g = torch.Generator().manual_seed(S * 3 + 1)
    dt = dtype_of(f16)
    offs = bias_offsets(S)
    H = len(offs)
    table = torch.zeros(H, 2 * S - 1)
    for h, d in enumerate(offs):
        table[h, d + S - 1] = BIAS_PEAK
    q = torch.zeros(1, H, S, 64, dtype=dt)
    k = torch.randn(1, H, S, 64, generator=g).to(dt)
    v = torch.randint(-8, 9, (1, H, S, 64), generator=g).to(dt)
    klen = S if key_len is None else min(key_len[0], S)
    tgt = torch.arange(S)[None, :] + torch.tensor(offs)[:, None]                  # [H,S]
    picked = (tgt >= 0) & (tgt < klen)
    mean = v[0, :, :klen].double().mean(dim=1, keepdim=True).expand(-1, S, -1)    # [H,S,64] fp64
    sel = torch.gather(v[0].double(), 1, tgt.clamp(0, S - 1)[..., None].expand(-1, -1, 64))
    exp = torch.where(picked[..., None], sel, mean).to(dt)                        # fp64 -> the tensor type, one rounding
    case = Case(q=q, k=k, v=v, table=table, key_len=key_len, scale=scale, offs=offs, picked=picked, tgt=tgt,
                expected=exp.permute(1, 0, 2).reshape(S, H * 64).contiguous(),
                picked_rows=picked.t().contiguous(), rows=torch.ones(1, S, dtype=torch.bool))
    return case


def ordered_bits(t):
    """16-bit float patterns as integers that ascend with the value: neighbours differ by 1 (+0 and -0 coincide)."""
    b = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7FFF))


def bias_copy_chunks(S):
    """csrc/attn.hip bias_copy_chunks: 16-byte chunks of one of the four shifted LDS copies of a head's [2S - 1] table."""
    need = (2 * S + 64 + 3 + 3) // 4
    return need + ((4 - (need & 15)) & 15)


def smallest_refused_bias_S():
    """The smallest S at which the biased hd-64 launch asks for more than 160 KiB of LDS: two 16 KiB stages + four table copies."""
    S = 1
    while 2 * 16384 + bias_copy_chunks(S) * 64 <= 160 * 1024:
        S += 1
    return S


# ---- both sides of the deferred rescale (RESCALE_THR = 6 log2 units): two 64-key tiles, one aligned key each
def rescale_case(hd, f16, gap_log2, B=1, H=2, seed=5):
    """Every query is close to one +-1 direction u; key 7 of tile 0 is 0.5 u, key 64 + 20 of tile 1 is a1 u with a1 the 8-bit value nearest to
    0.5 + gap / (hd * scale * log2 e): the second tile's row maximum sits about gap_log2 above the first tile's.  The other keys are small.
    Returns the case and the realised per-row gaps [B,H,S] in log2 units (fp32 reference)."""
    g = torch.Generator().manual_seed(seed + hd)
    dt = dtype_of(f16)
    S = 128
    scale = 0.125 if hd == 64 else HD128_SCALE
    u = (torch.randint(0, 2, (hd,), generator=g) * 2 - 1).float()
    q = (u + 0.1 * torch.randn(B, H, S, hd, generator=g)).to(dt)
    k = 0.1 * torch.randn(B, H, S, hd, generator=g)
    a1 = float(torch.tensor(0.5 + gap_log2 / (hd * scale * LOG2E)).to(torch.bfloat16))
    k[:, :, 7] = 0.5 * u
    k[:, :, 84] = a1 * u
    v = torch.randn(B, H, S, hd, generator=g).to(dt)
    case = Case(q=q, k=k.to(dt), v=v, scale=scale, rows=torch.ones(B, S, dtype=torch.bool))
    s = scores_fp32(case.q, case.k, scale) * LOG2E
    gaps = s[..., 64:].max(-1).values - s[..., :64].max(-1).values
    assert torch.equal(s[..., :64].argmax(-1), torch.full((B, H, S), 7)) and torch.equal(s[..., 64:].argmax(-1), torch.full((B, H, S), 20))
    return case, gaps


def masked_rows_case(hd, f16, causal, bias, poisoned, S=RAGGED_S, out_hd=0):
    """Gaussian inputs, one sample per ragged key length.  poisoned = False: zeros in K and V at positions >= key_len; True: finite values
    there that would win if they were visible (K rows = 16 x the sample's own query rows, V = 1000).  out_hd: lanes >= out_hd of q, k, v are
    zero and only out_hd lanes leave (the vision tower's heads)."""
    g = torch.Generator().manual_seed(11 + hd)
    dt = dtype_of(f16)
    kl = ragged_key_lens(S)
    B = len(kl)
    q = torch.randn(B, 1, S, hd, generator=g).to(dt)
    k = torch.randn(B, 1, S, hd, generator=g).to(dt)
    v = torch.randn(B, 1, S, hd, generator=g).to(dt)
    for b, klen in enumerate(kl):
        k[b, :, klen:] = 16 * q[b, :, klen:] if poisoned else 0
        v[b, :, klen:] = 1000.0 if poisoned else 0
    if out_hd:
        for t in (q, k, v):
            t[..., out_hd:] = 0
    case = Case(q=q, k=k, v=v, key_len=kl, causal=causal, out_hd=out_hd, scale=0.125 if hd == 64 else HD128_SCALE,
                rows=torch.arange(S)[None, :] < torch.tensor([min(x, S) for x in kl])[:, None])
    if bias:
        case.table = torch.randn(1, 2 * S - 1, generator=torch.Generator().manual_seed(3))
    return case
