"""Inputs and expectations of the single-launch GEMM epilogue tests (tests/test_gpu_gemm_epilogues.py runs them on the kernels through
vqs_debug_gemm_launch, tests/test_gemm_epilogue_inputs.py proves on the CPU that the expectations are exact, that every case runs the kernel
family it claims, and that the cases can fail).  Everything here is plain torch on the CPU.

Exact cases (everything that is indexing: the head-major scatter with 128-lane heads, narrow heads in wide slots, grouped-query k / v tensors,
the scaled fp16 families, the rotary embedding inside the epilogue).  A and W hold integers in [-2, 2], the bias integers in [-4, 4], acc_scale
and out_scale are powers of two, cos / sin come from {0, +-1/4, ..., +-1} and K <= 512: every accumulator (|acc| <= 4 K <= 2048), the fmaf with
the bias, the rotation (multiples of 1/4 below 2^14) and the scaling are exact in fp32 in ANY summation order, so the one rounding to bf16 /
fp16 is round-to-nearest of an exact value and the expected tensor is a torch expression compared bit for bit.  Scaled results are 0 or at
least 2^-7 in magnitude and at most 8200: no fp16 subnormal, nothing near the fp16 maximum.

The expected tensors are views of the dense product R = A @ W.T: columns [0, inner) are q heads of hd_src columns each, [inner, inner + ikv)
are k, the rest v; tensor t is [B, H_t, S, hd] and out[b, h, s, :hd_src] = R[b S + s, base_t + h hd_src : base_t + (h + 1) hd_src].  No offset
arithmetic of the kernels (heads_off_first) is restated there; scatter_restated below does restate it, once, as the thing the planted
mistakes are planted in.

Canaries: every output lives inside a larger buffer pre-filled with SENTINEL (a NaN pattern in bf16 and in fp16: no result is a NaN), and the
expected buffer holds the sentinel wherever the launch must not write: rows >= M, lanes [hd_src, hd) of every slot, the guard regions in
front of and behind each tensor, columns >= N (gated: >= N / 2) of an ldc wider than the result.

Arithmetic cases (random operands: the SiLU gate, the gated bias in packed column order, the scaled plain / GELU epilogues): reference = fp64
accumulate, the epilogue in fp64 on acc * acc_scale + bias, one rounding to the output type; criterion = the project's per-launch one
(tests/test_gpu_qwen.py _stage_locked_impl): no element more than one ulp of its own binade away, at most 0.5 % of a bf16 tensor's elements
and 2 % of an fp16 tensor's different at all."""
import functools
import math

import torch

SENTINEL = 0x7FC1                 # 16-bit pattern of every byte a launch must not write: a quiet NaN in bf16 and in fp16
FRONT_GUARD = 4096                # elements in front of every output
EPI_BF16, EPI_GELU, EPI_GATED, EPI_HEADS = 0, 2, 5, 6
T_BF16, T_F16, T_F16_BF16, T_F16S, T_F16S_BF16 = range(5)
TILE, TILE_PP, PERSISTENT, PINGPONG, STREAM, QUAD, SLIM = range(7)          # vqs_kernels.h GemmKernel
BIAS, ROWSS, NO_STREAM, ROPE_COS, ROPE_SIN = 1, 2, 4, 8, 16
PLAN_FIELDS = ("M", "N", "K", "lda", "ldw", "ldc", "epi", "batch", "variant", "S", "inner", "inner_kv", "hd", "hd_src", "Hkv", "type", "l2_touch",
               "split_off", "flags", "gate_act", "rowss_parts", "ldh")
MAX_OWN_ULPS = 1.001              # _stage_locked_impl's conditions
MAX_FRAC_DIFF = {7: 5e-3, 10: 2e-2}


def in_dtype(typ):
    return torch.bfloat16 if typ == T_BF16 else torch.float16


def out_dtype(typ):
    return torch.float16 if typ in (T_F16, T_F16S) else torch.bfloat16


class Geometry:
    def __init__(self, name, H, Hkv, hd, hd_src, inner, ikv, N, S, why):
        self.name, self.H, self.Hkv, self.hd, self.hd_src, self.inner, self.ikv, self.N, self.S, self.why = name, H, Hkv, hd, hd_src, inner, ikv, N, S, why
        self.hsrc = hd_src or hd
        assert inner == H * self.hsrc and ikv == self.heads(1) * self.hsrc and N == inner + 2 * ikv

    def heads(self, t):
        return self.H if t == 0 else (self.Hkv or self.H)

    @property
    def quad(self):               # gemm.hip quad_eligible_rt: a wave's 128 columns lie inside one of the q / k / v tensors
        return self.inner % 128 == 0 and self.ikv % 128 == 0

    @property
    def whole_heads(self):        # the rotary embedding needs whole 128-lane heads
        return self.hd == 128 and self.hsrc == 128


GEOMETRIES = {g.name: g for g in (
    Geometry("gqa31", 3, 1, 128, 0, 384, 128, 640, (8, 9, 15, 16, 17, 40),
             "q/k boundary inside tile 1; v in a ragged last tile; both the S < 16 and the S >= 16 stepping"),
    Geometry("gqa42", 4, 2, 128, 0, 512, 256, 1024, (8, 15, 24, 100), "Hkv > 1: the k / v wrap is non-zero and differs from q's"),
    Geometry("tower80", 8, 0, 128, 80, 640, 640, 1920, (9, 16, 40), "a lane's four 8-column chunks in different heads; pad lanes untouched"),
    Geometry("half64", 4, 0, 128, 64, 256, 256, 768, (16, 40), "the other hd_src the kernel comment names"),
    Geometry("lm71", 7, 1, 64, 0, 448, 64, 576, (8, 33), "inner % 128 != 0: the 8-wave family's generalised staged epilogue with inner_kv / Hkv"),
)}


def batches(S):
    """B such that M = B S lands below 128, between 128 and 256, on 256 (where S divides it), on the first multiple of S past 256 (256 + 8 for
    S = 8, 24, 33: the first rows of a second M-tile) and past 512."""
    bs = {max(1, 100 // S), -(-130 // S), 256 // S + 1, 512 // S + 1}
    if 256 % S == 0:
        bs.add(256 // S)
    return sorted(bs)


class Config:
    """One way of launching a geometry: operand type, variant, bias, scales, rope, K."""

    def __init__(self, name, typ, variant, bias, acc_scale=1.0, out_scale=1.0, rope=False, K=128):
        self.name, self.type, self.variant, self.bias, self.acc_scale, self.out_scale, self.rope, self.K = name, typ, variant, bias, acc_scale, out_scale, rope, K

    def but(self, **kw):
        c = Config(self.name, self.type, self.variant, self.bias, self.acc_scale, self.out_scale, self.rope, self.K)
        c.__dict__.update(kw)
        return c


CONFIGS = {c.name: c for c in (
    Config("bf16-v10", T_BF16, 10, False),
    Config("bf16-v10-bias", T_BF16, 10, True),
    Config("bf16-v11-bias", T_BF16, 11, True),
    Config("f16-v10-bias", T_F16, 10, True),
    Config("f16s-v10-unit", T_F16S, 10, False),                          # both scales 1: also bitwise the type-1 launch
    Config("f16s-v10-bias-a8-o32", T_F16S, 10, True, 8.0, 2.0 ** -5),
    Config("f16s-v10-a8", T_F16S, 10, False, 8.0, 1.0),
    Config("f16s-v10-bias-o32", T_F16S, 10, True, 1.0, 2.0 ** -5),
    Config("f16s-v10-rope-unit", T_F16S, 10, False, rope=True),
    Config("f16s-v10-rope-bias-a8-o32", T_F16S, 10, True, 8.0, 2.0 ** -5, rope=True),
    Config("bf16-v3-k256-bias", T_BF16, 3, True, K=256),                 # few rows under the library's rule: the slim kernel
    Config("f16-v3-k256", T_F16, 3, False, K=256),
    Config("f16s-v3-k256-rope-bias", T_F16S, 3, True, 8.0, 2.0 ** -5, rope=True, K=256),   # slim refuses rope (and type 3): the quad kernel
)}


def claimed_kernel(g, c):
    """The kernel family the case claims to run, None where it claims a refusal of the launcher."""
    if c.rope and not g.whole_heads:
        return None
    if not g.quad:                # the 8-wave family: bf16 only; its few-row stream form has plain epilogues only
        return PERSISTENT if c.type == T_BF16 else None
    if c.variant == 11:           # narrow heads in wide slots are quad-only
        return PERSISTENT if g.hsrc == g.hd and c.type == T_BF16 else None
    return SLIM if c.variant == 3 and c.type in (T_BF16, T_F16) and not c.rope else QUAD


def configs_of(g):
    """The configurations a geometry is crossed with (refusals included: they are asserted, not skipped)."""
    names = ["bf16-v10", "bf16-v10-bias", "bf16-v11-bias", "f16-v10-bias", "f16s-v10-unit", "f16s-v10-bias-a8-o32", "f16s-v10-a8", "f16s-v10-bias-o32"]
    if g.name in ("gqa31", "gqa42"):
        names += ["f16s-v10-rope-unit", "f16s-v10-rope-bias-a8-o32", "f16s-v3-k256-rope-bias"]
    if g.name == "tower80":
        names += ["f16s-v10-rope-unit"]                                  # rope with hd_src = 80: refused
    if g.quad:
        names += ["bf16-v3-k256-bias", "f16-v3-k256"]
    return [CONFIGS[n] for n in names]


EXACT_CASES = [(g.name, S, c.name) for g in GEOMETRIES.values() for c in configs_of(g) for S in g.S]


def launch_fields(g, c, B, S):
    """The launch as vqs_debug_gemm_launch's integers (a dict by name; H included)."""
    d = dict.fromkeys(PLAN_FIELDS + ("H",), 0)
    d.update(M=B * S, N=g.N, K=c.K, lda=c.K, ldw=c.K, ldc=0, epi=EPI_HEADS, batch=1, variant=c.variant, S=S, inner=g.inner, inner_kv=g.ikv if g.Hkv else 0, hd=g.hd,
             hd_src=g.hd_src, Hkv=g.Hkv, type=c.type, flags=(BIAS if c.bias else 0) | (ROPE_COS | ROPE_SIN if c.rope else 0), H=g.H)
    return d


def plan_list(fields):
    return [fields[f] for f in PLAN_FIELDS]


ROPE_VALUES = torch.tensor([0.0, 0.25, 0.5, 0.75, 1.0, -0.25, -0.5, -0.75, -1.0])


class Inputs:
    pass


@functools.lru_cache(maxsize=64)
def exact_inputs(name, S, B, K):
    """Integer operands (as float64; exact in bf16 and fp16), the rope tables and the dense product R, computed once per shape."""
    g = GEOMETRIES[name]
    gen = torch.Generator().manual_seed(1000003 * sorted(GEOMETRIES).index(name) + 10007 * S + 101 * B + K)
    x = Inputs()
    x.g, x.S, x.B, x.M, x.K = g, S, B, B * S, K
    x.A = torch.randint(-2, 3, (x.M, K), generator=gen).double()
    x.W = torch.randint(-2, 3, (g.N, K), generator=gen).double()
    x.bias = torch.randint(-4, 5, (g.N,), generator=gen).double()
    x.cos = ROPE_VALUES[torch.randint(0, 9, (x.M, 64), generator=gen)]       # fp32 [M, 64]: a different row for every GEMM row
    x.sin = ROPE_VALUES[torch.randint(0, 9, (x.M, 64), generator=gen)]
    x.R = x.A @ x.W.T
    return x


def tensor_elems(g, t, B, S):
    return B * g.heads(t) * S * g.hd


def back_guard(g, B, S):
    """Elements behind a tensor: the tile's row overhang (rows up to M + 255 would land in samples >= B) for the LARGEST head count, and the
    whole tensor once more -- a scatter with the wrong head count or a late wrap still lands inside the allocation."""
    return (B + 256 // S + 2) * g.H * S * g.hd


def sentinel_buffer(n, device="cpu"):
    return torch.full((n,), SENTINEL, dtype=torch.int16, device=device)


def expected_heads(x, c, acc=torch.float64):
    """The three expected tensors [B, H_t, S, hd] as int16 bit patterns (pad lanes = SENTINEL), from views of R; `acc` = the type the
    epilogue is evaluated in (the CPU test runs fp32 against fp64)."""
    g, B, S = x.g, x.B, x.S
    R = x.R if acc == torch.float64 else x.A.to(acc) @ x.W.to(acc).T
    E = R * c.acc_scale
    if c.bias:
        E = E + x.bias.to(acc)
    outs = []
    for t, part in enumerate(E.split([g.inner, g.ikv, g.ikv], dim=1)):
        v = part.view(B, S, g.heads(t), g.hsrc).permute(0, 2, 1, 3)                      # [B, H_t, S, hd_src]
        if c.rope and t < 2:
            cs, sn = x.cos.to(acc).view(B, 1, S, 64), x.sin.to(acc).view(B, 1, S, 64)    # table row b S + s
            lo, hi = v[..., :64], v[..., 64:]
            v = torch.cat([lo * cs - hi * sn, hi * cs + lo * sn], dim=-1)
        v = (v * c.out_scale).to(out_dtype(c.type))
        o = torch.full((B, g.heads(t), S, g.hd), SENTINEL, dtype=torch.int16)
        o[..., :g.hsrc] = v.contiguous().view(torch.int16)
        outs.append(o)
    return outs


def expected_values(x, c, acc=torch.float64):
    """The scaled results before the rounding, every tensor flattened and concatenated (range checks of the CPU test)."""
    g, B, S = x.g, x.B, x.S
    R = x.R if acc == torch.float64 else x.A.to(acc) @ x.W.to(acc).T
    E = R * c.acc_scale + (x.bias.to(acc) if c.bias else 0)
    vals = []
    for t, part in enumerate(E.split([g.inner, g.ikv, g.ikv], dim=1)):
        v = part.view(B, S, g.heads(t), g.hsrc).permute(0, 2, 1, 3)
        if c.rope and t < 2:
            cs, sn = x.cos.to(acc).view(B, 1, S, 64), x.sin.to(acc).view(B, 1, S, 64)
            v = torch.cat([v[..., :64] * cs - v[..., 64:] * sn, v[..., 64:] * cs + v[..., :64] * sn], dim=-1)
        vals.append((v * c.out_scale).reshape(-1))
    return torch.cat(vals)


def expected_buffers(x, c):
    """The whole device buffers a launch must leave: guard | tensor | guard, int16."""
    bufs = []
    for t, o in enumerate(expected_heads(x, c)):
        b = sentinel_buffer(FRONT_GUARD + o.numel() + back_guard(x.g, x.B, x.S))
        b[FRONT_GUARD:FRONT_GUARD + o.numel()] = o.reshape(-1)
        bufs.append(b)
    return bufs


# ---------------------------------------------------------------------------------------------------- the scatter, restated with its offset arithmetic
SCATTER_MISTAKES = ("kv_bases_swapped", "h_for_kv_wrap", "head_by_hd", "late_sample_wrap")
ROPE_MISTAKES = ("rope_partner_32", "rope_on_v", "rope_row_by_position")
SCALE_MISTAKES = ("bias_after_scale",)


def scatter_restated(x, c, mistake=None):
    """What the head-major epilogue does, element by element with the kernels' arithmetic (destination = tensor of the column range + head base +
    row offset with the sample wrap), into three flat buffers of tensor_elems + back_guard elements.  mistake: one planted error."""
    g, B, S, M = x.g, x.B, x.S, x.M
    rows, cols = torch.arange(M)[:, None], torch.arange(g.N)[None, :]
    which = (cols >= g.inner).long() + (cols >= g.inner + g.ikv).long()
    base = torch.tensor([0, g.inner, g.inner + g.ikv])[which]
    div = g.hd if mistake == "head_by_hd" else g.hsrc
    head = (cols - base) // div
    lane = (cols - base) - head * div
    hx = torch.where(which == 0, g.H, g.H if mistake == "h_for_kv_wrap" else g.heads(1))
    hb = rows // S
    hb_wrap = (rows - 16).clamp(min=0) // S if mistake == "late_sample_wrap" else hb
    dest = rows * g.hd + hb_wrap * (hx - 1) * S * g.hd + head * S * g.hd + lane          # (hb hx S + hs) hd = row hd + hb (hx - 1) S hd
    target = which.expand(M, g.N)
    if mistake == "kv_bases_swapped":
        target = torch.where(target == 1, 2, torch.where(target == 2, 1, target))
    if mistake == "bias_after_scale":
        E, post = x.R * c.acc_scale * c.out_scale + (x.bias if c.bias else 0), 1.0
    else:
        E, post = x.R * c.acc_scale + (x.bias if c.bias else 0), c.out_scale
    if c.rope:
        po = 32 if mistake == "rope_partner_32" else 64
        low = lane < 64
        partner = base + head * 128 + torch.where(low, (lane + po) % 128, (lane - po) % 128)
        tr = (rows - hb * S if mistake == "rope_row_by_position" else rows).expand(M, g.N)
        tc = (lane % 64).expand(M, g.N)
        cs, sn = x.cos.double()[tr, tc], x.sin.double()[tr, tc]
        Ep = E.gather(1, partner.expand(M, g.N))
        rot = torch.where(low, E * cs - Ep * sn, E * cs + Ep * sn)
        E = torch.where((which < (3 if mistake == "rope_on_v" else 2)).expand(M, g.N), rot, E)
    bits = (E * post).to(out_dtype(c.type)).view(torch.int16)
    outs = []
    for t in range(3):
        b = sentinel_buffer(tensor_elems(g, t, B, S) + back_guard(g, B, S))
        m = target == t
        b[dest.expand(M, g.N)[m]] = bits[m]
        outs.append(b)
    return outs


def expected_flat(x, c):
    """expected_heads in scatter_restated's buffers."""
    outs = []
    for t, o in enumerate(expected_heads(x, c)):
        b = sentinel_buffer(o.numel() + back_guard(x.g, x.B, x.S))
        b[:o.numel()] = o.reshape(-1)
        outs.append(b)
    return outs


# ---------------------------------------------------------------------------------------------------- arithmetic cases
class ArithCase:
    def __init__(self, epi, typ, variant, M, bias, gate_act=0, acc_scale=1.0, out_scale=1.0):
        self.epi, self.type, self.variant, self.M, self.bias, self.gate_act, self.acc_scale, self.out_scale = epi, typ, variant, M, bias, gate_act, acc_scale, out_scale
        self.N, self.K = 640, 192                 # gated: F = 320 output columns, ragged in a 256-column tile, N % 64 == 0
        self.n_out = self.N // 2 if epi == EPI_GATED else self.N
        self.ldc = self.n_out + 64                # wider than the result: columns >= n_out must stay untouched
        self.name = (f"{ {EPI_BF16: 'plain', EPI_GELU: 'gelu', EPI_GATED: 'gated'}[epi]}{'-silu' if gate_act else ''}-t{typ}-v{variant}-m{M}{'-bias' if bias else ''}"
                     f"{'' if acc_scale == 1.0 else f'-a{acc_scale:g}'}{'' if out_scale == 1.0 else f'-o{out_scale:g}'}")

    @property
    def mant_bits(self):
        return 10 if out_dtype(self.type) == torch.float16 else 7

    def fields(self):
        d = dict.fromkeys(PLAN_FIELDS + ("H",), 0)
        d.update(M=self.M, N=self.N, K=self.K, lda=self.K, ldw=self.K, ldc=self.ldc, epi=self.epi, batch=1, variant=self.variant, S=1, inner=1, type=self.type,
                 flags=BIAS if self.bias else 0, gate_act=self.gate_act)
        return d

    @property
    def kernel(self):
        return QUAD if self.variant == 10 else PERSISTENT


ARITH_CASES = [
    *[ArithCase(EPI_GATED, t, 10, M, b, gate_act=1) for t in (T_BF16, T_F16_BF16, T_F16S) for b in (False, True) for M in (130, 300)],
    *[ArithCase(EPI_GATED, T_F16S, 10, M, True, gate_act=1, out_scale=0.25) for M in (130, 300)],
    *[ArithCase(EPI_GATED, T_BF16, 11, M, b, gate_act=1) for b in (False, True) for M in (130, 300)],       # the 8-wave staged epilogue's SiLU / packed bias
    *[ArithCase(EPI_GATED, T_BF16, v, M, True, gate_act=0) for v in (10, 11) for M in (130, 300)],          # gelu_new with a bias
    *[ArithCase(e, T_F16S, 10, M, True, acc_scale=4.0, out_scale=0.125) for e in (EPI_BF16, EPI_GELU) for M in (130, 300)],
    *[ArithCase(EPI_BF16, T_F16S_BF16, 10, M, True, acc_scale=4.0, out_scale=0.125) for M in (130, 300)],
]


def deinterleave_gate(t):
    """Inverse of tests.gpu_util.interleave_gate along the last axis: packed columns in blocks of 64 = 32 gate | 32 linear -> (gate, linear)."""
    p = t.reshape(*t.shape[:-1], t.shape[-1] // 64, 2, 32)
    return p[..., 0, :].reshape(*t.shape[:-1], -1), p[..., 1, :].reshape(*t.shape[:-1], -1)


@functools.lru_cache(maxsize=None)
def arith_inputs(M, N, K, typ):
    """randn A, randn K^-0.5 W in the operand type; for a gated launch W and the bias are in packed (interleaved) order as they stand."""
    gen = torch.Generator().manual_seed(7919 * M + 31 * N + K + typ)
    x = Inputs()
    x.A = torch.randn(M, K, generator=gen).to(in_dtype(typ))
    x.W = (torch.randn(N, K, generator=gen) * K ** -0.5).to(in_dtype(typ))
    x.bias = torch.randn(N, generator=gen).to(torch.bfloat16)
    return x


def gelu_new(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def arith_reference(case, acc=torch.float64, mistake=None):
    """[M, n_out] in the output type: accumulate and epilogue in `acc`, one rounding.  mistake 'gate_linear_swapped': the planted error."""
    x = arith_inputs(case.M, case.N, case.K, case.type)
    t = (x.A.to(acc) @ x.W.to(acc).T) * case.acc_scale
    if case.bias:
        t = t + x.bias.to(acc)
    if case.epi == EPI_GATED:
        gate, lin = deinterleave_gate(t)
        if mistake == "gate_linear_swapped":
            gate, lin = lin, gate
        r = (gate * torch.sigmoid(gate) if case.gate_act == 1 else gelu_new(gate)) * lin
    elif case.epi == EPI_GELU:
        r = 0.5 * t * (1.0 + torch.erf(t / math.sqrt(2.0)))
    else:
        r = t
    return (r * case.out_scale).to(out_dtype(case.type))


def criterion(ref16, out16, mant_bits):
    """The per-launch criterion of tests/test_gpu_qwen.py _stage_locked_impl -> (ok, report)."""
    from oracle.clip_t5_engine_rounding import compare_tap
    r = compare_tap(ref16.float(), out16.float(), mant_bits=mant_bits)
    return r["max_own_ulps"] <= MAX_OWN_ULPS and r["frac_diff"] <= MAX_FRAC_DIFF[mant_bits], r


# ---------------------------------------------------------------------------------------------------- operands of a launch; refusals
def heads_launch_args(x, c, fields=None, drop=(), device="cuda"):
    """-> (the launch's integers, its tensors by vqs_debug_gemm_launch's names, the three whole sentinel-filled output buffers).  fields: overrides
    of the integers, drop: operand names withheld (their flags stay) -- both only for launches that must be refused.  An unmodified launch is
    checked here against what the kernels may read and write."""
    g = x.g
    f = launch_fields(g, c, x.B, x.S)
    dt = in_dtype(c.type)
    t = dict(A=x.A.to(dt).to(device), W=x.W.to(dt).to(device))
    if c.bias:
        t["bias"] = x.bias.to(torch.bfloat16).to(device)
    if c.rope:
        t["rope_cos"], t["rope_sin"] = x.cos.to(device), x.sin.to(device)
        assert t["rope_cos"].shape == t["rope_sin"].shape == (f["M"], 64) and t["rope_cos"].dtype == torch.float32
    assert t["A"].shape == (f["M"], f["K"]) and t["W"].shape == (f["N"], f["K"]) and f["lda"] == f["ldw"] == f["K"] and x.bias.shape == (f["N"],)
    assert f["M"] == x.B * f["S"] and f["H"] == g.H and f["hd"] == g.hd and f["S"] >= 8
    bufs = [sentinel_buffer(FRONT_GUARD + tensor_elems(g, i, x.B, x.S) + back_guard(g, x.B, x.S), device) for i in range(3)]
    for n, b in zip(("heads_q", "heads_k", "heads_v"), bufs):
        t[n] = b[FRONT_GUARD:]
    f.update(fields or {})
    for n in drop:
        del t[n]
    return f, t, bufs


def plain_launch_args(case, fields=None, bias=None, device="cuda"):
    """-> (integers, tensors, the whole sentinel-filled output buffer) of an arithmetic case; fields / bias: overrides for refusals."""
    x = arith_inputs(case.M, case.N, case.K, case.type)
    f = case.fields()
    t = dict(A=x.A.to(device), W=x.W.to(device))
    assert t["A"].shape == (f["M"], f["K"]) and t["W"].shape == (f["N"], f["K"]) and f["ldc"] >= case.n_out and x.bias.shape == (f["N"],)
    if case.bias if bias is None else bias:
        t["bias"] = x.bias.to(device)
    buf = sentinel_buffer(FRONT_GUARD + (case.M + 264) * case.ldc, device)            # a tile's row overhang fits behind the result
    t["C"] = buf[FRONT_GUARD:]
    f.update(fields or {})
    return f, t, buf


# (what, geometry, S, B, configuration, overrides of the integers, operands withheld): each is refused by the hook or by the launcher, with
# VQS_ERR_INVALID, before anything reaches the device
HEADS_REFUSALS = [
    ("a missing rope table (flag without its pointer)", "gqa31", 8, 17, "f16s-v10-rope-unit", None, ("rope_sin",)),
    ("one rope table only", "gqa31", 8, 17, "f16s-v10-rope-unit", dict(flags=ROPE_COS), ("rope_sin",)),
    ("a rope table without its flag", "gqa31", 8, 17, "f16s-v10-rope-unit", dict(flags=ROPE_COS), ()),
    ("rope with hd_src = 80", "tower80", 9, 15, "f16s-v10-rope-unit", None, ()),
    ("rope on the unscaled fp16 family", "gqa31", 8, 17, "f16s-v10-rope-unit", dict(type=T_F16), ()),
    ("hd = 128 under variant 0", "gqa31", 8, 17, "bf16-v10-bias", dict(variant=0), ()),
    ("hd = 128 under variant 2", "gqa31", 8, 17, "bf16-v10-bias", dict(variant=2), ()),
    ("S = 7 with hd = 128", "gqa31", 8, 17, "bf16-v10-bias", dict(S=7), ()),
    ("a bias without its flag", "gqa31", 8, 17, "bf16-v10-bias", dict(flags=0), ()),
    ("a bias flag without the vector", "gqa31", 8, 17, "bf16-v10", dict(flags=BIAS), ()),
    ("no q heads", "gqa31", 8, 17, "bf16-v10-bias", dict(H=0), ()),
    ("a batch", "gqa31", 8, 17, "bf16-v10-bias", dict(batch=2), ()),
    ("a split result", "gqa31", 8, 17, "bf16-v10-bias", dict(split_off=4096), ()),
    ("a handle's launch", "gqa31", 8, 17, "bf16-v10-bias", dict(flags=BIAS | 64), ()),
    ("no q tensor", "gqa31", 8, 17, "bf16-v10-bias", None, ("heads_q",)),
    ("no A", "gqa31", 8, 17, "bf16-v10-bias", None, ("A",)),
    ("narrow heads in wide slots under variant 11", "tower80", 9, 15, "bf16-v11-bias", None, ()),
]
# (what, overrides, bias override) on refusal_base_case()
PLAIN_REFUSALS = [
    ("a gated bias under variant 0", dict(variant=0), None),
    ("a SiLU gate under variant 0", dict(variant=0, gate_act=1, flags=0), False),
    ("the fused residual + RMSNorm", dict(epi=7), None),
    ("fp32 + residual", dict(epi=4), None),
    ("a gated fp16 result", dict(type=T_F16), None),
    ("a lab variant", dict(variant=7), None),
    ("no C", dict(epi=EPI_HEADS), None),
]


def refusal_base_case():
    """The accepted launch PLAIN_REFUSALS are one change away from: gelu_new gate with a bias, bf16, the quad kernel."""
    return next(c for c in ARITH_CASES if c.epi == EPI_GATED and c.type == T_BF16 and c.variant == 10 and c.bias and c.gate_act == 0 and c.M == 130)
