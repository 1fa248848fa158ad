"""Float64 restatements and error criteria shared by tests/test_gpu_precise_decoder_kernels.py (one launch per kernel on the GPU) and
tests/test_precise_decoder_reference.py (the same helpers held to the oracles on the CPU, so that a bug here neither passes for a kernel
bug nor hides one).  Nothing in this file touches a GPU.  Every reference takes the stored inputs exactly: 16-bit tensors widened, fp32
tensors as they are, all arithmetic in float64.

Criteria (FP32_REL = 2e-5 is the project's fp32 bound, tests/test_gpu_qwen.py FP32_TAPS; `allow` is the measured allowance of a kernel
that uses the hardware exp / rcp, in units of the fp32 term, 0 for every other kernel):
  fp32 output:            |out - ref|     <= (1 + allow) 2e-5 max|ref_row|
  split-bf16 output:      |hi + lo - ref| <= (1 + allow) 2e-5 max|ref_row|   and   |lo| <= 0.5 ulp_bf16(hi)
  one 16-bit rounding:    |out - ref|     <= 0.5 ulp16(ref) + (1 + allow) 2e-5 max|ref_row|
Caps on an allowance (a lost lo plane costs 2^-9 of an element, a wrong 16-bit value at least one ulp; both must still fail):
  split: (1 + allow) 2e-5 < 2^-12;   16-bit: 0.5 ulp + (1 + allow) 2e-5 max < 1.5 ulp at the row maximum, i.e. (1 + allow) 2e-5 < 2^-bits."""
import math

import torch

FP32_REL = 2e-5
BF16_BITS, F16_BITS = 8, 11              # significant bits
BF16_NAN, F16_NAN, F32_NAN = 0x7FC0, 0x7E00, 0x7FC00000
NEG_BIG = -1.0e30


def ulp16(x, bits=BF16_BITS):
    """Spacing of the 16-bit format with `bits` significant bits at |x|, float64 (bf16: 8, IEEE fp16: 11); below the smallest normal
    number the spacing of the subnormals."""
    emin = -125 if bits == BF16_BITS else -13             # frexp exponent of the smallest normal number
    _, ex = torch.frexp(x.abs().double())                 # |x| = m 2^ex, m in [0.5, 1); frexp(0) = (0, 0)
    ex = torch.where(x == 0, torch.full_like(ex, emin), ex).clamp(min=emin)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), ex - bits)


def split_bf16(x):
    """(hi, lo) of a split-bf16 tensor holding x: hi = bf16(fp32(x)), lo = bf16(fp32(x) - hi), both float64."""
    x = x.float()
    hi = x.to(torch.bfloat16).float()
    return hi.double(), (x - hi).to(torch.bfloat16).double()


def allowance_caps_hold(allow, kind):
    """kind: 'split', 'bf16' or 'f16'."""
    limit = {"split": 2.0 ** -12, "bf16": 2.0 ** -BF16_BITS, "f16": 2.0 ** -F16_BITS}[kind]
    return (1.0 + allow) * FP32_REL < limit


def _rowmax(ref):
    return ref.abs().amax(dim=-1, keepdim=True).clamp(min=torch.finfo(torch.float32).tiny)


def ratio_f32(out, ref, allow=0.0):
    return ((out.double() - ref).abs() / ((1.0 + allow) * FP32_REL * _rowmax(ref))).max().item()


def ratio_split(hi, lo, ref, allow=0.0):
    """-> (worst |hi + lo - ref| / bound, worst |lo| / 0.5 ulp_bf16(hi))."""
    hi, lo = hi.double(), lo.double()
    r_sum = ((hi + lo - ref).abs() / ((1.0 + allow) * FP32_REL * _rowmax(ref))).max().item()
    r_lo = (lo.abs() / (0.5 * ulp16(hi))).max().item()
    return r_sum, r_lo


def ratio_16(out, ref, bits=BF16_BITS, allow=0.0):
    bound = 0.5 * ulp16(ref, bits) + (1.0 + allow) * FP32_REL * _rowmax(ref)
    return ((out.double() - ref).abs() / bound).max().item()


def excess(out, ref, bits=None):
    """What a kernel's error leaves after the output format's own rounding (0.5 ulp16(ref); nothing for fp32 / split outputs), in units of
    the fp32 term 2e-5 max|ref_row|: the figure an allowance is derived from (profiles/precise_decoder_kernels.md)."""
    err = (out.double() - ref).abs()
    if bits is not None:
        err = (err - 0.5 * ulp16(ref, bits)).clamp(min=0.0)
    return (err / (FP32_REL * _rowmax(ref))).max().item()


# ---- activations (the exact functions)
def gelu_new(x):
    """HF activations.py NewGELUActivation, 0.5 x (1 + tanh(u)), written as x sigmoid(2u) -- the same function, and in float64 the form that
    keeps its relative accuracy in the negative tail (1 + tanh(u) cancels to 0 below u = -19; sigmoid(2u) does not)."""
    x = x.double()
    return x * torch.sigmoid(2.0 * math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3))


def silu(x):
    x = x.double()
    return x * torch.sigmoid(x)


def gate_col(oc):
    """Packed column of output column oc's GATE operand: blocks of 64 packed columns = 32 gate | 32 linear / up columns; the linear
    operand is 32 columns further."""
    return (oc >> 5) * 64 + (oc & 31)


def pack_gate_up(gate, up):
    """[rows, F] gate and up -> [rows, 2F] in the packed order, by the definition (block j = gate[:, 32j : 32j+32] | up[:, 32j : 32j+32])."""
    rows, F = gate.shape
    assert F % 32 == 0
    return torch.stack([gate.reshape(rows, F // 32, 32), up.reshape(rows, F // 32, 32)], dim=2).reshape(rows, 2 * F)


# ---- the reductions.  `part` is the flat fp32 buffer as the kernel reads it (gaps included).
def _gather(part, base, rows, cols, ldp):
    idx = base + torch.arange(rows)[:, None] * ldp + torch.arange(cols)[None, :]
    return part[idx]


def sum_planes_y(part, nslices, slice_stride, rows, cols, ldp, bias=None, dtype=torch.float64):
    """y[r][c] = (sum_k hi rows) + (sum_k lo rows) (+ bias), slices in index order; dtype float64 (the reference) or float32 (the kernel's
    own order of additions, for the bitwise check of the slice order)."""
    a = _gather(part, 0, rows, cols, ldp).to(dtype)
    b = _gather(part, rows * ldp, rows, cols, ldp).to(dtype)
    for k in range(1, nslices):
        a = a + _gather(part, k * slice_stride, rows, cols, ldp).to(dtype)
        b = b + _gather(part, k * slice_stride + rows * ldp, rows, cols, ldp).to(dtype)
    y = a + b
    return y if bias is None else y + bias.to(dtype)[None, :cols]


def reduce_slices_y(part, nslices, slice_stride, rows, cols, ldp, bias=None, dtype=torch.float64):
    a = _gather(part, 0, rows, cols, ldp).to(dtype)
    for k in range(1, nslices):
        a = a + _gather(part, k * slice_stride, rows, cols, ldp).to(dtype)
    return a if bias is None else a + bias.to(dtype)[None, :cols]


def gated(y, act):
    """y [rows, 2F] in the packed order -> act(gate) * linear, [rows, F]."""
    F = y.shape[1] // 2
    gc = gate_col(torch.arange(F))
    return act(y[:, gc]) * y[:, gc + 32].double()


# ---- norms, softmax, attention, head
def rmsnorm(x, w, eps):
    x = x.double()
    return w.double() * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps)


def masked_softmax(scores, key_len, rows):
    """scores [B * rows, S_pad] -> probabilities over the first min(key_len[b], S_pad) keys, exact zeros after them (and everywhere for a
    sample with no key).  Scores past the length are never looked at (they may be NaN)."""
    R, S_pad = scores.shape
    out = torch.zeros(R, S_pad, dtype=torch.float64)
    for r in range(R):
        n = max(0, min(int(key_len[r // rows]), S_pad))
        if n:
            out[r, :n] = torch.softmax(scores[r, :n].double(), dim=-1)
    return out


def self_attention(q, k, v, bias_table=None, qpos0=0):
    """The T5 decoder's causal self-attention (no 1 / sqrt(d) scale), float64.  q [B, T, H, 64]: query rows at decoder positions qpos0 + t;
    k, v [B, S, H, 64] with S >= qpos0 + T: key j is used by query t when j <= qpos0 + t; bias_table [H, >= qpos0 + T] indexed by
    (query position - key position).  -> [B, T, H * 64]."""
    B, T, H, d = q.shape
    S = qpos0 + T
    s = torch.einsum("bthd,bjhd->bhtj", q.double(), k[:, :S].double())
    dist = (qpos0 + torch.arange(T))[:, None] - torch.arange(S)[None, :]          # [T, S]
    if bias_table is not None:
        s = s + bias_table.double()[:, dist.clamp(min=0)][None]
    s = s.masked_fill((dist < 0)[None, None], float("-inf"))
    return torch.einsum("bhtj,bjhd->bthd", torch.softmax(s, dim=-1), v[:, :S].double()).reshape(B, T, H * d)


def cross_attention(q, k, v, key_len):
    """q [B, T, H, 64], k / v [B, H, S, 64] head-major, the first key_len[b] keys only.  -> [B, T, H * 64]."""
    B, T, H, d = q.shape
    out = torch.empty(B, T, H, d, dtype=torch.float64)
    for b in range(B):
        n = int(key_len[b])
        s = torch.einsum("thd,hjd->htj", q[b].double(), k[b, :, :n].double())
        out[b] = torch.einsum("htj,hjd->thd", torch.softmax(s, dim=-1), v[b, :, :n].double())
    return out.reshape(B, T, H * d)


def label_logprobs(logits, labels, V):
    """logits [B, T, ldl] (the first V columns count) -> (log-probs [B, T]: 0 where the label is outside [0, V), scores [B] =
    exp(sum over labels != -100 / max(count, 1)))."""
    lp = torch.log_softmax(logits[..., :V].double(), dim=-1)
    ok = (labels >= 0) & (labels < V)
    lp = torch.where(ok, lp.gather(-1, labels.clamp(0, V - 1).long()[..., None])[..., 0], torch.zeros_like(lp[..., 0]))
    cnt = (labels != -100).sum(-1).clamp(min=1)
    return lp, torch.exp((lp * (labels != -100)).sum(-1) / cnt)


def dec_attn_lds_bytes(T, S):
    """A copy of the LDS arithmetic of attn.hip launch_decoder_attention (q rows, T x S scores, 4 waves' partial outputs, the reduction
    scratch and the row sums, fp32); the launcher is the authority: the GPU test holds the copy to it by running the largest S this
    gives and being refused the next."""
    return ((T * 64 + T * S + 4 * T * 64 + 4 + T) * 4 + 15) & ~15
