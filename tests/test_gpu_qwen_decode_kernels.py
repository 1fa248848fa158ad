"""The Qwen2.5-VL decode-step kernels on their own (include/vqs_debug.h test hooks; csrc/qwen_decode.hip): qwen_decode_attn_gqa_kernel,
qwen_decode_attn_kernel and qwen_decode_rope_append_kernel, one launch each on caller tensors against a float64 restatement of the operation
computed from the exact values of the 16-bit inputs.  Every case is the smallest shape at which a branch, a loop boundary or a launch form
of the kernels is reached: the grouped kernel's 256-key iteration and its 4-key lanes, the per-head kernel's 256-key / 4-key loops, caches
whose length is no multiple of 4, both opt-in dynamic-LDS launches up to the launcher's limit, the length clamps, and the append kernel's
early-out.  Cache rows past a sample's keys hold NaN bit patterns, so a read past the count cannot hide; needle cases make ONE key carry the
whole softmax, so a dropped or misplaced key cannot hide among thousands either.

Criteria per output row (one sample, one head), none of them taken from the kernels' own results:
  mode 0 (decode step, bf16 out):   |out - ref| <= 0.5 ulp_bf16(ref) + 2e-5 max|ref_row|   (one final rounding + the fp32 bound of FP32_TAPS, test_gpu_qwen.py)
  modes 1, 2 (precise tail, split): |hi + lo - ref| <= 2e-5 max|ref_row|  and  |lo| <= 0.5 ulp_bf16(hi)
  rope + append, rotated lanes:     |out - ref| <= 0.5 ulp_bf16(ref) + 2^-22 (|a| + |c|)   (two fp32 products and one sum of the source lanes a, c)
Each case's worst error-to-bound ratio goes to the suite's parity_e2e.jsonl record (tests/test_gpu_e2e.py)."""
import functools
import math

import numpy as np
import pytest
import torch

from tests.test_gpu_e2e import _record

pytestmark = pytest.mark.gpu

INVALID = -1
HD = 128
FP32_REL = 2e-5
BF16_NAN, F16_NAN = 0x7FC0, 0x7E00
SENTINEL = 0x5A5A
GROUPED, PER_HEAD = 1, 0


def _lib():
    from t2v_metrics_amd import engine
    return engine.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _form(lib, Hq, Hkv, Lmax):
    import ctypes
    lds = ctypes.c_int64(-1)
    return lib.vqs_debug_qwen_decode_attention_form(Hq, Hkv, Lmax, ctypes.byref(lds)), lds.value


def _ulp_bf16(x):
    """Spacing of bf16 (8 significant bits) at |x|, float64; the smallest normal binade below it."""
    _, ex = torch.frexp(x.abs().double())                   # |x| = m 2^ex, m in [0.5, 1); frexp(0) = (0, 0)
    ex = torch.where(x == 0, torch.full_like(ex, -125), ex).clamp(min=-125)
    return torch.ldexp(torch.ones_like(x, dtype=torch.float64), ex - 8)


def _f32(v):
    return float(np.float32(v))


SCALE = _f32(1.0 / math.sqrt(HD))
# mode 2 (IEEE fp16 K / V behind power-of-two scales): stored = fp16(true * scale); the key scale is folded into `scale`, the output times 1 / vs
KSCALE, VSCALE = 4.0, 8.0


def _nan_fill(t16, ns, f16):
    """Rows at positions >= ns[b] of every sample's [Hkv, Lmax, 128] slab <- NaN bit patterns (in place, int16 view)."""
    bits = t16.view(torch.int16)
    for b, n in enumerate(ns):
        bits[b, :, n:] = F16_NAN if f16 else BF16_NAN
    return t16


def _reference(q, K, V, ns, scale, vscale=1.0):
    """softmax(q K^T scale) V vscale over the first ns[b] keys of the head's key/value head, float64.  q [B, Hq, 128]; K, V [B, Hkv, Lmax, 128]."""
    B, Hq, _ = q.shape
    G = Hq // K.shape[1]
    out = torch.empty(B, Hq, HD, dtype=torch.float64)
    for b, n in enumerate(ns):
        k = K[b, :, :n].double().repeat_interleave(G, dim=0)            # [Hq, n, 128]
        v = V[b, :, :n].double().repeat_interleave(G, dim=0)
        s = torch.einsum("hd,hnd->hn", q[b].double(), k) * scale
        out[b] = torch.einsum("hn,hnd->hd", torch.softmax(s, dim=-1), v) * vscale
    return out


def _launch(lib, mode, q, K, V, lens, Lmax, scale, vscale=1.0):
    """One launch of the hook; q [B, Hq, 128] (bf16 for mode 0, fp32 otherwise), K / V [B, Hkv, Lmax, 128] 16-bit.  -> float64 CPU planes
    (out,) or (hi, lo), each [B, Hq, 128].  The output starts as NaN patterns: an unwritten element is not finite."""
    B, Hq, _ = q.shape
    Hkv = K.shape[1]
    planes = 1 if mode == 0 else 2
    out = torch.full((planes, B, Hq, HD), BF16_NAN, dtype=torch.int16).view(torch.bfloat16).cuda()
    qd, kd, vd = q.contiguous().cuda(), K.contiguous().cuda(), V.contiguous().cuda()
    ld = torch.tensor(list(lens), dtype=torch.int32).cuda()
    rc = lib.vqs_debug_qwen_decode_attention(qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), ld.data_ptr(), out.data_ptr(), B * Hq * HD, B, Hq, Hkv, Lmax,
                                             scale, vscale, mode, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = out.cpu()
    assert torch.isfinite(res.float()).all(), "non-finite output (a NaN cache row past the count was read, or an element was not written)"
    return tuple(res[i].double() for i in range(planes))


def _ratios(mode, planes, ref):
    """Worst error-to-bound ratio per criterion over all rows: mode 0 -> (r,), modes 1, 2 -> (r_sum, r_lo)."""
    rowmax = ref.abs().amax(dim=-1, keepdim=True)
    if mode == 0:
        bound = 0.5 * _ulp_bf16(ref) + FP32_REL * rowmax
        return ((planes[0] - ref).abs() / bound).max().item(),
    hi, lo = planes
    r_sum = ((hi + lo - ref).abs() / (FP32_REL * rowmax)).max().item()
    r_lo = (lo.abs() / (0.5 * _ulp_bf16(hi))).max().item()
    return r_sum, r_lo


def _check(case, mode, planes, ref):
    r = _ratios(mode, planes, ref)
    _record("qwen_decode_kernels/" + case, {"mode": mode, "worst_error_to_bound": r[0], **({"worst_lo_to_half_ulp": r[1]} if mode else {})})
    print(case, "mode", mode, "error / bound", r)
    assert all(x <= 1.0 for x in r), (case, mode, r)


def _lens(mode, ns):
    return [n - 1 for n in ns] if mode == 0 else list(ns)


@functools.lru_cache(maxsize=4)
def _random_inputs(Hq, Hkv, Lmax, ns, mode, seed=0):
    """q with score standard deviation near 3 (a uniform softmax over thousands of keys hides a missing key), random K / V, NaN past ns[b];
    -> (q, K, V as the kernel reads them, scale, vscale, float64 reference).  Never modified by the tests that share it."""
    B = len(ns)
    g = torch.Generator().manual_seed(1000 * Lmax + 10 * Hq + Hkv + seed)
    q = 3.0 * torch.randn(B, Hq, HD, generator=g)
    k = torch.randn(B, Hkv, Lmax, HD, generator=g)
    v = torch.randn(B, Hkv, Lmax, HD, generator=g)
    q = q.to(torch.bfloat16) if mode == 0 else q
    if mode == 2:
        K, V = (k * KSCALE).to(torch.float16), (v * VSCALE).to(torch.float16)
        scale, vscale = _f32(SCALE / KSCALE), 1.0 / VSCALE
    else:
        K, V, scale, vscale = k.to(torch.bfloat16), v.to(torch.bfloat16), SCALE, 1.0
    ref = _reference(q, K, V, ns, scale, vscale)
    _nan_fill(K, ns, mode == 2)
    _nan_fill(V, ns, mode == 2)
    return q, K, V, scale, vscale, ref


def _run_random(lib, case, Hq, Hkv, Lmax, ns, mode, want_form, lens=None):
    form, lds = _form(lib, Hq, Hkv, Lmax)
    assert form == want_form, (form, lds)
    q, K, V, scale, vscale, ref = _random_inputs(Hq, Hkv, Lmax, tuple(ns), mode)
    planes = _launch(lib, mode, q, K, V, _lens(mode, ns) if lens is None else lens, Lmax, scale, vscale)
    _check(case, mode, planes, ref)
    return lds


# ---- 1. grouped form: the 256-key iteration (8 waves x 4 keys x 8-deep unroll), the 4-key lanes, Lmax no multiple of 4
LOOP_NS = (1, 2, 3, 4, 5, 31, 32, 33, 255, 256, 257, 511, 513, 808, 809)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("Hq,Hkv", [(7, 1), (4, 2), (8, 1), (2, 2)])
def test_grouped_kernel_loop_and_lane_edges(Hq, Hkv, mode):
    _run_random(_lib(), f"grouped_edges/Hq{Hq}_Hkv{Hkv}", Hq, Hkv, 809, LOOP_NS, mode, GROUPED)


# ---- 2. small odd caches
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("Hq,Hkv", [(7, 1), (2, 2)])
@pytest.mark.parametrize("Lmax", [1, 5, 130, 301])
def test_small_odd_caches(Lmax, Hq, Hkv, mode):
    _run_random(_lib(), f"small_cache/L{Lmax}_Hq{Hq}_Hkv{Hkv}", Hq, Hkv, Lmax, (1, Lmax), mode, GROUPED)


# ---- 3. grouped form with opt-in dynamic LDS (> 48 KiB), its largest cache, and the first one past it
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Lmax,form,lds", [(1760, GROUPED, 49280), (4388, GROUPED, 122864), (4389, PER_HEAD, 17556)])
def test_grouped_kernel_opt_in_lds_and_the_crossover(Lmax, form, lds, mode):
    got = _run_random(_lib(), f"crossover/L{Lmax}", 14, 2, Lmax, (Lmax, Lmax - 1, 257), mode, form)
    assert got == lds and (lds > 48 * 1024) == (Lmax != 4389)


# ---- 4. per-query-head kernel by group size (G > 8): 256 keys per score iteration, 4 per output iteration
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("Hq,Hkv", [(9, 1), (16, 1)])
def test_per_head_kernel_by_group_size(Hq, Hkv, mode):
    _run_random(_lib(), f"per_head/Hq{Hq}", Hq, Hkv, 520, (1, 3, 4, 5, 255, 256, 257, 519, 520), mode, PER_HEAD)


# ---- 5. per-query-head kernel with opt-in dynamic LDS, up to the launcher's limit.  At Hq = Hkv = 1 the 12 289-position cache (the first
# past 48 KiB) still takes the GROUPED form (G = 1: one padded row, below 120 KiB), so it is held as such and the per-head kernel's
# first opt-in size is reached at G = 3 (3 x 12 292 x 4 B > 120 KiB); 36 864 positions take the per-head kernel at any G.
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Hq,Lmax,form,lds", [(1, 12289, GROUPED, 49168), (3, 12289, PER_HEAD, 49156), (1, 36864, PER_HEAD, 147456)])
def test_per_head_kernel_opt_in_lds_and_the_limit(Hq, Lmax, form, lds, mode):
    got = _run_random(_lib(), f"per_head_lds/Hq{Hq}_L{Lmax}", Hq, 1, Lmax, (Lmax, 300), mode, form)
    assert got == lds > 48 * 1024


def test_a_cache_past_the_limit_is_refused_without_a_launch():
    lib = _lib()
    assert _form(lib, 1, 1, 36865) == (-1, 0) and _form(lib, 7, 1, 36865) == (-1, 0)
    x = torch.zeros(1, HD, dtype=torch.float32, device="cuda")          # would be far too small for a launch: the refusal comes first
    ln = torch.tensor([1], dtype=torch.int32, device="cuda")
    out = torch.full((2, HD), 3.0, dtype=torch.bfloat16, device="cuda")
    for mode in (0, 1, 2):
        assert lib.vqs_debug_qwen_decode_attention(x.data_ptr(), x.data_ptr(), x.data_ptr(), ln.data_ptr(), out.data_ptr(), HD, 1, 1, 1, 36865,
                                                   SCALE, 1.0, mode, _stream()) == INVALID
        assert lib.vqs_debug_qwen_decode_attention(x.data_ptr(), x.data_ptr(), x.data_ptr(), ln.data_ptr(), out.data_ptr(), HD, 1, 3, 2, 64,
                                                   SCALE, 1.0, mode, _stream()) == INVALID             # Hq % Hkv != 0
        assert lib.vqs_debug_qwen_decode_attention(None, x.data_ptr(), x.data_ptr(), ln.data_ptr(), out.data_ptr(), HD, 1, 1, 1, 64,
                                                   SCALE, 1.0, mode, _stream()) == INVALID
    assert lib.vqs_debug_qwen_decode_attention(x.data_ptr(), x.data_ptr(), x.data_ptr(), ln.data_ptr(), out.data_ptr(), HD, 1, 1, 1, 1, SCALE, 1.0, 3,
                                               _stream()) == INVALID
    torch.cuda.synchronize()
    assert (out == 3.0).all()


# ---- 6. length clamps: a length outside the cache is clamped to it, a count of 0 becomes 1
@pytest.mark.parametrize("Hq,Hkv,form", [(7, 1, GROUPED), (9, 1, PER_HEAD)])
def test_length_clamps(Hq, Hkv, form):
    lib, L = _lib(), 301
    _run_random(lib, f"clamp/Hq{Hq}", Hq, Hkv, L, (1, L, L, L), 0, form, lens=[-3, L - 1, L, L + 5])
    _run_random(lib, f"clamp/Hq{Hq}", Hq, Hkv, L, (1, 1, L), 1, form, lens=[0, -2, L + 9])


# ---- 7. needles: ONE key aligned with q carries the softmax (margin >= 30), its V row is a ramp no other row resembles
def _needle_inputs(Hq, Hkv, Lmax, n, needles, mode, seed):
    """Sample b: key needles[b] = c u, q = a u for a random unit u per sample; every other key is random with its u component removed,
    so its score is rounding noise.  V row needles[b] = (d + 1) 2^-b (exact in bf16 and fp16).  -> q, K, V, scale, vscale, expected rows."""
    B = len(needles)
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, 1, HD, generator=g, dtype=torch.float64)
    u = u / u.norm(dim=-1, keepdim=True)
    q = (32.0 * (1.0 + 0.25 * torch.rand(B, Hq, 1, generator=g, dtype=torch.float64)) * u).float()          # [B, Hq, 128]
    k = torch.randn(B, Hkv, Lmax, HD, generator=g, dtype=torch.float64)
    k = k - (k * u[:, None]).sum(-1, keepdim=True) * u[:, None]
    v = torch.randn(B, Hkv, Lmax, HD, generator=g)
    want = torch.empty(B, Hq, HD, dtype=torch.float64)
    for b, j in enumerate(needles):
        k[b, :, j] = 32.0 * u[b]
        v[b, :, j] = (torch.arange(HD) + 1).float() * 2.0 ** -b
        want[b] = v[b, 0, j].double()
    q = q.to(torch.bfloat16) if mode == 0 else q
    if mode == 2:
        K, V = (k * KSCALE).to(torch.float16), (v * VSCALE).to(torch.float16)
        scale, vscale = _f32(SCALE / KSCALE), 1.0 / VSCALE
    else:
        K, V, scale, vscale = k.to(torch.bfloat16), v.to(torch.bfloat16), SCALE, 1.0
    # the inputs, not the kernel: the needle's score leads every other key's by at least 30
    for b, j in enumerate(needles):
        s = torch.einsum("hd,hnd->hn", q[b].double(), K[b, :, :n].double().repeat_interleave(Hq // Hkv, dim=0)) * scale
        others = torch.cat([s[:, :j], s[:, j + 1:]], dim=1)
        assert others.numel() == 0 or (s[:, j] - others.amax(dim=1)).min().item() >= 30.0
    _nan_fill(K, [n] * B, mode == 2)
    _nan_fill(V, [n] * B, mode == 2)
    return q, K, V, scale, vscale, want


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("Hq,Hkv,Lmax,n,form", [(7, 1, 809, 257, GROUPED), (7, 1, 809, 808, GROUPED), (9, 1, 520, 520, PER_HEAD)])
def test_needle_key_is_found_wherever_it_lies(Hq, Hkv, Lmax, n, form, mode):
    lib = _lib()
    assert _form(lib, Hq, Hkv, Lmax)[0] == form
    needles = sorted({0, 255, 256, n - 1})
    q, K, V, scale, vscale, want = _needle_inputs(Hq, Hkv, Lmax, n, needles, mode, seed=n + Hq)
    planes = _launch(lib, mode, q, K, V, _lens(mode, [n] * len(needles)), Lmax, scale, vscale)
    _check(f"needle/Hq{Hq}_n{n}", mode, planes, want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Hq,Hkv,form", [(7, 1, GROUPED), (9, 1, PER_HEAD)])
def test_scores_spanning_plus_minus_200_need_the_max_subtraction(Hq, Hkv, form, mode):
    """Scores from -200 to +200 in shuffled key order: exp() of the raw scores overflows fp32, exp(t - max) does not.  The top key leads by
    30, so the fp32 rounding of the LARGE scores (2e-4 absolute at 200) stays out of the result and the usual bound holds."""
    lib, L, n = _lib(), 301, 300
    assert _form(lib, Hq, Hkv, L)[0] == form
    g = torch.Generator().manual_seed(200 + Hq)
    u = torch.randn(HD, generator=g, dtype=torch.float64)
    u = u / u.norm()
    t = torch.cat([torch.linspace(-200.0, 165.0, n - 1, dtype=torch.float64), torch.tensor([200.0], dtype=torch.float64)])
    t = torch.stack([t[torch.randperm(n, generator=g)] for _ in range(2)])                    # [2, n]: the top key elsewhere in each sample
    q = (32.0 * u).float().expand(2, Hq, HD).contiguous()
    k = torch.randn(2, Hkv, L, HD, generator=g, dtype=torch.float64)
    k = k - (k * u).sum(-1, keepdim=True) * u
    k[:, :, :n] += (t / (32.0 * SCALE)).view(2, 1, n, 1) * u
    v = torch.randn(2, Hkv, L, HD, generator=g)
    q = q.to(torch.bfloat16) if mode == 0 else q
    K, V = k.to(torch.bfloat16), v.to(torch.bfloat16)
    s = torch.einsum("bhd,bnd->bhn", q.double(), K[:, 0, :n].double()) * SCALE                # the inputs, not the kernel
    top2 = s.topk(2, dim=-1).values
    assert s.amax(-1).min() >= 190 and s.amin(-1).max() <= -190 and (top2[..., 0] - top2[..., 1]).min() >= 30.0
    ns = [n, n]
    ref = _reference(q, K, V, ns, SCALE)
    _nan_fill(K, ns, False)
    _nan_fill(V, ns, False)
    _check(f"span200/Hq{Hq}", mode, _launch(lib, mode, q, K, V, _lens(mode, ns), L, SCALE), ref)


# ---- 8. mode 2: fp16 K / V near 2^10 behind power-of-two scales, the reference in true units
@pytest.mark.parametrize("Hq,Hkv,form", [(7, 1, GROUPED), (9, 1, PER_HEAD)])
def test_fp16_cache_scales(Hq, Hkv, form):
    lib, L, ns = _lib(), 301, [1, 257, 301]
    assert _form(lib, Hq, Hkv, L)[0] == form
    ks, vs = 2.0 ** 8, 2.0 ** 9                              # |k| up to ~4.5, |v| up to ~4.5 / 2: stored magnitudes reach 2^10 .. 2^11
    g = torch.Generator().manual_seed(88 + Hq)
    q = 3.0 * torch.randn(3, Hq, HD, generator=g)
    K = (torch.randn(3, Hkv, L, HD, generator=g) * ks).to(torch.float16)
    V = (0.5 * torch.randn(3, Hkv, L, HD, generator=g) * vs).to(torch.float16)
    assert 2.0 ** 9 <= K.abs().max() < 2.0 ** 12 and 2.0 ** 9 <= V.abs().max() < 2.0 ** 12
    scale, vscale = _f32(1.0 / (math.sqrt(HD) * ks)), 1.0 / vs
    ref = _reference(q, K.double() / ks, V.double() / vs, ns, scale * ks)         # true units (ks, vs powers of two: exact)
    _nan_fill(K, ns, True)
    _nan_fill(V, ns, True)
    _check(f"fp16_scales/Hq{Hq}", 2, _launch(lib, 2, q, K, V, ns, L, scale, vscale), ref)


# ---- qwen_decode_rope_append_kernel
ROPE_LMAX = 37
ROPE_LEN = [0, 36, 17, -1, 37, 2 ** 31 - 1]


def _rope_case(Hq, Hkv, hd, half, lens, Lmax, seed, qkv=None):
    B = len(lens)
    g = torch.Generator().manual_seed(seed)
    if qkv is None:
        qkv = torch.randn(B, Hq + 2 * Hkv, hd, generator=g)
    qkv = qkv.to(torch.bfloat16)
    ang = 20.0 * torch.rand(B, half, generator=g, dtype=torch.float64)
    cs, sn = ang.cos().float(), ang.sin().float()
    q_out = torch.full((B, Hq, hd), SENTINEL, dtype=torch.int16)
    kc = torch.full((B, Hkv, Lmax, hd), SENTINEL, dtype=torch.int16)
    vc = torch.full((B, Hkv, Lmax, hd), SENTINEL, dtype=torch.int16)
    return qkv, cs, sn, q_out, kc, vc


def _rope_launch(lib, qkv, cs, sn, lens, q_out, kc, vc, Hq, Hkv, hd, half, Lmax):
    d = [x.contiguous().cuda() for x in (qkv, cs, sn, torch.tensor(lens, dtype=torch.int32), q_out, kc, vc)]
    rc = lib.vqs_debug_qwen_decode_rope_append(*(x.data_ptr() for x in d), len(lens), Hq, Hkv, hd, half, Lmax, _stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return d[4], d[5], d[6]                                  # device q_out, kc, vc (int16 views of bf16)


def _rope_ratio(got_bits, src, cs, sn, half):
    """got_bits [..., hd] int16 rows, src [..., hd] bf16 source rows, cs / sn [half] -> worst error-to-bound ratio of the rotated lanes;
    lanes >= 2 half must be bitwise the source."""
    got = got_bits.view(torch.bfloat16).double()
    a, c = src[..., :half].double(), src[..., half:2 * half].double()
    co, si = cs.double(), sn.double()
    ref = torch.cat([a * co - c * si, c * co + a * si], dim=-1)
    bound = 0.5 * _ulp_bf16(ref) + 2.0 ** -22 * torch.cat([a.abs() + c.abs()] * 2, dim=-1)
    assert torch.equal(got_bits[..., 2 * half:], src.view(torch.int16)[..., 2 * half:]), "pad lanes are not the source bits"
    return ((got[..., :2 * half] - ref).abs() / bound).max().item()


@pytest.mark.parametrize("Hq,Hkv,hd,half", [(4, 2, 128, 64), (7, 1, 128, 40), (2, 2, 128, 16)])
def test_rope_append_writes_one_row_and_nothing_else(Hq, Hkv, hd, half):
    lib, L, lens = _lib(), ROPE_LMAX, ROPE_LEN
    qkv, cs, sn, q_out, kc, vc = _rope_case(Hq, Hkv, hd, half, lens, L, seed=half + Hq)
    dq, dk, dv = (x.cpu() for x in _rope_launch(lib, qkv, cs, sn, lens, q_out, kc, vc, Hq, Hkv, hd, half, L))
    worst = 0.0
    for b, pos in enumerate(lens):
        if not 0 <= pos < L:                                 # outside the cache: the sample writes nothing, not even its q row
            assert (dq[b] == SENTINEL).all() and (dk[b] == SENTINEL).all() and (dv[b] == SENTINEL).all(), (b, pos)
            continue
        worst = max(worst, _rope_ratio(dq[b], qkv[b, :Hq], cs[b], sn[b], half), _rope_ratio(dk[b, :, pos], qkv[b, Hq:Hq + Hkv], cs[b], sn[b], half))
        assert torch.equal(dv[b, :, pos], qkv[b, Hq + Hkv:].view(torch.int16)), "V row is not the source bits"
        rest = torch.ones(L, dtype=torch.bool)
        rest[pos] = False
        assert (dk[b][:, rest] == SENTINEL).all() and (dv[b][:, rest] == SENTINEL).all(), (b, pos)
    _record(f"qwen_decode_kernels/rope_append/Hq{Hq}_Hkv{Hkv}_half{half}", {"worst_error_to_bound": worst})
    print("rope_append", Hq, Hkv, half, "error / bound", worst)
    assert worst <= 1.0, worst


def test_append_then_attend_finds_the_row_just_appended():
    """The decode step's two kernels in sequence on one cache: the new token's key (rotated with q: the rotation keeps their dot product) is
    the needle, its value row the ramp; every older cache row is small noise, rows past len[b] and the row to be appended start as NaN."""
    lib, Hq, Hkv, hd, half, L = _lib(), 4, 2, 128, 64, ROPE_LMAX
    lens = [0, 36, 17]
    B = len(lens)
    assert _form(lib, Hq, Hkv, L)[0] == GROUPED
    g = torch.Generator().manual_seed(5)
    u = torch.randn(B, 1, hd, generator=g)
    u = u / u.norm(dim=-1, keepdim=True)
    ramp = ((torch.arange(hd) + 1).float() * 2.0 ** -torch.arange(B).float().view(B, 1)).view(B, 1, hd)
    qkv = torch.cat([(32.0 * u).expand(B, Hq, hd), (32.0 * u).expand(B, Hkv, hd), ramp.expand(B, Hkv, hd)], dim=1)
    qkv, cs, sn, q_out, _, _ = _rope_case(Hq, Hkv, hd, half, lens, L, seed=6, qkv=qkv)
    kc = (0.05 * torch.randn(B, Hkv, L, hd, generator=g)).to(torch.bfloat16)
    vc = torch.randn(B, Hkv, L, hd, generator=g).to(torch.bfloat16)
    _nan_fill(kc, lens, False)                               # rows [len[b], Lmax): NaN, the appended row included
    _nan_fill(vc, lens, False)
    # the inputs: |q . k_old| scale <= 32 |k_old| / sqrt(128) stays 30 below the needle's 32^2 |u'|^2 / sqrt(128) (u' = u in bf16, rotated)
    old = 32.0 * 1.01 * kc.double().nan_to_num(0.0).norm(dim=-1).max().item() * SCALE
    assert 0.98 * 1024.0 * SCALE - old >= 30.0
    dq, dk, dv = _rope_launch(lib, qkv, cs, sn, lens, q_out, kc.view(torch.int16), vc.view(torch.int16), Hq, Hkv, hd, half, L)
    out = torch.full((B, Hq, hd), BF16_NAN, dtype=torch.int16).view(torch.bfloat16).cuda()
    ld = torch.tensor(lens, dtype=torch.int32).cuda()
    assert lib.vqs_debug_qwen_decode_attention(dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ld.data_ptr(), out.data_ptr(), 0, B, Hq, Hkv, L, SCALE, 1.0, 0,
                                               _stream()) == 0
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    _check("append_then_attend", 0, (got,), ramp.expand(B, Hq, hd).double())
