"""The reference helpers of tests/test_gpu_precise_decoder_kernels.py (tests/precise_decoder_ref.py) held to the oracles on the CPU: a bug in a
reference must neither pass for a kernel bug nor hide one.  The split / ulp helpers against oracle/clip_t5_engine_rounding.py, the
activations, the norm and the score head against oracle/clip_t5_oracle.py, the gate | up column map against the packing's definition, the
attention references against torch's softmax and oracle/clip_t5_engine_rounding.py's tiled restatement, and the cached form against the
teacher-forced one.  Last, each criterion's bound holds for the correctly rounded float64 reference: with a ratio of 0.5 at most for the
fp32 and split outputs, below 1 for an output whose one 16-bit rounding is the bound's leading term."""
import numpy as np
import pytest
import torch

from oracle import clip_t5_engine_rounding as ER
from oracle import clip_t5_oracle as OR
from tests import precise_decoder_ref as R


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_ulp_helper_is_the_spacing_of_the_format():
    g = _gen(1)
    x = torch.randn(4096, generator=g) * torch.exp(8.0 * torch.randn(4096, generator=g))
    for dtype, bits in ((torch.bfloat16, R.BF16_BITS), (torch.float16, R.F16_BITS)):
        v = x.to(dtype)
        v = v[torch.isfinite(v.float()) & (v != 0)]
        up = torch.nextafter(v.abs(), torch.full_like(v, float("inf")))
        ok = torch.isfinite(up.float())
        assert torch.equal((up.double() - v.abs().double())[ok], R.ulp16(v.double(), bits)[ok])
    assert R.ulp16(torch.tensor([1.0, 1.5, 2.0, 0.75]), 8).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8]
    assert R.ulp16(torch.tensor([0.0, 2.0 ** -14, 2.0 ** -20]), R.F16_BITS).tolist() == [2.0 ** -24] * 3       # fp16 subnormals
    assert R.ulp16(torch.tensor([0.0]), R.BF16_BITS).item() == 2.0 ** -133


def test_split_helper_is_the_engine_rounding_oracles_split():
    x = torch.randn(5000, generator=_gen(2)) * 37.0
    hi, lo = R.split_bf16(x.double())
    assert torch.equal((hi + lo).float(), ER.split_bf16_round(x))
    assert torch.equal(hi.float(), ER.bf16_round(x))
    assert (lo.abs() <= 0.5 * R.ulp16(hi)).all()
    # 16 significant bits: a lost lo plane is a hundred times the split criterion, a kept one is well inside it
    ref = x.double().reshape(50, 100)
    assert R.ratio_split(*R.split_bf16(ref), ref)[0] <= 0.5
    assert R.ratio_split(R.split_bf16(ref)[0], torch.zeros_like(ref), ref)[0] > 20.0


def test_activations_are_the_oracles():
    x = torch.linspace(-6.0, 6.0, 2401, dtype=torch.float64)
    assert torch.allclose(R.gelu_new(x), OR.gelu_new(x), rtol=0, atol=1e-14)               # HF's tanh form
    assert torch.allclose(R.gelu_new(x), ER.gelu_new_sigmoid(x), rtol=1e-14, atol=0)        # the engine's sigmoid form
    assert torch.allclose(R.silu(x), torch.nn.functional.silu(x), rtol=1e-15, atol=0)
    # the tails: no cancellation to 0 where the tanh form loses every digit
    t = torch.tensor([-30.0, -8.0, -1e-3, 0.0, 1e-3, 8.0, 30.0], dtype=torch.float64)
    g = R.gelu_new(t)
    assert g[0] == 0 and -4e-21 < g[1] < -2e-21 and g[3] == 0 and g[5] == 8.0 and g[6] == 30.0
    assert abs(R.silu(t)[0].item() / (-30.0 * np.exp(-30.0)) - 1.0) < 1e-12


def test_gate_pack_index_map():
    rows, F = 3, 160
    gate = torch.arange(rows * F, dtype=torch.float64).reshape(rows, F)
    up = -gate - 1.0
    packed = R.pack_gate_up(gate, up)
    for j in range(F // 32):                                  # the definition: block j = 32 gate | 32 up columns
        assert torch.equal(packed[:, 64 * j:64 * j + 32], gate[:, 32 * j:32 * j + 32])
        assert torch.equal(packed[:, 64 * j + 32:64 * j + 64], up[:, 32 * j:32 * j + 32])
    oc = torch.arange(F)
    gc = R.gate_col(oc)
    assert torch.equal(gc, (oc >> 5) * 64 + (oc & 31))
    assert torch.equal(packed[:, gc], gate) and torch.equal(packed[:, gc + 32], up)
    assert [R.gate_col(c) for c in (0, 28, 31, 32, 35, 60, 63, 64, 67)] == [0, 28, 31, 64, 67, 92, 95, 128, 131]
    ident = R.gated(packed, lambda x: x.double())
    assert torch.equal(ident, gate * up)


def test_reductions_read_the_layout_they_are_given():
    rows, cols, ldp, ns = 3, 8, 12, 4
    stride = 2 * rows * ldp + 8
    part = torch.full(((ns - 1) * stride + 2 * rows * ldp,), float("nan"))
    want = torch.zeros(rows, cols, dtype=torch.float64)
    g = _gen(3)
    for k in range(ns):
        for p in range(2):
            blk = torch.randn(rows, cols, generator=g)
            want += blk.double()
            for r in range(rows):
                o = k * stride + (p * rows + r) * ldp
                part[o:o + cols] = blk[r]
    bias = torch.randn(cols, generator=g).to(torch.bfloat16)
    assert torch.allclose(R.sum_planes_y(part, ns, stride, rows, cols, ldp), want, rtol=0, atol=1e-13)
    assert torch.allclose(R.sum_planes_y(part, ns, stride, rows, cols, ldp, bias), want + bias.double(), rtol=0, atol=1e-13)
    y32 = R.sum_planes_y(part, ns, stride, rows, cols, ldp, dtype=torch.float32)
    assert y32.dtype == torch.float32 and torch.allclose(y32.double(), want, rtol=0, atol=1e-5)
    hi_only = R.reduce_slices_y(part, ns, stride, rows, cols, ldp)
    assert torch.isfinite(hi_only).all() and not torch.allclose(hi_only, want)


def test_rmsnorm_and_score_head_are_the_oracles():
    g = _gen(4)
    x, w = torch.randn(5, 96, generator=g, dtype=torch.float64) * 3.0, torch.randn(96, generator=g, dtype=torch.float64)
    assert torch.allclose(R.rmsnorm(x, w, 1e-6), OR.t5_rms_norm(x, w, 1e-6), rtol=1e-13, atol=0)
    assert (R.rmsnorm(torch.zeros(1, 8), torch.ones(8), 1e-6) == 0).all()
    V, ldl = 50, 56
    lg = torch.randn(4, 3, ldl, generator=g, dtype=torch.float64) * 5.0
    labels = torch.randint(0, V, (4, 3), generator=g)
    labels[0] = -100
    labels[1, 1] = -100
    lp, sc = R.label_logprobs(lg, labels, V)
    want_lp = OR.Oracle.label_logprobs(lg[..., :V].float(), labels)
    assert torch.allclose(lp.float(), want_lp, rtol=1e-5, atol=1e-5)
    want_sc = OR.Oracle.scores_from_logprobs(want_lp, labels)
    ok = (labels != -100).any(-1)
    assert torch.allclose(sc.float()[ok], want_sc[ok], rtol=1e-5, atol=0)
    assert sc[0] == 1.0                                       # no label: exp(0 / max(0, 1))
    labels[2, 0] = V + 3                                      # out of range: log-prob 0, still counted
    lp2, sc2 = R.label_logprobs(lg, labels, V)
    assert lp2[2, 0] == 0 and torch.isclose(sc2[2], torch.exp((lp[2, 1] + lp[2, 2]) / 3))
    lg[..., V:] = float("nan")                                # columns past V are not read
    assert torch.equal(R.label_logprobs(lg, labels, V)[0], lp2)


def test_masked_softmax_reference():
    sc = torch.randn(6, 64, generator=_gen(5), dtype=torch.float64)
    lens = [1, 40, 70]
    want = torch.zeros(6, 64, dtype=torch.float64)
    for r in range(6):
        n = min(lens[r // 2], 64)
        e = torch.exp(sc[r, :n] - sc[r, :n].max())
        want[r, :n] = e / e.sum()
    poisoned = sc.clone()
    for r in range(6):
        poisoned[r, min(lens[r // 2], 64):] = float("nan")
    assert torch.allclose(R.masked_softmax(poisoned, lens, 2), want, rtol=1e-14, atol=0)
    assert (R.masked_softmax(poisoned, [0, 0, 0], 2) == 0).all()


@pytest.mark.parametrize("T,H", [(1, 1), (5, 3), (16, 2)])
def test_self_attention_reference_against_the_tiled_restatement(T, H):
    g = _gen(T)
    B = 2
    q, k, v = (0.5 * torch.randn(B, T, H, 64, generator=g) for _ in range(3))
    table = torch.randn(H, T, generator=g)                    # indexed by query - key
    got = R.self_attention(q, k, v, table)
    # by hand, per (sample, head, query)
    for b, h, t in [(0, 0, 0), (B - 1, H - 1, T - 1), (1, 0, T // 2)]:
        s = torch.stack([(q[b, t, h].double() * k[b, j, h].double()).sum() + table[h, t - j].double() for j in range(t + 1)])
        p = torch.softmax(s, 0)
        want = (p[:, None] * v[b, :t + 1, h].double()).sum(0)
        assert torch.allclose(got[b, t, h * 64:(h + 1) * 64], want, rtol=0, atol=1e-13)
    # oracle/clip_t5_engine_rounding.py: causal tiled attention, unrounded, its bias table indexed by key - query + S - 1
    enc_table = torch.zeros(H, 2 * T - 1)
    enc_table[:, :T] = table.flip(-1)                         # rel = -(dist): entry (T - 1 - dist)
    hm = lambda x: x.permute(0, 2, 1, 3).contiguous()         # noqa: E731  [B, H, T, 64]
    tiled = ER.tiled_attention(hm(q), hm(k), hm(v), 1.0, bias_table=enc_table, round_fn=lambda x: x, causal=True)
    assert torch.allclose(tiled.double(), got, rtol=0, atol=2e-5 * got.abs().max().item())


@pytest.mark.parametrize("T,qpos0", [(1, 0), (1, 1), (1, 37), (3, 5), (4, 12)])
def test_cached_reference_is_the_teacher_forced_one(T, qpos0):
    g = _gen(qpos0 + T)
    B, H, S = 2, 2, qpos0 + T
    q, k, v = (0.5 * torch.randn(B, S, H, 64, generator=g, dtype=torch.float64) for _ in range(3))
    table = torch.randn(H, S + 2, generator=g, dtype=torch.float64)
    full = R.self_attention(q, k, v, table)
    pad = torch.full((B, 3, H, 64), float("nan"), dtype=torch.float64)        # cache rows past qpos0 + T are not read
    cached = R.self_attention(q[:, -T:], torch.cat([k, pad], 1), torch.cat([v, pad], 1), table, qpos0=qpos0)
    assert torch.allclose(cached, full[:, -T:], rtol=0, atol=1e-13)
    if qpos0:                                                 # and it is not the uncached answer
        assert not torch.allclose(R.self_attention(q[:, -T:], k[:, -T:], v[:, -T:], table), full[:, -T:], atol=1e-6)


def test_cross_attention_reference():
    g = _gen(9)
    B, T, H, S = 2, 3, 2, 20
    q = torch.randn(B, T, H, 64, generator=g) * 0.5
    k, v = torch.randn(B, H, S, 64, generator=g) * 0.5, torch.randn(B, H, S, 64, generator=g)
    lens = [4, 20]
    got = R.cross_attention(q, k, v, lens)
    s = torch.einsum("bthd,bhjd->bhtj", q.double(), k.double())
    s = s.masked_fill(torch.arange(S)[None, None, None] >= torch.tensor(lens)[:, None, None, None], float("-inf"))
    want = torch.einsum("bhtj,bhjd->bthd", torch.softmax(s, -1), v.double()).reshape(B, T, H * 64)
    assert torch.allclose(got, want, rtol=0, atol=1e-13)


def test_each_criterion_holds_for_the_correctly_rounded_reference():
    g = _gen(10)
    ref = torch.randn(40, 96, generator=g, dtype=torch.float64) * torch.exp(2.0 * torch.randn(40, 1, generator=g, dtype=torch.float64))
    assert R.ratio_f32(ref.float(), ref) <= 0.5
    r_sum, r_lo = R.ratio_split(*R.split_bf16(ref), ref)
    assert r_sum <= 0.5 and r_lo <= 1.0
    # one 16-bit rounding: the rounding IS the bound's leading term (0.5 ulp), so the correct rounding reaches it but never passes it, and
    # what it leaves of the fp32 term is nothing
    assert 0.5 < R.ratio_16(ref.float().to(torch.bfloat16), ref, R.BF16_BITS) < 1.0
    assert 0.5 < R.ratio_16(ref.float().to(torch.float16), ref, R.F16_BITS) < 1.0
    assert R.excess(ref.float().to(torch.bfloat16), ref, R.BF16_BITS) == 0 and R.excess(ref.float(), ref) < 0.01
    # and what the criteria exist to catch does fail: a value one ulp off, a value of the neighbouring column
    off = ref.float().to(torch.bfloat16).double() + R.ulp16(ref)
    assert R.ratio_16(off, ref, R.BF16_BITS) > 1.0
    assert R.ratio_f32(ref.roll(1, dims=1), ref) > 1.0
    # the caps: an allowance may not let a lost lo plane or a one-ulp error through
    assert R.allowance_caps_hold(0.0, "split") and R.allowance_caps_hold(11.0, "split") and not R.allowance_caps_hold(11.3, "split")
    assert R.allowance_caps_hold(23.0, "f16") and not R.allowance_caps_hold(23.5, "f16")
    assert R.allowance_caps_hold(194.0, "bf16") and not R.allowance_caps_hold(194.4, "bf16")
    assert R.dec_attn_lds_bytes(16, 702) <= 65536 < R.dec_attn_lds_bytes(16, 703)
