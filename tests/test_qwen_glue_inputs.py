"""CPU proof of tests/qwen_glue_cases.py (the cases of tests/test_gpu_qwen_glue_kernels.py), no GPU:
  1. the references alone do not spend the caps: a plain fp32 torch restatement of each arithmetic kernel stays inside the very criterion / bound the
     GPU test applies to the kernel, against the float64 reference;
  2. the exact cases are exact: evaluated in fp32 and in float64 they give the same bits, so no contraction or summation order can move them;
  3. every planted mistake of MISTAKES changes the expectation of every case it applies to -- the expectations can fail;
  4. every index map of every case is in range (the kernels define nothing else)."""
import pytest
import torch

from tests import qwen_glue_cases as qc

F16, BF16 = torch.float16, torch.bfloat16


def _bits(t):
    return t.contiguous().view(qc.BITS[t.dtype])


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def test_mistake_list_is_covered():
    import inspect
    src = inspect.getsource(inspect.getmodule(test_mistake_list_is_covered))
    for m in qc.MISTAKES:
        assert src.count('"%s"' % m) >= 1, m + ": planted but never shown to change an expectation"


# ---------------------------------------------------------------------------------------------------- scaled RMSNorm
@pytest.mark.parametrize("D", qc.NORM_D)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_norm_fp32_restatement_is_inside_the_criterion(D, dtype):
    worst = {"max_own_ulps": 0.0, "frac_diff": 0.0}
    for M in qc.NORM_M:
        x, _, _, w = qc.norm_inputs(M, D)
        for sc in qc.NORM_SCALES:
            dl1, dl2 = qc.norm_deltas(M, D, sc)
            for mode in qc.NORM_MODES[dtype]:
                s64, ref = qc.norm_expected(x, dl1, dl2, w, mode, sc, dtype)
                s32, got = qc.norm_expected(x, dl1, dl2, w, mode, sc, dtype, acc=torch.float32)
                assert _same(s64, s32)                                  # the stream never goes through `acc`
                ok, r = qc.criterion(ref, got)
                assert ok, (M, D, sc, mode, r)
                assert bool(torch.isfinite(ref.float()).all())
                worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"norm D={D} {dtype}: fp32 restatement worst {worst}")
    assert worst["max_own_ulps"] <= 1.0 and worst["frac_diff"] <= 1e-3     # far from the caps: what is left belongs to the kernel


def test_norm_stream_products_are_exact():
    """d * delta is exact in fp32 for every scale (fp16 significand times a power of two), so x + d1 delta1 rounds once whether contracted or not"""
    for sc in qc.NORM_SCALES:
        dl1, dl2 = qc.norm_deltas(70, 200, sc)
        for d, dl in ((sc[0], dl1), (sc[1], dl2)):
            assert torch.equal((dl.float() * d).double(), dl.double() * d)
            assert abs(float((dl.float() * d).std()) - 0.5) < 0.02         # the true delta has deviation 0.5 under every scale


@pytest.mark.parametrize("mistake", ["d_swapped", "out_on_stream", "mean_over_out_ld"])
def test_norm_mistakes_change_the_expectation(mistake):
    n = 0
    for M in qc.NORM_M:
        for D in qc.NORM_D:
            x, _, _, w = qc.norm_inputs(M, D)
            for sc in qc.NORM_SCALES:
                dl1, dl2 = qc.norm_deltas(M, D, sc)
                for dtype in (F16, BF16):
                    for mode in qc.NORM_MODES[dtype]:
                        for out_ld in qc.norm_pitches(D):
                            if not qc.norm_mistake_applies(mistake, mode, sc, D, out_ld):
                                continue
                            s, o = qc.norm_expected(x, dl1, dl2, w, mode, sc, dtype, out_ld=out_ld)
                            sm, om = qc.norm_expected(x, dl1, dl2, w, mode, sc, dtype, out_ld=out_ld, mistake=mistake)
                            assert not _same(o, om), (mistake, M, D, sc, mode, out_ld)
                            if mistake != "mean_over_out_ld" and mode in (1, 3):
                                assert not _same(s, sm), (mistake, M, D, sc, mode)
                            n += 1
    assert n >= 100


def test_norm_pitches_and_shapes():
    assert [qc.norm_pitches(D)[1] for D in qc.NORM_D] == [512, 1536, 1536, 4096]
    assert all(D % 4 == 0 and p % 4 == 0 for D in qc.NORM_D for p in qc.norm_pitches(D))


# ---------------------------------------------------------------------------------------------------- rope_qk, tail_rope_q
ROPE_GEOMETRIES = [(hq, hk, hd, half) for hq, hk in qc.ROPE_HEADS for hd, half in qc.ROPE_LANES]


@pytest.mark.parametrize("half", [40, 64])
@pytest.mark.parametrize("dtype,scale", [(F16, 1.0), (F16, 2.0 ** -5), (BF16, 1.0)], ids=["f16", "f16-scaled", "bf16"])
def test_rope_fp32_restatement_is_inside_the_criterion(half, dtype, scale):
    for Hq, Hk in qc.ROPE_HEADS:
        for S in qc.ROPE_S:
            q, k, cos, sin = qc.rope_inputs(Hq, Hk, S, 128, half, dtype, False, scale=scale)
            for ref, got in zip(qc.rope_qk_expected(q, k, cos, sin, half), qc.rope_qk_expected(q, k, cos, sin, half, acc=torch.float32)):
                ok, r = qc.criterion(ref, got)
                assert ok and r["max_own_ulps"] <= 1.0 and r["frac_diff"] <= 1e-3, (Hq, Hk, S, half, r)


@pytest.mark.parametrize("Hq,Hk,hd,half", ROPE_GEOMETRIES)
def test_rope_exact_cases_are_exact_and_keep_the_other_lanes(Hq, Hk, hd, half):
    for dtype in (F16, BF16):
        for S in qc.ROPE_S:
            q, k, cos, sin = qc.rope_inputs(Hq, Hk, S, hd, half, dtype, True)
            e64 = qc.rope_qk_expected(q, k, cos, sin, half)
            e32 = qc.rope_qk_expected(q, k, cos, sin, half, acc=torch.float32)
            for x, a, b in zip((q, k), e64, e32):
                assert _same(a, b)
                assert torch.equal(a.double()[..., :half], x.double()[..., :half] * cos.double().view(qc.ROPE_B, 1, S, half)
                                   - x.double()[..., half:2 * half] * sin.double().view(qc.ROPE_B, 1, S, half))       # no rounding happened at all
                assert _same(a[..., 2 * half:], x[..., 2 * half:])
                assert not _same(a, x)


@pytest.mark.parametrize("mistake", ["partner_hd_half", "k_heads_by_hq", "table_row_by_s", "rotate_pad_lanes"])
def test_rope_mistakes_change_the_expectation(mistake):
    n = 0
    for Hq, Hk, hd, half in ROPE_GEOMETRIES:
        if not qc.rope_mistake_applies(mistake, Hq, Hk, hd, half):
            continue
        for exact in (True, False):
            for dtype in (F16, BF16):
                for S in qc.ROPE_S:
                    q, k, cos, sin = qc.rope_inputs(Hq, Hk, S, hd, half, dtype, exact)
                    good, bad = qc.rope_qk_expected(q, k, cos, sin, half), qc.rope_qk_expected(q, k, cos, sin, half, mistake=mistake)
                    if mistake != "k_heads_by_hq":
                        assert not _same(good[0], bad[0]), (mistake, Hq, Hk, hd, half, S, dtype)
                    assert not _same(good[1], bad[1]), (mistake, Hq, Hk, hd, half, S, dtype)
                    n += 1
    assert n >= 20
    if mistake != "k_heads_by_hq":                          # the tail's rotation: the same three index mistakes
        for Hq, _ in qc.ROPE_HEADS:
            for hd, half in qc.ROPE_LANES:
                if not qc.rope_mistake_applies(mistake, 1, 1, hd, half, B=qc.TAIL_B):
                    continue
                for exact in (True, False):
                    qkv, ld, cos, sin, row = qc.tail_rope_inputs(Hq, hd, half, exact)
                    good, _ = qc.tail_rope_expected(qkv, cos, sin, row, Hq, hd, half)
                    bad, _ = qc.tail_rope_expected(qkv, cos, sin, row, Hq, hd, half, mistake=mistake)
                    assert not torch.equal(good, bad), (mistake, Hq, hd, half)


def test_tail_rope_restatement_is_inside_its_bound_and_exact_cases_are_exact():
    for Hq, _ in qc.ROPE_HEADS:
        for hd, half in qc.ROPE_LANES:
            qkv, ld, cos, sin, row = qc.tail_rope_inputs(Hq, hd, half, False)
            assert ld > Hq * hd and len(set(row.tolist())) == qc.TAIL_B and int(row.max()) == cos.shape[0] - 1 and int(row.min()) == 0
            ref, mag = qc.tail_rope_expected(qkv, cos, sin, row, Hq, hd, half)
            got, _ = qc.tail_rope_expected(qkv, cos, sin, row, Hq, hd, half, acc=torch.float32)
            assert bool(((got.double() - ref).abs() <= qc.TAIL_ROPE_BOUND * mag).all())
            assert bool((mag.view(qc.TAIL_B, Hq, hd)[..., 2 * half:] == 0).all())           # copied lanes: equality is demanded
            qkv, ld, cos, sin, row = qc.tail_rope_inputs(Hq, hd, half, True)
            e64, _ = qc.tail_rope_expected(qkv, cos, sin, row, Hq, hd, half)
            e32, _ = qc.tail_rope_expected(qkv, cos, sin, row, Hq, hd, half, acc=torch.float32)
            assert torch.equal(e64, e32.double())


# ---------------------------------------------------------------------------------------------------- gathers, embed, fp16 -> bf16
@pytest.mark.parametrize("name", [c[0] for c in qc.GATHER_ROWS_CASES])
def test_gather_rows_cases_are_in_range_and_their_mistakes_show(name):
    src0, src1, rmap, rows, cols, src_ld, dst_ld = qc.gather_rows_inputs(name)
    assert src0.shape[1] == src_ld >= cols and dst_ld >= cols and rows >= 1
    if rmap is None:
        assert src0.shape[0] == rows
    else:
        m = rmap.long()
        assert len(m) == rows and int(m.max()) < src0.shape[0]
        if bool((m <= -2).any()):
            assert src1 is not None and int((-m[m <= -2] - 2).max()) < src1.shape[0]
    want = qc.gather_rows_expected(src0, src1, rmap, cols, dst_ld)
    assert want.shape == (rows, dst_ld) and bool((want[:, cols:].view(torch.int16) == 0).all())
    if src1 is not None:
        assert not _same(want, qc.gather_rows_expected(src0, src1, rmap, cols, dst_ld, mistake="src1_row_off_by_one"))
    if dst_ld > cols:
        assert not _same(want, qc.gather_rows_expected(src0, src1, rmap, cols, dst_ld, mistake="no_zero_fill"))


def test_gather_rows_cases_cover_what_the_engine_does():
    c = {x[0]: x for x in qc.GATHER_ROWS_CASES}
    assert {x[1] for x in qc.GATHER_ROWS_CASES} >= {1, 257}
    assert c["identity-pad-1176-1216"][2:5] == (1176, 1176, 1216) and any(x[2:5] == (1, 1, 1) for x in qc.GATHER_ROWS_CASES)
    assert any(x[4] % 256 for x in qc.GATHER_ROWS_CASES) and any(x[3] != x[4] for x in qc.GATHER_ROWS_CASES)
    m = qc.gate_up_map(64)
    assert m[:32].tolist() == list(range(32)) and m[32:64].tolist() == [-r - 2 for r in range(32)] and m[64:96].tolist() == list(range(32, 64))


def test_gather_cols_and_f32_cases_are_in_range():
    for d in ("spread", "compact"):
        src, cmap, rows, src_ld, dst_cols = qc.gather_cols_inputs(d)
        assert int(cmap.max()) < src_ld and int(cmap.min()) >= -1 and src.shape == (rows, src_ld)
        want = qc.gather_cols_expected(src, cmap)
        assert want.shape == (rows, dst_cols)
        assert bool((cmap == -1).any()) == (d == "spread")
    s, cm, *_ = qc.gather_cols_inputs("spread")
    back = qc.gather_cols_expected(qc.gather_cols_expected(s, cm), qc.gather_cols_inputs("compact")[1])
    assert _same(back, s)                                                           # the two maps are each other's inverse
    for D in qc.GATHER_F32_D:
        for form in (0, 1):
            src, rmap, rows, src_ld = qc.gather_f32_inputs(D, form)
            assert int(rmap.max()) < src.shape[0] and int(rmap.min()) >= (-1 if form == 0 else 0) and (src_ld > D) == (form == 1)
            assert bool((rmap == -1).any()) == (form == 0)
            assert qc.gather_f32_expected(src, rmap, D).shape == (rows, D)


def test_embed_cases():
    for D in qc.EMBED_D:
        for f16 in (False, True):
            ids, vis, embed, merged, rows = qc.embed_inputs(D, f16)
            assert int(ids.min()) < 0 and int(ids.max()) >= qc.EMBED_VOCAB and int(vis.max()) == qc.EMBED_SLOTS - 1 and int(vis.min()) == -1
            assert bool((vis[(ids < 0) | (ids >= qc.EMBED_VOCAB)] == -1).all())       # the clamped ids sit on text rows
            for u in (1.0, 2.0, 32.0):
                want = qc.embed_expected(ids, vis, embed, merged, u)
                assert _same(want[1], embed[0].float()) and _same(want[5], embed[-1].float())
                if f16:
                    assert torch.equal(want[vis >= 0].double(), merged[vis[vis >= 0].long()].double() * u)      # the fp32 product is exact
                    assert bool(torch.isfinite(want[vis >= 0]).all())


@pytest.mark.parametrize("cols", qc.F16_COLS)
def test_f16_rows_cases_and_the_planted_order_of_rounding(cols):
    src, src_ld = qc.f16_rows_inputs(cols)
    assert bool(torch.isfinite(src.float()).all()) and src_ld > cols
    assert int(src.view(torch.int16)[0, 0]) == 0x7BFF and float(src[0, 2]) == 2.0 ** -24
    for u in (1.0, 2.0 ** -5, 8.0):
        want = qc.f16_rows_expected(src, cols, u)
        assert torch.equal((src[:, :cols].float() * u).double(), src[:, :cols].double() * u)          # exact product: one rounding
        assert bool(torch.isfinite(want.float()).all())
        assert _same(want, qc.f16_rows_expected(src, cols, u, mistake="unscale_after_rounding"))      # a power of two commutes with the rounding ...
    want = qc.f16_rows_expected(src, cols, 3.0)                                                       # ... a factor of 3 does not: the case that pins the order
    assert torch.equal((src[:, :cols].float() * 3.0).double(), src[:, :cols].double() * 3.0)
    assert not _same(want, qc.f16_rows_expected(src, cols, 3.0, mistake="unscale_after_rounding"))
    if cols >= 16:       # ties to even in both directions, and the neighbours of the midpoint
        w1 = qc.f16_rows_expected(src, cols, 1.0)[0]
        assert [float(w1[i]) for i in (6, 7, 8, 9)] == [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 1.0]
        assert float(w1[0]) == 65536.0 and float(w1[10]) == 2.0


# ---------------------------------------------------------------------------------------------------- range proof
def test_absmax_and_gate_pair_cases():
    for n in qc.ABSMAX_N:
        x = qc.absmax_inputs(n)
        assert float(x.float().abs().max()) == 5.5 and float(x[-1]) == -5.5 and (n == 1 or float(x[:-1].float().abs().max()) < 5.5)
        assert float(qc.absmax_expected(x, qc.ABSMAX_R)) == float(torch.tensor(qc.ABSMAX_R) * 5.5)
    for mlp_p in (32, 96):
        rb = qc.gate_pair_inputs(mlp_p)
        for ld in (mlp_p, mlp_p + 32):
            u = qc.gate_pair_expected(rb, mlp_p, ld)
            assert bool((u[mlp_p:] == 0).all()) and bool((u[:mlp_p] > 0).all())
            assert float(u[33 % mlp_p]) == float(rb[(33 % mlp_p) // 32 * 64 + 1] * rb[(33 % mlp_p) // 32 * 64 + 33])
            if mlp_p > 32:                                   # one block pairs the same rows either way
                assert not torch.equal(u, qc.gate_pair_expected(rb, mlp_p, ld, mistake="pair_blocks_of_32"))


@pytest.mark.parametrize("K", qc.ROWBOUND_K)
def test_rowbound_exact_cases_are_exact(K):
    for N in qc.ROWBOUND_N:
        W, g, u, bias = qc.rowbound_inputs(N, K, True)
        assert W.shape == (N, K + 8) and K % 4 == 0
        for g_len in (K, K // 4):
            for b in (bias, None):
                e64 = qc.rowbound_expected(W, K, 0, g, g_len, qc.ROWBOUND_R_EXACT, None, None, b)
                e32 = qc.rowbound_expected_exact(W, K, 0, g, g_len, qc.ROWBOUND_R_EXACT, None, None, b)
                t = W[:, :K].double() * g[torch.arange(K) % g_len].double()
                assert float((t * t).sum(1).max()) * 16 < 2 ** 24                                       # every partial sum is an integer count of 1/16 units
                # the square root is the one inexact step: fp32 and float64 agree to one fp32 rounding of it
                assert bool(((e32.double() - e64).abs() <= 2.0 ** -23 * e64).all())
                root = torch.sqrt((t * t).sum(1)).float()                                             # the correctly rounded fp32 root: the squares of the
                lo = (torch.nextafter(root, torch.zeros_like(root)).double() + root.double()) / 2      # midpoints to its fp32 neighbours bracket the sum
                hi = (torch.nextafter(root, torch.full_like(root, 1e30)).double() + root.double()) / 2
                assert bool((lo * lo < (t * t).sum(1)).all()) and bool((hi * hi > (t * t).sum(1)).all())
                if g_len < K:
                    bad = qc.rowbound_expected(W, K, 0, g, g_len, qc.ROWBOUND_R_EXACT, None, None, b, mistake="g_clamped")
                    assert not torch.equal(e64, bad), (N, K)
        for uu, uc in ((u, None), (None, 1.5)):
            for b in (bias, None):
                e64 = qc.rowbound_expected(W, K, 1, None, 0, 0.0, uu, uc, b)
                e32 = qc.rowbound_expected_exact(W, K, 1, None, 0, 0.0, uu, uc, b)
                assert torch.equal(e64, e32.double()) and torch.equal(e32, qc.rowbound_expected(W, K, 1, None, 0, 0.0, uu, uc, b, acc=torch.float32))


@pytest.mark.parametrize("K", qc.ROWBOUND_ARITH_K)
def test_rowbound_fp32_restatement_is_inside_its_bound(K):
    W, g, u, bias = qc.rowbound_inputs(qc.ROWBOUND_ARITH_N, K, False)
    R = float(torch.tensor(float(K)).sqrt())
    for mode, args in ((0, (g, K, R, None, None)), (0, (g, K // 4, R, None, None)), (1, (None, 0, 0.0, u, None)), (1, (None, 0, 0.0, None, 0.75))):
        ref = qc.rowbound_expected(W, K, mode, *args, bias)
        got = qc.rowbound_expected(W, K, mode, *args, bias, acc=torch.float32).double()
        assert bool((ref > 0).all())
        assert bool(((got - ref).abs() <= qc.rowbound_bound(K) * ref).all()) and bool((got <= qc.ROWBOUND_HEADROOM * ref).all())
        assert qc.rowbound_bound(K) < qc.ROWBOUND_HEADROOM - 1.0 or K > 495                           # the head room covers the bound up to K = 495 ...
    assert qc.rowbound_bound(5120) > qc.ROWBOUND_HEADROOM - 1.0                                       # ... so at 1280 and 5120 the second condition is the sharper one
