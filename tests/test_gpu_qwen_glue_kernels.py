"""Single launches of the Qwen2.5-VL prefill's glue and of the bind-time range proof (-m gpu), through the hooks of include/vqs_debug.h: the scaled
RMSNorm (norm_rows_reg_kernel / norm_rows_loop_kernel with scales), rope_qk_kernel, qwen_embed_kernel, the bf16 / fp32 gathers, f16_to_bf16_rows_kernel,
qwen_tail_rope_q_kernel, rowbound_kernel, absmax_bf16_kernel and gate_pair_bound_kernel.  Cases, references and bounds: tests/qwen_glue_cases.py, proven
on the CPU by tests/test_qwen_glue_inputs.py; measured worst values: profiles/qwen_glue_kernels.md.

  test_exact_*       copies and exact arithmetic: the whole buffer -- guards, pad columns, untouched lanes -- bit for bit
  test_identity_*    two launches that must agree bit for bit (no reference)
  test_arithmetic_*  random operands against float64 under the per-launch criterion (one own ulp; 0.5 % / 2 % different at all) or a derived bound;
                     the figures go to the suite's parity_e2e.jsonl record (tests/test_gpu_e2e.py) under qwen_glue/
  test_*refus*       VQS_ERR_INVALID and not one byte written
Every tensor a launch writes sits between guards (and in front of guard columns where it has a pitch) filled with a sentinel pattern."""
import pytest
import torch

from tests import qwen_glue_cases as qc
from tests.qwen_glue_cases import Buf
from tests.test_gpu_e2e import _record

pytestmark = pytest.mark.gpu

INVALID = -1
F16, BF16 = torch.float16, torch.bfloat16
NAN_SLOT = 0x7FC00000


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from t2v_metrics_amd import engine
    return engine.load_library()


def _st():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _same_bits(got, want, what):
    g, w = got.bits(), want.bits()
    assert torch.equal(g, w), f"{what}: {qc.first_difference(g, w)}"


class _Pool:
    """The criterion, launch by launch, over the launches of one parametrised case; the record keeps the worst launch and the fraction of elements
    different at all over the case's launches together (its smallest tensors have 128 to 200 elements, where one element is 0.5 to 0.8 %)."""

    def __init__(self, dtype):
        self.dtype, self.ulps, self.frac, self.diff, self.n, self.launches = dtype, 0.0, 0.0, 0.0, 0, 0

    def add(self, ref, got, what):
        ok, r = qc.criterion(ref, got)
        self.ulps, self.frac = max(self.ulps, r["max_own_ulps"]), max(self.frac, r["frac_diff"])
        self.diff, self.n, self.launches = self.diff + r["frac_diff"] * r["n"], self.n + r["n"], self.launches + 1
        assert ok, (what, r)

    def close(self, name):
        m, pooled = qc.MANT[self.dtype], self.diff / max(self.n, 1)
        print(f"{name}: max_own_ulps {self.ulps:.4f} frac_diff {self.frac:.6f} (worst launch) {pooled:.6f} (all) over {self.launches} launches, {self.n} elements")
        _record("qwen_glue/" + name, {"max_own_ulps": self.ulps, "frac_diff": self.frac, "frac_diff_pooled": pooled, "mant_bits": m, "elements": self.n,
                                      "launches": self.launches, "limits": {"max_own_ulps": qc.MAX_OWN_ULPS, "frac_diff": qc.MAX_FRAC_DIFF[m]}})


# ---------------------------------------------------------------------------------------------------- scaled RMSNorm
def _norm(lib, x, dl1, dl2, w, mode, sc, dtype, out_ld):
    """one launch of add mode `mode` on device copies -> (return code, the stream's buffer, the operand's buffer)"""
    M, D = x.shape
    xb, ob = Buf.of(x, device="cuda"), Buf(M, out_ld, dtype, "cuda")
    d1t = dl1.cuda() if mode else None
    d2t = dl2.cuda() if mode == 3 else None
    rc = lib.vqs_debug_rmsnorm_f16s(xb.ptr(), _p(d1t), _p(d2t), 0 if mode == 2 else 1, w.data_ptr(), ob.ptr(), out_ld, M, D, qc.NORM_EPS, sc[0], sc[1], sc[2],
                                    1 if dtype == BF16 else 0, _st())
    torch.cuda.synchronize()
    return rc, xb, ob


NORM_PARAMS = [(D, dtype, mode) for D in qc.NORM_D for dtype in (F16, BF16) for mode in qc.NORM_MODES[dtype]]


@pytest.mark.parametrize("D,dtype,mode", NORM_PARAMS, ids=[f"D{D}-{'f16' if t == F16 else 'bf16'}-add{m}" for D, t, m in NORM_PARAMS])
def test_arithmetic_norm_scaled(lib, D, dtype, mode):
    pool = _Pool(dtype)
    for M in qc.NORM_M:
        x, _, _, w = qc.norm_inputs(M, D)
        wd = w.cuda()
        for sc in qc.NORM_SCALES:
            dl1, dl2 = qc.norm_deltas(M, D, sc)
            stored, ref = qc.norm_expected(x, dl1, dl2, w, mode, sc, dtype)
            for out_ld in qc.norm_pitches(D):
                what = f"M={M} D={D} out_ld={out_ld} add mode {mode} scales {sc}"
                rc, xb, ob = _norm(lib, x, dl1, dl2, wd, mode, sc, dtype, out_ld)
                assert rc == 0, what
                _same_bits(xb, Buf.of(stored), what + ": the stream (x + d1 delta1) + d2 delta2")
                assert ob.outside(D), what + ": a store behind column D or into a guard"
                out = ob.body[:, :D].cpu()
                assert bool(torch.isfinite(out.float()).all()), what
                pool.add(ref, out, what)
    pool.close(f"norm_f16s-D{D}-{'f16' if dtype == F16 else 'bf16'}-add{mode}")


@pytest.mark.parametrize("D", qc.NORM_D)
def test_identity_norm_unit_scales_are_the_unscaled_kernels(lib, D):
    from t2v_metrics_amd import engine
    for M in qc.NORM_M:
        x, _, _, w = qc.norm_inputs(M, D)
        wd = w.cuda()
        rc, xb, ob = _norm(lib, x, None, None, wd, 0, (1.0, 1.0, 1.0), F16, D)
        assert rc == 0
        plain = engine.norm16(0, x.cuda(), None, wd, types=1, eps=qc.NORM_EPS)
        assert torch.equal(ob.body.view(torch.int16), plain.view(torch.int16)), f"M={M} D={D}: fp16 form against vqs_debug_norm16 types 1"
        rc, xb, ob = _norm(lib, x, None, None, wd, 0, (1.0, 1.0, 1.0), BF16, D)
        assert rc == 0
        plain = engine.rmsnorm(x.cuda(), wd, qc.NORM_EPS)
        assert torch.equal(ob.body.view(torch.int16), plain.view(torch.int16)), f"M={M} D={D}: bf16 form against vqs_rmsnorm"
        _same_bits(xb, Buf.of(x), "a plain norm leaves the stream alone")


@pytest.mark.parametrize("D", qc.NORM_D)
def test_identity_norm_power_of_two_scales_commute_with_the_rounding(lib, D):
    M, k = 7, 3
    x, _, _, w = qc.norm_inputs(M, D)
    wd = w.cuda()
    dl1, dl2 = qc.norm_deltas(M, D, (1.0, 1.0, 1.0))
    up1, up2 = (dl1.float() * 2.0 ** k).to(F16), (dl2.float() * 2.0 ** k).to(F16)
    assert torch.equal(up1.float(), dl1.float() * 2.0 ** k) and torch.equal(up2.float(), dl2.float() * 2.0 ** k)      # delta 2^k is exact in fp16
    for dtype in (F16, BF16):
        for mode in qc.NORM_MODES[dtype]:
            if mode == 0:
                continue
            rc0, x0, o0 = _norm(lib, x, dl1, dl2, wd, mode, (1.0, 1.0, 1.0), dtype, D)
            rc1, x1, o1 = _norm(lib, x, up1, up2, wd, mode, (2.0 ** -k, 2.0 ** -k, 1.0), dtype, D)
            assert rc0 == 0 and rc1 == 0
            _same_bits(x1, x0, f"D={D} add mode {mode}: the stream under deltas stored as delta 2^{k}")
            _same_bits(o1, o0, f"D={D} add mode {mode}: the operand under deltas stored as delta 2^{k}")
    for so in (2.0 ** -6, 0.25, 8.0):
        rc0, _, o0 = _norm(lib, x, dl1, dl2, wd, 3, (1.0, 1.0, 1.0), F16, D)
        rc1, _, o1 = _norm(lib, x, dl1, dl2, wd, 3, (1.0, 1.0, so), F16, D)
        assert rc0 == 0 and rc1 == 0
        a, b = o0.body.float() * so, o1.body.float()
        normal = (a.abs() >= 2.0 ** -14) & (a.abs() <= 65504.0) & (o0.body.float().abs() >= 2.0 ** -14)
        assert int(normal.sum()) > 0.9 * a.numel() and torch.equal(a[normal], b[normal]), f"D={D}: operand under out = {so}"


def test_norm_unstored_form_keeps_the_stream_and_has_no_bf16_operand(lib):
    for D in qc.NORM_D:
        x, _, _, w = qc.norm_inputs(7, D)
        dl1, dl2 = qc.norm_deltas(7, D, (4.0, 0.5, 0.25))
        rc, xb, ob = _norm(lib, x, dl1, dl2, w.cuda(), 2, (4.0, 0.5, 0.25), F16, D)
        assert rc == 0
        _same_bits(xb, Buf.of(x), f"D={D}: add mode 2 must not write the stream")
        rc, xb, ob = _norm(lib, x, dl1, dl2, w.cuda(), 2, (4.0, 0.5, 0.25), BF16, D)
        assert rc == INVALID
        _same_bits(xb, Buf.of(x), "refused")
        assert ob.outside(0), "a refused launch wrote the operand"
    x, _, _, w = qc.norm_inputs(7, 200)
    for D, out_ld in ((200, 196), (200, 202), (198, 200)):          # a pitch below D, a pitch off the 4-element grid, D % 4
        xb, ob = Buf.of(x, device="cuda"), Buf(7, 512, F16, "cuda")
        assert lib.vqs_debug_rmsnorm_f16s(xb.ptr(), None, None, 1, w.cuda().data_ptr(), ob.ptr(), out_ld, 7, D, qc.NORM_EPS, 1.0, 1.0, 1.0, 0, _st()) == INVALID
        torch.cuda.synchronize()
        assert ob.outside(0)


# ---------------------------------------------------------------------------------------------------- rope_qk
def _rope_qk(lib, q, k, cos, sin, half, f16=None):
    B, Hq, S, hd = q.shape
    qb, kb = Buf.of(q.reshape(-1, hd), device="cuda"), Buf.of(k.reshape(-1, hd), device="cuda")
    cd, sd = cos.cuda(), sin.cuda()
    rc = lib.vqs_debug_rope_qk(qb.ptr(), kb.ptr(), cd.data_ptr(), sd.data_ptr(), B, Hq, k.shape[1], S, hd, half,
                               (1 if q.dtype == F16 else 0) if f16 is None else f16, _st())
    torch.cuda.synchronize()
    return rc, qb, kb


def _vqs_rope(lib, x, cos, sin, half):
    B, H, S, hd = x.shape
    xb, cd, sd = Buf.of(x.reshape(-1, hd), device="cuda"), cos.cuda(), sin.cuda()
    assert lib.vqs_rope(xb.ptr(), cd.data_ptr(), sd.data_ptr(), B, H, S, hd, half, _st()) == 0
    torch.cuda.synchronize()
    return xb


ROPE_PARAMS = [(hq, hk, hd, half, t) for hq, hk in qc.ROPE_HEADS for hd, half in qc.ROPE_LANES for t in (F16, BF16)]
ROPE_IDS = [f"q{a}k{b}-hd{c}-half{d}-{'f16' if t == F16 else 'bf16'}" for a, b, c, d, t in ROPE_PARAMS]


@pytest.mark.parametrize("Hq,Hk,hd,half,dtype", ROPE_PARAMS, ids=ROPE_IDS)
def test_exact_rope_qk(lib, Hq, Hk, hd, half, dtype):
    for S in qc.ROPE_S:
        q, k, cos, sin = qc.rope_inputs(Hq, Hk, S, hd, half, dtype, True)
        eq, ek = qc.rope_qk_expected(q, k, cos, sin, half)
        rc, qb, kb = _rope_qk(lib, q, k, cos, sin, half)
        what = f"Hq={Hq} Hk={Hk} S={S} hd={hd} half={half} {dtype}"
        assert rc == 0, what
        _same_bits(qb, Buf.of(eq.reshape(-1, hd)), what + ": q")
        _same_bits(kb, Buf.of(ek.reshape(-1, hd)), what + ": k")


@pytest.mark.parametrize("Hq,Hk,hd,half,dtype", ROPE_PARAMS, ids=ROPE_IDS)
def test_arithmetic_rope_qk(lib, Hq, Hk, hd, half, dtype):
    pool = _Pool(dtype)
    for scale in ((1.0, 2.0 ** -5) if dtype == F16 else (1.0,)):
        for S in qc.ROPE_S:
            q, k, cos, sin = qc.rope_inputs(Hq, Hk, S, hd, half, dtype, False, scale=scale)
            rq, rk = qc.rope_qk_expected(q, k, cos, sin, half)
            rc, qb, kb = _rope_qk(lib, q, k, cos, sin, half)
            what = f"Hq={Hq} Hk={Hk} S={S} hd={hd} half={half} {dtype} scale {scale}"
            assert rc == 0, what
            for name, x, ref, buf in (("q", q, rq, qb), ("k", k, rk, kb)):
                got = buf.body.cpu().view(x.shape)
                assert torch.equal(got[..., 2 * half:].contiguous().view(torch.int16), x[..., 2 * half:].contiguous().view(torch.int16)), what + ": lanes >= 2 half of " + name
                _same_bits(buf, Buf.of(got.reshape(-1, hd)), what + ": guards of " + name)
                pool.add(ref[..., :2 * half], got[..., :2 * half], what + ": " + name)
    pool.close(f"rope_qk-q{Hq}k{Hk}-hd{hd}-half{half}-{'f16' if dtype == F16 else 'bf16'}")


@pytest.mark.parametrize("Hq,Hk", qc.ROPE_HEADS)
@pytest.mark.parametrize("hd,half", qc.ROPE_LANES)
def test_identity_rope_qk_bf16_is_vqs_rope_on_q_and_on_k(lib, Hq, Hk, hd, half):
    for S in qc.ROPE_S:
        q, k, cos, sin = qc.rope_inputs(Hq, Hk, S, hd, half, BF16, False)
        rc, qb, kb = _rope_qk(lib, q, k, cos, sin, half)
        assert rc == 0
        _same_bits(qb, _vqs_rope(lib, q, cos, sin, half), f"q: Hq={Hq} S={S} hd={hd} half={half}")
        _same_bits(kb, _vqs_rope(lib, k, cos, sin, half), f"k: Hk={Hk} S={S} hd={hd} half={half}")


def test_rope_qk_fallback_and_refusals(lib):
    """half = 36 is off the 16-byte grid: bf16 takes two launches of vqs_rope's kernel, fp16 has no such form"""
    for exact in (True, False):
        q, k, cos, sin = qc.rope_inputs(4, 2, 33, 128, 36, BF16, exact)
        rc, qb, kb = _rope_qk(lib, q, k, cos, sin, 36)
        assert rc == 0
        _same_bits(qb, _vqs_rope(lib, q, cos, sin, 36), "fallback q")
        _same_bits(kb, _vqs_rope(lib, k, cos, sin, 36), "fallback k")
        if exact:
            eq, ek = qc.rope_qk_expected(q, k, cos, sin, 36)
            _same_bits(qb, Buf.of(eq.reshape(-1, 128)), "fallback q against the expectation")
            _same_bits(kb, Buf.of(ek.reshape(-1, 128)), "fallback k against the expectation")
    q, k, cos, sin = qc.rope_inputs(4, 2, 33, 128, 36, F16, True)
    for what, qq, kk, half in (("fp16 with half = 36", q, k, 36), ("an odd half", q.to(BF16), k.to(BF16), 35), ("2 half > hd", q.to(BF16), k.to(BF16), 72)):
        c = torch.zeros(2 * 33, half)
        rc, qb, kb = _rope_qk(lib, qq, kk, c, c, half)
        assert rc == INVALID, what
        _same_bits(qb, Buf.of(qq.reshape(-1, 128)), what)
        _same_bits(kb, Buf.of(kk.reshape(-1, 128)), what)


# ---------------------------------------------------------------------------------------------------- tail_rope_q
def _tail_rope(lib, qkv, ld, cos, sin, row, Hq, hd, half):
    B = qkv.shape[0]
    ob = Buf(B, Hq * hd, torch.float32, "cuda")
    qd, cd, sd, rd = qkv.cuda(), cos.cuda(), sin.cuda(), row.cuda()
    rc = lib.vqs_debug_qwen_tail_rope_q(qd.data_ptr(), ld, cd.data_ptr(), sd.data_ptr(), rd.data_ptr(), ob.ptr(), B, Hq, hd, half, _st())
    torch.cuda.synchronize()
    return rc, ob


@pytest.mark.parametrize("hd,half", qc.ROPE_LANES)
def test_exact_and_arithmetic_tail_rope_q(lib, hd, half):
    worst = 0.0
    for Hq in sorted({h for h, _ in qc.ROPE_HEADS}):
        qkv, ld, cos, sin, row = qc.tail_rope_inputs(Hq, hd, half, True)
        rc, ob = _tail_rope(lib, qkv, ld, cos, sin, row, Hq, hd, half)
        assert rc == 0
        _same_bits(ob, Buf.of(qc.tail_rope_expected(qkv, cos, sin, row, Hq, hd, half)[0].float()), f"exact: Hq={Hq} hd={hd} half={half}")
        qkv, ld, cos, sin, row = qc.tail_rope_inputs(Hq, hd, half, False)
        rc, ob = _tail_rope(lib, qkv, ld, cos, sin, row, Hq, hd, half)
        assert rc == 0 and ob.outside(Hq * hd)
        ref, mag = qc.tail_rope_expected(qkv, cos, sin, row, Hq, hd, half)
        err = (ob.body.cpu().double() - ref).abs()
        assert bool((err <= qc.TAIL_ROPE_BOUND * mag).all()), f"Hq={Hq} hd={hd} half={half}: {float((err / (mag + 1e-300)).max()) * 2 ** 24:.3f} x 2^-24"
        worst = max(worst, float((err[mag > 0] / mag[mag > 0]).max()) * 2.0 ** 24)
    print(f"tail_rope_q hd={hd} half={half}: worst |out - ref| / (|a c| + |b s|) = {worst:.4f} x 2^-24 (bound 3)")
    _record(f"qwen_glue/tail_rope_q-hd{hd}-half{half}", {"worst_over_2^-24_of_terms": worst, "bound": 3.0})


def test_tail_rope_q_refusals(lib):
    qkv, ld, cos, sin, row = qc.tail_rope_inputs(2, 256, 64, True)
    wide = torch.zeros(cos.shape[0], 72)
    for what, args in (("half > 64", (wide, wide, row, 2, 256, 72)), ("2 half > hd", (cos, sin, row, 4, 64, 64)), ("ld < Hq hd", (cos, sin, row, 4, 256, 64))):
        rc, ob = _tail_rope(lib, qkv, ld, *args)
        assert rc == INVALID and ob.outside(0), what


# ---------------------------------------------------------------------------------------------------- gathers, embed, fp16 -> bf16
@pytest.mark.parametrize("name", [c[0] for c in qc.GATHER_ROWS_CASES])
def test_exact_gather_rows_bf16(lib, name):
    src0, src1, rmap, rows, cols, src_ld, dst_ld = qc.gather_rows_inputs(name)
    s0, s1, md = src0.cuda(), None if src1 is None else src1.cuda(), None if rmap is None else rmap.cuda()
    db = Buf(rows, dst_ld, BF16, "cuda")
    assert lib.vqs_debug_gather_rows_bf16(s0.data_ptr(), _p(s1), _p(md), db.ptr(), rows, cols, src_ld, dst_ld, _st()) == 0
    torch.cuda.synchronize()
    _same_bits(db, Buf.of(qc.gather_rows_expected(src0, src1, rmap, cols, dst_ld)), name)


def test_gather_refusals_write_nothing(lib):
    src0, src1, rmap, rows, cols, src_ld, dst_ld = qc.gather_rows_inputs("heads-pad")
    s0, md, db = src0.cuda(), rmap.cuda(), Buf(rows, dst_ld, BF16, "cuda")
    for what, a in (("no source", (None, None, md.data_ptr(), db.ptr(), rows, cols, src_ld, dst_ld)), ("no destination", (s0.data_ptr(), None, None, None, rows, cols, src_ld, dst_ld)),
                    ("rows = 0", (s0.data_ptr(), None, md.data_ptr(), db.ptr(), 0, cols, src_ld, dst_ld)), ("cols = 0", (s0.data_ptr(), None, md.data_ptr(), db.ptr(), rows, 0, src_ld, dst_ld)),
                    ("dst_ld < cols", (s0.data_ptr(), None, md.data_ptr(), db.ptr(), rows, cols, src_ld, cols - 1))):
        assert lib.vqs_debug_gather_rows_bf16(*a, _st()) == INVALID, what
    assert lib.vqs_debug_gather_cols_bf16(s0.data_ptr(), None, db.ptr(), rows, src_ld, cols, _st()) == INVALID
    assert lib.vqs_debug_gather_cols_bf16(s0.data_ptr(), md.data_ptr(), db.ptr(), 0, src_ld, cols, _st()) == INVALID
    assert lib.vqs_debug_gather_cols_bf16(s0.data_ptr(), md.data_ptr(), db.ptr(), rows, src_ld, 0, _st()) == INVALID
    f = torch.zeros(8, 64, device="cuda")
    for a in ((8, 64, 64, 2), (8, 62, 62, 0), (8, 62, 64, 1), (8, 64, 60, 1), (0, 64, 64, 0), (8, 64, 68, 0)):
        assert lib.vqs_debug_gather_rows_f32(f.data_ptr(), md.data_ptr(), db.ptr(), *a, _st()) == INVALID, a
    torch.cuda.synchronize()
    assert db.outside(0)


@pytest.mark.parametrize("direction", ["spread", "compact"])
def test_exact_gather_cols_bf16(lib, direction):
    src, cmap, rows, src_ld, dst_cols = qc.gather_cols_inputs(direction)
    sd, cd, db = src.cuda(), cmap.cuda(), Buf(rows, dst_cols, BF16, "cuda")
    assert lib.vqs_debug_gather_cols_bf16(sd.data_ptr(), cd.data_ptr(), db.ptr(), rows, src_ld, dst_cols, _st()) == 0
    torch.cuda.synchronize()
    _same_bits(db, Buf.of(qc.gather_cols_expected(src, cmap)), direction)


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("D", qc.GATHER_F32_D)
def test_exact_gather_rows_f32(lib, D, form):
    src, rmap, rows, src_ld = qc.gather_f32_inputs(D, form)
    sd, md, db = src.cuda(), rmap.cuda(), Buf(rows, D, torch.float32, "cuda")
    assert lib.vqs_debug_gather_rows_f32(sd.data_ptr(), md.data_ptr(), db.ptr(), rows, D, src_ld, form, _st()) == 0
    torch.cuda.synchronize()
    _same_bits(db, Buf.of(qc.gather_f32_expected(src, rmap, D)), f"D={D} form {form}")


@pytest.mark.parametrize("D", qc.EMBED_D)
@pytest.mark.parametrize("merged_f16", [False, True], ids=["merged-bf16", "merged-f16"])
def test_exact_qwen_embed(lib, D, merged_f16):
    ids, vis, embed, merged, rows = qc.embed_inputs(D, merged_f16)
    idd, vd, ed, md = ids.cuda(), vis.cuda(), embed.cuda(), merged.cuda()
    for unscale in ((1.0, 2.0, 32.0) if merged_f16 else (1.0, 2.0)):        # the bf16 path ignores the factor
        ob = Buf(rows, D, torch.float32, "cuda")
        assert lib.vqs_debug_qwen_embed(idd.data_ptr(), vd.data_ptr(), ed.data_ptr(), md.data_ptr(), ob.ptr(), rows, D, qc.EMBED_VOCAB, 1 if merged_f16 else 0, unscale,
                                        _st()) == 0
        torch.cuda.synchronize()
        _same_bits(ob, Buf.of(qc.embed_expected(ids, vis, embed, merged, unscale)), f"D={D} unscale {unscale}")
    ob = Buf(rows, D, torch.float32, "cuda")
    assert lib.vqs_debug_qwen_embed(idd.data_ptr(), None, ed.data_ptr(), md.data_ptr(), ob.ptr(), rows, D, qc.EMBED_VOCAB, 0, 1.0, _st()) == INVALID
    assert lib.vqs_debug_qwen_embed(idd.data_ptr(), vd.data_ptr(), ed.data_ptr(), md.data_ptr(), ob.ptr(), 0, D, qc.EMBED_VOCAB, 0, 1.0, _st()) == INVALID
    torch.cuda.synchronize()
    assert ob.outside(0)


def _f16_rows(lib, src, rows, cols, src_ld, dst_ld, unscale):
    sd, db = src.cuda(), Buf(rows, dst_ld, BF16, "cuda")
    rc = lib.vqs_debug_f16_to_bf16_rows(sd.data_ptr(), db.ptr(), rows, cols, src_ld, dst_ld, unscale, _st())
    torch.cuda.synchronize()
    return rc, db


@pytest.mark.parametrize("cols", qc.F16_COLS)
def test_exact_f16_to_bf16_rows(lib, cols):
    src, src_ld = qc.f16_rows_inputs(cols)
    for unscale, dst_ld in ((1.0, cols), (2.0 ** -5, cols + 40), (8.0, cols + 8), (3.0, cols + 40)):
        rc, db = _f16_rows(lib, src, src.shape[0], cols, src_ld, dst_ld, unscale)
        assert rc == 0
        want = Buf(src.shape[0], dst_ld, BF16)
        want.body[:, :cols] = qc.f16_rows_expected(src, cols, unscale)            # nothing between a row's cols and the next row
        _same_bits(db, want, f"cols={cols} dst_ld={dst_ld} unscale {unscale}")


def test_exact_f16_to_bf16_rows_grid_stride(lib):
    cols = qc.F16_COLS_STRIDE
    src, src_ld = qc.f16_rows_inputs(cols, rows=2)
    rc, db = _f16_rows(lib, src, 2, cols, src_ld, cols + 8, 0.5)
    assert rc == 0
    want = Buf(2, cols + 8, BF16)
    want.body[:, :cols] = qc.f16_rows_expected(src, cols, 0.5)
    _same_bits(db, want, "the grid-stride loop's second step")


def test_f16_to_bf16_rows_refusals(lib):
    src, src_ld = qc.f16_rows_inputs(2040)
    for what, rows, cols, dl in (("cols % 8", 5, 2036, 2048), ("rows = 0", 0, 2040, 2048), ("dst_ld < cols", 5, 2040, 2032)):
        rc, db = _f16_rows(lib, src, rows, cols, src_ld, dl, 1.0)
        assert rc == INVALID and db.outside(0), what
    sd, db = src.cuda(), Buf(5, 2048, BF16, "cuda")
    assert lib.vqs_debug_f16_to_bf16_rows(sd.data_ptr(), db.ptr(), 65536, 2040, src_ld, 2048, 1.0, _st()) == INVALID        # rows > 65535: the grid's y limit
    torch.cuda.synchronize()
    assert db.outside(0)


# ---------------------------------------------------------------------------------------------------- range proof
def _slot(bits_or_value=0.0):
    b = Buf(1, 1, torch.float32, "cuda")
    if isinstance(bits_or_value, int):
        b.body.view(torch.int32)[0, 0] = bits_or_value
    else:
        b.body[0, 0] = bits_or_value
    return b


def _slot_bits(b):
    assert b.outside(1), "a store next to the slot"
    return int(b.body.view(torch.int32).cpu()[0, 0]) & 0xFFFFFFFF


def _f32_bits(v):
    return int(torch.tensor(float(v), dtype=torch.float32).view(torch.int32)) & 0xFFFFFFFF


def _absmax(lib, x, R, slot):
    xd = x.cuda()
    rc = lib.vqs_debug_absmax_bf16(xd.data_ptr(), x.numel(), R, slot.ptr(), _st())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("n", qc.ABSMAX_N)
def test_exact_absmax(lib, n):
    x = qc.absmax_inputs(n)
    want = _f32_bits(qc.absmax_expected(x, qc.ABSMAX_R))
    for _ in range(2):
        s = _slot(0.0)
        assert _absmax(lib, x, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == want, n
    s = _slot(1.0e6)                                                  # a slot seeded larger stays
    assert _absmax(lib, x, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == _f32_bits(1.0e6)
    s = _slot(1.0)                                                    # ... and one seeded smaller is raised
    assert _absmax(lib, x, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == want
    inf, nan = x.clone(), x.clone()
    inf[n // 2], nan[n // 3] = float("-inf"), float("nan")
    s = _slot(0.0)
    assert _absmax(lib, inf, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == _f32_bits(float("inf"))
    assert _absmax(lib, nan, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == NAN_SLOT      # NaN after inf
    assert _absmax(lib, inf, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == NAN_SLOT      # inf after NaN: the NaN pattern is the larger one and stays
    assert _absmax(lib, x, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == NAN_SLOT
    s = _slot(0.0)
    assert _absmax(lib, nan, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == NAN_SLOT
    both = inf.clone()
    both[n // 3] = float("nan")
    s = _slot(0.0)
    assert _absmax(lib, both, qc.ABSMAX_R, s) == 0 and _slot_bits(s) == NAN_SLOT                 # both in one launch


def test_absmax_and_gate_pair_refusals(lib):
    x, s = qc.absmax_inputs(256).cuda(), _slot(0.0)
    assert lib.vqs_debug_absmax_bf16(None, 256, 1.0, s.ptr(), _st()) == INVALID and lib.vqs_debug_absmax_bf16(x.data_ptr(), 0, 1.0, s.ptr(), _st()) == INVALID
    assert lib.vqs_debug_absmax_bf16(x.data_ptr(), 256, 1.0, None, _st()) == INVALID
    rb, ub = qc.gate_pair_inputs(96).cuda(), Buf(1, 128, torch.float32, "cuda")
    assert lib.vqs_debug_gate_pair_bound(rb.data_ptr(), 80, 128, ub.ptr(), s.ptr(), _st()) == INVALID           # mlp_p % 32
    assert lib.vqs_debug_gate_pair_bound(rb.data_ptr(), 96, 64, ub.ptr(), s.ptr(), _st()) == INVALID            # ld < mlp_p
    assert lib.vqs_debug_gate_pair_bound(None, 96, 128, ub.ptr(), s.ptr(), _st()) == INVALID
    torch.cuda.synchronize()
    assert ub.outside(0) and _slot_bits(s) == 0


@pytest.mark.parametrize("mlp_p", [32, 96])
def test_exact_gate_pair_bound(lib, mlp_p):
    rb = qc.gate_pair_inputs(mlp_p)
    for ld in (mlp_p, mlp_p + 32):
        want = qc.gate_pair_expected(rb, mlp_p, ld)
        rd, ub, s = rb.cuda(), Buf(1, ld, torch.float32, "cuda"), _slot(0.0)
        assert lib.vqs_debug_gate_pair_bound(rd.data_ptr(), mlp_p, ld, ub.ptr(), s.ptr(), _st()) == 0
        torch.cuda.synchronize()
        _same_bits(ub, Buf.of(want[None, :]), f"mlp_p={mlp_p} ld={ld}")
        assert _slot_bits(s) == _f32_bits(want.max())
        bad = rb.clone()
        bad[mlp_p // 2] = float("nan")
        s2 = _slot(0.0)
        assert lib.vqs_debug_gate_pair_bound(bad.cuda().data_ptr(), mlp_p, ld, ub.ptr(), s2.ptr(), _st()) == 0
        torch.cuda.synchronize()
        assert _slot_bits(s2) == NAN_SLOT


def _rowbound(lib, W, K, mode, g, g_len, R, u, uconst, bias, want_out=True, slot=None):
    N = W.shape[0]
    Wd, gd, ud, bd = W.cuda(), None if g is None else g.cuda(), None if u is None else u.cuda(), None if bias is None else bias.cuda()
    uc = None if uconst is None else torch.tensor([uconst], dtype=torch.float32, device="cuda")
    ob, s = Buf(1, N, torch.float32, "cuda"), slot or _slot(0.0)
    rc = lib.vqs_debug_rowbound(Wd.data_ptr(), W.shape[1], N, K, mode, _p(gd), g_len, R, _p(ud), _p(uc), _p(bd), ob.ptr() if want_out else None, s.ptr(), _st())
    torch.cuda.synchronize()
    return rc, ob, s


ROWBOUND_FORMS = (("g", 0), ("g-wrap", 0), ("u", 1), ("uconst", 1))


def _rowbound_args(form, K, g, u, R):
    return {"g": (g, K, R, None, None), "g-wrap": (g, K // 4, R, None, None), "u": (None, 0, 0.0, u, None), "uconst": (None, 0, 0.0, None, 1.5)}[form]


@pytest.mark.parametrize("K", qc.ROWBOUND_K)
@pytest.mark.parametrize("form,mode", ROWBOUND_FORMS)
def test_exact_rowbound(lib, K, form, mode):
    for N in qc.ROWBOUND_N:
        W, g, u, bias = qc.rowbound_inputs(N, K, True)
        args = _rowbound_args(form, K, g, u, qc.ROWBOUND_R_EXACT)
        for b in (bias, None):
            want = qc.rowbound_expected_exact(W, K, mode, *args, b)                         # exact sums; the square root and the bias add round once each
            what = f"N={N} K={K} {form} bias {b is not None}"
            rc, ob, s = _rowbound(lib, W, K, mode, *args, b)
            assert rc == 0, what
            _same_bits(ob, Buf.of(want[None, :]), what)
            assert _slot_bits(s) == _f32_bits(want.max()), what + ": the slot is the maximum of out"
            rc, ob, s = _rowbound(lib, W, K, mode, *args, b, want_out=False)               # out == NULL: the slot alone
            assert rc == 0 and ob.outside(0) and _slot_bits(s) == _f32_bits(want.max()), what + ": out == NULL"
        rc, ob, s = _rowbound(lib, W, K, mode, *args, bias, slot=_slot(1.0e9))
        assert rc == 0 and _slot_bits(s) == _f32_bits(1.0e9)
        bad = W.clone()
        bad[N - 1, K - 1] = float("nan")
        rc, ob, s = _rowbound(lib, bad, K, mode, *args, bias)
        assert rc == 0 and _slot_bits(s) == NAN_SLOT, what + ": a NaN weight poisons the slot"
        pad = W.clone()
        pad[:, K:] = float("nan")                                                           # the columns behind K are not read
        rc, ob, s = _rowbound(lib, pad, K, mode, *args, bias)
        assert rc == 0 and _slot_bits(s) == _f32_bits(qc.rowbound_expected_exact(W, K, mode, *args, bias).max()), what + ": ldw > K"


@pytest.mark.parametrize("K", qc.ROWBOUND_ARITH_K)
@pytest.mark.parametrize("form,mode", ROWBOUND_FORMS)
def test_arithmetic_rowbound(lib, K, form, mode):
    W, g, u, bias = qc.rowbound_inputs(qc.ROWBOUND_ARITH_N, K, False)
    args = _rowbound_args(form, K, g, u, float(torch.tensor(float(K)).sqrt()))
    ref = qc.rowbound_expected(W, K, mode, *args, bias)
    rc, ob, s = _rowbound(lib, W, K, mode, *args, bias)
    assert rc == 0 and ob.outside(qc.ROWBOUND_ARITH_N)
    out = ob.body[0].cpu().double()
    rel, over = float(((out - ref).abs() / ref).max()), float((out / ref).max())
    print(f"rowbound K={K} {form}: max |out - ref| / ref = {rel * 2 ** 24:.2f} x 2^-24 (bound {K + 16}), max out / ref = 1 + {(over - 1) * 2 ** 24:.2f} x 2^-24 (head room 512.02)")
    _record(f"qwen_glue/rowbound-K{K}-{form}", {"max_rel_err_over_2^-24": rel * 2 ** 24, "bound_over_2^-24": K + 16, "max_out_over_ref_minus_1_over_2^-24": (over - 1) * 2 ** 24})
    assert bool(((out - ref).abs() <= qc.rowbound_bound(K) * ref).all()), (K, form, rel)
    assert bool((out <= qc.ROWBOUND_HEADROOM * ref).all()), (K, form, over)
    assert _slot_bits(s) == _f32_bits(ob.body[0].max()), "the slot is the maximum of out"


def test_rowbound_refusals(lib):
    W, g, u, bias = qc.rowbound_inputs(5, 64, True)
    for what, a in (("mode 0 without g", (0, None, 64, 2.0, None, None)), ("g_len = 0", (0, g, 0, 2.0, None, None)), ("mode 1 without u and uconst", (1, None, 0, 0.0, None, None)),
                    ("no such mode", (2, g, 64, 2.0, u, None))):
        rc, ob, s = _rowbound(lib, W, 64, *a, bias)
        assert rc == INVALID and ob.outside(0) and _slot_bits(s) == 0, what
    rc, ob, s = _rowbound(lib, W, 80, 1, None, 0, 0.0, None, 1.5, bias)                      # ldw = 72 < K
    assert rc == INVALID and ob.outside(0) and _slot_bits(s) == 0
