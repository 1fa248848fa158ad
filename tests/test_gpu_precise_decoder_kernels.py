"""The precise decoder's glue, the split-K reductions, the decoder attentions and the greedy / score tail on their own (include/vqs_debug.h
test hooks; csrc/elementwise.hip, csrc/attn.hip): rmsnorm_split, sum_planes (fp32 / split / gated split / fp16, with and without the
Qwen2.5-VL tail's bias + SiLU forms), reduce_slices, reduce_slices_act, masked_softmax, transpose_pad, argmax_append, dec_self_attn_precise,
dec_attn (self, cross, cached) and the score head -- one launch each on caller tensors, against the float64 restatements of
tests/precise_decoder_ref.py computed from the exact values of the stored inputs (held to the oracles by
tests/test_precise_decoder_reference.py).  Shapes are the smallest that reach each edge: rows no multiple of the rows per block, row
lengths around the 64 lanes and the 256 threads, row pitches / plane offsets / slice strides wider than the data with NaN in the gaps,
sentinel guard rows around every output plane, every mode and slice count.

Criteria (tests/precise_decoder_ref.py), none taken from the kernels' results: fp32 out: 2e-5 max|ref_row|; split-bf16 out: the same for
hi + lo, and |lo| <= 0.5 ulp_bf16(hi); one 16-bit rounding: 0.5 ulp16(ref) + 2e-5 max|ref_row|; transpose / argmax / the slice order of the
reductions: exact.  The kernels that use the hardware exp / rcp (gated sum_planes in both activations, gated reduce_slices_act,
masked_softmax, both decoder attentions) get (1 + allow) times the fp32 term.  allow is meant to be 4 x the worst error left after the
output's own rounding, measured on an MI355X in units of that term (the `excess` figure every case records).  UNMEASURED on MI355X so
far: each allowance stands at the largest value under its cap -- the total bound of a split
output below 2^-12 of the row maximum (a lost lo plane costs 2^-9), that of a 16-bit output below 1.5 ulp at the row maximum -- and the
caps are the only limits (profiles/precise_decoder_kernels.md says how to replace them by measured ones).  Without a GPU every case of
this file runs over an fp32 CPU restatement of the kernels, and over seven mutated copies of it (tests/test_precise_decoder_restatement.py).
Each case's worst error-to-bound ratio goes to the suite's parity_e2e.jsonl record (tests/test_gpu_e2e.py) under precise_decoder_kernels/."""
import pytest
import torch

from tests import precise_decoder_ref as R
from tests.test_gpu_e2e import _record

pytestmark = pytest.mark.gpu

INVALID = -1
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
GUARD = 2                                  # guard rows before, between and after output planes
# allowances of the kernels that use the hardware exp / rcp, in units of the fp32 term.  UNMEASURED: the largest under each cap (module docstring)
_SPLIT_CAP, _BF16_CAP, _F16_CAP = 11.0, 194.0, 23.0
ALLOW = {"gated_gelu": _SPLIT_CAP, "gated_silu": _SPLIT_CAP, "dec_precise": _SPLIT_CAP, "reduce_act_gated": _BF16_CAP, "dec_attn": _BF16_CAP,
         "masked_softmax_bf16": _BF16_CAP, "masked_softmax_f16": _F16_CAP}


def test_allowances_stay_under_their_caps():
    for name, kind in [("gated_gelu", "split"), ("gated_silu", "split"), ("dec_precise", "split"), ("reduce_act_gated", "bf16"),
                       ("dec_attn", "bf16"), ("masked_softmax_bf16", "bf16"), ("masked_softmax_f16", "f16")]:
        assert R.allowance_caps_hold(ALLOW[name], kind), (name, kind)


def _lib():
    from t2v_metrics_amd import engine
    return engine.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rec(case, **kw):
    _record("precise_decoder_kernels/" + case, kw)
    print(case, kw)


def _bits16(t):
    return t.view(torch.int16)


def _nan16(*shape, f16=False):
    return torch.full(shape, R.F16_NAN if f16 else R.BF16_NAN, dtype=torch.int16).view(torch.float16 if f16 else torch.bfloat16)


def _nan32(*shape):
    return torch.full(shape, R.F32_NAN, dtype=torch.int32).view(torch.float32)


def _check_split(case, hi, lo, ref, allow=0.0, **kw):
    """hi, lo, ref: [rows, cols].  The inputs first: the correctly rounded reference meets the bound with a ratio below 0.5."""
    assert R.ratio_split(*R.split_bf16(ref), ref)[0] < 0.5, case
    r_sum, r_lo = R.ratio_split(hi, lo, ref, allow)
    _rec(case, worst_error_to_bound=r_sum, worst_lo_to_half_ulp=r_lo, excess=R.excess(hi.double() + lo.double(), ref), **kw)
    assert r_sum <= 1.0 and r_lo <= 1.0, (case, r_sum, r_lo)


def _check16(case, out, ref, bits=R.BF16_BITS, allow=0.0, **kw):
    rounded = ref.float().to(torch.bfloat16 if bits == R.BF16_BITS else torch.float16)
    assert R.ratio_16(rounded, ref, bits) < 1.0, case                  # the inputs: the correctly rounded reference is inside the bound
    r = R.ratio_16(out, ref, bits, allow)
    _rec(case, worst_error_to_bound=r, excess=R.excess(out, ref, bits), **kw)
    assert r <= 1.0, (case, r)


def _check32(case, out, ref, **kw):
    r = R.ratio_f32(out, ref)
    _rec(case, worst_error_to_bound=r, **kw)
    assert r <= 1.0, (case, r)


class _Planes:
    """An output of `planes` [rows, ld] planes (cols <= ld used) with GUARD sentinel rows before, between and after them; everything
    starts as the sentinel, so an element the kernel does not write is far off and one it must not write is detected bitwise."""

    def __init__(self, rows, cols, ld, planes, dtype=torch.bfloat16):
        self.rows, self.cols, self.ld, self.planes, self.dtype = rows, cols, ld, planes, dtype
        self.wide = dtype == torch.float32
        total = (planes * (rows + GUARD) + GUARD) * ld
        self.buf = torch.full((total,), SENT32 if self.wide else SENT16, dtype=torch.int32 if self.wide else torch.int16).cuda()
        self.plane = (rows + GUARD) * ld                        # elements between planes
        self.esize = 4 if self.wide else 2

    def ptr(self):
        return self.buf.data_ptr() + GUARD * self.ld * self.esize

    def read(self):
        """-> the planes [planes, rows, cols] (float64); asserts that nothing else changed."""
        torch.cuda.synchronize()
        raw = self.buf.cpu()
        grid = raw.view((self.planes * (self.rows + GUARD) + GUARD), self.ld)
        written = torch.zeros_like(grid, dtype=torch.bool)
        out = []
        for p in range(self.planes):
            r0 = GUARD + p * (self.rows + GUARD)
            written[r0:r0 + self.rows, :self.cols] = True
            out.append(grid[r0:r0 + self.rows, :self.cols].contiguous().view(self.dtype).double())
        assert (grid[~written] == (SENT32 if self.wide else SENT16)).all(), "a guard row or a pad column was written"
        return torch.stack(out)

    def untouched(self):
        torch.cuda.synchronize()
        return bool((self.buf == (SENT32 if self.wide else SENT16)).all())


# =====================================================================================================================================
# rmsnorm_split
# =====================================================================================================================================
def _rmsnorm_split(lib, x, delta, w, out, M, D, eps, out_plane=None):
    return lib.vqs_debug_rmsnorm_split(x.data_ptr(), None if delta is None else delta.data_ptr(), w.data_ptr(), out.ptr(),
                                       out.plane if out_plane is None else out_plane, M, D, eps, _stream())


@pytest.mark.parametrize("with_delta", [False, True])
@pytest.mark.parametrize("M,D", [(1, 4), (3, 100), (5, 256), (7, 260), (9, 2048), (6, 4096)])
def test_rmsnorm_split(M, D, with_delta):
    lib, eps = _lib(), 1e-6
    g = _gen(17 * M + D)
    x = 3.0 * torch.randn(M, D, generator=g) + 0.5
    delta = torch.randn(M, D, generator=g) if with_delta else None
    if M >= 3:
        x[1] *= 1.0e4                                         # magnitudes near 1e4
        x[2] = 0.0                                            # an all-zero row: exactly 0 out, not NaN
        if with_delta:
            delta[1] *= 1.0e3
            delta[2] = 0.0
    w = (1.0 + 0.5 * torch.randn(D, generator=g)).to(torch.bfloat16)
    xd, dd, wd = x.cuda(), None if delta is None else delta.cuda(), w.cuda()
    out = _Planes(M, D, D, 2)
    assert _rmsnorm_split(lib, xd, dd, wd, out, M, D, eps) == 0
    hi, lo = out.read()
    x_after = xd.cpu()
    stream = x.double() + (delta.double() if with_delta else 0.0)
    if with_delta:
        assert ((x_after.double() - stream).abs() <= 1e-6 * stream.abs()).all(), "stream != x + delta"
        assert torch.equal(dd.cpu(), delta)
    else:
        assert torch.equal(x_after.view(torch.int32), x.view(torch.int32)), "stream changed without a delta"
    _check32(f"rmsnorm_split/stream_M{M}_D{D}_delta{int(with_delta)}", x_after, stream)
    _check_split(f"rmsnorm_split/M{M}_D{D}_delta{int(with_delta)}", hi, lo, R.rmsnorm(stream, w, eps))
    if M >= 3:
        assert (hi[2] == 0).all() and (lo[2] == 0).all()


def test_rmsnorm_split_refusals():
    lib = _lib()
    x, w = torch.ones(4, 8).cuda(), torch.ones(8, dtype=torch.bfloat16).cuda()
    out = _Planes(4, 8, 8, 2)
    assert _rmsnorm_split(lib, x, None, w, out, 4, 6, 1e-6) == INVALID                 # D % 4
    assert _rmsnorm_split(lib, x, None, w, out, 4, 8, 1e-6, out_plane=8 * 6 + 2) == INVALID
    assert _rmsnorm_split(lib, x, None, w, out, 0, 8, 1e-6) == INVALID
    assert out.untouched() and (x.cpu() == 1).all()


# =====================================================================================================================================
# sum_planes / reduce_slices / reduce_slices_act
# =====================================================================================================================================
GATE_VALUES = [-30.0, -8.0, -1e-3, 0.0, 1e-3, 8.0, 30.0]
NSLICES = [1, 2, 7, 16]
SHAPES = [(1, 64), (3, 128), (5, 192), (17, 320)]
# ungated extras: cols 4 and 36, and rows * cols / 4 at 255, 256, 257 (the last thread of a block, a full block, one thread of the next)
UNGATED_EXTRA = [(3, 4), (5, 36), (15, 68), (16, 64), (1, 1028)]
GATED_EXTRA = [(32, 64)]                   # 32 rows x 8 groups = 256 threads exactly (gated thread counts are multiples of 8)


def _partials(target, nslices, planes, ldp, slice_stride, seed, relative=False):
    """A flat fp32 buffer of `nslices` slices of `planes` * rows rows of pitch ldp whose valid entries sum to `target` [rows, cols] (to fp32
    rounding: every piece but the first is uniform in +-0.25 -- times |target| of its element when `relative`, so that a tiny target is not
    the difference of large pieces -- and the first is the remainder), NaN everywhere else."""
    rows, cols = target.shape
    g = _gen(seed)
    pieces = 0.5 * torch.rand(nslices, planes, rows, cols, generator=g) - 0.25
    if relative:
        pieces = pieces * target.abs()
    pieces[0, 0] = (target.double() - pieces.double().sum(dim=(0, 1)) + pieces[0, 0].double()).float()
    buf = _nan32((nslices - 1) * slice_stride + planes * rows * ldp + 8)
    for k in range(nslices):
        for p in range(planes):
            base = k * slice_stride + p * rows * ldp
            idx = base + torch.arange(rows)[:, None] * ldp + torch.arange(cols)[None, :]
            buf[idx] = pieces[k, p]
    return buf


def _targets(rows, cols, gated, seed):
    t = 1.5 * torch.randn(rows, cols, generator=_gen(seed))
    if gated:                                                 # the gate values of both tails, in the last row's first gate columns
        t[rows - 1, :len(GATE_VALUES)] = torch.tensor(GATE_VALUES)
    return t


def _sum_planes_case(lib, mode, nslices, rows, cols, bias_on=False, silu=0, pad=4):
    gated = mode == 2
    ldp, out_cols = cols + pad, cols // 2 if gated else cols
    ld_out = out_cols + pad
    slice_stride = 2 * rows * ldp + 2 * pad
    seed = 1000 * mode + 100 * nslices + rows + cols + 7 * silu + 3 * bias_on
    part = _partials(_targets(rows, cols, gated, seed), nslices, 2, ldp, slice_stride, seed + 1)
    bias = (0.5 * torch.randn(cols, generator=_gen(seed + 2))).to(torch.bfloat16) if bias_on else None
    planes = 2 if mode in (1, 2) else 1
    out = _Planes(rows, out_cols, ld_out, planes, {0: torch.float32, 3: torch.float16}.get(mode, torch.bfloat16))
    pd, bd = part.cuda(), None if bias is None else bias.cuda()
    rc = lib.vqs_debug_sum_planes(pd.data_ptr(), nslices, slice_stride, rows, cols, ldp, mode, out.ptr(), ld_out, out.plane,
                                  None if bd is None else bd.data_ptr(), silu, _stream())
    assert rc == 0, rc
    got = out.read()
    y = R.sum_planes_y(part, nslices, slice_stride, rows, cols, ldp, bias)
    case = f"sum_planes/mode{mode}_k{nslices}_{rows}x{cols}_bias{int(bias_on)}_silu{silu}"
    if mode == 0:
        y32 = R.sum_planes_y(part, nslices, slice_stride, rows, cols, ldp, bias, dtype=torch.float32)
        assert torch.equal(got[0].float(), y32), "fp32 sums differ from the index-order sum: the slice order is the documented determinism"
        _check32(case, got[0], y)
    elif mode == 1:
        _check_split(case, got[0], got[1], y)
    elif mode == 2:
        tail = bias_on or silu
        _check_split(case, got[0], got[1], R.gated(y, R.silu if tail else R.gelu_new), ALLOW["gated_silu" if tail else "gated_gelu"])
    else:
        _check16(case, got[0], y, R.F16_BITS)


@pytest.mark.parametrize("nslices", NSLICES)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_sum_planes(mode, nslices):
    lib = _lib()
    for rows, cols in SHAPES + (GATED_EXTRA if mode == 2 else UNGATED_EXTRA):
        _sum_planes_case(lib, mode, nslices, rows, cols)
    assert any(c // 2 >= 68 for _, c in SHAPES)               # gated outputs reach columns 28-35 and 60-67: both 32 | 32 block boundaries


@pytest.mark.parametrize("bias_on,silu", [(True, 0), (False, 1), (True, 1)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_sum_planes_bias_and_silu_forms(mode, bias_on, silu):
    lib = _lib()
    for nslices in (1, 7):
        for rows, cols in SHAPES + (GATED_EXTRA if mode == 2 else UNGATED_EXTRA):
            _sum_planes_case(lib, mode, nslices, rows, cols, bias_on, silu)


def test_sum_planes_with_tight_pitches():
    """ldp == cols, ld_out == out_cols, slice_stride == 2 rows ldp: the engine's own layout."""
    lib = _lib()
    for mode in (0, 1, 2, 3):
        _sum_planes_case(lib, mode, 7, 5, 192, pad=0)


@pytest.mark.parametrize("silu", [0, 1])
def test_gated_activation_tails(silu):
    """Row i: every gate is GATE_VALUES[i] (jittered by 1e-3 relative), so each tail of rcp(1 + exp(-x)) / gelu_new is judged against its
    own row maximum; the reference is the exact function in float64."""
    lib, rows, cols, ns = _lib(), len(GATE_VALUES), 128, 2
    g = _gen(40 + silu)
    gate = torch.tensor(GATE_VALUES)[:, None] * (1.0 + 1e-3 * torch.randn(rows, cols // 2, generator=g))
    up = (0.5 + torch.rand(rows, cols // 2, generator=g)) * torch.where(torch.rand(rows, cols // 2, generator=g) < 0.5, -1.0, 1.0)
    part = _partials(R.pack_gate_up(gate, up), ns, 2, cols, 2 * rows * cols, 41, relative=True)
    out = _Planes(rows, cols // 2, cols // 2, 2)
    pd = part.cuda()
    assert lib.vqs_debug_sum_planes(pd.data_ptr(), ns, 2 * rows * cols, rows, cols, cols, 2, out.ptr(), cols // 2, out.plane, None, silu, _stream()) == 0
    hi, lo = out.read()
    y = R.sum_planes_y(part, ns, 2 * rows * cols, rows, cols, cols)
    _check_split(f"sum_planes/gate_tails_silu{silu}", hi, lo, R.gated(y, R.silu if silu else R.gelu_new), ALLOW["gated_silu" if silu else "gated_gelu"])
    # reduce_slices_act's gated form on the hi rows alone
    o2 = _Planes(rows, cols // 2, cols // 2, 1)
    if silu:
        assert lib.vqs_debug_reduce_slices_act(pd.data_ptr(), ns, 2 * rows * cols, rows, cols, cols, None, 1, o2.ptr(), cols // 2, _stream()) == 0
        y1 = R.reduce_slices_y(part, ns, 2 * rows * cols, rows, cols, cols)
        _check16("reduce_slices_act/gate_tails", o2.read()[0], R.gated(y1, R.silu), allow=ALLOW["reduce_act_gated"])


def test_sum_planes_refusals():
    lib = _lib()
    part = torch.zeros(4096).cuda()
    bias = torch.zeros(256, dtype=torch.bfloat16).cuda()
    out = _Planes(4, 64, 64, 2, torch.float32)

    def call(mode, cols=64, ldp=64, ld_out=64, out_plane=None, stride=512, b=None, silu=0, ns=2, rows=4):
        return lib.vqs_debug_sum_planes(part.data_ptr(), ns, stride, rows, cols, ldp, mode, out.ptr(), ld_out, out.plane if out_plane is None else out_plane,
                                        b, silu, _stream())
    assert call(3, b=bias.data_ptr()) == INVALID and call(3, silu=1) == INVALID          # SUM_F16 has no bias / SiLU form
    assert call(2, cols=96, ldp=96) == INVALID                                            # gated: cols % 64
    assert call(2, cols=32, ldp=32) == INVALID
    for mode in (0, 1, 2, 3):
        assert call(mode, ldp=66) == INVALID and call(mode, ld_out=66) == INVALID and call(mode, out_plane=out.plane + 2) == INVALID
        assert call(mode, stride=514) == INVALID and call(mode, ns=0) == INVALID and call(mode, rows=0) == INVALID
    assert call(0, cols=6) == INVALID and call(4) == INVALID and call(-1) == INVALID and call(4, silu=1) == INVALID
    assert out.untouched()


@pytest.mark.parametrize("nslices", NSLICES)
def test_reduce_slices(nslices):
    lib = _lib()
    for rows, cols in SHAPES + UNGATED_EXTRA:
        n = rows * cols
        part = _partials(_targets(rows, cols, False, n + nslices), nslices, 1, cols, n, n + nslices + 1)[:nslices * n].contiguous()
        out = _Planes(1, n, n, 1)
        pd = part.cuda()
        assert lib.vqs_debug_reduce_slices(pd.data_ptr(), nslices, n, out.ptr(), _stream()) == 0
        got = out.read()[0].reshape(rows, cols)
        y32 = R.reduce_slices_y(part, nslices, n, rows, cols, cols, dtype=torch.float32)
        assert torch.equal(got, y32.to(torch.bfloat16).double()), "not the index-order fp32 sum, rounded once"
        _check16(f"reduce_slices/k{nslices}_{rows}x{cols}", got, R.reduce_slices_y(part, nslices, n, rows, cols, cols))


def test_reduce_slices_refusals():
    lib = _lib()
    part = torch.zeros(64).cuda()
    out = _Planes(1, 16, 16, 1)
    assert lib.vqs_debug_reduce_slices(part.data_ptr(), 2, 6, out.ptr(), _stream()) == INVALID           # n % 4
    assert lib.vqs_debug_reduce_slices(part.data_ptr(), 2, 0, out.ptr(), _stream()) == INVALID
    for kw in [dict(cols=6), dict(ldp=18), dict(ld_out=18), dict(stride=66), dict(cols=32, gated=1), dict(ns=0)]:
        a = dict(ns=2, stride=32, rows=2, cols=16, ldp=16, gated=0, ld_out=16)
        a.update(kw)
        assert lib.vqs_debug_reduce_slices_act(part.data_ptr(), a["ns"], a["stride"], a["rows"], a["cols"], a["ldp"], None, a["gated"], out.ptr(), a["ld_out"],
                                               _stream()) == INVALID, kw
    assert out.untouched()


@pytest.mark.parametrize("bias_on", [False, True])
@pytest.mark.parametrize("gated", [0, 1])
@pytest.mark.parametrize("nslices", NSLICES)
def test_reduce_slices_act(nslices, gated, bias_on):
    lib, pad = _lib(), 4
    for rows, cols in SHAPES + (GATED_EXTRA if gated else UNGATED_EXTRA):
        ldp, out_cols = cols + pad, cols // 2 if gated else cols
        stride, seed = rows * ldp + 2 * pad, 5000 + 100 * nslices + rows + cols + gated
        part = _partials(_targets(rows, cols, bool(gated), seed), nslices, 1, ldp, stride, seed + 1)
        bias = (0.5 * torch.randn(cols, generator=_gen(seed + 2))).to(torch.bfloat16) if bias_on else None
        out = _Planes(rows, out_cols, out_cols + pad, 1)
        pd, bd = part.cuda(), None if bias is None else bias.cuda()
        assert lib.vqs_debug_reduce_slices_act(pd.data_ptr(), nslices, stride, rows, cols, ldp, None if bd is None else bd.data_ptr(), gated, out.ptr(),
                                               out_cols + pad, _stream()) == 0
        got = out.read()[0]
        y = R.reduce_slices_y(part, nslices, stride, rows, cols, ldp, bias)
        case = f"reduce_slices_act/k{nslices}_{rows}x{cols}_gated{gated}_bias{int(bias_on)}"
        if gated:
            _check16(case, got, R.gated(y, R.silu), allow=ALLOW["reduce_act_gated"])
        else:
            y32 = R.reduce_slices_y(part, nslices, stride, rows, cols, ldp, bias, dtype=torch.float32)
            assert torch.equal(got, y32.to(torch.bfloat16).double()), "not the index-order fp32 sum (+ bias), rounded once"
            _check16(case, got, y)


# =====================================================================================================================================
# masked_softmax / transpose_pad
# =====================================================================================================================================
@pytest.mark.parametrize("out_f16", [0, 1])
@pytest.mark.parametrize("rows", [1, 5, 80])
@pytest.mark.parametrize("S_pad", [64, 128, 640])
def test_masked_softmax(S_pad, rows, out_f16):
    lib, B = _lib(), 3
    bits = R.F16_BITS if out_f16 else R.BF16_BITS
    g = _gen(S_pad + rows)
    for key_len in ([1, 63, 64], [65, S_pad, S_pad + 7], [0, 1, S_pad]):
        sc = 3.0 * torch.randn(B * rows, S_pad, generator=g)
        for b in range(B):
            n = max(0, min(key_len[b], S_pad))
            r0 = b * rows
            if n >= 2:                                        # first row of the sample: scores spanning +-200, the top one leading by 30
                span = torch.cat([torch.linspace(-200.0, 170.0, n - 1), torch.tensor([200.0])])
                sc[r0, :n] = span[torch.randperm(n, generator=g)]
            if n >= 2 and rows > 1:                           # second row: one needle key
                sc[r0 + 1, :n] = 0.01 * torch.randn(n, generator=g)
                sc[r0 + 1, int(torch.randint(0, n, (1,), generator=g))] = 40.0
            sc[r0:r0 + rows, n:] = float("nan")               # never read: the output there is exactly 0
        out = _Planes(B * rows, S_pad, S_pad, 1, torch.float16 if out_f16 else torch.bfloat16)
        sd, kd = sc.cuda(), torch.tensor(key_len, dtype=torch.int32).cuda()
        assert lib.vqs_debug_masked_softmax(sd.data_ptr(), out.ptr(), kd.data_ptr(), B, rows, S_pad, out_f16, _stream()) == 0
        got = out.read()[0]
        ref = R.masked_softmax(sc, key_len, rows)
        assert torch.isfinite(got).all(), "a score past key_len was read"
        assert (got[ref == 0] == 0).all(), "keys past key_len (or a sample without keys) are not exact zeros"
        _check16(f"masked_softmax/S{S_pad}_rows{rows}_f16{out_f16}_len{key_len[0]}", got, ref, bits, ALLOW["masked_softmax_f16" if out_f16 else "masked_softmax_bf16"])


@pytest.mark.parametrize("B,S,D,S_pad", [(2, 1, 64, 64), (3, 63, 128, 64), (2, 65, 64, 128), (1, 608, 192, 640)])
def test_transpose_pad(B, S, D, S_pad):
    lib = _lib()
    x = torch.randn(B, S, D, generator=_gen(S + D)).to(torch.bfloat16)
    out = _nan16(B, D, S_pad).cuda()
    xd = x.cuda()
    assert lib.vqs_debug_transpose_pad(xd.data_ptr(), out.data_ptr(), B, S, D, S_pad, _stream()) == 0
    torch.cuda.synchronize()
    want = torch.zeros(B, D, S_pad, dtype=torch.bfloat16)
    want[:, :, :S] = x.transpose(1, 2)
    assert torch.equal(_bits16(out.cpu()), _bits16(want))     # bitwise: the pad columns are +0, whatever the buffer held


def test_transpose_pad_refusals():
    lib = _lib()
    x = torch.zeros(2 * 64 * 64, dtype=torch.bfloat16).cuda()
    out = _Planes(1, 4096, 4096, 1)
    for B, S, D, S_pad in [(1, 8, 32, 64), (1, 8, 96, 64), (1, 8, 64, 32), (1, 8, 64, 96), (1, 65, 64, 64)]:
        assert lib.vqs_debug_transpose_pad(x.data_ptr(), out.ptr(), B, S, D, S_pad, _stream()) == INVALID, (S, D, S_pad)
    assert out.untouched()


# =====================================================================================================================================
# argmax_append / score head
# =====================================================================================================================================
def _argmax(lib, logits, V, T, dst_col, ld_tokens=4, flags=True):
    """logits [B * T, ldl] -> (tokens [B, ld_tokens] after the launch, flags word or None).  tokens start at -7."""
    B, ldl = logits.shape[0] // T, logits.shape[1]
    tok = torch.full((B, ld_tokens), -7, dtype=torch.int32).cuda()
    fl = torch.zeros(1, dtype=torch.int32).cuda() if flags else None
    ld = logits.cuda()
    assert lib.vqs_debug_argmax_append(ld.data_ptr(), ldl, V, tok.data_ptr(), ld_tokens, B, T, dst_col, None if fl is None else fl.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return tok.cpu(), None if fl is None else int(fl.cpu())


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("V", [1, 255, 256, 257, 32128])
def test_argmax_append(V, T):
    lib, pad = _lib(), 5
    g = _gen(V + T)
    ties = [(5, 261), (256, 3), (V - 1, 0)]
    B = 4 + len(ties)
    lg = torch.randn(B * T, V + pad, generator=g)
    lg[:, V:] = float("inf")                                  # columns [V, ldl) must not win
    last = lg[T - 1::T]                                       # the row of each sample that is read (a view)
    last[1, :V] = 0.25                                        # an all-equal row -> 0
    last[2, :V] = -torch.arange(V, dtype=torch.float32)       # maximum at index 0
    last[3, :V] = torch.arange(V, dtype=torch.float32)        # maximum at the last index
    for i, (a, b) in enumerate(ties):                         # the same maximum twice -> the lowest index
        if a < V and b < V:
            last[4 + i, a] = last[4 + i, b] = 9.0
    if T > 1:
        lg[0::T, :V] += 50.0 * torch.nn.functional.one_hot(torch.full((B,), V // 2), V)       # rows that are NOT read hold another maximum
    want = last[:, :V].argmax(dim=-1).to(torch.int32)
    assert want[1] == 0 and want[2] == 0 and want[3] == V - 1
    for i, (a, b) in enumerate(ties):
        if a < V and b < V:
            assert want[4 + i] == min(a, b)
    for dst_col in (-1, 0, 2):
        tok, fl = _argmax(lib, lg, V, T, dst_col)
        col = T - 1 if dst_col < 0 else dst_col
        assert torch.equal(tok[:, col], want), (dst_col, tok[:, col], want)
        rest = torch.ones(tok.shape[1], dtype=torch.bool)
        rest[col] = False
        assert (tok[:, rest] == -7).all(), "another column of tokens changed"
        assert fl == 0, "a finite row raised the status bit"
    tok, fl = _argmax(lib, lg, V, T, -1, flags=False)         # flags = NULL is accepted
    assert torch.equal(tok[:, T - 1], want) and fl is None
    _rec(f"argmax_append/V{V}_T{T}", exact=True)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_argmax_append_status_bit(bad):
    lib, V, T = _lib(), 257, 3
    lg = torch.randn(2 * T, V + 3, generator=_gen(3))
    lg[T - 1, 200] = bad
    tok, fl = _argmax(lib, lg, V, T, -1)
    assert fl == 2
    if bad > 0:
        assert tok[0, T - 1] == 200
    lg[T - 1, 200] = 0.0
    lg[0, 200] = bad                                          # in a row that is not scanned: clear
    assert _argmax(lib, lg, V, T, -1)[1] == 0


@pytest.mark.parametrize("V,ldl", [(32128, 32256), (257, 264)])
def test_score_head(V, ldl):
    from t2v_metrics_amd import engine
    B, T = 6, 3
    g = _gen(V)
    lg = torch.empty(B, T, ldl).uniform_(-80.0, 40.0, generator=g)
    dom = torch.randint(0, V, (B, T), generator=g)
    lg.scatter_(-1, dom[..., None], 80.0)                     # one dominant label per row
    lg[..., V:] = float("nan")                                # columns [V, ldl) are never read
    labels = dom.clone()
    labels[0] = -100                                          # a pair without a label: exp(0) = 1
    labels[1, 0], labels[1, 1] = V + 5, -100                  # out of range: contributes 0 but counts
    labels[2, :2] = V - 1                                     # the last index
    labels[3] = (dom[3] + 1) % V                              # labels 120 below the dominant one: the score underflows to 0
    lg[3].scatter_(-1, labels[3][:, None], -40.0)
    lg[2, 0, V - 1] = 79.0
    flags = torch.zeros(1, dtype=torch.int32).cuda()
    lp, sc = engine.score_head(lg.cuda(), labels.cuda(), V=V, flags=flags)
    torch.cuda.synchronize()
    lp, sc = lp.cpu().double(), sc.cpu().double()
    ref_lp, ref_sc = R.label_logprobs(lg, labels, V)
    tol = 1e-5 + 1e-6 * ref_lp.abs()
    r = ((lp - ref_lp).abs() / tol).max().item()
    # exp(mean of the log-probs): their tolerances add up in the exponent, plus two fp32 roundings (the mean, expf) and the subnormal step
    n = (labels != -100).sum(-1).clamp(min=1)
    tol_sc = ref_sc * (torch.expm1(tol.sum(-1) / n) + 4.0 * 2.0 ** -23) + 2.0 ** -149
    r_sc = ((sc - ref_sc).abs() / tol_sc).max().item()
    _rec(f"score_head/V{V}", worst_error_to_bound=r, worst_score_error_to_bound=r_sc)
    assert r <= 1.0 and r_sc <= 1.0, (r, r_sc)
    assert sc[0] == 1.0 and (lp[0] == 0).all() and lp[1, 0] == 0 and lp[1, 1] == 0
    assert int(flags.cpu()) == 0, "finite rows raised the status bit"
    lp2, sc2 = engine.score_head(lg.cuda(), labels.cuda(), V=V)                      # without the status word: the boundary's entry point
    assert torch.equal(lp2.cpu().double(), lp) and torch.equal(sc2.cpu().double(), sc)
    lg[4, 1, 7] = float("nan")
    engine.score_head(lg.cuda(), labels.cuda(), V=V, flags=flags)
    assert int(flags.cpu()) == 2, "a NaN row did not raise the status bit"


# =====================================================================================================================================
# decoder attention: dec_self_attn_precise_kernel, dec_attn_kernel (self, cross, cached)
# =====================================================================================================================================
def _dec_attn(lib, q, k, v, out_ptr, bias, key_len, B, H, T, S, ldq, ldk, cross=0, kv_stride_b=0, qpos0=0, bias_ld=0, precise=0, out_plane=0):
    return lib.vqs_debug_decoder_attention(q, k, v, out_ptr, None if bias is None else bias.data_ptr(), None if key_len is None else key_len.data_ptr(),
                                           B, H, T, S, ldq, ldk, cross, kv_stride_b, qpos0, bias_ld, precise, out_plane, _stream())


def _self_inputs(B, T, H, kind, seed, dtype):
    """q, k, v [B, T, H, 64] of `dtype` (values exactly representable in it).  kind: 'random'; 'span': scores from -200 to +200 with key 0
    on top by 30; 'needle0' / 'needle_t': key 0 / key t carries query t's whole softmax (margin >= 30, checked on the inputs)."""
    g = _gen(seed)
    q = 0.5 * torch.randn(B, T, H, 64, generator=g)
    k = 0.5 * torch.randn(B, T, H, 64, generator=g)
    v = torch.randn(B, T, H, 64, generator=g)
    if kind != "random":
        u = torch.linalg.qr(torch.randn(B, H, 64, 64, generator=g, dtype=torch.float64)).Q[..., :T].permute(0, 3, 1, 2)   # [B, T, H, 64] orthonormal over T
        if kind == "span":
            t = torch.cat([torch.tensor([200.0]), torch.linspace(165.0, -200.0, T - 1)]) if T > 1 else torch.tensor([200.0])
            q = (16.0 * u[:, :1]).expand(B, T, H, 64).float()
            k = (t.view(1, T, 1, 1).double() / 16.0 * u[:, :1]).float()
        elif kind == "needle0":
            q = (32.0 * u[:, :1]).expand(B, T, H, 64).float()
            k = (0.05 * k.double() + torch.where(torch.arange(T).view(1, T, 1, 1) == 0, 32.0 * u[:, :1], torch.zeros(()).double())).float()
        else:
            q, k = (32.0 * u).float(), (32.0 * u).float()
    q, k, v = q.contiguous().to(dtype), k.contiguous().to(dtype), v.to(dtype)
    if kind != "random":                                      # the inputs, not the kernel
        s = torch.einsum("bthd,bjhd->bhtj", q.double(), k.double())
        s = s.masked_fill(torch.arange(T)[None, :] > torch.arange(T)[:, None], float("-inf"))
        top = s.topk(min(2, T), dim=-1).values
        if T > 1:
            assert (top[..., 1:, 0] - top[..., 1:, 1]).min() >= 30.0
        if kind == "span" and T > 1:
            assert s[..., -1, :].max() >= 190 and s[..., -1, :].min() <= -190
    return q, k, v


@pytest.mark.parametrize("kind,with_bias,wide", [("random", True, False), ("random", False, True), ("span", False, False), ("needle0", True, False),
                                                 ("needle_t", True, True)])
@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("T", [1, 3, 4, 5, 13, 16])
def test_dec_self_attn_precise(T, H, kind, with_bias, wide):
    lib, B, I = _lib(), 2, H * 64
    ldq = 3 * I + (8 if wide else 0)
    q, k, v = _self_inputs(B, T, H, kind, 100 * T + H, torch.float32)
    bias = torch.randn(H, T, generator=_gen(T + H)) if with_bias else None
    qkv = _nan32(B * T, ldq)
    qkv[:, :3 * I] = torch.cat([q.reshape(B * T, I), k.reshape(B * T, I), v.reshape(B * T, I)], dim=1)
    qd, bd = qkv.cuda(), None if bias is None else bias.cuda()
    out = _Planes(B * T, I, I, 2)
    assert _dec_attn(lib, qd.data_ptr(), qd.data_ptr() + 4 * I, qd.data_ptr() + 8 * I, out.ptr(), bd, None, B, H, T, T, ldq, ldq, precise=1,
                     out_plane=out.plane) == 0
    hi, lo = out.read()
    ref = R.self_attention(q, k, v, bias).reshape(B * T, I)
    for h in range(H):                                        # a row of the criterion = one head of one token
        _check_split(f"dec_self_attn_precise/T{T}_H{H}_{kind}_wide{int(wide)}/h{h}", hi[:, h * 64:(h + 1) * 64], lo[:, h * 64:(h + 1) * 64],
                     ref[:, h * 64:(h + 1) * 64], ALLOW["dec_precise"])


def test_dec_self_attn_precise_refusals():
    lib, B, H = _lib(), 1, 1
    qkv = torch.zeros(17, 192).cuda()
    kl = torch.tensor([1], dtype=torch.int32).cuda()
    out = _Planes(17, 64, 64, 2)
    p = qkv.data_ptr()

    def call(T=4, S=4, cross=0, qpos0=0, out_plane=None, ldk=192, stride=0, bias_ld=0):
        return _dec_attn(lib, p, p + 256, p + 512, out.ptr(), None, kl if cross else None, B, H, T, S, 192, ldk, cross=cross, kv_stride_b=stride, qpos0=qpos0,
                         bias_ld=bias_ld, precise=1, out_plane=out.plane if out_plane is None else out_plane)
    assert call(T=17, S=17) == INVALID and call(cross=1) == INVALID and call(S=5) == INVALID and call(qpos0=1) == INVALID
    assert call(out_plane=0) == INVALID and call(out_plane=-64) == INVALID and call(ldk=200) == INVALID and call(stride=768) == INVALID
    assert call(bias_ld=5) == INVALID and call(T=0, S=0) == INVALID
    assert out.untouched()


def _bf16_rows(case, got, ref, H):
    for h in range(H):
        _check16(f"{case}/h{h}", got[:, h * 64:(h + 1) * 64], ref[:, h * 64:(h + 1) * 64], allow=ALLOW["dec_attn"])


@pytest.mark.parametrize("kind", ["random", "span", "needle_t"])
@pytest.mark.parametrize("T", [13, 16])
def test_dec_attn_self_form_at_the_row_limit(T, kind):
    lib, B, H = _lib(), 2, 3
    I = H * 64
    q, k, v = _self_inputs(B, T, H, kind, 7 * T, torch.bfloat16)
    bias = torch.randn(H, T, generator=_gen(T)) if kind == "random" else None
    qkv = torch.cat([q.reshape(B * T, I), k.reshape(B * T, I), v.reshape(B * T, I)], dim=1).contiguous().cuda()
    bd = None if bias is None else bias.cuda()
    out = _Planes(B * T, I, I, 1)
    assert _dec_attn(lib, qkv.data_ptr(), qkv.data_ptr() + 2 * I, qkv.data_ptr() + 4 * I, out.ptr(), bd, None, B, H, T, T, 3 * I, 3 * I) == 0
    _bf16_rows(f"dec_attn/self_T{T}_{kind}", out.read()[0], R.self_attention(q, k, v, bias).reshape(B * T, I), H)
    assert _dec_attn(lib, qkv.data_ptr(), qkv.data_ptr() + 2 * I, qkv.data_ptr() + 4 * I, out.ptr(), bd, None, B, H, 17, 17, 3 * I, 3 * I) == INVALID


@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("S", [1, 255, 256, 257, 700])
def test_dec_attn_cross_form(S, T):
    """Keys past key_len[b] hold NaN bit patterns and must not reach the output.  The VALUE loop of dec_attn_kernel runs over all S keys with
    probability exactly 0 past key_len, so a value row there is multiplied by 0: it must be finite (include/vqs.h states the precondition; the
    engine's encoder rows past a prompt's length are zeros) and holds 1e30 here, which any non-zero weight would show."""
    lib, H = _lib(), 2
    key_len = sorted({1, min(4, S), S})
    B, I = len(key_len), H * 64
    g = _gen(S + T)
    q = (0.5 * torch.randn(B, T, H, 64, generator=g)).to(torch.bfloat16)
    k = (0.5 * torch.randn(B, H, S, 64, generator=g)).to(torch.bfloat16)
    v = torch.randn(B, H, S, 64, generator=g).to(torch.bfloat16)
    ref = R.cross_attention(q, k, v, key_len).reshape(B * T, I)
    for b, n in enumerate(key_len):
        _bits16(k)[b, :, n:] = R.BF16_NAN
        v[b, :, n:] = 1.0e30
    qd, kd, vd, ld = q.cuda(), k.cuda(), v.cuda(), torch.tensor(key_len, dtype=torch.int32).cuda()
    out = _Planes(B * T, I, I, 1)
    assert _dec_attn(lib, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.ptr(), None, ld, B, H, T, S, I, 0, cross=1) == 0
    got = out.read()[0]
    assert torch.isfinite(got).all(), "a key or value row past key_len reached the output"
    _bf16_rows(f"dec_attn/cross_S{S}_T{T}", got, ref, H)


@pytest.mark.parametrize("T,qpos0", [(1, 0), (1, 1), (1, 37), (3, 5)])
def test_dec_attn_cached_form(T, qpos0):
    """vqs_generate's form: T new query rows at decoder positions qpos0 + t over a K / V cache of qpos0 + T rows; cache rows after them hold
    NaN, the sample stride and the bias table's rows are wider than what is in use.  Held to the float64 reference of the teacher-forced
    pass over the same qpos0 + T positions (its last T rows), and -- where those fit the kernel's 16 rows -- the teacher-forced launch too."""
    lib, B, H, Lmax = _lib(), 2, 3, 48
    I, S = H * 64, qpos0 + T
    ldk = I + 8
    qf, kf, vf = _self_inputs(B, S, H, "random", 31 * S + T, torch.bfloat16)                  # all S positions
    bias_ld = S + 3
    bias = torch.randn(H, bias_ld, generator=_gen(S))
    ref = R.self_attention(qf, kf, vf, bias)[:, -T:].reshape(B * T, I)                        # teacher-forced, last T rows
    assert torch.allclose(ref, R.self_attention(qf[:, -T:], kf, vf, bias, qpos0=qpos0).reshape(B * T, I), rtol=0, atol=1e-12)
    kc, vc = _nan16(B, Lmax, ldk), _nan16(B, Lmax, ldk)
    kc[:, :S, :I], vc[:, :S, :I] = kf.reshape(B, S, I), vf.reshape(B, S, I)
    qd, kd, vd, bd = qf[:, -T:].reshape(B * T, I).contiguous().cuda(), kc.cuda(), vc.cuda(), bias.cuda()
    out = _Planes(B * T, I, I, 1)
    assert _dec_attn(lib, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.ptr(), bd, None, B, H, T, S, I, ldk, kv_stride_b=Lmax * ldk, qpos0=qpos0,
                     bias_ld=bias_ld) == 0
    got = out.read()[0]
    assert torch.isfinite(got).all()
    _bf16_rows(f"dec_attn/cached_T{T}_qpos{qpos0}", got, ref, H)
    if S <= 16:
        qkv = torch.cat([qf.reshape(B * S, I), kf.reshape(B * S, I), vf.reshape(B * S, I)], dim=1).contiguous().cuda()
        tf_bias = bias[:, :S].contiguous().cuda()
        o2 = _Planes(B * S, I, I, 1)
        assert _dec_attn(lib, qkv.data_ptr(), qkv.data_ptr() + 2 * I, qkv.data_ptr() + 4 * I, o2.ptr(), tf_bias, None, B, H, S, S, 3 * I, 3 * I) == 0
        full = o2.read()[0].reshape(B, S, I)
        _bf16_rows(f"dec_attn/teacher_forced_S{S}_last{T}", full[:, -T:].reshape(B * T, I), ref, H)


def test_dec_attn_lds_limit():
    """The largest S at T = 16 whose dynamic LDS fits 65 536 bytes (by the reference module's copy of the launcher's arithmetic) runs and is
    correct; the next is refused by the launcher itself, which is what holds the copy to it."""
    lib, B, H, T = _lib(), 1, 1, 16
    S = max(s for s in range(1, 2048) if R.dec_attn_lds_bytes(T, s) <= 65536)
    assert S == 702 and R.dec_attn_lds_bytes(T, S + 1) > 65536
    g = _gen(702)
    q = (0.5 * torch.randn(B, T, H, 64, generator=g)).to(torch.bfloat16)
    k = (0.5 * torch.randn(B, H, S + 1, 64, generator=g)).to(torch.bfloat16)
    v = torch.randn(B, H, S + 1, 64, generator=g).to(torch.bfloat16)
    qd, kd, vd = q.cuda(), k[:, :, :S].contiguous().cuda(), v[:, :, :S].contiguous().cuda()
    ld = torch.tensor([S], dtype=torch.int32).cuda()
    out = _Planes(T, 64, 64, 1)
    assert _dec_attn(lib, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), out.ptr(), None, ld, B, H, T, S, 64, 0, cross=1) == 0
    _bf16_rows("dec_attn/lds_limit_T16_S702", out.read()[0], R.cross_attention(q, k[:, :, :S], v[:, :, :S], [S]).reshape(T, 64), H)
    o2 = _Planes(T, 64, 64, 1)
    kd, vd = k.cuda(), v.cuda()
    assert _dec_attn(lib, qd.data_ptr(), kd.data_ptr(), vd.data_ptr(), o2.ptr(), None, ld, B, H, T, S + 1, 64, 0, cross=1) == INVALID
    assert o2.untouched()
