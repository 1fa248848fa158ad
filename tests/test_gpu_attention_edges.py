"""Exact-selection tests of the MFMA flash attention kernels at their tile edges (-m gpu): attn_fwd_dma_kernel / attn_fwd_dma_f16_kernel
<HAS_BIAS>, attn_fwd_hd_kernel<128, CAUSAL, F16> (through the hook vqs_debug_attention_hd: causal or not, bf16 or fp16, full-width or the
tower's 80-lane output) and attn_suffix_hd_kernel<F16>.

The inputs (tests/attention_edge_cases.py) make every compared output row ONE value row, bit for bit: the selected key's score lies G >= 200
log2 units above every other visible score, so all other probabilities and all rescale factors are exactly 0 in fp32, the needle's probability
packs to 1.0 and the row sum is 1 -- for any correct softmax, whatever its tiling (tests/test_attention_edge_inputs.py shows that on the CPU).
A key dropped, duplicated or swapped inside a tile, a hidden diagonal, one key too many at a ragged end or a masked row that leaks changes
whole rows, where a tolerance on Gaussian inputs moves by less than its absolute term.

  (a) test_*_selects_the_needle            every tile edge, every map, B.H = 9
  (b) test_*_ragged_ends / *_without_keys  key_len on both sides of the tile edges, 1, 0, S - 1, S, S + 5; guard rows around every output
  (c) test_*_masked_rows_do_not_matter     bitwise the same rows whatever lies behind key_len
  (d) test_bias_table_selects_*            the position-bias table as the only selector, S = 1 100: > 64 KiB of LDS, two table-fill passes
  (e) test_deferred_rescale_*              the second tile's maximum 5.5 and 6.5 log2 units above the first's (RESCALE_THR = 6)
  (f) test_*refus*                         launches that must be refused before anything reaches the device"""
import pytest
import torch

from tests import attention_edge_cases as ec
from tests.gpu_util import assert_close, attention_ref

pytestmark = pytest.mark.gpu

INVALID = -1
TOL = {False: (2e-2, 2e-2), True: (4e-3, 3e-3)}       # the per-type tolerances of tests/test_gpu_kernels.py (bf16, fp16)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from t2v_metrics_amd import engine
    engine.load_library()
    return engine


def _bits(t):
    return t.contiguous().view(torch.int16)


class Guarded:
    """An output of `rows` x `width` 16-bit elements with ec.GUARD sentinel rows in front of it and behind it."""

    def __init__(self, rows, width, dtype):
        self.buf = torch.full((rows + 2 * ec.GUARD, width), ec.SENTINEL, dtype=torch.int16, device="cuda")
        self.out = self.buf[ec.GUARD: ec.GUARD + rows].view(dtype)

    def assert_guards_intact(self):
        g = ec.GUARD
        assert bool((self.buf[:g] == ec.SENTINEL).all()) and bool((self.buf[-g:] == ec.SENTINEL).all()), "a store outside the output"


def _launch(eng, case):
    """One launch of the kernel the case is about, into a guarded output; returns it on the CPU as [rows, width]."""
    q, k, v = case.q.cuda(), case.k.cuda(), case.v.cuda()
    B, H, S, hd = q.shape
    kl = case.key_len_tensor("cuda")
    q0 = getattr(case, "q0", None)
    if q0 is not None:                                  # attn_suffix_hd_kernel: compact queries, three rows more than the suffix has
        Sq = S - q0 + 3
        qs = torch.full((B, H, Sq, hd), 3.0, dtype=q.dtype, device="cuda")
        qs[:, :, : S - q0] = q[:, :, q0:]
        g = Guarded(B * Sq, H * hd, q.dtype)
        rc = eng.load_library().vqs_debug_qwen_attention_suffix(qs.data_ptr(), k.data_ptr(), v.data_ptr(), g.out.data_ptr(), kl.data_ptr(), B, H,
                                                                k.shape[1], S, Sq, q0, case.scale, int(q.dtype == torch.float16),
                                                                torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        g.assert_guards_intact()
        full = torch.full((B, S, H * hd), float("nan"), dtype=q.dtype)
        full[:, q0:] = g.out.view(B, Sq, H * hd)[:, : S - q0].cpu()
        # the rows behind the suffix are never written
        assert bool((_bits(g.out.view(B, Sq, H * hd)[:, S - q0:]) == ec.SENTINEL).all())
        return full.view(B * S, H * hd)
    if hd == 64:
        g = Guarded(B * S, H * 64, q.dtype)
        eng.attention(q, k, v, case.scale, bias_table=None if case.table is None else case.table.cuda(), key_len=kl, out=g.out)
    else:
        g = Guarded(B * S, H * (case.out_hd or hd), q.dtype)
        eng.debug_attention_hd(q, k, v, case.scale, causal=case.causal, key_len=kl, out_hd=case.out_hd, out=g.out)
    torch.cuda.synchronize()
    g.assert_guards_intact()
    return g.out.cpu()


def _assert_selected(eng, case, what):
    G = ec.selection_margin(case)
    print(f"{what}: G = {G:.1f} log2 units")
    assert G >= ec.G_MIN, G
    out = _launch(eng, case)
    exp, m = ec.expected_rows(case), ec.row_mask(case)
    same = (_bits(out) == _bits(exp)).all(dim=1)
    bad = torch.nonzero(m & ~same).flatten()
    S = case.q.shape[2]
    assert bad.numel() == 0, (f"{what}: {bad.numel()} of {int(m.sum())} rows are not the selected value row; first (sample, row): "
                              f"{[(int(r) // S, int(r) % S) for r in bad[:12]]}")
    return out


# ---------------------------------------------------------------------------- (a) exact key selection through q.k
@pytest.mark.parametrize("S,f16,mode,B,H", ec.HD64_SELECT)
def test_hd64_selects_the_needle(eng, S, f16, mode, B, H):
    _assert_selected(eng, ec.hd64_case(S, f16, mode, B, H), f"hd64 S{S} f16={f16} {mode} B{B} H{H}")


@pytest.mark.parametrize("S,f16,causal,H,Hkv,out_hd,B", ec.HD128_SELECT)
def test_hd128_selects_the_needle(eng, S, f16, causal, H, Hkv, out_hd, B):
    _assert_selected(eng, ec.hd128_case(S, f16, causal, H, Hkv, out_hd, B), f"hd128 S{S} f16={f16} causal={causal} H{H}/{Hkv} out_hd={out_hd} B{B}")


@pytest.mark.parametrize("S,q0,f16", ec.SUFFIX_SELECT)
def test_suffix_selects_the_needle(eng, S, q0, f16):
    _assert_selected(eng, ec.suffix_case(S, q0, f16), f"suffix S{S} q0={q0} f16={f16}")


# ---------------------------------------------------------------------------- (b) ragged ends
@pytest.mark.parametrize("m,f16,mode", ec.HD64_RAGGED)
def test_hd64_ragged_ends(eng, m, f16, mode):
    _assert_selected(eng, ec.hd64_ragged_case(m, f16, mode), f"hd64 ragged {m} f16={f16} {mode}")


@pytest.mark.parametrize("m,f16,causal,out_hd", ec.HD128_RAGGED)
def test_hd128_ragged_ends(eng, m, f16, causal, out_hd):
    _assert_selected(eng, ec.hd128_ragged_case(m, f16, causal, out_hd), f"hd128 ragged {m} f16={f16} causal={causal} out_hd={out_hd}")


@pytest.mark.parametrize("m,f16", ec.SUFFIX_RAGGED)
def test_suffix_ragged_ends(eng, m, f16):
    _assert_selected(eng, ec.suffix_ragged_case(m, f16), f"suffix ragged {m} f16={f16}")


NO_KEYS = [129, 0, 65]      # key_len per sample


def _assert_zero_rows_of_the_sample_without_keys(out, case, first_row=0):
    """Both kernels end with `inv = l_tot > 0 ? 1 / l_tot : 0` and store o * inv: a sample without a visible key gets rows of zeros."""
    B, S = case.q.shape[0], case.q.shape[2]
    rows = out.view(B, S, -1)[1, first_row:]
    assert bool((_bits(rows) == 0).all()), "key_len = 0: the sample's rows are not +0"


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("mode", list(ec.HD64_MODES))
def test_hd64_sample_without_keys(eng, f16, mode):
    case = ec.hd64_case(129, f16, mode, 3, 4, key_len=NO_KEYS, poison=True)
    _assert_zero_rows_of_the_sample_without_keys(_assert_selected(eng, case, f"hd64 key_len 0 f16={f16} {mode}"), case)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("out_hd", [0, 80])
def test_hd128_sample_without_keys(eng, out_hd, causal, f16):
    case = ec.hd128_case(129, f16, causal, 4, 2, out_hd, 3, key_len=NO_KEYS, poison=True)
    _assert_zero_rows_of_the_sample_without_keys(_assert_selected(eng, case, f"hd128 key_len 0 f16={f16} causal={causal} out_hd={out_hd}"), case)


@pytest.mark.parametrize("f16", [False, True])
def test_suffix_sample_without_keys(eng, f16):
    case = ec.suffix_case(129, 32, f16, B=3, key_len=NO_KEYS, poison=True)
    _assert_zero_rows_of_the_sample_without_keys(_assert_selected(eng, case, f"suffix key_len 0 f16={f16}"), case, first_row=32)


# ---------------------------------------------------------------------------- (c) masked rows do not matter
def _assert_masked_rows_do_not_matter(eng, hd, f16, causal, bias, q0=None, out_hd=0):
    outs = []
    for poisoned in (False, True):
        case = ec.masked_rows_case(hd, f16, causal, bias, poisoned, out_hd=out_hd)
        if q0 is not None:
            case.q0 = q0
        outs.append(_launch(eng, case))
    m = ec.row_mask(case)
    if q0 is not None:
        m = m & (torch.arange(case.q.shape[2]) >= q0).repeat(case.q.shape[0])
    assert int(m.sum()) > 0 and torch.isfinite(outs[0][m].float()).all()
    assert torch.equal(_bits(outs[0][m]), _bits(outs[1][m])), "rows in front of key_len depend on what lies behind it"
    # and the rows are the operation's (the file's per-type tolerance): the mask is where it should be
    ref = ec.attention_fp32(case.q, case.k, case.v, case.scale, case.table, case.key_len, causal)[:, : out_hd or hd]      # one head
    assert_close(outs[1][m], ref[m], *TOL[f16], f"masked rows hd{hd} f16={f16} causal={causal} bias={bias}")


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_hd64_masked_rows_do_not_matter(eng, bias, f16):
    _assert_masked_rows_do_not_matter(eng, 64, f16, False, bias)


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("out_hd", [0, 80])
def test_hd128_masked_rows_do_not_matter(eng, out_hd, causal, f16):
    _assert_masked_rows_do_not_matter(eng, 128, f16, causal, False, out_hd=out_hd)


@pytest.mark.parametrize("f16", [False, True])
def test_suffix_masked_rows_do_not_matter(eng, f16):
    _assert_masked_rows_do_not_matter(eng, 128, f16, True, False, q0=ec.RAGGED_Q0)


# ---------------------------------------------------------------------------- (d) exact selection through the bias table
@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("S,f16,scale", ec.BIAS_SELECT)
def test_bias_table_selects_the_key(eng, S, f16, scale, ragged):
    """Picked rows are V[i + d_h] bit for bit.  The other rows are uniform means: the kernel's sum is exact (small integers), it multiplies by
    an fp32 1 / key_len and rounds to the tensor type, so it may sit one unit in the last place off the fp64 mean rounded once."""
    case = ec.bias_select_case(S, f16, scale, [S - 5] if ragged else None)
    out = _launch(eng, case)
    H = len(case.offs)
    d = (ec.ordered_bits(out) - ec.ordered_bits(case.expected)).abs().view(S, H, 64)
    picked = case.picked_rows                                              # [S,H]
    assert int(d[picked].max() if picked.any() else 0) == 0, "a picked row is not the selected value row"
    rest = d[~picked]
    print(f"bias selection S{S} f16={f16} scale={scale} ragged={ragged}: {int((rest == 1).sum())} of {rest.numel()} mean elements one ulp off, "
          f"{int(picked.sum())} picked rows exact")
    assert int(rest.max() if rest.numel() else 0) <= 1, f"a mean row is {int(rest.max())} ulp off"


@pytest.mark.parametrize("f16", [False, True])
def test_bias_attention_at_1100_keys(eng, f16):
    """Gaussian inputs at the size whose launch asks for more than 64 KiB of dynamic LDS and fills the bias table in two passes."""
    B, H, S = 1, 2, 1100
    g = torch.Generator().manual_seed(21)
    dt = ec.dtype_of(f16)
    q, k, v = ((torch.randn(B, H, S, 64, generator=g) * s).to(dt).cuda() for s in (0.5, 0.5, 1.0))
    table = torch.randn(H, 2 * S - 1, generator=g).cuda()
    key_len = torch.tensor([S - 3], dtype=torch.int32, device="cuda")
    idx = (torch.arange(S)[None, :] - torch.arange(S)[:, None] + S - 1).cuda()
    ref = attention_ref(q, k, v, 1.0, table[:, idx], key_len)
    assert_close(eng.attention(q, k, v, 1.0, bias_table=table, key_len=key_len), ref, *TOL[f16], f"attention S1100 bias f16={f16}")


# ---------------------------------------------------------------------------- (e) both sides of the deferred rescale
@pytest.mark.parametrize("gap,lo,hi", [(5.5, 5.0, 6.0), (6.5, 6.0, 7.0)])
@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_deferred_rescale_on_both_sides_of_the_threshold(eng, hd, f16, gap, lo, hi):
    case, gaps = ec.rescale_case(hd, f16, gap)
    assert lo < float(gaps.min()) and float(gaps.max()) < hi, (float(gaps.min()), float(gaps.max()))
    q, k, v = case.q.cuda(), case.k.cuda(), case.v.cuda()
    ref = attention_ref(q, k, v, case.scale)
    out = eng.attention(q, k, v, case.scale) if hd == 64 else eng.debug_attention_hd(q, k, v, case.scale)
    assert_close(out, ref, *TOL[f16], f"rescale hd{hd} f16={f16} gap={gap}")
    if hd == 128:                                       # the causal form: rows 0..63 see the first tile only
        ref = ec.attention_fp32(case.q, case.k, case.v, case.scale, causal=True)
        assert_close(eng.debug_attention_hd(q, k, v, case.scale, causal=True), ref, *TOL[f16], f"rescale hd128 causal f16={f16} gap={gap}")


# ---------------------------------------------------------------------------- (f) refusals: nothing is launched
@pytest.mark.parametrize("f16", [False, True])
def test_bias_table_beyond_the_lds_is_refused(eng, f16):
    S = ec.smallest_refused_bias_S()
    x = torch.zeros(1, 1, S, 64, dtype=ec.dtype_of(f16), device="cuda")            # real sizes: a launch would stay inside them
    table = torch.zeros(1, 2 * S - 1, device="cuda")
    g = Guarded(S, 64, x.dtype)
    with pytest.raises(eng.VqsError):
        eng.attention(x, x, x, 1.0, bias_table=table, out=g.out)
    torch.cuda.synchronize()
    assert bool((g.buf == ec.SENTINEL).all())


@pytest.mark.parametrize("H,Hkv,out_hd", [(4, 4, 6), (4, 4, 82), (4, 4, 132), (4, 4, -4), (4, 3, 0), (7, 2, 0)])
@pytest.mark.parametrize("causal", [0, 1])
@pytest.mark.parametrize("f16", [0, 1])
def test_hd128_refuses_bad_head_geometry(eng, f16, causal, H, Hkv, out_hd):
    S = 64
    dt = ec.dtype_of(f16)
    q = torch.zeros(1, H, S, 128, dtype=dt, device="cuda")
    kv = torch.zeros(1, H, S, 128, dtype=dt, device="cuda")                        # as large as any reading of (H, Hkv) would need
    g = Guarded(S, H * 128 + 128, dt)
    rc = eng.load_library().vqs_debug_attention_hd(q.data_ptr(), kv.data_ptr(), kv.data_ptr(), g.out.data_ptr(), None, 1, H, Hkv, S, 0.1, causal, f16,
                                                   out_hd, torch.cuda.current_stream().cuda_stream)
    assert rc == INVALID
    with pytest.raises(eng.VqsError):
        eng.debug_attention_hd(q, kv[:, :Hkv].contiguous(), kv[:, :Hkv].contiguous(), 0.1, causal=bool(causal), out_hd=out_hd)
    torch.cuda.synchronize()
    assert bool((g.buf == ec.SENTINEL).all())
