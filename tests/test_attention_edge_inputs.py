"""The inputs of tests/test_gpu_attention_edges.py, checked without a GPU: for every parametrised case of the exact-selection, ragged-end
and bias-selection tests a plain fp32 softmax of the operation gives the needle a weight of exactly 1.0 and every other key exactly 0, with
G >= 200 log2 units between them.  So the rows those tests expect are properties of the operation, not of a kernel."""
import pytest
import torch

from tests import attention_edge_cases as ec


def _assert_one_hot(case):
    G, s = ec.selection_margin(case, return_scores=True)
    assert G >= ec.G_MIN, G
    p = torch.softmax(s, dim=-1)                                         # fp32
    rows = case.rows[:, None, :].expand(-1, s.shape[1], -1)
    one_hot = torch.zeros_like(p).scatter_(-1, case.pi[..., None], 1.0)
    assert torch.equal(p[rows], one_hot[rows])
    # and then softmax . V is the selected value row, bit for bit
    out = ec.attention_fp32(case.q, case.k, case.v, case.scale, case.table, case.key_len, case.causal).to(case.v.dtype)
    B, H, S, hd = case.q.shape
    w = case.out_hd if case.out_hd > 0 else hd
    out = out.view(B * S, H, hd)[..., :w].reshape(B * S, H * w)
    m = ec.row_mask(case)
    assert torch.equal(out[m].view(torch.int16), ec.expected_rows(case)[m].view(torch.int16))
    return G


@pytest.mark.parametrize("S,f16,mode,B,H", ec.HD64_SELECT)
def test_hd64_selection_inputs(S, f16, mode, B, H):
    _assert_one_hot(ec.hd64_case(S, f16, mode, B, H))


@pytest.mark.parametrize("S,f16,causal,H,Hkv,out_hd,B", ec.HD128_SELECT)
def test_hd128_selection_inputs(S, f16, causal, H, Hkv, out_hd, B):
    case = ec.hd128_case(S, f16, causal, H, Hkv, out_hd, B)
    _assert_one_hot(case)
    if out_hd:
        assert not case.q[..., out_hd:].any() and not case.k[..., out_hd:].any() and not case.v[..., out_hd:].any()
    if causal:
        assert (case.pi <= torch.arange(S)).all()


@pytest.mark.parametrize("S,q0,f16", ec.SUFFIX_SELECT)
def test_suffix_selection_inputs(S, q0, f16):
    case = ec.suffix_case(S, q0, f16)
    _assert_one_hot(case)
    assert q0 % 32 == 0 and not case.rows[:, :q0].any() and case.rows[:, q0:].all()


@pytest.mark.parametrize("m,f16,mode", ec.HD64_RAGGED)
def test_hd64_ragged_inputs(m, f16, mode):
    case = ec.hd64_ragged_case(m, f16, mode)
    _assert_one_hot(case)
    _assert_poisoned_rows_would_win(case, m)


@pytest.mark.parametrize("m,f16,causal,out_hd", ec.HD128_RAGGED)
def test_hd128_ragged_inputs(m, f16, causal, out_hd):
    case = ec.hd128_ragged_case(m, f16, causal, out_hd)
    _assert_one_hot(case)
    if not causal:
        _assert_poisoned_rows_would_win(case, m)


@pytest.mark.parametrize("m,f16", ec.SUFFIX_RAGGED)
def test_suffix_ragged_inputs(m, f16):
    _assert_one_hot(ec.suffix_ragged_case(m, f16))


def _assert_poisoned_rows_would_win(case, m):
    """Sharpness of the ragged cases: with ONE key too many visible (key_len + 1), every compared row of the 'last' map would select the
    poisoned key instead -- a kernel that masks `key > key_len` instead of `key >= key_len` changes exactly those rows."""
    if m != "last":
        return
    S = case.q.shape[2]
    longer = [x + 1 for x in case.key_len]
    s = ec.scores_fp32(case.q, case.k, case.scale, case.table, longer, case.causal)
    for b, klen in enumerate(case.klens):
        if klen < S:
            assert (s[b, :, :klen].argmax(-1) == klen).all(), (b, klen)
            assert (case.v[b, :, klen, : case.live] == 1000).all()


def test_ragged_lengths_sit_on_both_sides_of_the_tile_edges():
    kl = ec.ragged_key_lens(ec.RAGGED_S)
    assert {1, 63, 64, 65, 127, 128, 129} <= set(kl) and {ec.RAGGED_S - 1, ec.RAGGED_S, ec.RAGGED_S + 5} <= set(kl)
    assert ec.RAGGED_Q0 % 32 == 0 and min(kl) < ec.RAGGED_Q0 < ec.RAGGED_S         # a key_len below the suffix's first row


@pytest.mark.parametrize("ragged", [False, True])
@pytest.mark.parametrize("S,f16,scale", ec.BIAS_SELECT)
def test_bias_selection_inputs(S, f16, scale, ragged):
    key_len = [S - 5] if ragged else None
    case = ec.bias_select_case(S, f16, scale, key_len)
    klen = case.klens[0]
    offs = case.offs
    assert {d % 4 for d in offs} == {0, 1, 2, 3} and {0, 1, -1, 2, -2, 3, -3, S - 1, 1 - S} <= set(offs)
    if S > 64:
        assert {63, -63, 64, -64} <= set(offs)
    s = ec.scores_fp32(case.q, case.k, scale, case.table, case.key_len)
    assert not case.q.any()
    p = torch.softmax(s, dim=-1)[0]                                       # [H,S,S] fp32
    one_hot = torch.zeros_like(p).scatter_(-1, case.tgt.clamp(0, S - 1)[..., None], 1.0)
    assert torch.equal(p[case.picked], one_hot[case.picked])
    # G of the picked rows: the peak against a table of zeros
    vis = s[0].masked_fill(one_hot.bool(), float("-inf"))
    if S > 1:
        assert float(((ec.BIAS_PEAK - vis.max(-1).values) * ec.LOG2E)[case.picked].min()) >= ec.G_MIN
    # every other row: all visible scores equal (the peak is absent or masked), so the weights are uniform over the klen visible keys
    rest = ~case.picked
    assert (s[0][rest][:, :klen] == 0).all() and torch.isinf(s[0][rest][:, klen:]).all()
    on_masked_key = (case.tgt >= klen) & (case.tgt < S)                # rows whose peak lies on a masked key are among them: the mask wins
    assert bool(on_masked_key.any()) == ragged and not (on_masked_key & case.picked).any()
    # the integer sums are exact in fp32 in any order
    v = case.v[0, :, :klen].float()
    exact = case.v[0, :, :klen].to(torch.int64).sum(1)
    perm = torch.randperm(klen, generator=torch.Generator().manual_seed(1))
    for order in (v, v.flip(1), v[:, perm]):
        acc = torch.zeros(v.shape[0], 64)
        for j in range(klen):
            acc = acc + order[:, j]
        assert torch.equal(acc.to(torch.int64), exact)
    assert int(case.v.float().abs().max()) <= 8 and 8 * klen < 2 ** 24
    # the expectation: fp64 mean / selected row, rounded once
    e = case.expected.view(S, len(offs), 64)
    h, i = 1, S // 2                                                     # offset +1: row i selects key i + 1 while it is visible
    want = case.v[0, h, i + 1] if i + 1 < klen else case.v[0, h, :klen].double().mean(0).to(case.v.dtype)
    assert torch.equal(e[i, h], want)


def test_ordered_bits_counts_units_in_the_last_place():
    for dt in (torch.bfloat16, torch.float16):
        x = torch.tensor([1.0, -1.0, 0.0, -0.0, 3.5], dtype=dt)
        up = torch.nextafter(x.float(), torch.full((5,), float("inf"))).to(dt)       # fp32 neighbours round back: same 16-bit value
        assert torch.equal(ec.ordered_bits(x), ec.ordered_bits(up))
        one = torch.tensor([1.0], dtype=dt)
        nxt = (one.view(torch.int16) + 1).view(dt)
        assert int(ec.ordered_bits(nxt) - ec.ordered_bits(one)) == 1 and int(ec.ordered_bits(-nxt) - ec.ordered_bits(-one)) == -1
        assert int(ec.ordered_bits(torch.tensor([0.0], dtype=dt))) == int(ec.ordered_bits(torch.tensor([-0.0], dtype=dt))) == 0


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("f16", [False, True])
def test_rescale_inputs_sit_on_both_sides_of_the_threshold(hd, f16):
    _, below = ec.rescale_case(hd, f16, 5.5)
    _, above = ec.rescale_case(hd, f16, 6.5)
    assert 5.0 < float(below.min()) and float(below.max()) < 6.0, (float(below.min()), float(below.max()))
    assert 6.0 < float(above.min()) and float(above.max()) < 7.0, (float(above.min()), float(above.max()))


def test_refusal_size_follows_the_launchers_formula():
    S = ec.smallest_refused_bias_S()
    assert 2 * 16384 + ec.bias_copy_chunks(S) * 64 > 160 * 1024 >= 2 * 16384 + ec.bias_copy_chunks(S - 1) * 64
    # the shapes the tests launch: T5-XL's 608 keys fit three workgroups per CU, 1 100 keys pass 64 KiB and need a second table-fill pass
    assert 2 * 16384 + ec.bias_copy_chunks(608) * 64 == 53504
    assert 2 * 16384 + ec.bias_copy_chunks(1100) * 64 > 65536 and 4 * ec.bias_copy_chunks(1100) + 3 > 2048
