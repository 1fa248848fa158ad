"""The precise tail's attention over a ROW LIST on its own (include/vqs_debug.h vqs_debug_qwen_rows_attention; csrc/qwen_decode.hip
qwen_rows_attn_kernel / qwen_rows_attn_head_kernel): single launches on caller tensors.  Row r of Q attends over the K / V slabs of sample
row_sample[r] with row_keys[r] keys -- the kernel behind vqs_qwen_score_rows (teacher-forced answers: several rows per sample).

  (a) the identity list (row b = sample b with its length) is launch_qwen_tail_attn (vqs_debug_qwen_decode_attention modes 1, 2) BIT FOR BIT, in
      the grouped form, in the grouped form at its largest cache (opt-in dynamic LDS) and in the per-query-head form one position further;
  (b) shuffled and repeated samples with key counts around the kernels' 4- / 32- / 64-key steps: every row against the float64 reference under
      the criteria tests/test_gpu_qwen_decode_kernels.py holds the same arithmetic to (|hi + lo - ref| <= 2e-5 max|ref_row|, |lo| <= half an
      ulp of hi), and bitwise the same row in a launch of its own (a row does not depend on its neighbours in the list);
  (c) a sample outside [0, R) gives a zero row, key counts are clamped to [1, L], and nothing outside the Q rows of the two planes is written.
Neither bound is taken from the kernels' own results."""
import pytest
import torch

from tests import test_gpu_qwen_decode_kernels as dk

pytestmark = pytest.mark.gpu

HD, GROUPED, PER_HEAD, INVALID = dk.HD, dk.GROUPED, dk.PER_HEAD, dk.INVALID
HEADS = [(4, 2), (7, 1), (8, 1), (2, 1)]
GUARD = 3               # guard rows around each output plane
EDGE_KEYS = (1, 2, 31, 32, 33, 63, 64, 65)


def _crossover(lib, Hq, Hkv):
    """-> the largest cache the grouped form takes for this geometry (G rows of ((L + 3) & ~3) fp32 scores within 120 KiB); one position
    further the launcher takes the per-query-head kernel.  Held against the launcher's own decision function."""
    G = Hq // Hkv
    L = (120 * 1024 // (4 * G)) & ~3
    assert dk._form(lib, Hq, Hkv, L)[0] == GROUPED and dk._form(lib, Hq, Hkv, L + 1)[0] == PER_HEAD, (Hq, Hkv, L)
    return L


def _inputs(Q, R, Hq, Hkv, L, f16, seed):
    """q fp32 [Q, Hq, 128] with score deviation near 3, random K / V [R, Hkv, L, 128] as the kernel reads them -> (q, K, V, scale, vscale)."""
    g = torch.Generator().manual_seed(seed)
    q = 3.0 * torch.randn(Q, Hq, HD, generator=g)
    k = torch.randn(R, Hkv, L, HD, generator=g)
    v = torch.randn(R, Hkv, L, HD, generator=g)
    if f16:
        return q, (k * dk.KSCALE).to(torch.float16), (v * dk.VSCALE).to(torch.float16), dk._f32(dk.SCALE / dk.KSCALE), 1.0 / dk.VSCALE
    return q, k.to(torch.bfloat16), v.to(torch.bfloat16), dk.SCALE, 1.0


class _Dev:
    """The operands of one geometry on the device, uploaded once and never modified."""

    def __init__(self, q, K, V):
        self.q, self.K, self.V = q.contiguous().cuda(), K.contiguous().cuda(), V.contiguous().cuda()
        self.R, self.Hkv, self.L = K.shape[0], K.shape[1], K.shape[2]
        self.Hq = q.shape[1]


def _launch_rows(lib, d, q_rows, samples, keys, scale, vscale, f16):
    """One launch of the hook over the rows q_rows of d.q.  -> (hi, lo) int16 CPU [Q, Hq, 128]; asserts the guard rows around both planes."""
    Q, W = len(samples), d.Hq * HD
    qd = d.q[torch.tensor(q_rows, device="cuda")].contiguous()
    buf = torch.full((2 * (Q + GUARD) + GUARD, W), dk.SENTINEL, dtype=torch.int16, device="cuda")
    out = buf[GUARD:]
    rs = torch.tensor(samples, dtype=torch.int32).cuda()
    rk = torch.tensor(keys, dtype=torch.int32).cuda()
    rc = lib.vqs_debug_qwen_rows_attention(qd.data_ptr(), d.K.data_ptr(), d.V.data_ptr(), rs.data_ptr(), rk.data_ptr(), out.data_ptr(), (Q + GUARD) * W,
                                           Q, d.R, d.Hq, d.Hkv, d.L, scale, 1 if f16 else 0, vscale, dk._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    res = buf.cpu()
    for lo, hi in ((0, GUARD), (GUARD + Q, 2 * GUARD + Q), (2 * GUARD + 2 * Q, 3 * GUARD + 2 * Q)):
        assert (res[lo:hi] == dk.SENTINEL).all(), "a guard row around the output planes was written"
    return res[GUARD:GUARD + Q].view(Q, d.Hq, HD), res[2 * GUARD + Q:2 * GUARD + 2 * Q].view(Q, d.Hq, HD)


def _reference_rows(q, K, V, samples, keys, scale, vscale):
    """float64: row r = softmax(q_r K^T scale) V vscale over the first keys[r] keys of sample samples[r]."""
    G = q.shape[1] // K.shape[1]
    out = torch.empty(len(samples), q.shape[1], HD, dtype=torch.float64)
    for r, (b, n) in enumerate(zip(samples, keys)):
        k = K[b, :, :n].double().repeat_interleave(G, dim=0)
        v = V[b, :, :n].double().repeat_interleave(G, dim=0)
        s = torch.einsum("hd,hnd->hn", q[r].double(), k) * scale
        out[r] = torch.einsum("hn,hnd->hd", torch.softmax(s, dim=-1), v) * vscale
    return out


def _values(bits):
    return bits.view(torch.bfloat16).double()


# ---- (a) the identity list is the one-row-per-sample tail attention, bit for bit
@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("where", ["small", "grouped_limit", "per_head"])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_identity_row_list_is_the_tail_attention_bit_for_bit(Hq, Hkv, where, f16):
    lib = dk._lib()
    Lx = _crossover(lib, Hq, Hkv)
    L, ns = {"small": (301, (1, 257, 301, 64)), "grouped_limit": (Lx, (Lx, 257)), "per_head": (Lx + 1, (Lx + 1, 257))}[where]
    assert dk._form(lib, Hq, Hkv, L)[0] == (PER_HEAD if where == "per_head" else GROUPED)
    R = len(ns)
    q, K, V, scale, vscale = _inputs(R, R, Hq, Hkv, L, f16, seed=17 * Hq + Hkv + L)
    d = _Dev(q, K, V)
    hi, lo = _launch_rows(lib, d, list(range(R)), list(range(R)), list(ns), scale, vscale, f16)
    out = torch.full((2, R, Hq, HD), dk.BF16_NAN, dtype=torch.int16).cuda()
    ld = torch.tensor(ns, dtype=torch.int32).cuda()
    rc = lib.vqs_debug_qwen_decode_attention(d.q.data_ptr(), d.K.data_ptr(), d.V.data_ptr(), ld.data_ptr(), out.data_ptr(), R * Hq * HD, R, Hq, Hkv, L, scale,
                                             vscale, 2 if f16 else 1, dk._stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    want = out.cpu()
    assert torch.isfinite(_values(want)).all()
    assert torch.equal(hi, want[0]) and torch.equal(lo, want[1])


# ---- (b) shuffled and repeated samples, key counts at the kernels' steps
def _edge_list(R, L):
    keys = list(EDGE_KEYS) + [L, L - 1, 3, L]
    samples = [(5 * i + 2) % R for i in range(len(keys))]          # shuffled, every sample several times, not in order
    assert len(set(samples)) == R and samples != sorted(samples)
    return samples, keys


@pytest.mark.parametrize("f16", [False, True], ids=["bf16", "fp16"])
@pytest.mark.parametrize("form", [GROUPED, PER_HEAD])
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_rows_of_shuffled_and_repeated_samples(Hq, Hkv, form, f16):
    lib, R = dk._lib(), 3
    L = 97 if form == GROUPED else _crossover(lib, Hq, Hkv) + 1
    assert dk._form(lib, Hq, Hkv, L)[0] == form
    samples, keys = _edge_list(R, L)
    Q = len(keys)
    q, K, V, scale, vscale = _inputs(Q, R, Hq, Hkv, L, f16, seed=31 * Hq + Hkv + L)
    d = _Dev(q, K, V)
    hi, lo = _launch_rows(lib, d, list(range(Q)), samples, keys, scale, vscale, f16)
    ref = _reference_rows(q, K, V, samples, keys, scale, vscale)
    assert torch.isfinite(_values(hi)).all() and torch.isfinite(_values(lo)).all()
    r_sum, r_lo = dk._ratios(1, (_values(hi), _values(lo)), ref)
    dk._record(f"qwen_rows_kernels/shuffled/Hq{Hq}_Hkv{Hkv}_L{L}_{'fp16' if f16 else 'bf16'}", {"worst_error_to_bound": r_sum, "worst_lo_to_half_ulp": r_lo})
    print("rows", Hq, Hkv, L, f16, "error / bound", r_sum, r_lo)
    assert r_sum <= 1.0 and r_lo <= 1.0, (r_sum, r_lo)
    for r in range(Q):                                             # a row's bits do not depend on the rows it shares the launch with
        h1, l1 = _launch_rows(lib, d, [r], [samples[r]], [keys[r]], scale, vscale, f16)
        assert torch.equal(h1[0], hi[r]) and torch.equal(l1[0], lo[r]), r


# ---- (c) values outside their range: a zero row, clamped counts, untouched neighbours
@pytest.mark.parametrize("Hq,Hkv,form", [(7, 1, GROUPED), (4, 2, GROUPED), (7, 1, PER_HEAD)])
def test_out_of_range_samples_and_key_counts(Hq, Hkv, form):
    lib, R = dk._lib(), 2
    L = 67 if form == GROUPED else _crossover(lib, Hq, Hkv) + 1
    assert dk._form(lib, Hq, Hkv, L)[0] == form
    samples = [0, -1, 1, R, 0, 2 ** 31 - 1, 1, 1, -(2 ** 31)]
    keys = [5, 5, 0, 5, -7, 5, L + 9, 2 ** 31 - 1, 0]
    Q = len(samples)
    q, K, V, scale, vscale = _inputs(Q, R, Hq, Hkv, L, False, seed=7 + Hq + L)
    d = _Dev(q, K, V)
    hi, lo = _launch_rows(lib, d, list(range(Q)), samples, keys, scale, vscale, False)      # asserts the guard rows
    valid = [r for r in range(Q) if 0 <= samples[r] < R]
    for r in range(Q):
        if r not in valid:
            assert (hi[r] == 0).all() and (lo[r] == 0).all(), r
    clamped = [min(max(keys[r], 1), L) for r in valid]
    h2, l2 = _launch_rows(lib, d, valid, [samples[r] for r in valid], clamped, scale, vscale, False)
    ref = _reference_rows(q[valid], K, V, [samples[r] for r in valid], clamped, scale, vscale)
    for i, r in enumerate(valid):
        assert torch.equal(hi[r], h2[i]) and torch.equal(lo[r], l2[i]), r
    r_sum, r_lo = dk._ratios(1, (_values(h2), _values(l2)), ref)
    assert r_sum <= 1.0 and r_lo <= 1.0, (r_sum, r_lo)


def test_refusals_launch_nothing():
    lib = dk._lib()
    x = torch.zeros(4 * HD, dtype=torch.float32, device="cuda")
    i1 = torch.ones(1, dtype=torch.int32, device="cuda")
    out = torch.full((2, HD), 3.0, dtype=torch.bfloat16, device="cuda")
    p, st = x.data_ptr(), dk._stream()

    def call(q=p, k=p, v=p, rs=i1.data_ptr(), rk=i1.data_ptr(), o=out.data_ptr(), plane=HD, Q=1, R=1, Hq=1, Hkv=1, L=4):
        return lib.vqs_debug_qwen_rows_attention(q, k, v, rs, rk, o, plane, Q, R, Hq, Hkv, L, dk.SCALE, 0, 1.0, st)

    assert call(Q=0) == INVALID and call(R=0) == INVALID and call(L=36865) == INVALID and call(Hq=3, Hkv=2) == INVALID
    assert call(plane=HD - 1) == INVALID                    # the lo plane would overlap the hi plane
    for name in ("q", "k", "v", "rs", "rk", "o"):
        assert call(**{name: None}) == INVALID, name
    torch.cuda.synchronize()
    assert (out == 3.0).all()
