"""Single launches of the GEMM epilogues that only the Qwen2.5-VL row reaches (-m gpu), through the hook vqs_debug_gemm_launch: the head-major
scatter with 128-lane heads, narrow heads in wide slots (hd_src), grouped-query k / v tensors (inner_kv / Hkv), the scaled fp16 families, the
rotary embedding inside the epilogue, the slim form's head geometry, the SiLU gate and the gated bias in packed column order -- gemm_quad.inc
quad_epilogue_all / quad_epilogue_rows, the EPI_HEADS branch of gemm_slim.inc and the generalised staged epilogue of gemm.hip.

  (a) test_exact_*       integer operands: every result is exact in fp32, the expected buffers (tests/gemm_epilogue_cases.py: views of the dense
                         product, sentinel wherever nothing may be written) are compared bit for bit, guard regions and pad lanes included
  (b) test_arithmetic_*  random operands against an fp64 reference under the per-launch criterion of tests/test_gpu_qwen.py (one own ulp; 0.5 % /
                         2 % of the elements different at all); each case's figures go to the suite's parity_e2e.jsonl record (tests/test_gpu_e2e.py)
                         under gemm_epilogues/
  (c) test_*refus*       the launches the hook or the launcher must refuse: VQS_ERR_INVALID and not one byte written
Every launch runs twice into freshly filled buffers.  tests/test_gemm_epilogue_inputs.py proves on the CPU that each case runs the kernel it
claims and that the expectations can fail."""
import pytest
import torch

from tests import gemm_epilogue_cases as gc
from tests.test_gpu_e2e import _record

pytestmark = pytest.mark.gpu

INVALID = -1


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a HIP device")
    from t2v_metrics_amd import engine
    engine.load_library()
    return engine


def _launch_heads(eng, x, c, fields=None, drop=()):
    """One launch of geometry x.g under configuration c into fresh sentinel buffers -> (return code, the three whole buffers on the CPU).
    fields: overrides of the launch's integers; drop: operand names withheld (their flags stay)."""
    f, t, bufs = gc.heads_launch_args(x, c, fields, drop, "cuda")
    rc = eng.gemm_launch(f, acc_scale=c.acc_scale, out_scale=c.out_scale, **t)
    torch.cuda.synchronize()
    return rc, [b.cpu() for b in bufs]


def _where(x, t, got, want):
    """The first element of tensor t that differs, in the tensor's own coordinates."""
    i = int(torch.nonzero(got != want)[0])
    j = i - gc.FRONT_GUARD
    n = gc.tensor_elems(x.g, t, x.B, x.S)
    if j < 0 or j >= n:
        return f"tensor {t}: guard element {j} (tensor has {n}) written: {int(got[i]) & 0xffff:#06x}"
    lane, s, h, b = j % x.g.hd, j // x.g.hd % x.S, j // (x.g.hd * x.S) % x.g.heads(t), j // (x.g.hd * x.S * x.g.heads(t))
    return (f"tensor {t} [b {b}, head {h}, pos {s}, lane {lane}]: {int(got[i]) & 0xffff:#06x} != {int(want[i]) & 0xffff:#06x}; "
            f"{int((got != want).sum())} elements differ")


def _assert_buffers(x, got, want, what):
    for t, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), f"{what}: {_where(x, t, a, b)}"


@pytest.mark.parametrize("name,S,cname", gc.EXACT_CASES, ids=["-".join(map(str, c)) for c in gc.EXACT_CASES])
def test_exact_scatter(eng, name, S, cname):
    g, c = gc.GEOMETRIES[name], gc.CONFIGS[cname]
    claim = gc.claimed_kernel(g, c)
    for B in gc.batches(S):
        x = gc.exact_inputs(name, S, B, c.K)
        what = f"{name} S={S} B={B} M={B * S} {cname}"
        if claim is None:                                    # refused by the launcher: nothing is written
            rc, got = _launch_heads(eng, x, c)
            assert rc == INVALID, what
            assert all(bool((b == gc.SENTINEL).all()) for b in got), what
            continue
        want = gc.expected_buffers(x, c)
        runs = []
        for _ in range(2):
            rc, got = _launch_heads(eng, x, c)
            assert rc == 0, what
            _assert_buffers(x, got, want, what)
            runs.append(got)
        if cname == "f16s-v10-unit":                         # both scales 1: bitwise the unscaled fp16 kernel
            rc, plain = _launch_heads(eng, x, c.but(type=gc.T_F16))
            assert rc == 0
            _assert_buffers(x, plain, runs[0], what + " against the type-1 launch")
        if c.rope:                                           # v is not rotated: bitwise the launch without tables
            rc, flat = _launch_heads(eng, x, c.but(rope=False))
            assert rc == 0
            assert torch.equal(flat[2], runs[0][2]), what + ": v differs from the no-rope launch"
            assert not torch.equal(flat[0], runs[0][0]) and not torch.equal(flat[1], runs[0][1])
        if c.variant == 3:                                   # the library's rule (slim; with rope: quad) against the quad kernel itself
            rc, quad = _launch_heads(eng, x, c.but(variant=10))
            assert rc == 0
            _assert_buffers(x, quad, runs[0], what + " against variant 10")


def _launch_plain(eng, case, fields=None, bias=None):
    """One launch of an arithmetic case into a fresh sentinel buffer -> (return code, whole buffer on the CPU as int16)."""
    f, t, buf = gc.plain_launch_args(case, fields, bias, "cuda")
    rc = eng.gemm_launch(f, acc_scale=case.acc_scale, out_scale=case.out_scale, **t)
    torch.cuda.synchronize()
    return rc, buf.cpu()


def _split_plain(case, buf):
    """-> (result [M, n_out] in the output type, everything else of the buffer with the result's own cells set to the sentinel)."""
    body = buf[gc.FRONT_GUARD:gc.FRONT_GUARD + case.M * case.ldc].view(case.M, case.ldc)
    out = body[:, :case.n_out].clone().view(gc.out_dtype(case.type))
    rest = buf.clone()
    rest[gc.FRONT_GUARD:gc.FRONT_GUARD + case.M * case.ldc].view(case.M, case.ldc)[:, :case.n_out] = gc.SENTINEL
    return out, rest


@pytest.mark.parametrize("case", gc.ARITH_CASES, ids=[c.name for c in gc.ARITH_CASES])
def test_arithmetic_epilogue(eng, case):
    ref = gc.arith_reference(case)
    outs = []
    for _ in range(2):
        rc, buf = _launch_plain(eng, case)
        assert rc == 0, case.name
        out, rest = _split_plain(case, buf)
        assert bool((rest == gc.SENTINEL).all()), f"{case.name}: a store outside the result (rows >= M, columns >= {case.n_out} or a guard)"
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), case.name
    assert bool(torch.isfinite(outs[0].float()).all()), case.name
    ok, r = gc.criterion(ref, outs[0], case.mant_bits)
    print(f"{case.name}: max_own_ulps {r['max_own_ulps']:.4f} frac_diff {r['frac_diff']:.6f}")
    _record("gemm_epilogues/" + case.name, {"max_own_ulps": r["max_own_ulps"], "frac_diff": r["frac_diff"], "mant_bits": case.mant_bits, "elements": r["n"],
                        "limits": {"max_own_ulps": gc.MAX_OWN_ULPS, "frac_diff": gc.MAX_FRAC_DIFF[case.mant_bits]}})
    assert ok, (case.name, r)


def test_hook_refusals_write_nothing(eng):
    rc, got = _launch_heads(eng, gc.exact_inputs("gqa31", 8, 17, 128), gc.CONFIGS["f16s-v10-rope-unit"])
    assert rc == 0                                           # the launch the refusals are one change away from
    for what, name, S, B, cname, fields, drop in gc.HEADS_REFUSALS:
        rc, got = _launch_heads(eng, gc.exact_inputs(name, S, B, 128), gc.CONFIGS[cname], fields, drop)
        assert rc == INVALID, what
        assert all(bool((b == gc.SENTINEL).all()) for b in got), what


def test_plain_and_gated_refusals_write_nothing(eng):
    gated = gc.refusal_base_case()
    rc, buf = _launch_plain(eng, gated)
    assert rc == 0
    for what, fields, bias in gc.PLAIN_REFUSALS:
        rc, buf = _launch_plain(eng, gated, fields, bias)
        assert rc == INVALID, what
        assert bool((buf == gc.SENTINEL).all()), what
