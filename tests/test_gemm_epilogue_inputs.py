"""CPU-side proof of tests/gemm_epilogue_cases.py: the exact expectations are exact (fp32 and fp64 evaluations give the same bits, nothing
subnormal or near the fp16 maximum), every case runs the kernel family it claims (vqs_debug_gemm_plan, the launcher's own rule) or is refused
as it claims, the offset-arithmetic restatement of the scatter agrees with the view / permute expectation, every planted mistake changes the
expected bits of every family it applies to, and the fp32 evaluation of the arithmetic references stays inside the criterion.  No GPU."""
import pytest
import torch

from tests import gemm_epilogue_cases as gc
from tests.test_gemm_plan import plan


def _shapes(g):
    return [(S, B) for S in g.S for B in gc.batches(S)]


def test_row_counts_cover_every_tile_position():
    for g in gc.GEOMETRIES.values():
        ms = sorted({S * B for S, B in _shapes(g)})
        assert any(m < 128 for m in ms) and any(128 < m < 256 for m in ms) and any(256 < m <= 256 + max(g.S) for m in ms) and any(m > 512 for m in ms), (g.name, ms)
        assert 256 in ms or all(256 % S for S in g.S), (g.name, ms)
        assert max(ms) <= 700, ms
    assert 264 in {S * B for g in gc.GEOMETRIES.values() for S, B in _shapes(g)}
    assert all(8 <= S for g in gc.GEOMETRIES.values() for S in g.S) and any(S < 16 for S in gc.GEOMETRIES["gqa31"].S)


@pytest.mark.parametrize("name,S,cname", gc.EXACT_CASES, ids=["-".join(map(str, c)) for c in gc.EXACT_CASES])
def test_exact_cases_are_exact_and_plan_as_claimed(name, S, cname):
    g, c = gc.GEOMETRIES[name], gc.CONFIGS[cname]
    claim = gc.claimed_kernel(g, c)
    for B in gc.batches(S):
        p = plan(gc.plan_list(gc.launch_fields(g, c, B, S)))
        assert (p[0] if p else None) == claim and (p is None or p[2] == c.type), (name, S, B, cname, p, claim)
        if claim is None:
            continue
        x = gc.exact_inputs(name, S, B, c.K)
        assert c.K <= 512 and x.A.abs().max() <= 2 and x.W.abs().max() <= 2 and x.bias.abs().max() <= 4
        e64, e32 = gc.expected_heads(x, c), gc.expected_heads(x, c, acc=torch.float32)
        assert all(torch.equal(a, b) for a, b in zip(e64, e32)), (name, S, B, cname)
        v = gc.expected_values(x, c)
        assert torch.equal(v, gc.expected_values(x, c, acc=torch.float32).double())
        mag = v.abs()
        assert float(mag.max()) <= 32768.0 and float(mag[mag > 0].min()) >= 2.0 ** -14, (float(mag.max()), float(mag[mag > 0].min()))
        assert not any(bool((o[..., :g.hsrc] == gc.SENTINEL).any()) for o in e64)            # no result has the sentinel's bits
        if c.rope:
            assert len({tuple(r.tolist()) for r in torch.cat([x.cos, x.sin], 1)}) == x.M      # a different table row for every GEMM row


def test_slim_and_staged_cases_cannot_silently_run_another_kernel():
    kernels = {(g.name, gc.claimed_kernel(g, c)) for g in gc.GEOMETRIES.values() for c in gc.configs_of(g)}
    for name in ("gqa31", "gqa42", "tower80", "half64"):
        assert {(name, gc.QUAD), (name, gc.SLIM)} <= kernels
    assert {("gqa31", gc.PERSISTENT), ("gqa42", gc.PERSISTENT), ("lm71", gc.PERSISTENT), ("tower80", None), ("half64", None), ("lm71", None)} <= kernels
    assert ("lm71", gc.QUAD) not in kernels and ("lm71", gc.SLIM) not in kernels


def test_the_restated_scatter_is_the_view_expectation():
    for name, S, cname in gc.EXACT_CASES:
        g, c = gc.GEOMETRIES[name], gc.CONFIGS[cname]
        if gc.claimed_kernel(g, c) is None or c.variant == 3:
            continue
        for B in gc.batches(S)[1:3]:
            x = gc.exact_inputs(name, S, B, c.K)
            assert all(torch.equal(a, b) for a, b in zip(gc.scatter_restated(x, c), gc.expected_flat(x, c))), (name, S, B, cname)


def _changes(name, cname, mistake):
    """Does the planted mistake change the expected bits of at least one shape of the geometry?"""
    g, c = gc.GEOMETRIES[name], gc.CONFIGS[cname]
    for S, B in _shapes(g):
        if B < 2:
            continue
        x = gc.exact_inputs(name, S, B, c.K)
        if not all(torch.equal(a, b) for a, b in zip(gc.scatter_restated(x, c, mistake), gc.expected_flat(x, c))):
            return True
    return False


# mistake -> (configuration it is planted under, the geometries -- one per kernel family -- it applies to)
PLANTED = {
    "kv_bases_swapped": ("bf16-v10-bias", ("gqa31", "gqa42", "tower80", "half64", "lm71")),
    "h_for_kv_wrap": ("bf16-v10-bias", ("gqa31", "gqa42", "lm71")),                              # grouped-query geometries: Hkv != H
    "head_by_hd": ("f16-v10-bias", ("tower80", "half64")),                                       # narrow heads in wide slots
    "late_sample_wrap": ("bf16-v10-bias", ("gqa31", "gqa42", "tower80", "half64", "lm71")),
    "rope_partner_32": ("f16s-v10-rope-bias-a8-o32", ("gqa31", "gqa42")),
    "rope_on_v": ("f16s-v10-rope-unit", ("gqa31", "gqa42")),
    "rope_row_by_position": ("f16s-v10-rope-bias-a8-o32", ("gqa31", "gqa42")),
    "bias_after_scale": ("f16s-v10-bias-a8-o32", ("gqa31", "gqa42", "tower80", "half64")),
}


def test_every_mistake_is_planted():
    assert set(PLANTED) == set(gc.SCATTER_MISTAKES + gc.ROPE_MISTAKES + gc.SCALE_MISTAKES)


@pytest.mark.parametrize("mistake", sorted(PLANTED))
def test_a_planted_mistake_changes_the_expected_bits(mistake):
    cname, names = PLANTED[mistake]
    for name in names:
        assert gc.claimed_kernel(gc.GEOMETRIES[name], gc.CONFIGS[cname]) is not None
        assert _changes(name, cname, mistake), (mistake, name)
    if mistake in gc.ROPE_MISTAKES:       # the slim-shaped launch with rope tables (the quad kernel under the library's rule) sees it too
        assert _changes("gqa31", "f16s-v3-k256-rope-bias", mistake)


@pytest.mark.parametrize("case", gc.ARITH_CASES, ids=[c.name for c in gc.ARITH_CASES])
def test_arithmetic_cases_plan_as_claimed_and_fp32_meets_the_criterion(case):
    p = plan(gc.plan_list(case.fields()))
    assert p is not None and p[0] == case.kernel and p[2] == case.type, (case.name, p)
    ref = gc.arith_reference(case)
    assert ref.shape == (case.M, case.n_out) and bool(torch.isfinite(ref.float()).all())
    ok, r = gc.criterion(ref, gc.arith_reference(case, acc=torch.float32), case.mant_bits)
    assert ok, (case.name, r)
    if case.epi == gc.EPI_GATED:          # the planted mistake: gate and linear columns swapped
        bad, r = gc.criterion(ref, gc.arith_reference(case, mistake="gate_linear_swapped"), case.mant_bits)
        assert not bad and r["max_own_ulps"] > 10.0, (case.name, r)


def test_deinterleave_is_the_inverse_of_the_packing():
    from tests.gpu_util import interleave_gate
    a, b = torch.arange(320.0 * 3).reshape(320, 3), -torch.arange(320.0 * 3).reshape(320, 3)
    g, l = gc.deinterleave_gate(interleave_gate(a, b).T)
    assert torch.equal(g.T, a) and torch.equal(l.T, b)


def test_the_arithmetic_cases_cover_what_the_issue_lists():
    have = {(c.epi, c.type, c.variant, c.M, c.bias, c.gate_act, c.out_scale != 1.0) for c in gc.ARITH_CASES}
    for M in (130, 300):
        for t in (gc.T_BF16, gc.T_F16_BF16, gc.T_F16S):
            assert {(gc.EPI_GATED, t, 10, M, False, 1, False), (gc.EPI_GATED, t, 10, M, True, 1, False)} <= have
        assert (gc.EPI_GATED, gc.T_F16S, 10, M, True, 1, True) in have and (gc.EPI_GATED, gc.T_BF16, 10, M, True, 0, False) in have
        assert {(gc.EPI_BF16, gc.T_F16S, 10, M, True, 0, True), (gc.EPI_GELU, gc.T_F16S, 10, M, True, 0, True), (gc.EPI_BF16, gc.T_F16S_BF16, 10, M, True, 0, True)} <= have


def _hook(f, t, scales=(1.0, 1.0)):
    from t2v_metrics_amd import engine
    import ctypes
    ints = (ctypes.c_int32 * len(engine.GEMM_LAUNCH_FIELDS))(*[int(f.get(n, 0)) for n in engine.GEMM_LAUNCH_FIELDS])
    ptrs = (ctypes.c_void_p * len(engine.GEMM_LAUNCH_PTRS))(*[None if t.get(n) is None else t[n].data_ptr() for n in engine.GEMM_LAUNCH_PTRS])
    sc = (ctypes.c_float * 4)(scales[0], scales[1], 0.0, 0.0)
    return engine.load_library().vqs_debug_gemm_launch(ctypes.cast(ints, ctypes.c_void_p), len(ints), ctypes.cast(ptrs, ctypes.c_void_p), len(ptrs),
                                                       ctypes.cast(sc, ctypes.c_void_p), 4, None)


def test_hook_and_launcher_refusals_need_no_device():
    """Every refusal the GPU test asserts is decided in host code before any device call: here on host tensors (nothing is launched, so nothing is
    read), with the hook's own return code.  The plan hook on the same integers agrees wherever the refusal is the launcher's."""
    from t2v_metrics_amd import engine
    assert engine.GEMM_LAUNCH_FIELDS == gc.PLAN_FIELDS + ("H",)
    for what, name, S, B, cname, fields, drop in gc.HEADS_REFUSALS:
        c = gc.CONFIGS[cname]
        f, t, bufs = gc.heads_launch_args(gc.exact_inputs(name, S, B, 128), c, fields, drop, "cpu")
        assert _hook(f, t, (c.acc_scale, c.out_scale)) == -1, what
        assert all(bool((b == gc.SENTINEL).all()) for b in bufs), what
    base = gc.refusal_base_case()
    for what, fields, bias in gc.PLAIN_REFUSALS:
        f, t, buf = gc.plain_launch_args(base, fields, bias, "cpu")
        assert _hook(f, t) == -1, what
        assert bool((buf == gc.SENTINEL).all()), what
    for what in ("hd = 128 under variant 0", "S = 7 with hd = 128", "one rope table only", "rope with hd_src = 80"):
        _, name, S, B, cname, fields, drop = next(r for r in gc.HEADS_REFUSALS if r[0] == what)
        f, _, _ = gc.heads_launch_args(gc.exact_inputs(name, S, B, 128), gc.CONFIGS[cname], fields, (), "cpu")
        assert plan(gc.plan_list(f)) is None, what
    assert plan(gc.plan_list(gc.plain_launch_args(base, dict(variant=0), None, "cpu")[0])) is None
    lib = engine.load_library()                               # bad calls of the hook itself
    f, t, _ = gc.plain_launch_args(base, None, None, "cpu")
    ok = [f.get(n, 0) for n in engine.GEMM_LAUNCH_FIELDS]
    import ctypes
    ints, ptrs, sc = (ctypes.c_int32 * 23)(*ok), (ctypes.c_void_p * 10)(), (ctypes.c_float * 4)(1, 1, 0, 0)
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)      # noqa: E731
    for args in ((None, 23, cast(ptrs), 10, cast(sc), 4), (cast(ints), 22, cast(ptrs), 10, cast(sc), 4), (cast(ints), 23, None, 10, cast(sc), 4),
                 (cast(ints), 23, cast(ptrs), 9, cast(sc), 4), (cast(ints), 23, cast(ptrs), 10, None, 4), (cast(ints), 23, cast(ptrs), 10, cast(sc), 3),
                 (cast(ints), 23, cast(ptrs), 10, cast(sc), 4)):                                 # the last: every pointer null
        assert lib.vqs_debug_gemm_launch(*args, None) == -1, args[1::2]
