"""The GEMM dispatch rule (gemm.hip gemm_plan) through its host-side hook vqs_debug_gemm_plan: no GPU needed.

tests/golden/gemm_plan_parent.json pins what the launcher did BEFORE the rule was gathered into one function: one line per corner of the rule
(tools/launch_sequence.py GEMM_CASES), each the launch as integers and the kernel, workgroup count and workgroup size that a kernel trace of
the previous launcher showed for it on an MI355X (profiles/gemm_dispatch_sequence.md).  The kernels of one family produce the same bits, so
the bitwise GPU tests cannot see a launch move between lock-step, ping-pong and touch; this test can.  The refusals are the launcher's
`return hipErrorInvalidValue` lines, one launch each, next to the accepted launch they were derived from by changing one field."""
import ctypes
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_plan_parent.json")
FIELDS = ("M", "N", "K", "lda", "ldw", "ldc", "epi", "batch", "variant", "S", "inner", "inner_kv", "hd", "hd_src", "Hkv", "type", "l2_touch", "split_off",
          "flags", "gate_act", "rowss_parts", "ldh")
BIAS, ROWSS, NO_STREAM, ROPE_COS, ROPE_SIN, RMS, HANDLE = 1, 2, 4, 8, 16, 32, 64
TILE, TILE_PP, PERSISTENT, PINGPONG, STREAM, QUAD, SLIM = range(7)
QUAD_NAMES = ("gemm_bf16_quad", "gemm_f16_quad", "gemm_f16b_quad", "gemm_f16s_quad", "gemm_f16bs_quad")


def plan(launch):
    from t2v_metrics_amd import engine
    assert len(launch) == len(FIELDS)
    arr, out = (ctypes.c_int32 * len(FIELDS))(*launch), (ctypes.c_int32 * 5)()
    rc = engine.load_library().vqs_debug_gemm_plan(ctypes.cast(arr, ctypes.c_void_p), len(FIELDS), ctypes.cast(out, ctypes.c_void_p))
    assert rc in (0, 1), rc
    return tuple(out) if rc == 1 else None


def launch(M, N, K, epi, **kw):
    d = dict.fromkeys(FIELDS, 0)
    d.update(M=M, N=N, K=K, lda=K, ldw=K, ldc=N, epi=epi, batch=1, variant=3, S=1, inner=1)
    assert set(kw) <= set(FIELDS), kw
    d.update(kw)
    return [d[f] for f in FIELDS]


def kernel_name(p, epi):
    """The trace's name of the kernel a plan instantiates."""
    kernel, touch, typ = p[:3]
    name = {TILE: f"gemm_bf16_kernel<{epi}, 0>", TILE_PP: f"gemm_bf16_kernel<{epi}, 2>", PERSISTENT: f"gemm_bf16_persistent<{epi}, {touch}, {typ}>",
            PINGPONG: f"gemm_bf16_pingpong<{epi}>", STREAM: f"gemm_bf16_stream<{epi}, {typ}>", QUAD: f"{QUAD_NAMES[typ]}<{epi}>",
            SLIM: f"gemm_slim<{epi}, {typ}>"}[kernel]
    return f"void vqs::{name}(vqs::GemmParams)"


with open(GOLDEN) as _f:
    PARENT = [json.loads(line) for line in _f if line.strip()]


def test_the_fixture_covers_every_kernel_family_and_both_touch_forms():
    names = " ".join(c["kernel"] for c in PARENT)
    for word in ("gemm_bf16_kernel<0, 0>", "gemm_bf16_kernel<0, 2>", "gemm_bf16_persistent<3, 0, 0>", "gemm_bf16_persistent<3, 2, 0>", "gemm_bf16_persistent<3, 0, 1>",
                 "gemm_bf16_pingpong<3>", "gemm_bf16_stream<3, 0>", "gemm_bf16_stream<3, 1>", "gemm_bf16_quad<0>", "gemm_f16_quad<0>", "gemm_f16b_quad<5>",
                 "gemm_slim<0, 0>", "gemm_slim<0, 1>", "gemm_bf16_kernel<6, 0>", "gemm_bf16_kernel<4, 0>", "gemm_bf16_persistent<7, 0, 0>", "gemm_bf16_pingpong<7>"):
        assert word in names, word
    assert len(PARENT) >= 38


@pytest.mark.parametrize("case", PARENT, ids=[c["what"] for c in PARENT])
def test_plan_is_what_the_previous_launcher_launched(case):
    p = plan(case["launch"])
    assert p is not None, case
    assert (kernel_name(p, case["launch"][FIELDS.index("epi")]), p[3], p[4]) == (case["kernel"], case["workgroups"], case["workgroup_size"]), (case, p)


# (accepted launch, the same launch with one field changed: refused) -- one pair for each refusal of the launcher
REFUSALS = [
    ("rope needs both tables", launch(256, 3 * 128, 256, 6, S=8, inner=128, hd=128, type=3, flags=ROPE_COS | ROPE_SIN), dict(flags=ROPE_COS)),
    ("rope: scaled fp16 family only", launch(256, 3 * 128, 256, 6, S=8, inner=128, hd=128, type=3, flags=ROPE_COS | ROPE_SIN), dict(type=1)),
    ("rope: whole 128-lane heads", launch(256, 3 * 128, 256, 6, S=8, inner=128, hd=128, type=3, flags=ROPE_COS | ROPE_SIN), dict(hd_src=80)),
    *[(f"lab variant {v}", launch(512, 512, 256, 0), dict(variant=v)) for v in (1, 4, 6, 7, 8, 9)],
    ("M > 0", launch(512, 512, 256, 0), dict(M=0)),
    ("K a multiple of 64", launch(512, 512, 256, 0), dict(K=288, lda=288, ldw=288)),
    ("N a multiple of 8", launch(512, 516, 256, 3, ldc=516), dict(epi=0)),
    ("ragged fp32 N needs room in ldc", launch(512, 518, 256, 3, ldc=520), dict(ldc=518)),
    ("ragged fp32 N takes no bias", launch(512, 516, 256, 3, ldc=516), dict(flags=BIAS)),
    ("a batch under variant 0", launch(256, 512, 256, 0, batch=4), dict(variant=0)),
    ("a batch under variant 2", launch(256, 512, 256, 0, batch=4), dict(variant=2)),
    ("a batch of head-major results", launch(256, 768, 256, 6, S=8, inner=256), dict(batch=2)),
    ("a batch of fp32 + residual", launch(256, 512, 256, 4), dict(batch=2)),
    ("lda a multiple of 8", launch(512, 512, 256, 0), dict(lda=260)),
    ("ldw a multiple of 8", launch(512, 512, 256, 0), dict(ldw=260)),
    ("split result: plain bf16 epilogue", launch(256, 512, 256, 0, split_off=4096), dict(epi=3)),
    ("split result: offset a multiple of 8", launch(256, 512, 256, 0, split_off=4096), dict(split_off=4100)),
    ("128-lane heads under variant 0", launch(256, 3 * 128, 256, 6, S=8, inner=128, hd=128), dict(variant=0)),
    ("grouped-query heads under variant 2", launch(256, 512, 256, 6, S=8, inner=256, inner_kv=128, Hkv=2, variant=11), dict(variant=2)),
    ("SiLU gate under variant 0", launch(256, 512, 256, 5, ldc=256, gate_act=1), dict(variant=0)),
    ("gated bias under variant 0", launch(256, 512, 256, 5, ldc=256, flags=BIAS), dict(variant=0)),
    ("row scale: parts >= 0", launch(512, 512, 256, 0, flags=ROWSS, rowss_parts=2), dict(rowss_parts=-1)),
    ("row scale under variant 2", launch(512, 512, 256, 0, flags=ROWSS, rowss_parts=2), dict(variant=2)),
    ("row scale on fp32 + residual", launch(512, 512, 256, 3, flags=ROWSS, rowss_parts=2), dict(epi=4)),
    ("residual + RMSNorm needs its operands", launch(512, 512, 256, 7, flags=RMS, ldh=512), dict(flags=0)),
    ("residual + RMSNorm takes no bias", launch(512, 512, 256, 7, flags=RMS, ldh=512), dict(flags=RMS | BIAS)),
    ("residual + RMSNorm takes no batch", launch(512, 512, 256, 7, flags=RMS, ldh=512), dict(batch=2)),
    ("residual + RMSNorm: ldh a multiple of 4", launch(512, 512, 256, 7, flags=RMS, ldh=512), dict(ldh=514)),
    ("residual + RMSNorm: ldc a multiple of 4", launch(512, 512, 256, 7, flags=RMS, ldh=512), dict(ldc=514)),
    ("residual + RMSNorm: 32-bit kernels only", launch(512, 4096, 10240, 7, flags=RMS, ldh=4096), dict(M=400000)),
    ("epilogue 8", launch(512, 512, 256, 7, flags=RMS, ldh=512), dict(epi=8)),
    ("epilogue -1", launch(512, 512, 256, 0), dict(epi=-1)),
    ("fp16 result has no gated kernel", launch(256, 512, 256, 5, ldc=256, type=2), dict(type=1)),
    ("fp16 -> bf16 has plain and gated kernels only", launch(256, 512, 256, 0, type=2), dict(epi=1)),
    ("scaled fp16 has no quick-GELU kernel", launch(256, 512, 256, 2, type=3), dict(epi=1)),
    ("scaled fp16 -> bf16 has the plain kernel only", launch(256, 512, 256, 0, type=4), dict(epi=5, ldc=256)),
    ("scaled fp16: quad family only", launch(256, 512, 256, 0, type=3), dict(epi=3)),
    ("fp16 off the quad family: variant 3 only", launch(256, 256, 64, 3, type=1), dict(variant=11)),
    ("fp16 off the quad family: plain results only", launch(256, 256, 64, 3, type=1), dict(epi=4)),
    ("fp16 off the quad family: no bias", launch(256, 256, 64, 3, type=1), dict(flags=BIAS)),
    ("fp16 off the quad family: no row scale", launch(256, 256, 64, 0, type=2), dict(flags=ROWSS)),
    ("fp16 result: no split", launch(256, 512, 256, 0, type=2, batch=4, split_off=4 * 256 * 512), dict(type=1)),
    ("fp16 on the 8-wave kernel: 32-bit kernels only", launch(209715, 4096, 10240, 3, type=1), dict(M=209716)),
    ("narrow heads in wide slots: quad family only", launch(256, 3 * 128, 256, 6, S=8, inner=128, hd=128, hd_src=80), dict(variant=11)),
    ("a batch of 4 GiB entries", launch(209715, 4096, 10240, 3, batch=2), dict(M=209716)),
    ("tile variants: plain launches only", launch(512, 512, 256, 0, variant=0), dict(hd_src=32)),
    ("S < 8 heads: plain launches only", launch(256, 768, 256, 6, S=4, inner=256), dict(inner_kv=128, Hkv=2)),
    ("operand type 5", launch(512, 512, 256, 0, type=4), dict(type=5)),
]


@pytest.mark.parametrize("what,ok,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_of_the_launcher(what, ok, change):
    assert plan(ok) is not None, what
    bad = dict(zip(FIELDS, ok))
    bad.update(change)
    assert plan([bad[f] for f in FIELDS]) is None, what


def test_batched_launches_of_a_handle_follow_the_library_rule():
    """vqs_host.h run_gemm: the option gemm_variant speaks for unbatched launches; only the 8-wave and stream kernels take a batch."""
    for v in (0, 2, 3, 5, 11):
        assert plan(launch(128, 608, 4096, 3, batch=4, variant=v, flags=HANDLE)) == plan(launch(128, 608, 4096, 3, batch=4)) == (STREAM, 0, 0, 20, 256)
        assert plan(launch(256, 512, 256, 0, batch=4, variant=v, flags=HANDLE)) == (PERSISTENT, 0, 0, 8, 512)
        assert plan(launch(512, 512, 256, 0, variant=v, flags=HANDLE)) == plan(launch(512, 512, 256, 0, variant=v))
    assert plan(launch(256, 512, 256, 0, batch=4, variant=5)) == (PINGPONG, 0, 0, 8, 512)      # a bare launch keeps its variant


def test_scaled_families_and_rope_run_the_quad_kernels():
    """Only the Qwen2.5-VL handle launches these (its launch-sequence record covers them on the GPU); from the launcher's source."""
    qkv = dict(S=8, inner=3584, inner_kv=512, hd=128, Hkv=4, type=3)
    assert plan(launch(1024, 3584 + 1024, 3584, 6, **qkv, flags=ROPE_COS | ROPE_SIN | BIAS)) == (QUAD, 0, 3, 4 * 18, 256)
    assert plan(launch(64, 3584 + 1024, 3584, 6, **qkv)) == (QUAD, 0, 3, 18, 256)                 # type 3 has no slim kernel
    assert plan(launch(1024, 3584, 3584, 0, type=4)) == (QUAD, 0, 4, 4 * 14, 256)
    assert plan(launch(1024, 2 * 18944, 3584, 5, ldc=18944, gate_act=1, type=3)) == (QUAD, 0, 3, 256, 256)


def test_gemm_form_is_a_read_of_the_plan():
    from t2v_metrics_amd import engine
    lib = engine.load_library()
    form = {TILE: 0, TILE_PP: 0, PERSISTENT: 3, PINGPONG: 3, STREAM: 12, QUAD: 10, SLIM: 13}
    for M, N, K, epi, batch, v in ((608, 4096, 4096, 0, 1, 3), (608, 4096, 4096, 0, 1, 10), (128, 608, 4096, 3, 16, 3), (64, 384, 4096, 3, 1, 3),
                                   (400000, 4096, 10240, 3, 1, 3), (400000, 4096, 10240, 3, 2, 3), (512, 512, 256, 0, 1, 5), (512, 512, 256, 0, 1, 7)):
        p = plan(launch(M, N, K, epi, batch=batch, variant=v, S=0, inner=0))
        assert lib.vqs_debug_gemm_form(M, N, K, K, K, epi, batch, v, 0, 0, 0) == (form[p[0]] if p else -1)
