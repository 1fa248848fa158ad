"""tests/test_gpu_precise_decoder_kernels.py without a GPU: every case of that file -- its own generators, references, criteria and
assertions -- run over the fp32 CPU restatement of the kernels (tests/precise_decoder_fp32.py) in place of the library's hooks.  Two things
are shown.  A correct fp32 implementation passes every case, so no case asks for more than fp32 arithmetic in the documented order can give
(a bound too tight, a wrong reference or a wrong stride in a test would show here, not first on an MI355X).  And the checks discriminate:
seven copies of the restatement, each with one planted mistake (a lo plane stored over the hi plane, the linear operand 16 instead of 32
columns after the gate, the slice loop starting at 2, no max subtraction in the softmax, one key past key_len kept, the argmax tie-break
reversed, the causal mask without the cache offset), each fail the cases named for them below."""
import itertools

import pytest
import torch

import tests.test_gpu_precise_decoder_kernels as G
from tests.precise_decoder_fp32 import Fp32Kernels


def _cases(fn):
    """Every parameter combination of a test function of the GPU file, from its parametrize marks."""
    axes = []
    for m in getattr(fn, "pytestmark", []):
        if m.name == "parametrize":
            names = [n.strip() for n in m.args[0].split(",")]
            axes.append([dict(zip(names, v if len(names) > 1 else (v,))) for v in m.args[1]])
    for combo in itertools.product(*axes):
        kw = {}
        for d in combo:
            kw.update(d)
        yield kw


ALL = [(name, kw) for name in sorted(dir(G)) if name.startswith("test_") for kw in _cases(getattr(G, name))]


@pytest.fixture
def on_cpu(monkeypatch):
    """The GPU file's device plumbing on the host: .cuda() is a copy (the tests compare inputs before and after a launch), the stream is 0."""
    from t2v_metrics_amd import engine

    def use(mutation=0):
        k = Fp32Kernels(mutation)
        monkeypatch.setattr(G, "_lib", lambda: k)
        monkeypatch.setattr(engine, "load_library", lambda path=None: k)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **kw: self.clone())
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: None)
    monkeypatch.setattr(G, "_stream", lambda: 0)
    monkeypatch.setattr(engine, "_stream_ptr", lambda: 0)
    monkeypatch.setattr(G, "_record", lambda name, payload: None)
    return use


def test_the_gpu_file_has_the_cases_this_file_expects():
    assert len(ALL) == 183 and len({n for n, _ in ALL}) >= 20


@pytest.mark.parametrize("name,kw", ALL, ids=[n[5:] + "-" + "-".join(str(v) for v in kw.values()) for n, kw in ALL])
def test_fp32_restatement_passes_every_case(on_cpu, name, kw):
    on_cpu(0)
    getattr(G, name)(**kw)


# mutation -> the test functions of the GPU file that launch the mutated kernel; at least the listed one must fail
MUTATIONS = {
    1: ("the lo plane of sum_planes' split store lands on the hi plane", ["test_sum_planes", "test_sum_planes_with_tight_pitches"], "test_sum_planes"),
    2: ("the gated form reads its linear operand at gc + 16", ["test_sum_planes", "test_gated_activation_tails", "test_reduce_slices_act"], "test_sum_planes"),
    3: ("the slice loop starts at k = 2", ["test_sum_planes", "test_reduce_slices_act"], "test_reduce_slices_act"),
    4: ("masked_softmax without the max subtraction", ["test_masked_softmax"], "test_masked_softmax"),
    5: ("masked_softmax keeps key j == key_len", ["test_masked_softmax"], "test_masked_softmax"),
    6: ("the argmax reduction prefers the higher index on a tie", ["test_argmax_append"], "test_argmax_append"),
    7: ("the causal mask ignores qpos0", ["test_dec_attn_cached_form", "test_dec_attn_self_form_at_the_row_limit"], "test_dec_attn_cached_form"),
}


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_each_planted_mistake_is_caught(on_cpu, mutation):
    what, names, must = MUTATIONS[mutation]
    on_cpu(mutation)
    caught = []
    for name, kw in ALL:
        if name in names:
            try:
                getattr(G, name)(**kw)
            except AssertionError:
                caught.append((name, kw))
    print(f"mutation {mutation} ({what}): {len(caught)} cases fail:", sorted({n for n, _ in caught}))
    assert any(n == must for n, _ in caught), (mutation, what, caught)
