"""Row lists of the Qwen2.5-VL row's teacher-forced scoring, without a GPU: layout.answer_rows against a brute-force enumeration, and
the refusals of vqs_qwen_score_rows / vqs_qwen_score_suffix_rows and their size queries, which come before any launch and so need
nothing but vqs_qwen_create."""
import ctypes

import pytest
import torch

from t2v_metrics_amd.qwen.layout import answer_rows

INVALID, STATE = -1, -5


def _brute(seq_len, n, L, offset):
    """Every (sample, position) pair of the padded batch that is one of the sample's last n_b valid positions, in batch order."""
    out = []
    for b in range(len(seq_len)):
        for p in range(offset, offset + L):
            if seq_len[b] - n[b] <= p < seq_len[b]:
                out.append((b * L + (p - offset), b, p + 1))
    return out


@pytest.mark.parametrize("offset", [0, 32])
def test_answer_rows_equals_the_brute_force_enumeration(offset):
    g = torch.Generator().manual_seed(11 + offset)
    for _ in range(200):
        B = int(torch.randint(1, 7, (1,), generator=g))
        L = int(torch.randint(1, 40, (1,), generator=g))
        seq = [offset + int(torch.randint(1, L + 1, (1,), generator=g)) for _ in range(B)]
        n = [int(torch.randint(1, s - offset + 1, (1,), generator=g)) for s in seq]          # 1 .. the whole tail of the pass
        idx, smp, keys = answer_rows(torch.tensor(seq), n, L, offset=offset)
        want = _brute(seq, n, L, offset)
        assert idx.dtype == smp.dtype == keys.dtype == torch.int32
        assert list(zip(idx.tolist(), smp.tolist(), keys.tolist())) == want
        assert idx.numel() == sum(n) and int(idx.max()) < B * L and int(keys.max()) <= offset + L and int(keys.min()) > offset
    # one count for every sample; one row per sample is the last-row map of text_layout / shared_prefix_plan
    idx, smp, keys = answer_rows([offset + 5, offset + 9], 1, 12, offset=offset)
    assert idx.tolist() == [4, 12 + 8] and smp.tolist() == [0, 1] and keys.tolist() == [offset + 5, offset + 9]
    idx, _, _ = answer_rows(torch.tensor([offset + 5, offset + 9]), 3, 12, offset=offset)
    assert idx.tolist() == [2, 3, 4, 18, 19, 20]


def test_answer_rows_refuses_rows_outside_the_pass():
    # more rows than the sequence has; no row; a sequence longer than the pass; rows that reach into the shared prefix; a sequence that ends in it
    for seq, n, L, off in [([5], 6, 8, 0), ([5], 0, 8, 0), ([9], 1, 8, 0), ([40], 9, 16, 32), ([31], 1, 16, 32)]:
        with pytest.raises(ValueError):
            answer_rows(seq, n, L, offset=off)
    with pytest.raises(ValueError):
        answer_rows([5, 6], [1, 2, 3], 8)


@pytest.fixture(scope="module")
def handle():
    from t2v_metrics_amd import engine
    from t2v_metrics_amd.qwen import engine as qengine
    from t2v_metrics_amd.qwen import get_qwen_config
    lib = engine.load_library()
    for name, (res, args) in qengine._SIGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    cfg = get_qwen_config("qwen-tiny")
    v, t = cfg.vision, cfg.text
    mask = 0
    for i in v.fullatt_blocks:
        mask |= 1 << i
    c = qengine.VqsQwenConfig(v.depth, v.hidden, v.heads, v.mlp, v.patch_dim, v.merge_unit, v.out_hidden, mask, v.rms_eps,
                              t.vocab, t.hidden, t.layers, t.heads, t.kv_heads, t.mlp, t.rms_eps)
    h = ctypes.c_void_p()
    assert lib.vqs_qwen_create(ctypes.byref(c), ctypes.byref(h)) == 0
    yield lib, h
    lib.vqs_qwen_destroy(h)


P = 0x1000          # a non-null address that is never dereferenced: every call below is refused before any launch


def _score_rows(lib, h, B=2, L=40, Q=3, rows=(P, P, P), other=P):
    return lib.vqs_qwen_score_rows(h, other, P, P, P, P, P, B, L, rows[0], rows[1], rows[2], Q, P, P, 1 << 40, None)


def _suffix_rows(lib, h, B=2, Lp=32, Ls=8, U=1, Q=3, rows=(P, P, P)):
    return lib.vqs_qwen_score_suffix_rows(h, P, P, P, P, P, P, P, B, Lp, Ls, P, U, 1 << 40, rows[0], rows[1], rows[2], Q, P, P, 1 << 40, None)


def test_row_list_entry_points_refuse_before_any_launch(handle):
    lib, h = handle
    # a well-formed call gets as far as "weights not bound": the argument checks are what the other calls stop at
    assert _score_rows(lib, h) == STATE and b"not bound" in lib.vqs_qwen_last_error(h)
    assert _suffix_rows(lib, h) == STATE
    for kw in (dict(Q=0), dict(Q=-4), dict(Q=2 * 40 + 1), dict(B=0), dict(L=0), dict(rows=(None, P, P)), dict(rows=(P, None, P)), dict(rows=(P, P, None))):
        assert _score_rows(lib, h, **kw) == INVALID, kw
    for kw in (dict(Q=0), dict(Q=2 * 8 + 1), dict(B=0), dict(Lp=33), dict(Lp=0), dict(Ls=7), dict(U=0), dict(Lp=36864, Ls=8),
               dict(rows=(None, P, P)), dict(rows=(P, None, P)), dict(rows=(P, P, None))):
        assert _suffix_rows(lib, h, **kw) == INVALID, kw
    # the precise tail is what evaluates a row list
    assert lib.vqs_qwen_debug_option(h, b"tail_precise", 0) == 0
    try:
        assert _score_rows(lib, h) == INVALID and b"tail_precise" in lib.vqs_qwen_last_error(h)
        assert _suffix_rows(lib, h) == INVALID and b"tail_precise" in lib.vqs_qwen_last_error(h)
    finally:
        assert lib.vqs_qwen_debug_option(h, b"tail_precise", 1) == 0
    assert _score_rows(lib, h) == STATE


def test_row_list_workspace_queries(handle):
    lib, h = handle
    one = lib.vqs_qwen_score_workspace_bytes(h, 3, 40)
    assert lib.vqs_qwen_score_rows_workspace_bytes(h, 3, 40, 3) == one > 0          # Q = B: today's layout
    assert lib.vqs_qwen_score_rows_workspace_bytes(h, 3, 40, 15) > one              # the tail state grows with Q
    assert lib.vqs_qwen_score_rows_workspace_bytes(h, 3, 40, 100) > lib.vqs_qwen_score_rows_workspace_bytes(h, 3, 40, 64)
    for B, L, Q in [(0, 40, 1), (3, 0, 1), (3, 40, 0), (3, 40, -1), (3, 40, 121)]:
        assert lib.vqs_qwen_score_rows_workspace_bytes(h, B, L, Q) == 0, (B, L, Q)
    assert lib.vqs_qwen_suffix_rows_workspace_bytes(h, 3, 32, 8, 3) == lib.vqs_qwen_suffix_workspace_bytes(h, 3, 32, 8) > 0
    assert lib.vqs_qwen_suffix_rows_workspace_bytes(h, 3, 32, 8, 20) > lib.vqs_qwen_suffix_workspace_bytes(h, 3, 32, 8)
    for B, Lp, Ls, Q in [(0, 32, 8, 1), (3, 31, 8, 1), (3, 32, 7, 1), (3, 32, 8, 0), (3, 32, 8, 25)]:
        assert lib.vqs_qwen_suffix_rows_workspace_bytes(h, B, Lp, Ls, Q) == 0, (B, Lp, Ls, Q)
