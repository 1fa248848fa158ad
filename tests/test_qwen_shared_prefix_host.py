"""Host side of the Qwen2.5-VL row's shared prompt prefix (no GPU): the prefix / suffix split of the prompts, the shared-prefix plan
against the unshared text layout, and the size queries of include/vqs_qwen.h."""
import ctypes

import pytest
import torch

from t2v_metrics_amd.models.vqascore_models.qwen25vl_model import Qwen25VLModel
from t2v_metrics_amd.qwen import get_qwen_config
from t2v_metrics_amd.qwen.layout import shared_prefix_plan, split_prompt_ids, text_layout
from tests.test_qwen_host import FakeQwenTokenizer, OracleQwenEngine

QUESTIONS = ["", " leading space", 'a "quoted" phrase', "café naïve 日本語 \U0001f600", "long " * 200,
             "a person waves", "Does it?"]


def _model(name="qwen-tiny"):
    cfg = get_qwen_config(name)
    return Qwen25VLModel(model_name="qwen2.5-vl-7b", device="cpu", config=cfg, engine=object(), tokenizer=FakeQwenTokenizer(cfg.text.vocab))


@pytest.mark.parametrize("kind", ["image", "video"])
def test_split_reassembles_build_ids_and_the_prefix_is_shared(kind):
    m = _model()
    prefixes = set()
    for q in QUESTIONS:
        ids = m.build_ids(q, kind, 40)
        pre, suf = m.split_prompt(ids)
        assert pre + suf == ids
        assert pre[-1] == m.cfg.vision_end_token_id and m.cfg.vision_end_token_id not in suf
        prefixes.add(tuple(pre))
    assert len(prefixes) == 1


def test_split_refuses_a_prompt_without_one_vision_end():
    with pytest.raises(ValueError):
        split_prompt_ids([1, 2, 3], 7)
    with pytest.raises(ValueError):
        split_prompt_ids([7, 1, 7], 7)


def _batch(m, questions, media, n_tok):
    rows = [m.build_ids(q, "video", n_tok) for q in questions]
    B, L = len(rows), max(len(r) for r in rows)
    ids = torch.zeros(B, L, dtype=torch.long)
    mask = torch.zeros(B, L, dtype=torch.long)
    for k, r in enumerate(rows):
        ids[k, : len(r)] = torch.tensor(r)
        mask[k, : len(r)] = 1
    return ids, mask


def test_plan_is_the_unshared_layout_sliced():
    m = _model()
    cfg = m.cfg
    grid = (2, 8, 16)
    n_tok = 2 * 8 * 16 // 4
    qs = ["a", "b c d e", "f g", "h", "i j k l m n o"]
    media = ["v1", "v0", "v1", "v1", "v2"]
    ids, mask = _batch(m, qs, media, n_tok)
    B, L = ids.shape
    plan = shared_prefix_plan(cfg, ids, mask, [grid] * B, media)
    lay = text_layout(cfg, ids, mask, [grid] * B)
    Lp, Ls, U = plan["Lp"], plan["Ls"], plan["U"]
    split = len(m.split_prompt(m.build_ids("a", "video", n_tok))[0])
    assert Lp % 32 == 0 and Lp <= split < Lp + 32 and Lp + Ls == L and Ls >= 8
    assert U == 3 and plan["media_idx"].tolist() == [0, 1, 0, 0, 2] and plan["first"] == [0, 1, 4]
    assert torch.equal(plan["seq_len"], lay["seq_len"])
    assert torch.equal(plan["last_row"], (torch.arange(B) * Ls + lay["seq_len"] - 1 - Lp).to(torch.int32))
    half = lay["cos"].shape[1]
    cos, sin = lay["cos"].view(B, L, half), lay["sin"].view(B, L, half)
    assert torch.equal(plan["suffix_cos"], cos[:, Lp:].reshape(-1, half)) and torch.equal(plan["suffix_sin"], sin[:, Lp:].reshape(-1, half))
    fi = torch.tensor(plan["first"])
    assert torch.equal(plan["prefix_cos"], cos[fi, :Lp].reshape(-1, half)) and torch.equal(plan["prefix_sin"], sin[fi, :Lp].reshape(-1, half))
    assert torch.equal(plan["suffix_ids"], ids[:, Lp:].to(torch.int32)) and torch.equal(plan["prefix_ids"], ids[fi, :Lp].to(torch.int32))
    assert torch.equal(plan["suffix_vis_slot"], lay["vis_slot"][:, Lp:])
    # prefix slots index the U media's merged tokens: medium u's run is rows u*n_tok ..
    pv = plan["prefix_vis_slot"]
    for u in range(U):
        v = pv[u][pv[u] >= 0]
        assert torch.equal(v, torch.arange(u * n_tok, u * n_tok + v.numel(), dtype=torch.int32))
    assert torch.equal(plan["next_pos"], lay["next_pos"])


def test_plan_is_none_when_no_medium_repeats_or_the_prefix_is_short():
    m = _model()
    ids, mask = _batch(m, ["a", "b"], ["x", "y"], 64)
    assert shared_prefix_plan(m.cfg, ids, mask, [(2, 8, 16)] * 2, ["x", "y"]) is None
    ids, mask = _batch(m, ["a", "b"], ["x", "x"], 8)          # 11 header + 8 vision + 1 rows: below one 32-row wave
    assert shared_prefix_plan(m.cfg, ids, mask, [(1, 4, 8)] * 2, ["x", "x"]) is None


def test_plan_refuses_samples_of_one_medium_with_different_prefixes():
    m = _model()
    ids, mask = _batch(m, ["a", "b"], ["x", "x"], 64)
    ids[1, 3] = 99
    with pytest.raises(AssertionError):
        shared_prefix_plan(m.cfg, ids, mask, [(2, 8, 16)] * 2, ["x", "x"])


def test_engines_without_the_shared_path_keep_todays_path(tmp_path):
    """share_prefix defaults on; an engine without score_shared (here the fp32 CPU oracle) takes today's path: the same engine calls
    and the same scores as share_prefix=False, for several questions about one medium."""
    import numpy as np
    import t2v_metrics_amd as t2v
    from t2v_metrics_amd.qwen.weights import make_seeded_qwen_weights
    cfg = get_qwen_config("qwen-tiny")
    w = make_seeded_qwen_weights(cfg, seed=3)
    rng = np.random.RandomState(1)
    paths = []
    for i, shape in enumerate([(2, 56, 112, 3), (112, 112, 3)]):      # two grids
        p = tmp_path / f"m{i}.npy"
        np.save(p, rng.randint(0, 256, shape, dtype=np.uint8))
        paths.append(str(p))
    images, texts = [paths[0]] * 3 + [paths[1]] * 2, ["a", "b c", "d e f", "g", "h i"]
    out = {}
    for share in (True, False):
        eng = OracleQwenEngine(cfg, w)
        calls = []
        real = eng.score_logits
        eng.score_logits = lambda *a, **k: calls.append(a[1].shape) or real(*a, **k)
        s = t2v.VQAScore(model="qwen2.5-vl-7b", device="cpu", config=cfg, engine=eng, tokenizer=FakeQwenTokenizer(cfg.text.vocab), share_prefix=share)
        assert s.model.share_prefix is share
        out[share] = (s.model.forward(images, texts), calls)
    assert Qwen25VLModel.__init__.__defaults__[-1] is True
    assert out[True][1] == out[False][1] and len(out[True][1]) == 2          # one prefill per grid, as before
    assert torch.equal(out[True][0], out[False][0])


def test_size_queries_are_arithmetic_and_refuse_invalid_sizes():
    from t2v_metrics_amd import engine
    from t2v_metrics_amd.qwen import engine as qengine
    lib = engine.load_library()
    for name, (res, args) in qengine._SIGS.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    c = qengine.VqsQwenConfig(32, 1280, 16, 3420, 1176, 4, 3584, (1 << 7) | (1 << 15) | (1 << 23) | (1 << 31), 1e-6,
                              152064, 3584, 28, 28, 4, 18944, 1e-6)
    h = ctypes.c_void_p()
    assert lib.vqs_qwen_create(ctypes.byref(c), ctypes.byref(h)) == 0
    try:
        # per layer K and V, [U, kv_heads, Lp, 128] bf16: 57 344 bytes per prefix token at 7B
        assert lib.vqs_qwen_prefix_kv_bytes(h, 8, 768) == 2 * 28 * 8 * 4 * 768 * 128 * 2
        assert lib.vqs_qwen_prefix_kv_bytes(h, 1, 32) == 57344 * 32
        for U, Lp in [(0, 768), (8, 0), (8, 770), (8, 16), (1, 36864 + 32)]:
            assert lib.vqs_qwen_prefix_kv_bytes(h, U, Lp) == 0
            assert lib.vqs_qwen_prefix_workspace_bytes(h, U, Lp) == 0
        assert lib.vqs_qwen_prefix_workspace_bytes(h, 8, 768) >= lib.vqs_qwen_score_workspace_bytes(h, 8, 768)
        assert lib.vqs_qwen_suffix_workspace_bytes(h, 64, 768, 40) > lib.vqs_qwen_score_workspace_bytes(h, 64, 808)
        for B, Lp, Ls in [(0, 768, 40), (64, 770, 40), (64, 768, 7), (64, 36864 - 32, 40)]:
            assert lib.vqs_qwen_suffix_workspace_bytes(h, B, Lp, Ls) == 0
        # shapes are refused with VQS_ERR_INVALID before anything else is looked at (here: a handle without weights, null buffers)
        INVALID, STATE = -1, -5
        n = ctypes.c_void_p(0)
        for U, Lp in [(1, 48), (0, 64), (1, 16), (1, 36864 + 32)]:
            assert lib.vqs_qwen_prefix(h, n, n, n, n, n, U, Lp, n, 0, n, 0, None) == INVALID
        assert lib.vqs_qwen_prefix(h, n, n, n, n, n, 1, 64, n, 0, n, 0, None) == STATE          # a valid shape gets past the size check
        for B, Lp, Ls in [(4, 48, 40), (4, 64, 7), (4, 36864 - 32, 40), (0, 64, 40)]:
            args = [h] + [n] * 8 + [B, Lp, Ls, n, 1, 0, n, n, 0]
            assert lib.vqs_qwen_score_suffix(*args, None) == INVALID
            assert lib.vqs_qwen_prefill_suffix(*args, n, 0, Lp + Ls + 2, None) == INVALID
        args = [h] + [n] * 8 + [4, 64, 40, n, 1, 0, n, n, 0]
        assert lib.vqs_qwen_prefill_suffix(*args, n, 0, 36864 + 1, None) == INVALID                # a cache past the decode kernel's limit
        assert lib.vqs_qwen_score_suffix(*args, None) == STATE
    finally:
        lib.vqs_qwen_destroy(h)
