"""Shared prompt prefix of the Qwen2.5-VL row on the MI355X (include/vqs_qwen.h vqs_qwen_prefix / vqs_qwen_score_suffix /
vqs_qwen_prefill_suffix, QwenEngine.score_shared): with sharing on, the logits, the processed step scores, the generated ids and the
final scores are BITWISE those of sharing off, for every small configuration, in the fp16 and the bf16 forms."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from t2v_metrics_amd.models.vqascore_models.qwen25vl_model import Qwen25VLModel
from t2v_metrics_amd.qwen import get_qwen_config
from t2v_metrics_amd.qwen.weights import make_seeded_qwen_weights
from tests.test_qwen_host import FakeQwenTokenizer

# ragged questions: the suffixes differ in length within one batch
QUESTIONS = ["a person waves", "a car turns left at the corner of a busy street", "red", "two dogs play in the snow near a fence"]
LONG = " ".join(f"w{i}" for i in range(150))       # a suffix of more than 128 rows: the suffix attention runs several 128-row blocks


def _media(tmp_path, rng):
    """two 4-frame videos, one 2-frame video, one image and one 10-frame video, all 112 x 224 (one grid per frame count; the 10-frame
    video's prompt splits after 172 rows: 160 shared rows, off the attention kernel's 128-row blocks)"""
    paths = []
    for i, shape in enumerate([(4, 112, 224, 3), (4, 112, 224, 3), (2, 112, 224, 3), (112, 224, 3), (10, 112, 224, 3)]):
        p = tmp_path / f"m{i}.npy"
        np.save(p, rng.randint(0, 256, shape, dtype=np.uint8))
        paths.append(str(p))
    return paths


def _model(name, seed=5):
    cfg = get_qwen_config(name)
    w = make_seeded_qwen_weights(cfg, seed=seed, dtype=torch.bfloat16, lm_head_gain=4.0)
    return Qwen25VLModel(model_name="qwen2.5-vl-7b", device="cuda", config=cfg, weights=w, tokenizer=FakeQwenTokenizer(cfg.text.vocab))


def _run(m, images, texts, max_new_tokens, share):
    m.share_prefix = share
    out = m._generate_scores(images, texts, None, 'Does this figure show "{}"? Please answer Yes or No.', "Yes", max_new_tokens)
    scores = m.forward(images, texts, max_new_tokens=max_new_tokens)
    return out, scores


def _assert_same(a, b):
    (out_a, s_a), (out_b, s_b) = a, b
    assert torch.equal(s_a, s_b), (s_a.tolist(), s_b.tolist())
    for (st_a, gen_a, _), (st_b, gen_b, _) in zip(out_a, out_b):
        assert gen_a == gen_b
        assert len(st_a) == len(st_b)
        for x, y in zip(st_a, st_b):
            assert torch.equal(x, y), (x - y).abs().max().item()


@pytest.mark.parametrize("name", ["qwen-tiny", "qwen-small", "qwen-small-c80", "qwen-tiny-g7"])
def test_shared_prefix_is_bitwise_the_unshared_path(tmp_path, name):
    rng = np.random.RandomState(3)
    paths = _media(tmp_path, rng)
    m = _model(name)
    # a window that mixes a one-sample medium (paths[0]) with a four-sample medium (paths[1]); a second video grid with two questions;
    # an image with three; a 10-frame video with three, one of them longer than a 128-row block
    images = [paths[0]] + [paths[1]] * 4 + [paths[2]] * 2 + [paths[3]] * 3 + [paths[4]] * 3
    texts = [QUESTIONS[0]] + QUESTIONS + QUESTIONS[1:3] + QUESTIONS[:3] + [LONG, QUESTIONS[2], QUESTIONS[0]]
    shared_calls = []
    real = m.engine.score_shared
    m.engine.score_shared = lambda *a, **k: shared_calls.append(real(*a, **k)) or shared_calls[-1]
    forms = [True, False] if m.engine.fp16_active else [False]
    for f16 in forms:
        m.engine.set_option("fp16", 1 if f16 else 0)
        for mnt in (1, 3):
            n0 = len(shared_calls)
            on = _run(m, images, texts, mnt, True)
            assert any(r is not None for r in shared_calls[n0:]), "the shared path did not run"
            n1 = len(shared_calls)
            off = _run(m, images, texts, mnt, False)
            assert len(shared_calls) == n1
            _assert_same(on, off)
        # generate(): the free-form path through the same front half
        gens = {}
        for share in (True, False):
            m.share_prefix = share
            gens[share] = m.generate(images, texts, max_new_tokens=3)
        assert gens[True] == gens[False]


def test_shared_prefix_engine_logits_and_decode_bitwise():
    """QwenEngine.score_shared against score_logits / prefill + decode on the same batch, in both forms."""
    from t2v_metrics_amd.qwen.layout import shared_prefix_plan
    cfg = get_qwen_config("qwen-small")
    m = _model("qwen-small", seed=9)
    rng = np.random.RandomState(4)
    frames = torch.from_numpy(rng.randint(0, 256, (4, 112, 224, 3), dtype=np.uint8))
    px, grid = m.preprocess({"type": "video", "frames": frames.numpy()})
    eng = m.engine
    forms = [True, False] if eng.fp16_active else [False]
    for f16 in forms:
        eng.set_option("fp16", 1 if f16 else 0)
        merged1 = eng.encode_vision(px, [grid])
        n_tok = merged1.shape[0]
        rows = [m.build_ids(q, "video", n_tok) for q in QUESTIONS]
        B, L = len(rows), max(len(r) for r in rows)
        ids = torch.zeros(B, L, dtype=torch.long)
        mask = torch.zeros(B, L, dtype=torch.long)
        for k, r in enumerate(rows):
            ids[k, : len(r)] = torch.tensor(r)
            mask[k, : len(r)] = 1
        merged = torch.cat([merged1] * B)
        grids = [grid] * B
        plan = shared_prefix_plan(cfg, ids, mask, grids, [0] * B)
        assert plan is not None and plan["Lp"] % 32 == 0 and plan["U"] == 1
        ref = eng.score_logits(merged, ids, mask, grids)
        got, state = eng.score_shared(merged, ids, mask, grids, [0] * B, 1)
        assert state is None and torch.equal(got, ref)
        ref_l, ref_st = eng.prefill(merged, ids, mask, grids, 3)
        got_l, got_st = eng.score_shared(merged, ids, mask, grids, [0] * B, 3)
        assert torch.equal(got_l, ref_l)
        def cache(st):      # rows [0, L) of every layer's K and V slabs (rows past L are not written by either prefill)
            return st["kv"].view(torch.bfloat16).view(2 * cfg.text.layers, B, cfg.text.kv_heads, st["Lmax"], 128)[:, :, :, :L]
        assert torch.equal(cache(got_st), cache(ref_st))
        tok = ref_l.argmax(-1)
        for _ in range(2):
            a = eng.decode(ref_st, tok)
            b = eng.decode(got_st, tok)
            assert torch.equal(a, b)
            tok = a.argmax(-1)


def test_shared_prefix_7b_two_videos_four_questions_and_the_grid_tool(tmp_path):
    """Full 7B size on seeded weights (tools/bench_qwen_grid.py's model and videos: 8 frames at 336 x 448 = 768 vision tokens, 768 shared
    rows): 2 videos x 4 questions, one of them longer than a 128-row block, bitwise equal with sharing on and off; then the tool's grid run."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_qwen_grid", os.path.join(root, "tools", "bench_qwen_grid.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    m = tool.make_model()
    paths = tool.make_videos(2, str(tmp_path))
    texts = ["a person waves at the camera", "red", LONG, "the camera pans to the right"]
    got = {}
    for share in (True, False):
        m.share_prefix = share
        got[share] = m.forward_grid(paths, texts)
    assert got[True].shape == (2, 4) and torch.isfinite(got[True]).all()
    assert torch.equal(got[True], got[False]), (got[True] - got[False]).abs().max().item()
    recs = tool.run_grid(m, paths, [1, 4], reps=1)
    assert [r["scores_bitwise_equal"] for r in recs if "scores_bitwise_equal" in r] == [True, True]
    assert all(r["ms_per_grid"] > 0 for r in recs if "ms_per_grid" in r)


def test_suffix_pass_rows_are_bitwise_the_full_pass_rows_at_every_tapped_stage():
    """The one language-model pass (text_pass) taps its intermediates in every mode: for one 4-frame video (64 vision tokens) and five
    questions, one of them longer than a 128-row attention block, every valid suffix row r - Lp of score_shared's suffix pass is bitwise row r
    of score_logits' full pass -- the stream and the FFN output at the first and the last layer, and the final stream -- in both forms."""
    from t2v_metrics_amd.qwen.layout import shared_prefix_plan
    cfg = get_qwen_config("qwen-tiny")
    m = _model("qwen-tiny", seed=9)
    rng = np.random.RandomState(4)
    px, grid = m.preprocess({"type": "video", "frames": rng.randint(0, 256, (4, 112, 224, 3), dtype=np.uint8)})
    eng = m.engine
    TH, last = cfg.text.hidden, cfg.text.layers - 1
    # in the order the pass produces them; h / h_out are the fp32 stream, d_mlp is a 16-bit tensor (bf16, or fp16 behind its scale)
    names = [("txt.0.h", 4), ("txt.0.d_mlp", 2), (f"txt.{last}.h", 4), (f"txt.{last}.d_mlp", 2), ("txt.h_out", 4)]
    try:
        for f16 in ([True, False] if eng.fp16_active else [False]):
            eng.set_option("fp16", 1 if f16 else 0)
            merged1 = eng.encode_vision(px, [grid])
            assert merged1.shape[0] == 64
            rows = [m.build_ids(q, "video", 64) for q in QUESTIONS + [LONG]]
            B, L = len(rows), max(len(r) for r in rows)
            ids = torch.zeros(B, L, dtype=torch.long)
            mask = torch.zeros(B, L, dtype=torch.long)
            for k, r in enumerate(rows):
                ids[k, : len(r)] = torch.tensor(r)
                mask[k, : len(r)] = 1
            merged, grids = torch.cat([merged1] * B), [grid] * B
            plan = shared_prefix_plan(cfg, ids, mask, grids, [0] * B)
            assert plan is not None and plan["U"] == 1
            Lp, Ls, seq_len = plan["Lp"], plan["Ls"], plan["seq_len"].tolist()
            assert max(seq_len) - Lp > 128, "one suffix must span more than one 128-row attention block"
            # B * L rows hold the full pass, the prefix pass (Lp rows) and the suffix pass (B * Ls rows)
            bufs = {n: torch.zeros(B * L * TH * size, dtype=torch.uint8, device="cuda") for n, size in names}
            for n, _ in names:
                eng.tap(n, bufs[n])
            ref = eng.score_logits(merged, ids, mask, grids)
            full = {n: bufs[n].clone().view(B, L, TH * size) for n, size in names}
            for n, _ in names:
                bufs[n].zero_()
            got, _ = eng.score_shared(merged, ids, mask, grids, [0] * B, 1)
            for n, size in names:
                sfx = bufs[n][: B * Ls * TH * size].view(B, Ls, TH * size)
                for b in range(B):
                    assert Lp < seq_len[b] <= Lp + Ls
                    same = torch.equal(sfx[b, : seq_len[b] - Lp], full[n][b, Lp : seq_len[b]])
                    assert same, f"first difference at tap {n} (fp16 forms {f16}): sample {b}'s suffix rows are not the full pass's"
            assert torch.equal(got, ref)
    finally:
        eng.tap(None)
