"""Teacher-forced answer scoring of the Qwen2.5-VL row (Qwen25VLModel.forward_with_trace_teacher_forcing / forward_teacher_forcing /
forward(teacher_forcing=True)) on the CPU, with the fp32 oracle behind the engine interface: the double below implements score_rows from
QwenOracle hidden states.  What is checked is the host's semantics -- which sequence is built, which rows are read, how each row is
processed -- against the rollout method on the same double and against a literal restatement over the oracle's logits."""
import re

import numpy as np
import pytest
import torch

import t2v_metrics_amd as t2v
from t2v_metrics_amd.models.vqascore_models.qwen25vl_model import default_question_template
from t2v_metrics_amd.qwen import get_qwen_config
from t2v_metrics_amd.qwen.layout import answer_rows, shared_prefix_plan
from t2v_metrics_amd.qwen.weights import make_seeded_qwen_weights
from tests.test_qwen_host import FakeQwenTokenizer, OracleQwenEngine


class IdTokenizer(FakeQwenTokenizer):
    """FakeQwenTokenizer whose words "#<id>" encode to that id: an answer can be spelled token by token (the decoded rollout)."""

    def encode(self, text, add_special_tokens=False):
        out = []
        for w in text.split():
            out += [int(w[1:])] if re.fullmatch(r"#\d+", w) else super().encode(w)
        return out


class RowsOracleEngine(OracleQwenEngine):
    """OracleQwenEngine + score_rows / score_rows_shared: fp32 logits of the last n_b valid positions of every sample."""

    def __init__(self, cfg, weights):
        super().__init__(cfg, weights)
        self.rows_calls, self.shared_calls = [], []

    def _hidden(self, merged, input_ids, attention_mask, grids):
        from oracle.qwen25vl_oracle import mrope_position_ids
        o, c = self.o, self.cfg
        with torch.no_grad():
            emb = o._w("model.language_model.embed_tokens.weight")[input_ids]
            m = (input_ids == c.video_token_id) & attention_mask.bool()
            emb = emb.masked_scatter(m[..., None].expand_as(emb), merged.float())
            pos = mrope_position_ids(input_ids, attention_mask, c.image_token_id, c.video_token_id, [], grids, c.vision.spatial_merge,
                                     c.vision.tokens_per_second)
            return o.text_model(emb, pos, attention_mask)

    def score_rows(self, merged, input_ids, attention_mask, grids, n_rows):
        B, L = input_ids.shape
        idx, _, _ = answer_rows(attention_mask.long().sum(-1), n_rows, L)
        self.rows_calls.append(list(n_rows) if not isinstance(n_rows, int) else n_rows)
        hid = self._hidden(merged, input_ids, attention_mask, grids).reshape(B * L, -1)
        return hid[idx.long()] @ self.o._w("lm_head.weight").t()

    def score_rows_shared(self, merged, input_ids, attention_mask, grids, media, n_rows):
        plan = shared_prefix_plan(self.cfg, input_ids, attention_mask, grids, media)
        if plan is None:
            return None
        idx, smp, keys = answer_rows(plan["seq_len"], n_rows, plan["Ls"], offset=plan["Lp"])       # the suffix pass's list: must lie in the suffix
        full = answer_rows(plan["seq_len"], n_rows, input_ids.shape[1])
        assert torch.equal(keys, full[2]) and torch.equal(smp, full[1]) and torch.equal(idx + smp * plan["Lp"] + plan["Lp"], full[0])
        self.shared_calls.append(len(idx))
        calls = len(self.rows_calls)
        out = self.score_rows(merged, input_ids, attention_mask, grids, n_rows)
        del self.rows_calls[calls:]
        return out


Q_T = default_question_template


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    cfg = get_qwen_config("qwen-tiny")
    w = make_seeded_qwen_weights(cfg, seed=3, dtype=torch.bfloat16, lm_head_gain=4.0)
    d = tmp_path_factory.mktemp("tf")
    rng = np.random.RandomState(2)
    paths = []
    for i, shape in enumerate([(112, 112, 3), (4, 112, 112, 3)]):
        p = d / f"m{i}.npy"
        np.save(p, rng.randint(0, 256, shape, dtype=np.uint8))
        paths.append(str(p))
    return cfg, w, paths


def _model(setup, **kw):
    cfg, w, _ = setup
    eng = RowsOracleEngine(cfg, w)
    scorer = t2v.VQAScore(model="qwen2.5-vl-7b", device="cpu", config=cfg, engine=eng, tokenizer=IdTokenizer(cfg.text.vocab), **kw)
    scorer.model._gen_eos_ids = []
    return scorer, scorer.model, eng


def _spell(ids):
    return " ".join(f"#{i}" for i in ids)


def _rollout(m, path, text, n):
    return m._generate_scores([path], [text], None, Q_T, "Yes", n)[0][1]


def _literal(m, eng, path, text, a, temperature=1.0):
    """P(answer) restated: for every t one oracle pass over prompt + a[:t], its last row processed over prompt + a[:t], softmax."""
    item = m.load_images([path])[0]
    patches, grid = m.preprocess(item)
    merged = eng.encode_vision(patches, [grid])
    prompt = m.build_ids(Q_T.format(text), item["type"], merged.shape[0])
    ps = []
    for t in range(len(a)):
        ids = torch.tensor([prompt + a[:t]])
        row = eng.score_logits(merged, ids, torch.ones_like(ids), [grid])
        row = m._processed_scores(row, [prompt + a[:t]])
        ps.append(torch.softmax(row[0].double() / temperature, -1)[a[t]].item())
    return float(np.prod(ps) ** (1.0 / len(a))), ps


def test_one_token_answer_equals_forward_exactly(setup):
    _, m, eng = _model(setup)
    paths, texts = setup[2], ["a red cube", "a dog runs fast"]
    ref = m.forward(paths, texts)
    assert torch.equal(m.forward_teacher_forcing(paths, texts), ref)
    assert torch.equal(m.forward(paths, texts, teacher_forcing=True), ref)
    assert torch.equal(m.forward_with_trace_teacher_forcing(paths, texts)[0], ref)
    assert torch.equal(m.forward(paths, texts, answer_template="No", temperature=1.7, teacher_forcing=True), m.forward(paths, texts, answer_template="No", temperature=1.7))
    assert eng.rows_calls and all(n == [1] for n in eng.rows_calls)


def test_answer_equal_to_the_greedy_rollout_agrees_with_forward_with_trace(setup):
    """The reference's own criterion (test_teacher_vs_rollout.py): where the rollout produces the answer, the two methods agree to 1e-6."""
    _, m, eng = _model(setup)
    path, text, n = setup[2][1], "a red cube", 4
    gen = _rollout(m, path, text, n)
    assert len(gen) == n
    s_roll, tr_roll = m.forward_with_trace([path], [text], answer_template=_spell(gen), max_new_tokens=n)
    s_tf, tr_tf = m.forward_with_trace_teacher_forcing([path], [text], answer_template=_spell(gen), max_new_tokens=n)
    assert abs(float(s_roll[0]) - float(s_tf[0])) <= 1e-6
    for a, b in zip(tr_roll[0]["token_details"], tr_tf[0]["token_details"]):
        assert a["expected_token_id"] == b["expected_token_id"] and abs(a["probability"] - b["probability"]) <= 1e-6
        assert [x["token_id"] for x in a["top_alternatives"]] == [x["token_id"] for x in b["top_alternatives"]]
    assert all(d["is_greedy"] and d["greedy_token_id"] == g for d, g in zip(tr_tf[0]["token_details"], gen))
    assert eng.rows_calls == [[n]]
    want, _ = _literal(m, eng, path, text, gen)
    assert abs(float(s_tf[0]) - want) <= 1e-6


def test_a_diverging_rollout_is_marked_and_only_teacher_forcing_is_the_answers_probability(setup):
    _, m, eng = _model(setup)
    path, text, n = setup[2][1], "a red cube", 4
    gen = _rollout(m, path, text, n)
    other = next(i for i in range(10, 400) if i not in gen)
    a = [gen[0], other] + gen[2:]                                   # the rollout leaves the answer at its second token
    s_tf, tr = m.forward_with_trace_teacher_forcing([path], [text], answer_template=_spell(a), max_new_tokens=n)
    det = tr[0]["token_details"]
    assert det[0]["is_greedy"] and not det[1]["is_greedy"] and det[1]["greedy_token_id"] == gen[1] and det[1]["expected_token_id"] == other
    want, ps = _literal(m, eng, path, text, a)
    assert abs(float(s_tf[0]) - want) <= 1e-6
    assert all(abs(d["probability"] - p) <= 1e-6 * max(1.0, p) + 1e-9 for d, p in zip(det, ps))
    # the rollout reads tokens 3 and 4 from distributions conditioned on ITS second token, not the answer's
    s_roll = m.forward([path], [text], answer_template=_spell(a), max_new_tokens=n)
    assert abs(float(s_roll[0]) - float(s_tf[0])) > 1e-6


def test_truncation_temperature_and_repetition_penalty(setup):
    _, m, eng = _model(setup)
    path, text = setup[2][0], "two birds"
    a = [41, 97, 41, 203]
    full = m.forward_teacher_forcing([path], [text], answer_template=_spell(a), max_new_tokens=4)
    cut = m.forward_teacher_forcing([path], [text], answer_template=_spell(a), max_new_tokens=2)
    assert torch.equal(cut, m.forward_teacher_forcing([path], [text], answer_template=_spell(a[:2]), max_new_tokens=9)) and not torch.equal(cut, full)
    assert eng.rows_calls == [[4], [2], [2]]
    _, tr = m.forward_with_trace_teacher_forcing([path], [text], answer_template=_spell(a), max_new_tokens=3)
    assert tr[0]["generated_length"] == 3 and tr[0]["scored_indices"] == [0, 1, 2] and [d["expected_token_id"] for d in tr[0]["token_details"]] == a[:3]
    with pytest.raises(ValueError):
        m.forward_teacher_forcing([path], [text], max_new_tokens=0)
    hot = m.forward_teacher_forcing([path], [text], answer_template=_spell(a), max_new_tokens=4, temperature=2.5)
    assert abs(float(hot[0]) - _literal(m, eng, path, text, a, temperature=2.5)[0]) <= 1e-6 and abs(float(hot[0]) - float(full[0])) > 1e-6
    # the penalty of row t covers the prompt and the t forced tokens before it: a[2] repeats a[0], so its row is penalised where row 0's is not
    m.repetition_penalty = 1.3
    try:
        pen = m.forward_with_trace_teacher_forcing([path], [text], answer_template=_spell(a), max_new_tokens=4)
        want, ps = _literal(m, eng, path, text, a)
        assert abs(float(pen[0][0]) - want) <= 1e-6 and abs(want - float(full[0])) > 1e-6
        assert all(abs(d["probability"] - p) <= 1e-6 for d, p in zip(pen[1][0]["token_details"], ps))
    finally:
        m.repetition_penalty = 1.0


def test_trace_has_the_keys_of_forward_with_trace(setup):
    _, m, _ = _model(setup)
    path, text, ans = setup[2][0], "two birds", "Yes it does"
    _, roll = m.forward_with_trace([path], [text], answer_template=ans, max_new_tokens=3)
    s, tf = m.forward_with_trace_teacher_forcing([path], [text], answer_template=ans, max_new_tokens=3, debug=True)
    t = tf[0]
    assert set(t) == set(roll[0])
    assert set(t["token_details"][0]) == set(roll[0]["token_details"][0]) | {"greedy_token_id", "is_greedy"}
    ids = m.tokenizer.encode(ans)
    assert t["score_position"] == "teacher_forcing" and t["scored_indices"] == [0, 1, 2] and t["score_start_idx"] == 0 and t["generated_length"] == 3
    assert t["generated_text"] == t["scored_tokens_text"] == m.tokenizer.decode(ids, skip_special_tokens=True)
    assert abs(t["probability"] - float(s[0])) <= 1e-7
    for d in t["token_details"]:
        alts = d["top_alternatives"]
        assert len(alts) == 5 and all(alts[i]["probability"] >= alts[i + 1]["probability"] for i in range(4))
        assert d["is_greedy"] == (d["greedy_token_id"] == d["expected_token_id"]) and alts[0]["token_id"] == d["greedy_token_id"]


def test_the_keyword_reaches_the_model_through_the_scorer_and_sharing_changes_nothing(setup):
    scorer, m, eng = _model(setup, max_batch=4)
    paths, texts, ans = setup[2], ["a cat jumps", "a dog runs fast in the park", "rain"], "Yes it really does"
    m.share_prefix = False
    grid = scorer(images=paths, texts=texts, answer_template=ans, max_new_tokens=4, teacher_forcing=True)
    assert grid.shape == (2, 3) and eng.rows_calls and not eng.shared_calls
    assert sum(len(c) for c in eng.vision_calls) == 2                                    # one tower pass per medium
    flat = m.forward_teacher_forcing([p for p in paths for _ in texts], [t for _ in paths for t in texts], answer_template=ans, max_new_tokens=4)
    assert torch.equal(grid.cpu().reshape(-1), flat)
    rollout = scorer(images=paths, texts=texts, answer_template=ans, max_new_tokens=4)
    assert not torch.equal(rollout, grid)                                                # default False: the rollout path, another number
    ds = [{"images": [p], "texts": texts} for p in paths]
    assert torch.equal(scorer.batch_forward(ds, batch_size=2, answer_template=ans, max_new_tokens=4, teacher_forcing=True).reshape(2, 3).cpu(), grid.cpu())
    # several texts per medium with share_prefix: the shared path, the same scores
    m.share_prefix = True
    n_rows = len(eng.rows_calls)
    shared = scorer(images=paths, texts=texts, answer_template=ans, max_new_tokens=4, teacher_forcing=True)
    # the video's three prompts share their prefix (12 rows from one suffix pass); the image's prefix is shorter than 32 rows and is not shared
    assert eng.shared_calls == [12] and len(eng.rows_calls) == n_rows + 1 and torch.equal(shared, grid)


def test_an_engine_without_score_rows_is_refused(setup):
    cfg, w, paths = setup
    m = t2v.VQAScore(model="qwen2.5-vl-7b", device="cpu", config=cfg, engine=OracleQwenEngine(cfg, w), tokenizer=IdTokenizer(cfg.text.vocab)).model
    assert m.forward(paths[:1], ["x"]).shape == (1,)
    with pytest.raises(NotImplementedError, match="score_rows"):
        m.forward(paths[:1], ["x"], teacher_forcing=True)
    with pytest.raises(NotImplementedError, match="score_rows"):
        m.forward_with_trace_teacher_forcing(paths[:1], ["x"])


def test_non_finite_rows_under_the_fp16_forms_fall_back_to_bf16_once(setup):
    """The backstop of forward (tests/test_qwen_host.py) holds for the teacher-forced calls: one warning, option fp16 off, the call run again."""
    import warnings
    cfg, w, paths = setup

    class Overflowing(RowsOracleEngine):
        fp16_active = True

        def set_option(self, name, value):
            self.switched = getattr(self, "switched", []) + [(name, value)]
            if name == "fp16":
                self.fp16_active = bool(value)

        def score_rows(self, *a):
            lg = super().score_rows(*a)
            return lg * float("nan") if self.fp16_active else lg

    eng = Overflowing(cfg, w)
    m = t2v.VQAScore(model="qwen2.5-vl-7b", device="cpu", config=cfg, engine=eng, tokenizer=IdTokenizer(cfg.text.vocab)).model
    _, ref, _ = _model(setup)
    kw = dict(answer_template="Yes it does", max_new_tokens=3)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        s = m.forward_teacher_forcing(paths, ["a thing happens", "rain"], **kw)
    assert torch.isfinite(s).all() and torch.equal(s, ref.forward_teacher_forcing(paths, ["a thing happens", "rain"], **kw))
    assert eng.switched == [("fp16", 0)] and sum("fp16" in str(r.message) for r in rec) == 1
