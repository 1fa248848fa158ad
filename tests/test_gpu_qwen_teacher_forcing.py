"""Teacher-forced scoring of multi-token answers on the MI355X: QwenEngine.score_rows / score_rows_shared (vqs_qwen_score_rows,
vqs_qwen_score_suffix_rows: the precise tail over a row list) and Qwen25VLModel.forward_with_trace_teacher_forcing on top of them.

  (1) one row per sample is score_logits bit for bit;
  (2) rows (1, 3, 5) per sample, some straddling a multiple of 32 and of 64 positions: every row against the fp32 evaluation of that row over
      the engine's own tapped K / V (tests/test_gpu_qwen.py _tail_reference, restated here for a row list) within that test's 6e-5, while the
      16-bit evaluation of the same rows is not this close;
  (3) 9 samples x 8 rows = 72 rows > the tail's 64-row chunk: every sample's rows are bitwise those of a call with that sample alone;
  (4) the shared-prefix form is bitwise the unshared one (two media x three questions, answers of different lengths);
  (5) end to end through Qwen25VLModel: every answer token's log-probability against the fp32 oracle within the calibrated bound of the
      fixture's last row (tests/test_gpu_qwen.py _calibrated_bound);
  (6) the rollout method on the same samples with the answer set to its own greedy rollout agrees per token within DECODE_CEILING;
  (7) two identical calls give identical scores.
Configurations: qwen-tiny (4/2 heads of 32 lanes), qwen-tiny-g7 (7 query heads per key/value head), qwen-small (128-lane heads, fp16 forms)."""
import functools

import numpy as np
import pytest
import torch

from t2v_metrics_amd.models.vqascore_models.qwen25vl_model import Qwen25VLModel, default_question_template
from t2v_metrics_amd.qwen import get_qwen_config
from t2v_metrics_amd.qwen.layout import answer_rows, shared_prefix_plan, text_layout
from t2v_metrics_amd.qwen.weights import make_seeded_qwen_weights
from tests.test_gpu_qwen import DECODE_CEILING, _calibrated_bound, _record
from tests.test_qwen_teacher_forcing_host import IdTokenizer

pytestmark = pytest.mark.gpu

NAMES = ["qwen-tiny", "qwen-tiny-g7", "qwen-small"]
TAIL_REL = 6e-5          # tests/test_gpu_qwen.py: split-bf16 operands, 2^-16 relative per rounding, a few dozen roundings deep


@functools.lru_cache(maxsize=None)
def _model(name):
    """One scorer (and engine) per configuration for the whole module; tests restore every option they change."""
    cfg = get_qwen_config(name)
    w = make_seeded_qwen_weights(cfg, seed=9, dtype=torch.bfloat16, lm_head_gain=4.0)
    m = Qwen25VLModel(model_name="qwen2.5-vl-7b", device="cuda", config=cfg, weights=w, tokenizer=IdTokenizer(cfg.text.vocab))
    m._gen_eos_ids = []
    return m, cfg, w


def _batch(cfg, grids, lens, seed):
    """A seeded ragged right-padded batch: sample b = text, one video run of grid b, text, lens[b] tokens in all.  -> ids, mask, px (bf16 values)."""
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(sum(a * b * c for a, b, c in grids), cfg.vision.patch_dim, generator=g).to(torch.bfloat16)
    rows = []
    for i, (gr, n) in enumerate(zip(grids, lens)):
        n_merged = gr[0] * gr[1] * gr[2] // cfg.vision.merge_unit
        pre = torch.randint(10, cfg.text.vocab, (4 + i % 3,), generator=g)
        post = torch.randint(10, cfg.text.vocab, (n - len(pre) - n_merged - 2,), generator=g)
        rows.append(torch.cat([pre, torch.tensor([cfg.vision_start_token_id]), torch.full((n_merged,), cfg.video_token_id),
                               torch.tensor([cfg.vision_end_token_id]), post]))
        assert len(rows[-1]) == n
    L = max(lens)
    ids = torch.stack([torch.nn.functional.pad(r, (0, L - len(r))) for r in rows])
    mask = torch.stack([torch.nn.functional.pad(torch.ones(len(r), dtype=torch.long), (0, L - len(r))) for r in rows])
    return ids, mask, px


def _encode(eng, px, grids):
    merged, off = [], 0
    for g in grids:
        n = g[0] * g[1] * g[2]
        merged.append(eng.encode_vision(px[off: off + n].cuda(), [g]))
        off += n
    return torch.cat(merged)


# rows (1, 3, 5): sample 1's rows are positions 94, 95, 96 (across 3 x 32), sample 2's 61 .. 65 (across 64, and 65 keys)
GRIDS3, LENS3, ROWS3 = [(2, 8, 8), (2, 8, 12), (2, 8, 8)], [50, 97, 66], [1, 3, 5]


@pytest.mark.parametrize("name", NAMES)
def test_one_row_per_sample_is_score_logits_bit_for_bit(name):
    m, cfg, _ = _model(name)
    eng = m.engine
    ids, mask, px = _batch(cfg, GRIDS3, LENS3, seed=21)
    merged = _encode(eng, px, GRIDS3)
    ref = eng.score_logits(merged, ids, mask, GRIDS3)
    for n_rows in (1, [1, 1, 1]):
        got = eng.score_rows(merged, ids, mask, GRIDS3, n_rows)
        assert got.shape == ref.shape and torch.equal(got, ref)


def _rows_reference(cfg, w, lay, rows, emb, k_taps, v_taps):
    """tests/test_gpu_qwen.py _tail_reference for a row list: row r = row index[r] of the pass through all layers in plain fp32 torch on
    the device -- its own q, softmax and sub-layer outputs in fp32, attending over the first keys[r] positions of the ENGINE's K / V of
    sample sample[r] (true units) -- then the final norm and lm_head.  Formulas: oracle/qwen25vl_oracle.py."""
    import torch.nn.functional as F
    from oracle.qwen25vl_oracle import rms_norm
    t = cfg.text
    index, sample, keys = (x.long().cuda() for x in rows)
    Q, L = index.numel(), k_taps[0].shape[2]
    hd, half = t.head_dim, t.head_dim // 2
    cos, sin = lay["cos"].cuda()[index], lay["sin"].cuda()[index]
    W = lambda name: w[name].float().cuda()      # noqa: E731
    h = emb.float()[index]
    rep = t.heads // t.kv_heads
    for i in range(t.layers):
        p = f"model.language_model.layers.{i}."
        x = rms_norm(h, W(p + "input_layernorm.weight"), t.rms_eps)
        q = (x @ W(p + "self_attn.q_proj.weight").t() + W(p + "self_attn.q_proj.bias")).view(Q, t.heads, hd)
        a, b2 = q[..., :half], q[..., half:]
        q = torch.cat([a * cos[:, None] - b2 * sin[:, None], b2 * cos[:, None] + a * sin[:, None]], -1)
        K = k_taps[i][sample][..., :hd].repeat_interleave(rep, 1)                          # [Q, H, L, hd]
        V = v_taps[i][sample][..., :hd].repeat_interleave(rep, 1)
        sc = torch.einsum("qhd,qhld->qhl", q, K) * hd ** -0.5
        sc = sc.masked_fill(torch.arange(L, device="cuda")[None, None, :] >= keys[:, None, None], float("-inf"))
        o = torch.einsum("qhl,qhld->qhd", torch.softmax(sc, -1), V).reshape(Q, -1)
        h = h + o @ W(p + "self_attn.o_proj.weight").t()
        x = rms_norm(h, W(p + "post_attention_layernorm.weight"), t.rms_eps)
        h = h + (F.silu(x @ W(p + "mlp.gate_proj.weight").t()) * (x @ W(p + "mlp.up_proj.weight").t())) @ W(p + "mlp.down_proj.weight").t()
    return rms_norm(h, W("model.language_model.norm.weight"), t.rms_eps) @ W("lm_head.weight").t()


@pytest.mark.parametrize("name", NAMES)
def test_every_listed_row_is_its_fp32_evaluation_over_the_engines_kv(name):
    from oracle.qwen25vl_engine_rounding import sites_from_report
    m, cfg, w = _model(name)
    eng, t = m.engine, cfg.text
    ids, mask, px = _batch(cfg, GRIDS3, LENS3, seed=22)
    merged = _encode(eng, px, GRIDS3)
    B, L = ids.shape
    F16 = eng.fp16_active
    assert F16 == (name == "qwen-small")
    sig = sites_from_report(cfg, eng.range_report()[1]) if F16 else None
    bufs = {f"txt.{i}.{nm}": torch.zeros(B, t.kv_heads, L, 128, dtype=torch.float16 if F16 else torch.bfloat16, device="cuda")
            for i in range(t.layers) for nm in "kv"}
    bufs["txt.emb"] = torch.zeros(B * L, t.hidden, dtype=torch.float32, device="cuda")
    try:
        for nme, b in bufs.items():
            eng.tap(nme, b)
        logits = eng.score_rows(merged, ids, mask, GRIDS3, ROWS3).float()
        torch.cuda.synchronize()
    finally:
        eng.tap(None)
    lay = text_layout(cfg, ids, mask, GRIDS3)
    rows = answer_rows(lay["seq_len"], ROWS3, L)
    assert rows[2].tolist() == [50, 95, 96, 97, 62, 63, 64, 65, 66] and logits.shape == (9, t.vocab)
    kv_true = lambda nm, i: bufs[f"txt.{i}.{nm}"].float() / (sig[("txt", i, "qkv")] if F16 else 1.0)      # noqa: E731
    ref = _rows_reference(cfg, w, lay, rows, bufs["txt.emb"], [kv_true("k", i) for i in range(t.layers)], [kv_true("v", i) for i in range(t.layers)])
    top = float(ref.abs().max())
    err_rows = ((logits - ref).abs().amax(-1) / top).cpu()
    # the 16-bit evaluation of the same rows: row p of a sample is the last row of the pass over its first p + 1 positions, tail off
    low = torch.empty_like(logits)
    eng.set_option("tail_precise", 0)
    try:
        r0 = 0
        for b, n in enumerate(ROWS3):
            for j in range(n):
                mk = mask.clone()
                mk[b, LENS3[b] - (n - 1 - j):] = 0
                low[r0 + j] = eng.score_logits(merged, ids, mk, GRIDS3).float()[b]
            r0 += n
        torch.cuda.synchronize()
    finally:
        eng.set_option("tail_precise", 1)
    err_low = float((low - ref).abs().max()) / top
    err_tail = float(err_rows.max())
    _record({"case": f"qwen-rows-tail/{name}", "rows_vs_fp32_rows_over_engine_kv_rel": err_tail, "per_row": [float(x) for x in err_rows],
             "16bit_rows_vs_same_rel": err_low})
    print(name, "rows vs fp32 rows over the engine's K/V:", err_rows.tolist(), "16-bit rows:", err_low)
    assert err_tail <= TAIL_REL, (err_rows.tolist(), err_low)
    assert err_low > (2 if F16 else 5) * err_tail, (err_tail, err_low)      # a tail that silently ran in 16 bits would be noticed


@pytest.mark.parametrize("name", NAMES)
def test_a_chunk_boundary_inside_a_sample_changes_nothing(name):
    m, cfg, _ = _model(name)
    eng = m.engine
    grids = [(2, 8, 8)] * 9
    lens = [48 + 3 * b for b in range(9)]
    ids, mask, px = _batch(cfg, grids, lens, seed=23)
    merged = _encode(eng, px, grids)
    got = eng.score_rows(merged, ids, mask, grids, 8)                  # 72 rows: the second chunk starts at sample 8's first row
    assert got.shape[0] == 72 and bool(torch.isfinite(got).all())
    n_tok = merged.shape[0] // 9
    for b in range(9):
        alone = eng.score_rows(merged[b * n_tok: (b + 1) * n_tok], ids[b: b + 1], mask[b: b + 1], grids[b: b + 1], 8)
        assert torch.equal(alone, got[8 * b: 8 * b + 8]), b


@pytest.mark.parametrize("name", NAMES)
def test_shared_prefix_rows_are_bitwise_the_unshared_rows(name):
    m, cfg, _ = _model(name)
    eng = m.engine
    rng = np.random.RandomState(4)
    questions = ["a person waves", "a car turns left at the corner of a busy street", "red"]
    n_rows = [1, 4, 2, 3, 1, 5]
    g = torch.Generator().manual_seed(24)
    seqs, merged, grids = [], [], []
    for u in range(2):
        px, grid = m.preprocess({"type": "video", "frames": rng.randint(0, 256, (4, 112, 224, 3), dtype=np.uint8)})
        mu = eng.encode_vision(px, [grid])
        for k, q in enumerate(questions):
            forced = torch.randint(10, cfg.text.vocab, (n_rows[3 * u + k] - 1,), generator=g).tolist()
            seqs.append(m.build_ids(default_question_template.format(q), "video", mu.shape[0]) + forced)
            merged.append(mu)
            grids.append(grid)
    B, L = len(seqs), max(len(s) for s in seqs)
    ids, mask = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
    for k, s in enumerate(seqs):
        ids[k, : len(s)] = torch.tensor(s)
        mask[k, : len(s)] = 1
    merged, media = torch.cat(merged), [0, 0, 0, 1, 1, 1]
    plan = shared_prefix_plan(cfg, ids, mask, grids, media)
    assert plan is not None and plan["U"] == 2 and plan["Lp"] % 32 == 0
    ref = eng.score_rows(merged, ids, mask, grids, n_rows)
    got = eng.score_rows_shared(merged, ids, mask, grids, media, n_rows)
    assert got is not None and got.shape == (sum(n_rows), cfg.text.vocab) and torch.equal(got, ref)
    assert eng.score_rows_shared(merged, ids, mask, grids, list(range(B)), n_rows) is None      # nothing to share


# ---- through the public interface
TEXTS = ["a person waves", "a car turns left", "a red square"]
ANSWERS = [4, 3, 2]          # answer tokens per sample


def _paths(tmp_path):
    rng = np.random.RandomState(2)
    paths = []
    for i, shape in enumerate([(2, 112, 224, 3), (2, 112, 224, 3), (224, 112, 3)]):
        p = tmp_path / f"v{i}.npy"
        np.save(p, rng.randint(0, 256, shape, dtype=np.uint8))
        paths.append(str(p))
    return paths


def _oracle_rows(m, cfg, w, paths, answers):
    """fp32 truth of every answer token: sample i's sequence = prompt + a[:n-1]; QwenOracle hidden state at its last n rows times lm_head
    -> (per sample log-softmax rows [n, vocab], ids, mask, px, grids of the batch)."""
    from oracle.qwen25vl_oracle import QwenOracle
    seqs, px, grids = [], [], []
    for path, text, a in zip(paths, TEXTS, answers):
        item = m.load_images([path])[0]
        p, grid = m.preprocess(item)
        px.append(p.to(torch.bfloat16).float())              # the values the engine's tower reads
        grids.append(grid)
        n_tok = grid[0] * grid[1] * grid[2] // cfg.vision.merge_unit
        seqs.append(m.build_ids(default_question_template.format(text), item["type"], n_tok) + a[:-1])
    B, L = len(seqs), max(len(s) for s in seqs)
    ids, mask = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
    for k, s in enumerate(seqs):
        ids[k, : len(s)] = torch.tensor(s)
        mask[k, : len(s)] = 1
    px = torch.cat(px)
    o = QwenOracle(cfg, w)
    hid = o.forward(ids, mask, px, grids, return_stages=True)["hidden"]
    head = o._w("lm_head.weight")
    out = []
    for b, a in enumerate(answers):
        n = len(seqs[b])
        out.append(torch.log_softmax(hid[b, n - len(a): n].float() @ head.t(), -1))
    return out, ids, mask, px, grids


@pytest.mark.parametrize("name", NAMES)
def test_answer_tokens_against_the_fp32_oracle_and_the_rollout_method(tmp_path, name):
    m, cfg, w = _model(name)
    paths = _paths(tmp_path)
    spell = lambda a: " ".join(f"#{i}" for i in a)      # noqa: E731
    # the answers: every sample's own greedy rollout, so that the rollout method reads the same distributions
    answers = []
    for p, text, n in zip(paths, TEXTS, ANSWERS):
        gen = m._generate_scores([p], [text], None, default_question_template, "Yes", n)[0][1]
        assert len(gen) == n
        answers.append([int(x) for x in gen])
    ref_rows, ids, mask, px, grids = _oracle_rows(m, cfg, w, paths, answers)
    # the calibrated bound of this fixture's last row, over its five most likely tokens and the answer's last token
    last = torch.stack([r[-1] for r in ref_rows])
    toks = torch.cat([last.topk(5).indices, torch.tensor([[a[-1]] for a in answers])], dim=1)
    bound, floor = _calibrated_bound(cfg, w, grids, ids, mask, px, last, toks)
    worst_tf, worst_roll, worst_between = 0.0, 0.0, 0.0
    s_tf, s_again = [], []
    for i, (p, text, a) in enumerate(zip(paths, TEXTS, answers)):
        s, tr = m.forward_with_trace_teacher_forcing([p], [text], answer_template=spell(a), max_new_tokens=len(a))
        s2 = m.forward([p], [text], answer_template=spell(a), max_new_tokens=len(a), teacher_forcing=True)
        s_tf.append(float(s[0]))
        s_again.append(float(s2[0]))
        sr, trr = m.forward_with_trace([p], [text], answer_template=spell(a), max_new_tokens=len(a))
        assert trr[0]["scored_indices"] == list(range(len(a))), "the rollout did not reproduce its own answer"
        for t, (d, dr) in enumerate(zip(tr[0]["token_details"], trr[0]["token_details"])):
            truth = float(ref_rows[i][t, a[t]])
            e_tf, e_roll = abs(np.log(d["probability"]) - truth), abs(np.log(dr["probability"]) - truth)
            between = abs(np.log(d["probability"]) - np.log(dr["probability"]))
            print(name, "sample", i, "token", t, "|dlogp| teacher forcing", e_tf, "rollout", e_roll, "between the methods", between, "bound", bound)
            worst_tf, worst_roll, worst_between = max(worst_tf, e_tf), max(worst_roll, e_roll), max(worst_between, between)
    _record({"case": f"qwen-teacher-forcing/{name}", "max_abs_dlogp_answer_tokens_teacher_forcing_vs_fp32_oracle": worst_tf,
             "max_abs_dlogp_answer_tokens_rollout_vs_fp32_oracle": worst_roll, "max_abs_dlogp_between_the_methods": worst_between,
             "bf16_floor_rounding_matched_vs_fp32": floor, "bound": bound})
    assert worst_tf <= bound, (worst_tf, bound, floor)                          # (5)
    assert worst_between <= DECODE_CEILING, (worst_between, worst_roll)         # (6) the two methods compute the same quantity
    assert s_tf == s_again                                                      # (7) and through forward(teacher_forcing=True)
    # a batch of all three with answers of different lengths, twice: bitwise repeatable
    batch = [m.forward_teacher_forcing(paths, TEXTS, answer_template="Yes it really does", max_new_tokens=4) for _ in range(2)]
    assert torch.equal(batch[0], batch[1]) and bool(((batch[0] > 0) & (batch[0] < 1)).all())
