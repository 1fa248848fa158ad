#!/usr/bin/env python3
"""What teacher-forced answer scoring of the Qwen2.5-VL row costs and how exact it is, at full size: seeded 7B weights, --clips distinct
in-memory 8-frame 336 x 448 clips (768 vision tokens) with one question each per call, answers of --answers tokens.

Timing (through the drop-in API, ONE scorer, media front end on the device): for every answer length A the two methods alternate --
forward(answer, max_new_tokens=A, teacher_forcing=True) and the rollout forward(answer, max_new_tokens=A) -- one warm-up call each, then
--reps timed calls each; host clock around a call that ends with the scores on the host (a device synchronise).  Per A: median, min and max
ms per call of both methods, and the extra cost of teacher forcing over its own A = 1 call (the Q = clips x A rows of the precise tail
instead of clips rows, plus A - 1 more positions per prompt).  No speed-up is claimed: these are the first measurements of the tail at
Q > B.

Exactness (a record, not a test): one sample, a 4-token answer.  Per token |delta log P| against the fp32 oracle's code
(oracle/qwen25vl_oracle.py) evaluated in fp32 by torch on the device over the same sequence, for the teacher-forced rows (precise tail)
and for the rollout's rows (token 1 from the prefill's precise tail, tokens 2 .. 4 from the cached decode step).

One JSON line per record on stdout, appended to --out.
  python tools/bench_qwen_teacher.py [--clips 64] [--answers 1 4 8] [--reps 3] [--out profiles/qwen_teacher_forcing.jsonl] [--no-parity]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_qwen_grid import QUESTIONS, make_model  # noqa: E402

WORDS = ["yes", "it", "does", "show", "that", "quite", "clearly", "indeed"]          # one token each under the test tokenizer


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 2), "min_ms": round(min(xs), 2), "max_ms": round(max(xs), 2), "calls": len(xs)}


def run_timing(m, clips, answers, reps):
    texts = [QUESTIONS[i % len(QUESTIONS)] for i in range(len(clips))]
    out, tf1 = [], None
    for A in answers:
        ans = " ".join(WORDS[:A])
        assert len(m.tokenizer.encode(ans)) == A
        calls = {True: lambda: m.forward(clips, texts, answer_template=ans, max_new_tokens=A, teacher_forcing=True),
                 False: lambda: m.forward(clips, texts, answer_template=ans, max_new_tokens=A)}
        times, scores = {True: [], False: []}, {}
        for tf in (True, False):
            calls[tf]()                                      # warm-up: every shape of the timed calls
        for _ in range(reps):
            for tf in (True, False):                         # alternate the two methods
                ms, scores[tf] = timed(calls[tf])
                times[tf].append(ms)
        rec = {"record": "timing", "clips": len(clips), "answer_tokens": A, "tail_rows": len(clips) * A,
               "teacher_forcing": stats(times[True]), "rollout": stats(times[False]),
               "scores_finite": bool(torch.isfinite(scores[True]).all() and torch.isfinite(scores[False]).all()),
               "max_abs_dlog_score_between_methods": float((scores[True].log() - scores[False].log()).abs().max())}
        if A == 1:
            tf1 = rec["teacher_forcing"]["median_ms"]
            rec["scores_bitwise_equal"] = bool(torch.equal(scores[True], scores[False]))
        if tf1 is not None:
            rec["teacher_forcing_extra_ms_over_one_token"] = round(rec["teacher_forcing"]["median_ms"] - tf1, 2)
            rec["teacher_forcing_extra_share_of_one_token_call"] = round(rec["teacher_forcing"]["median_ms"] / tf1 - 1.0, 4)
        out.append(rec)
    return out


def run_parity(m, n_answer=4, seed=77):
    from oracle.qwen25vl_oracle import QwenOracle
    cfg, eng = m.cfg, m.engine
    w = eng._weights
    grid = (4, 24, 32)
    n_patches = grid[0] * grid[1] * grid[2]
    g = torch.Generator().manual_seed(seed)
    px = torch.randn(n_patches, cfg.vision.patch_dim, generator=g).to(torch.bfloat16)
    n_merged = n_patches // cfg.vision.merge_unit
    pre = torch.randint(10, 150000, (14,), generator=g)
    post = torch.randint(10, 150000, (24,), generator=g)
    prompt = torch.cat([pre, torch.tensor([cfg.vision_start_token_id]), torch.full((n_merged,), cfg.video_token_id),
                        torch.tensor([cfg.vision_end_token_id]), post])
    merged = eng.encode_vision(px.cuda(), [grid])
    # the answer: the engine's own greedy rollout, so that both methods score the same tokens
    ids_p = prompt[None]
    logits, state = eng.prefill(merged, ids_p, torch.ones_like(ids_p), [grid], n_answer)
    roll, a = [logits.float().cpu()[0]], []
    for t in range(n_answer):
        a.append(int(roll[-1].argmax()))
        if t + 1 < n_answer:
            roll.append(eng.decode(state, torch.tensor([a[-1]])).float().cpu()[0])
    ids = torch.cat([prompt, torch.tensor(a[:-1], dtype=torch.long)])[None]
    mask = torch.ones_like(ids)
    tf = eng.score_rows(merged, ids, mask, [grid], n_answer).float().cpu()
    with torch.device("cuda:0"):
        o = QwenOracle(cfg, w, device="cuda:0")
        hid = o.forward(ids.cuda(), mask.cuda(), px.float().cuda(), [grid], return_stages=True)["hidden"]
        ref = (hid[0, -n_answer:].float() @ o._w("lm_head.weight").t()).float().cpu()
    lp_ref, lp_tf, lp_roll = torch.log_softmax(ref, -1), torch.log_softmax(tf, -1), torch.log_softmax(torch.stack(roll), -1)
    per = [{"token": t, "id": a[t], "logp_fp32": float(lp_ref[t, a[t]]), "abs_dlogp_teacher_forcing": abs(float(lp_tf[t, a[t]] - lp_ref[t, a[t]])),
            "abs_dlogp_rollout": abs(float(lp_roll[t, a[t]] - lp_ref[t, a[t]]))} for t in range(n_answer)]
    return {"record": "parity", "model": "qwen2.5-vl-7b (seeded)", "sample": "one 8-frame 336x448 clip (768 vision tokens) + 40 text tokens",
            "answer_tokens": n_answer, "reference": "oracle/qwen25vl_oracle.py evaluated in fp32 by torch on the device", "per_token": per,
            "max_abs_dlogp_teacher_forcing": max(p["abs_dlogp_teacher_forcing"] for p in per),
            "max_abs_dlogp_rollout": max(p["abs_dlogp_rollout"] for p in per)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=64)
    ap.add_argument("--answers", type=int, nargs="+", default=[1, 4, 8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "qwen_teacher_forcing.jsonl"))
    ap.add_argument("--no-parity", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_qwen_teacher.py measures on an MI355X; no GPU here")
    m = make_model()
    m.device_preprocess, m.max_batch, m._gen_eos_ids = True, a.clips, []
    rng = np.random.RandomState(0)
    clips = [rng.randint(0, 256, (8, 336, 448, 3), dtype=np.uint8) for _ in range(a.clips)]
    recs = run_timing(m, clips, sorted(a.answers), a.reps)
    if not a.no_parity:
        recs.append(run_parity(m))
    with open(a.out, "a") as f:
        for r in recs:
            line = json.dumps(r)
            print(line, flush=True)
            f.write(line + "\n")


if __name__ == "__main__":
    main()
