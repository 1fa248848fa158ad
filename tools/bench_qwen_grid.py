#!/usr/bin/env python3
"""Grid timing of the Qwen2.5-VL row with and without the shared prompt prefix (QwenEngine.score_shared): seeded 7B weights, M videos
(8 frames at 336 x 448 = 768 vision tokens each) x N questions per call (forward_grid, one scorer call), N in --questions.  Per grid:
ms per call (median of --reps after one warm-up), pairs/s, language-model rows per pair, and whether the two forms' scores are
bitwise equal.  One JSON line per (N, form) on stdout.  The new kernels' share of kernel time: run one form under
rocprofv3 --kernel-trace --stats (profiles/shared_prefix_rocprof_7b_summary.md).
  python tools/bench_qwen_grid.py [--videos 8] [--questions 1 2 8] [--reps 3] [--forms both|on|off]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from t2v_metrics_amd.models.vqascore_models.qwen25vl_model import Qwen25VLModel  # noqa: E402
from t2v_metrics_amd.qwen import get_qwen_config  # noqa: E402
from t2v_metrics_amd.qwen.layout import shared_prefix_plan  # noqa: E402
from test_qwen_host import FakeQwenTokenizer  # noqa: E402

QUESTIONS = ["a person waves at the camera", "a car turns left", "the camera pans to the right", "two dogs play in the snow",
             "a man rides a bicycle down a hill", "the camera zooms in on a face", "rain falls on a city street at night", "a red ball"]


def lm_rows(m, paths, texts, n_tok):
    """language-model rows per pair: unshared = the padded prompt length of each chunk; shared = (U * Lp + B * Ls) / B"""
    rows_off = rows_on = 0
    pairs = [(p, t) for p in paths for t in texts]
    for s in range(0, len(pairs), m.max_batch):
        chunk = pairs[s: s + m.max_batch]
        ids = [m.build_ids(m_q(t), "video", n_tok) for _, t in chunk]
        B, L = len(ids), max(len(r) for r in ids)
        x = torch.zeros(B, L, dtype=torch.long)
        mask = torch.zeros(B, L, dtype=torch.long)
        for k, r in enumerate(ids):
            x[k, : len(r)] = torch.tensor(r)
            mask[k, : len(r)] = 1
        rows_off += B * L
        plan = shared_prefix_plan(m.cfg, x, mask, [(4, 24, 32)] * B, [p for p, _ in chunk])
        rows_on += B * L if plan is None else plan["U"] * plan["Lp"] + B * plan["Ls"]
    return rows_off / len(pairs), rows_on / len(pairs)


class Tokenizer7B(FakeQwenTokenizer):
    """the test tokenizer with the 7B checkpoint's special-token ids (words hash into the vocabulary below them)"""

    def __init__(self, cfg):
        super().__init__(151643)
        self.specials = {"<|im_start|>": 151644, "<|im_end|>": 151645, "<|vision_start|>": cfg.vision_start_token_id,
                         "<|vision_end|>": cfg.vision_end_token_id, "<|video_pad|>": cfg.video_token_id, "<|image_pad|>": cfg.image_token_id}

    def encode(self, text, add_special_tokens=False):
        for s in self.specials:
            text = text.replace(s, f" {s} ")
        return [self.specials[w] if w in self.specials else 10 + zlib.crc32(w.encode()) % (self.vocab - 10) for w in text.split()]


def m_q(t):
    return 'Does this figure show "{}"? Please answer Yes or No.'.format(t)


def make_model():
    cfg = get_qwen_config("qwen2.5-vl-7b")
    return Qwen25VLModel(model_name="qwen2.5-vl-7b", device="cuda", config=cfg, weights="seeded", tokenizer=Tokenizer7B(cfg))


def make_videos(n, directory, seed=0):
    rng = np.random.RandomState(seed)
    paths = []
    for i in range(n):
        p = os.path.join(directory, f"v{i}.npy")
        np.save(p, rng.randint(0, 256, (8, 336, 448, 3), dtype=np.uint8))
        paths.append(p)
    return paths


def run_grid(m, paths, questions, reps, forms=(False, True)):
    """-> JSON records: per (N, form) the timing, per N whether the two forms' scores are bitwise equal (when both ran)"""
    n_tok = 4 * 24 * 32 // 4
    out = []
    for n in questions:
        texts = QUESTIONS[:n]
        off_rows, on_rows = lm_rows(m, paths, texts, n_tok)
        scores = {}
        for share in forms:
            m.share_prefix = share
            m.forward_grid(paths, texts)
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                t0 = time.perf_counter()
                s = m.forward_grid(paths, texts)
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            scores[share] = s
            ms = statistics.median(ts)
            out.append({"videos": len(paths), "questions": n, "share_prefix": share, "ms_per_grid": round(ms, 1), "ms_all": [round(t, 1) for t in ts],
                        "pairs_per_s": round(len(paths) * n / ms * 1e3, 2), "lm_rows_per_pair": round(on_rows if share else off_rows, 1)})
        if len(scores) == 2:
            out.append({"videos": len(paths), "questions": n, "scores_bitwise_equal": bool(torch.equal(scores[False], scores[True]))})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=8)
    ap.add_argument("--questions", type=int, nargs="+", default=[1, 2, 8])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--forms", default="both", choices=["both", "on", "off"],
                    help="sharing off and on (default), or one form only (a rocprofv3 kernel trace of one form)")
    a = ap.parse_args()
    m = make_model()
    forms = {"both": (False, True), "on": (True,), "off": (False,)}[a.forms]
    for rec in run_grid(m, make_videos(a.videos, tempfile.mkdtemp()), a.questions, a.reps, forms):
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
