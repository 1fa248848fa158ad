#!/usr/bin/env python3
"""What the media front end of the Qwen2.5-VL row costs through the drop-in API, on the host (device_preprocess=False: PIL resize, fp32
normalise + patchify on a thread pool, pageable upload of fp32 patch rows) and on the device (True: uint8 frames through pinned staging,
vqs_qwen_patches_u8).  Seeded 7B weights, ONE scorer whose switch is flipped between calls, n distinct in-memory 8-frame clips with one
question each per `forward` call; the two settings alternate, one warm-up call each, then --reps timed calls each (host clock around a
call that ends in the scores on the host).  Per (clips, size): median and min / max ms per call for both settings, the front-end stage
alone (frames -> bf16 patch rows on the device, synchronised), and whether the scores are bitwise equal.  One JSON line each on stdout
(and appended to --out).
  python tools/bench_qwen_frontend.py [--clips 8 64] [--sizes 336x448 360x640] [--reps 5] [--out profiles/qwen_device_frontend.jsonl]"""
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


def make_clips(n, H, W, frames=8, seed=0):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (frames, H, W, 3), dtype=np.uint8) for _ in range(n)]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def front_end_only(m, clips):
    """frames -> bf16 patch rows on the device, as forward() gets them under the current setting"""
    prepared, _, media_of = m._prepare_media(clips)
    us = list(dict.fromkeys(media_of))
    rows = []
    for s in range(0, len(us), m.max_batch):
        x = m._window_patches(prepared, us[s: s + m.max_batch])
        rows.append(x.to(m.engine.device, torch.bfloat16))
    return rows


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 2), "min_ms": round(min(xs), 2), "max_ms": round(max(xs), 2), "calls": len(xs)}


def run(m, n, H, W, reps):
    clips = make_clips(n, H, W)
    texts = [QUESTIONS[i % len(QUESTIONS)] for i in range(n)]
    rh, rw = m._resized_hw(H, W)
    times = {False: [], True: []}
    stage = {False: [], True: []}
    scores = {}
    for rep in range(reps + 1):                                   # rep 0 warms both settings up
        for on in (False, True):
            m.device_preprocess = on
            ms, s = timed(lambda: m.forward(clips, texts))
            ms_stage, _ = timed(lambda: front_end_only(m, clips))
            if rep:
                times[on].append(ms)
                stage[on].append(ms_stage)
            scores[on] = s
    off, on = stats(times[False]), stats(times[True])
    return {"clips": n, "frames": 8, "source": [H, W], "resized": [rh, rw], "u8_bytes": int(sum(c.nbytes for c in clips)),
            "fp32_patch_row_bytes": int(n * 4 * (rh // 14) * (rw // 14) * 1176 * 4),
            "forward_off": off, "forward_on": on, "forward_on_over_off": round(on["median_ms"] / off["median_ms"], 4),
            "front_end_off": stats(stage[False]), "front_end_on": stats(stage[True]),
            "videos_per_s_off": round(n / off["median_ms"] * 1e3, 2), "videos_per_s_on": round(n / on["median_ms"] * 1e3, 2),
            "scores_bitwise_equal": bool(torch.equal(scores[False], scores[True]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--sizes", nargs="+", default=["336x448", "360x640"])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-batch", type=int, default=64)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_qwen_frontend.py measures on the GPU; there is none here")
    m = make_model()
    m.max_batch = a.max_batch
    head = {"what": "ms per Qwen25VLModel.forward call, device_preprocess off (the host front end) and on, alternating in one process",
            "model": "qwen2.5-vl-7b seeded", "device": torch.cuda.get_device_name(0), "max_batch": m.max_batch, "num_workers": m.num_workers,
            "reps": a.reps}
    lines = [head]
    print(json.dumps(head), flush=True)
    for size in a.sizes:
        H, W = (int(x) for x in size.split("x"))
        for n in a.clips:
            rec = run(m, n, H, W, a.reps)
            lines.append(rec)
            print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for rec in lines:
                f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
