#!/usr/bin/env python3
"""What the image front end of the CLIP-FlanT5 row costs for IN-MEMORY images through the drop-in API, on the host (device_preprocess=False:
expand2square + PIL resize + crop on the thread pool, uint8 [S, S, 3] upload, vqs_normalize_u8) and on the device (True: the uint8 sources
go up through pinned staging, vqs_images_u8).  Seeded clip-flant5-xl weights, ONE scorer whose switch is flipped between calls, n distinct
in-memory uint8 images with one text each per `forward` call; the two settings alternate, one warm-up call each, then --reps timed calls each
(host clock around a call that ends in the scores on the host).  Per (n, size): median and min / max ms per call for both settings, the
front-end stage alone (images -> bf16 pixels on the device, synchronised) for both, the engine.images_from_u8 call alone on sources already
on the GPU (host clock around ~50 ms of back-to-back calls ended by one synchronise: both launches plus the call's allocations, not a kernel trace),
whether the scores are bitwise equal, and the bytes the device front end must move (source + intermediate written and read + result) over
the stage's and that call's time, beside the ~6 TB/s the norm kernels reach.  One JSON line each on stdout (and written to --out).
  python tools/bench_image_frontend.py [--images 8 64 256] [--sizes 1024x1024 768x512] [--reps 3] [--out profiles/clip_image_frontend.jsonl]"""
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

import t2v_metrics_amd as t2v  # noqa: E402
from bench_pipeline import WordTokenizer  # noqa: E402

CALL_WINDOW_MS = 50.0           # the device call alone is timed over this many ms of back-to-back calls
NORM_KERNEL_TBPS = 6.0          # about what the register-resident norm kernels reach on this device (README: 5.5-5.9 TB/s)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "calls": len(xs)}


def front_end_only(m, images):
    """images -> bf16 pixels on the device, chunked as forward() chunks them, under the current setting"""
    return [m.load_images(images[s: s + m.max_images]) for s in range(0, len(images), m.max_images)]


def run(m, n, H, W, reps):
    from t2v_metrics_amd.imagefront import image_plan
    rng = np.random.RandomState(0)
    images = [rng.randint(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(n)]
    texts = [f"a photo number {i} of someone doing something in place {i}" for i in range(n)]
    S, pad = m.cfg.vision.image, m.image_aspect_ratio == 'pad'
    times, stage, scores = {False: [], True: []}, {False: [], True: []}, {}
    for rep in range(reps + 1):                                   # rep 0 warms both settings up
        for on in (False, True):
            m.device_preprocess = on
            ms, s = timed(lambda: m.forward(images, texts))
            ms_stage, _ = timed(lambda: front_end_only(m, images))
            if rep:
                times[on].append(ms)
                stage[on].append(ms_stage)
            scores[on] = s
    # the device call alone: the sources of one chunk already on the device
    k = min(n, m.max_images)
    src = torch.from_numpy(np.stack(images[:k])).cuda()
    one, _ = timed(lambda: m.engine.images_from_u8(src, S, pad))                  # warm-up (tables, allocator) and a first estimate
    one, _ = timed(lambda: m.engine.images_from_u8(src, S, pad))
    loops = max(4, int(CALL_WINDOW_MS / max(one, 1e-3)) + 1)                      # back-to-back calls for a window of tens of ms, one sync
    kern = []
    for rep in range(reps):
        ms, _ = timed(lambda: [m.engine.images_from_u8(src, S, pad) for _ in range(loops)][-1])
        kern.append(ms / loops * n / k)
    del src
    plan = image_plan(H, W, S, pad)
    mid = plan.rows * S * 3 if plan.weights_h is not None else 0
    moved = n * (H * W * 3 + 2 * mid + 3 * S * S * 2)
    off, on = stats(times[False]), stats(times[True])
    st_on, kn = stats(stage[True]), stats(kern)
    tbps = lambda ms: moved / (ms * 1e-3) / 1e12              # noqa: E731
    return {"images": n, "source": [H, W], "size": S, "pad": pad, "u8_source_bytes": n * H * W * 3, "device_front_end_bytes_moved": moved,
            "forward_off": off, "forward_on": on, "forward_on_over_off": round(on["median_ms"] / off["median_ms"], 4),
            "front_end_off": stats(stage[False]), "front_end_on": st_on, "device_call_looped": dict(kn, calls_per_window=loops),
            "front_end_on_TBps": round(tbps(st_on["median_ms"]), 4), "device_call_TBps": round(tbps(kn["median_ms"]), 4),
            "device_call_fraction_of_norm_kernel_rate": round(tbps(kn["median_ms"]) / NORM_KERNEL_TBPS, 4),
            "front_end_on_fraction_of_norm_kernel_rate": round(tbps(st_on["median_ms"]) / NORM_KERNEL_TBPS, 4),
            "images_per_s_off": round(n / off["median_ms"] * 1e3, 1), "images_per_s_on": round(n / on["median_ms"] * 1e3, 1),
            "scores_bitwise_equal": bool(torch.equal(scores[False], scores[True]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, nargs="+", default=[8, 64, 256])
    ap.add_argument("--sizes", nargs="+", default=["1024x1024", "768x512"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model", default="clip-flant5-xl")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_image_frontend.py measures on the GPU; there is none here")
    from t2v_metrics_amd.config import get_config
    cfg = get_config(a.model)
    m = t2v.VQAScore(model=a.model, device="cuda", weights="seeded", tokenizer=WordTokenizer(cfg.t5.vocab)).model
    head = {"what": "ms per CLIPT5Model.forward call on in-memory uint8 images, device_preprocess off (the host front end) and on, alternating in one process",
            "model": a.model + " seeded", "device": torch.cuda.get_device_name(0), "max_images": m.max_images, "max_pairs": m.max_pairs,
            "num_workers": m.num_workers, "reps": a.reps, "norm_kernel_TBps": NORM_KERNEL_TBPS}
    lines = [head]
    print(json.dumps(head), flush=True)
    for size in a.sizes:
        H, W = (int(x) for x in size.split("x"))
        for n in a.images:
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
