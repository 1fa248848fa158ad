#!/usr/bin/env python3
"""Throughput of the CLIPScore row on seeded weights: images/s of the image half, texts/s of the text half and pairs/s of an
M x N grid (distinct images and texts encoded once each, one similarity launch) -- by default 256 synthetic images x 256 texts of
mixed lengths on ``openai:ViT-L-14`` (224 px, the image size the main bench's synthetic images have).  Prints one JSON line and,
with --out, appends it to a file (profiles/clipscore_bench.jsonl on the GPU run).

Timing: every shape is warmed up first; each figure is the median of --steps windows, each window a host clock around work that
ends in a device synchronise and repeated until it covers at least --min-window seconds; the spread (min / max window) is
reported with it.  There is no parent-commit figure to compare with: the record is the deliverable.  As a cross-check the image
half is set against the tower's share of the CLIP-FlanT5 encode stage measured in the same process (the same launches for 23 of
the 24 layers plus the mlp2x projector on 2048-wide features): --compare-encode times vqs_encode_images on the same pixels."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps, min_window):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    one = max(time.perf_counter() - t0, 1e-6)
    reps = max(1, int(min_window / one + 0.999))
    out = []
    for _ in range(steps):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps)
    return {"s": statistics.median(out), "min_s": min(out), "max_s": max(out), "reps": reps, "windows": steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="openai:ViT-L-14")
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--texts", type=int, default=256)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--min-window", type=float, default=1.0)
    ap.add_argument("--fp16", type=int, default=1)
    ap.add_argument("--compare-encode", type=int, default=1, help="also time the CLIP-FlanT5 row's vqs_encode_images (XL) on the same pixels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from t2v_metrics_amd.clip.config import get_clip_config
    from t2v_metrics_amd.clip.engine import ClipEngine
    from t2v_metrics_amd.clip.weights import make_seeded_clip_weights
    cfg = get_clip_config(args.model)
    dev = torch.device("cuda:0")
    eng = ClipEngine(cfg, make_seeded_clip_weights(cfg, seed=0, device="cpu"), device=dev, options={"fp16": args.fp16})
    g = torch.Generator().manual_seed(1234)
    M, N, t = args.images, args.texts, cfg.text
    px = torch.randn(M, 3, cfg.vision.image, cfg.vision.image, generator=g).to(torch.bfloat16).to(dev)
    lengths = torch.randint(5, t.context + 1, (N,), generator=g)
    lengths[0] = t.context                                    # the batch is padded to the context, as the HF tokenizer pads
    ids = torch.full((N, t.context), t.eot_id, dtype=torch.int32)
    for i, n in enumerate(lengths.tolist()):
        ids[i, 0] = t.bos_id
        ids[i, 1:n - 1] = torch.randint(1, min(t.bos_id, t.eot_id), (n - 2,), generator=g, dtype=torch.int32)
    pos = (lengths - 1).to(torch.int32)
    ids_d, pos_d = ids.to(dev), pos.to(dev)

    state = {}

    def f_img():
        state["img"] = eng.encode_images(px)

    def f_txt():
        state["txt"] = eng.encode_texts(ids_d, pos_d)

    def f_grid():
        f_img()
        f_txt()
        state["grid"] = eng.similarity(state["img"], state["txt"])

    for _ in range(args.warmup):
        f_grid()
    torch.cuda.synchronize()
    r_img, r_txt, r_grid = (timed(f, args.steps, args.min_window) for f in (f_img, f_txt, f_grid))
    grid = state["grid"]
    rec = {
        "tool": "bench_clipscore", "model": cfg.name, "image": cfg.vision.image, "images": M, "texts": N, "text_len": t.context,
        "fp16": eng.get_option("fp16"), "weights": "seeded", "device": torch.cuda.get_device_name(0),
        "images_per_s": M / r_img["s"], "texts_per_s": N / r_txt["s"], "pairs_per_s": M * N / r_grid["s"],
        "image_half": r_img, "text_half": r_txt, "grid": r_grid,
        "image_tflops": cfg.flops_image() * M / r_img["s"] / 1e12, "text_tflops": cfg.flops_text(t.context) * N / r_txt["s"] / 1e12,
        "grid_finite": bool(torch.isfinite(grid).all()), "grid_abs_max": float(grid.abs().max()),
    }
    eng.close()
    if args.compare_encode:
        # the CLIP-FlanT5 row's encode stage on the same pixels: 23 of the 24 tower layers (the same launches) + the projector
        from t2v_metrics_amd.config import ClipT5Config, T5Config, VisionConfig
        from t2v_metrics_amd.engine import VqsEngine
        from t2v_metrics_amd.weights import make_seeded_weights
        v = cfg.vision
        c5 = ClipT5Config(name="bench-encode", vision=VisionConfig(hidden=v.hidden, layers=v.layers, heads=v.heads, mlp=v.mlp, patch=v.patch, image=v.image),
                          t5=T5Config(d_model=2048, heads=32, d_kv=64, d_ff=5120, layers=1, dec_layers=1))
        e5 = VqsEngine(c5, make_seeded_weights(c5, seed=0, device="cpu"), device=dev)
        r_enc = timed(lambda: e5.encode_images(px), args.steps, args.min_window)
        tower_share = c5.flops_vit() / (c5.flops_vit() + c5.flops_projector())
        expect = r_enc["s"] * tower_share * v.layers / (v.layers - 1)
        rec["encode_stage"] = {"images_per_s": M / r_enc["s"], **r_enc, "tower_flop_share": tower_share,
                               "image_half_expected_s": expect, "image_half_over_expected": r_img["s"] / expect}
        e5.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
