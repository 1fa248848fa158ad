"""Writes tests/golden/clipscore_tiny.npz: the clip-tiny configuration on seeded weights through HF ``transformers`` ``CLIPModel`` in
fp32 (ids, pixels, unit embeddings, cosine grid) and the grid of HF's bf16 execution (the tolerance's yardstick; the ranking check's
coverage is verified here, on the CPU).  Run from the repository root: python tests/golden/make_clipscore_tiny.py"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from t2v_metrics_amd.clip.config import get_clip_config  # noqa: E402
from tests import clip_truth as ct  # noqa: E402

SEED = 0


def main():
    cfg = get_clip_config("clip-tiny")
    W = ct.seeded_weights(cfg, SEED)
    px, ids, pos = ct.seeded_inputs(cfg, 4, [3, 5, 8, 12, 17, 21], seed=SEED + 1)
    img, txt, grid = ct.hf_grid(cfg, W, px, ids, torch.float32)
    _, _, grid16 = ct.hf_grid(cfg, W, px, ids, torch.bfloat16)
    f = ct.parity_figures(grid16, grid, grid16)
    print(f)
    assert f["coverage"] >= 0.5, "pick another seed: too many text pairs closer than 2 e_ref16"
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "clipscore_tiny.npz"), seed=np.int64(SEED), pixels=px.float().numpy(),
                        ids=ids.numpy(), eot_pos=pos.numpy(), image_embeds=img.numpy(), text_embeds=txt.numpy(), grid=grid.numpy(),
                        grid_bf16=grid16.numpy())


if __name__ == "__main__":
    main()
