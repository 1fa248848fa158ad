"""Host side of the Qwen2.5-VL media front end (include/vqs_qwen.h vqs_qwen_patches_u8): the float tail of the processor as ONE
expression (`normalize_frames`, which `Qwen25VLModel.preprocess` calls and `normalize_lut` tabulates for the device), and Pillow's
8-bit bicubic resampler restated as tables + integer passes (`pillow_bicubic_tables`, `bicubic_resize_u8`).  Pure host code; the
installed Pillow is the authority (tests/test_qwen_media_host.py compares bit for bit)."""
from __future__ import annotations

from functools import lru_cache
from typing import Tuple

import numpy as np
import torch

OPENAI_CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
OPENAI_CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
PRECISION_BITS = 32 - 8 - 2          # Pillow src/libImaging/Resample.c: 8-bit pixels, 2 bits of headroom for the bicubic's overshoot


def normalize_frames(frames_u8: np.ndarray) -> torch.Tensor:
    """uint8 [T, H, W, 3] -> fp32 [T, 3, H, W]: rescale by 1/255, then CLIP mean / std (the HF processor's fp32 arithmetic)."""
    x = torch.from_numpy(np.ascontiguousarray(frames_u8)).permute(0, 3, 1, 2).to(torch.float32) * (1.0 / 255.0)
    mean = torch.tensor(OPENAI_CLIP_MEAN).view(1, 3, 1, 1)
    std = torch.tensor(OPENAI_CLIP_STD).view(1, 3, 1, 1)
    return (x - mean) / std


def normalize_lut() -> torch.Tensor:
    """bf16 [3, 256]: normalize_frames of every uint8 value per channel, rounded as the upload rounds (.to(bfloat16)) -- a uint8 input
    has 256 values per channel, so the device looks the result up instead of re-deriving the fp32 arithmetic."""
    v = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None, None], 3, axis=3)          # [1, 256, 1, 3]: a 256 x 1 "frame"
    return normalize_frames(v)[0, :, :, 0].to(torch.bfloat16).contiguous()


def _bicubic(x: float, a: float = -0.5) -> float:
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


@lru_cache(maxsize=64)
def pillow_bicubic_tables(n_in: int, n_out: int) -> Tuple[np.ndarray, np.ndarray]:
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for one axis of Image.resize(..., BICUBIC) on 8-bit pixels
    -> (first_tap int32 [n_out], weights int32 [n_out, taps]): output i = clip8(((1 << 21) + sum_j weights[i, j] * px[first_tap[i] + j]) >> 22).
    Rows shorter than `taps` (at the borders) are zero-padded.  The tap count grows with the downscale factor."""
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    first = np.zeros(n_out, dtype=np.int32)
    rows = []
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in)
        w = [_bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        first[i] = xmin
        rows.append([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w])
    taps = max(len(r) for r in rows)
    weights = np.zeros((n_out, taps), dtype=np.int32)
    for i, r in enumerate(rows):
        weights[i, : len(r)] = r
    first.setflags(write=False)
    weights.setflags(write=False)
    return first, weights


def _resample_axis0(a: np.ndarray, n_out: int) -> np.ndarray:
    first, weights = pillow_bicubic_tables(a.shape[0], n_out)
    idx = np.minimum(first[:, None].astype(np.int64) + np.arange(weights.shape[1])[None], a.shape[0] - 1)      # padded taps weigh 0
    acc = np.einsum("ij,ij...->i...", weights.astype(np.int64), a.astype(np.int64)[idx]) + (1 << (PRECISION_BITS - 1))
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def bicubic_resize_u8(frames_u8: np.ndarray, rh: int, rw: int) -> np.ndarray:
    """uint8 [..., H, W, 3] -> uint8 [..., rh, rw, 3]: the two integer passes of Pillow's resampler (horizontal, then vertical, each
    rounding to uint8; a pass is skipped when its axis keeps its size) -- what the device kernels compute."""
    a = np.asarray(frames_u8)
    H, W = a.shape[-3], a.shape[-2]
    if rw != W:
        a = np.moveaxis(_resample_axis0(np.moveaxis(a, -2, 0), rw), 0, -2)
    if rh != H:
        a = np.moveaxis(_resample_axis0(np.moveaxis(a, -3, 0), rh), 0, -3)
    return np.ascontiguousarray(a)
