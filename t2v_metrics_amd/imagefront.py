"""In-memory image entries of the CLIP-FlanT5 and CLIPScore rows, and the host side of their device front end (include/vqs.h vqs_images_u8).

An entry of an ``images`` list is a path (``str`` / ``os.PathLike``), a ``PIL.Image.Image``, a ``np.ndarray`` of uint8 [H, W, 3] RGB or a
``torch.Tensor`` of uint8 [H, W, 3] on the CPU or a GPU.  Paths are keyed by ``str(p)`` inside a call, in-memory entries by object identity
(the same object twice is one image; two equal-content objects are two).  The caller chooses the quantisation: float arrays are refused.

``image_plan`` folds ALL geometry of ``_imgprep.clip_preprocess_u8`` -- expand2square, the shortest-edge resize, the centre crop -- into the
argument set of the device call: a virtual canvas, and per axis either the rows [crop, crop + S) of Pillow's bicubic tables or a crop
offset.  ``device_pixels`` runs the front end for the in-memory entries of one ``load_images`` chunk, one call per source size.
"""
from __future__ import annotations

import os
from functools import lru_cache
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch
from PIL import Image

from ._imgprep import OPENAI_CLIP_MEAN


def is_path(p) -> bool:
    return isinstance(p, (str, os.PathLike))


def _describe(p) -> str:
    return f"dtype {p.dtype}, shape {tuple(p.shape)}"


def check_entry(p) -> None:
    """Raise for anything that is not a legal ``images`` entry -- before any decode or engine call."""
    if is_path(p):
        return
    if isinstance(p, Image.Image):
        if p.size[0] <= 0 or p.size[1] <= 0:
            raise ValueError(f"empty PIL image (size {p.size})")
        return
    if isinstance(p, (np.ndarray, torch.Tensor)):
        if p.dtype != (torch.uint8 if isinstance(p, torch.Tensor) else np.uint8):
            raise TypeError(f"in-memory images must be uint8 [H, W, 3] RGB (quantise floats yourself: the library does not guess the range); got {_describe(p)}")
        if p.ndim != 3 or p.shape[2] != 3:
            raise ValueError(f"in-memory images must be uint8 [H, W, 3] RGB (channels last); got {_describe(p)}")
        if p.shape[0] == 0 or p.shape[1] == 0:
            raise ValueError(f"empty image; got {_describe(p)}")
        return
    raise TypeError(f"an image must be a path, a PIL.Image, a uint8 np.ndarray [H, W, 3] or a uint8 torch.Tensor [H, W, 3]; got {type(p).__name__}")


def dedupe(images: Sequence) -> Tuple[list, List[int]]:
    """-> (distinct entries in order of first appearance, index of every input into them); every entry is checked first."""
    uniq: Dict[object, int] = {}
    entries, index = [], []
    for p in images:
        check_entry(p)
        key = str(p) if is_path(p) else ("mem", id(p))
        if key not in uniq:
            uniq[key] = len(entries)
            entries.append(p)
        index.append(uniq[key])
    return entries, index


def entry_hw(p) -> Tuple[int, int]:
    if isinstance(p, Image.Image):
        return p.size[1], p.size[0]
    return int(p.shape[0]), int(p.shape[1])


def entry_array(p) -> np.ndarray:
    """An in-memory entry as a host uint8 [H, W, 3] RGB array (a device tensor is copied to the host)."""
    if isinstance(p, Image.Image):
        return np.asarray(p.convert("RGB"))
    if isinstance(p, torch.Tensor):
        return p.detach().cpu().numpy()
    return p


def entry_image(p) -> Image.Image:
    """An in-memory entry as the PIL image the host path preprocesses (what the same pixels read from a lossless file give)."""
    if isinstance(p, Image.Image):
        return p.convert("RGB")
    return Image.fromarray(np.ascontiguousarray(entry_array(p)), "RGB")


class ImagePlan(NamedTuple):
    """The argument set of vqs_images_u8 for sources of one size (fields as in include/vqs.h vqs_image_geometry)."""
    H: int
    W: int
    S: int
    Hc: int
    Wc: int
    oy: int
    ox: int
    color: Tuple[int, int, int]
    resized_h: int
    resized_w: int
    crop_y: int
    crop_x: int
    first_h: Optional[np.ndarray]      # int32 [S], canvas columns; None: the width is not resampled
    weights_h: Optional[np.ndarray]    # int32 [S, taps_h]
    first_v: Optional[np.ndarray]
    weights_v: Optional[np.ndarray]
    row0: int                          # canvas rows [row0, row0 + rows) the horizontal pass has to compute
    rows: int


@lru_cache(maxsize=64)
def image_plan(H: int, W: int, S: int, pad: bool) -> ImagePlan:
    """clip_preprocess_u8(image of H x W, S, pad) as canvas + sliced tables.  The resized lengths are _resize_shortest_edge's, including its
    int(S * long / short) and the short == S early return (neither axis is resampled then); Pillow skips the pass of an axis whose length
    does not change."""
    from .qwen.media import pillow_bicubic_tables
    if pad:
        Hc = Wc = max(H, W)
        oy, ox = (Hc - H) // 2, (Wc - W) // 2
    else:
        Hc, Wc, oy, ox = H, W, 0, 0
    short, long = min(Hc, Wc), max(Hc, Wc)
    if short == S:
        rh, rw = Hc, Wc
    else:
        new_long = int(S * long / short)
        rw, rh = (S, new_long) if Wc <= Hc else (new_long, S)
    if rh < S or rw < S:
        raise ValueError(f"{H} x {W} resizes to {rh} x {rw}, smaller than the crop {S}")
    crop_y, crop_x = (rh - S) // 2, (rw - S) // 2

    def axis(n_in, n_out, crop):
        if n_in == n_out:
            return None, None
        first, weights = pillow_bicubic_tables(n_in, n_out)
        return np.ascontiguousarray(first[crop: crop + S]), np.ascontiguousarray(weights[crop: crop + S])

    first_h, weights_h = axis(Wc, rw, crop_x)
    first_v, weights_v = axis(Hc, rh, crop_y)
    if first_v is None:
        row0, rows = crop_y, S
    else:                               # zero-padded taps may reach past the last weighted row: harmless, they weigh nothing
        row0 = int(first_v.min())
        rows = min(Hc, int(first_v.max()) + weights_v.shape[1]) - row0
    return ImagePlan(H, W, S, Hc, Wc, oy, ox, tuple(int(m * 255) for m in OPENAI_CLIP_MEAN), rh, rw, crop_y, crop_x, first_h, weights_h,
                     first_v, weights_v, row0, rows)


class SourceStaging:
    """One pinned uint8 buffer for the uploads of in-memory sources, grown on demand and handed out again only after the copy that last read
    it has completed (its event) -- the rule of CLIPT5Model._staging_buffer.  The buffer is as large as the largest group the model has
    uploaded (n * H * W * 3 bytes: 805 MB after 256 images of 1024 x 1024) and stays pinned for the model's lifetime, as the uint8 staging
    buffers of the host path do; ``release()`` gives it back."""

    def __init__(self):
        self.buf, self.event = None, None

    def release(self) -> None:
        if self.event is not None:
            self.event.synchronize()
        self.buf, self.event = None, None

    def take(self, nbytes: int) -> torch.Tensor:
        if self.event is not None:
            self.event.synchronize()
        if self.buf is None or self.buf.numel() < nbytes:
            self.buf = torch.empty(nbytes, dtype=torch.uint8).pin_memory()
        return self.buf[:nbytes]


def device_pixels(engine, device, staging: SourceStaging, entries: Sequence, S: int, pad: bool, pool=None) -> List[Tuple[List[int], torch.Tensor]]:
    """The device front end for in-memory `entries` (positions are indices into it): grouped by source (H, W), each group uploaded once as
    uint8 [n, H, W, 3] through pinned staging -- or gathered on the device where the entries already live there, with no host round trip --
    and turned into bf16 [n, 3, S, S] by ONE engine.images_from_u8 call.  -> [(positions, pixels)] per group.  May run on an image thread:
    the copies, the staging event and the launches sit on `device` and its current stream."""
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i, p in enumerate(entries):
        groups.setdefault(entry_hw(p), []).append(i)
    out = []
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream(device)
        for (H, W), idx in groups.items():
            on_dev = [i for i in idx if isinstance(entries[i], torch.Tensor) and entries[i].is_cuda]
            on_host = [i for i in idx if not (isinstance(entries[i], torch.Tensor) and entries[i].is_cuda)]
            if not on_host:
                src = torch.stack([entries[i].to(device) for i in on_dev])
            else:
                per = H * W * 3
                host = staging.take(len(on_host) * per)
                view = host.numpy().reshape(len(on_host), H, W, 3)

                def put(j):
                    view[j] = entry_array(entries[on_host[j]])

                if pool is not None and len(on_host) > 1 and len(on_host) * per >= (8 << 20):      # numpy's copy releases the GIL
                    list(pool.map(put, range(len(on_host))))
                else:
                    for j in range(len(on_host)):
                        put(j)
                src = torch.empty(len(idx), H, W, 3, dtype=torch.uint8, device=device)
                src[: len(on_host)].view(-1).copy_(host, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(stream)
                staging.event = ev
                for j, i in enumerate(on_dev):
                    src[len(on_host) + j].copy_(entries[i])
            out.append((on_host + on_dev, engine.images_from_u8(src, S, pad)))
    return out


def load_pixels(engine, device, staging: SourceStaging, image: Sequence, S: int, pad: bool, host_path, pool=None) -> torch.Tensor:
    """load_images with the device front end on: the in-memory entries of `image` through device_pixels, the paths through
    `host_path(list of paths) -> bf16 [k, 3, S, S]` (the model's host front end), rows back in the order of `image`."""
    held = [i for i, p in enumerate(image) if not is_path(p)]
    rest = [i for i, p in enumerate(image) if is_path(p)]
    parts = [([held[j] for j in pos], px) for pos, px in device_pixels(engine, device, staging, [image[i] for i in held], S, pad, pool)]
    if rest:
        parts.append((rest, host_path([image[i] for i in rest])))
    with torch.cuda.device(device):
        return scatter_rows(parts, len(image))


def scatter_rows(parts: List[Tuple[List[int], torch.Tensor]], n: int) -> torch.Tensor:
    """[(positions, rows)] -> one tensor of n rows in position order (a single part that is already in order is returned as it is)."""
    if len(parts) == 1 and parts[0][0] == list(range(n)):
        return parts[0][1]
    ref = parts[0][1]
    out = torch.empty((n,) + tuple(ref.shape[1:]), dtype=ref.dtype, device=ref.device)
    for idx, rows in parts:
        if idx == list(range(idx[0], idx[0] + len(idx))):
            out[idx[0]: idx[0] + len(idx)] = rows
        else:
            out[torch.as_tensor(idx, device=ref.device)] = rows.to(ref.device)
    return out
