"""Shared by tests/test_image_frontend_host.py and tests/test_gpu_image_frontend.py: the case list of the image front end
(include/vqs.h vqs_images_u8), its source images, and a numpy restatement of the DEVICE arithmetic that reads nothing but the argument
set of the C call (imagefront.ImagePlan: canvas, offsets, colour, sliced tables or crop offsets) -- two integer passes."""
import numpy as np

# (S, (H, W), n): the sizes at which the kernels take another path
CASES_56 = [
    (56, (61, 45), 1), (56, (45, 61), 1),          # odd pad offsets
    (56, (56, 56), 1),                             # no pass at all
    (56, (56, 100), 1), (56, (100, 56), 1),        # crop only without pad; both axes resampled with pad
    (56, (20, 300), 1), (56, (300, 20), 1),        # output windows wholly inside the padding
    (56, (17, 17), 1),                             # upscale, 5 taps
    (56, (200, 301), 1),                           # 4 to 5 x downscale, the most taps
    (56, (61, 45), 3),                             # per-image strides
]
# 42: a legal size no vector width divides (the scalar store path) -- resample, crop only, the most taps
CASES_42 = [(42, (61, 45), 1), (42, (42, 80), 1), (42, (200, 301), 2)]
SMALL_CASES = [(S, hw, n, pad, kind) for (S, hw, n) in CASES_56 + CASES_42 for pad in (True, False) for kind in ("random", "noise")]
# one case each at real size
REAL_CASES = [(336, (768, 1024), 1, True, "random"), (224, (512, 768), 1, False, "random")]


def case_id(c):
    S, (H, W), n, pad, kind = c
    return f"S{S}-{H}x{W}-n{n}-{'pad' if pad else 'nopad'}-{kind}"


def make_images(kind, n, H, W, seed=0):
    """uint8 [n, H, W, 3]: 'random' = uniform bytes, 'noise' = 0 / 255 only (drives the bicubic overshoot into both clamps)"""
    rng = np.random.RandomState(seed + 1000 * H + W)
    if kind == "noise":
        return (rng.randint(0, 2, (n, H, W, 3)) * 255).astype(np.uint8)
    return rng.randint(0, 256, (n, H, W, 3), dtype=np.uint8)


def _clip8_q22(acc):
    return np.clip(acc >> 22, 0, 255)


def folded_reference(a, plan):
    """a uint8 [H, W, 3] -> uint8 [S, S, 3]: what the two device passes compute from `plan` alone."""
    H, W, S = plan.H, plan.W, plan.S
    assert a.shape == (H, W, 3)
    color = np.asarray(plan.color, dtype=np.int64)

    def canvas(rows, cols):
        """the virtual canvas at rows x cols (index arrays that broadcast): the source inside its rectangle, the colour elsewhere"""
        rows, cols = np.broadcast_arrays(rows, cols)
        sy, sx = rows - plan.oy, cols - plan.ox
        inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        out = np.broadcast_to(color, rows.shape + (3,)).copy()
        out[inside] = a[sy[inside], sx[inside]]
        return out

    if plan.weights_h is not None:                    # horizontal pass over the kept canvas rows only
        taps = plan.weights_h.shape[1]
        first = np.clip(plan.first_h.astype(np.int64), 0, plan.Wc - 1)
        cols = np.minimum(first[:, None] + np.arange(taps)[None], plan.Wc - 1)                     # [S, taps]
        win = np.arange(plan.row0, plan.row0 + plan.rows)
        mid = np.empty((plan.rows, S, 3), dtype=np.int64)
        for r0 in range(0, plan.rows, 64):
            px = canvas(win[r0: r0 + 64, None, None], cols[None])                                  # [rows, S, taps, 3]
            mid[r0: r0 + 64] = _clip8_q22((1 << 21) + np.einsum("xt,rxtc->rxc", plan.weights_h.astype(np.int64), px))

        def read(rows):                               # [k] canvas rows -> [k, S, 3]; rows clamped to the window kept
            return mid[np.clip(rows - plan.row0, 0, plan.rows - 1)]
    else:
        def read(rows):
            return canvas(rows[:, None], (plan.crop_x + np.arange(S))[None])

    if plan.weights_v is not None:
        taps = plan.weights_v.shape[1]
        first = np.clip(plan.first_v.astype(np.int64), 0, plan.Hc - 1)
        rows = np.minimum(first[:, None] + np.arange(taps)[None], plan.Hc - 1)                     # [S, taps]
        px = read(rows.reshape(-1)).reshape(S, taps, S, 3)
        out = _clip8_q22((1 << 21) + np.einsum("yt,ytxc->yxc", plan.weights_v.astype(np.int64), px))
    else:
        out = read(plan.crop_y + np.arange(S))
    return out.astype(np.uint8)
