"""Host side of the Qwen2.5-VL media front end (t2v_metrics_amd/qwen/media.py, Qwen25VLModel's in-memory inputs), no GPU:
the tables + integer passes the device kernels run are Pillow's 8-bit bicubic resize bit for bit, the normalisation table is
`preprocess`'s fp32 expression rounded to bf16, np.ndarray media score like the same arrays saved as .npy, and the argument checks of
vqs_qwen_patches_u8 answer before any launch."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import t2v_metrics_amd as t2v
from t2v_metrics_amd.models.vqascore_models.qwen25vl_model import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, Qwen25VLModel
from t2v_metrics_amd.qwen import get_qwen_config
from t2v_metrics_amd.qwen.media import bicubic_resize_u8, normalize_lut, pillow_bicubic_tables
from t2v_metrics_amd.qwen.weights import make_seeded_qwen_weights
from tests.test_qwen_host import FakeQwenTokenizer, OracleQwenEngine

RESIZE_CASES = [((61, 45), (56, 84)), ((200, 300), (56, 84)), ((56, 84), (56, 84)), ((56, 100), (56, 84)), ((37, 53), (84, 112)),
                ((97, 131), (56, 56)), ((360, 640), (364, 644)), ((720, 1280), (364, 644))]


def _pixels(kind, shape, seed):
    rng = np.random.RandomState(seed)
    if kind == "random":
        return rng.randint(0, 256, shape, dtype=np.uint8)
    return (rng.randint(0, 2, shape) * 255).astype(np.uint8)          # 0 / 255 noise: the bicubic overshoots, the clip decides


@pytest.mark.parametrize("kind", ["random", "noise"])
@pytest.mark.parametrize("src,dst", RESIZE_CASES)
def test_tables_and_integer_passes_equal_pillow_bicubic(src, dst, kind):
    a = _pixels(kind, src + (3,), seed=src[0] * 7 + dst[1])
    want = np.asarray(Image.fromarray(a).resize((dst[1], dst[0]), Image.BICUBIC))
    got = bicubic_resize_u8(a, dst[0], dst[1])
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), int(np.abs(got.astype(int) - want.astype(int)).max())


def test_table_shapes_and_fixed_point_sums():
    for n_in, n_out in ((45, 84), (300, 84), (1280, 644), (640, 644), (84, 84)):
        first, w = pillow_bicubic_tables(n_in, n_out)
        assert first.dtype == np.int32 and w.dtype == np.int32 and first.shape == (n_out,) and w.shape[0] == n_out
        support = 2.0 * max(n_in / n_out, 1.0)
        assert w.shape[1] <= 2 * int(np.ceil(support)) + 1
        assert first.min() >= 0 and int((first + (w != 0).sum(1)).max()) <= n_in          # the real taps stay on the axis
        # the weights of one output are a rounded partition of 2^22, and with the negative lobes the int32 sums have room
        assert np.abs(w.astype(np.int64).sum(1) - (1 << 22)).max() <= w.shape[1]
        assert int(np.abs(w.astype(np.int64)).sum(1).max()) * 255 + (1 << 21) < 2 ** 31
    assert pillow_bicubic_tables(1280, 644)[1].shape[1] > pillow_bicubic_tables(640, 644)[1].shape[1]     # grows with the downscale


def test_normalize_lut_is_the_preprocess_expression_in_bf16():
    lut = normalize_lut()
    assert lut.dtype == torch.bfloat16 and tuple(lut.shape) == (3, 256)
    v = torch.arange(256, dtype=torch.uint8)
    frames = v.view(1, 16, 16, 1).expand(1, 16, 16, 3).contiguous()           # every value in every channel
    x = frames.permute(0, 3, 1, 2).to(torch.float32) * (1.0 / 255.0)
    want = ((x - torch.tensor(OPENAI_CLIP_MEAN).view(1, 3, 1, 1)) / torch.tensor(OPENAI_CLIP_STD).view(1, 3, 1, 1)).to(torch.bfloat16)
    assert torch.equal(lut, want.reshape(3, 256))
    # and through preprocess itself: a 56 x 56 image needs no resize, so its patch rows are the table's entries in patchify's order
    from t2v_metrics_amd.models.vqascore_models.qwen25vl_model import patchify
    cfg = get_qwen_config("qwen-tiny")
    m = Qwen25VLModel(model_name="qwen2.5-vl-7b", device="cpu", config=cfg, engine=object(), tokenizer=FakeQwenTokenizer(cfg.text.vocab))
    img = np.random.RandomState(0).randint(0, 256, (56, 56, 3), dtype=np.uint8)
    rows, grid = m.preprocess({"type": "image", "frames": img[None]})
    assert tuple(grid) == (1, 4, 4)
    looked_up = torch.stack([lut[c][torch.from_numpy(img[..., c]).long()] for c in range(3)])[None]          # bf16 [1, 3, 56, 56]
    assert torch.equal(rows.to(torch.bfloat16), patchify(looked_up.float(), 14, 2, 2)[0].to(torch.bfloat16))


def _scorer(engine=None, **kw):
    cfg = get_qwen_config("qwen-tiny")
    w = make_seeded_qwen_weights(cfg, seed=3, dtype=torch.bfloat16, lm_head_gain=4.0)
    eng = engine if engine is not None else OracleQwenEngine(cfg, w)
    return t2v.VQAScore(model="qwen2.5-vl-7b", device="cpu", config=cfg, engine=eng, tokenizer=FakeQwenTokenizer(cfg.text.vocab), **kw), eng


def test_ndarray_media_score_like_the_same_arrays_saved_as_npy(tmp_path):
    rng = np.random.RandomState(1)
    arrays = [rng.randint(0, 256, s, dtype=np.uint8) for s in [(4, 112, 112, 3), (3, 61, 45, 3), (112, 168, 3)]]
    paths = []
    for i, a in enumerate(arrays):
        np.save(tmp_path / f"a{i}.npy", a)
        paths.append(str(tmp_path / f"a{i}.npy"))
    texts = ["a cat jumps", "a dog runs fast", "two birds"]
    scorer, _ = _scorer()
    m = scorer.model
    from_files = m.forward(paths, texts)
    from_memory = m.forward(arrays, texts)
    assert torch.equal(from_memory, from_files)
    # mixed lists, the grid, the trace and generate take them as well
    assert torch.equal(m.forward([arrays[0], paths[1], arrays[2]], texts), from_files)
    assert torch.equal(m.forward_grid(arrays[:2], texts[:2]), m.forward_grid(paths[:2], texts[:2]))
    assert torch.equal(scorer(images=arrays[:2], texts=texts[:2]), scorer(images=paths[:2], texts=texts[:2]))
    s_a, tr_a = m.forward_with_trace(arrays[:1], texts[:1], max_new_tokens=2)
    s_p, tr_p = m.forward_with_trace(paths[:1], texts[:1], max_new_tokens=2)
    assert torch.equal(s_a, s_p) and tr_a[0]["generated_text"] == tr_p[0]["generated_text"]
    assert m.generate(arrays[1:], texts[1:], max_new_tokens=3) == m.generate(paths[1:], texts[1:], max_new_tokens=3)
    item = m.load_images([arrays[2], arrays[0]])
    assert [it["type"] for it in item] == ["image", "video"] and item[0]["frames"].shape == (1, 112, 168, 3)


def test_one_array_object_is_one_medium_and_bad_arrays_raise():
    rng = np.random.RandomState(2)
    a = rng.randint(0, 256, (2, 56, 56, 3), dtype=np.uint8)
    b = a.copy()
    scorer, eng = _scorer()
    m = scorer.model
    s = m.forward([a, a, a], ["one", "two", "three"])
    assert sum(len(c) for c in eng.vision_calls) == 1                  # three references, one tower pass
    eng.vision_calls.clear()
    s2 = m.forward([a, b, a], ["one", "two", "three"])                  # an equal COPY is another object: its own pass, the same scores
    assert sum(len(c) for c in eng.vision_calls) == 2 and torch.equal(s, s2)
    eng.vision_calls.clear()
    assert m.forward_grid([a, b], ["one", "two", "three"]).shape == (2, 3)
    assert sum(len(c) for c in eng.vision_calls) == 2                  # the grid: one pass per medium
    for bad in (a.astype(np.float32), a[0, :, :, 0], a[..., :2], a[None]):
        with pytest.raises(ValueError):
            m.forward([bad], ["x"])


def test_device_preprocess_falls_back_on_engines_without_the_front_end_and_groups_by_shape():
    rng = np.random.RandomState(3)
    arrays = [rng.randint(0, 256, s, dtype=np.uint8) for s in [(3, 61, 45, 3), (4, 56, 56, 3), (4, 61, 45, 3), (56, 84, 3)]]
    texts = ["a", "b c", "d", "e f g"]
    off, _ = _scorer()
    want = off.model.forward(arrays, texts)
    on, eng = _scorer(device_preprocess=True)
    assert on.model.device_preprocess and not off.model.device_preprocess
    assert torch.equal(on.model.forward(arrays, texts), want)          # the double has no patches_from_frames: the host path, silently

    cfg = get_qwen_config("qwen-tiny")

    class WithFrontEnd(OracleQwenEngine):
        """the double plus a front end that computes the host path's rows per clip and records its groups"""
        groups = []

        def patches_from_frames(self, clips, resized_hw):
            self.groups.append(([tuple(c.shape) for c in clips], tuple(resized_hw)))
            rows = [host.preprocess({"type": "video", "frames": c})[0] for c in clips]
            return torch.cat(rows).to(torch.bfloat16)

    host = off.model
    on2, eng2 = _scorer(engine=WithFrontEnd(cfg, make_seeded_qwen_weights(cfg, seed=3, dtype=torch.bfloat16, lm_head_gain=4.0)),
                        device_preprocess=True)
    got = on2.model.forward(arrays, texts)
    # grid (2, 4, 4): the 3-frame and the 4-frame (61, 45) clips (smart_resize: 56 x 56) and the 4-frame (56, 56) clip -> three groups in
    # ONE tower call; grid (1, 4, 6): the image
    assert sorted(len(c) for c in eng2.vision_calls) == [1, 3]
    assert sorted(eng2.groups) == sorted([([(3, 61, 45, 3)], (56, 56)), ([(4, 56, 56, 3)], (56, 56)), ([(4, 61, 45, 3)], (56, 56)),
                                          ([(1, 56, 84, 3)], (56, 84))])
    # the double's tower reads fp32 rows; these went through bf16, as on the device -- so compare with bf16-rounded host rows
    class Rounding(OracleQwenEngine):
        def encode_vision(self, patches, grids):
            return super().encode_vision(patches.to(torch.bfloat16), grids)

    ref, _ = _scorer(engine=Rounding(cfg, make_seeded_qwen_weights(cfg, seed=3, dtype=torch.bfloat16, lm_head_gain=4.0)))
    assert torch.equal(got, ref.model.forward(arrays, texts))


def test_patches_u8_argument_checks_answer_before_any_launch():
    """No device here: every call below must return from the size / pointer checks (a launch would fail with VQS_ERR_HIP = -4)."""
    from t2v_metrics_amd import engine
    from t2v_metrics_amd.qwen import engine as qengine
    lib = engine.load_library()
    for name in ("vqs_qwen_media_workspace_bytes", "vqs_qwen_patches_u8"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = qengine._SIGS[name]
    INVALID, WORKSPACE = -1, -3
    ws = lib.vqs_qwen_media_workspace_bytes
    assert ws(1, 3, 61, 45, 56, 84) >= 3 * 61 * 84 * 3 and ws(2, 3, 61, 45, 56, 84) >= 2 * 3 * 61 * 84 * 3
    assert ws(1, 4, 56, 84, 56, 84) == 256 and ws(1, 4, 200, 84, 56, 84) == 256          # no horizontal pass: nothing to keep
    assert ws(0, 4, 56, 84, 56, 84) == 0 and ws(1, 4, 56, 84, 0, 84) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)          # never dereferenced: the checks come first

    def call(rh=56, rw=84, H=61, W=45, x0h=p, kh=p, th=5, x0v=p, kv=p, tv=5, ws_ptr=p, ws_bytes=1 << 30, frames=p, lut=p, out=p, n=1, T=3,
             patch=14, merge=2, temporal=2):
        return lib.vqs_qwen_patches_u8(frames, n, T, H, W, rh, rw, x0h, kh, th, x0v, kv, tv, lut, patch, merge, temporal, out, ws_ptr, ws_bytes, None)

    assert call(rh=70) == INVALID and call(rw=98) == INVALID                # multiples of 14, not of 28
    assert call(n=0) == INVALID and call(T=0) == INVALID and call(patch=0) == INVALID
    assert call(frames=None) == INVALID and call(lut=None) == INVALID and call(out=None) == INVALID
    assert call(x0h=None) == INVALID and call(kh=None) == INVALID and call(th=0) == INVALID      # the width changes: its table is needed
    assert call(x0v=None) == INVALID and call(kv=None) == INVALID and call(tv=0) == INVALID      # and so does the height
    assert call(ws_bytes=3 * 61 * 84 * 3 - 1) == WORKSPACE and call(ws_ptr=None) == WORKSPACE
    assert call(H=56, W=45, x0v=None, kv=None, tv=0, ws_bytes=0) == WORKSPACE                    # one axis: only its table, still its workspace
