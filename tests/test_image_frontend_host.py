"""In-memory image entries of the CLIP-FlanT5 and CLIPScore rows and the host side of their device front end, on the CPU: the folded
plan (imagefront.image_plan) restated in numpy against the installed Pillow, the drop-in API on recording engine doubles, and the argument
checks vqs_images_u8 answers before any launch."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

import t2v_metrics_amd as t2v
from t2v_metrics_amd.imagefront import image_plan
from t2v_metrics_amd.preprocess import OPENAI_CLIP_MEAN, clip_preprocess, clip_preprocess_u8
from tests.image_frontend_cases import REAL_CASES, SMALL_CASES, case_id, folded_reference, make_images
from tests.test_host_api import FakeTokenizer, RecordingEngine


# ---------------------------------------------------------------- 1. the folded plan
@pytest.mark.parametrize("case", SMALL_CASES + REAL_CASES, ids=case_id)
def test_folded_plan_equals_the_host_path(case):
    S, (H, W), n, pad, kind = case
    plan = image_plan(H, W, S, pad)
    for a in make_images(kind, n, H, W):
        assert np.array_equal(folded_reference(a, plan), clip_preprocess_u8(Image.fromarray(a), S, pad))


def test_plan_geometry():
    p = image_plan(61, 45, 56, True)               # expand2square: odd offsets, floor on the leading side
    assert (p.Hc, p.Wc, p.oy, p.ox) == (61, 61, 0, 8) and p.color == tuple(int(m * 255) for m in OPENAI_CLIP_MEAN)
    assert (p.resized_h, p.resized_w, p.crop_y, p.crop_x) == (56, 56, 0, 0) and p.first_h.shape == (56,) and p.weights_v.shape[0] == 56
    p = image_plan(56, 100, 56, False)             # short == S: neither axis is resampled, crop only
    assert p.weights_h is None and p.weights_v is None and (p.crop_y, p.crop_x, p.row0, p.rows) == (0, 22, 0, 56)
    p = image_plan(20, 300, 56, False)             # int(S * long / short)
    assert (p.resized_h, p.resized_w, p.crop_x) == (56, 840, 392) and p.rows == 20
    p = image_plan(768, 1024, 336, True)           # the rows kept are the canvas rows the vertical taps reach, inside the canvas
    assert p.row0 == 0 and p.rows == 1024 and p.weights_h.shape[1] >= 13
    p = image_plan(300, 20, 56, False)             # the crop keeps rows from the middle only: the horizontal pass skips the rest
    assert p.row0 > 0 and p.row0 + p.rows < 300


def test_normalize_lut_equals_the_float_expression_of_clip_preprocess():
    from t2v_metrics_amd.qwen.media import normalize_lut
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    img = np.stack([v, v[::-1], v.T], axis=-1)                                        # every value in every channel
    want = torch.from_numpy(clip_preprocess(Image.fromarray(img), 16, False)).to(torch.bfloat16)      # 16 x 16 at size 16: no resize
    lut = normalize_lut()
    for c in range(3):
        assert torch.equal(lut[c][torch.from_numpy(img[..., c].astype(np.int64))], want[c])


# ---------------------------------------------------------------- 2. drop-in API on engine doubles
class PixelRecorder(RecordingEngine):
    def __init__(self, cfg):
        super().__init__(cfg)
        self.pixels = []

    def encode_images(self, pixels):
        self.pixels.append(pixels.clone())
        return super().encode_images(pixels)

    def generate(self, feats, img_index, input_ids, max_new_tokens):
        return torch.ones(input_ids.shape[0], max_new_tokens, dtype=torch.int32)


def t5_scorer(tmp_path, **kw):
    from t2v_metrics_amd.config import get_config
    cfg = get_config("tiny")
    eng = PixelRecorder(cfg)
    s = t2v.VQAScore(model="clip-flant5-xl", device="cpu", cache_dir=str(tmp_path / "cache"), config=cfg, engine=eng,
                     tokenizer=FakeTokenizer(cfg.t5.vocab), **kw)
    return s, eng


class ClipPixelRecorder:
    def __init__(self, cfg):
        from tests.test_clipscore_host import RecordingClipEngine
        self._e = RecordingClipEngine(cfg)
        self.calls, self.pixels = self._e.calls, []

    def encode_images(self, px):
        self.pixels.append(px.clone())
        return self._e.encode_images(px)

    def __getattr__(self, name):
        return getattr(self._e, name)


def clip_scorer(**kw):
    from t2v_metrics_amd.clip.config import get_clip_config
    from tests.clip_truth import ClipTokenizerDouble
    cfg = get_clip_config("clip-tiny")
    eng = ClipPixelRecorder(cfg)
    s = t2v.CLIPScore(model="openai:ViT-L-14-336", device="cpu", config=cfg, engine=eng, tokenizer=ClipTokenizerDouble(cfg), **kw)
    return s, eng


@pytest.fixture()
def arrays_and_files(tmp_path):
    rng = np.random.RandomState(7)
    arrays = [rng.randint(0, 256, hw + (3,), dtype=np.uint8) for hw in [(60, 60), (40, 70), (80, 50), (61, 45), (56, 100)]]
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / f"a{i}.png"))
        Image.fromarray(a).save(paths[-1])
    return arrays, paths


TEXTS = ["a cat", "a dog on a mat", "x", "two words", "a red cube"]


def as_kind(a, kind):
    return {"ndarray": lambda: a, "pil": lambda: Image.fromarray(a), "pil-rgba": lambda: Image.fromarray(a).convert("RGBA"),
            "tensor": lambda: torch.from_numpy(a.copy())}[kind]()


@pytest.mark.parametrize("kind", ["ndarray", "pil", "pil-rgba", "tensor"])
@pytest.mark.parametrize("which", ["clip-flant5", "clipscore"])
def test_in_memory_entries_hand_the_engine_the_pixels_of_the_png(tmp_path, arrays_and_files, kind, which):
    arrays, paths = arrays_and_files
    make = (lambda: t5_scorer(tmp_path)) if which == "clip-flant5" else clip_scorer
    s_mem, e_mem = make()
    s_png, e_png = make()
    held = [as_kind(a, kind) for a in arrays]
    got, want = s_mem.model.forward(held, TEXTS), s_png.model.forward(paths, TEXTS)
    assert torch.equal(got, want)
    assert len(e_mem.pixels) == 1 and e_mem.pixels[0].shape[0] == 5 and torch.equal(e_mem.pixels[0], e_png.pixels[0])
    assert torch.equal(s_mem(images=held, texts=TEXTS), s_png(images=paths, texts=TEXTS))          # the M x N call of the Score class
    ds = [{"images": held[:2], "texts": TEXTS[:2]}, {"images": held[2:4], "texts": TEXTS[2:4]}]
    ds_png = [{"images": paths[:2], "texts": TEXTS[:2]}, {"images": paths[2:4], "texts": TEXTS[2:4]}]
    assert torch.equal(s_mem.batch_forward(ds, batch_size=2), s_png.batch_forward(ds_png, batch_size=2))


@pytest.mark.parametrize("which", ["clip-flant5", "clipscore"])
def test_mixed_lists_keep_their_order_and_identity_dedupes(tmp_path, arrays_and_files, which):
    arrays, paths = arrays_and_files
    make = (lambda **kw: t5_scorer(tmp_path, **kw)) if which == "clip-flant5" else clip_scorer
    s, e = make()
    s_png, e_png = make()
    mixed = [paths[0], arrays[1], Image.fromarray(arrays[2]), torch.from_numpy(arrays[3].copy()), paths[4]]
    assert torch.equal(s.model.forward(mixed, TEXTS), s_png.model.forward(paths, TEXTS))
    assert torch.equal(e.pixels[0], e_png.pixels[0])
    # the same object twice is one encode; an equal-content copy is a second image; a repeated path is one
    e.pixels.clear()
    twice = s.model.forward([arrays[1], arrays[1], arrays[1].copy(), paths[0], paths[0]], TEXTS)
    assert e.pixels[0].shape[0] == 3 and torch.equal(e.pixels[0][0], e.pixels[0][1])
    assert twice.shape == (5,)
    # forward_grid: M images are encoded for M x N pairs
    e.pixels.clear()
    grid = s.model.forward_grid([arrays[0], arrays[3], arrays[0]], TEXTS[:4])
    assert grid.shape == (3, 4) and sum(p.shape[0] for p in e.pixels) == 2 and torch.equal(grid[0], grid[2])
    assert torch.equal(grid, s_png.model.forward_grid([paths[0], paths[3], paths[0]], TEXTS[:4]))
    # the switch on an engine without images_from_u8 (and with no GPU): the host path, same result
    s_on, e_on = make(device_preprocess=True)
    assert s_on.model.device_preprocess is True and not hasattr(e_on, "images_from_u8")
    assert torch.equal(s_on.model.forward(mixed, TEXTS), s_png.model.forward(paths, TEXTS))


def test_generate_ids_and_score_pairs_take_in_memory_entries(tmp_path, arrays_and_files):
    arrays, paths = arrays_and_files
    s, e = t5_scorer(tmp_path)
    assert s.model.generate_ids([arrays[0], arrays[0], arrays[1]], ["q one", "q two", "q three"], max_new_tokens=3) == [[1]] * 3
    assert e.pixels[0].shape[0] == 2
    sc = s.model.score_pairs([arrays[0], arrays[1]], [0, 1, 1], ["q one", "q two", "q three"], ["Yes"] * 3)
    assert torch.equal(sc, s.model.score_pairs(paths[:2], [0, 1, 1], ["q one", "q two", "q three"], ["Yes"] * 3))
    with pytest.raises(TypeError, match="float32"):
        s.model.score_pairs([arrays[0].astype(np.float32)], [0], ["q"], ["Yes"])


@pytest.mark.parametrize("image_workers", ["process", "thread"])
def test_more_images_than_max_images_run_the_chunk_pipeline(tmp_path, arrays_and_files, image_workers):
    arrays, paths = arrays_and_files
    s, e = t5_scorer(tmp_path, max_images=3, max_pairs=2, image_workers=image_workers, num_workers=3)
    s_png, e_png = t5_scorer(tmp_path, max_images=3, max_pairs=2, image_workers="thread", num_workers=3)
    mixed = [arrays[0], paths[1], paths[2], arrays[3], Image.fromarray(arrays[4])]
    assert torch.equal(s.model.forward(mixed, TEXTS), s_png.model.forward(paths, TEXTS))
    assert [p.shape[0] for p in e.pixels] == [3, 2]
    assert all(torch.equal(a, b) for a, b in zip(e.pixels, e_png.pixels))


BAD = [(np.zeros((8, 8, 3), dtype=np.float32), TypeError, r"float32.*\(8, 8, 3\)"),
       (torch.zeros(8, 8, 3), TypeError, r"torch\.float32.*\(8, 8, 3\)"),
       (np.zeros((8, 8, 4), dtype=np.uint8), ValueError, r"uint8.*\(8, 8, 4\)"),
       (np.zeros((3, 8, 8), dtype=np.uint8), ValueError, r"\(3, 8, 8\)"),
       (np.zeros((8, 8), dtype=np.uint8), ValueError, r"\(8, 8\)"),
       (np.zeros((0, 8, 3), dtype=np.uint8), ValueError, r"\(0, 8, 3\)"),
       (torch.zeros(8, 0, 3, dtype=torch.uint8), ValueError, r"\(8, 0, 3\)"),
       (12345, TypeError, "int")]


@pytest.mark.parametrize("bad,exc,match", BAD, ids=[str(i) for i in range(len(BAD))])
def test_illegal_entries_raise_before_the_engine_is_touched(tmp_path, arrays_and_files, bad, exc, match):
    arrays, _ = arrays_and_files
    s, e = t5_scorer(tmp_path)
    c, ce = clip_scorer()
    for call in (lambda: s.model.forward([arrays[0], bad], ["a", "b"]), lambda: s.model.forward_grid([arrays[0], bad], ["a"]),
                 lambda: s.model.generate_ids([bad], ["a"]), lambda: s(images=[arrays[0], bad], texts=["a"]),
                 lambda: c.model.forward([arrays[0], bad], ["a", "b"]), lambda: c.model.forward_grid([bad], ["a"]),
                 lambda: c(images=[bad, arrays[0]], texts=["a"])):
        with pytest.raises(exc, match=match):
            call()
    assert not e.pixels and not e.score_calls and not ce.calls


# ---------------------------------------------------------------- 3. the C call's argument checks
def test_images_u8_argument_checks_answer_before_any_launch():
    """No device here: every call below must return from the checks (a launch would fail with VQS_ERR_HIP = -4)."""
    from t2v_metrics_amd import engine
    lib = engine.load_library()
    INVALID, WORKSPACE = -1, -3
    ws = lib.vqs_images_workspace_bytes
    assert ws(2, 61, 56) >= 2 * 61 * 56 * 3 and ws(2, 61, 56) % 256 == 0 and ws(1, 0, 56) == 256
    assert ws(0, 61, 56) == 0 and ws(1, -1, 56) == 0 and ws(1, 61, 0) == 0
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)          # never dereferenced: the checks come first
    plan = image_plan(61, 45, 56, True)               # both axes resampled, canvas 61 x 61, offsets (0, 8)

    def call(src=p, lut=p, out=p, fh=p, kh=p, fv=p, kv=p, ws_ptr=p, ws_bytes=1 << 30, geo=True, **fields):
        g = engine.image_geometry(plan, 1)
        for k, v in fields.items():
            assert hasattr(g, k)
            setattr(g, k, v)
        return lib.vqs_images_u8(src, ctypes.byref(g) if geo else None, fh, kh, fv, kv, lut, out, ws_ptr, ws_bytes, None)

    assert call(src=None) == INVALID and call(lut=None) == INVALID and call(out=None) == INVALID and call(geo=False) == INVALID
    for name in ("n", "H", "W", "Hc", "Wc", "S", "resized_h", "resized_w"):                       # non-positive sizes
        assert call(**{name: 0}) == INVALID and call(**{name: -3}) == INVALID, name
    assert call(color_r=256) == INVALID and call(color_b=-1) == INVALID
    # the source rectangle must lie inside the canvas
    assert call(ox=17) == INVALID and call(ox=-1) == INVALID and call(oy=1) == INVALID and call(oy=-1) == INVALID
    assert call(Wc=44, ox=0) == INVALID and call(Hc=60) == INVALID and call(ox=2 ** 31 - 1) == INVALID
    # the crop window must lie inside the resized axis
    assert call(crop_x=1) == INVALID and call(crop_y=-1) == INVALID and call(S=57) == INVALID and call(crop_y=2 ** 31 - 1) == INVALID
    # a table is needed where the length changes
    assert call(fh=None) == INVALID and call(kh=None) == INVALID and call(taps_h=0) == INVALID
    assert call(fv=None) == INVALID and call(kv=None) == INVALID and call(taps_v=0) == INVALID
    # the rows the horizontal pass keeps: inside the canvas; and they cover the kept rows where the height is not resampled
    assert call(row0=-1) == INVALID and call(rows=0) == INVALID and call(row0=1, rows=61) == INVALID
    assert call(Hc=61, resized_h=61, S=56, crop_y=3, row0=4, rows=56, fv=None, kv=None) == INVALID
    assert call(Hc=61, resized_h=61, S=56, crop_y=3, row0=3, rows=55, fv=None, kv=None) == INVALID
    assert call(n=65536) == INVALID and call(H=1, W=20000, Hc=1, Wc=20000, ox=0, resized_h=1, S=1, row0=0, rows=1) == INVALID
    # the workspace of the horizontal pass
    need = 61 * 56 * 3
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_ptr=None) == WORKSPACE and call(n=2, ws_bytes=2 * need - 1) == WORKSPACE
