"""Image front end of the CLIP-FlanT5 and CLIPScore rows on the MI355X (include/vqs.h vqs_images_u8, engine.images_from_u8, the models'
device_preprocess switch).  Bitwise equality with the host path -- engine.normalize_u8 of _imgprep.clip_preprocess_u8 -- is the bar
throughout: Pillow's 8-bit resampler is integer arithmetic and the normalisation of a uint8 is a table, so no tolerance appears here.
Every test runs under its own time limit."""
import ctypes
import faulthandler

import numpy as np
import pytest
import torch
from PIL import Image

from tests.image_frontend_cases import REAL_CASES, SMALL_CASES, case_id, make_images

pytestmark = pytest.mark.gpu

STEP_TIMEOUT_S = 120


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_TIMEOUT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def host_pixels(arrays, S, pad):
    """the host path: pad / PIL resize / crop on the CPU, the float tail on the GPU"""
    from t2v_metrics_amd import engine
    from t2v_metrics_amd.preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD, clip_preprocess_u8
    u8 = np.stack([clip_preprocess_u8(Image.fromarray(a), S, pad) for a in arrays])
    return engine.normalize_u8(torch.from_numpy(u8).cuda(), OPENAI_CLIP_MEAN, OPENAI_CLIP_STD)


# ---------------------------------------------------------------- 1. the kernels, through the C ABI
@pytest.mark.parametrize("case", SMALL_CASES + REAL_CASES, ids=case_id)
def test_images_u8_equals_the_host_path_bitwise(case):
    from t2v_metrics_amd import engine
    S, (H, W), n, pad, kind = case
    arrays = make_images(kind, n, H, W)
    got = engine.images_from_u8(torch.from_numpy(arrays).cuda(), S, pad)
    torch.cuda.synchronize()
    want = host_pixels(arrays, S, pad)
    assert got.shape == (n, 3, S, S) and got.dtype == torch.bfloat16
    assert torch.equal(got.cpu(), want.cpu())


def test_a_source_that_is_not_16_byte_aligned_takes_the_bytewise_edges():
    """The horizontal pass stages rows with 16-byte loads from 16-byte aligned addresses; the chunks at the two ends of the source array
    that are not wholly inside it are read bytewise.  A source that starts 3 bytes into an allocation and ends at its last byte."""
    from t2v_metrics_amd import engine
    H, W, S = 61, 45, 56
    arrays = make_images("random", 2, H, W, seed=5)
    raw = torch.zeros(3 + arrays.size, dtype=torch.uint8, device="cuda")
    raw[3:] = torch.from_numpy(arrays).cuda().view(-1)
    src = raw[3:].view(2, H, W, 3)
    assert src.data_ptr() % 16 == 3 and src.is_contiguous()
    for pad in (True, False):
        assert torch.equal(engine.images_from_u8(src, S, pad).cpu(), host_pixels(arrays, S, pad).cpu())


@pytest.mark.parametrize("axis", ["horizontal", "vertical"])
def test_one_axis_geometries_through_the_c_abi(axis):
    """image_plan resamples both axes or neither, so the forms "horizontal pass + plain row crop" and "vertical pass straight from the canvas"
    are reached only by a hand-built geometry: a 61 x 100 source whose one axis is resampled (100 -> 70 columns, or 61 -> 70 rows) and
    cropped to S = 56 (vector stores) and S = 42 (scalar stores) while the other axis is only cropped.  Reference: Pillow's own resize."""
    from t2v_metrics_amd import engine
    from t2v_metrics_amd.preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
    from t2v_metrics_amd.qwen.media import normalize_lut, pillow_bicubic_tables
    lib = engine.load_library()
    H, W, n = 61, 100, 2
    arrays = make_images("noise", n, H, W, seed=3)
    lut, src = normalize_lut().cuda(), torch.from_numpy(arrays).cuda()
    for S in (56, 42):
        if axis == "horizontal":
            rh, rw, crop_y, crop_x = H, 70, 3, 7
            first, weights = pillow_bicubic_tables(W, rw)
            first, weights = first[crop_x: crop_x + S], weights[crop_x: crop_x + S]
            row0, rows = 2, S + 2                                       # a window wider than the kept rows is legal
        else:
            rh, rw, crop_y, crop_x = 70, W, 7, 21
            first, weights = pillow_bicubic_tables(H, rh)
            first, weights = first[crop_y: crop_y + S], weights[crop_y: crop_y + S]
            row0, rows = 0, 0
        d_first, d_weights = torch.from_numpy(first.copy()).cuda(), torch.from_numpy(weights.copy()).cuda()
        g = engine.VqsImageGeometry(n, H, W, H, W, 0, 0, 1, 2, 3, S, rh, rw, crop_y, crop_x, weights.shape[1] if axis == "vertical" else 0,
                                    weights.shape[1] if axis == "horizontal" else 0, row0, rows)
        out = torch.empty(n, 3, S, S, dtype=torch.bfloat16, device="cuda")
        ws = torch.empty(lib.vqs_images_workspace_bytes(n, rows, S), dtype=torch.uint8, device="cuda")
        tabs = (d_first.data_ptr(), d_weights.data_ptr(), None, None) if axis == "horizontal" else (None, None, d_first.data_ptr(), d_weights.data_ptr())
        rc = lib.vqs_images_u8(src.data_ptr(), ctypes.byref(g), *tabs, lut.data_ptr(), out.data_ptr(), ws.data_ptr(),
                               ws.numel(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0
        want = np.stack([np.asarray(Image.fromarray(a).resize((rw, rh), Image.BICUBIC))[crop_y: crop_y + S, crop_x: crop_x + S] for a in arrays])
        want = engine.normalize_u8(torch.from_numpy(np.ascontiguousarray(want)).cuda(), OPENAI_CLIP_MEAN, OPENAI_CLIP_STD)
        assert torch.equal(out.cpu(), want.cpu()), (axis, S)


def test_error_paths_return_their_codes_and_leave_the_output_untouched():
    from t2v_metrics_amd import engine
    from t2v_metrics_amd.imagefront import image_plan
    from t2v_metrics_amd.qwen.media import normalize_lut
    lib = engine.load_library()
    H, W, S = 61, 45, 56
    plan = image_plan(H, W, S, True)
    src = torch.from_numpy(make_images("random", 1, H, W)).cuda()
    up = lambda a: torch.from_numpy(a.copy()).cuda()          # noqa: E731
    fh, kh, fv, kv = up(plan.first_h), up(plan.weights_h), up(plan.first_v), up(plan.weights_v)
    lut = normalize_lut().cuda()
    out = torch.full((1, 3, S, S), 7.0, dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(lib.vqs_images_workspace_bytes(1, plan.rows, S), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(fh=fh, kh=kh, fv=fv, kv=kv, ws_ptr=ws.data_ptr(), ws_bytes=ws.numel(), **fields):
        g = engine.image_geometry(plan, 1)
        for k, v in fields.items():
            setattr(g, k, v)
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        return lib.vqs_images_u8(src.data_ptr(), ctypes.byref(g), ptr(fh), ptr(kh), ptr(fv), ptr(kv), lut.data_ptr(), out.data_ptr(), ws_ptr, ws_bytes,
                                 stream)

    INVALID, WORKSPACE = -1, -3
    assert call(n=0) == INVALID and call(S=0) == INVALID and call(Wc=0) == INVALID              # non-positive sizes
    assert call(ox=17) == INVALID and call(oy=1) == INVALID                                     # the source leaves the canvas
    assert call(crop_x=1) == INVALID and call(crop_y=-1) == INVALID                             # the crop window leaves the axis
    assert call(kh=None) == INVALID and call(fv=None) == INVALID and call(taps_v=0) == INVALID  # a table is missing where the length changes
    assert call(row0=1, rows=61) == INVALID
    assert call(ws_bytes=61 * 56 * 3 - 1) == WORKSPACE and call(ws_ptr=None) == WORKSPACE       # a short workspace
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0                                                                          # and the same call with nothing wrong
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), host_pixels(make_images("random", 1, H, W), S, True).cpu())


# ---------------------------------------------------------------- 2. end to end through the models
class CountingFrontEnd:
    """The engine with images_from_u8 wrapped: records each call's source shape and whether the source was on the device."""

    def __init__(self, eng):
        self._e, self.front_calls = eng, []

    def images_from_u8(self, src, size, pad):
        self.front_calls.append((tuple(src.shape), bool(src.is_cuda)))
        return self._e.images_from_u8(src, size, pad)

    def __getattr__(self, name):
        return getattr(self._e, name)


class WithoutFrontEnd:
    """The engine as one that lacks images_from_u8."""

    def __init__(self, eng):
        self._e = eng

    def __getattr__(self, name):
        if name == "images_from_u8":
            raise AttributeError(name)
        return getattr(self._e, name)


def _sources(tmp_path):
    """three source sizes, one of them twice, as arrays and as PNG files"""
    rng = np.random.RandomState(11)
    arrays = [rng.randint(0, 256, hw + (3,), dtype=np.uint8) for hw in [(61, 45), (100, 56), (61, 45), (56, 56), (80, 120)]]
    paths = []
    for i, a in enumerate(arrays):
        paths.append(str(tmp_path / f"s{i}.png"))
        Image.fromarray(a).save(paths[-1])
    return arrays, paths


TEXTS = ["a red cube", "two dogs playing in the snow", "nothing", "a photo of an astronaut riding a horse", "a dog"]


def _check_model(m, arrays, paths, grid_texts):
    """forward and forward_grid bitwise equal across device_preprocess on / off / the same images as PNG paths; one front-end call per
    source size; a device-resident tensor entry arrives there still on the device; an engine without the method falls back."""
    held = [arrays[0], Image.fromarray(arrays[1]), torch.from_numpy(arrays[2].copy()).cuda(), torch.from_numpy(arrays[3].copy()), paths[4]]
    want, want_grid = m.forward(paths, TEXTS), m.forward_grid(paths, grid_texts)
    assert torch.isfinite(want).all() and len(set(want.tolist())) > 1
    m.device_preprocess = False
    assert torch.equal(m.forward(held, TEXTS), want) and torch.equal(m.forward_grid(held, grid_texts), want_grid)
    real = m.engine
    m.engine = counting = CountingFrontEnd(real)
    assert torch.equal(m.forward(held, TEXTS), want) and not counting.front_calls               # the switch is off: the host path
    m.device_preprocess = True
    from t2v_metrics_amd import imagefront
    to_host, real_entry_array = [], imagefront.entry_array
    imagefront.entry_array = lambda p: (to_host.append(isinstance(p, torch.Tensor) and p.is_cuda), real_entry_array(p))[1]
    try:
        assert torch.equal(m.forward(held, TEXTS), want)
    finally:
        imagefront.entry_array = real_entry_array
    assert len(to_host) == 3 and not any(to_host)              # the three host entries were staged; the device tensor never came to the host
    # (61, 45) twice -- one host array, one device tensor -- is ONE call; (100, 56) and (56, 56) one each; the path stays on the host
    assert sorted(c[0] for c in counting.front_calls) == [(1, 56, 56, 3), (1, 100, 56, 3), (2, 61, 45, 3)]
    assert all(on_device for _, on_device in counting.front_calls)
    counting.front_calls.clear()
    assert torch.equal(m.forward_grid(held, grid_texts), want_grid) and len(counting.front_calls) == 3
    counting.front_calls.clear()
    on_dev = [torch.from_numpy(a.copy()).cuda() for a in arrays[:3]]                             # nothing but device tensors: stacked there
    assert torch.equal(m.forward(on_dev, TEXTS[:3]), want[:3]) and sorted(c[0][0] for c in counting.front_calls) == [1, 2]
    m.engine = WithoutFrontEnd(real)
    assert torch.equal(m.forward(held, TEXTS), want)
    m.engine = real


def test_clip_flant5_scores_are_bitwise_equal_across_the_three_front_ends(tmp_path):
    import t2v_metrics_amd as t2v
    from t2v_metrics_amd.config import get_config
    from tests.test_host_api import FakeTokenizer
    cfg = get_config("tiny")
    arrays, paths = _sources(tmp_path)
    s = t2v.VQAScore(model="clip-flant5-xl", device="cuda:0", cache_dir=str(tmp_path / "c"), config=cfg, weights="seeded",
                     tokenizer=FakeTokenizer(cfg.t5.vocab), image_workers="thread", device_preprocess=True)
    assert s.model.device_preprocess is True
    _check_model(s.model, arrays, paths, TEXTS[:2])
    # more images than max_images: the chunk pipeline loads chunk i + 1 on the image thread
    s.model.max_images = 2
    want = s.model.forward(paths, TEXTS)
    assert torch.equal(s.model.forward([arrays[0], arrays[1], paths[2], arrays[3], arrays[4]], TEXTS), want)
    assert torch.equal(s(images=arrays, texts=TEXTS[:2]).cpu(), s(images=paths, texts=TEXTS[:2]).cpu())


def test_clipscore_cosines_are_bitwise_equal_across_the_three_front_ends(tmp_path):
    import t2v_metrics_amd as t2v
    from t2v_metrics_amd.clip.config import get_clip_config
    from tests.clip_truth import ClipTokenizerDouble
    cfg = get_clip_config("clip-tiny")
    arrays, paths = _sources(tmp_path)
    s = t2v.CLIPScore(model="openai:ViT-L-14-336", device="cuda:0", config=cfg, weights="seeded", tokenizer=ClipTokenizerDouble(cfg),
                      device_preprocess=True)
    assert s.model.device_preprocess is True
    _check_model(s.model, arrays, paths, TEXTS[:2])
    assert torch.equal(s(images=arrays, texts=TEXTS[:2]).cpu(), s(images=paths, texts=TEXTS[:2]).cpu())
