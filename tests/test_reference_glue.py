"""The host glue against the reference's OWN code, through its recorded outputs (tests/golden/reference_glue.json).

What the reference still holds of the CLIP-FlanT5 path (the model wrapper itself was dropped in v3.1) is
``constants.py``, ``score.py`` (``Score.forward`` / ``batch_forward``) and the helpers in
``models/vqascore_models/mm_utils.py`` (``expand2square``, ``t5_tokenizer_image_token``), and ``models/model.py``
(``image_loader``).  Those functions were run on exactly the inputs these tests build (same ids, same pixels, same
[M, N] / [n, n_vis, n_txt] tensors, same call log of the scoring model) and what they returned is the fixture; this
package's restatements must return the same.
"""
import hashlib
import json
import os
import types
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import t2v_metrics_amd.constants as our_constants
from t2v_metrics_amd.models.vqascore_models.mm_utils import expand2square, t5_tokenizer_image_token
from t2v_metrics_amd.score import Score as OurScore

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_glue.json")) as _f:
    REF = json.load(_f)


def _calls(calls):
    return [[list(i), list(t), dict(k)] for i, t, k in calls]


def _ref_tensor(rec):
    return torch.tensor(rec["values"], dtype=torch.float32).reshape(rec["shape"])


class WordTokenizer:
    """HF call protocol with the T5 convention (no BOS, trailing </s> = 1 on every call, also on the empty string)."""

    bos_token_id = None

    def __call__(self, text):
        return types.SimpleNamespace(input_ids=[3 + zlib.crc32(w.encode()) % 32000 for w in text.split()] + [1])


class PieceTokenizer(WordTokenizer):
    """Same protocol over a real sentencepiece unigram model (trained here on the prompts, T5's special ids)."""

    def __init__(self, tmp_path, corpus):
        spm = pytest.importorskip("sentencepiece")
        src = tmp_path / "corpus.txt"
        src.write_text("\n".join(corpus * 20))
        spm.SentencePieceTrainer.train(input=str(src), model_prefix=str(tmp_path / "sp"), vocab_size=96, model_type="unigram",
                                       pad_id=0, eos_id=1, unk_id=2, bos_id=-1, hard_vocab_limit=False, minloglevel=2)
        self.sp = spm.SentencePieceProcessor(model_file=str(tmp_path / "sp.model"))

    def __call__(self, text):
        return types.SimpleNamespace(input_ids=self.sp.encode(text) + [1])


PROMPTS = [
    our_constants.SYSTEM_MSG + ' USER: <image>\nDoes this figure show "a dog chasing a red ball"? Please answer yes or no. ASSISTANT: ',
    "<image>", "", "no image token at all", "<image><image>", "tail <image>", "<image> head", "a <image> b <image> c",
    "  spaces   around  <image>   kept by split  ", "<image>\n<image>\n", "<Image> is not the token", "x<image>y",
]


def test_constants_are_the_references():
    ref = REF["constants"]
    assert set(ref) == {"HF_CACHE_DIR", "CONTEXT_LEN", "SYSTEM_MSG", "IGNORE_INDEX", "IMAGE_TOKEN_INDEX", "DEFAULT_IMAGE_TOKEN"}
    for name, value in ref.items():
        assert getattr(our_constants, name) == value, name


def test_t5_tokenizer_image_token_is_the_references(tmp_path):
    ref = REF["t5_tokenizer_image_token"]
    assert ref["prompts"] == PROMPTS
    for kind, tok in (("word", WordTokenizer()), ("piece", PieceTokenizer(tmp_path, [p for p in PROMPTS if p.strip()]))):
        for prompt, want in zip(PROMPTS, ref[kind]["ids"]):
            assert t5_tokenizer_image_token(prompt, tok) == want, (kind, prompt)
            assert want.count(REF["constants"]["IMAGE_TOKEN_INDEX"]) == prompt.count("<image>")
            got = t5_tokenizer_image_token(prompt, tok, return_tensors="pt")
            assert got.dtype == torch.long and torch.equal(got, torch.tensor(want, dtype=torch.long))
        with pytest.raises(ValueError, match="Unsupported tensor type") as err:
            t5_tokenizer_image_token("x", tok, return_tensors="np")
        assert str(err.value) == ref[kind]["return_tensors_np_error"]          # the reference raised the same error
        other = t5_tokenizer_image_token("a <image> b", tok, image_token_index=-7)
        assert other == ref[kind]["image_token_index_-7"] and other.count(-7) == 1


@pytest.mark.parametrize("mode,fill", [("RGB", (124, 116, 104)), ("RGB", (0, 0, 0)), ("L", 77), ("RGBA", (1, 2, 3, 4))])
def test_expand2square_is_the_references(mode, fill):
    """The reference's output images are recorded as size, mode and sha256 of their pixel bytes."""
    ref = REF["expand2square"]["%s %s" % (mode, fill)]
    rng = np.random.default_rng(5)
    sizes = ((10, 4), (4, 10), (7, 7), (1, 9), (9, 1), (33, 32), (32, 33), (640, 427), (427, 640))
    assert [(r["w"], r["h"]) for r in ref] == list(sizes)
    for (w, h), theirs in zip(sizes, ref):
        bands = len(Image.new(mode, (1, 1)).getbands())
        px = rng.integers(0, 256, (h, w) if bands == 1 else (h, w, bands), dtype=np.uint8)
        im = Image.fromarray(px, mode)
        ours = expand2square(im, fill)
        assert ours.size == tuple(theirs["size"]) == (max(w, h),) * 2 and ours.mode == theirs["mode"] == mode
        a = np.ascontiguousarray(np.asarray(ours))
        assert list(a.shape) == theirs["shape"] and hashlib.sha256(a.tobytes()).hexdigest() == theirs["sha256"]
        if w == h:
            assert ours is im and theirs["same_object"]     # the square case hands the SAME object back, in both


class PairModel:
    """A score model both Score classes can drive: a deterministic function of the (image, text) strings; keeps the calls."""

    video_mode = "concat"
    allows_image = True

    def __init__(self):
        self.calls = []

    def forward(self, images, texts, **kwargs):
        assert len(images) == len(texts)
        self.calls.append((list(images), list(texts), dict(kwargs)))
        gain = kwargs.get("gain", 1.0)
        return torch.tensor([gain * (zlib.crc32((i + "|" + t).encode()) % 10007) / 10007.0 for i, t in zip(images, texts)])


def _scorer():
    class S(OurScore):
        def list_all_models(self):
            return ["pair-model"]

        def prepare_scoremodel(self, model, device, cache_dir, **kwargs):
            return PairModel()
    return S("pair-model", device="cpu")


def test_score_forward_grid_is_the_references():
    ours, ref = _scorer(), REF["score_forward_grid"]
    images = [f"img_{k}.png" for k in range(5)]
    texts = [f"caption number {k}" for k in range(3)]
    cases = ((images, texts), (images[0], texts), (images, texts[1]), (images[2], texts[2]), (images[:1] * 3, texts))
    assert len(cases) == len(ref["cases"])
    for (im, tx), theirs in zip(cases, ref["cases"]):
        a, b = ours(images=im, texts=tx), _ref_tensor(theirs)
        assert a.shape == b.shape and a.dtype == torch.float32 and torch.equal(a, b)
    a = ours(images=images, texts=texts, gain=0.5)                                 # kwargs reach the model
    assert torch.equal(a, _ref_tensor(ref["gain_0.5"])) and ours.model.calls[-1][2] == ref["calls"][-1][2] == {"gain": 0.5}
    # what the model is asked, call by call, is the reference's too (score.py:104-106: one call per image, the image repeated)
    assert _calls(ours.model.calls) == ref["calls"]


def test_score_forward_video_gate_is_the_references(capsys):
    ours, ref = _scorer(), REF["score_forward_video_gate"]
    ours.model.video_mode = "neither"
    assert ours(images=["clip.MP4"], texts=["x"]) is None and ref["neither_returns"] is None
    said = capsys.readouterr().out.strip().splitlines()
    assert said == ref["neither_printed"] and len(said) == 1 and "video_mode" in said[0]
    ours.model.video_mode = "direct"                         # video-native: the path reaches the model untouched
    assert torch.equal(ours(images=["clip.mp4", "b.mov"], texts=["x", "y"]), _ref_tensor(ref["direct"]))
    assert _calls(ours.model.calls) == ref["calls"] and ours.model.calls[0][0] == ["clip.mp4", "clip.mp4"]


@pytest.mark.parametrize("n_samples,n_vis,n_txt,batch_size", [(7, 2, 3, 4), (4, 1, 1, 16), (5, 3, 1, 1), (9, 1, 4, 3)])
def test_batch_forward_is_the_references(n_samples, n_vis, n_txt, batch_size):
    ours, theirs = _scorer(), REF["batch_forward"]["%d,%d,%d,%d" % (n_samples, n_vis, n_txt, batch_size)]
    dataset = [{"images": [f"s{k}_v{v}.png" for v in range(n_vis)], "texts": [f"s{k} text {t}" for t in range(n_txt)]}
               for k in range(n_samples)]
    a = ours.batch_forward(dataset, batch_size=batch_size, gain=2.0)
    b = _ref_tensor(theirs)
    assert a.shape == b.shape == (n_samples, n_vis, n_txt) and str(a.dtype) == theirs["dtype"] and torch.equal(a, b)
    # the same set of (image, text) pairs was asked of the model, each exactly once -- in fewer, larger calls
    flat = sorted([i, t] for im, tx, _ in ours.model.calls for i, t in zip(im, tx))
    assert flat == theirs["pairs"] and len(flat) == n_samples * n_vis * n_txt
    assert len(ours.model.calls) == -(-n_samples // batch_size) and theirs["n_calls"] == n_samples * n_vis * n_txt
    assert all(kw == {"gain": 2.0} for _, _, kw in ours.model.calls) and theirs["kwargs"] == ['{"gain": 2.0}']


def test_batch_forward_rejects_ragged_samples_like_the_reference():
    ours = _scorer()
    dataset = [{"images": ["a.png", "b.png"], "texts": ["x"]}, {"images": ["c.png"], "texts": ["y"]}]
    with pytest.raises(AssertionError, match="Expected 2 visuals"):
        ours.batch_forward(dataset, batch_size=1)
    assert REF["batch_forward_ragged"]["raises"]             # the reference trips in DataLoader collation or on its own assert


def test_image_loader_is_the_references(tmp_path):
    """models/model.py:10-14: a .npy file holds BGR pixels (cv2 layout) and is flipped to RGB, everything else goes through PIL."""
    from t2v_metrics_amd.models.model import image_loader
    ref = REF["image_loader"]
    rs = np.random.RandomState(8)
    px = rs.randint(0, 256, (9, 13, 3), dtype=np.uint8)
    np.save(tmp_path / "a.npy", px)
    Image.fromarray(px).save(tmp_path / "a.png")
    Image.fromarray(px[..., 0]).save(tmp_path / "grey.png")                      # mode L -> RGB
    Image.fromarray(np.dstack([px, px[..., :1]]), "RGBA").save(tmp_path / "alpha.png")
    Image.fromarray(px).save(tmp_path / "a.jpg", quality=90)
    for name in ("a.npy", "a.png", "grey.png", "alpha.png", "a.jpg"):
        ours, theirs = image_loader(str(tmp_path / name)), ref[name]
        assert ours.mode == theirs["mode"] == "RGB" and ours.size == tuple(theirs["size"])
        assert np.array_equal(np.asarray(ours), np.array(theirs["pixels"], dtype=np.uint8)), name
    assert np.array_equal(np.asarray(image_loader(str(tmp_path / "a.npy"))), px[..., ::-1])
