"""CPU-side checks of the CLIPScore row: the C ABI surface (include/vqs_clip.h == exports == the binding's signature table),
the host glue of ``CLIPScore`` against a recording engine double, the HF fixture and its plain-torch restatement, and the
preprocessing call (``pad_to_square=False``) against HF ``CLIPImageProcessor``."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "clipscore_tiny.npz")


# ---------------------------------------------------------------- 1. C ABI
def _declared(header):
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(vqs_[a-z_0-9]+)\s*\(", src)))


def test_header_exports_and_binding_agree():
    from t2v_metrics_amd.clip import engine as ce
    lib = ce.clip_library()
    declared = _declared("vqs_clip.h")
    assert len(declared) >= 14 and all(n.startswith("vqs_clip_") for n in declared)
    assert set(declared) == set(ce._SIGS), "clip/engine.py signatures out of sync with include/vqs_clip.h"
    so = os.path.join(ROOT, "t2v_metrics_amd", "libvqs_hip.so")
    exported = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", so], text=True).splitlines() if " T " in l}
    assert {n for n in exported if n.startswith("vqs_clip_")} == set(declared)
    for n in declared:
        assert hasattr(lib, n)
    # the boundary of include/vqs.h is untouched: none of the new names leaked into it
    assert not [n for n in _declared("vqs.h") if n.startswith("vqs_clip_")]


def _create(cfg):
    from t2v_metrics_amd.clip import engine as ce
    lib = ce.clip_library()
    h = ctypes.c_void_p()
    c = ce.make_clip_config(cfg) if not isinstance(cfg, ce.VqsClipConfig) else cfg
    return lib, h, lib.vqs_clip_create(ctypes.byref(c), ctypes.byref(h))


def test_create_and_size_queries_need_no_gpu():
    from t2v_metrics_amd.clip.config import get_clip_config
    cfg = get_clip_config("openai:ViT-L-14-336")
    lib, h, rc = _create(cfg)
    assert rc == 0
    # packed: q|k|v + their fp16 copies and the fp16 out / fc1 / fc2 copies of both towers
    per_vis = 2 * (2 * 3 * 1024 * 1024 + 1024 * 1024 + 2 * 4096 * 1024)
    per_txt = 2 * (2 * 3 * 768 * 768 + 768 * 768 + 2 * 3072 * 768)
    assert lib.vqs_clip_packed_bytes(h) >= 24 * per_vis + 12 * per_txt
    assert lib.vqs_clip_image_workspace_bytes(h, 8) > 8 * 577 * 1024 * 4
    assert lib.vqs_clip_image_workspace_bytes(h, 0) == 0
    assert lib.vqs_clip_text_workspace_bytes(h, 16, 77) > 16 * 77 * 768 * 4
    assert lib.vqs_clip_text_workspace_bytes(h, 16, 78) == 0 and lib.vqs_clip_text_workspace_bytes(h, 16, 7) == 0
    v = ctypes.c_int32(-1)
    assert lib.vqs_clip_get_option(h, b"fp16", ctypes.byref(v)) == 0 and v.value == 1
    assert lib.vqs_clip_set_option(h, b"fp16", 0) == 0 and lib.vqs_clip_get_option(h, b"fp16", ctypes.byref(v)) == 0 and v.value == 0
    assert lib.vqs_clip_set_option(h, b"fp16", 2) != 0 and lib.vqs_clip_set_option(h, b"vit_fp16", 1) != 0
    # unbound handle: the passes refuse before touching anything
    assert lib.vqs_clip_encode_images(h, 1, 1, 1, 1, 1 << 40, None) != 0 and b"not bound" in lib.vqs_clip_last_error(h)
    lib.vqs_clip_destroy(h)
    lib224, h224, rc = _create(get_clip_config("openai:ViT-L-14"))
    assert rc == 0 and lib224.vqs_clip_image_workspace_bytes(h224, 8) > 8 * 257 * 1024 * 4
    lib224.vqs_clip_destroy(h224)


@pytest.mark.parametrize("field,value,word", [("txt_heads", 16, b"text head dim"), ("vis_heads", 8, b"vision head dim"), ("txt_context", 129, b"txt_context"),
                                              ("vis_image", 330, b"multiple of the patch"), ("embed_dim", 770, b"embed_dim"), ("txt_layers", 0, b"layer counts"),
                                              ("txt_context", 4, b"txt_context")])
def test_bad_configs_are_refused(field, value, word):
    from t2v_metrics_amd.clip import engine as ce
    from t2v_metrics_amd.clip.config import get_clip_config
    c = ce.make_clip_config(get_clip_config("openai:ViT-L-14-336"))
    setattr(c, field, value)
    lib, h, rc = _create(c)
    assert rc != 0 and word in lib.vqs_clip_last_error(h)
    assert lib.vqs_clip_packed_bytes(h) == 0 and lib.vqs_clip_image_workspace_bytes(h, 1) == 0
    lib.vqs_clip_destroy(h)


def test_engine_refuses_cpu_device_and_unsafe_fp16_weights():
    from t2v_metrics_amd.clip import engine as ce
    from t2v_metrics_amd.clip.config import get_clip_config
    from t2v_metrics_amd.engine import VqsError
    with pytest.raises(VqsError, match="no CPU path"):
        ce.ClipEngine(get_clip_config("clip-tiny"), {}, device="cpu")
    w = {"text_model.encoder.layers.0.mlp.fc1.weight": torch.full((4, 4), 7.0e4), "text_projection.weight": torch.full((4, 4), 7.0e4),
         "vision_model.encoder.layers.1.self_attn.q_proj.weight": torch.ones(4, 4)}
    assert ce.clip_fp16_unsafe_weights(w) == ["text_model.encoder.layers.0.mlp.fc1.weight"]


# ---------------------------------------------------------------- 2. host glue
class RecordingClipEngine:
    """Engine double: embeddings are a deterministic function of the input rows, every call is recorded."""

    def __init__(self, cfg):
        self.cfg, self.calls = cfg, []

    def encode_images(self, px):
        self.calls.append(("encode_images", tuple(px.shape)))
        e = px.float().reshape(px.shape[0], -1)[:, :8]
        return torch.nn.functional.normalize(e + 1.0, dim=-1)

    def encode_texts(self, ids, eot_pos):
        self.calls.append(("encode_texts", ids.clone(), eot_pos.clone()))
        e = torch.stack([(ids[:, : 4].float().sum(1) * (k + 1)).sin() for k in range(8)], 1)
        return torch.nn.functional.normalize(e + 0.1, dim=-1)

    def similarity(self, a, b):
        self.calls.append(("similarity", a.shape[0], b.shape[0]))
        return a @ b.t()

    def similarity_pairs(self, a, b, ii, tt):
        self.calls.append(("similarity_pairs", len(ii)))
        return (a[torch.tensor(ii)] * b[torch.tensor(tt)]).sum(-1)


@pytest.fixture()
def scorer_and_files(tmp_path):
    from PIL import Image
    import t2v_metrics_amd as t2v
    from t2v_metrics_amd.clip.config import get_clip_config
    from tests.clip_truth import ClipTokenizerDouble
    cfg = get_clip_config("clip-tiny")
    rng = np.random.RandomState(1)
    paths = []
    for i in range(3):
        p = str(tmp_path / f"i{i}.png")
        Image.fromarray(rng.randint(0, 256, (60 + 9 * i, 80, 3), dtype=np.uint8)).save(p)
        paths.append(p)
    eng = RecordingClipEngine(cfg)
    s = t2v.CLIPScore(model="openai:ViT-L-14-336", device="cpu", config=cfg, engine=eng, tokenizer=ClipTokenizerDouble(cfg), num_workers=1)
    return s, eng, paths


def test_forward_encodes_each_image_and_text_once(scorer_and_files):
    s, eng, paths = scorer_and_files
    texts = ["a cat", "a dog on a mat", "x", "two words"]
    out = s(images=paths, texts=texts)
    assert out.shape == (3, 4) and out.dtype == torch.float32
    kinds = [c[0] for c in eng.calls]
    assert kinds == ["encode_images", "encode_texts", "similarity"]
    assert eng.calls[0][1] == (3, 3, 56, 56) and eng.calls[1][1].shape[0] == 4 and eng.calls[2][1:] == (3, 4)
    # duplicates are encoded once and expanded on the host
    eng.calls.clear()
    out2 = s(images=[paths[0], paths[1], paths[0]], texts=["a cat", "a cat", "x"])
    assert eng.calls[0][1][0] == 2 and eng.calls[1][1].shape[0] == 2 and eng.calls[2][1:] == (2, 2)
    assert torch.equal(out2[0], out2[2]) and torch.equal(out2[:, 0], out2[:, 1])
    assert torch.allclose(out2[0, 0], out[0, 0]) and torch.allclose(out2[1, 2], out[1, 2])
    # pair form and batch_forward: de-duplicated encodes per call / batch
    eng.calls.clear()
    pairs = s.model.forward([paths[0]] * 4, texts)
    assert [c[0] for c in eng.calls] == ["encode_images", "encode_texts", "similarity_pairs"] and eng.calls[0][1][0] == 1
    assert torch.allclose(pairs, out[0])
    eng.calls.clear()
    bf = s.batch_forward([{"images": paths[:2], "texts": texts[:2]}, {"images": paths[1:], "texts": texts[2:]}], batch_size=2)
    assert bf.shape == (2, 2, 2) and torch.allclose(bf[0], out[:2, :2]) and torch.allclose(bf[1], out[1:, 2:])
    assert eng.calls[0][1][0] == 3 and eng.calls[1][1].shape[0] == 4           # 8 pairs -> 3 distinct images, 4 distinct texts


def test_tokenize_eot_index_and_truncation(scorer_and_files):
    s, _, _ = scorer_and_files
    m, t = s.model, s.model.cfg.text
    ids, pos = m.tokenize(["one two three", "w " * 40, "solo"])
    assert ids.shape == (3, t.context) and ids.dtype == torch.int32
    assert pos.tolist() == [4, t.context - 1, 2]
    assert int(ids[1, -1]) == t.eot_id and int(ids[1, 0]) == t.bos_id and t.eot_id not in ids[1, :-1].tolist()   # truncation keeps the EOT last
    assert ids[0, 5:].tolist() == [t.eot_id] * (t.context - 5)                   # right padding
    from t2v_metrics_amd.clip.engine import eot_positions
    assert eot_positions(ids, t.eot_id).tolist() == pos.tolist()
    with pytest.raises(ValueError):
        eot_positions(torch.zeros(1, 5, dtype=torch.int32), t.eot_id)
    from t2v_metrics_amd.clip.config import get_clip_config
    assert get_clip_config("openai:ViT-L-14-336").text.context == 77 and get_clip_config("openai:ViT-L-14").vision.image == 224


def test_public_names():
    import t2v_metrics_amd as t2v
    from tests.test_clipscore_host import RecordingClipEngine as R          # noqa: F401
    from t2v_metrics_amd.clip.config import get_clip_config
    from tests.clip_truth import ClipTokenizerDouble
    assert t2v.list_all_clipscore_models() == ["openai:ViT-L-14-336", "openai:ViT-L-14"]
    assert t2v.list_all_models() == ["clip-flant5-xxl", "clip-flant5-xl", "qwen2.5-vl-7b"]            # unchanged by this row
    cfg = get_clip_config("openai:ViT-L-14-336")
    s = t2v.get_score_model("openai:ViT-L-14-336", device="cpu", engine=R(cfg), tokenizer=ClipTokenizerDouble(cfg))
    assert isinstance(s, t2v.CLIPScore) and s.model.video_mode == "concat" and s.model.context_len == 77
    with pytest.raises(NotImplementedError):
        t2v.get_score_model("openai:ViT-B-32")


def test_checkpoint_directory_loading(tmp_path):
    from safetensors.torch import save_file
    from t2v_metrics_amd.clip.config import get_clip_config
    from t2v_metrics_amd.clip.weights import clip_weight_specs, load_clip_checkpoint, make_seeded_clip_weights
    cfg = get_clip_config("clip-tiny")
    w = make_seeded_clip_weights(cfg, seed=3)
    sd = {k: v.float() for k, v in w.items()}
    sd["logit_scale"] = torch.tensor(4.6)
    save_file(sd, str(tmp_path / "model.safetensors"))
    got = load_clip_checkpoint(cfg, str(tmp_path), "cpu")
    assert set(got) == {n for n, _, _ in clip_weight_specs(cfg)} and all(torch.equal(got[k], w[k]) for k in w)
    del sd["text_projection.weight"]
    save_file(sd, str(tmp_path / "model.safetensors"))
    with pytest.raises(KeyError, match="text_projection"):
        load_clip_checkpoint(cfg, str(tmp_path), "cpu")


# ---------------------------------------------------------------- 3. fixture
def test_fixture_is_reproduced_by_the_restatement_and_by_hf():
    """tests/golden/clipscore_tiny.npz (written by tests/golden/make_clipscore_tiny.py from HF CLIPModel in fp32): the plain-torch fp32
    restatement the GPU tests take their pieces from reproduces it, and so does HF today.  fp32 on both sides, different summation
    orders: 1e-5 on entries of unit vectors.  The bf16 run recorded with it keeps the ranking check's coverage above one half."""
    from t2v_metrics_amd.clip.config import get_clip_config
    from tests import clip_truth as ct
    z = np.load(GOLDEN)
    cfg = get_clip_config("clip-tiny")
    W = ct.seeded_weights(cfg, int(z["seed"]))
    px = torch.from_numpy(z["pixels"]).to(torch.bfloat16)
    ids, pos = torch.from_numpy(z["ids"]), torch.from_numpy(z["eot_pos"])
    img, txt = ct.restated_embeddings(cfg, W, px, ids, pos)
    assert float((img - torch.from_numpy(z["image_embeds"])).abs().max()) <= 1e-5
    assert float((txt - torch.from_numpy(z["text_embeds"])).abs().max()) <= 1e-5
    assert float((img @ txt.t() - torch.from_numpy(z["grid"])).abs().max()) <= 1e-5
    himg, htxt, hgrid = ct.hf_grid(cfg, W, px, ids)
    assert float((hgrid - torch.from_numpy(z["grid"])).abs().max()) <= 1e-5
    f = ct.parity_figures(torch.from_numpy(z["grid_bf16"]), torch.from_numpy(z["grid"]), torch.from_numpy(z["grid_bf16"]))
    assert f["coverage"] >= 0.5 and f["misordered"] == 0 and 0 < f["e_ref16"] < 0.05


# ---------------------------------------------------------------- 4. preprocessing
def test_preprocess_without_padding_equals_hf_clip_image_processor():
    from PIL import Image
    from transformers import CLIPImageProcessor
    from t2v_metrics_amd.preprocess import clip_preprocess
    rng = np.random.RandomState(4)
    proc = CLIPImageProcessor(size={"shortest_edge": 336}, crop_size={"height": 336, "width": 336})
    for h, w in ((500, 380), (300, 640)):
        im = Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8))
        ref = proc(images=im, return_tensors="np")["pixel_values"][0]
        got = clip_preprocess(im, 336, pad_to_square=False)
        assert got.shape == (3, 336, 336)
        np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6)
