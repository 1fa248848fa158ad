"""OpenAI CLIP ViT-L/14 CLIPScore model on the MI355X-native engine.

Host-side mirror of the v3.0 CLIPScore wrapper the reference documents (V_3.0_README.md "CLIPScore", ``t2v_metrics.CLIPScore(model=
'openai:ViT-L-14-336')``).  [RECALLED: the v3.0 ``clip_model.py`` is not in the in-tree snapshot of the reference; from memory it loads
the open_clip model, preprocesses with the model's transform, tokenises at context 77, L2-normalises both features and returns their
plain dot product -- ``logit_scale`` is NOT applied.  That recipe is what is restated here.]

What runs where:
  host (this file)   PIL decode, shortest-edge bicubic resize + centre crop (no expand2square), tokenisation (HF ``CLIPTokenizer``
                     protocol: ``tokenizer(text).input_ids`` = BOS ... EOT), truncation at 77 keeping the EOT last, EOT position;
  device (engine)    uint8 -> CLIP-normalised bf16 pixels, both towers, projection heads, L2 norm, cosine -- hand-written gfx950
                     kernels behind the C ABI (include/vqs_clip.h).  No torch.nn forward, no HF forward, no CPU fallback.
Each distinct image and each distinct text of a call is encoded once; the reference runs a full forward per pair.
An entry of ``images`` may also be an in-memory image (``PIL.Image``, uint8 ``np.ndarray`` / ``torch.Tensor`` [H, W, 3] RGB; imagefront.py);
with ``device_preprocess=True`` their resize + crop runs on the GPU (include/vqs.h vqs_images_u8), bitwise the host path.
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ...clip.config import CLIPSCORE_MODELS, get_clip_config
from ...constants import HF_CACHE_DIR
from ...imagefront import SourceStaging, dedupe, entry_image, is_path, load_pixels
from .clipscore_model import CLIPScoreModel

CLIP_MODELS = {name: {'config': name, 'hf_repo': get_clip_config(name).hf_repo} for name in CLIPSCORE_MODELS}


class CLIPModel(CLIPScoreModel):
    video_mode = "concat"
    allows_image = True
    allows_video = False

    def __init__(self, model_name='openai:ViT-L-14-336', device='cuda', cache_dir=HF_CACHE_DIR, *, weights=None, tokenizer=None,
                 checkpoint: Optional[str] = None, config=None, max_images: int = 256, max_texts: int = 1024, seed: int = 0, engine=None,
                 num_workers: Optional[int] = None, engine_options: Optional[Dict[str, int]] = None, device_preprocess: bool = False):
        """
        weights:    None -> load ``checkpoint`` (a local HF ``CLIPModel`` directory of safetensors); 'seeded' -> seeded random weights at the
                    exact architecture (benchmarks, tests); or a dict name -> tensor (HF CLIPModel state_dict names).
        tokenizer:  any object with the HF ``CLIPTokenizer`` protocol (``tokenizer(text).input_ids`` -> [BOS, ..., EOT]); None -> the
                    tokenizer of the checkpoint directory.
        config:     a ClipConfig overriding the registry entry (tests use the tiny configurations).
        engine:     an already constructed engine-like object (tests inject a recording double).
        engine_options: options of include/vqs_clip.h, e.g. {'fp16': 0} for bf16 operands.
        device_preprocess: True = the in-memory entries of a call are resized and cropped on the GPU (engine.images_from_u8), bitwise the
                    host path; paths keep the host path.  Ignored by an engine without that method.
        """
        assert config is not None or model_name in CLIP_MODELS
        self._weights_arg, self._tokenizer_arg, self._checkpoint = weights, tokenizer, checkpoint
        self._cfg = config if config is not None else get_clip_config(CLIP_MODELS[model_name]['config'])
        self._seed, self._engine_arg = seed, engine
        self._engine_options = dict(engine_options or {})
        try:
            cores = len(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            cores = os.cpu_count() or 1
        self.num_workers = min(32, cores) if num_workers is None else max(1, int(num_workers))
        self._pool = None
        self.device_preprocess = bool(device_preprocess)
        self._src_staging = SourceStaging()
        self.max_images, self.max_texts = int(max_images), int(max_texts)
        super().__init__(model_name=model_name, device=device, cache_dir=cache_dir)

    # ------------------------------------------------------------------ loading
    def load_model(self):
        self.cfg = self._cfg
        self.context_len = self.cfg.text.context
        self.tokenizer = self._tokenizer_arg if self._tokenizer_arg is not None else self._load_tokenizer()
        if self._engine_arg is not None:
            self.engine = self._engine_arg
            return
        from ...clip.engine import ClipEngine   # raises if libvqs_hip.so is missing; no fallback
        from ...clip.weights import load_clip_checkpoint, make_seeded_clip_weights
        dev = torch.device(self.device if str(self.device) != 'cuda' else 'cuda:0')
        if isinstance(self._weights_arg, dict):
            weights = self._weights_arg
        elif self._weights_arg == 'seeded':
            weights = make_seeded_clip_weights(self.cfg, seed=self._seed, device=dev)
        else:
            weights = load_clip_checkpoint(self.cfg, self._checkpoint_dir(must_exist=True), dev)
        self.engine = ClipEngine(self.cfg, weights, device=dev, options=self._engine_options)

    def _checkpoint_dir(self, must_exist: bool = False) -> str:
        path = self._checkpoint or os.path.join(self.cache_dir, (self.cfg.hf_repo or self.model_name).split('/')[-1])
        if must_exist and not os.path.isdir(path):
            raise FileNotFoundError(f"no checkpoint at {path} (no network here). Pass checkpoint=<local HF dir> or weights='seeded'.")
        return path

    def _load_tokenizer(self):
        path = self._checkpoint_dir()
        if not os.path.isdir(path):
            raise FileNotFoundError(f"no tokenizer: {path} does not exist (no network here). Pass tokenizer=... or checkpoint=<local HF dir>.")
        from transformers import CLIPTokenizer
        return CLIPTokenizer.from_pretrained(path)

    # ------------------------------------------------------------------ host-side preparation
    def _preprocess_one_u8(self, path) -> np.ndarray:
        from ...preprocess import clip_preprocess_u8
        img = self.image_loader(path) if is_path(path) else entry_image(path)      # in-memory entries: the same pixels as a PIL image
        return clip_preprocess_u8(img, self.cfg.vision.image, False)

    def _load_u8(self, image: Sequence[str]) -> torch.Tensor:
        S = self.cfg.vision.image
        out = torch.empty(len(image), S, S, 3, dtype=torch.uint8)
        arr = out.numpy()
        if self._pool is None and self.num_workers > 1 and len(image) > 1:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.num_workers, thread_name_prefix="clip-img")
        results = self._pool.map(self._preprocess_one_u8, image) if (self._pool is not None and len(image) > 1) else map(self._preprocess_one_u8, image)
        for i, a in enumerate(results):
            arr[i] = a
        return out

    def load_images(self, image: List[str]) -> torch.Tensor:
        """Decode + shortest-edge bicubic resize + centre crop on the host; rescale + CLIP mean / std + bf16 on the GPU
        (vqs_normalize_u8, the fp32 arithmetic of HF CLIPImageProcessor) -> bf16 [N, 3, S, S] on the device."""
        on_gpu = str(self.device).startswith('cuda') and torch.cuda.is_available()
        if self.device_preprocess and on_gpu and hasattr(self.engine, "images_from_u8"):
            if not all(is_path(p) for p in image):      # the device front end, one call per source size; paths keep the host path
                return load_pixels(self.engine, self.device, self._src_staging, image, self.cfg.vision.image, False, self._load_images_from_host,
                                   self._pool)
        return self._load_images_from_host(image)

    def _load_images_from_host(self, image: List[str]) -> torch.Tensor:
        from ...preprocess import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
        u8 = self._load_u8(image)
        if hasattr(self.engine, "normalize_u8") and str(self.device).startswith('cuda') and torch.cuda.is_available():
            return self.engine.normalize_u8(u8.to(self.device), OPENAI_CLIP_MEAN, OPENAI_CLIP_STD)
        px = (u8.float() * (1.0 / 255.0) - torch.tensor(OPENAI_CLIP_MEAN).view(1, 1, 1, 3)) / torch.tensor(OPENAI_CLIP_STD).view(1, 1, 1, 3)
        return px.permute(0, 3, 1, 2).contiguous().to(torch.bfloat16)

    def tokenize(self, texts: Sequence[str]) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (ids int32 [n, L] right-padded with the EOT id, eot_pos int32 [n]).  Rows longer than the context are cut to it with the
        EOT token kept last (HF / open_clip truncation); the EOT position is the first occurrence of the EOT id."""
        eot, ctx = self.cfg.text.eot_id, self.context_len
        rows = []
        for t in texts:
            ids = list(self.tokenizer(t).input_ids)
            if len(ids) > ctx:
                ids = ids[:ctx]
                ids[-1] = eot
            if eot not in ids:
                raise ValueError("the tokenizer did not end the text with the EOT token")
            rows.append(ids)
        L = max(len(r) for r in rows)
        out = torch.full((len(rows), L), eot, dtype=torch.int32)
        pos = torch.empty(len(rows), dtype=torch.int32)
        for i, r in enumerate(rows):
            out[i, :len(r)] = torch.tensor(r, dtype=torch.int32)
            pos[i] = r.index(eot)
        return out, pos

    # ------------------------------------------------------------------ scoring
    @torch.no_grad()
    def encode(self, images: Sequence[str], texts: Sequence[str]):
        """Distinct images and texts, each encoded once -> (image embeddings [U, E], text embeddings [V, E], image index per input,
        text index per input)."""
        ut: Dict[str, int] = {}
        paths, img_ix = dedupe(images)                # paths by str(p), in-memory images by identity; every entry checked first
        txt_ix = [ut.setdefault(t, len(ut)) for t in texts]
        utexts = list(ut.keys())
        img = [self.engine.encode_images(self.load_images(paths[s: s + self.max_images])) for s in range(0, len(paths), self.max_images)]
        txt = []
        for s in range(0, len(utexts), self.max_texts):
            ids, pos = self.tokenize(utexts[s: s + self.max_texts])
            txt.append(self.engine.encode_texts(ids, pos))
        return (img[0] if len(img) == 1 else torch.cat(img, 0)), (txt[0] if len(txt) == 1 else torch.cat(txt, 0)), img_ix, txt_ix

    def forward(self, images: List[str], texts: List[str]) -> torch.Tensor:
        """n cosines for n (image, text) pairs -> CPU fp32 [n]."""
        assert len(images) == len(texts), "Number of images and texts must match"
        if not images:
            return torch.zeros(0, dtype=torch.float32)
        img, txt, ii, tt = self.encode(images, texts)
        return self.engine.similarity_pairs(img, txt, ii, tt).float().cpu()

    def forward_grid(self, images: List[str], texts: List[str]) -> torch.Tensor:
        """All M x N pairs: M image encodes, N text encodes, one similarity launch -> CPU fp32 [M, N]."""
        if not images or not texts:
            return torch.zeros(len(images), len(texts), dtype=torch.float32)
        img, txt, ii, tt = self.encode(images, texts)
        grid = self.engine.similarity(img, txt).float().cpu()
        if ii != list(range(img.shape[0])) or tt != list(range(txt.shape[0])):     # duplicates in the call: expand the distinct grid
            grid = grid[torch.tensor(ii)][:, torch.tensor(tt)]
        return grid
