"""``CLIPScore`` -- the user-facing cosine scorer (v3.0 interface: ``t2v_metrics.CLIPScore(model='openai:ViT-L-14-336')``).

A ``Score`` whose plugin comes from the CLIPScore model registry; ``forward(images, texts) -> [M, N]`` encodes each distinct image and
each distinct text once and takes one similarity launch, ``batch_forward`` goes through ``Score.batch_forward`` (de-duplicated encodes
per batch), ``distributed=True`` shards as the VQAScore path does.  Extra keyword arguments reach the plugin's constructor unchanged
(``weights=``, ``tokenizer=``, ``checkpoint=``, ``config=``, ``engine=``, ``engine_options=``).
"""
from typing import List

from . import constants
from .models import clipscore_models as _registry
from .models.clipscore_models import list_all_clipscore_models  # noqa: F401  (re-exported: t2v_metrics_amd/__init__.py)
from .score import Score


class CLIPScore(Score):
    """cos(image embedding, text embedding) scorers: OpenAI CLIP ViT-L/14 (336 px / 224 px) on the MI355X engine."""

    def prepare_scoremodel(self, model='openai:ViT-L-14-336', device='cuda', cache_dir=constants.HF_CACHE_DIR, **kwargs):
        return _registry.get_clipscore_model(model, device=device, cache_dir=cache_dir, **kwargs)

    def list_all_models(self) -> List[str]:
        return _registry.list_all_clipscore_models()
