"""CLIPScore model registry (the interface of the reference's models/clipscore_models package)."""
from ...constants import HF_CACHE_DIR
from .clip_model import CLIP_MODELS, CLIPModel
from .clipscore_model import CLIPScoreModel  # noqa: F401

ALL_CLIP_MODELS = [CLIP_MODELS]


def list_all_clipscore_models():
    return [model for models in ALL_CLIP_MODELS for model in models]


def get_clipscore_model(model_name, device='cuda', cache_dir=HF_CACHE_DIR, **kwargs):
    assert model_name in list_all_clipscore_models()
    if model_name in CLIP_MODELS:
        return CLIPModel(model_name, device=device, cache_dir=cache_dir, **kwargs)
    raise NotImplementedError()
