"""CLIPScore row: OpenAI CLIP ViT-L/14 towers on the HIP engine (C ABI: include/vqs_clip.h)."""
from .config import CLIP_CONFIGS, ClipConfig, get_clip_config  # noqa: F401
