"""Architecture constants of the CLIPScore row: HF ``CLIPConfig`` (models/clip/configuration_clip.py) restated as plain data.

``openai:ViT-L-14-336`` = openai/clip-vit-large-patch14-336, ``openai:ViT-L-14`` = openai/clip-vit-large-patch14 (224 px); the two
differ in the image size only.  The test configurations keep every kernel constraint (64-wide heads in both towers, hidden sizes
multiples of 128): ``clip-tiny`` has a context that is not a multiple of 16, ``clip-small`` the real context of 77.
"""
from __future__ import annotations

from dataclasses import asdict, dataclass, field

from ..config import VisionConfig


@dataclass(frozen=True)
class ClipTextConfig:
    hidden: int = 768
    layers: int = 12
    heads: int = 12
    mlp: int = 3072
    vocab: int = 49408
    context: int = 77
    ln_eps: float = 1e-5
    bos_id: int = 49406
    eot_id: int = 49407          # also HF's pad id for the OpenAI vocabulary


@dataclass(frozen=True)
class ClipConfig:
    name: str = "openai:ViT-L-14-336"
    vision: VisionConfig = field(default_factory=lambda: VisionConfig(select_layer=24))     # every layer is run
    text: ClipTextConfig = field(default_factory=ClipTextConfig)
    embed_dim: int = 768
    hf_repo: str = "openai/clip-vit-large-patch14-336"

    def to_dict(self):
        return asdict(self)

    # algorithmic FLOPs (2 per MAC; GEMMs + QK^T + PV), as ClipT5Config counts them
    def flops_image(self) -> float:
        v = self.vision
        s, d, f = v.seq, v.hidden, v.mlp
        return v.layers * (8 * s * d * d + 4 * s * d * f + 4 * s * s * d) + 2 * v.n_patches * (3 * v.patch * v.patch) * d + 2 * d * self.embed_dim

    def flops_text(self, L: int) -> float:
        t = self.text
        return t.layers * (8 * L * t.hidden ** 2 + 4 * L * t.hidden * t.mlp + 4 * L * L * t.hidden) + 2 * t.hidden * self.embed_dim


def _vit(**kw) -> VisionConfig:
    kw.setdefault("select_layer", kw.get("layers", 24))
    return VisionConfig(**kw)


CLIP_VIT_L_14_336 = ClipConfig()
CLIP_VIT_L_14 = ClipConfig(name="openai:ViT-L-14", vision=_vit(image=224), hf_repo="openai/clip-vit-large-patch14")
CLIP_TINY = ClipConfig(name="clip-tiny", vision=_vit(hidden=128, layers=3, heads=2, mlp=256, image=56),
                       text=ClipTextConfig(hidden=128, layers=2, heads=2, mlp=256, vocab=512, context=21, bos_id=510, eot_id=511),
                       embed_dim=64, hf_repo="")
CLIP_SMALL = ClipConfig(name="clip-small", vision=_vit(hidden=256, layers=4, heads=4, mlp=512, image=112),
                        text=ClipTextConfig(hidden=256, layers=3, heads=4, mlp=512, vocab=1024, context=77, bos_id=1022, eot_id=1023),
                        embed_dim=128, hf_repo="")

CLIP_CONFIGS = {c.name: c for c in (CLIP_VIT_L_14_336, CLIP_VIT_L_14, CLIP_TINY, CLIP_SMALL)}
CLIPSCORE_MODELS = ("openai:ViT-L-14-336", "openai:ViT-L-14")


def get_clip_config(name: str) -> ClipConfig:
    return CLIP_CONFIGS[name]


def to_hf_config(cfg: ClipConfig):
    """The HF ``CLIPConfig`` of this architecture (what the parity tests build their fp32 truth from)."""
    from transformers import CLIPConfig
    v, t = cfg.vision, cfg.text
    return CLIPConfig(
        text_config=dict(vocab_size=t.vocab, hidden_size=t.hidden, intermediate_size=t.mlp, num_hidden_layers=t.layers,
                         num_attention_heads=t.heads, max_position_embeddings=t.context, hidden_act="quick_gelu", layer_norm_eps=t.ln_eps,
                         bos_token_id=t.bos_id, eos_token_id=t.eot_id, pad_token_id=t.eot_id, projection_dim=cfg.embed_dim),
        vision_config=dict(hidden_size=v.hidden, intermediate_size=v.mlp, num_hidden_layers=v.layers, num_attention_heads=v.heads,
                           image_size=v.image, patch_size=v.patch, hidden_act="quick_gelu", layer_norm_eps=v.ln_eps,
                           projection_dim=cfg.embed_dim),
        projection_dim=cfg.embed_dim)
