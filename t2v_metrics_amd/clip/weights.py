"""Weight inventory of HF ``CLIPModel`` (state_dict names) and a seeded generator for checkpoint-free runs, as
t2v_metrics_amd/weights.py has for CLIP-FlanT5: every tensor from its own seeded normal distribution, the same materialised bf16
tensors going to the HIP engine and to the fp32 truth."""
from __future__ import annotations

from typing import Dict, Iterator, List, Tuple

import torch

from ..weights import Spec, _tensor_seed, read_checkpoint_dir
from .config import ClipConfig


def clip_weight_specs(cfg: ClipConfig) -> List[Spec]:
    v, t = cfg.vision, cfg.text
    specs: List[Spec] = []

    def tower(prefix: str, layers: int, hd: int, mlp: int):
        for i in range(layers):
            p = f"{prefix}encoder.layers.{i}."
            for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
                specs.append((p + f"self_attn.{nm}.weight", (hd, hd), ("normal", hd ** -0.5)))
                specs.append((p + f"self_attn.{nm}.bias", (hd,), ("zeros", 0.02)))
            specs.extend([
                (p + "layer_norm1.weight", (hd,), ("ones", 0.1)), (p + "layer_norm1.bias", (hd,), ("zeros", 0.02)),
                (p + "mlp.fc1.weight", (mlp, hd), ("normal", hd ** -0.5)), (p + "mlp.fc1.bias", (mlp,), ("zeros", 0.02)),
                (p + "mlp.fc2.weight", (hd, mlp), ("normal", mlp ** -0.5)), (p + "mlp.fc2.bias", (hd,), ("zeros", 0.02)),
                (p + "layer_norm2.weight", (hd,), ("ones", 0.1)), (p + "layer_norm2.bias", (hd,), ("zeros", 0.02)),
            ])

    hd = v.hidden
    specs += [
        ("vision_model.embeddings.class_embedding", (hd,), ("normal", 0.5)),
        ("vision_model.embeddings.patch_embedding.weight", (hd, 3, v.patch, v.patch), ("normal", (3 * v.patch * v.patch) ** -0.5)),
        ("vision_model.embeddings.position_embedding.weight", (v.seq, hd), ("normal", 0.1)),
        ("vision_model.pre_layrnorm.weight", (hd,), ("ones", 0.1)),
        ("vision_model.pre_layrnorm.bias", (hd,), ("zeros", 0.02)),
    ]
    tower("vision_model.", v.layers, hd, v.mlp)
    specs += [
        ("vision_model.post_layernorm.weight", (hd,), ("ones", 0.1)),
        ("vision_model.post_layernorm.bias", (hd,), ("zeros", 0.02)),
        ("visual_projection.weight", (cfg.embed_dim, hd), ("normal", hd ** -0.5)),
        ("text_model.embeddings.token_embedding.weight", (t.vocab, t.hidden), ("normal", 0.5)),
        ("text_model.embeddings.position_embedding.weight", (t.context, t.hidden), ("normal", 0.2)),
    ]
    tower("text_model.", t.layers, t.hidden, t.mlp)
    specs += [
        ("text_model.final_layer_norm.weight", (t.hidden,), ("ones", 0.1)),
        ("text_model.final_layer_norm.bias", (t.hidden,), ("zeros", 0.02)),
        ("text_projection.weight", (cfg.embed_dim, t.hidden), ("normal", t.hidden ** -0.5)),
    ]
    return specs


def iter_seeded_clip_weights(cfg: ClipConfig, seed: int = 0, device="cpu", dtype=torch.bfloat16) -> Iterator[Tuple[str, torch.Tensor]]:
    dev = torch.device(device)
    for name, shape, (kind, scale) in clip_weight_specs(cfg):
        g = torch.Generator(device=dev)
        g.manual_seed(_tensor_seed(seed, name))
        x = torch.randn(shape, generator=g, device=dev, dtype=torch.float32).mul_(scale)
        if kind == "ones":
            x.add_(1.0)
        yield name, x.to(dtype)


def make_seeded_clip_weights(cfg: ClipConfig, seed: int = 0, device="cpu", dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    return dict(iter_seeded_clip_weights(cfg, seed, device, dtype))


def load_clip_checkpoint(cfg: ClipConfig, path: str, device, dtype=torch.bfloat16) -> Dict[str, torch.Tensor]:
    """A local HF ``CLIPModel`` directory (safetensors / .bin shards) -> the inventory, cast to bf16.  ``logit_scale`` and the
    ``position_ids`` buffers are not used.  Raises KeyError naming what is missing, ValueError on a shape mismatch."""
    sd = read_checkpoint_dir(path)
    out, missing = {}, []
    for name, shape, _ in clip_weight_specs(cfg):
        if name not in sd:
            missing.append(name)
            continue
        if tuple(sd[name].shape) != tuple(shape):
            raise ValueError(f"{name}: checkpoint shape {tuple(sd[name].shape)} != expected {shape}")
        out[name] = sd[name].to(device=device, dtype=dtype).contiguous()
    if missing:
        raise KeyError(f"{len(missing)} tensors missing from checkpoint, e.g. {missing[:5]}")
    return out
