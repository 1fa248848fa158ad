"""fp32 truth of the CLIPScore tests: HF ``transformers`` ``CLIPModel`` built from a config with the seeded weights (the installed
dependency that holds the arithmetic), its bf16 execution (the tolerance's yardstick), a plain-torch fp32 restatement of the same
forward (what the per-kernel GPU tests take their pieces from), seeded inputs and a tokenizer double (no vocabulary files here)."""
from __future__ import annotations

import math
import zlib
from typing import Dict, List, Sequence, Tuple

import torch

from t2v_metrics_amd.clip.config import ClipConfig, to_hf_config
from t2v_metrics_amd.clip.weights import make_seeded_clip_weights


def hf_model(cfg: ClipConfig, weights: Dict[str, torch.Tensor], dtype=torch.float32):
    """HF CLIPModel holding `weights` (bf16 values) in `dtype`, eager attention, eval mode."""
    from transformers import CLIPModel
    hc = to_hf_config(cfg)
    hc._attn_implementation = "eager"
    model = CLIPModel(hc)
    sd = {k: v.float() for k, v in weights.items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    missing = [k for k in missing if not (k.endswith("position_ids") or k == "logit_scale")]
    assert not missing and not unexpected, (missing[:5], unexpected[:5])
    return model.to(dtype).eval()


@torch.no_grad()
def hf_embeddings(cfg: ClipConfig, weights, pixels: torch.Tensor, ids: torch.Tensor, dtype=torch.float32) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (image embeddings [M, E], text embeddings [N, E]) as fp32 unit vectors, computed by HF in `dtype`.  Pooling is HF's own
    (first position of eos_token_id)."""
    m = hf_model(cfg, weights, dtype)
    vis = m.vision_model(pixel_values=pixels.to(dtype)).pooler_output
    img = m.visual_projection(vis)
    txt = m.text_projection(m.text_model(input_ids=ids.long()).pooler_output)
    img, txt = img.float(), txt.float()
    return img / img.norm(dim=-1, keepdim=True), txt / txt.norm(dim=-1, keepdim=True)


def hf_grid(cfg, weights, pixels, ids, dtype=torch.float32):
    img, txt = hf_embeddings(cfg, weights, pixels, ids, dtype)
    return img, txt, img @ txt.t()


# ---------------------------------------------------------------- plain-torch fp32 restatement
def causal_attention_ref(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float = 0.125) -> torch.Tensor:
    """q / k / v [B, H, S, 64] -> fp32 [B*S, H*64]; mask = key <= query."""
    B, H, S, hd = q.shape
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    s = s.masked_fill(torch.ones(S, S, dtype=torch.bool, device=q.device).triu(1), float("-inf"))
    o = torch.softmax(s, dim=-1) @ v.float()
    return o.permute(0, 2, 1, 3).reshape(B * S, H * hd)


def pool_head_ref(x: torch.Tensor, rows, ln_w, ln_b, proj, eps: float) -> torch.Tensor:
    """x fp32 [n, S, D] -> LayerNorm of row rows[b] (None: 0), bias-free projection, L2 normalisation; fp32 [n, E]."""
    n = x.shape[0]
    r = torch.zeros(n, dtype=torch.long) if rows is None else rows.long().cpu()
    p = x.float().cpu()[torch.arange(n), r]
    p = torch.nn.functional.layer_norm(p, (p.shape[-1],), ln_w.float().cpu(), ln_b.float().cpu(), eps)
    e = p @ proj.float().cpu().t()
    return e / e.norm(dim=-1, keepdim=True)


def _blocks(x, W, prefix, layers, heads, eps, causal):
    n, S, D = x.shape
    for i in range(layers):
        p = f"{prefix}encoder.layers.{i}."
        ln = lambda t, nm: torch.nn.functional.layer_norm(t, (D,), W[p + nm + ".weight"], W[p + nm + ".bias"], eps)   # noqa: E731
        lin = lambda t, nm: t @ W[p + nm + ".weight"].t() + W[p + nm + ".bias"]   # noqa: E731
        h = ln(x, "layer_norm1")
        q, k, v = (lin(h, "self_attn." + nm).view(n, S, heads, 64).transpose(1, 2) for nm in ("q_proj", "k_proj", "v_proj"))
        s = (q @ k.transpose(-1, -2)) * 0.125
        if causal:
            s = s.masked_fill(torch.ones(S, S, dtype=torch.bool).triu(1), float("-inf"))
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(n, S, D)
        x = x + lin(a, "self_attn.out_proj")
        h = lin(ln(x, "layer_norm2"), "mlp.fc1")
        x = x + lin(h * torch.sigmoid(1.702 * h), "mlp.fc2")
    return x


@torch.no_grad()
def restated_embeddings(cfg: ClipConfig, weights, pixels: torch.Tensor, ids: torch.Tensor, eot_pos: torch.Tensor):
    """The CLIP forward in plain fp32 torch (no HF module): -> (image [M, E], text [N, E]) unit vectors."""
    W = {k: v.float().cpu() for k, v in weights.items()}
    v, t = cfg.vision, cfg.text
    px = pixels.float().cpu()
    n = px.shape[0]
    patches = torch.nn.functional.conv2d(px, W["vision_model.embeddings.patch_embedding.weight"], stride=v.patch).flatten(2).transpose(1, 2)
    x = torch.cat([W["vision_model.embeddings.class_embedding"].expand(n, 1, -1), patches], 1) + W["vision_model.embeddings.position_embedding.weight"]
    x = torch.nn.functional.layer_norm(x, (v.hidden,), W["vision_model.pre_layrnorm.weight"], W["vision_model.pre_layrnorm.bias"], v.ln_eps)
    x = _blocks(x, W, "vision_model.", v.layers, v.heads, v.ln_eps, False)
    img = pool_head_ref(x, None, W["vision_model.post_layernorm.weight"], W["vision_model.post_layernorm.bias"], W["visual_projection.weight"], v.ln_eps)
    L = ids.shape[1]
    y = W["text_model.embeddings.token_embedding.weight"][ids.long().cpu()] + W["text_model.embeddings.position_embedding.weight"][:L]
    y = _blocks(y, W, "text_model.", t.layers, t.heads, t.ln_eps, True)
    txt = pool_head_ref(y, eot_pos, W["text_model.final_layer_norm.weight"], W["text_model.final_layer_norm.bias"], W["text_projection.weight"], t.ln_eps)
    return img, txt


# ---------------------------------------------------------------- seeded inputs
def seeded_inputs(cfg: ClipConfig, n_img: int, lengths: Sequence[int], seed: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """-> (pixels bf16 [n_img, 3, S, S], ids int32 [n_txt, max(lengths)] = BOS, words, EOT, EOT padding; eot_pos int32 [n_txt]).
    lengths count BOS and EOT (>= 2).  Words avoid the BOS / EOT ids."""
    g = torch.Generator().manual_seed(seed)
    S, t = cfg.vision.image, cfg.text
    pixels = torch.randn(n_img, 3, S, S, generator=g).to(torch.bfloat16)
    L = max(lengths)
    assert min(lengths) >= 2 and L <= t.context
    ids = torch.full((len(lengths), L), t.eot_id, dtype=torch.int32)
    pos = torch.empty(len(lengths), dtype=torch.int32)
    hi = min(t.bos_id, t.eot_id)
    for i, n in enumerate(lengths):
        ids[i, 0] = t.bos_id
        ids[i, 1:n - 1] = torch.randint(1, hi, (n - 2,), generator=g, dtype=torch.int32)
        pos[i] = n - 1
    return pixels, ids, pos


def parity_figures(grid: torch.Tensor, grid32: torch.Tensor, grid16: torch.Tensor) -> dict:
    """The issue's figures: e_ref16 = max |cos_bf16 - cos_fp32| (HF's own 16-bit execution), the engine's max |cos - cos_fp32|, and the
    ranking check -- for every image, every pair of texts whose fp32 cosines differ by more than 2 e_ref16 must be ordered the same way."""
    g, g32, g16 = grid.double().cpu(), grid32.double().cpu(), grid16.double().cpu()
    e_ref16 = float((g16 - g32).abs().max())
    d32 = g32[:, :, None] - g32[:, None, :]
    de = g[:, :, None] - g[:, None, :]
    N = g32.shape[1]
    upper = torch.ones(N, N, dtype=torch.bool).triu(1)[None]
    judged = (d32.abs() > 2 * e_ref16) & upper
    total = int(upper.sum()) * g32.shape[0]
    wrong = int((judged & (torch.sign(d32) != torch.sign(de))).sum())
    return {"e_ref16": e_ref16, "e_engine": float((g - g32).abs().max()), "triples": total, "judged": int(judged.sum()),
            "coverage": (int(judged.sum()) / total) if total else 1.0, "misordered": wrong}


class ClipTokenizerDouble:
    """HF ``CLIPTokenizer`` protocol without a vocabulary: ``tokenizer(text).input_ids`` = [BOS, one id per whitespace word (a stable
    hash into the ids below BOS / EOT), EOT]."""

    def __init__(self, cfg: ClipConfig):
        self.bos, self.eot = cfg.text.bos_id, cfg.text.eot_id
        self.hi = min(self.bos, self.eot)

    class _Out:
        def __init__(self, ids):
            self.input_ids = ids

    def __call__(self, text: str):
        words = [1 + zlib.crc32(w.encode()) % (self.hi - 1) for w in text.split()]
        return self._Out([self.bos] + words + [self.eot])


def seeded_weights(cfg: ClipConfig, seed: int = 0):
    return make_seeded_clip_weights(cfg, seed=seed, device="cpu")


def sqrt_embed_scatter(cfg: ClipConfig) -> float:
    return 1.0 / math.sqrt(cfg.embed_dim)
