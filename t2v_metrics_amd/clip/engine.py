"""ctypes binding of the CLIPScore row of ``libvqs_hip.so`` (C ABI in ``include/vqs_clip.h``).

PyTorch is used for device memory and the current HIP stream only; every FLOP runs in the hand-written gfx950 kernels behind
the C ABI.  There is deliberately NO fallback: if the library is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes
import warnings
from typing import Dict, List, Optional, Sequence, Tuple

import torch

from ..engine import FP16_MAX_FINITE_ROUNDED, VqsError, _stream_ptr, images_from_u8, load_library, normalize_u8
from .config import ClipConfig

_c_i32, _c_i64, _c_f32, _c_vp, _c_sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t


class VqsClipConfig(ctypes.Structure):
    _fields_ = [
        ("vis_hidden", _c_i32), ("vis_layers", _c_i32), ("vis_heads", _c_i32), ("vis_mlp", _c_i32), ("vis_patch", _c_i32),
        ("vis_image", _c_i32), ("vis_eps", _c_f32),
        ("txt_hidden", _c_i32), ("txt_layers", _c_i32), ("txt_heads", _c_i32), ("txt_mlp", _c_i32), ("txt_vocab", _c_i32),
        ("txt_context", _c_i32), ("txt_eps", _c_f32), ("embed_dim", _c_i32),
    ]


class VqsClipWeightDesc(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("d_data", _c_vp), ("numel", _c_i64)]


# every symbol declared in include/vqs_clip.h: (restype, argtypes)
_SIGS = {
    "vqs_clip_create": (_c_i32, [ctypes.POINTER(VqsClipConfig), ctypes.POINTER(_c_vp)]),
    "vqs_clip_destroy": (None, [_c_vp]),
    "vqs_clip_last_error": (ctypes.c_char_p, [_c_vp]),
    "vqs_clip_packed_bytes": (_c_sz, [_c_vp]),
    "vqs_clip_bind_weights": (_c_i32, [_c_vp, ctypes.POINTER(VqsClipWeightDesc), _c_i32, _c_vp, _c_sz, _c_vp]),
    "vqs_clip_image_workspace_bytes": (_c_sz, [_c_vp, _c_i32]),
    "vqs_clip_encode_images": (_c_i32, [_c_vp, _c_vp, _c_i32, _c_vp, _c_vp, _c_sz, _c_vp]),
    "vqs_clip_text_workspace_bytes": (_c_sz, [_c_vp, _c_i32, _c_i32]),
    "vqs_clip_encode_texts": (_c_i32, [_c_vp, _c_vp, _c_vp, _c_i32, _c_i32, _c_vp, _c_vp, _c_sz, _c_vp]),
    "vqs_clip_similarity": (_c_i32, [_c_vp, _c_vp, _c_i32, _c_i32, _c_i32, _c_vp, _c_vp]),
    "vqs_clip_similarity_pairs": (_c_i32, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i32, _c_i32, _c_i32, _c_i32, _c_vp, _c_vp]),
    "vqs_clip_set_option": (_c_i32, [_c_vp, ctypes.c_char_p, _c_i32]),
    "vqs_clip_get_option": (_c_i32, [_c_vp, ctypes.c_char_p, ctypes.POINTER(_c_i32)]),
    "vqs_clip_causal_attention": (_c_i32, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i32, _c_i32, _c_i32, _c_f32, _c_i32, _c_vp]),
    "vqs_clip_embed": (_c_i32, [_c_vp, _c_vp, _c_vp, _c_vp, _c_i32, _c_i32, _c_i32, _c_i32, _c_vp]),
    "vqs_clip_pool_head": (_c_i32, [_c_vp, _c_vp, _c_i32, _c_vp, _c_vp, _c_vp, _c_vp, _c_vp, _c_i32, _c_i32, _c_i32, _c_i32, _c_f32, _c_vp]),
}

_typed = None


def clip_library() -> ctypes.CDLL:
    """libvqs_hip.so with the include/vqs_clip.h entry points typed.  Raises if the library or one of them is missing."""
    global _typed
    lib = load_library()
    if _typed is not lib:
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is not exported
            fn.restype, fn.argtypes = res, args
        _typed = lib
    return lib


def make_clip_config(cfg: ClipConfig) -> VqsClipConfig:
    v, t = cfg.vision, cfg.text
    return VqsClipConfig(v.hidden, v.layers, v.heads, v.mlp, v.patch, v.image, v.ln_eps, t.hidden, t.layers, t.heads, t.mlp, t.vocab,
                         t.context, t.ln_eps, cfg.embed_dim)


def clip_fp16_unsafe_weights(weights: Dict[str, torch.Tensor]) -> List[str]:
    """Names of the towers' linear weights an fp16 copy cannot hold (|w| >= 65 520 or not finite): what vqs_clip_bind_weights converts
    for option fp16 (q / k / v / out_proj / fc1 / fc2 of both towers), as engine.fp16_unsafe_weights does for the CLIP-FlanT5 row."""
    bad = []
    for k, w in weights.items():
        if w.dim() == 2 and k.endswith(".weight") and ".encoder.layers." in k:
            m = float(w.detach().abs().max().float()) if w.numel() else 0.0
            if not (m < FP16_MAX_FINITE_ROUNDED):
                bad.append(k)
    return bad


def eot_positions(ids: torch.Tensor, eot_id: int) -> torch.Tensor:
    """First occurrence of the EOT id in each row of ids [n, L] -> int32 [n] (for the OpenAI vocabulary, where EOT is the largest id,
    that is also argmax(ids): what open_clip and HF's legacy path take).  Raises if a row has none."""
    hit = ids == eot_id
    if not bool(hit.any(dim=1).all()):
        raise ValueError("every text row must contain the EOT token")
    return hit.to(torch.int32).argmax(dim=1).to(torch.int32)


class ClipEngine:
    """One CLIP replica (both towers + heads) on one GPU."""

    MIN_TEXT_LEN = 8           # rows shorter than this are padded: the q|k|v epilogue steps rows by 8 within a sample

    def __init__(self, cfg: ClipConfig, weights: Dict[str, torch.Tensor], device="cuda:0", options: Optional[Dict[str, int]] = None):
        self.lib = clip_library()
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise VqsError("ClipEngine needs a HIP device (device='cuda[:i]'); there is no CPU path")
        self._h = _c_vp()
        c = make_clip_config(cfg)
        rc = self.lib.vqs_clip_create(ctypes.byref(c), ctypes.byref(self._h))
        if rc != 0:
            msg = self.lib.vqs_clip_last_error(self._h).decode() if self._h else "vqs_clip_create failed"
            self.close()
            raise VqsError(f"vqs_clip_create: {msg}")
        self._explicit = set(options or {})
        self.fp16_auto_off: Optional[str] = None
        self._ws: Dict[str, torch.Tensor] = {}
        for k, v in (options or {}).items():
            self.set_option(k, v)
        self.bind(weights)

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise VqsError(f"{what} failed ({rc}): {self.lib.vqs_clip_last_error(self._h).decode()}")

    def close(self):
        if getattr(self, "_h", None):
            self.lib.vqs_clip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_option(self, name: str, value: int):
        self._check(self.lib.vqs_clip_set_option(self._h, name.encode(), int(value)), f"vqs_clip_set_option({name}={value})")

    def get_option(self, name: str) -> int:
        v = _c_i32()
        self._check(self.lib.vqs_clip_get_option(self._h, name.encode(), ctypes.byref(v)), f"vqs_clip_get_option({name})")
        return int(v.value)

    def bind(self, weights: Dict[str, torch.Tensor]):
        with torch.cuda.device(self.device):
            self.weights = {}
            for k, w in weights.items():
                if w.dtype != torch.bfloat16 or w.device != self.device or not w.is_contiguous():
                    w = w.to(device=self.device, dtype=torch.bfloat16).contiguous()
                self.weights[k] = w
            # fp16 copies must hold the weights: refused if the caller asked for fp16, switched off (one warning) if it was the default
            bad = clip_fp16_unsafe_weights(self.weights)
            if bad and self.get_option("fp16"):
                if "fp16" in self._explicit:
                    raise VqsError("fp16 = 1 refused: these weights exceed the fp16 range (|w| >= 65520): " + ", ".join(bad[:4]))
                self.set_option("fp16", 0)
                self.fp16_auto_off = "weights outside the fp16 range: " + ", ".join(bad[:4])
                warnings.warn("t2v_metrics_amd: CLIPScore option fp16 switched off at bind time -- " + self.fp16_auto_off +
                              "; both towers run on bf16 operands", RuntimeWarning, stacklevel=3)
            n = len(self.weights)
            descs = (VqsClipWeightDesc * n)()
            self._names = [k.encode() for k in self.weights]   # keep the char* alive
            for i, (k, w) in enumerate(self.weights.items()):
                descs[i] = VqsClipWeightDesc(self._names[i], w.data_ptr(), w.numel())
            nbytes = self.lib.vqs_clip_packed_bytes(self._h)
            self._packed = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._check(self.lib.vqs_clip_bind_weights(self._h, descs, n, self._packed.data_ptr(), nbytes, _stream_ptr()), "vqs_clip_bind_weights")

    def _workspace(self, key: str, need: int) -> torch.Tensor:
        if need == 0:
            raise VqsError(f"{key} workspace query refused the shape")
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._ws[key] = ws
        return ws

    # ------------------------------------------------------------------ passes
    def normalize_u8(self, x_u8: torch.Tensor, mean, std) -> torch.Tensor:
        with torch.cuda.device(self.device):
            return normalize_u8(x_u8.to(self.device), mean, std)

    def images_from_u8(self, src_u8: torch.Tensor, size: int, pad: bool) -> torch.Tensor:
        with torch.cuda.device(self.device):
            return images_from_u8(src_u8.to(self.device), size, pad)

    def encode_images(self, pixels: torch.Tensor) -> torch.Tensor:
        """pixels [n, 3, S, S] (CLIP-normalised; cast to bf16) -> fp32 unit embeddings [n, embed_dim] on the device."""
        S = self.cfg.vision.image
        if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (3, S, S):
            raise VqsError(f"encode_images expects [n, 3, {S}, {S}], got {tuple(pixels.shape)}")
        with torch.cuda.device(self.device):
            px = pixels.to(device=self.device, dtype=torch.bfloat16).contiguous()
            n = px.shape[0]
            out = torch.empty(n, self.cfg.embed_dim, dtype=torch.float32, device=self.device)
            ws = self._workspace("img", self.lib.vqs_clip_image_workspace_bytes(self._h, n))
            self._check(self.lib.vqs_clip_encode_images(self._h, px.data_ptr(), n, out.data_ptr(), ws.data_ptr(), ws.numel(), _stream_ptr()),
                        "vqs_clip_encode_images")
            return out

    def encode_texts(self, ids: torch.Tensor, eot_pos: Optional[torch.Tensor] = None) -> torch.Tensor:
        """ids int [n, L <= context], eot_pos int [n] (None: first occurrence of cfg.text.eot_id) -> fp32 unit embeddings [n, embed_dim]."""
        t = self.cfg.text
        if ids.dim() != 2 or not 1 <= ids.shape[1] <= t.context:
            raise VqsError(f"encode_texts expects ids [n, L <= {t.context}], got {tuple(ids.shape)}")
        ids = ids.to(torch.int32)
        if eot_pos is None:
            eot_pos = eot_positions(ids, t.eot_id)
        n, L = ids.shape
        if eot_pos.shape != (n,) or bool((eot_pos < 0).any()) or bool((eot_pos >= L).any()):
            raise VqsError("eot_pos must hold one position in [0, L) per row")
        if L < self.MIN_TEXT_LEN:          # rows behind the EOT are never read by the pooled row (causal mask)
            ids = torch.cat([ids, torch.full((n, self.MIN_TEXT_LEN - L), t.eot_id, dtype=torch.int32, device=ids.device)], 1)
            L = self.MIN_TEXT_LEN
        with torch.cuda.device(self.device):
            d_ids = ids.to(self.device).contiguous()
            d_eot = eot_pos.to(device=self.device, dtype=torch.int32).contiguous()
            out = torch.empty(n, self.cfg.embed_dim, dtype=torch.float32, device=self.device)
            ws = self._workspace("txt", self.lib.vqs_clip_text_workspace_bytes(self._h, n, L))
            self._check(self.lib.vqs_clip_encode_texts(self._h, d_ids.data_ptr(), d_eot.data_ptr(), n, L, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                                       _stream_ptr()), "vqs_clip_encode_texts")
            return out

    def similarity(self, img: torch.Tensor, txt: torch.Tensor) -> torch.Tensor:
        """fp32 [M, E] x [N, E] -> cosine grid fp32 [M, N] (the embeddings are unit vectors)."""
        return similarity(img, txt)

    def similarity_pairs(self, img: torch.Tensor, txt: torch.Tensor, idx_i: Sequence[int], idx_t: Sequence[int]) -> torch.Tensor:
        return similarity_pairs(img, txt, idx_i, idx_t)


def _f32(x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 2:
        raise VqsError("expected an fp32 [rows, E] tensor on the GPU")
    return x.contiguous()


def similarity(img: torch.Tensor, txt: torch.Tensor) -> torch.Tensor:
    lib = clip_library()
    img, txt = _f32(img), _f32(txt)
    (M, E), (N, E2) = img.shape, txt.shape
    if E != E2 or txt.device != img.device:
        raise VqsError("similarity: embeddings disagree on width or device")
    with torch.cuda.device(img.device):
        out = torch.empty(M, N, dtype=torch.float32, device=img.device)
        if M and N:
            rc = lib.vqs_clip_similarity(img.data_ptr(), txt.data_ptr(), M, N, E, out.data_ptr(), _stream_ptr())
            if rc != 0:
                raise VqsError(f"vqs_clip_similarity failed ({rc})")
        return out


def similarity_pairs(img: torch.Tensor, txt: torch.Tensor, idx_i, idx_t) -> torch.Tensor:
    lib = clip_library()
    img, txt = _f32(img), _f32(txt)
    with torch.cuda.device(img.device):
        ii = torch.as_tensor(idx_i, dtype=torch.int32).to(img.device).contiguous()
        tt = torch.as_tensor(idx_t, dtype=torch.int32).to(img.device).contiguous()
        if ii.shape != tt.shape or ii.dim() != 1 or img.shape[1] != txt.shape[1]:
            raise VqsError("similarity_pairs: index lists / embedding widths disagree")
        out = torch.empty(ii.shape[0], dtype=torch.float32, device=img.device)
        if ii.shape[0]:
            rc = lib.vqs_clip_similarity_pairs(img.data_ptr(), txt.data_ptr(), ii.data_ptr(), tt.data_ptr(), img.shape[0], txt.shape[0],
                                               ii.shape[0], img.shape[1], out.data_ptr(), _stream_ptr())
            if rc != 0:
                raise VqsError(f"vqs_clip_similarity_pairs failed ({rc})")
        return out


# ---- single-kernel wrappers (parity tests)
def causal_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float = 0.125) -> torch.Tensor:
    """q / k / v [B, H, S, 64] bf16 or fp16 on the GPU -> [B*S, H*64] of the same type."""
    lib = clip_library()
    B, H, S, hd = q.shape
    if hd != 64 or q.dtype not in (torch.bfloat16, torch.float16) or k.shape != q.shape or v.shape != q.shape:
        raise VqsError("causal_attention expects three [B, H, S, 64] bf16 / fp16 tensors")
    with torch.cuda.device(q.device):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        out = torch.empty(B * S, H * 64, dtype=q.dtype, device=q.device)
        rc = lib.vqs_clip_causal_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), B, H, S, float(scale),
                                           1 if q.dtype == torch.float16 else 0, _stream_ptr())
        if rc != 0:
            raise VqsError(f"vqs_clip_causal_attention failed ({rc})")
        return out


def embed(ids: torch.Tensor, tok: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    lib = clip_library()
    n, L = ids.shape
    with torch.cuda.device(tok.device):
        ids = ids.to(device=tok.device, dtype=torch.int32).contiguous()
        out = torch.empty(n, L, tok.shape[1], dtype=torch.float32, device=tok.device)
        rc = lib.vqs_clip_embed(ids.data_ptr(), tok.data_ptr(), pos.data_ptr(), out.data_ptr(), n, L, tok.shape[1], tok.shape[0], _stream_ptr())
        if rc != 0:
            raise VqsError(f"vqs_clip_embed failed ({rc})")
        return out


def pool_head(x: torch.Tensor, delta: Optional[torch.Tensor], rows: Optional[torch.Tensor], ln_w, ln_b, proj, eps: float) -> torch.Tensor:
    lib = clip_library()
    n, S, D = x.shape
    with torch.cuda.device(x.device):
        out = torch.empty(n, proj.shape[0], dtype=torch.float32, device=x.device)
        r = None if rows is None else rows.to(device=x.device, dtype=torch.int32).contiguous()
        rc = lib.vqs_clip_pool_head(x.data_ptr(), None if delta is None else delta.data_ptr(), 1 if (delta is not None and delta.dtype == torch.float16) else 0,
                                    None if r is None else r.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), proj.data_ptr(), out.data_ptr(),
                                    n, S, D, proj.shape[0], float(eps), _stream_ptr())
        if rc != 0:
            raise VqsError(f"vqs_clip_pool_head failed ({rc})")
        return out
