#!/usr/bin/env python
"""Print, as JSON, every size and offset the host side of libvqs_hip.so computes for a fixed list of configurations and shapes:
packed-buffer sizes, every *_workspace_bytes / kv_bytes / prefix_* / suffix_* query and vqs_workspace_offset (with its ld) for every
name the carvers register.  The size queries touch no device, so this runs without a GPU.

tests/golden/host_layout.json is this tool's output on a library built from the commit BEFORE the three handles' host scaffolding
was merged into csrc/vqs_host.h; tests/test_host_layout.py holds the current library to it byte for byte.  To repeat it: build
that commit (make -C t2v_metrics_amd/csrc) and run  python tools/host_layout_dump.py --lib <its libvqs_hip.so> > host_layout.json

usage: python tools/host_layout_dump.py [--lib PATH]"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OFFSET_NAMES = ("vit_hidden", "enc_len", "flags", "enc_in", "enc_out", "dec_out", "logits")
BATCHES = (1, 4, 256)


def _key(*xs):
    return "x".join(str(x) for x in xs)


def dump_clip_t5(lib, name):
    from t2v_metrics_amd.config import get_config
    from t2v_metrics_amd.engine import make_vqs_config
    c = make_vqs_config(get_config(name))
    h = ctypes.c_void_p()
    assert lib.vqs_create(ctypes.byref(c), ctypes.byref(h)) == 0, name
    out = {"packed_bytes": lib.vqs_packed_bytes(h)}
    out["encode_workspace_bytes"] = {_key(n): lib.vqs_encode_workspace_bytes(h, n) for n in BATCHES + (0,)}
    shapes = [(B, L, T) for B in BATCHES for (L, T) in ((33, 2), (9, 1), (33, 16))] + [(0, 33, 2)]
    out["score_workspace_bytes"] = {_key(*s): lib.vqs_score_workspace_bytes(h, *s) for s in shapes}
    out["generate_workspace_bytes"] = {_key(B, 33, n): lib.vqs_generate_workspace_bytes(h, B, 33, n)
                                       for B in BATCHES for n in (1, 64)}
    offs = {}
    for s in shapes[:-1]:
        for nm in OFFSET_NAMES:
            ld = ctypes.c_int64(-7)
            off = lib.vqs_workspace_offset(h, nm.encode(), *s, ctypes.byref(ld))
            offs[f"{nm}@{_key(*s)}"] = [off, ld.value]
    out["workspace_offset"] = offs
    lib.vqs_destroy(h)
    return out


def dump_qwen(lib, name, x_pitch=None):
    from t2v_metrics_amd.qwen import engine as qe
    from t2v_metrics_amd.qwen.config import get_qwen_config
    for fn, (res, args) in qe._SIGS.items():
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, args
    cfg = get_qwen_config(name)
    v, t = cfg.vision, cfg.text
    mask = 0
    for i in v.fullatt_blocks:
        mask |= 1 << i
    c = qe.VqsQwenConfig(v.depth, v.hidden, v.heads, v.mlp, v.patch_dim, v.merge_unit, v.out_hidden, mask, v.rms_eps,
                         t.vocab, t.hidden, t.layers, t.heads, t.kv_heads, t.mlp, t.rms_eps)
    h = ctypes.c_void_p()
    assert lib.vqs_qwen_create(ctypes.byref(c), ctypes.byref(h)) == 0, name
    if x_pitch is not None:
        assert lib.vqs_qwen_debug_option(h, b"x_pitch", x_pitch) == 0, (name, x_pitch)
    out = {}
    for fp16 in (0, 1):          # the packed buffer holds the fp16 weight copies only when they are asked for
        if lib.vqs_qwen_debug_option(h, b"fp16", fp16) == 0:
            out[f"packed_bytes_fp16={fp16}"] = lib.vqs_qwen_packed_bytes(h)
    mu = v.merge_unit
    out["vision_workspace_bytes"] = {_key(N, Np): lib.vqs_qwen_vision_workspace_bytes(h, N, Np)
                                     for (N, Np) in ((mu, mu), (64 * mu, 64 * mu), (256 * mu, 320 * mu), (3072, 3072), (mu + 1, 2 * mu))}
    sl = [(B, 33) for B in BATCHES] + [(64, 808), (0, 33)]
    out["score_workspace_bytes"] = {_key(*s): lib.vqs_qwen_score_workspace_bytes(h, *s) for s in sl}
    out["kv_bytes"] = {_key(*s): lib.vqs_qwen_kv_bytes(h, *s) for s in ((1, 97), (4, 97), (256, 97), (64, 816), (0, 97))}
    out["decode_workspace_bytes"] = {_key(B): lib.vqs_qwen_decode_workspace_bytes(h, B) for B in BATCHES + (64, 0)}
    pl = ((8, 768), (1, 32), (8, 40))
    out["prefix_kv_bytes"] = {_key(*s): lib.vqs_qwen_prefix_kv_bytes(h, *s) for s in pl}
    out["prefix_workspace_bytes"] = {_key(*s): lib.vqs_qwen_prefix_workspace_bytes(h, *s) for s in pl}
    out["suffix_workspace_bytes"] = {_key(*s): lib.vqs_qwen_suffix_workspace_bytes(h, *s)
                                     for s in ((64, 768, 40), (1, 768, 8), (4, 32, 33), (256, 768, 40), (4, 768, 7))}
    lib.vqs_qwen_destroy(h)
    return out


def dump_clip(lib, name):
    from t2v_metrics_amd.clip.config import get_clip_config
    from t2v_metrics_amd.clip.engine import _SIGS, make_clip_config
    for fn, (res, args) in _SIGS.items():
        f = getattr(lib, fn)
        f.restype, f.argtypes = res, args
    c = make_clip_config(get_clip_config(name))
    h = ctypes.c_void_p()
    assert lib.vqs_clip_create(ctypes.byref(c), ctypes.byref(h)) == 0, name
    out = {"packed_bytes": lib.vqs_clip_packed_bytes(h)}
    out["image_workspace_bytes"] = {_key(n): lib.vqs_clip_image_workspace_bytes(h, n) for n in BATCHES + (0,)}
    out["text_workspace_bytes"] = {_key(n, L): lib.vqs_clip_text_workspace_bytes(h, n, L) for n in BATCHES for L in (8, 33, 77, 7)}
    lib.vqs_clip_destroy(h)
    return out


def dump(lib_path=None):
    from t2v_metrics_amd.engine import load_library
    lib = load_library(lib_path)
    out = {"clip_t5": {n: dump_clip_t5(lib, n) for n in ("tiny", "small", "clip-flant5-xl", "clip-flant5-xxl")}}
    out["qwen"] = {"qwen-tiny": dump_qwen(lib, "qwen-tiny"), "qwen-small": dump_qwen(lib, "qwen-small"),
                   "qwen2.5-vl-7b": dump_qwen(lib, "qwen2.5-vl-7b"),
                   "qwen2.5-vl-7b,x_pitch=4096": dump_qwen(lib, "qwen2.5-vl-7b", 4096),
                   "qwen2.5-vl-7b,x_pitch=3584": dump_qwen(lib, "qwen2.5-vl-7b", 3584)}
    out["clip"] = {n: dump_clip(lib, n) for n in ("openai:ViT-L-14", "openai:ViT-L-14-336")}
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=None, help="library to query (default: the package's own t2v_metrics_amd/libvqs_hip.so)")
    a = ap.parse_args()
    json.dump(dump(a.lib), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
