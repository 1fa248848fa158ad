#!/usr/bin/env python3
"""VQAScore throughput bench (driver contract: one JSON line on rank 0).

Default workload = the configuration BASELINE.json's metric is quoted on: clip-flant5-XXL, bf16, one batch of 256
(image, text) pairs per GPU per step, synthetic 224x224 uint8 images (bicubic-resized to the tower's 336x336 and
CLIP-normalised once, outside the timed region, pixels resident in HBM as bf16) + 32-position prompts (8 prefix ids,
the image sentinel, 24 suffix ids => encoder length 576 + 32 = 608), labels [2163, 1] (T = 2) -- SURVEY.md §8d
"Config 2" generator at the XXL size.  Distinct image per pair (no ViT reuse).  Weights: seeded random at the exact
architecture (no checkpoint offline).  `--model clip-flant5-xl` is BASELINE.json configs[1].

A "step" = one full scoring pass over one batch: ViT-L/14-336 (23 layers) + projector + T5 encoder (24) + 2-row
teacher-forced decoder (24) + lm_head + log-softmax/score.

Other workloads (whole-job runs; --steps is then derived from the job):
  --workload genai1600   BASELINE.json configs[2] stand-in (the real prompt file is fetched at run time by the reference,
                         dataset.py:1247-1281, unreachable offline): 1 600 prompts x 6 images = 9 600 pairs
                         (dataset.py:1226,1235), caption lengths uniform 8-40 tokens (seed 1600) => encoder lengths
                         616-648; pairs are sorted by prompt length into batches of --batch (no padding waste), scores
                         scattered back to input order inside the timed region.
  --pairs N              BASELINE.json configs[3]: N pairs in total (100 000 in the config), inputs a function of the
                         GLOBAL pair block index (so sharding does not change them), contiguous blocks per rank.

N > 1: one process per GPU.  `python bench.py --gpus N` launches its own ranks (re-executes itself under
torch.distributed.run on 127.0.0.1); under an existing launcher (RANK/WORLD_SIZE set) it just joins.  Ranks are
independent replicas over disjoint pairs (weak scaling by default: per-GPU work fixed), no data-path collective, ONE RCCL
all_gather of the fp32 scores at the end of the timed region.

Extra objects:
  roofline     -- dominant kernel family = vqs::gemm_bf16_* : algorithmic GEMM FLOPs (2*M*N*K per launch) over the summed
                  per-launch durations measured with HIP events on the launch stream during the timed region
                  (vqs_profile_*), against the 2.5 PFLOP/s dense bf16 MFMA peak; `traffic` from the committed
                  rocprofv3 --pmc passes over this same command (profiles/gemm_traffic_<model>_b<batch>.json).
  cpu_baseline -- (--full only) the reference's own arithmetic (HF CLIPVisionModel + T5ForConditionalGeneration cast to
                  bf16 as mm_utils.py:228 does, oracle/hf_reference.py) timed on the host cores: 1 warm-up + 3 repetitions
                  on the first pair(s) of the same batch (rank 0, N = 1 only), the fp32 port beside it, and the three-way
                  |delta log P| table BASELINE.md §3 prescribes.
  also         -- (--full only) short legs of the other BASELINE configurations, each in its own process.

A plain run (no --full) sets up, warms up, times the steps and prints its line; --dump-outputs DIR also writes the last
timed step's outputs (label log-probs, scores) as DIR/<name>.npy, float32, from the same seeded inputs every run.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import socket
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from t2v_metrics_amd.config import get_config  # noqa: E402
from t2v_metrics_amd.sharding import shard_range  # noqa: E402
from t2v_metrics_amd.weights import make_seeded_weights  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0     # dense; /opt/skills/guides/MI355X_MICROARCH.md "Peak BF16/FP16 MFMA"
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)
METRIC = "image-text pairs scored/sec (whole node), "


def synth_pixels(cfg, n, gen, device):
    """seeded 224x224 uint8 images -> bicubic 336 -> CLIP-normalised bf16 [n,3,336,336] on `device` (a4+a5 of SURVEY §8)."""
    out = []
    for s in range(0, n, 256):
        m = min(256, n - s)
        img = torch.randint(0, 256, (m, 224, 224, 3), generator=gen, dtype=torch.uint8)
        x = img.to(device).permute(0, 3, 1, 2).float()
        x = torch.nn.functional.interpolate(x, size=(cfg.vision.image, cfg.vision.image), mode="bicubic", align_corners=False)
        x = x.clamp(0, 255) / 255.0
        mean = torch.tensor(CLIP_MEAN, device=device).view(1, 3, 1, 1)
        std = torch.tensor(CLIP_STD, device=device).view(1, 3, 1, 1)
        out.append(((x - mean) / std).to(torch.bfloat16))
    return torch.cat(out).contiguous()


def synth_prompts(cfg, n, gen, cap_len=None):
    """int32 ids [n, L]: 8 prefix ids (last = 1) + sentinel -200 + [caption of cap_len[i] ids] + 24 suffix ids (last = 1),
    right-padded with 0 to the longest row.  cap_len None = SURVEY §8d config 2 (L = 33, no caption, no padding)."""
    hi = min(32100, cfg.t5.vocab)
    pre = torch.randint(3, hi, (n, 8), generator=gen)
    pre[:, 7] = 1
    suf = torch.randint(3, hi, (n, 24), generator=gen)
    suf[:, 23] = 1
    sent = torch.full((n, 1), -200)
    if cap_len is None:
        return torch.cat([pre, sent, suf], dim=1).to(torch.int32)
    width = 33 + int(cap_len.max())
    ids = torch.zeros(n, width, dtype=torch.int64)
    cap = torch.randint(3, hi, (n, int(cap_len.max())), generator=gen)
    for i in range(n):
        c = int(cap_len[i])
        row = torch.cat([pre[i], sent[i], cap[i, :c], suf[i]])
        ids[i, : row.numel()] = row
    return ids.to(torch.int32)


def synth_batch(cfg, batch, seed, device, ragged=False):
    """SURVEY.md §8d "Config 2" generator (one batch); ragged=True draws a caption of 8-40 tokens per pair."""
    g = torch.Generator().manual_seed(seed)
    pixels = synth_pixels(cfg, batch, g, device)
    cap_len = torch.randint(8, 41, (batch,), generator=g) if ragged else None
    ids = synth_prompts(cfg, batch, g, cap_len)
    labels = torch.tensor([[min(2163, cfg.t5.vocab - 1), 1]] * batch, dtype=torch.int32)
    return pixels, torch.arange(batch, dtype=torch.int32).to(device), ids.to(device), labels.to(device)


def csrc_hash():
    """sha256 over the kernel sources: stamps PMC-derived numbers (profiles/gemm_traffic_*.json) with the code they were measured
    on -- the GPU box has no .git, so a commit id cannot be checked there."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "t2v_metrics_amd", "csrc")
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".inc", ".h", ".cpp")):
            with open(os.path.join(d, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read())
    return h.hexdigest()[:16]


def device_code_hash(path=None):
    """sha256 over the `.hip_fatbin` section of the shipped library = the device code the process actually runs.  The stronger of the
    two stamps: it survives edits that do not change the shipped kernels (comments, host code, `-DVQS_LAB`-only blocks; the build is
    deterministic -- a comment-only edit of gemm_quad.inc rebuilds to the same section) and changes with anything that does, the
    compiler included.  None if the library or the section is missing."""
    import hashlib
    import struct
    path = path or os.path.join(ROOT, "t2v_metrics_amd", "libvqs_hip.so")
    try:
        with open(path, "rb") as f:
            b = f.read()
        if b[:4] != b"\x7fELF" or b[4] != 2:
            return None
        shoff = struct.unpack_from("<Q", b, 0x28)[0]
        shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)

        def sh(i):
            name, _typ, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", b, shoff + i * shentsize)
            return name, off, size
        _, stroff, strsize = sh(shstrndx)
        names = b[stroff: stroff + strsize]
        for i in range(shnum):
            n, off, size = sh(i)
            if names[n: names.index(b"\0", n)] == b".hip_fatbin":
                return hashlib.sha256(b[off: off + size]).hexdigest()[:16]
    except Exception:
        return None
    return None


def _fatbin_section(path):
    import struct
    with open(path, "rb") as f:
        b = f.read()
    if b[:4] != b"\x7fELF" or b[4] != 2:
        return None
    shoff = struct.unpack_from("<Q", b, 0x28)[0]
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", b, 0x3A)

    def sh(i):
        name, _typ, _flags, _addr, off, size = struct.unpack_from("<IIQQQQ", b, shoff + i * shentsize)
        return name, off, size
    _, stroff, strsize = sh(shstrndx)
    names = b[stroff: stroff + strsize]
    for i in range(shnum):
        n, off, size = sh(i)
        if names[n: names.index(b"\0", n)] == b".hip_fatbin":
            return b[off: off + size]
    return None


def device_kernels(path=None):
    """{kernel symbol: (machine code bytes, kernel descriptor bytes)} of every kernel in the gfx950 code objects of the shipped library:
    the `.hip_fatbin` section is a sequence of clang offload bundles (one per translation unit), each holding one amdgcn ELF whose
    symbol table names a FUNC symbol `<kernel>` in .text and an OBJECT symbol `<kernel>.kd` (64-byte descriptor: register counts, LDS
    size, ...) in .rodata."""
    import struct
    path = path or os.path.join(ROOT, "t2v_metrics_amd", "libvqs_hip.so")
    fb = _fatbin_section(path)
    if fb is None:
        return {}
    out = {}
    magic, at = b"__CLANG_OFFLOAD_BUNDLE__", 0
    while True:
        at = fb.find(magic, at)
        if at < 0:
            break
        n_entries = struct.unpack_from("<Q", fb, at + 24)[0]
        q = at + 32
        for _ in range(n_entries):
            off, size, tl = struct.unpack_from("<QQQ", fb, q)
            triple = fb[q + 24: q + 24 + tl]
            q += 24 + tl
            if b"amdgcn" not in triple or size == 0:
                continue
            e = fb[at + off: at + off + size]
            if e[:4] != b"\x7fELF":
                continue
            shoff = struct.unpack_from("<Q", e, 0x28)[0]
            shentsize, shnum, _ = struct.unpack_from("<HHH", e, 0x3A)
            secs = [struct.unpack_from("<IIQQQQII", e, shoff + i * shentsize) for i in range(shnum)]   # name type flags addr off size link info
            for (_n, typ, _f, _a, soff, ssize, link, _i) in secs:
                if typ != 2:                                   # SHT_SYMTAB
                    continue
                stab = secs[link]
                strs = e[stab[4]: stab[4] + stab[5]]
                syms = {}
                for k in range(ssize // 24):
                    st_name, st_info, _o, st_shndx, st_value, st_size = struct.unpack_from("<IBBHQQ", e, soff + 24 * k)
                    if st_shndx == 0 or st_shndx >= shnum or st_size == 0:
                        continue
                    name = strs[st_name: strs.index(b"\0", st_name)].decode()
                    sec = secs[st_shndx]
                    lo = sec[4] + (st_value - sec[3])
                    syms[name] = e[lo: lo + st_size]
                for name, code in syms.items():
                    if name + ".kd" in syms:
                        out[name] = (code, syms[name + ".kd"])
        at += len(magic)
    return out


GEMM_KERNEL_PATTERNS = ("gemm_bf16_",)      # the record of round 4 was collected before the fp16 instantiations existed; newer records name theirs


def gemm_kernels_hash(path=None, patterns=GEMM_KERNEL_PATTERNS):
    """sha256 over the machine code and the kernel descriptors of every GEMM kernel of the shipped library (`vqs::gemm_bf16_*`, the launches
    `roofline.traffic` was measured on; `patterns`: which symbols count -- a record made with the fp16 tower in the step names
    ("gemm_bf16_", "gemm_f16_")), by sorted symbol name.  Finer than device_code_hash(): it does not change when OTHER kernels are
    added to or edited in the library, and changes with any instruction or register count of a GEMM kernel.  None without the library."""
    import hashlib
    ks = {n: v for n, v in device_kernels(path).items() if any(p in n for p in patterns)}
    if not ks:
        return None
    h = hashlib.sha256()
    for n in sorted(ks):
        code, kd = ks[n]
        kd = kd[:16] + b"\0" * 8 + kd[24:]          # kernel_code_entry_byte_offset: where the linker put the code, not what it is
        h.update(n.encode() + b"\0" + code + b"\0" + kd)
    return h.hexdigest()[:16]


# The execution options that decide which 16-bit type a stage computes in (include/vqs.h): option -> (stage, what is fp16 when it is on).  The
# bench line's `dtype`, `config.workload` label and `config.arithmetic` are all built from THIS table and the engine's current option values.
ARITHMETIC_OPTIONS = (
    ("vit_fp16", "vision tower", "norm outputs, q / k / v, probabilities, attention output, sub-layer outputs, FFN product; every linear's weights"),
    ("proj_fp16", "feature select + projector", "hidden_states[-2] cast and the projector's hidden tensor (behind the bind-time scales proj_fs_shift / proj_mid_shift); its weights"),
    ("enc_fp16", "T5 encoder attention side", "both norm outputs, q / k / v, probabilities, attention output; q|k|v, o, wi weights (sub-layer outputs, FFN product, wo stay bf16)"),
    ("dec_fp16", "decoder cross-attention score path", "encoder output, cross q, q.Wk, probabilities"),
)


def describe_arithmetic(eng):
    """-> {"on": {option: bool}, "dtype", "label", "arithmetic"}: what the engine computes in, from its option values (engine doubles: all off)."""
    get = (lambda k: int(eng.get_option(k))) if hasattr(eng, "get_option") else (lambda k: 0)
    on = {k: bool(get(k)) for k, _, _ in ARITHMETIC_OPTIONS}
    on["proj_fp16"] = on["proj_fp16"] and on["vit_fp16"]
    on["dec_fp16"] = on["dec_fp16"] and bool(get("dec_precise")) and bool(get("cross_mode"))
    enc_mode = get("enc_fp16")
    fp16_stages = [stage + (" (attention sub-block only)" if k == "enc_fp16" and enc_mode == 2 else " (FFN input side only)" if k == "enc_fp16" and enc_mode == 3 else "")
                   for k, stage, _ in ARITHMETIC_OPTIONS if on[k]]
    label = "bf16 + fp16 (" + ", ".join(fp16_stages) + ")" if fp16_stages else "bf16"
    dtype = ("bf16 (T5 GEMM operands elsewhere; decoder activations split-bf16 / fp32)" + (" + IEEE fp16 (" + "; ".join(fp16_stages) + ")" if fp16_stages else "")
             + ": 16-bit MFMA operands at one rate, fp32 accumulation, residual streams, statistics and softmax")
    arithmetic = "; ".join("%s: %s" % (stage, ("IEEE fp16 (option %s = %d): %s" % (k, get(k), what)) if on[k] else "bf16 (option %s = %d)" % (k, get(k)))
                           for k, stage, what in ARITHMETIC_OPTIONS)
    arithmetic += "; everything else: bf16 operands (the reference's dtype, mm_utils.py:228), decoder activations split-bf16 / fp32"
    return {"on": on, "dtype": dtype, "label": label, "arithmetic": arithmetic}


def traffic_stamp_matches(tj):
    """Is the PMC record `tj` (profiles/gemm_traffic_*.json) about the code this process runs?  The stamp of the GEMM kernels' machine
    code if the record has one, else the whole-library device-code stamp, else the source stamp of older records.  -> (bool, description)."""
    if tj.get("gemm_kernels_sha256_16"):       # the measured kernels themselves (survives additions of other kernels to the library)
        now = gemm_kernels_hash(patterns=tuple(tj.get("gemm_kernels_patterns") or GEMM_KERNEL_PATTERNS))
        return tj["gemm_kernels_sha256_16"] == now, "GEMM kernels' code sha256 %s (now %s)" % (tj["gemm_kernels_sha256_16"], now)
    if tj.get("device_code_sha256_16"):
        now = device_code_hash()
        return tj["device_code_sha256_16"] == now, "device code sha256 %s (now %s)" % (tj["device_code_sha256_16"], now)
    now = csrc_hash()
    return tj.get("csrc_sha256_16") == now, "csrc sha256 %s (now %s)" % (tj.get("csrc_sha256_16"), now)


ALSO_LEGS = {
    # name: (argv after the interpreter, what BASELINE.json config it is)
    "xl": (["bench.py", "--full", "--model", "clip-flant5-xl", "--steps", "5", "--warmup", "2", "--cpu-pairs", "0", "--also", "none", "--parity-only", "32"],
           "configs[1]: clip-flant5-xl bf16, batch=256 synthetic 224x224 + 32-tok prompts; + its own 32-pair |delta log P| table"),
    "genai1600": (["bench.py", "--full", "--workload", "genai1600", "--buckets", "6", "--warmup", "1", "--cpu-pairs", "0", "--also", "none", "--parity-only", "32"],
                  "configs[2]: clip-flant5-xxl, GenAI-Bench-1600 stand-in, 6 of its 38 length buckets; + a 32-pair |delta log P| table over its "
                  "shortest and longest batch (ragged prompts, padded and masked)"),
    "qwen": (["bench.py", "--full", "--model", "qwen2.5-vl-7b", "--steps", "3", "--warmup", "1", "--cpu-pairs", "0", "--also", "none", "--parity-only", "32"],
             "configs[4]: qwen2.5-vl-7b, 8-frame video samples (range-safe fp16 forms + precise tail); + |delta log P(answer)| of 32 samples against the fp32 "
             "oracle evaluated on the device, held to the 1e-3 bound (exit 3)"),
    "bf16_operands": (["bench.py", "--full", "--steps", "3", "--warmup", "1", "--cpu-pairs", "0", "--also", "none", "--opt", "vit_fp16=0", "--opt", "enc_fp16=0", "--opt", "dec_fp16=0", "--parity-only", "32"],
                      "INFORMATIONAL, allowed to exceed the bound: the headline configuration with every 16-bit tensor of the vision tower and the T5 encoder "
                      "in bf16 (options vit_fp16 = 0, enc_fp16 = 0, dec_fp16 = 0: the reference's dtype, mm_utils.py:228; rounds 1-3's arithmetic there) -- throughput and "
                      "the 32-pair |delta log P| table next to the main line's fp16 forms"),
    "pipeline": (["tools/bench_pipeline.py", "--model", "clip-flant5-xxl", "--pairs", "1280", "--reps", "1", "--host-slice", "8"],
                 "SURVEY 8f-1: VQAScoreModel.forward from 512x512 PNG files (decode, preprocessing, H2D, tokenisation, engine) on 1/8 of the "
                 "host's cores -- a rank's share at 8 GPUs per node"),
}


def run_also_leg(name):
    """One short extra leg in its own process (its own engine and workspaces; a failure cannot take the main line down)."""
    import subprocess
    argv, what = ALSO_LEGS[name]
    t0 = time.perf_counter()
    try:
        r = subprocess.run([sys.executable] + [os.path.join(ROOT, argv[0])] + argv[1:], capture_output=True, text=True, timeout=420,
                           env={k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")})
        line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")][-1]
        j = json.loads(line)
    except Exception as e:                                  # noqa: BLE001 -- reported, not raised
        return {"what": what, "error": repr(e)[:300], "wall_s": round(time.perf_counter() - t0, 1)}
    out = {"what": what, "value": j.get("value"), "unit": j.get("unit", "pairs/s"), "wall_s": round(time.perf_counter() - t0, 1)}
    for k in ("ms_per_step", "steps", "metric"):
        if k in j:
            out[k] = j[k]
    if isinstance(j.get("config"), dict):
        out["workload"] = j["config"].get("workload")
    if isinstance(j.get("roofline"), dict):
        out["roofline_frac"] = j["roofline"].get("frac")
        out["roofline_achieved_tflops"] = j["roofline"].get("achieved")
    if isinstance(j.get("decode"), dict):
        out["decode_ms_per_step"] = j["decode"].get("ms_per_step")
        out["decode_tokens_per_s"] = j["decode"].get("tokens_per_s")
    if isinstance(j.get("parity"), dict) and isinstance(j["parity"].get("gains"), dict):
        out["dlogp_hip_vs_fp32_truth"] = {g: {k: v.get(k) for k in ("max", "mean", "yes_token_max", "pairs_over_bound", "per_job")} for g, v in j["parity"]["gains"].items()}
        out["dlogp_pairs"] = j["parity"].get("pairs")
        out["dlogp_max"] = j["parity"]["gains"].get("1", {}).get("max")            # gain 1 = the model as seeded: the number the bound is about
        out["dlogp_gain4_max"] = j["parity"]["gains"].get("4", {}).get("max")      # the peaked regime, held to DLOGP_BOUND_GAIN4
        out["dlogp_bound"] = j["parity"].get("bound")
        out["dlogp_encoder_len_range"] = j["parity"].get("encoder_len_range")
        if j["parity"].get("status"):
            out["dlogp_status"] = j["parity"]["status"]
    elif isinstance(j.get("parity"), dict):
        out["dlogp_error"] = j["parity"].get("error")
    for k in ("model_frac_of_mfma_peak", "host_preprocess_256_images_s", "workers", "pairs", "png_edge", "image_workers", "host_threads_allowed",
              "engine_only_same_inputs_pairs_per_s", "ratio_to_engine_only_same_inputs", "encoder_len_first_batch"):
        if k in j:
            out[k] = j[k]
    return out


def length_buckets(lengths: torch.Tensor, batch: int):
    """Sort pair indices by prompt length (stable) and cut into batches: every batch is padded only to ITS longest
    prompt.  Returns a list of index tensors; concatenated they are a permutation of range(n)."""
    order = torch.argsort(lengths, stable=True)
    return [order[s: s + batch] for s in range(0, order.numel(), batch)]


def make_jobs(args, cfg, rank, world, device):
    """-> (jobs, info): jobs = [(pixels, img_index, ids, labels, dest_index or None)], one per step of this rank."""
    B = args.batch
    yes = [[min(2163, cfg.t5.vocab - 1), 1]]
    if args.workload == "genai1600":
        n_prompts, per = 1600, 6
        g = torch.Generator().manual_seed(1600)
        cap_prompt = torch.randint(8, 41, (n_prompts,), generator=g)
        ids_prompt = synth_prompts(cfg, n_prompts, g, cap_prompt)
        pair_prompt = torch.arange(n_prompts).repeat_interleave(per)          # pair i = prompt i // 6, image i % 6
        n = n_prompts * per
        buckets = length_buckets(cap_prompt[pair_prompt], B)
        if getattr(args, "buckets", 0) and args.buckets < len(buckets):     # a short leg: evenly spaced over the sorted lengths
            pick = sorted({round(i * (len(buckets) - 1) / max(args.buckets - 1, 1)) for i in range(args.buckets)})
            buckets = [buckets[i] for i in pick]
            n = sum(b.numel() for b in buckets)
        subset = n != n_prompts * per
        starts = [0]
        for b in buckets:
            starts.append(starts[-1] + b.numel())
        lo, hi = shard_range(len(buckets), rank, world)
        jobs = []
        for bi in range(lo, hi):
            idx = buckets[bi]
            gi = torch.Generator().manual_seed(16000 + bi)                   # images: a function of the bucket index
            ids = ids_prompt[pair_prompt[idx]]
            L = int((ids != 0).sum(1).max())
            jobs.append((synth_pixels(cfg, idx.numel(), gi, device), torch.arange(idx.numel(), dtype=torch.int32, device=device),
                         ids[:, :L].contiguous().to(device), torch.tensor(yes * idx.numel(), dtype=torch.int32, device=device),
                         (torch.arange(starts[bi], starts[bi + 1]) if subset else idx).to(device)))
        return jobs, {"total_pairs": n, "name": f"GenAI-Bench-1600 stand-in: 1600 prompts x 6 images = 9600 pairs, caption 8-40 tok "
                      f"(S_e 616-648), length-bucketed into batches of {B}" + (f"; {len(buckets)} of the 38 buckets, evenly spaced over the lengths" if subset else ""),
                      "scaling": "strong"}
    if args.pairs > 0:
        n = args.pairs
        nblocks = (n + B - 1) // B
        lo, hi = shard_range(nblocks, rank, world)
        jobs = []
        for bi in range(lo, hi):
            m = min(B, n - bi * B)
            px, ii, ids, lab = synth_batch(cfg, m, seed=1234 + bi, device=device)     # seed per GLOBAL block index
            jobs.append((px, ii, ids, lab, torch.arange(bi * B, bi * B + m, device=device)))
        return jobs, {"total_pairs": n, "name": f"{n} synthetic pairs in total (config-2 generator per global block of {B}), "
                      f"contiguous blocks per rank", "scaling": "strong"}
    px, ii, ids, lab = synth_batch(cfg, B, seed=1234 + rank, device=device, ragged=args.ragged)
    return [(px, ii, ids, lab, None)] * args.steps, {
        "total_pairs": B * args.steps * world, "scaling": "weak",
        "name": f"batch={B} synthetic 224x224 + " + ("ragged 41-73-tok prompts (padded, masked)" if args.ragged else "32-tok prompts")
                + " per GPU per step"}


def free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--model", default="clip-flant5-xxl", help="clip-flant5-xxl (the metric's model) | clip-flant5-xl | qwen2.5-vl-7b")
    ap.add_argument("--batch", type=int, default=256, help="pairs per GPU per step")
    ap.add_argument("--workload", default="synthetic", choices=["synthetic", "genai1600"])
    ap.add_argument("--pairs", type=int, default=0, help="fixed total number of pairs over all ranks (BASELINE configs[3]: 100000)")
    ap.add_argument("--full", action="store_true", help="everything beyond the headline figure as well: the cpu_baseline leg with its |delta log P| "
                    "tables (--cpu-pairs defaults to 4) and the extra legs (--also defaults to auto); a plain run only sets up, warms up, "
                    "times the steps and prints its line")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR", help="after the timed steps, write what the last step computed "
                    "(label log-probs and scores of this rank's batch) as DIR/<name>.npy in float32")
    ap.add_argument("--cpu-pairs", type=int, default=None, help="pairs in the CPU reference sample (BASELINE.md section 3: 4 at XXL; 0 = skip the "
                    "cpu_baseline leg); default 4 with --full, 0 without")
    ap.add_argument("--also", default=None, help="extra short legs reported under \"also\" (the other BASELINE configs): comma list of "
                    "xl,genai1600,qwen,pipeline,config0; auto = all of them for the default single-GPU XXL run, none otherwise; none = off; "
                    "default auto with --full, none without")
    ap.add_argument("--buckets", type=int, default=0, help="genai1600: time only this many length buckets, evenly spaced over the sorted workload (0 = all 38)")
    ap.add_argument("--cpu-emulation", action="store_true", help="also run the rounding-matched CPU oracle on pair 0 (~40 s at XXL)")
    ap.add_argument("--cpu-reps", type=int, default=3, help="timed repetitions of the CPU reference after 1 warm-up (BASELINE.md section 3: >= 3; a 4-pair XXL pass is ~50 s)")
    ap.add_argument("--parity-pairs", type=int, default=64, help="pairs of the |delta log P| table (HIP vs fp32 truth, head gains 1 and 4)")
    ap.add_argument("--parity-only", type=int, default=0, metavar="N", help="report the N-pair |delta log P| table (device-evaluated fp32 truth) without the CPU "
                    "reference leg: used by the also-leg that runs the bf16 tower")
    ap.add_argument("--ragged", action="store_true", help="one batch of variable-length prompts, padded + masked (no bucketing)")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="execution-form option of include/vqs.h vqs_set_option (e.g. gemm_variant=6, tile_order:20480x4096=520); "
                         "every form computes the same function -- for A/B runs, recorded in config.options")
    args = ap.parse_args(argv)
    if args.cpu_pairs is None:
        args.cpu_pairs = 4 if args.full else 0
    if args.also is None:
        args.also = "auto" if args.full else "none"
    return args


DUMP_LIMIT_BYTES = 64 << 20


def write_outputs(out_dir, arrays, limit=DUMP_LIMIT_BYTES):
    """arrays: {name: tensor} -> out_dir/<name>.npy, float32 (float64 kept).  Above `limit` bytes in all, every array is cut to the
    same fixed, seeded sample of its flattened elements (the positions depend only on its size), so two runs stay comparable."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    host = {}
    for name, t in arrays.items():
        a = t.detach().cpu()
        host[name] = a.double().numpy() if a.dtype == torch.float64 else a.float().numpy()
    total = sum(a.nbytes for a in host.values())
    for name, a in host.items():
        if total > limit:
            keep = max(1, int(a.size * limit / total))
            pos = np.sort(np.random.default_rng(0).choice(a.size, size=keep, replace=False))
            a = a.reshape(-1)[pos]
        np.save(os.path.join(out_dir, name + ".npy"), np.ascontiguousarray(a))


def main():
    args = parse_args()

    if args.model.startswith("qwen"):
        # BASELINE.json configs[4] (Qwen2.5-VL-7B, 8-frame video): measured by tools/bench_qwen.py, one GPU
        if args.gpus != 1:
            raise SystemExit("the Qwen2.5-VL bench line is single-GPU (replicas need no collective: run one process per GPU)")
        sys.argv = [os.path.join(ROOT, "tools", "bench_qwen.py"), "--model", args.model, "--steps", str(args.steps), "--warmup",
                    str(args.warmup), "--batch", str(min(args.batch, 64)), "--cpu-samples", str(min(args.cpu_pairs, 1)),
                    "--decode-steps", "16" if args.full else "0",   # --full: + the cached decode step (generation beyond the first token), under "decode"
                    "--parity-samples", str(max(args.parity_only, 0))]
        if args.dump_outputs:
            sys.argv += ["--dump-outputs", args.dump_outputs]
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_qwen
        return bench_qwen.main()

    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # plain `python bench.py --gpus N`: launch the ranks as child processes -- one rank per GPU, rendezvous on 127.0.0.1
        import subprocess
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        sys.exit(subprocess.call(cmd))

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}")
    # Harness self-test hook (tests/test_bench_harness.py): VQS_BENCH_ENGINE_DOUBLE="module:Class" swaps the HIP engine
    # for a test double so the launcher / sharding / gather / JSON logic runs on a box without GPUs.  Never set by the
    # driver; the line it produces is labelled as not-a-measurement.
    double = os.environ.get("VQS_BENCH_ENGINE_DOUBLE")
    if not double and not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    # VQS_BENCH_BACKEND=gloo lets the N > 1 code path be exercised on a box with fewer GPUs than ranks (ranks share
    # devices, collectives go through host memory); the driver's runs use the default: nccl = RCCL, one GPU per rank.
    backend = "gloo" if double else os.environ.get("VQS_BENCH_BACKEND", "nccl")
    if double:
        device = coll_device = torch.device("cpu")
    else:
        dev_index = local_rank if backend == "nccl" else local_rank % torch.cuda.device_count()
        torch.cuda.set_device(dev_index)
        device = torch.device("cuda", dev_index)
        coll_device = device if backend == "nccl" else torch.device("cpu")
    dist = None
    # VQS_BENCH_FORCE_DIST=1: take the multi-rank branch with ONE rank -- init_process_group("nccl", device_id=...), the device-side
    # all_gather / all_reduce / barrier and destroy_process_group run on a single MI355X (tests/test_gpu_rccl_single_rank.py); the
    # 1/2/4/8-GPU curve itself is the driver's to measure.
    force_dist = os.environ.get("VQS_BENCH_FORCE_DIST") == "1" and not double
    if world > 1 or force_dist:
        import torch.distributed as dist_mod
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if world == 1:
            os.environ.setdefault("MASTER_PORT", str(free_port()))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        # one rank per GPU: keep the rank's host threads on the cores next to its device (first touch of pinned buffers, the image
        # thread pool): cores are split evenly by local rank unless the launcher already restricted the affinity
        # (t2v_metrics_amd/sharding.py: the cores of the NUMA node the rank's GPU hangs off, shared evenly by the ranks of that node;
        # an equal split of the allowed cores when the topology is unknown)
        from t2v_metrics_amd.sharding import set_rank_affinity
        if os.environ.get("VQS_BENCH_NO_AFFINITY") != "1" and not double:
            set_rank_affinity(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", str(world))))
        if backend == "nccl":
            dist_mod.init_process_group(backend="nccl", device_id=device)
        else:
            dist_mod.init_process_group(backend=backend)
        dist = dist_mod

    cfg = get_config(args.model)
    if double:
        mod, cls = double.split(":")
        eng = getattr(importlib.import_module(mod), cls)(cfg)
        weights = None
    else:
        from t2v_metrics_amd.engine import VqsEngine
        weights = make_seeded_weights(cfg, seed=0, device=device)
        options = {}
        for item in args.opt:
            name, _, value = item.partition("=")
            options[name] = int(value)
        eng = VqsEngine(cfg, weights, device=device, options=options)
    B = args.batch
    jobs, info = make_jobs(args, cfg, rank, world, device)
    steps_local = len(jobs)
    T = jobs[0][3].shape[1] if jobs else 2

    def run(job):
        pixels, img_index, ids, labels, _ = job
        return eng.score(eng.encode_images(pixels), img_index, ids, labels)

    def barrier():
        if dist is not None:
            dist.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()

    if jobs:
        longest = max(jobs, key=lambda j: j[2].shape[1] * j[2].shape[0])   # sizes the workspaces once, outside the timed region
        for _ in range(max(args.warmup, 1)):
            run(longest)
    barrier()
    eng.profile(True)
    eng.profile_read(reset=True)
    t0 = time.perf_counter()
    n_total = info["total_pairs"]
    ordered = info["scaling"] == "strong"
    local = torch.zeros(n_total if ordered else steps_local * B, device=device)
    lp = None
    # per-step device time (HIP events on the launch stream, recorded without synchronising; read after the closing barrier): shows
    # whether a long run drifts -- sustained board power -- or the box is simply slower
    step_ev = [torch.cuda.Event(enable_timing=True) for _ in range(len(jobs) + 1)] if device.type == "cuda" else None
    if step_ev:
        step_ev[0].record()
    for si, job in enumerate(jobs):
        lp, sc = run(job)
        if step_ev:
            step_ev[si + 1].record()
        if ordered:
            local[job[4]] = sc                     # scatter back to input order (other ranks' slots stay 0)
        else:
            local[si * B: si * B + sc.numel()] = sc
    ranks_seen = 1
    if dist is not None:
        local_c = local.to(coll_device)
        gathered = [torch.empty_like(local_c) for _ in range(world)]
        dist.all_gather(gathered, local_c)          # the path's only exchange: scores to every rank
        ranks_seen = len(gathered)
        final = torch.stack(gathered).sum(0) if ordered else torch.cat(gathered)
    else:
        final = local
    barrier()
    elapsed_local = time.perf_counter() - t0
    if args.dump_outputs and rank == 0 and lp is not None:
        write_outputs(args.dump_outputs, {"label_logprobs": lp, "scores": sc})     # what the last timed step handed its caller
    step_ms = [round(step_ev[i].elapsed_time(step_ev[i + 1]), 2) for i in range(len(jobs))] if step_ev else None
    eng.profile(False)
    gemm_bytes = eng.profile_bytes()
    n_gemm, gemm_ms, gemm_flops = eng.profile_read(reset=True)
    if rank == 0 and os.environ.get("VQS_BENCH_REPORT"):
        print(eng.profile_report(), file=sys.stderr, flush=True)

    pairs_local = sum(j[2].shape[0] for j in jobs)
    t_el = torch.tensor([elapsed_local], device=coll_device, dtype=torch.float64)
    per_rank = torch.tensor([pairs_local / elapsed_local if elapsed_local > 0 else 0.0], device=coll_device, dtype=torch.float64)
    per_rank_list = [float(per_rank.item())]
    if dist is not None:
        dist.all_reduce(t_el, op=dist.ReduceOp.MAX)
        pr = [torch.empty_like(per_rank) for _ in range(world)]
        dist.all_gather(pr, per_rank)
        per_rank_list = [float(x.item()) for x in pr]
    # per-rank footprint (weights + packed copies incl. the fp16 ones + workspaces + inputs): what N replicas ask of N GPUs' HBM
    mem_local = float(torch.cuda.max_memory_allocated(device)) if device.type == "cuda" else 0.0
    mem_t = torch.tensor([mem_local], device=coll_device, dtype=torch.float64)
    mem_list = [mem_local]
    if dist is not None:
        mm = [torch.empty_like(mem_t) for _ in range(world)]
        dist.all_gather(mm, mem_t)
        mem_list = [float(x.item()) for x in mm]
    elapsed = float(t_el.item())
    total_pairs = n_total if ordered else pairs_local * world
    value = total_pairs / elapsed if elapsed > 0 and total_pairs > 0 else 0.0
    steps = max(steps_local, 1)
    if dist is not None:
        st = torch.tensor([steps_local], device=coll_device)
        dist.all_reduce(st, op=dist.ReduceOp.MAX)
        steps = max(int(st.item()), 1)

    # real (unpadded) encoder lengths: padding the engine computes over is not algorithmic work
    flops_sum, n_len = 0.0, 0
    seen = set()
    for j in jobs:
        if id(j[2]) in seen:
            continue
        seen.add(id(j[2]))
        lens = ((j[2] != 0).sum(1) - 1 + cfg.vision.n_patches).tolist()
        flops_sum += sum(cfg.flops_pair(int(l), T) for l in lens)
        n_len += len(lens)
    flops_pair = flops_sum / max(n_len, 1)
    s_e = (jobs[0][2].shape[1] - 1 + cfg.vision.n_patches) if jobs else 0
    arith = describe_arithmetic(eng)
    tower_fp16 = arith["on"].get("vit_fp16", False)
    out = {
        "metric": METRIC + cfg.name,
        "value": value,
        "unit": "pairs/s",
        "n_gpus": world,
        "steps": steps,
        "warmup": args.warmup,
        "ms_per_step": 1e3 * elapsed / steps,
        "higher_is_better": True,
        "scaling": info["scaling"],
        "vs_baseline": None,
        "dtype": arith["dtype"],
        "data": "synthetic (seeded 224x224 uint8 images resized to 336, seeded token ids, seeded random weights)"
                if not double else "ENGINE DOUBLE -- harness self-test, not a measurement",
        "config": {"workload": f"{cfg.name} {arith['label']}, {info['name']}",
                   "pairs_per_gpu_per_step": B, "encoder_len": s_e, "decoder_len": T, "total_pairs": total_pairs,
                   "parallelism": f"replica x{world} (pairs sharded, RCCL all_gather of scores)",
                   "arithmetic": arith["arithmetic"],
                   "fp16_options_switched_off_at_bind_time": getattr(eng, "fp16_auto_off", {}) or None,
                   **({"options": args.opt} if args.opt else {})},
        "ranks_seen": ranks_seen,
        "collective": (backend + (" (RCCL over xGMI)" if backend == "nccl" else "")) if dist is not None else None,
        "per_rank_pairs_per_s": per_rank_list,
        "per_rank_peak_hbm_gb": [round(x / 1e9, 3) for x in mem_list],
        "step_ms_rank0": step_ms,
        "scores_checksum": float(final.double().sum().item()),
        # FLOPs of the REFERENCE algorithm (SURVEY.md §8d formula).  The engine's reassociated decoder
        # cross-attention executes 4*S_e*D*I*layers fewer FLOPs per pair than that (same function);
        # "roofline" below is computed from the FLOPs the GEMM kernel really executed.
        "algorithmic_tflop_per_pair": flops_pair / 1e12,
        "executed_gemm_tflop_per_pair": (gemm_flops / max(pairs_local, 1)) / 1e12 if n_gemm > 0 else None,
        "model_tflops_per_gpu": value * flops_pair / 1e12 / world,
        "model_frac_of_mfma_peak": value * flops_pair / 1e12 / world / PEAK_BF16_TFLOPS,
    }
    if n_gemm > 0 and gemm_ms > 0:
        achieved = gemm_flops / (gemm_ms * 1e-3) / 1e12
        out["roofline"] = {"kernel": "vqs::gemm_bf16_quad / gemm_f16_quad / gemm_f16b_quad (16-bit-result launches: the same kernel on bf16 / fp16 fragments; dominant: "
                                     "gemm_f16b_quad<5>, the encoder's gated wi) + gemm_bf16_persistent / gemm_bf16_stream (fp32-result / batched): every GEMM launch of the step",
                           "bound": "mfma", "achieved": achieved,
                           "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s", "frac": achieved / PEAK_BF16_TFLOPS,
                           "traffic": None, "launches": n_gemm, "avg_launch_ms": gemm_ms / n_gemm,
                           "avg_launch_tflop": gemm_flops / n_gemm / 1e12,
                           "algorithmic_bytes_per_launch": gemm_bytes / n_gemm,
                           "gemm_share_of_step_time": gemm_ms * 1e-3 / elapsed_local}
        # HBM-side bytes per GEMM launch: PMC counters cannot be read from inside the process; they come from the
        # committed rocprofv3 --pmc passes over this same command (tools/gpu_pmc_bench.sh -> profiles/gemm_traffic_*.json)
        tpath = os.path.join(ROOT, "profiles", "gemm_traffic_%s_b%d.json" % (cfg.name.replace("clip-flant5-", ""), B))
        if os.path.exists(tpath) and args.workload == "synthetic" and args.pairs == 0 and not args.ragged:
            with open(tpath) as f:
                tj = json.load(f)
            # PMC counters cannot be read in-process: the number is valid only for the device code it was measured on
            same, how = traffic_stamp_matches(tj)
            if same:
                out["roofline"]["traffic"] = tj["traffic_bytes_per_launch"]
                out["roofline"]["traffic_unit"] = ("bytes per launch (fabric side, Infinity-Cache hits included: 2 x FETCH_SIZE + WRITE_SIZE), rocprofv3 --pmc passes over "
                                                   "this command on the same code, %s: profiles/%s" % (how, os.path.basename(tpath))
                                                   + ("; collected with the bf16 tower (vit_fp16 = 0) -- the fp16 tower's launches (94 of a step's 432) run the same kernel "
                                                      "on fp16 fragments: same tiles, same bytes" if tower_fp16 and not tj.get("vit_fp16") else ""))
            else:
                out["roofline"]["traffic_unit"] = "null: profiles/%s was measured on other code, %s" % (os.path.basename(tpath), how)

    default_run = (world == 1 and not double and args.model == "clip-flant5-xxl" and args.workload == "synthetic" and args.pairs == 0
                   and not args.ragged and not args.opt and B == 256)
    legs = [] if args.also == "none" else ([k for k in ("xl", "genai1600", "bf16_operands", "qwen", "pipeline", "config0")] if args.also == "auto" else args.also.split(","))
    if args.also == "auto" and not default_run:
        legs = []
    also, config0 = {}, None
    if rank == 0 and world == 1 and not double and legs:
        # Order matters for what each leg measures: the XL and GenAI legs are GPU-bound (a few hundred launches per step) and run in
        # their own processes WHILE the host cores time configs[0]; the Qwen leg (launch-bound on the host: 37.6 instead of 66 videos/s
        # next to a 128-thread CPU job, profiles/r3_call17_*) and the PNG pipeline (uses the host cores itself) run alone; the CPU
        # reference of the cpu_baseline leg runs last, alone.
        import threading
        phase_a = [k for k in legs if k in ("xl", "genai1600", "bf16_operands")]
        t_also = time.perf_counter()
        ALSO_WALL_S = 480.0            # the extra legs may not take the default run past "a few minutes" on a slow box: later legs are skipped, and say so

        def budget_left(k):
            if time.perf_counter() - t_also <= ALSO_WALL_S:
                return True
            also[k] = {"what": ALSO_LEGS[k][1], "skipped": "wall budget of the extra legs (%.0f s) spent" % ALSO_WALL_S}
            return False

        def run_phase_a():
            for k in phase_a:
                if budget_left(k):
                    also[k] = run_also_leg(k)
        th = threading.Thread(target=run_phase_a)
        th.start()
        if "config0" in legs and args.cpu_pairs > 0:
            config0 = run_config0()
        th.join()
        for k in ("qwen", "pipeline"):
            if k in legs and budget_left(k):
                also[k] = run_also_leg(k)

    failed = None
    if rank == 0 and world == 1 and args.cpu_pairs > 0 and not double and jobs:
        parity, truth_dev = None, None
        try:
            parity, truth_dev = parity_jobs(cfg, weights, eng, jobs, args.parity_pairs)
        except Exception as e:                           # noqa: BLE001 -- the table then falls back to the host-evaluated pairs
            parity_err = repr(e)[:300]
        out["cpu_baseline"] = cpu_baseline(cfg, weights, jobs[-1], min(args.cpu_pairs, jobs[-1][2].shape[0]), lp, args.cpu_reps,
                                           args.cpu_emulation, parity, truth_dev)
        if parity is None:
            out["cpu_baseline"]["dlogp"]["parity_sample_error"] = parity_err
        if config0 is not None:
            out["cpu_baseline"]["config0"] = config0
        failed = out["cpu_baseline"]["dlogp"].get("violation")
        # the other configurations' tables are held to the same bound -- since round 6 the Qwen row too (the informational bf16-operand leg
        # excepted); their maxima ride along as flat scalars
        for k, leg in also.items():
            if not isinstance(leg, dict) or leg.get("dlogp_max") is None:
                continue
            out["cpu_baseline"]["dlogp_also_%s_max" % k] = leg["dlogp_max"]
            if k in ("xl", "genai1600", "qwen") and leg["dlogp_max"] > DLOGP_BOUND and not failed:
                failed = "also.%s: max |dlogP| HIP vs fp32 truth %.3e > %.1e over %s pairs" % (k, leg["dlogp_max"], DLOGP_BOUND, leg.get("dlogp_pairs"))
            if k in ("xl", "genai1600") and (leg.get("dlogp_gain4_max") or 0.0) > DLOGP_BOUND_GAIN4 and not failed:
                failed = "also.%s: head gain 4: max |dlogP| HIP vs fp32 truth %.3e > %.1e over %s pairs" % (k, leg["dlogp_gain4_max"], DLOGP_BOUND_GAIN4, leg.get("dlogp_pairs"))
        out["cpu_baseline"]["dlogp"]["violation"] = out["cpu_baseline"]["dlogp_violation"] = failed
    if rank == 0 and world == 1 and args.parity_only > 0 and args.cpu_pairs <= 0 and not double and jobs:
        try:
            out["parity"], _ = parity_jobs(cfg, weights, eng, jobs, args.parity_only)
        except Exception as e:                           # noqa: BLE001 -- reported, not raised
            out["parity"] = {"error": repr(e)[:300]}
    if also:
        out["also"] = also

    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.destroy_process_group()
    if failed:
        print("bench.py: parity violation on the bench batch: " + failed, file=sys.stderr, flush=True)
        sys.exit(3)


def run_config0():
    """BASELINE configs[0] on THIS box's host cores: clip-flant5-xl, 4 images x 4 prompts, the reference's row loop (score.py:104-106:
    N-fold image work per row), HF modules in bf16 as mm_utils.py:228 casts them; one pass (a pass is ~60 s on 128 threads of the GPU
    box's 2 x EPYC 9575F -- slower than the 8-vCPU build container's 15.6 s: oneDNN's bf16 kernels do not scale over the sockets)."""
    try:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import config1_cpu
        t0 = time.perf_counter()
        c0 = config1_cpu.run("clip-flant5-xl", reps=0, dtypes=(torch.bfloat16,), verbose=False, api_pass=False)
        r = c0["runs"]["bf16 (reference as shipped)"]["reference_semantics"]
        return {"what": c0["config"] + "; HF modules in bf16 on this box's host cores, one cold pass; images: " + c0["images"],
                "value": r["pairs_per_s"], "unit": "pairs/s", "wall_s": r["wall_s_median_after_warmup"], "stages_s": r["stages_last_rep"],
                "cores": c0["torch_threads"], "host_cpus": c0["nproc"], "wall_s_incl_weights": round(time.perf_counter() - t0, 1)}
    except Exception as e:                                  # noqa: BLE001 -- reported, not raised
        return {"error": repr(e)[:300]}


PARITY_GAINS = (1.0, 4.0)          # lm_head x gain: 1 = the seeded head (log P ~ -10), 4 = the peaked-head regime (the head is linear: re-read)
DLOGP_BOUND_GAIN4 = 4e-3           # the PEAKED regime SURVEY.md section 7 asks about (lm_head x 4: logits four times as steep, so a given operand error moves log P four
                                   # times as far): gated at 4 x the bound -- the same relative accuracy of the logits.  Measured in round 6: 2.2e-3 over 256 pairs
DLOGP_BOUND = 1e-3                 # north_star's tolerance itself: max |delta log P| of the HIP path vs fp32 truth over the parity sample at gain 1
                                   # (>= 64 pairs of the bench batch; every `also` leg carries its own table and is held to the same number).
                                   # History: round 3's bf16 decoder measured 2.6e-3 .. 9.0e-3 (gate 2.5e-2), round 4 6.98e-4 over 16 pairs (gate 2.1e-3)
PARITY_CHUNK = 32                  # pairs per evaluation of the fp32 truth (bounds its [B, H, S, S] score tensors: 6 GB at XXL)


def parity_sample(cfg, weights, eng, job, n_pairs, rescore=True):
    """|delta log P| of the HIP path against fp32 truth on the first n_pairs pairs of `job`, at head gains 1 and 4 (a peaked head:
    the lm_head is the last op and linear, so the engine's fp32 logits and the truth's are re-read at gain g -- exactly a model whose
    lm_head weights are g x, g a power of two).  Truth = oracle/clip_t5_oracle.py's arithmetic evaluated in torch fp32 ON THE DEVICE
    (64 XXL pairs take the host cores ~40 minutes, the device seconds); cpu_baseline() cross-checks it against the same oracle on the
    host cores on the pairs both evaluate.  `rescore`: score the job again first, so that the engine's logits are this job's whatever
    ran last.  Test infrastructure: runs after the timed region."""
    from oracle.clip_t5_oracle import Oracle
    pixels, img_index, ids, labels, _ = job
    n = min(n_pairs, ids.shape[0])
    dev = pixels.device
    if rescore:
        eng.score(eng.encode_images(pixels), img_index, ids, labels)
    logits_hip = eng.stage("logits")[:n].float()
    ids_c, lab_c = ids[:n].long(), labels[:n].long()
    keep = int((ids_c != 0).sum(1).max())
    t0 = time.perf_counter()
    o = Oracle(cfg, weights, device=dev)
    parts = []
    with torch.device(dev):
        for s in range(0, n, PARITY_CHUNK):
            e = min(s + PARITY_CHUNK, n)
            uniq, inv = torch.unique(img_index[s:e].long(), return_inverse=True)      # a chunk's own images, once each
            parts.append(o.forward(pixels[uniq].float(), inv, ids_c[s:e, :keep], lab_c[s:e], return_stages=True)["logits"].float())
    logits_ref = torch.cat(parts)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t_truth = time.perf_counter() - t0
    enc_len = ((ids_c != 0).sum(1) - 1 + cfg.vision.n_patches)
    out = {"pairs": n, "truth": "oracle/clip_t5_oracle.py evaluated in torch fp32 on the device (%.1f s); cross-checked on the host cores below" % t_truth,
           "encoder_len_range": [int(enc_len.min()), int(enc_len.max())], "bound": DLOGP_BOUND, "gains": {}}
    for g in PARITY_GAINS:
        lh = Oracle.label_logprobs(logits_hip * g, lab_c)
        lr = Oracle.label_logprobs(logits_ref * g, lab_c)
        d = (lh - lr)
        per_pair = d.abs().max(1).values
        q = torch.quantile(per_pair, torch.tensor([0.5, 0.9], device=per_pair.device))
        out["gains"]["%g" % g] = {"max": float(per_pair.max()), "mean": float(per_pair.mean()), "median": float(q[0]), "p90": float(q[1]),
                                  "pairs_over_bound": int((per_pair > DLOGP_BOUND).sum()), "mean_signed": float(d.mean()),
                                  "yes_token_max": float(d[:, 0].abs().max()), "yes_token_mean": float(d[:, 0].abs().mean()),
                                  "per_pair": [round(float(x), 6) for x in per_pair],
                                  "logp_yes_range": [round(float(lr[:, 0].min()), 3), round(float(lr[:, 0].max()), 3)]}
    return out, Oracle.label_logprobs(logits_ref, lab_c).float().cpu()


def parity_jobs(cfg, weights, eng, jobs, n_pairs):
    """The |delta log P| table of a run: one job (fixed-length workloads: the batch scored last) or, when the jobs differ in length
    (length-bucketed / ragged workloads), the SHORTEST and the LONGEST job with half of the pairs each -- the two ends of the key-mask
    and padding range.  -> (table, truth log-probs of the first sample for cpu_baseline's cross-check)."""
    by_len = sorted(range(len(jobs)), key=lambda i: jobs[i][2].shape[1])
    picks = [by_len[-1]] if jobs[by_len[0]][2].shape[1] == jobs[by_len[-1]][2].shape[1] else [by_len[0], by_len[-1]]
    tables, truth0 = [], None
    for k, ji in enumerate(picks):
        t, truth = parity_sample(cfg, weights, eng, jobs[ji], max(n_pairs // len(picks), 1))
        t["job"] = ji
        tables.append(t)
        truth0 = truth if k == len(picks) - 1 else truth0
    if len(tables) == 1:
        return tables[0], truth0
    merged = {"pairs": sum(t["pairs"] for t in tables), "truth": tables[-1]["truth"], "bound": DLOGP_BOUND,
              "encoder_len_range": [min(t["encoder_len_range"][0] for t in tables), max(t["encoder_len_range"][1] for t in tables)],
              "jobs": "shortest and longest batch of the run (jobs %s): the two ends of the padding / key-mask range" % picks, "gains": {}}
    for g in tables[0]["gains"]:
        pp = [x for t in tables for x in t["gains"][g]["per_pair"]]
        merged["gains"][g] = {"max": max(pp), "mean": sum(pp) / len(pp), "pairs_over_bound": sum(t["gains"][g]["pairs_over_bound"] for t in tables),
                              "yes_token_max": max(t["gains"][g]["yes_token_max"] for t in tables),
                              "per_job": [{k: t["gains"][g][k] for k in ("max", "mean", "median", "p90", "mean_signed", "logp_yes_range")} | {"encoder_len_range": t["encoder_len_range"]}
                                          for t in tables], "per_pair": pp}
    return merged, truth0


def cpu_baseline(cfg, weights, job, n_pairs, lp_gpu, reps, with_emulation=False, parity=None, truth_dev=None, port_pairs=2):
    """The reference's arithmetic on the host cores: HF modules cast to bf16 as mm_utils.py:228 does,
    inference mode, all cores, 1 warm-up + `reps` timed repetitions on the first n_pairs pairs (one batch) of the batch the
    GPU scored last; beside it the fp32 port (oracle/clip_t5_oracle.py) on the same pairs = fp32 truth, and the per-pair
    |delta log P| table: HIP vs truth, reference-as-shipped vs truth, HIP vs reference-as-shipped.  `violation` is set (and
    bench.py exits non-zero after printing its line) when the HIP path is not at least as close to fp32 truth as the reference's
    own bf16 path on this sample, or leaves the end-to-end bound the GPU tests assert (2.5e-2)."""
    import warnings
    warnings.filterwarnings("ignore")
    from oracle.clip_t5_oracle import Oracle
    from oracle.hf_reference import HFReference
    pixels, img_index, ids, labels, _ = job
    px = pixels[:n_pairs].cpu()
    idx = torch.arange(n_pairs)
    ids_c, lab_c = ids[:n_pairs].cpu().long(), labels[:n_pairs].cpu().long()
    keep = int((ids_c != 0).sum(1).max())
    ids_c = ids_c[:, :keep]
    w_cpu = {k: v.cpu() for k, v in weights.items()}
    ref = HFReference(cfg, w_cpu, torch.bfloat16)
    times = []
    for r in range(reps + 1):                       # repetition 0 = warm-up
        t0 = time.perf_counter()
        out_ref = ref.forward(px, idx, ids_c, lab_c, timed=True)
        times.append(time.perf_counter() - t0)
    timed = sorted(times[1:]) or times
    med = timed[len(timed) // 2]
    lp_ref = out_ref["label_logprobs"]
    stage_s = dict(ref.stage_s)
    del ref
    # fp32 port on the host cores (up-casts every weight per use: slow by design, ~37 s per XXL pair): with a device-evaluated truth
    # (parity_sample) it runs on `port_pairs` pairs only -- the port's own timing and the cross-check of that truth
    n_port = n_pairs if truth_dev is None else max(1, min(port_pairs, n_pairs))
    t0 = time.perf_counter()
    truth_cpu = Oracle(cfg, w_cpu).forward(px[:n_port].float(), idx[:n_port], ids_c[:n_port], lab_c[:n_port])["label_logprobs"]
    t_port = time.perf_counter() - t0
    truth_check = None
    if truth_dev is None:
        truth = truth_cpu
    else:
        truth = truth_dev[:n_pairs]
        truth_check = float((truth_dev[:n_port] - truth_cpu).abs().max())
    emu = None
    if with_emulation:
        emu = Oracle(cfg, w_cpu, emulate="engine", acc=torch.float32).forward(px[:1].float(), idx[:1], ids_c[:1], lab_c[:1])["label_logprobs"]
    lp_hip = lp_gpu[:n_pairs].float().cpu()
    try:
        cpu_model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        cpu_model = "unknown"
    e_hip = (lp_hip - truth)                         # [pairs, T] signed
    e_ref = (lp_ref - truth)
    hip_pair = e_hip.abs().max(1).values
    ref_pair = e_ref.abs().max(1).values
    # The exit-status gate is the ABSOLUTE bound only (a strict HIP-vs-reference comparison on a few cold pairs is a noisy
    # gate); "HIP no closer to truth than the reference's own bf16 path" needs a margin and is reported as a warning field.
    violation, warning = None, None
    worst = max(float(hip_pair.max()), parity["gains"]["1"]["max"] if parity else 0.0)
    if worst > DLOGP_BOUND:
        violation = "max |dlogP| HIP vs fp32 truth %.3e > %.1e" % (worst, DLOGP_BOUND)
    worst4 = parity["gains"].get("4", {}).get("max") if parity else None
    if violation is None and worst4 is not None and worst4 > DLOGP_BOUND_GAIN4:
        violation = "head gain 4 (peaked regime): max |dlogP| HIP vs fp32 truth %.3e > %.1e" % (worst4, DLOGP_BOUND_GAIN4)
    if truth_check is not None and truth_check > 2e-4:
        violation = "device-evaluated fp32 truth differs from the host-evaluated oracle by %.3e" % truth_check
    if float(hip_pair.mean()) > 1.5 * float(ref_pair.mean()):
        warning = "mean |dlogP| vs fp32 truth: HIP %.3e > 1.5 x reference-as-shipped (HF bf16) %.3e" % (float(hip_pair.mean()), float(ref_pair.mean()))
    import transformers
    out = {"value": n_pairs / med, "unit": "pairs/s", "cores": torch.get_num_threads(), "kind": "reference",
           "kind_detail": "reference as shipped: the HF modules its CLIP-FlanT5 wrapper calls, bf16, on the host cores (oracle/hf_reference.py)",
           "sample": f"first {n_pairs} pairs of the same batch as ONE batch; HF CLIPVisionModel + T5ForConditionalGeneration in bf16, inference mode; "
                     f"1 warm-up + {len(timed)} timed repetitions, median {med:.2f} s (all: {', '.join('%.2f' % t for t in times)})",
           "stage_seconds_last_rep": stage_s,
           "host_cpus": os.cpu_count(), "cpu_model": cpu_model, "torch": torch.__version__, "transformers": transformers.__version__,
           "port_fp32": {"value": n_port / t_port, "unit": "pairs/s", "kind": "port",
                         "sample": f"oracle/clip_t5_oracle.py, fp32, the first {n_port} of those pairs, one cold pass ({t_port:.1f} s)"},
           "dlogp": {"pairs": parity["pairs"] if parity else n_pairs,
                     "hip_vs_fp32_truth": parity,          # >= 64 pairs by default, head gains 1 and 4 (peaked): BASELINE.md section 3, row (iii) vs (i)
                     "device_truth_vs_host_oracle_max": truth_check,
                     "reference_pairs": n_pairs,
                     "per_pair_abs_hip_vs_fp32_truth": [round(float(x), 6) for x in hip_pair],
                     "per_pair_abs_hf_bf16_vs_fp32_truth": [round(float(x), 6) for x in ref_pair],
                     "per_pair_abs_hip_vs_hf_bf16": [round(float(x), 6) for x in (lp_hip - lp_ref).abs().max(1).values],
                     "mean_signed_hip_vs_fp32_truth": float(e_hip.mean()), "mean_signed_hf_bf16_vs_fp32_truth": float(e_ref.mean()),
                     "hip_vs_fp32_truth_max": float(hip_pair.max()), "hf_bf16_vs_fp32_truth_max": float(ref_pair.max()),
                     "hip_vs_hf_bf16_max": (lp_hip - lp_ref).abs().max().item(),
                     "hip_closer_to_truth_than_hf_bf16_on_pairs": int((hip_pair <= ref_pair).sum()),
                     "rounding_matched_cpu_vs_fp32_truth_pair0": (emu - truth[:1]).abs().max().item() if emu is not None else None,
                     "logp_hip_pair0": lp_hip[0].tolist(), "logp_fp32_truth_pair0": truth[0].tolist(),
                     "violation": violation, "warning": warning, "bound": DLOGP_BOUND},
           "max_abs_dlogp_hip_vs_oracle": worst,
           # the same facts as flat scalars (a driver that keeps only scalar fields of this object still carries the gate)
           "dlogp_bound": DLOGP_BOUND, "dlogp_bound_gain4": DLOGP_BOUND_GAIN4, "dlogp_gain4_max": worst4, "dlogp_pairs": parity["pairs"] if parity else n_pairs,
           "dlogp_max": worst, "dlogp_mean": parity["gains"]["1"]["mean"] if parity else float(hip_pair.mean()),
           "dlogp_yes_token_max": parity["gains"]["1"]["yes_token_max"] if parity else float(e_hip[:, 0].abs().max()),
           "dlogp_pairs_over_bound": parity["gains"]["1"]["pairs_over_bound"] if parity else int((hip_pair > DLOGP_BOUND).sum()),
           "dlogp_gain4_max": parity["gains"]["4"]["max"] if parity else None,
           "dlogp_violation": violation}
    del w_cpu
    return out


if __name__ == "__main__":
    main()
