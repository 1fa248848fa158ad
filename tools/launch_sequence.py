"""Launch-sequence records: the evidence that a host-side change moved no launch.

  run [qwen]       qwen-tiny, one 4-frame 112 x 224 video, five questions (one longer than a 128-row attention block): score_logits,
                   prefill(3), score_shared(1), score_shared(3), once each
  run gemm         one launch of each corner of the GEMM dispatch rule (gemm.hip gemm_plan): GEMM_CASES below, through the single-kernel
                   wrappers of t2v_metrics_amd.engine
  run clipt5 [NAME=VALUE ...]
                   the `small` CLIP-FlanT5 configuration on the inputs of smoke(): encode_images, score, generate of 3 tokens, under the
                   given options (gemm_variant=11 vit_fp16=0 ...)
  run clipscore    clip-tiny, 4 images x 6 texts: both towers and the similarity grid
                   Every run takes the package from the current directory and is to be run under
                   `rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/launch_sequence.py run ...`.
  list CSV         -> the ordered list "kernel name | grid | workgroup | LDS bytes", one dispatch per line, in dispatch order
  compare A B OUT  the kernel-trace CSVs of two builds -> OUT (markdown): identical or the first difference, and build A's list with
                   consecutive repeats folded
  fixture CSV OUT  the kernel trace of `run gemm` + GEMM_CASES -> OUT (JSON, one line per case: the launch as vqs_debug_gemm_plan
                   takes it, and the kernel, workgroups and workgroup size the trace shows): tests/golden/gemm_plan_parent.json
"""
import csv
import hashlib
import json
import os
import sys

# ---------------------------------------------------------------------------------------------- the GEMM dispatch corners
# call: gemm (engine.gemm), batched (engine.gemm_batched), rms (engine.gemm_resid_rms), rowscaled (engine.gemm_rowscaled); v = variant,
# t = operand type (0 bf16, 1 fp16, 2 fp16 -> bf16), touch = the l2_touch override, Z = batch entries.
def _c(what, call, M, N, K, epi, v=3, t=0, **kw):
    return dict(what=what, call=call, M=M, N=N, K=K, epi=epi, v=v, t=t, **kw)


GEMM_CASES = [
    _c("quad, one tile", "gemm", 256, 256, 128, 0),
    _c("quad, 192 tiles: slim refuses", "gemm", 4096, 3072, 256, 0),
    _c("slim", "gemm", 608, 4096, 4096, 0),
    _c("quad on request", "gemm", 608, 4096, 4096, 0, v=10),
    _c("fp16 slim", "gemm", 608, 4096, 4096, 0, t=1),
    _c("fp16 quad on request", "gemm", 608, 4096, 4096, 0, v=10, t=1),
    _c("fp16 -> bf16 gated quad", "gemm", 256, 256, 128, 5, t=2),
    _c("fp16 -> bf16 gated slim", "gemm", 608, 4096, 4096, 5, t=2),
    _c("stream, one entry", "gemm", 4, 12288, 4096, 3),
    _c("stream, batched", "batched", 128, 608, 4096, 3, Z=4),
    _c("stream, batched fp16", "batched", 128, 608, 4096, 3, t=1, Z=4),
    _c("no_stream, batched", "batched", 128, 608, 4096, 3, Z=4, no_stream=1),
    _c("no_stream, batched fp16", "batched", 128, 608, 4096, 3, t=1, Z=4, no_stream=1),
    _c("8-wave, one tile", "gemm", 256, 256, 64, 3),
    _c("8-wave, 128 workgroups: no touch, no ping-pong", "gemm", 4096, 2048, 256, 3),
    _c("8-wave, K < 256: ping-pong", "gemm", 8192, 2048, 128, 3),
    _c("8-wave, N <= 2048: touch", "gemm", 8192, 2048, 256, 3),
    _c("8-wave, N > 2048, K <= 1024: ping-pong", "gemm", 5632, 3072, 256, 3),
    _c("8-wave, N = 4096: no touch", "gemm", 4096, 4096, 2048, 3),
    _c("8-wave, N = 4096, K >= 8192: touch", "gemm", 4096, 4096, 8192, 3),
    _c("8-wave, touch forced on", "gemm", 4096, 4096, 2048, 3, touch=1),
    _c("8-wave, touch forced off: ping-pong", "gemm", 8192, 2048, 256, 3, touch=2),
    _c("8-wave rule on a quad call site", "gemm", 8192, 2048, 256, 0, v=11),
    _c("variant 0", "gemm", 512, 512, 256, 0, v=0),
    _c("variant 2", "gemm", 512, 512, 256, 0, v=2),
    _c("variant 5", "gemm", 512, 512, 256, 0, v=5),
    _c("heads, S = 4", "gemm", 256, 768, 256, 6, S=4, H=4),
    _c("heads, S = 4, variant 2", "gemm", 256, 768, 256, 6, v=2, S=4, H=4),
    _c("fp32 + residual", "gemm", 512, 512, 256, 4),
    _c("fp32 + residual, variant 5", "gemm", 512, 512, 256, 4, v=5),
    _c("fp32 + residual, variant 11", "gemm", 512, 512, 256, 4, v=11),
    _c("residual + RMSNorm producer", "rms", 512, 512, 256, 7),
    _c("residual + RMSNorm producer, variant 5", "rms", 512, 512, 256, 7, v=5),
    _c("row-scaled consumer", "rowscaled", 512, 512, 256, 0),
    _c("batched bf16 result", "batched", 256, 512, 256, 0, Z=4),
    _c("batched split-bf16 result", "batched", 256, 512, 256, 0, Z=4, split=1),
    _c("fp16 on the 8-wave kernel", "gemm", 256, 256, 64, 3, t=1),
    _c("fp16 -> bf16 on the 8-wave kernel", "gemm", 256, 256, 64, 3, t=2),
]


def plan_launch(c):
    """A case as the integers of vqs_debug_gemm_plan (include/vqs_debug.h), filled as the C entry point behind its wrapper fills the launch."""
    M, N, K, epi, Z = c["M"], c["N"], c["K"], c["epi"], c.get("Z", 1)
    S, H = c.get("S", 0), c.get("H", 0)
    ldc = {5: N // 2, 6: 0}.get(epi, N)
    flags = (2 if c["call"] == "rowscaled" else 0) | (4 if c.get("no_stream") else 0) | (32 if c["call"] == "rms" else 0)
    inner = 1 if c["call"] == "batched" or H == 0 else H * 64
    return [M, N, K, K, K, ldc, epi, Z, c["v"], max(S, 1), inner, 0, 0, 0, 0, c["t"], c.get("touch", 0),
            Z * M * ldc if c.get("split") else 0, flags, 0, 1 if c["call"] == "rowscaled" else 0, N if c["call"] in ("rms", "rowscaled") else 0]


def run_gemm():
    sys.path.insert(0, os.getcwd())
    import torch
    from t2v_metrics_amd import engine
    for c in GEMM_CASES:
        M, N, K, epi, Z = c["M"], c["N"], c["K"], c["epi"], c.get("Z", 1)
        dt = torch.float16 if c["t"] else torch.bfloat16
        A, W = torch.zeros(Z, M, K, dtype=dt, device="cuda"), torch.zeros(Z, N, K, dtype=dt, device="cuda")
        if c["call"] == "gemm":
            resid = torch.zeros(M, N, dtype=torch.float32, device="cuda") if epi == 4 else None
            engine.gemm(A[0], W[0], epi, resid=resid, S=c.get("S", 0), H=c.get("H", 0), variant=c["v"], l2_touch=c.get("touch", 0), ftype=c["t"])
        elif c["call"] == "batched":
            engine.gemm_batched(A, W, epi, split=bool(c.get("split")), no_stream=bool(c.get("no_stream")), variant=c["v"], ftype=c["t"])
        elif c["call"] == "rms":
            engine.gemm_resid_rms(A[0], W[0], torch.zeros(M, N, dtype=torch.float32, device="cuda"), torch.ones(N, dtype=dt, device="cuda"), variant=c["v"])
        else:
            engine.gemm_rowscaled(A[0], W[0], epi, torch.ones(1, M, dtype=torch.float32, device="cuda"), K, 1e-6, variant=c["v"])
        torch.cuda.synchronize()
    print("gemm:", len(GEMM_CASES), "launches")


def run_clipt5(options):
    sys.path.insert(0, os.getcwd())
    import torch
    from t2v_metrics_amd.config import get_config
    from t2v_metrics_amd.engine import VqsEngine
    from t2v_metrics_amd.weights import make_seeded_weights
    cfg = get_config("small")
    w = make_seeded_weights(cfg, seed=1, device="cpu")
    pix = torch.randn(2, 3, cfg.vision.image, cfg.vision.image, generator=torch.Generator().manual_seed(2)).to(torch.bfloat16)
    ids = torch.tensor([[11, 12, -200, 13, 14, 1], [21, -200, 22, 1, 0, 0]])
    labels, idx = torch.tensor([[40, 1], [41, 1]]), torch.tensor([0, 1])
    eng = VqsEngine(cfg, w, device="cuda:0")
    for o in options:
        name, value = o.split("=")
        eng.set_option(name, int(value))
    feats = eng.encode_images(pix.cuda())
    lp, sc = eng.score(feats, idx, ids, labels)
    tokens = eng.generate(feats, idx, ids, 3)
    torch.cuda.synchronize()
    print("clipt5", options, "scores", sc.cpu().tolist(), "tokens", tokens.cpu().tolist())
    eng.close()


def run_clipscore():
    sys.path.insert(0, os.getcwd())
    import torch
    from t2v_metrics_amd.clip.config import get_clip_config
    from t2v_metrics_amd.clip.engine import ClipEngine
    from t2v_metrics_amd.clip.weights import make_seeded_clip_weights
    from tests.clip_truth import seeded_inputs
    cfg = get_clip_config("clip-tiny")
    px, ids, pos = seeded_inputs(cfg, 4, [3, 5, 8, 12, 17, 21], seed=1)
    eng = ClipEngine(cfg, make_seeded_clip_weights(cfg, seed=0, device="cpu"), device="cuda:0")
    grid = eng.similarity(eng.encode_images(px.cuda()), eng.encode_texts(ids, pos))
    torch.cuda.synchronize()
    print("clipscore grid", [round(x, 4) for x in grid.cpu().reshape(-1).tolist()])
    eng.close()


def run_qwen():
    sys.path.insert(0, os.getcwd())
    import numpy as np
    import torch
    from t2v_metrics_amd.models.vqascore_models.qwen25vl_model import Qwen25VLModel
    from t2v_metrics_amd.qwen import get_qwen_config
    from t2v_metrics_amd.qwen.weights import make_seeded_qwen_weights
    from tests.test_gpu_qwen_shared_prefix import LONG, QUESTIONS
    from tests.test_qwen_host import FakeQwenTokenizer
    cfg = get_qwen_config("qwen-tiny")
    w = make_seeded_qwen_weights(cfg, seed=9, dtype=torch.bfloat16, lm_head_gain=4.0)
    m = Qwen25VLModel(model_name="qwen2.5-vl-7b", device="cuda", config=cfg, weights=w, tokenizer=FakeQwenTokenizer(cfg.text.vocab))
    px, grid = m.preprocess({"type": "video", "frames": np.random.RandomState(4).randint(0, 256, (4, 112, 224, 3), dtype=np.uint8)})
    eng = m.engine
    merged1 = eng.encode_vision(px, [grid])
    rows = [m.build_ids(q, "video", merged1.shape[0]) for q in QUESTIONS + [LONG]]
    B, L = len(rows), max(len(r) for r in rows)
    ids, mask = torch.zeros(B, L, dtype=torch.long), torch.zeros(B, L, dtype=torch.long)
    for k, r in enumerate(rows):
        ids[k, : len(r)] = torch.tensor(r)
        mask[k, : len(r)] = 1
    merged, grids = torch.cat([merged1] * B), [grid] * B
    a = eng.score_logits(merged, ids, mask, grids)
    b, _ = eng.prefill(merged, ids, mask, grids, 3)
    c, _ = eng.score_shared(merged, ids, mask, grids, [0] * B, 1)
    d, _ = eng.score_shared(merged, ids, mask, grids, [0] * B, 3)
    torch.cuda.synchronize()
    print("fp16 forms", eng.fp16_active, "logits bitwise equal", bool(torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)))


def dispatches(path):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    col = {k.lower(): k for k in rows[0]}
    lds = col.get("lds_block_size") or col["group_segment_size"]
    rows.sort(key=lambda r: int(r[col["dispatch_id"]]))
    dim = lambda r, what: "x".join(r[col[f"{what}_{a}"]] for a in "xyz")
    return [f'{r[col["kernel_name"]]} | {dim(r, "grid_size")} | {dim(r, "workgroup_size")} | {r[lds]}' for r in rows]


def compare(a, b, out):
    la, lb = dispatches(a), dispatches(b)
    first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None if len(la) == len(lb) else min(len(la), len(lb)))
    digest = lambda l: hashlib.sha256("\n".join(l).encode()).hexdigest()[:16]
    with open(out, "w") as f:
        f.write(f"A: {len(la)} dispatches, sha256 {digest(la)}\nB: {len(lb)} dispatches, sha256 {digest(lb)}\n")
        f.write("identical line for line\n" if first is None else f"DIFFERENT from dispatch {first}:\n  A: {la[first:first + 1]}\n  B: {lb[first:first + 1]}\n")
        f.write("\nA, consecutive repeats folded (kernel name | grid | workgroup | LDS bytes):\n\n```\n")
        i = 0
        while i < len(la):
            n = 1
            while i + n < len(la) and la[i + n] == la[i]:
                n += 1
            f.write(la[i] + (f"   x {n}" if n > 1 else "") + "\n")
            i += n
        f.write("```\n")
    return 0 if first is None else 1


def fixture(trace, out):
    rows = [d.split(" | ") for d in dispatches(trace) if "vqs::gemm_" in d]
    assert len(rows) == len(GEMM_CASES), (len(rows), len(GEMM_CASES))
    with open(out, "w") as f:
        for c, (name, grid, wg, _lds) in zip(GEMM_CASES, rows):
            g, b = int(grid.split("x")[0]), int(wg.split("x")[0])
            assert g % b == 0 and grid.split("x")[1:] == ["1", "1"] and wg.split("x")[1:] == ["1", "1"], (grid, wg)
            f.write(json.dumps({"what": c["what"], "launch": plan_launch(c), "kernel": name, "workgroups": g // b, "workgroup_size": b}) + "\n")


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        mode = sys.argv[2] if len(sys.argv) > 2 else "qwen"
        {"qwen": run_qwen, "gemm": run_gemm, "clipt5": lambda: run_clipt5(sys.argv[3:]), "clipscore": run_clipscore}[mode]()
    elif sys.argv[1:2] == ["list"]:
        print("\n".join(dispatches(sys.argv[2])))
    elif sys.argv[1:2] == ["fixture"]:
        fixture(*sys.argv[2:4])
    else:
        sys.exit(compare(*sys.argv[2:5]))
