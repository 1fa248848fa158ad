"""Launch-sequence record of the Qwen2.5-VL language-model passes: the evidence that a host-side change moved no launch.

  run              qwen-tiny, one 4-frame 112 x 224 video, five questions (one longer than a 128-row attention block): score_logits,
                   prefill(3), score_shared(1), score_shared(3), once each, from the package in the current directory.  To be run under
                   `rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/qwen_launch_sequence.py run`.
  list CSV         -> the ordered list "kernel name | grid | workgroup | LDS bytes", one dispatch per line, in dispatch order
  compare A B OUT  the kernel-trace CSVs of two builds -> OUT (markdown): identical or the first difference, and build A's list with
                   consecutive repeats folded
"""
import csv
import hashlib
import os
import sys


def run():
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


if __name__ == "__main__":
    if sys.argv[1:2] == ["run"]:
        run()
    elif sys.argv[1:2] == ["list"]:
        print("\n".join(dispatches(sys.argv[2])))
    else:
        sys.exit(compare(*sys.argv[2:5]))
