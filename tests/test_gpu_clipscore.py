"""GPU tests of the CLIPScore row (include/vqs_clip.h): each new kernel against fp32 torch, the tiny / small configurations and
the full-size ViT-L/14-336 end to end against HF ``CLIPModel`` in fp32, and the drop-in ``CLIPScore`` class.  Everything goes
through the C ABI.  Every test runs under its own time limit (a test that hangs ends the process instead of the machine's queue).

Tolerance of the end-to-end cosines (there is no number for a cosine elsewhere in the project; it is NOT taken from the engine):
on the same seeded weights and inputs HF runs in fp32 (truth) and in bf16 (the 16-bit execution of the same modules);
e_ref16 = max |cos_bf16 - cos_fp32| over the grid.  The engine must satisfy max |cos_engine - cos_fp32| <= e_ref16 with option
fp16 = 1 (three more significand bits than bf16 at every 16-bit tensor) and <= 2 e_ref16 with fp16 = 0 (the same operand width as
the bf16 run in another accumulation order: the factor 2 is that allowance).  Ranking: for every image, every pair of texts whose
fp32 cosines differ by more than 2 e_ref16 must be ordered the same way by the engine; the pairs judged must be at least half of
all (image, text pair) triples.  The figures are printed, and written as JSON where CLIPSCORE_PARITY_JSON names a file."""
import faulthandler
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEP_TIMEOUT_S = 300


@pytest.fixture(autouse=True)
def _step_time_limit():
    faulthandler.dump_traceback_later(STEP_TIMEOUT_S, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def _record(name, figures):
    print("clipscore parity", name, json.dumps(figures))
    path = os.environ.get("CLIPSCORE_PARITY_JSON")
    if path:
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[name] = figures
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)


# ---------------------------------------------------------------- 5. kernels
U16 = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}      # unit roundoff of the 16-bit formats


def _attn_inputs(B, H, S, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, H, S, 64, generator=g).mul(s).to(dtype).cuda() for s in (1.5, 1.5, 1.0)]


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("S", [1, 8, 33, 77, 128])
def test_causal_attention_matches_fp32_torch(S, dtype):
    """Against fp32 softmax attention on the SAME 16-bit q / k / v.  Bound: the probabilities enter P.V rounded to 16 bits (relative
    error <= u each, so <= u max|v| on the normalised sum) and the output is rounded once more (<= u |o| <= u max|v|); scores, softmax
    and accumulation are fp32 (the third u covers them with room): |err| <= 3 u max|v|, u = 2^-11 (fp16) / 2^-8 (bf16)."""
    from t2v_metrics_amd.clip import engine as ce
    from tests.clip_truth import causal_attention_ref
    q, k, v = _attn_inputs(3, 5, S, dtype, seed=S)
    out = ce.causal_attention(q, k, v)
    torch.cuda.synchronize()
    ref = causal_attention_ref(q, k, v)
    err = float((out.float() - ref).abs().max())
    bound = 3 * U16[dtype] * float(v.float().abs().max())
    print(f"causal attention S={S} {dtype}: max err {err:.3e} bound {bound:.3e}")
    assert torch.isfinite(out.float()).all()
    assert err <= bound


def test_causal_attention_rows_up_to_eot_ignore_what_follows():
    """A batch whose rows end at different EOT positions: rows <= EOT are compared (same bound), and they do not change bitwise when
    everything behind each sample's EOT is replaced -- the causal mask is the only mask the text tower needs.  Padded rows stay finite."""
    from t2v_metrics_amd.clip import engine as ce
    from tests.clip_truth import causal_attention_ref
    S, eot = 77, [2, 15, 16, 40, 76]
    q, k, v = _attn_inputs(len(eot), 12, S, torch.float16, seed=7)
    out = ce.causal_attention(q, k, v).view(len(eot), S, -1)
    ref = causal_attention_ref(q, k, v).view(len(eot), S, -1)
    q2, k2, v2 = _attn_inputs(len(eot), 12, S, torch.float16, seed=8)
    for b, e in enumerate(eot):
        for dst, src in ((q2, q), (k2, k), (v2, v)):
            dst[b, :, :e + 1] = src[b, :, :e + 1]
    out2 = ce.causal_attention(q2, k2, v2).view(len(eot), S, -1)
    torch.cuda.synchronize()
    bound = 3 * U16[torch.float16] * float(v.float().abs().max())
    for b, e in enumerate(eot):
        assert float((out[b, :e + 1].float() - ref[b, :e + 1]).abs().max()) <= bound
        assert torch.equal(out[b, :e + 1], out2[b, :e + 1])
    assert torch.isfinite(out.float()).all() and torch.isfinite(out2.float()).all()


def test_causal_attention_refuses_long_sequences():
    from t2v_metrics_amd.clip import engine as ce
    from t2v_metrics_amd.engine import VqsError
    q, k, v = _attn_inputs(1, 1, 129, torch.float16, seed=0)
    with pytest.raises(VqsError):
        ce.causal_attention(q, k, v)


def test_embedding_is_the_fp32_sum():
    from t2v_metrics_amd.clip import engine as ce
    g = torch.Generator().manual_seed(3)
    tok = torch.randn(500, 768, generator=g).to(torch.bfloat16).cuda()
    pos = torch.randn(77, 768, generator=g).mul(0.1).to(torch.bfloat16).cuda()
    ids = torch.randint(0, 500, (5, 33), generator=g, dtype=torch.int32)
    out = ce.embed(ids, tok, pos)
    ref = tok.float()[ids.long().cuda()] + pos.float()[:33]
    assert torch.equal(out, ref)             # one fp32 addition of two bf16 values per element: nothing to differ in


@pytest.mark.parametrize("D,E,delta_dtype", [(768, 768, torch.float16), (1024, 768, torch.bfloat16), (128, 64, None)])
def test_pool_head_matches_fp32_torch(D, E, delta_dtype):
    """fp32 throughout on both sides; they differ in summation order only.  Outputs are entries of a unit vector (<= 1); a dot product
    of length D accumulates at most D u relative to the sum of magnitudes (u = 2^-24): bound D 2^-24 per stage, three stages (norm
    statistics, projection, L2 norm) -> 3 D 2^-24."""
    from t2v_metrics_amd.clip import engine as ce
    from tests.clip_truth import pool_head_ref
    g = torch.Generator().manual_seed(D)
    n, S = 6, 9
    x = torch.randn(n, S, D, generator=g).cuda()
    delta = None if delta_dtype is None else torch.randn(n, S, D, generator=g).mul(0.3).to(delta_dtype).cuda()
    rows = torch.randint(0, S, (n,), generator=g, dtype=torch.int32)
    lw = (1 + 0.1 * torch.randn(D, generator=g)).to(torch.bfloat16).cuda()
    lb = (0.02 * torch.randn(D, generator=g)).to(torch.bfloat16).cuda()
    proj = (torch.randn(E, D, generator=g) * D ** -0.5).to(torch.bfloat16).cuda()
    for r in (rows, None):
        out = ce.pool_head(x, delta, r, lw, lb, proj, 1e-5).cpu()
        ref = pool_head_ref(x.cpu() + (0 if delta is None else delta.float().cpu()), r, lw, lb, proj, 1e-5)
        err = float((out - ref).abs().max())
        print(f"pool+head D={D} E={E}: max err {err:.3e}")
        assert err <= 3 * D * 2.0 ** -24
        assert float((out.norm(dim=-1) - 1).abs().max()) <= 1e-6


def test_similarity_grid_and_pairs_agree_bitwise():
    from t2v_metrics_amd.clip import engine as ce
    g = torch.Generator().manual_seed(5)
    M, N, E = 37, 130, 768
    img = torch.nn.functional.normalize(torch.randn(M, E, generator=g), dim=-1).cuda()
    txt = torch.nn.functional.normalize(torch.randn(N, E, generator=g), dim=-1).cuda()
    grid = ce.similarity(img, txt)
    ii = torch.arange(M).repeat_interleave(N)
    tt = torch.arange(N).repeat(M)
    pairs = ce.similarity_pairs(img, txt, ii, tt)
    assert torch.equal(grid.reshape(-1), pairs)
    ref = img.double() @ txt.double().t()
    assert float((grid.double() - ref).abs().max()) <= E * 2.0 ** -24        # fp32 FMA chain of unit vectors: at most E u
    assert torch.isnan(ce.similarity_pairs(img, txt, [M], [0])).all()           # out-of-range index: NaN, not a read


# ---------------------------------------------------------------- 6 / 7. end to end vs HF fp32
def _end_to_end(cfg_name, n_img, lengths, seed, name):
    from t2v_metrics_amd.clip.config import get_clip_config
    from t2v_metrics_amd.clip.engine import ClipEngine
    from tests import clip_truth as ct
    cfg = get_clip_config(cfg_name)
    W = ct.seeded_weights(cfg, seed)
    px, ids, pos = ct.seeded_inputs(cfg, n_img, lengths, seed=seed + 1)
    img32, txt32, g32 = ct.hf_grid(cfg, W, px, ids, torch.float32)
    _, _, g16 = ct.hf_grid(cfg, W, px, ids, torch.bfloat16)
    out = {}
    for fp16 in (1, 0):
        eng = ClipEngine(cfg, W, device="cuda:0", options={"fp16": fp16})
        assert eng.get_option("fp16") == fp16
        img = eng.encode_images(px.cuda())
        txt = eng.encode_texts(ids, pos)
        grid = eng.similarity(img, txt)
        torch.cuda.synchronize()
        f = ct.parity_figures(grid, g32, g16)
        f["e_img"] = float((img.cpu() - img32).abs().max())
        f["e_txt"] = float((txt.cpu() - txt32).abs().max())
        out[fp16] = f
        _record(f"{name}.fp16={fp16}", f)
        eng.close()
    for fp16, f in out.items():
        assert f["coverage"] >= 0.5, f             # the ranking check judges at least half of all triples
    for fp16, f in out.items():
        allowed = f["e_ref16"] if fp16 else 2 * f["e_ref16"]
        assert f["e_engine"] <= allowed, (fp16, f)
        assert f["misordered"] == 0, (fp16, f)
        # the embeddings themselves: entries of unit vectors, held to the same yardstick as their dot products
        assert f["e_img"] <= allowed and f["e_txt"] <= allowed, (fp16, f)
    return out


def test_tiny_end_to_end_vs_hf_fp32():
    _end_to_end("clip-tiny", 4, [3, 5, 8, 12, 17, 21], seed=0, name="clip-tiny")


def test_small_end_to_end_vs_hf_fp32():
    _end_to_end("clip-small", 4, [3, 9, 16, 33, 50, 64, 77, 20], seed=0, name="clip-small")


def test_fullsize_vit_l_14_336_vs_hf_fp32():
    """openai:ViT-L-14-336 on seeded weights, 8 images x 16 texts of mixed lengths (3 to 77 tokens), HF fp32 / bf16 on the host."""
    lengths = [3, 4, 6, 9, 12, 16, 17, 23, 31, 32, 40, 48, 55, 64, 70, 77]
    _end_to_end("openai:ViT-L-14-336", 8, lengths, seed=0, name="openai:ViT-L-14-336")


# ---------------------------------------------------------------- 8. drop-in
def test_clipscore_drop_in_from_files(tmp_path):
    """CLIPScore(...)(images=[png...], texts=[...]) from files on disk equals the engine-level grid bitwise; forward on [image] * N
    pairs equals row extraction of the grid bitwise (batch-size invariance); batch_forward agrees as well."""
    from PIL import Image
    import t2v_metrics_amd as t2v
    from t2v_metrics_amd.clip.config import get_clip_config
    from tests.clip_truth import ClipTokenizerDouble
    cfg = get_clip_config("clip-small")
    rng = np.random.RandomState(0)
    paths = []
    for i, (h, w) in enumerate([(150, 200), (240, 130), (112, 112)]):
        p = str(tmp_path / f"im{i}.png")
        Image.fromarray(rng.randint(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        paths.append(p)
    texts = ["a red cube", "two dogs playing in the snow under a pale winter sun", "nothing", "a " + "very " * 90 + "long caption"]
    scorer = t2v.CLIPScore(model="openai:ViT-L-14-336", config=cfg, weights="seeded", tokenizer=ClipTokenizerDouble(cfg), device="cuda:0")
    grid = scorer(images=paths, texts=texts)
    assert grid.shape == (3, 4) and grid.dtype == torch.float32 and torch.isfinite(grid).all()
    m = scorer.model
    ids, pos = m.tokenize(texts)
    assert ids.shape[1] == cfg.text.context and int(pos[3]) == cfg.text.context - 1
    eng_grid = m.engine.similarity(m.engine.encode_images(m.load_images(paths)), m.engine.encode_texts(ids, pos))
    assert torch.equal(grid.cpu(), eng_grid.cpu())
    for i, p in enumerate(paths):
        row = m.forward([p] * len(texts), texts)
        assert torch.equal(row, grid[i].cpu())
    one = m.forward([paths[1]], [texts[2]])
    assert torch.equal(one[0], grid[1, 2].cpu())
    ds = [{"images": [paths[0], paths[1]], "texts": [texts[0], texts[1]]}, {"images": [paths[2], paths[0]], "texts": [texts[3], texts[0]]}]
    bf = scorer.batch_forward(ds, batch_size=2).cpu()
    assert torch.equal(bf[0], grid[:2, :2].cpu()) and torch.equal(bf[1, 0], grid[2, [3, 0]].cpu()) and torch.equal(bf[1, 1], grid[0, [3, 0]].cpu())
