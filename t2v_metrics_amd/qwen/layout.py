"""Integer layout work of the Qwen2.5-VL path that stays on the host (as in the reference, where the HF processor and
``get_rope_index`` run on the CPU): window permutation of the vision tower, rotary tables, placeholder slots.
Implements what HF computes in vision_utils.py:81-188 and modeling_qwen2_5_vl.py:892-1061 for the input class the HIP
path supports: every video of one vision call has the same (t, h, w) grid (the wrapper groups samples by grid); partial
attention windows at the right / bottom edge of a frame are handled by a padded windowed layout."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch

from .config import Qwen25VLConfig


def window_slots(t: int, h: int, w: int, merge: int, window: int, patch: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """Windowed, padded cell layout of ONE video: (slots long [n_windows * ws*ws] = original cell index or -1,
    valid_cells long [n_windows]).  Windows ordered (t, window row, window column), the cells of a window row-major with
    the present ones first -- the order HF's get_vision_window_index produces (vision_utils.py:130-188) once its padding
    entries are dropped; partial windows at the right / bottom edge keep their empty slots here."""
    gh, gw, ws = h // merge, w // merge, window // merge // patch
    nh, nw = -(-gh // ws), -(-gw // ws)
    index = torch.arange(t * gh * gw).reshape(t, gh, gw)
    padded = torch.nn.functional.pad(index, (0, nw * ws - gw, 0, nh * ws - gh), value=-1)
    win = padded.reshape(t, nh, ws, nw, ws).permute(0, 1, 3, 2, 4).reshape(t * nh * nw, ws * ws)
    valid = (win >= 0).sum(-1)
    # present cells first inside every window (stable: keeps row-major order)
    order = torch.argsort((win < 0).to(torch.int8), dim=-1, stable=True)
    win = torch.gather(win, 1, order)
    keep = valid > 0
    return win[keep].reshape(-1), valid[keep]


def vision_layout(cfg: Qwen25VLConfig, grids: Sequence[Tuple[int, int, int]]) -> Dict[str, torch.Tensor]:
    """Arrays vqs_qwen_encode_vision needs for the videos of one call (same grid each); see include/vqs_qwen.h."""
    v = cfg.vision
    if len(set(tuple(g) for g in grids)) != 1:
        raise ValueError("all videos of a call must share one (t, h, w) grid")
    t, h, w = grids[0]
    unit = v.merge_unit
    cells_per = t * (h // v.spatial_merge) * (w // v.spatial_merge)
    slots1, valid1 = window_slots(t, h, w, v.spatial_merge, v.window, v.patch)
    ws = v.window // v.spatial_merge // v.patch
    slots = torch.cat([torch.where(slots1 >= 0, slots1 + i * cells_per, slots1) for i in range(len(grids))])   # [n_win * ws*ws]
    valid = valid1.repeat(len(grids))
    row_map = torch.where(slots[:, None] >= 0, slots[:, None] * unit + torch.arange(unit)[None, :], torch.full((1, unit), -1)).reshape(-1)
    N = cells_per * len(grids) * unit
    Np = row_map.numel()
    real = row_map >= 0
    inv_row = torch.empty(N, dtype=torch.long)
    inv_row[row_map[real]] = torch.nonzero(real)[:, 0]
    cell_inv = torch.empty(N // unit, dtype=torch.long)
    cell_real = slots >= 0
    cell_inv[slots[cell_real]] = torch.nonzero(cell_real)[:, 0]
    # 2-D rotary angles per ORIGINAL patch row (block-major over merge x merge, repeated per temporal patch)
    hp, wp = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    shape = (h // v.spatial_merge, v.spatial_merge, w // v.spatial_merge, v.spatial_merge)
    hp = hp.reshape(shape).transpose(1, 2).flatten().repeat(t)
    wp = wp.reshape(shape).transpose(1, 2).flatten().repeat(t)
    dim = v.head_dim // 2
    inv_freq = 1.0 / (10000.0 ** (torch.arange(0, dim, 2, dtype=torch.float32) / dim))
    ang_f = torch.cat([hp[:, None].float() * inv_freq, wp[:, None].float() * inv_freq], dim=1).repeat(len(grids), 1)   # [N, hd/2]
    ang_w = torch.where(real[:, None], ang_f[row_map.clamp(min=0)], torch.zeros(1, ang_f.shape[1]))
    return {"row_map": row_map.to(torch.int32), "inv_row": inv_row.to(torch.int32), "win_valid": (valid * unit).to(torch.int32),
            "cell_inv": cell_inv.to(torch.int32), "cos_w": ang_w.cos().contiguous(), "sin_w": ang_w.sin().contiguous(),
            "cos_f": ang_f.cos().contiguous(), "sin_f": ang_f.sin().contiguous(), "N": N, "Np": Np,
            "win_len": ws * ws * unit, "frame_len": h * w}


def text_layout(cfg: Qwen25VLConfig, input_ids: torch.Tensor, attention_mask: torch.Tensor,
                grids: Sequence[Tuple[int, int, int]]) -> Dict[str, torch.Tensor]:
    """input_ids [B, L] right-padded with one video placeholder run per sample (sample b uses grids[b]) ->
    vis_slot int32 [B, L], seq_len int32 [B], last_row int32 [B], cos/sin fp32 [B*L, head_dim/2] (M-RoPE, sections applied)."""
    t_, v = cfg.text, cfg.vision
    B, L = input_ids.shape
    is_vid = input_ids == cfg.video_token_id
    slot = torch.cumsum(is_vid.reshape(-1).long(), 0) - 1
    vis_slot = torch.where(is_vid.reshape(-1), slot, torch.full_like(slot, -1)).reshape(B, L)
    seq_len = attention_mask.long().sum(-1)
    pos = torch.zeros(3, B, L, dtype=torch.long)
    for b in range(B):
        n = int(seq_len[b])
        kinds = is_vid[b, :n].tolist()
        cur, i, chunks = 0, 0, []
        while i < n:
            j = i
            while j < n and kinds[j] == kinds[i]:
                j += 1
            if not kinds[i]:
                chunks.append(torch.arange(j - i).view(1, -1).expand(3, -1) + cur)
                cur += j - i
            else:
                t, h, w = grids[b]
                gh, gw = h // v.spatial_merge, w // v.spatial_merge
                if j - i != t * gh * gw:
                    raise ValueError("placeholder run length does not match the video grid")
                tt, hh, ww = torch.meshgrid(torch.arange(t) * v.tokens_per_second, torch.arange(gh) + cur, torch.arange(gw) + cur,
                                            indexing="ij")
                vp = torch.stack([tt, hh, ww], 0).reshape(3, -1)
                vp[0] += cur
                chunks.append(vp)
                cur += max(h, w) // v.spatial_merge
            i = j
        pos[:, b, :n] = torch.cat(chunks, 1)
    hd = t_.head_dim
    inv_freq = 1.0 / (t_.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    freqs = pos[..., None].float() * inv_freq                                      # [3, B, L, hd/2]
    sec = list(t_.mrope_section)
    ang = torch.cat([m[i % 3] for i, m in enumerate(freqs.split(sec, dim=-1))], dim=-1).reshape(B * L, hd // 2)
    last_row = torch.arange(B) * L + seq_len - 1
    # position of the first generated token: HF generate advances the prompt's LAST position by one on each axis per new token
    # (GenerationMixin updates position_ids incrementally; pinned by tests/golden/qwen_tiny_gen4.npz, whose long narrow video
    # separates this rule from "max prompt position + 1", the rope_deltas formula the cached forward would use on its own)
    next_pos = torch.stack([pos[:, b, int(seq_len[b]) - 1] + 1 for b in range(B)], dim=1)          # [3, B]
    return {"vis_slot": vis_slot.to(torch.int32), "seq_len": seq_len.to(torch.int32), "last_row": last_row.to(torch.int32),
            "cos": ang.cos().contiguous(), "sin": ang.sin().contiguous(), "position_ids": pos, "next_pos": next_pos}


def decode_tables(cfg: Qwen25VLConfig, positions: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """positions long [3, B] (t, h, w axes of the new token; equal when the prompt ends in text) -> cos, sin fp32 [B, head_dim/2],
    M-RoPE sections applied as in text_layout."""
    hd = cfg.text.head_dim
    inv_freq = 1.0 / (cfg.text.rope_theta ** (torch.arange(0, hd, 2, dtype=torch.float32, device=positions.device) / hd))
    freqs = positions[..., None].float() * inv_freq                                  # [3, B, hd/2]; on the positions' device
    ang = torch.cat([m[i % 3] for i, m in enumerate(freqs.split(list(cfg.text.mrope_section), dim=-1))], dim=-1)
    return ang.cos().contiguous(), ang.sin().contiguous()


def split_prompt_ids(ids: Sequence[int], vision_end_id: int) -> Tuple[List[int], List[int]]:
    """One prompt's ids -> (prefix, suffix): the prefix ends with (and includes) its <|vision_end|> token, the suffix is the rest."""
    ids = list(ids)
    if ids.count(vision_end_id) != 1:
        raise ValueError("a prompt must hold exactly one <|vision_end|> token")
    k = ids.index(vision_end_id) + 1
    return ids[:k], ids[k:]


SHARE_ALIGN = 32        # shared rows are a multiple of the attention kernel's 32-row waves (include/vqs_qwen.h)
MIN_SUFFIX = 8          # the q|k|v GEMM's head-major epilogue steps rows by 8 within a sample


def shared_prefix_plan(cfg: Qwen25VLConfig, input_ids: torch.Tensor, attention_mask: torch.Tensor, grids: Sequence[Tuple[int, int, int]],
                       media: Sequence) -> Optional[Dict]:
    """The shared-prefix form of one text_layout batch (vqs_qwen_prefix / vqs_qwen_score_suffix): samples b with equal media[b] share
    their prompt prefix.  None when no medium has two samples or the prefix is too short to share.  Every table is a slice of the
    unshared text_layout's, so both forms read the same numbers.
      Lp: shared rows = the split after <|vision_end|>, rounded down to a multiple of 32 (and leaving >= 8 suffix rows); Ls = L - Lp
      media_idx [B] int32 (index into the U distinct media, in order of first appearance), first [U] (each medium's first sample)
      prefix_ids / prefix_vis_slot [U, Lp] int32 (slots into the U media's merged tokens), prefix_cos / prefix_sin [U*Lp, hd/2]
      suffix_ids / suffix_vis_slot [B, Ls] int32 (slots into the batch's merged tokens), suffix_cos / suffix_sin [B*Ls, hd/2]
      seq_len [B] (whole sequences), last_row [B] = b*Ls + seq_len - 1 - Lp, next_pos [3, B]"""
    B, L = input_ids.shape
    if len(media) != B:
        raise ValueError("one medium per sample")
    order: Dict = {}
    media_idx = [order.setdefault(m, len(order)) for m in media]
    U = len(order)
    if U == B:
        return None
    seq_len = attention_mask.long().sum(-1)
    splits = []
    for b in range(B):
        pre, _ = split_prompt_ids(input_ids[b, : int(seq_len[b])].tolist(), cfg.vision_end_token_id)
        splits.append(len(pre))
    first = [media_idx.index(u) for u in range(U)]
    for b in range(B):
        f = first[media_idx[b]]
        if splits[b] != splits[f] or not torch.equal(input_ids[b, : splits[b]], input_ids[f, : splits[f]]):
            raise AssertionError("samples of one medium must share their prompt prefix")
    Lp = min(splits) // SHARE_ALIGN * SHARE_ALIGN
    while Lp >= SHARE_ALIGN and L - Lp < MIN_SUFFIX:
        Lp -= SHARE_ALIGN
    if Lp < SHARE_ALIGN:
        return None
    Ls = L - Lp
    lay = text_layout(cfg, input_ids, attention_mask, grids)
    half = lay["cos"].shape[1]
    cos, sin = lay["cos"].view(B, L, half), lay["sin"].view(B, L, half)
    vs = lay["vis_slot"]
    n_vis = (input_ids == cfg.video_token_id).sum(-1)
    off = torch.cumsum(n_vis, 0) - n_vis                                  # first merged row of each sample
    fi = torch.tensor(first)
    off_u = torch.cumsum(n_vis[fi], 0) - n_vis[fi]                        # ... of each medium among the U media
    pv = vs[fi, :Lp]
    pv = torch.where(pv >= 0, pv - off[fi, None].to(pv.dtype) + off_u[:, None].to(pv.dtype), pv)
    return {"Lp": Lp, "Ls": Ls, "U": U, "first": first, "media_idx": torch.tensor(media_idx, dtype=torch.int32),
            "prefix_ids": input_ids[fi, :Lp].to(torch.int32).contiguous(), "prefix_vis_slot": pv.to(torch.int32).contiguous(),
            "prefix_cos": cos[fi, :Lp].reshape(-1, half).contiguous(), "prefix_sin": sin[fi, :Lp].reshape(-1, half).contiguous(),
            "suffix_ids": input_ids[:, Lp:].to(torch.int32).contiguous(), "suffix_vis_slot": vs[:, Lp:].contiguous(),
            "suffix_cos": cos[:, Lp:].reshape(-1, half).contiguous(), "suffix_sin": sin[:, Lp:].reshape(-1, half).contiguous(),
            "seq_len": lay["seq_len"], "last_row": (torch.arange(B) * Ls + seq_len - 1 - Lp).to(torch.int32),
            "next_pos": lay["next_pos"]}


def answer_rows(seq_len, n_rows_per_sample, L: int, offset: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The row list of vqs_qwen_score_rows / vqs_qwen_score_suffix_rows (include/vqs_qwen.h) for "the last n_b valid positions of sample
    b", in sample order and, within a sample, in position order.  seq_len [B]: whole-sequence lengths; n_rows_per_sample: one int for all
    samples or [B]; L: rows per sample of the pass (the padded length, or Ls for the suffix pass); offset: the pass's first position
    (Lp for the suffix pass).  -> (row_index, row_sample, row_keys) int32 [sum n_b]: position p of sample b is row b * L + p - offset
    of the pass and sees p + 1 keys."""
    seq = [int(x) for x in torch.as_tensor(seq_len).reshape(-1).tolist()]
    B = len(seq)
    n = torch.as_tensor(n_rows_per_sample).reshape(-1).tolist()
    n = [int(n[0])] * B if len(n) == 1 else [int(x) for x in n]
    if len(n) != B:
        raise ValueError("one row count per sample")
    index, sample, keys = [], [], []
    for b in range(B):
        if n[b] < 1 or seq[b] - n[b] < offset or seq[b] > offset + L:
            raise ValueError(f"sample {b}: {n[b]} rows of a sequence of {seq[b]} do not lie in the pass's positions [{offset}, {offset + L})")
        for p in range(seq[b] - n[b], seq[b]):
            index.append(b * L + p - offset)
            sample.append(b)
            keys.append(p + 1)
    mk = lambda x: torch.tensor(x, dtype=torch.int32)      # noqa: E731
    return mk(index), mk(sample), mk(keys)
