"""An fp32 CPU restatement of the kernels that tests/test_gpu_precise_decoder_kernels.py launches, behind the same entry points as the
library's test hooks: every function takes the raw addresses, strides and shapes the hooks take, reads and writes the caller's (host) memory
in place, refuses what the launchers refuse, and computes in fp32 in the kernels' order where the order is documented (slices in index
order, hi rows before lo rows, the argmax's thread partition and tree).  tests/test_precise_decoder_restatement.py drives the GPU file's own
case generators and checks over it without a GPU, and over copies carrying one planted mistake each (`mutation` = 1 .. 7), which the checks
must catch.  This is test infrastructure: nothing in the package imports it, and it is no fall-back for a missing kernel."""
import ctypes

import numpy as np
import torch

from tests import precise_decoder_ref as R

OK, INVALID = 0, -1
_CT = {torch.float32: ctypes.c_float, torch.int32: ctypes.c_int32, torch.int16: ctypes.c_int16}


def _view(ptr, n, dtype):
    """n elements at address ptr as a tensor sharing that memory (bf16 / fp16: through int16)."""
    base = torch.int16 if dtype in (torch.bfloat16, torch.float16) else dtype
    t = torch.from_numpy(np.ctypeslib.as_array((_CT[base] * int(n)).from_address(int(ptr))))
    return t if base == dtype else t.view(dtype)


def _sigmoid32(x):
    return 1.0 / (1.0 + torch.exp(-x))                      # fp32; exp overflow -> inf -> 0, as rcp(inf)


def _split_store(hi_view, lo_view, idx, y):
    hi = y.to(torch.bfloat16)
    hi_view[idx] = hi
    lo_view[idx] = (y - hi.float()).to(torch.bfloat16)      # written second: a lo plane at the hi plane's address overwrites it


class Fp32Kernels:
    def __init__(self, mutation=0):
        self.m = mutation

    # ---- elementwise.hip
    def vqs_debug_rmsnorm_split(self, x, delta, w, out, out_plane, M, D, eps, stream):
        if not x or not w or not out or M <= 0 or D <= 0 or D % 4 or out_plane % 4:
            return INVALID
        X = _view(x, M * D, torch.float32).view(M, D)
        if delta:
            X += _view(delta, M * D, torch.float32).view(M, D)
        rs = torch.rsqrt((X * X).sum(-1, keepdim=True) * np.float32(1.0 / D) + np.float32(eps))
        y = X * rs * _view(w, D, torch.bfloat16).float()
        idx = torch.arange(M * D)
        _split_store(_view(out, M * D, torch.bfloat16), _view(out + 2 * out_plane, M * D, torch.bfloat16), idx, y.reshape(-1))
        return OK

    def _slices(self, part, base, nslices, stride, rows, cols, ldp):
        idx = base + torch.arange(rows)[:, None] * ldp + torch.arange(cols)[None, :]
        a = part[idx]
        for k in range(2 if self.m == 3 else 1, nslices):
            a = a + part[idx + k * stride]
        return a

    def _gate(self, y, silu):
        F = y.shape[1] // 2
        gc = R.gate_col(torch.arange(F))
        g, l = y[:, gc], y[:, gc + (16 if self.m == 2 else 32)]
        if silu:
            return g * _sigmoid32(g) * l
        return g * _sigmoid32(np.float32(1.5957691216057308) * (g + np.float32(0.044715) * g * g * g)) * l

    def vqs_debug_sum_planes(self, part, nslices, stride, rows, cols, ldp, mode, out, ld_out, out_plane, bias, silu, stream):
        if not part or not out or rows <= 0 or cols <= 0 or nslices <= 0 or ldp % 4 or ld_out % 4 or out_plane % 4 or stride % 4:
            return INVALID
        out_cols = cols // 2 if mode == 2 else cols
        if out_cols % 4 or (mode == 2 and cols % 64) or mode not in (0, 1, 2, 3) or ((bias or silu) and mode == 3):
            return INVALID
        P = _view(part, (nslices - 1) * stride + 2 * rows * ldp, torch.float32)
        y = self._slices(P, 0, nslices, stride, rows, cols, ldp) + self._slices(P, rows * ldp, nslices, stride, rows, cols, ldp)
        if bias:
            y = y + _view(bias, cols, torch.bfloat16).float()
        if mode == 2:
            y = self._gate(y, bool(bias or silu))
        idx = (torch.arange(rows)[:, None] * ld_out + torch.arange(out_cols)[None, :])
        n = rows * ld_out
        if mode == 0:
            _view(out, n, torch.float32)[idx] = y
        elif mode == 3:
            _view(out, n, torch.float16)[idx] = y.to(torch.float16)
        else:
            lo_at = out if (self.m == 1 and mode == 1) else out + 2 * out_plane
            _split_store(_view(out, n, torch.bfloat16), _view(lo_at, n, torch.bfloat16), idx, y)
        return OK

    def vqs_debug_reduce_slices(self, part, nslices, n, out, stream):
        if not part or not out or nslices <= 0 or n <= 0 or n % 4:
            return INVALID
        P = _view(part, nslices * n, torch.float32)
        a = P[:n].clone()
        for s in range(1, nslices):
            a = a + P[s * n:(s + 1) * n]
        _view(out, n, torch.bfloat16)[:] = a.to(torch.bfloat16)
        return OK

    def vqs_debug_reduce_slices_act(self, part, nslices, stride, rows, cols, ldp, bias, gated, out, ld_out, stream):
        if not part or not out or rows <= 0 or cols <= 0 or nslices <= 0 or ldp % 4 or ld_out % 4 or stride % 4:
            return INVALID
        out_cols = cols // 2 if gated else cols
        if out_cols % 4 or (gated and cols % 64):
            return INVALID
        y = self._slices(_view(part, (nslices - 1) * stride + rows * ldp, torch.float32), 0, nslices, stride, rows, cols, ldp)
        if bias:
            y = y + _view(bias, cols, torch.bfloat16).float()
        if gated:
            y = self._gate(y, True)
        idx = torch.arange(rows)[:, None] * ld_out + torch.arange(out_cols)[None, :]
        _view(out, rows * ld_out, torch.bfloat16)[idx] = y.to(torch.bfloat16)
        return OK

    def vqs_debug_masked_softmax(self, scores, probs, key_len, B, rows, S_pad, out_f16, stream):
        if not scores or not probs or not key_len or B <= 0 or rows <= 0 or S_pad <= 0:
            return INVALID
        sc = _view(scores, B * rows * S_pad, torch.float32).view(B * rows, S_pad)
        out = _view(probs, B * rows * S_pad, torch.float16 if out_f16 else torch.bfloat16).view(B * rows, S_pad)
        kl = _view(key_len, B, torch.int32)
        j = torch.arange(S_pad)
        for r in range(B * rows):
            klen = min(int(kl[r // rows]), S_pad)
            live = sc[r, :max(klen, 0)]
            mx = live.max() if klen > 0 else torch.tensor(-3.0e38)
            e = torch.exp(live if self.m == 4 else live - mx)
            sm = e.sum()
            inv = 1.0 / sm if sm > 0 else torch.tensor(0.0)
            pv = torch.exp(sc[r] if self.m == 4 else sc[r] - mx) * inv
            keep = (j <= klen) if self.m == 5 else (j < klen)
            out[r] = torch.where(keep, pv, torch.zeros(())).to(out.dtype)
        return OK

    def vqs_debug_transpose_pad(self, inp, out, B, S, D, S_pad, stream):
        if not inp or not out or B <= 0 or S <= 0 or D <= 0 or D % 64 or S_pad % 64 or S_pad < S:
            return INVALID
        x = _view(inp, B * S * D, torch.int16).view(B, S, D)
        o = _view(out, B * D * S_pad, torch.int16).view(B, D, S_pad)
        o[:] = 0
        o[:, :, :S] = x.transpose(1, 2)
        return OK

    def vqs_debug_argmax_append(self, logits, ldl, V, tokens, ld_tokens, B, T, dst_col, flags, stream):
        if not logits or not tokens or B <= 0 or T <= 0 or V <= 0:
            return INVALID
        lg = _view(logits, B * T * ldl, torch.float32).view(B * T, ldl)
        tok = _view(tokens, B * ld_tokens, torch.int32).view(B, ld_tokens)
        col = T - 1 if dst_col < 0 else dst_col
        n = (V + 255) // 256
        for b in range(B):
            row = lg[b * T + T - 1, :V]
            if flags and not bool((row.abs() <= 3.0e38).all()):
                _view(flags, 1, torch.int32)[0] |= 2
            pad = torch.full((n * 256,), float("-inf"))
            pad[:V] = torch.nan_to_num(row, nan=float("-inf"), posinf=float("inf"), neginf=float("-inf"))       # a NaN never wins a comparison
            grid = pad.view(n, 256)                         # thread tid scans v = tid, tid + 256, ...: the first of its maxima
            first = grid.argmax(dim=0)
            val = grid.gather(0, first[None])[0]
            idx = (first * 256 + torch.arange(256)).to(torch.int32)
            won = val > -3.0e38                             # x > best, best starting at -3e38 with index 0
            val, idx = torch.where(won, val, torch.tensor(-3.0e38)), torch.where(won, idx, torch.zeros((), dtype=torch.int32))
            off = 128
            while off:
                o, oi, c, ci = val[off:2 * off], idx[off:2 * off], val[:off], idx[:off]
                take = (o > c) | ((o == c) & ((oi > ci) if self.m == 6 else (oi < ci)))
                val = torch.where(take, o, c)
                idx = torch.where(take, oi, ci)
                off >>= 1
            tok[b, col] = idx[0]
        return OK

    def _score_head(self, logits, ldl, V, labels, lp, scores, B, T, flags):
        if not logits or not labels or not lp or not scores or B <= 0 or T <= 0 or V <= 0:
            return INVALID
        lg = _view(logits, B * T * ldl, torch.float32).view(B * T, ldl)[:, :V]
        lab = _view(labels, B * T, torch.int32)
        mx = torch.nan_to_num(lg, nan=-3.0e38).amax(-1)     # fmaxf skips a NaN; the sum below does not
        tot = torch.exp(lg - mx[:, None]).sum(-1)
        ok = (lab >= 0) & (lab < V)
        picked = lg.gather(-1, lab.clamp(0, V - 1).long()[:, None])[:, 0]
        out = torch.where(ok, picked - mx - torch.log(tot), torch.zeros(()))
        _view(lp, B * T, torch.float32)[:] = out
        cnt = (lab != -100).view(B, T)
        s = torch.where(cnt, out.view(B, T), torch.zeros(())).sum(-1)
        _view(scores, B, torch.float32)[:] = torch.exp(s / cnt.sum(-1).clamp(min=1).float())
        if flags and not bool((s.abs() <= 3.0e38).all()):
            _view(flags, 1, torch.int32)[0] |= 2
        return OK

    def vqs_score_head(self, logits, ldl, V, labels, lp, scores, B, T, stream):
        return self._score_head(logits, ldl, V, labels, lp, scores, B, T, None)

    def vqs_debug_score_head(self, logits, ldl, V, labels, lp, scores, B, T, flags, stream):
        return self._score_head(logits, ldl, V, labels, lp, scores, B, T, flags)

    # ---- attn.hip
    def vqs_debug_decoder_attention(self, q, k, v, out, bias, key_len, B, H, T, S, ldq, ldk, cross, kv_stride_b, qpos0, bias_ld, precise, out_plane, stream):
        if not q or not k or not v or not out or B <= 0 or H <= 0 or T <= 0 or T > 16 or S <= 0:
            return INVALID
        if precise:
            if cross or S != T or kv_stride_b or qpos0 or ldq != ldk or (bias_ld and bias_ld != T) or out_plane <= 0:
                return INVALID
        elif R.dec_attn_lds_bytes(T, S) > 65536:
            return INVALID
        dt = torch.float32 if precise else torch.bfloat16
        I, lane = H * 64, torch.arange(64)
        Q = _view(q, B * T * ldq, dt)
        kvb = kv_stride_b if kv_stride_b else T * ldk
        nkv = B * H * S * 64 if cross else (B - 1) * kvb + S * ldk
        K, Vv = _view(k, nkv, dt), _view(v, nkv, dt)
        bld = bias_ld if bias_ld else T
        bt = _view(bias, H * bld, torch.float32).view(H, bld) if bias else None
        kl = _view(key_len, B, torch.int32) if key_len else None
        n = B * T * I
        hi_v = _view(out, n, torch.bfloat16)
        lo_v = _view(out + 2 * out_plane, n, torch.bfloat16) if precise else None
        t_i, j_i = torch.arange(T)[:, None], torch.arange(S)[None, :]
        for b in range(B):
            for h in range(H):
                qm = Q[((b * T + torch.arange(T)) * ldq + h * 64)[:, None] + lane].float()
                rows = ((b * H + h) * S + torch.arange(S)) * 64 if cross else b * kvb + torch.arange(S) * ldk + h * 64
                km, vm = K[rows[:, None] + lane].float(), Vv[rows[:, None] + lane].float()
                sc = qm @ km.T
                if cross:
                    klen = min(int(kl[b]), S) if kl is not None else S
                    masked = (j_i >= klen).expand(T, S)
                else:
                    masked = j_i > (t_i if self.m == 7 else t_i + qpos0)
                    if bt is not None:
                        sc = sc + bt[h][(t_i + qpos0 - j_i).clamp(min=0)]
                sc = torch.where(masked, torch.tensor(R.NEG_BIG, dtype=torch.float32), sc)
                e = torch.exp(sc - sc.amax(-1, keepdim=True))
                if precise:                                 # the value loop stops at the diagonal
                    e = torch.where(masked, torch.zeros(()), e)
                    o = (e @ torch.nan_to_num(vm)) / e.sum(-1, keepdim=True)
                else:                                       # ... and here it runs over all S keys: 0 * NaN stays NaN
                    o = (e @ vm) / e.sum(-1, keepdim=True)
                idx = ((b * T + torch.arange(T)) * I + h * 64)[:, None] + lane
                if precise:
                    _split_store(hi_v, lo_v, idx, o)
                else:
                    hi_v[idx] = o.to(torch.bfloat16)
        return OK
