"""The shared-prompt-prefix kernels of the Qwen2.5-VL row on their own (include/vqs_debug.h test hooks): attn_suffix_hd_kernel against
attn_fwd_hd_kernel on the same K / V slabs, and qwen_kv_assemble_kernel against a torch index copy -- bitwise.  The attention shapes put
the suffix's first row off the full kernel's 128-row blocks (Lp = 160, 224), give it more than one block of its own (Ls > 128), and vary
key norms along the sequence so that the deferred rescale fires in late tiles: the geometries the kernel's exact-no-op argument is about."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

INVALID = -1


def _lib():
    from t2v_metrics_amd import engine
    return engine.load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.view(torch.int16)


# (S, q0, H, Hkv): q0 aligned and unaligned to 128, suffixes of one and of several 128-row blocks, GQA 7:1 and 2:1
CASES = [(300, 160, 7, 1), (420, 224, 4, 2), (99, 32, 2, 1), (300, 128, 4, 2), (270, 256, 7, 1), (600, 96, 2, 2)]


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("S,q0,H,Hkv", CASES)
def test_suffix_attention_is_bitwise_the_full_kernel(S, q0, H, Hkv, f16):
    lib = _lib()
    dt = torch.float16 if f16 else torch.bfloat16
    B = 3
    g = torch.Generator().manual_seed(S * 7 + q0)
    q = torch.randn(B, H, S, 128, generator=g)
    # key norms growing / varying along the sequence: later tiles raise the running max past the rescale threshold
    k = torch.randn(B, Hkv, S, 128, generator=g) * (0.5 + 3.5 * torch.rand(B, Hkv, S, 1, generator=g)) * torch.linspace(0.5, 1.5, S).view(1, 1, S, 1)
    v = torch.randn(B, Hkv, S, 128, generator=g)
    q, k, v = (x.to(dt).cuda().contiguous() for x in (q, k, v))
    key_len = torch.tensor([S, S - 5, q0 + 9], dtype=torch.int32, device="cuda")      # ragged: padded rows past key_len in two samples
    scale = 1.0 / math.sqrt(128)
    full = torch.zeros(B * S, H * 128, dtype=dt, device="cuda")
    assert lib.vqs_debug_qwen_attention(q.data_ptr(), k.data_ptr(), v.data_ptr(), full.data_ptr(), key_len.data_ptr(), B, H, Hkv, S, scale,
                                        int(f16), _stream()) == 0
    Sq = S - q0 + 5                                                     # compact q with rows past the sequence (never read as queries)
    qs = torch.randn(B, H, Sq, 128, generator=g).to(dt).cuda()
    qs[:, :, : S - q0] = q[:, :, q0:]
    qs = qs.contiguous()
    out = torch.zeros(B * Sq, H * 128, dtype=dt, device="cuda")
    assert lib.vqs_debug_qwen_attention_suffix(qs.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), key_len.data_ptr(), B, H, Hkv, S, Sq, q0,
                                               scale, int(f16), _stream()) == 0
    torch.cuda.synchronize()
    a = full.view(B, S, -1)[:, q0:]
    b = out.view(B, Sq, -1)[:, : S - q0]
    assert torch.isfinite(a.float()).all()
    assert torch.equal(_bits(a.contiguous()), _bits(b.contiguous())), (a.float() - b.float()).abs().max().item()


def test_suffix_attention_refuses_a_first_row_off_the_32_row_waves():
    lib = _lib()
    x = torch.zeros(1, 1, 128, 128, dtype=torch.bfloat16, device="cuda")
    kl = torch.tensor([128], dtype=torch.int32, device="cuda")
    out = torch.zeros(128, 128, dtype=torch.bfloat16, device="cuda")
    for q0 in (48, 16, 128):            # not a multiple of 32; q0 >= S
        assert lib.vqs_debug_qwen_attention_suffix(x.data_ptr(), x.data_ptr(), x.data_ptr(), out.data_ptr(), kl.data_ptr(), 1, 1, 1, 128, 128, q0,
                                                   0.1, 0, _stream()) == INVALID


@pytest.mark.parametrize("U,B,Hkv,Lp,Ls", [(3, 5, 2, 96, 40), (1, 4, 4, 768, 33), (2, 2, 1, 32, 8)])
def test_kv_assemble_is_a_torch_index_copy(U, B, Hkv, Lp, Ls):
    lib = _lib()
    g = torch.Generator().manual_seed(U * 100 + Lp)

    def rnd(*shape):   # arbitrary 16-bit patterns (NaN / inf encodings included): the kernel copies bits
        return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).cuda()

    pk, pv, sk, sv = rnd(U, Hkv, Lp, 128), rnd(U, Hkv, Lp, 128), rnd(B, Hkv, Ls, 128), rnd(B, Hkv, Ls, 128)
    media = torch.tensor([(3 * b + 1) % U for b in range(B)], dtype=torch.int32)
    if B > 2:
        media[-1] = U + 4                  # outside [0, U): zero prefix rows
    media = media.cuda()
    dk = torch.full((B, Hkv, Lp + Ls, 128), 123, dtype=torch.int16, device="cuda")
    dv = torch.full_like(dk, 77)
    assert lib.vqs_debug_qwen_kv_assemble(pk.data_ptr(), pv.data_ptr(), sk.data_ptr(), sv.data_ptr(), media.data_ptr(), dk.data_ptr(), dv.data_ptr(),
                                          B, U, Hkv, Lp, Ls, _stream()) == 0
    torch.cuda.synchronize()
    ok = ((media >= 0) & (media < U)).view(B, 1, 1, 1)
    idx = media.clamp(0, U - 1).long()
    for src_p, src_s, dst in ((pk, sk, dk), (pv, sv, dv)):
        ref = torch.cat([torch.where(ok, src_p[idx], torch.zeros_like(src_p[idx])), src_s], dim=2)
        assert torch.equal(dst, ref)
