"""Which kernel a Qwen2.5-VL decode-step / precise-tail attention launch takes, by the launcher's own function (vqs_kernels.h
qwen_decode_attn_form through the host-only hook vqs_debug_qwen_decode_attention_form; no GPU needed): the grouped-query kernel while its
G = Hq / Hkv <= 8 rows of fp32 scores fit 120 KiB of dynamic LDS, the per-query-head kernel beyond, nothing past 36 864 cache positions.
tests/test_gpu_qwen_decode_kernels.py asserts the form of every case it launches; these are the boundaries themselves."""
import ctypes

import pytest

GROUPED, PER_HEAD, REFUSED = 1, 0, -1


def _form(Hq, Hkv, Lmax):
    from t2v_metrics_amd import engine
    lds = ctypes.c_int64(-1)
    return engine.load_library().vqs_debug_qwen_decode_attention_form(Hq, Hkv, Lmax, ctypes.byref(lds)), lds.value


@pytest.mark.parametrize("Hq,Hkv,Lmax,form,lds", [
    (28, 4, 809, GROUPED, 7 * 812 * 4),            # the 7B geometry at the benchmarked row's length: rows padded to a multiple of 4 scores
    (7, 1, 4388, GROUPED, 122864),                 # the largest cache the grouped form takes at G = 7 ...
    (7, 1, 4389, PER_HEAD, 4389 * 4),              # ... and the first one past it (7 x 4392 x 4 = 122 976 > 120 KiB)
    (14, 2, 1760, GROUPED, 49280),                 # the first G = 7 size past 48 KiB: an opt-in launch
    (8, 1, 809, GROUPED, 8 * 812 * 4),
    (9, 1, 809, PER_HEAD, 809 * 4),                # G > 8
    (16, 1, 520, PER_HEAD, 520 * 4),
    (2, 2, 30720, GROUPED, 122880),                # G = 1: exactly 120 KiB
    (2, 2, 30721, PER_HEAD, 30721 * 4),
    (1, 1, 12289, GROUPED, 12292 * 4),
    (1, 1, 36864, PER_HEAD, 147456),               # the launcher's limit (VQS_QWEN_MAX_CACHE_POSITIONS)
    (1, 1, 36865, REFUSED, 0),
    (7, 1, 36865, REFUSED, 0),
    (7, 2, 809, REFUSED, 0),                       # Hq % Hkv != 0
    (0, 1, 809, REFUSED, 0), (7, 0, 809, REFUSED, 0), (7, 1, 0, REFUSED, 0), (7, 1, -5, REFUSED, 0),
])
def test_decode_attention_form(Hq, Hkv, Lmax, form, lds):
    assert _form(Hq, Hkv, Lmax) == (form, lds)


def test_form_hook_takes_a_null_out_parameter():
    from t2v_metrics_amd import engine
    assert engine.load_library().vqs_debug_qwen_decode_attention_form(28, 4, 809, None) == GROUPED
