"""``_hsgpu.so`` has one error channel: a message per thread, read with
``hsg_last_error()``, which every failing ``hsg_*`` call sets first.

The calls below fail their argument checks before anything is launched (the
buffers are real all the same), so each test costs a few host calls.
"""

import ctypes
import threading

import pytest
import torch

from hipsnapshot.ops import native

pytestmark = pytest.mark.gpu


def _last_error(lib) -> str:
    return lib.hsg_last_error().decode()


def _bad_quantize(lib, gpu) -> int:
    src = torch.zeros(256, dtype=torch.bfloat16, device=gpu)
    out = torch.zeros(256, dtype=torch.uint8, device=gpu)
    scales = torch.zeros(4, dtype=torch.float32, device=gpu)
    return lib.hsg_fp8_quantize(0, src.data_ptr(), native.dtype_code(src.dtype), src.numel(),
                                out.data_ptr(), scales.data_ptr(), 3, None)


def _bad_hsz_encode(lib, gpu) -> int:
    src = torch.zeros(256, dtype=torch.uint8, device=gpu)
    out = torch.zeros(4096, dtype=torch.uint8, device=gpu)
    meta = torch.zeros(int(lib.hsg_hsz_meta_bytes(8)), dtype=torch.uint8, device=gpu)
    total = torch.zeros(1, dtype=torch.int64, device=gpu)
    return lib.hsg_hsz_encode(0, src.data_ptr(), src.numel(), 3, 48, out.data_ptr(),
                              meta.data_ptr(), total.data_ptr(), None)


def test_quantize_with_bad_vpt_names_the_vpt(gpu):
    lib = native.require_gpu_lib()
    assert _bad_quantize(lib, gpu) != 0
    assert "vpt 3" in _last_error(lib)
    with pytest.raises(native.HipError, match=r"hsg_fp8_quantize failed \(-\d+\): .*vpt 3"):
        native._check(_bad_quantize(lib, gpu), "hsg_fp8_quantize")


def test_hsz_encode_and_decode_with_bad_width_name_the_width(gpu):
    lib = native.require_gpu_lib()
    assert _bad_hsz_encode(lib, gpu) != 0
    msg = _last_error(lib)
    assert "encode" in msg and "width 3" in msg
    frames = torch.zeros(256, dtype=torch.uint8, device=gpu)
    offsets = torch.zeros(2, dtype=torch.int64, device=gpu)
    out = torch.zeros(256, dtype=torch.uint8, device=gpu)
    assert lib.hsg_hsz_decode(0, frames.data_ptr(), offsets.data_ptr(), 0, 1, 48, 3, 48,
                              out.data_ptr(), None, None) != 0
    msg = _last_error(lib)
    assert "decode" in msg and "width 3" in msg


def test_hash_result_of_a_bad_handle_is_negative_with_a_message(gpu):
    lib = native.require_gpu_lib()
    out = ctypes.c_uint64(0)
    assert lib.hsg_hash64_result(0, 0, -1, ctypes.byref(out)) < 0
    assert "handle -1" in _last_error(lib)


def test_messages_are_per_thread(gpu):
    lib = native.require_gpu_lib()
    seen = {}
    a_failed, b_done = threading.Event(), threading.Event()

    def thread_a():
        seen["a_rc"] = _bad_quantize(lib, gpu)
        seen["a_first"] = _last_error(lib)
        a_failed.set()
        assert b_done.wait(60)
        seen["a_again"] = _last_error(lib)

    def thread_b():
        try:
            seen["b_rc"] = _bad_hsz_encode(lib, gpu)
            seen["b"] = _last_error(lib)
        finally:
            b_done.set()

    a = threading.Thread(target=thread_a)
    a.start()
    assert a_failed.wait(60)
    b = threading.Thread(target=thread_b)  # started after A's failure
    b.start()
    b.join(60)
    a.join(60)
    assert not a.is_alive() and not b.is_alive()
    assert seen["a_rc"] != 0 and seen["b_rc"] != 0
    assert "vpt 3" in seen["a_first"]
    assert seen["a_again"] == seen["a_first"]
    assert "width 3" in seen["b"] and "vpt" not in seen["b"]
