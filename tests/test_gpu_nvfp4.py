"""``hs_nvfp4_amax`` / ``hs_nvfp4_quant`` / ``hs_nvfp4_dequant`` through
``ops.native`` against the torch reference (``test_nvfp4.py``), byte for byte,
outputs between guards."""

import functools
import math

import pytest
import torch

import fp8_oracle as O
from hipsnapshot import Snapshot, StateDict
from hipsnapshot.ops import native, quant
from hipsnapshot.utils.test_utils import env
from test_gpu_fp8_oracle import _run, _stream, _to_gpu
from test_mxfp4 import DST_DTYPES, SRC_DTYPES
from test_nvfp4 import KINDS, values

pytestmark = pytest.mark.gpu

# partial block, tail chunk, first full chunk (the amax kernel's is twice as long), a larger grid
CHUNKS = sorted({m * native.nvfp4_chunk_elems(dt) for dt in DST_DTYPES for m in (1, 2)})
SIZES = [1, 15, 16, 17] + [c + d for c in CHUNKS for d in (-1, 0, 1)] + [4096 + 35, 65536 + 77]


@functools.lru_cache(maxsize=None)
def _case(kind, n, dtype):
    x = values(kind, n, dtype)
    return (x,) + quant.nvfp4_quantize_reference(x)


def _check_quant(gpu, ctx, x, payload, sbytes, amax, src_off=0):
    src = _to_gpu(x, gpu, src_off * x.element_size())
    nb = sbytes.numel()
    codes, scales, a = _run(gpu, f"{ctx} quantize",
                            [payload.numel(), native.nvfp4_scale_bytes(x.numel()), 4],
                            lambda c, s, a: native.nvfp4_quantize(0, src, c, s, a, _stream()))
    assert torch.equal(a, amax.view(torch.uint8)), f"{ctx}: A {a.view(torch.float32)} {amax}"
    assert torch.equal(scales[:nb], sbytes) and not scales[nb:].any(), f"{ctx}: {scales} {sbytes}"
    assert torch.equal(codes, payload), f"{ctx}: bytes {(codes != payload).nonzero()[:4]}"


def _check_dequant(gpu, ctx, n, payload, sbytes, amax, dst_off=0, q_off=0):
    for dst in DST_DTYPES:
        want = O.bits_of(quant.nvfp4_dequantize_reference(payload, sbytes, amax, n, dst))
        es = torch.empty(0, dtype=dst).element_size()
        q_dev, s_dev, a_dev = _to_gpu(payload, gpu, q_off), _to_gpu(sbytes, gpu), _to_gpu(amax, gpu)
        hs = _stream()
        (raw,) = _run(gpu, f"{ctx} dequantize", [n * es],
                      lambda d: native.nvfp4_dequantize(0, q_dev, s_dev, a_dev, d.view(dst), hs),
                      offs=[dst_off * es])
        bad = (O.bits_of(raw.view(dst)) != want).nonzero()[0]
        assert bad.size == 0, f"{ctx} -> {dst} dst+{dst_off} q+{q_off}: elements {bad[:4]}"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_kernels_vs_reference(gpu, dtype, n):
    """"peak" puts the tensor's amax into the last block: A crosses workgroups
    and the first blocks' scale bytes come from the middle of the e4m3 range."""
    for kind in KINDS:
        x, payload, sbytes, amax = _case(kind, n, dtype)
        _check_quant(gpu, f"nvfp4 {dtype} n={n} {kind}", x, payload, sbytes, amax)
        _check_dequant(gpu, f"nvfp4 {dtype} n={n} {kind}", n, payload, sbytes, amax)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_misaligned_views(gpu, dtype):
    """Source / destination one element, payload one byte off: the element paths."""
    n = 4096 + 35
    x, payload, sbytes, amax = _case("peak", n, dtype)
    _check_quant(gpu, f"nvfp4 {dtype} src+1", x, payload, sbytes, amax, src_off=1)
    _check_dequant(gpu, f"nvfp4 {dtype}", n, payload, sbytes, amax, dst_off=1)
    _check_dequant(gpu, f"nvfp4 {dtype}", n, payload, sbytes, amax, q_off=1)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_non_finite_and_floor(gpu, dtype):
    """NaN block: 0x7F and zeros; inf: no part in A or in its block's scale; a
    block more than 2^23 below A: s8 == 0 and the sign bits alone."""
    n = 2 * native.nvfp4_chunk_elems(dtype) + 70
    x = values("randn", n, dtype).clone()
    x[100] = 48.0  # A
    x[256:272] = 0.0  # -inf at 261 is this block's only non-zero
    x[512:528] = 48.0 * 2.0 ** -25
    x[513:528:2] *= -1.0
    for at, v in ((5, math.nan), (64 + 15, math.nan), (n - 3, math.nan), (33, math.inf),
                  (200, -math.inf), (261, -math.inf), (n - 40, math.inf), (n - 39, -math.inf)):
        x[at] = v
    payload, sbytes, amax = quant.nvfp4_quantize_reference(x)
    assert amax.item() == 48.0
    assert sbytes[0] == 0x7F and sbytes[4] == 0x7F and sbytes[-1] == 0x7F
    assert not payload[:8].any() and not payload[(n - 3) // 16 * 8: (n + 1) // 2].any()
    assert payload[16] >> 4 == 7 and payload[100] & 0xF == 15  # +inf at 33, -inf at 200: +-6
    assert sbytes[16] == 0 and payload[130] == 0x80 and not payload[128:130].any()  # -inf at 261
    assert sbytes[32] == 0 and (payload[256:264] == 0x80).all()  # signed zeros
    _check_quant(gpu, f"nvfp4 {dtype} non-finite", x, payload, sbytes, amax)
    _check_dequant(gpu, f"nvfp4 {dtype} non-finite", n, payload, sbytes, amax)


def test_snapshot_gpu(gpu, tmp_path):
    w = values("peak", 777 * 333, torch.bfloat16).view(777, 333).to(gpu)
    with env(HIPSNAPSHOT_FP8_FORMAT="nvfp4"):
        Snapshot.take(str(tmp_path / "s"), {"sd": StateDict(w=w)}, quantize=["sd/*"])
    assert Snapshot(str(tmp_path / "s")).get_manifest()["0/sd/w"].quant["format"] == "fp4_e2m1_nv"
    payload, sbytes, amax = quant.nvfp4_quantize_reference(w.cpu())
    ref = quant.nvfp4_dequantize_reference(payload, sbytes, amax, w.numel(),
                                           torch.bfloat16).view(w.shape)
    for out in (torch.zeros_like(w), torch.zeros(w.shape, dtype=torch.bfloat16)):
        Snapshot(str(tmp_path / "s")).restore({"sd": StateDict(w=out)})
        assert torch.equal(out.cpu(), ref)
