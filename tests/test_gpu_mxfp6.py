"""``hs_mxfp6_quant`` / ``hs_mxfp6_dequant`` through ``ops.native`` against the
torch reference (``test_mxfp6.py``), byte for byte, outputs between guards."""

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
from test_mxfp6 import KINDS, values

pytestmark = pytest.mark.gpu

# the partial block, the tail chunk, the first full LDS-transposed step, a multi-wave grid
CHUNKS = sorted({native.mxfp6_chunk_elems(dt) for dt in DST_DTYPES})
SIZES = [1, 31, 32, 33] + [c + d for c in CHUNKS for d in (-1, 0, 1)] + [4096 + 35, 65536 + 77]


@functools.lru_cache(maxsize=None)
def _case(kind, n, dtype):
    x = values(kind, n, dtype)
    return (x,) + quant.mxfp6_quantize_reference(x)


def _check_quant(gpu, ctx, x, payload, sbytes, src_off=0):
    src = _to_gpu(x, gpu, src_off * x.element_size())
    codes, scales = _run(gpu, f"{ctx} quantize", [payload.numel(), sbytes.numel()],
                         lambda c, s: native.mxfp6_quantize(0, src, c, s, _stream()))
    assert torch.equal(scales, sbytes), f"{ctx}: blocks {(scales != sbytes).nonzero()[:4]}"
    assert torch.equal(codes, payload), f"{ctx}: bytes {(codes != payload).nonzero()[:4]}"


def _check_dequant(gpu, ctx, n, payload, sbytes, dst_off=0, q_off=0):
    for dst in DST_DTYPES:
        want = O.bits_of(quant.mxfp6_dequantize_reference(payload, sbytes, n, dst))
        es = torch.empty(0, dtype=dst).element_size()
        q_dev, s_dev = _to_gpu(payload, gpu, q_off), _to_gpu(sbytes, gpu)
        (raw,) = _run(gpu, f"{ctx} dequantize", [n * es],
                      lambda d: native.mxfp6_dequantize(0, q_dev, s_dev, d.view(dst), _stream()),
                      offs=[dst_off * es])
        bad = (O.bits_of(raw.view(dst)) != want).nonzero()[0]
        assert bad.size == 0, f"{ctx} -> {dst} dst+{dst_off} q+{q_off}: elements {bad[:4]}"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_kernels_vs_reference(gpu, dtype, n):
    for kind in KINDS:
        x, payload, sbytes = _case(kind, n, dtype)
        _check_quant(gpu, f"mxfp6 {dtype} n={n} {kind}", x, payload, sbytes)
        _check_dequant(gpu, f"mxfp6 {dtype} n={n} {kind}", n, payload, sbytes)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_misaligned_views(gpu, dtype):
    """Source / destination one element, payload one byte off: the element paths."""
    n = 4096 + 35
    x, payload, sbytes = _case("sweep", n, dtype)
    _check_quant(gpu, f"mxfp6 {dtype} src+1", x, payload, sbytes, src_off=1)
    _check_dequant(gpu, f"mxfp6 {dtype}", n, payload, sbytes, dst_off=1)
    _check_dequant(gpu, f"mxfp6 {dtype}", n, payload, sbytes, q_off=1)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_nan_blocks_and_infinities(gpu, dtype):
    """NaN block: 0xFF and zeros; inf: code +-7.5, no part in the scale."""
    n = 2 * native.mxfp6_chunk_elems(dtype) + 70
    x = values("randn", n, dtype).clone()
    x[256:288] = 0.0  # -inf at 261 is this block's only non-zero
    for at, v in ((5, math.nan), (64 + 31, math.nan), (n - 3, math.nan), (33, math.inf),
                  (200, -math.inf), (261, -math.inf), (n - 40, math.inf), (n - 39, -math.inf)):
        x[at] = v
    payload, sbytes = quant.mxfp6_quantize_reference(x)
    assert sbytes[0] == 0xFF and sbytes[2] == 0xFF and sbytes[-1] == 0xFF and sbytes[8] == 127
    # element 5 of block 8 straddles two payload words: bits 30 .. 35 are all set
    assert (payload[:24] == 0).all() and payload[8 * 24 + 3] == 0xC0 and payload[8 * 24 + 4] == 0x0F
    assert payload[24] >> 6 == 3 and payload[25] & 0xF == 7  # +inf, element 1 of block 1: code 31
    _check_quant(gpu, f"mxfp6 {dtype} non-finite", x, payload, sbytes)
    _check_dequant(gpu, f"mxfp6 {dtype} non-finite", n, payload, sbytes)


def test_snapshot_gpu(gpu, tmp_path):
    w = values("randn", 777 * 333, torch.bfloat16).view(777, 333).to(gpu)
    with env(HIPSNAPSHOT_FP8_FORMAT="mxfp6"):
        Snapshot.take(str(tmp_path / "s"), {"sd": StateDict(w=w)}, quantize=["sd/*"])
    assert Snapshot(str(tmp_path / "s")).get_manifest()["0/sd/w"].quant["format"] == "fp6_e2m3_mx"
    payload, sbytes = quant.mxfp6_quantize_reference(w.cpu())
    ref = quant.mxfp6_dequantize_reference(payload, sbytes, w.numel(), torch.bfloat16).view(w.shape)
    for out in (torch.zeros_like(w), torch.zeros(w.shape, dtype=torch.bfloat16)):
        Snapshot(str(tmp_path / "s")).restore({"sd": StateDict(w=out)})
        assert torch.equal(out.cpu(), ref)
