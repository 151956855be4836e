"""``hs_mxfp4_hadamard_quant`` / ``_dequant`` (``csrc/hsquant.hip``) through ``ops.native``
against the torch references, which ``test_mxfp4_hadamard.py`` checks against float64."""

import functools

import pytest
import torch

import fp8_oracle as O
from hipsnapshot import Snapshot, StateDict
from hipsnapshot.ops import native, quant
from hipsnapshot.utils.test_utils import env
from test_gpu_fp8_oracle import _run, _stream, _to_gpu
from test_mxfp4 import DST_DTYPES, SRC_DTYPES, values
from test_mxfp4_hadamard import edge_blob, exact_sum

pytestmark = pytest.mark.gpu

TILES = {native.mxfp4_hadamard_tiles(dt, r) for dt in SRC_DTYPES for r in (False, True)}
SIZES = sorted({1, 31, 32, 33, 1023, 1024, 1025, 4096 + 35, 65536 + 77}
               | {u * 1024 + d for u in TILES for d in (-1, 1)})


@functools.lru_cache(maxsize=None)
def _case(kind, n, dtype):
    x = exact_sum(n, dtype) if kind == "exact" else values(kind, n, dtype)
    return (x,) + quant.mxfp4_hadamard_quantize_reference(x)


def _quantize(gpu, ctx, x, src_off=0):
    src, nb = _to_gpu(x, gpu, src_off * x.element_size()), (x.numel() + 31) // 32
    return _run(gpu, f"{ctx} quantize", [16 * nb, nb],
                lambda c, s: native.mxfp4_hadamard_quantize(0, src, c, s, _stream()))


def _check_quant(gpu, ctx, x, payload, sbytes, src_off=0):
    codes, scales = _quantize(gpu, ctx, x, src_off)
    assert torch.equal(scales, sbytes), f"{ctx}: groups {(scales != sbytes).nonzero()[:4]}"
    assert torch.equal(codes, payload), f"{ctx}: bytes {(codes != payload).nonzero()[:4]}"


def _check_dequant(gpu, ctx, n, payload, sbytes, dst_off=0, q_off=0):
    for dst in DST_DTYPES:
        want = O.bits_of(quant.mxfp4_hadamard_dequantize_reference(payload, sbytes, n, dst))
        es = torch.empty(0, dtype=dst).element_size()
        q_dev, s_dev = _to_gpu(payload, gpu, q_off), _to_gpu(sbytes, gpu)
        (raw,) = _run(gpu, f"{ctx} dequant", [n * es], lambda d: native.mxfp4_hadamard_dequantize(
            0, q_dev, s_dev, d.view(dst), _stream()), offs=[dst_off * es])
        bad = (O.bits_of(raw.view(dst)) != want).nonzero()[0]
        assert bad.size == 0, f"{ctx} -> {dst} dst+{dst_off} q+{q_off}: elements {bad[:4]}"


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_kernels_vs_reference(gpu, dtype, n):
    """Byte for byte: every kind for f32, exact-sum values for the 16-bit MFMA."""
    f32 = dtype == torch.float32
    for kind in ("sweep", "special", "randn", "ties", "exact") if f32 else ("exact",):
        x, payload, sbytes = _case(kind, n, dtype)
        _check_quant(gpu, f"fp4h {dtype} n={n} {kind}", x, payload, sbytes)
        _check_dequant(gpu, f"fp4h {dtype} n={n} {kind}", n, payload, sbytes)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
def test_16bit_sums_move_few_codes(gpu, dtype):
    """The 16-bit MFMA sums in its own order, so a code on a rounding boundary can move.
    Three other summation orders moved at most 1 code in 2^20 on the CPU: the cap is 8."""
    x, payload, sbytes = _case("randn", 65536 + 77, dtype)
    codes, scales = _quantize(gpu, f"fp4h {dtype} randn", x)
    assert torch.equal(scales, sbytes)
    got = torch.stack([codes & 0xF, codes >> 4], dim=1).reshape(-1).int()
    want = torch.stack([payload & 0xF, payload >> 4], dim=1).reshape(-1).int()
    moved = (got != want).nonzero().reshape(-1)
    print(f"{dtype}: {moved.numel()} codes moved")
    assert moved.numel() <= 8, moved[:8]
    assert ((got[moved] - want[moved]).abs() == 1).all()  # one grid index ...
    assert (got[moved] >> 3 == want[moved] >> 3).all()  # ... with the same sign


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_misaligned_views_and_edge_scales(gpu, dtype):
    """Source / destination one element, codes one byte off: the element paths."""
    n = 4096 + 35
    x, payload, sbytes = _case("exact", n, dtype)
    _check_quant(gpu, f"fp4h {dtype} src+1", x, payload, sbytes, src_off=1)
    _check_dequant(gpu, f"fp4h {dtype}", n, payload, sbytes, dst_off=1)
    _check_dequant(gpu, f"fp4h {dtype}", n, payload, sbytes, q_off=1)
    payload, sbytes = edge_blob()
    _check_dequant(gpu, "fp4h edge scales", 32 * sbytes.numel() - 3, payload, sbytes)


def test_snapshot_gpu(gpu, tmp_path):
    w = exact_sum(777 * 333, torch.bfloat16).view(777, 333).to(gpu)
    with env(HIPSNAPSHOT_FP8_FORMAT="mxfp4_hadamard32"):
        Snapshot.take(str(tmp_path / "s"), {"sd": StateDict(w=w)}, quantize=["sd/*"])
    ref = quant.mxfp4_hadamard_dequantize_reference(
        *quant.mxfp4_hadamard_quantize_reference(w.cpu()), w.numel(), torch.bfloat16).view(w.shape)
    for out in (torch.zeros_like(w), torch.zeros(w.shape, dtype=torch.bfloat16)):
        Snapshot(str(tmp_path / "s")).restore({"sd": StateDict(w=out)})
        assert torch.equal(out.cpu(), ref)
