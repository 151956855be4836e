"""The fp8 kernels of ``csrc/hsquant.hip`` against the float64 oracle
(``fp8_oracle.py``, proved on the CPU by ``test_fp8_oracle.py``): blockwise with
vpt 2, 4, 8 and 16, MX and Hadamard-rotated, quantize and dequantize, driven
through ``ops.native`` directly.

Sizes are the smallest that cross each structural edge (block, wave chunk plus
tail per element size, several tiles with an odd tile count); sources and
destinations also come as views with a storage offset, which take the kernels'
element paths.  Every output buffer sits between 64 guard bytes filled with
0xAB; each kernel runs a second time into a buffer filled with 0x54, and the
two results must agree, so every byte the format owns was written."""

import functools

import pytest
import torch

import fp8_oracle as O
from hipsnapshot.ops import native

pytestmark = pytest.mark.gpu

SRC_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DST_DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64]
SIZES = [1, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 1024 + 5, 2048 + 5, 2049, 8192 + 17,
         65536 + 77]
# source view offsets in elements: 1 breaks every vector alignment, 4 leaves a
# 16-bit source 8-byte but not 16-byte aligned
SRC_CASES = [(dt, off) for dt in SRC_DTYPES for off in ((0, 1) if dt == torch.float32 else (0, 1, 4))]
GUARD = 64
FILLS = (0xAB, 0x54)


@functools.lru_cache(maxsize=None)
def _values(kind, n, dtype, blk, rotated):
    x = O.build_values(kind, n, dtype, blk)
    x = O.hadamard_safe(x) if rotated else x
    return (x,) + O.source_arrays(x)


def _stream():
    return int(torch.cuda.current_stream().cuda_stream)


def _to_gpu(t, gpu, off_bytes=0):
    """A copy of CPU ``t`` on the GPU whose storage starts ``off_bytes`` past
    an aligned address."""
    raw = t.contiguous().view(torch.uint8)
    buf = torch.empty(off_bytes + raw.numel(), dtype=torch.uint8, device=gpu)
    buf[off_bytes:].copy_(raw)
    out = buf[off_bytes:].view(t.dtype)
    assert out.data_ptr() % 256 == off_bytes % 256
    return out


class _Guarded:
    """``sizes[i]`` owned bytes each between two 64-byte guards, ``offs[i]``
    more bytes of guard in front to misalign the owned region."""

    def __init__(self, gpu, fill, sizes, offs):
        self.fill, self.sizes, self.offs = fill, sizes, offs
        self.bufs = [torch.full((GUARD + o + s + GUARD,), fill, dtype=torch.uint8, device=gpu)
                     for s, o in zip(sizes, offs)]

    def owned(self, i):
        lo = GUARD + self.offs[i]
        return self.bufs[i][lo: lo + self.sizes[i]]

    def collect(self, what):
        out = []
        for i, buf in enumerate(self.bufs):
            host = buf.cpu()
            lo = GUARD + self.offs[i]
            hi = lo + self.sizes[i]
            assert bool((host[:lo] == self.fill).all()), f"{what}: guard before output {i} overwritten"
            assert bool((host[hi:] == self.fill).all()), f"{what}: guard after output {i} overwritten"
            out.append(host[lo:hi].clone())
        return out


def _run(gpu, what, sizes, launch, offs=None):
    """``launch(owned views)`` into 0xAB- and 0x54-filled buffers: guards
    intact, both results equal (every owned byte written).  Returns the owned
    bytes on the CPU."""
    offs = offs or [0] * len(sizes)
    results = []
    for fill in FILLS:
        g = _Guarded(gpu, fill, sizes, offs)
        launch(*[g.owned(i) for i in range(len(sizes))])
        results.append(g.collect(what))
    for i, (a, b) in enumerate(zip(*results)):
        diff = (a != b).nonzero()
        assert diff.numel() == 0, f"{what}: byte {int(diff[0])} of output {i} was not written"
    return results[0]


def _checked(ctx, fn, *args):
    try:
        fn(*args)
    except AssertionError as e:
        raise AssertionError(f"[{ctx}] {e}") from None


# -- the three formats: geometry, kernels, oracle ------------------------------

class _Block:
    rotated = False

    def __init__(self, vpt):
        self.vpt, self.blk = vpt, 64 * vpt

    def out_sizes(self, n):
        return [n, 4 * ((n + self.blk - 1) // self.blk)]

    def quant(self, src, codes, scales):
        native.fp8_quantize(0, src, codes, scales.view(torch.float32), self.vpt, _stream())

    def check_quant(self, x64, neg, codes, scales):
        O.check_block_quant(x64, neg, codes.numpy(), scales.view(torch.float32).numpy(), self.blk)

    def dequant(self, n, codes, scales, dst):
        native.fp8_dequantize(0, codes[:n], scales.view(torch.float32), dst, self.vpt, _stream())

    def check_dequant(self, codes, scales, out_bits, dst):
        O.check_block_dequant(codes.numpy(), scales.view(torch.float32).numpy(), self.blk,
                              out_bits, dst)


class _Mx:
    rotated, blk = False, O.MX_BLOCK

    def out_sizes(self, n):
        return [(n + 15) // 16 * 16, (n + 31) // 32]

    def quant(self, src, codes, scales):
        native.mx8_quantize(0, src, codes, scales, _stream())

    def check_quant(self, x64, neg, codes, scales):
        O.check_mx_quant(x64, neg, codes.numpy(), scales.numpy())

    def dequant(self, n, codes, scales, dst):
        native.mx8_dequantize(0, codes[:n], scales, dst, _stream())

    def check_dequant(self, codes, scales, out_bits, dst):
        O.check_mx_dequant(codes.numpy(), scales.numpy(), out_bits, dst)


class _Hadamard:
    rotated, blk = True, O.HAD_BLOCK

    def out_sizes(self, n):
        n_pad = (n + 31) // 32 * 32
        return [n_pad, 4 * ((n_pad + 127) // 128)]

    def quant(self, src, codes, scales):
        native.fp8_hadamard_quantize(0, src, codes, scales.view(torch.float32), _stream())

    def check_quant(self, x64, neg, codes, scales):
        O.check_hadamard_quant(x64, codes.numpy(), scales.view(torch.float32).numpy())

    def dequant(self, n, codes, scales, dst):
        native.fp8_hadamard_dequantize(0, codes, scales.view(torch.float32), dst, _stream())

    def check_dequant(self, codes, scales, out_bits, dst):
        O.check_hadamard_dequant(codes.numpy(), scales.view(torch.float32).numpy(), out_bits, dst)


FORMATS = {"block2": _Block(2), "block4": _Block(4), "block8": _Block(8), "block16": _Block(16),
           "mx": _Mx(), "hadamard": _Hadamard()}


def _dequant_case(gpu, fmt, ctx, n, codes, scales, dst_dtype, dst_off, q_off):
    """Restore the kernel's own codes and scales: ``dst`` a view ``dst_off``
    elements into its buffer, ``q`` ``q_off`` bytes past an aligned address."""
    es = torch.empty(0, dtype=dst_dtype).element_size()
    q_dev = _to_gpu(codes, gpu, q_off)
    s_dev = _to_gpu(scales, gpu)  # scale arrays stay 4-byte aligned
    (raw,) = _run(gpu, f"{ctx} dequantize", [n * es],
                  lambda dst: fmt.dequant(n, q_dev, s_dev, dst.view(dst_dtype)),
                  offs=[dst_off * es])
    _checked(f"{ctx} -> {dst_dtype} dst+{dst_off} q+{q_off}", fmt.check_dequant, codes, scales,
             O.bits_of(raw.view(dst_dtype)), dst_dtype)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("dtype,src_off", SRC_CASES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("name", list(FORMATS))
def test_fp8_kernels_vs_oracle(gpu, name, dtype, src_off, n):
    fmt = FORMATS[name]
    es = torch.empty(0, dtype=dtype).element_size()
    for kind in O.VALUE_SETS:
        ctx = f"{name} {dtype} n={n} src+{src_off} {kind}"
        x, x64, neg = _values(kind, n, dtype, fmt.blk, fmt.rotated)
        src = _to_gpu(x, gpu, src_off * es)
        codes, scales = _run(gpu, f"{ctx} quantize", fmt.out_sizes(n),
                             lambda c, s: fmt.quant(src, c, s))
        _checked(ctx, fmt.check_quant, x64, neg, codes, scales)
        if src_off:
            continue  # restore does not depend on where the source lay
        for dst_dtype in DST_DTYPES:
            _dequant_case(gpu, fmt, ctx, n, codes, scales, dst_dtype, 0, 0)
            if kind == "sweep":  # the widest range of scales: misaligned destination / codes
                _dequant_case(gpu, fmt, ctx, n, codes, scales, dst_dtype, 1, 0)
                _dequant_case(gpu, fmt, ctx, n, codes, scales, dst_dtype, 0, 1)


@pytest.mark.parametrize("name", ["block2", "block16", "hadamard"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_tiny_blocks_keep_their_zeros(gpu, name, dtype):
    """Blocks of values around 1e-38 with exact zeros among them (whole groups
    of 32 for the rotated format): the stored scale is the floor 2^-126, every
    zero restores as zero and nothing as NaN.  Before the floor the scale was
    subnormal, its reciprocal inf, and the zeros of such a block restored as
    -amax (0 * inf = NaN, swallowed by the clamp as -448)."""
    fmt = FORMATS[name]
    n = 4 * fmt.blk + 5
    g = torch.Generator().manual_seed(3)
    v = torch.rand(n, generator=g, dtype=torch.float64) * 3e-38 + 2e-39
    v *= torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    groups = torch.arange(n) // 32
    zero = (groups % 2 == 1) if fmt.rotated else (torch.rand(n, generator=g) < 0.3)
    v[zero] = 0.0
    x = v.to(dtype)
    x64, neg = O.source_arrays(x)
    src = _to_gpu(x, gpu)
    codes, scales = _run(gpu, f"{name} tiny quantize", fmt.out_sizes(n),
                         lambda c, s: fmt.quant(src, c, s))
    assert bool((scales.view(torch.float32) == 2.0 ** -126).all()), scales.view(torch.float32)
    _checked(f"{name} tiny", fmt.check_quant, x64, neg, codes, scales)
    q_dev, s_dev = _to_gpu(codes, gpu), _to_gpu(scales, gpu)
    (raw,) = _run(gpu, f"{name} tiny dequantize", [n * x.element_size()],
                  lambda dst: fmt.dequant(n, q_dev, s_dev, dst.view(dtype)))
    out = raw.view(dtype)
    assert not out.isnan().any()
    assert zero.sum() >= n // 4 and bool((out[zero] == 0).all()), out[zero].abs().max()
