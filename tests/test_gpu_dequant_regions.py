"""``hs_dequant_regions`` through ``native.dequant_regions`` against the host
reference decode of the whole piece, narrowed: destination bits exact (NaN bits
included), everything outside the regions and the guards around every buffer
untouched.  The reference's bits for an e4m3 NaN code of ``mx`` are those of
the host's torch build (its vector f32 -> bf16 / f16 conversions), which the
kernel reproduces; they are no rule of the format."""

import ctypes
import functools

import pytest
import torch

from hipsnapshot.format.manifest import TensorEntry
from hipsnapshot.format.serialization import SER, dtype_to_string
from hipsnapshot.ops import native, quant
from test_gpu_fp8_oracle import GUARD, _to_gpu

pytestmark = pytest.mark.gpu

FORMATS = ["mx", "mxfp4", "mxfp6", "nvfp4"]
# (entry dtype, destination dtype): the three entry dtypes, and one cross-dtype restore
DTYPES = [(torch.bfloat16, torch.bfloat16), (torch.float16, torch.float16),
          (torch.float32, torch.float32), (torch.bfloat16, torch.float32)]
FILL = 0xAB
# column halves of 512: 16 runs per smallest tile, 3 tiles and 3 workgroups per half
BIG = (3 * native.DEQUANT_TILE_ELEMS // 512, 1024)
assert BIG[0] * 512 >= 3 * native.DEQUANT_TILE_ELEMS
# runs longer than a tile: cut inside the run, where the source index is a multiple of 32
LONG = 3 * native.DEQUANT_TILE_ELEMS + 77
ROW = native.DEQUANT_TILE_ELEMS + 45  # the second row starts 13 past a multiple of 32


@functools.lru_cache(maxsize=None)
def _base():
    """N(0, 1) with, among the first 192 values: a NaN (35), +inf (70), -inf
    (75), an all-zero block [96, 128), negative zeros (130..133) and the block
    [160, 176) 2^-30 below the rest (its nvfp4 scale byte is 0)."""
    g = torch.Generator().manual_seed(20240607)
    x = torch.randn(BIG[0] * BIG[1], generator=g)
    x[35], x[70], x[75] = float("nan"), float("inf"), float("-inf")
    x[96:128] = 0.0
    x[130:134] = -0.0
    x[160:176] *= 2.0 ** -30
    return x


@functools.lru_cache(maxsize=None)
def _piece(fmt, shape, dtype):
    """(entry, blob bytes) of the first prod(shape) base values under ``fmt``."""
    n = 1
    for z in shape:
        n *= z
    t = _base()[:n].to(dtype).view(shape)
    entry = TensorEntry("x", SER.FP8_BLOCK, dtype_to_string(dtype), list(shape), False,
                        quant=quant.fp8_entry_quant_info(t, fmt=fmt))
    staged = quant.stage_fp8(t, entry, None)
    return entry, torch.frombuffer(bytearray(staged.view), dtype=torch.uint8)


def _view(shape, kind):
    """(elements of the backing buffer, offset, strides) of a destination view
    of ``shape``."""
    st = [1] * len(shape)
    for i in range(len(shape) - 2, -1, -1):
        st[i] = st[i + 1] * shape[i + 1]
    numel = st[0] * shape[0]
    if kind == "contig":
        return numel, 0, st
    if kind == "offset1":  # contiguous, one element past an aligned address
        return numel + 1, 1, st
    if kind == "stride2":
        return 2 * numel, 0, [2 * s for s in st]
    if kind == "window":  # a column window of a wider 2-D tensor
        return shape[0] * 64, 11, [64, 1]
    assert kind == "transposed" and len(shape) == 2
    return numel, 0, [1, shape[0]]


# (piece shape, [(narrows, destination kind)]): one launch per case
CASES = {
    "one_element": ((255,), [([(0, 33, 1)], "contig")]),
    "odd_n_stride2": ((255,), [(None, "stride2")]),
    "cols_contig": ((5, 51), [([(1, 3, 37)], "contig")]),
    "cols_window": ((5, 51), [([(1, 3, 37)], "window")]),
    "rows_transposed": ((5, 51), [([(0, 1, 3)], "transposed")]),
    "collapse_partly": ((3, 4, 40), [([(0, 0, 2), (1, 0, 2)], "contig")]),
    "collapse_none": ((3, 4, 40), [([(0, 0, 2), (1, 0, 2), (2, 5, 33)], "contig")]),
    "two_regions": ((5, 51), [([(0, 0, 2), (1, 0, 20)], "contig"), ([(0, 2, 3), (1, 20, 31)], "stride2")]),
    "tiles_aligned": (BIG, [([(1, 0, 512)], "contig"), ([(1, 512, 512)], "contig")]),
    "tiles_offset1": (BIG, [([(1, 0, 512)], "offset1"), ([(1, 512, 512)], "offset1")]),
    "long_run": ((LONG,), [([(0, 5, LONG - 8)], "contig"), ([(0, 5, LONG - 8)], "offset1")]),
    "long_rows": ((2, ROW), [([(1, 3, ROW - 10)], "contig"), (None, "offset1")]),
}


def _launch(gpu, fmt, entry, blob, regions, dst_dtype):
    """Decode ``regions`` into guarded buffers; returns [(buffer, view)]."""
    info = entry.quant
    p, total = info["payload_bytes"], info["total_bytes"]
    dev_blob = _to_gpu(blob, gpu)
    es = torch.empty(0, dtype=dst_dtype).element_size()
    out, args = [], []
    for narrows, kind in regions:
        shape = list(entry.shape)
        for d, _start, length in narrows or ():
            shape[d] = length
        numel, off, strides = _view(shape, kind)
        buf = torch.full((GUARD + numel * es + GUARD,), FILL, dtype=torch.uint8, device=gpu)
        view = buf.view(dst_dtype).as_strided(shape, strides, GUARD // es + off)
        out.append((buf, view))
        args.append((narrows, view))
    native.dequant_regions(0, info["format"], dev_blob[:p], dev_blob[p: p + info["nblocks"]],
                           dev_blob[total - 4: total] if fmt == "nvfp4" else None, entry.shape,
                           args, int(torch.cuda.current_stream().cuda_stream))
    return out


@pytest.mark.parametrize("dtypes", DTYPES, ids=lambda d: f"{d[0]}-{d[1]}".replace("torch.", ""))
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("case", list(CASES))
def test_regions_equal_the_narrowed_host_decode(gpu, case, fmt, dtypes):
    shape, regions = CASES[case]
    entry, blob = _piece(fmt, shape, dtypes[0])
    as_dst = TensorEntry("x", SER.FP8_BLOCK, dtype_to_string(dtypes[1]), list(shape), False,
                         quant=entry.quant)
    ref = quant.dequantize_host_fp8(blob.numpy().tobytes(), as_dst)
    bits = torch.int32 if dtypes[1] == torch.float32 else torch.int16
    for (narrows, _kind), (buf, view) in zip(regions, _launch(gpu, fmt, entry, blob, regions,
                                                              dtypes[1])):
        want = ref
        for d, start, length in narrows or ():
            want = want.narrow(d, start, length)
        got, want = view.cpu().view(bits).reshape(-1), want.contiguous().view(bits).reshape(-1)
        bad = (got != want).nonzero().reshape(-1).tolist()
        assert not bad, (narrows, bad[:8], [hex(int(got[i]) & 0xFFFFFFFF) for i in bad[:8]],
                         [hex(int(want[i]) & 0xFFFFFFFF) for i in bad[:8]])
        # what the view does not cover still holds the fill, guards included
        view.view(bits).fill_(0)
        rest = buf.cpu()
        assert int((rest == FILL).sum()) == rest.numel() - view.numel() * view.element_size()


def test_region_past_the_piece_is_refused(gpu):
    entry, blob = _piece("mx", (5, 51), torch.bfloat16)
    dev_blob = _to_gpu(blob, gpu)
    p = entry.quant["payload_bytes"]
    dst = torch.full((5, 20), 7.0, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(ValueError, match="reaches outside the piece"):
        native.dequant_regions(0, entry.quant["format"], dev_blob[:p], dev_blob[p:], None,
                               entry.shape, [([(1, 40, 20)], dst)],
                               int(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert bool((dst == 7.0).all())


@pytest.mark.parametrize("what,fmt_id,sizes,ws,match", [
    ("past the piece", 0, [5, 60], True, "outside the piece"), ("format id", 9, [5, 20], True, "format"),
    ("null workspace", 0, [5, 20], False, "null workspace"), ("nine dims", 0, None, True, "dims")])
def test_native_entry_refuses(gpu, what, fmt_id, sizes, ws, match):
    """``hsg_dequant_regions`` itself, on a (5, 51) piece: nothing is launched."""
    lib = native.require_gpu_lib()
    entry, blob = _piece("mx", (5, 51), torch.bfloat16)
    dev_blob, dst = _to_gpu(blob, gpu), torch.full((5, 64), 7.0, dtype=torch.bfloat16, device=gpu)
    arr = native.np.zeros(1, dtype=native.DEQUANT_REGION_DTYPE)
    arr[0] = (dst.data_ptr(), 0, 100, 2, 11, tuple(sizes or ()) + (0,) * (8 - len(sizes or ())),
              (51, 1) + (0,) * 6, (64, 1) + (0,) * 6)
    if sizes is None:
        arr["ndim"] = 9
    arr["numel"] = arr["sizes"][0, 0] * arr["sizes"][0, 1]
    work, stage = torch.empty(4096, dtype=torch.uint8, device=gpu), native.PinnedBuffer(4096)
    p = entry.quant["payload_bytes"]
    rc = lib.hsg_dequant_regions(0, fmt_id, dev_blob.data_ptr(), dev_blob[p:].data_ptr(), None, 255,
                                 arr.ctypes.data, 1, work.data_ptr() if ws else None, 4096, stage.ptr,
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), 1)
    stage.release()
    assert rc != 0 and match in lib.hsg_last_error().decode(), what
    assert bool((dst == 7.0).all())
