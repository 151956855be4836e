"""``quant.gpu_region_decodable`` over every format's ``quant`` dict, and the
descriptor row of a region (``native.dequant_region_row``)."""

import pytest
import torch

from hipsnapshot.ops import native, quant


@pytest.mark.parametrize("fmt,ok", [("mx", True), ("mxfp4", True), ("mxfp6", True),
                                    ("nvfp4", True), ("block", False), ("hadamard32", False),
                                    ("mxfp4_hadamard32", False)])
def test_gpu_region_decodable(fmt, ok):
    info = quant.fp8_entry_quant_info(torch.zeros(5, 51, dtype=torch.bfloat16), fmt=fmt)
    assert quant.gpu_region_decodable(info) is ok
    assert not quant.gpu_region_decodable(None)


def test_region_row_collapses_and_refuses():
    row = native.dequant_region_row
    dst = torch.zeros(2, 2, 40)
    # dims 1 and 2 merge on both sides: runs of 80 source elements
    assert row((3, 4, 40), [(0, 1, 2), (1, 1, 2)], dst)[1:] == (200, 160, 2, 12, [2, 80],
                                                                [160, 1], [80, 1])
    # a box one column wide: runs of length 1 behind the collapsed dims
    assert row((5, 51), [(1, 7, 1)], torch.zeros(5, 1))[5:] == ([5, 1], [51, 1], [1, 1])
    assert row((5, 51), [(0, 2, 0)], torch.zeros(0, 51)) is None
    with pytest.raises(ValueError, match="reaches outside the piece"):
        row((5, 51), [(1, 40, 20)], torch.zeros(5, 20))
    with pytest.raises(ValueError, match="unsupported"):
        row((5, 51), None, torch.zeros(5, 51, dtype=torch.float64))
