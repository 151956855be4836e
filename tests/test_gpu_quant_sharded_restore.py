"""Quantized ShardedTensor shards and strided plain tensors restore on the GPU
(``hs_dequant_regions``): end to end through ``Snapshot`` with the CPU
dequantizer made to raise, bits against the host reference decode of every
saved shard."""

import pytest
import torch

from hipsnapshot import Snapshot, StateDict
from hipsnapshot.ops import quant
from hipsnapshot.utils.test_utils import env, run_distributed

pytestmark = pytest.mark.gpu

FORMATS = ["mx", "mxfp4", "mxfp6", "nvfp4"]
ROWS, COLS = 37, 72  # saved as row shards of 19 + 18 rows: shard edges inside blocks


def _refuse(*_a, **_k):
    raise AssertionError("the CPU dequantizer was called")


def _reference(x, fmt):
    """``x`` through the torch references of ``fmt``, in ``x``'s dtype."""
    return quant._restore_f32(x.reshape(-1).cpu(), fmt).to(x.dtype).view(x.shape)


def _sharded(boxes, fill=None):
    from torch.distributed._shard import sharded_tensor
    from torch.distributed._shard.metadata import ShardMetadata
    from torch.distributed._shard.sharding_spec import EnumerableShardingSpec

    spec = EnumerableShardingSpec([ShardMetadata(list(o), list(z), "rank:0/cuda:0")
                                   for o, z in boxes])
    st = sharded_tensor.zeros(spec, ROWS, COLS, dtype=torch.bfloat16)
    for s in st.local_shards() if fill is not None else ():
        o, z = s.metadata.shard_offsets, s.metadata.shard_sizes
        s.tensor.copy_(fill[o[0]:o[0] + z[0], o[1]:o[1] + z[1]])
    return st


def _worker(tmp):
    saved = [((0, 0), (19, COLS)), ((19, 0), (18, COLS))]
    targets = [saved,  # the saved layout
               [((0, 0), (13, COLS)), ((13, 0), (12, 40)), ((13, 40), (12, 32)),
                ((25, 0), (12, COLS))]]  # three row shards, the middle one split by columns
    x = torch.randn(ROWS, COLS, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    for fmt in FORMATS:
        with env(HIPSNAPSHOT_FP8_FORMAT=fmt):
            Snapshot.take(f"{tmp}/{fmt}", {"sd": StateDict(st=_sharded(saved, x.cuda()))},
                          quantize=["**"])
        entry = Snapshot(f"{tmp}/{fmt}").get_manifest()["0/sd/st"]
        assert all(s.tensor.quant["format"] for s in entry.shards)
        want = torch.cat([_reference(x[o[0]:o[0] + z[0]], fmt) for o, z in saved])
        host = quant.dequantize_host_fp8
        quant.dequantize_host_fp8 = _refuse
        try:
            for boxes in targets:
                out = _sharded(boxes)
                Snapshot(f"{tmp}/{fmt}").restore({"sd": StateDict(st=out)})
                for s in out.local_shards():
                    o, z = s.metadata.shard_offsets, s.metadata.shard_sizes
                    ref = want[o[0]:o[0] + z[0], o[1]:o[1] + z[1]]
                    assert torch.equal(s.tensor.cpu().view(torch.int16),
                                       ref.contiguous().view(torch.int16)), (fmt, o, z)
        finally:
            quant.dequantize_host_fp8 = host


def test_quantized_shards_restore_on_the_gpu(gpu, tmp_path):
    run_distributed(_worker, 1, str(tmp_path))


@pytest.mark.parametrize("fmt", FORMATS)
def test_quantized_tensor_into_a_strided_view(gpu, tmp_path, fmt, monkeypatch):
    w = torch.randn(33, 50, generator=torch.Generator().manual_seed(6)).to(torch.float16).to(gpu)
    with env(HIPSNAPSHOT_FP8_FORMAT=fmt):
        Snapshot.take(str(tmp_path / "s"), {"sd": StateDict(w=w)}, quantize=["**"])
    monkeypatch.setattr(quant, "dequantize_host_fp8", _refuse)
    out = torch.zeros(50, 33, dtype=torch.float16, device=gpu).t()  # not contiguous
    Snapshot(str(tmp_path / "s")).restore({"sd": StateDict(w=out)})
    assert torch.equal(out.cpu().view(torch.int16), _reference(w, fmt).view(torch.int16))
