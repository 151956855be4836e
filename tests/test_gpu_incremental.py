"""Incremental takes on HBM tensors: the ``hs_hash64_batch`` kernel against
the NumPy definition and the per-blob kernel, then ``take(base=...)`` end to
end (slab members, own blobs, HSZ1, DTensor shards, ineligible leaves)."""

import contextlib
import json
import os

import pytest
import torch

import incremental_workers as W
from hipsnapshot import Snapshot, StateDict, knobs
from hipsnapshot.engine import incremental
from hipsnapshot.knobs import override_knob, override_slab_size_threshold_bytes
from hipsnapshot.ops import checksum
from hipsnapshot.ops.checksum import hs64_reference
from hipsnapshot.snapshot import TakeStats
from hipsnapshot.utils.test_utils import run_distributed

pytestmark = pytest.mark.gpu

TILE = 32 << 10  # the batch kernel's smallest tile (every launch here but one is small)
SMALL_SIZES = [0, 1, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097]
TILE_SIZES = [TILE - 8, TILE, TILE + 8, 3 * TILE + 24 + 5]
OFFSETS = [0, 2, 4, 8]
POOL_BYTES = 2 << 20


@pytest.fixture(scope="module")
def pool():
    """Random device bytes (16-byte aligned base) and their host copy: every
    kernel test hashes windows of it, the references are computed once."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    g = torch.Generator(device="cuda:0").manual_seed(7)
    dev = torch.randint(0, 256, (POOL_BYTES,), dtype=torch.uint8, device="cuda:0", generator=g)
    assert dev.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    return dev, dev.cpu().numpy(), {}


def _reference(pool, start, n):
    _dev, host, memo = pool
    if (start, n) not in memo:
        memo[(start, n)] = hs64_reference(host[start:start + n])
    return memo[(start, n)]


def _per_blob_kernel(ptr, n):
    return checksum.device_hash_result(0, 0, checksum.device_hash_start(0, 0, ptr, n), n)


def _windows(sizes, offsets):
    """Disjoint windows of the pool: (start, nbytes), start = 16k + offset."""
    out, at = [], 0
    for off in offsets:
        for n in sizes:
            out.append((at + off, n))
            at += (off + n + 15) // 16 * 16 + 16
    assert at <= POOL_BYTES
    return out


def _check(pool, windows):
    dev = pool[0]
    base = dev.data_ptr()
    got = checksum.device_hash_batch(0, [(base + s, n) for s, n in windows])
    assert len(got) == len(windows)
    for (s, n), h in zip(windows, got):
        assert h == _reference(pool, s, n), (s, n)
        assert h == _per_blob_kernel(base + s, n), (s, n)


@pytest.mark.parametrize("offset", OFFSETS)
def test_batch_hash_small_sizes(gpu, pool, offset):
    _check(pool, _windows(SMALL_SIZES, [offset]))


@pytest.mark.parametrize("offset", OFFSETS)
def test_batch_hash_around_a_tile_and_across_three(gpu, pool, offset):
    _check(pool, _windows(TILE_SIZES, [offset]))


@pytest.mark.parametrize("n", SMALL_SIZES + TILE_SIZES[:1] + TILE_SIZES[-1:])
def test_batch_hash_single_leaf(gpu, pool, n):
    _check(pool, [(0, n)])
    _check(pool, [(16 + 2, n)])


def test_batch_hash_more_leaves_than_workgroups(gpu, pool):
    windows = [(64 * i, 64) for i in range(3000)]
    got = checksum.device_hash_batch(0, [(pool[0].data_ptr() + s, n) for s, n in windows])
    assert got == [_reference(pool, s, n) for s, n in windows]
    for i in (0, 1, 2047, 2048, 2999):  # (the per-blob kernel: a sample, one sync each)
        assert got[i] == _per_blob_kernel(pool[0].data_ptr() + windows[i][0], 64)


def test_batch_hash_mix_in_one_launch(gpu, pool):
    windows = _windows(SMALL_SIZES + TILE_SIZES, OFFSETS)
    at = (max(s + n for s, n in windows) + 15) // 16 * 16
    windows += [(at + 64 * i, 64) for i in range(3000)]
    assert windows[-1][0] + 64 <= POOL_BYTES
    _check(pool, windows[:len(windows) - 3000])
    dev = pool[0]
    got = checksum.device_hash_batch(0, [(dev.data_ptr() + s, n) for s, n in windows])
    assert got == [_reference(pool, s, n) for s, n in windows]


def test_batch_hash_larger_tiles(gpu):
    """Enough bytes that the tile grows past 32 KiB (>= 4096 tiles of 64 KiB):
    a leaf of many tiles plus an unaligned one, against the per-blob kernel
    and the C++ hasher (the NumPy definition would take seconds here)."""
    n_big = (288 << 20) + 8 + 3
    g = torch.Generator(device="cuda:0").manual_seed(11)
    dev = torch.randint(0, 256, (n_big + (1 << 20),), dtype=torch.uint8, device="cuda:0",
                        generator=g)
    torch.cuda.synchronize()
    small_at = (n_big + 15) // 16 * 16 + 2
    blobs = [(dev.data_ptr(), n_big), (dev.data_ptr() + small_at, 200_001)]
    got = checksum.device_hash_batch(0, blobs)
    assert got == [_per_blob_kernel(p, n) for p, n in blobs]
    host = dev.cpu()
    assert got[0] == checksum.hs64_host(host.data_ptr(), n_big)
    assert got[1] == hs64_reference(host[small_at:small_at + 200_001].numpy())


def test_batch_hash_is_ordered_after_the_producer(gpu):
    """The launch goes on the current stream: it sees what was queued there."""
    t = torch.zeros(1 << 20, dtype=torch.float32, device=gpu)
    for _ in range(20):
        t.add_(1.0)
    h = checksum.device_hash_batch(0, [(t.data_ptr(), t.numel() * 4)])[0]
    assert h == hs64_reference(torch.full((1 << 20,), 20.0).numpy())


# -- end to end ------------------------------------------------------------------

SIZES = {"a": 4 << 10, "b": 6 << 10, "odd": (5 << 10) + 3, "c": 16 << 10, "d": 40 << 10,
         "e": 64 << 10}


def _state(gpu, seed=0):
    g = torch.Generator(device=gpu).manual_seed(seed)
    return StateDict(**{k: torch.randint(0, 256, (n,), dtype=torch.uint8, device=gpu,
                                         generator=g) for k, n in SIZES.items()})


def _leaf_entries(path):
    return {k.split("/")[-1]: e for k, e in Snapshot(path).get_manifest().items()
            if hasattr(e, "location")}


@pytest.mark.parametrize("threshold", [None, 8 << 10], ids=["slabs", "slab_threshold_8k"])
def test_two_changed_hbm_tensors(gpu, tmp_path, threshold):
    from hipsnapshot.engine import native_restore

    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    cm = override_slab_size_threshold_bytes(threshold) if threshold \
        else contextlib.nullcontext()
    with cm:
        sd = _state(gpu)
        Snapshot.take(A, {"sd": sd}, content_digests=True)
        sd["b"][17] ^= 0xFF
        sd["odd"][-1] ^= 1  # one bit in the zero-padded tail word
        Snapshot.take(B, {"sd": sd}, base=A)
    changed = ("b", "odd")
    stats = dict(TakeStats.last)
    for k, e in _leaf_entries(B).items():
        assert e.location.startswith("../") == (k not in changed), (k, e.location)
    assert stats["bytes_reused"] == sum(n for k, n in SIZES.items() if k not in changed)
    assert stats["bytes"] <= SIZES["b"] + SIZES["odd"] + knobs.slab_align()
    out = StateDict(**{k: torch.zeros_like(v) for k, v in sd.items()})
    native_restore.last_stats.clear()
    with override_knob("NATIVE_RESTORE", "1"):
        Snapshot(B).restore({"sd": out})
    torch.cuda.synchronize()
    assert native_restore.last_stats.get("items", 0) > 0  # the native job read the base's blobs
    for k in SIZES:
        assert torch.equal(out[k], sd[k]), k
    rep = Snapshot(B).verify()
    assert rep.ok and rep.checked == rep.blobs, rep.as_dict()
    out2 = StateDict(**{k: torch.zeros_like(v) for k, v in sd.items()})
    with override_knob("NATIVE_RESTORE", "0"):
        Snapshot(B).restore({"sd": out2}, verify=True)
    torch.cuda.synchronize()
    for k in SIZES:
        assert torch.equal(out2[k], sd[k]), k


def test_hsz1_base(gpu, tmp_path):
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    g = torch.Generator(device=gpu).manual_seed(3)
    sd = StateDict(
        big=(torch.randn(300, 1024, device=gpu, generator=g) * 0.02).to(torch.bfloat16),
        own=torch.randn(70_001, device=gpu, generator=g),
        s1=torch.randn(20_000, device=gpu, generator=g),
        s2=(torch.randn(33_333, device=gpu, generator=g) * 0.1).to(torch.float16))
    with override_slab_size_threshold_bytes(256 << 10):  # big, own: blobs of their own
        Snapshot.take(A, {"sd": sd}, compression="hsz1", content_digests=True)
        a_entries = _leaf_entries(A)
        assert all(e.codec is not None for e in a_entries.values())
        sd["s1"][5] += 1.0
        Snapshot.take(B, {"sd": sd}, compression="hsz1", base=A)
    b_entries = _leaf_entries(B)
    for k, e in b_entries.items():
        assert e.location.startswith("../") == (k != "s1"), (k, e.location)
        if k != "s1":  # A's codec record and byte range travel with the location
            assert e.codec == a_entries[k].codec and e.byte_range == a_entries[k].byte_range
    doc = json.loads((tmp_path / "B" / ".snapshot_content" / "0").read_text())
    for k, e in b_entries.items():  # digests of the raw bytes, not of the HSZ1 blob
        assert int(doc["leaves"][incremental.content_key(e)], 16) == \
            hs64_reference(sd[k].cpu().view(torch.uint8).numpy()), k
    out = StateDict(**{k: torch.zeros_like(v) for k, v in sd.items()})
    Snapshot(B).restore({"sd": out})
    torch.cuda.synchronize()
    for k in sd.keys():
        assert torch.equal(out[k], sd[k]), k
    assert Snapshot(B).verify().ok


def test_dtensor_shards_on_a_one_rank_mesh(gpu, tmp_path):
    # a process of its own: the mesh needs a default process group
    run_distributed(W.dtensor_one_rank_mesh, 1, str(tmp_path))


def test_ineligible_leaves_are_written_in_full(gpu, tmp_path):
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    g = torch.Generator(device=gpu).manual_seed(9)
    m = torch.randn(128, 96, device=gpu, generator=g)
    sd = StateDict(plain=torch.randn(5000, device=gpu, generator=g),
                   view=m.t(),                                  # non-contiguous
                   q=torch.randn(64, 512, device=gpu, generator=g).to(torch.bfloat16))
    Snapshot.take(A, {"sd": sd}, quantize=["sd/q"], content_digests=True)
    Snapshot.take(B, {"sd": sd}, quantize=["sd/q"], base=A)
    entries = _leaf_entries(B)
    assert entries["plain"].location.startswith("../")
    assert not entries["view"].location.startswith("../")
    assert not entries["q"].location.startswith("../")
    assert TakeStats.last["leaves_reused"] == 1
    doc = json.loads((tmp_path / "B" / ".snapshot_content" / "0").read_text())
    assert list(doc["leaves"]) == [incremental.content_key(entries["plain"])]
    out = StateDict(plain=torch.zeros_like(sd["plain"]), view=torch.zeros(96, 128, device=gpu),
                    q=torch.zeros_like(sd["q"]))
    Snapshot(B).restore({"sd": out})
    torch.cuda.synchronize()
    assert torch.equal(out["plain"], sd["plain"]) and torch.equal(out["view"], sd["view"])
    ref = StateDict(q=torch.zeros_like(sd["q"]))
    Snapshot(A).restore({"sd": StateDict(plain=torch.zeros_like(sd["plain"]),
                                         view=torch.zeros(96, 128, device=gpu), q=ref["q"])})
    torch.cuda.synchronize()
    assert torch.equal(out["q"], ref["q"])  # the lossy fp8 path: the same codes as in A
    assert os.path.exists(os.path.join(B, ".snapshot_bases"))
