"""Incremental takes (``Snapshot.take(base=...)``, engine/incremental.py) on
host tensors: the C++ hasher covers them, so everything here runs on the CPU."""

import contextlib
import json
import os
import shutil

import pytest
import torch

import incremental_workers as W
from hipsnapshot import Snapshot, StateDict, knobs
from hipsnapshot.engine import incremental
from hipsnapshot.ops.checksum import hs64_reference
from hipsnapshot.snapshot import TakeStats
from hipsnapshot.utils.test_utils import run_distributed

# six host tensors of 4-64 KiB; "odd" has a byte count that is no multiple of 8
SIZES = {"a": 4 << 10, "b": 6 << 10, "odd": (5 << 10) + 3, "c": 16 << 10, "d": 40 << 10,
         "e": 64 << 10}
SLAB_ALIGN = 256


def make_state(seed=0):
    g = torch.Generator().manual_seed(seed)
    return StateDict(**{k: torch.randint(0, 256, (n,), dtype=torch.uint8, generator=g)
                        for k, n in SIZES.items()})


def zeros_like_state():
    return StateDict(**{k: torch.zeros(n, dtype=torch.uint8) for k, n in SIZES.items()})


def assert_restores(path, sd):
    out = zeros_like_state()
    Snapshot(path).restore({"sd": out})
    for k in SIZES:
        assert torch.equal(out[k], sd[k]), k


def leaf_entries(path):
    return {k.split("/")[-1]: e for k, e in Snapshot(path).get_manifest().items()
            if hasattr(e, "location")}


def blob_bytes(root):
    total = 0
    for d, _dirs, files in os.walk(root):
        if os.path.basename(d).startswith(".snapshot"):
            continue
        total += sum(os.path.getsize(os.path.join(d, f)) for f in files
                     if not f.startswith(".snapshot"))
    return total


@pytest.fixture(params=[None, 8 << 10], ids=["slabs", "slab_threshold_8k"])
def slab_threshold(request):
    """Default batching (every tensor a slab member), and an 8 KiB slab
    threshold (a, b, odd are slab members; c, d, e are blobs of their own)."""
    cm = knobs.override_slab_size_threshold_bytes(request.param) if request.param \
        else contextlib.nullcontext()
    with cm:
        yield request.param


def test_base_is_a_take_argument(tmp_path):
    """The test that fails without the feature: ``take`` has no ``base``."""
    sd = make_state()
    a = Snapshot.take(str(tmp_path / "A"), {"sd": sd}, content_digests=True)
    b = Snapshot.take(str(tmp_path / "B"), {"sd": sd}, base=a)
    assert all(e.location.startswith("../") for e in leaf_entries(b.path).values())


def test_two_changed_tensors(tmp_path, slab_threshold):
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    sd["b"][17] ^= 0xFF
    sd["d"][-1] ^= 1
    changed = ("b", "d")
    Snapshot.take(B, {"sd": sd}, base=A)
    stats = dict(TakeStats.last)
    entries = leaf_entries(B)
    for k, e in entries.items():
        assert e.location.startswith("../") == (k not in changed), (k, e.location)
    # B holds the changed leaves only: b is alone in its slab, d is a slab
    # member after b (padded to the slab alignment) or a blob of its own
    if slab_threshold is None:
        pad = -SIZES["b"] % SLAB_ALIGN
        assert knobs.slab_align() == SLAB_ALIGN
    else:
        pad = 0
    assert blob_bytes(B) == SIZES["b"] + SIZES["d"] + pad
    assert stats["bytes_reused"] == sum(n for k, n in SIZES.items() if k not in changed)
    assert stats["leaves_reused"] == len(SIZES) - len(changed)
    assert stats["digest_s"] > 0
    assert_restores(B, sd)
    rep = Snapshot(B).verify()
    assert rep.ok and rep.checked == rep.blobs, rep.as_dict()
    assert Snapshot(B).dependencies() == [os.path.realpath(A)]
    # the content file: one record per leaf under its final location, the
    # digest of the raw bytes
    doc = json.loads((tmp_path / "B" / ".snapshot_content" / "0").read_text())
    assert doc["algo"] == "hs64" and len(doc["leaves"]) == len(SIZES)
    for k, e in entries.items():
        assert int(doc["leaves"][incremental.content_key(e)], 16) == \
            hs64_reference(sd[k].numpy()), k


def test_last_byte_of_an_odd_sized_tensor(tmp_path, slab_threshold):
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    assert SIZES["odd"] % 8
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    sd["odd"][-1] ^= 1  # one bit, in the zero-padded tail word
    Snapshot.take(B, {"sd": sd}, base=A)
    entries = leaf_entries(B)
    assert not entries["odd"].location.startswith("../")
    assert all(e.location.startswith("../") for k, e in entries.items() if k != "odd")
    assert_restores(B, sd)


def test_same_values_other_dtype_or_shape(tmp_path, slab_threshold):
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    sd2 = StateDict(**{k: sd[k] for k in SIZES})
    sd2["a"] = sd["a"].view(torch.int8)          # same bytes, another dtype
    sd2["c"] = sd["c"].view(2, -1)               # same bytes, another shape
    Snapshot.take(B, {"sd": sd2}, base=A)
    entries = leaf_entries(B)
    for k, e in entries.items():
        assert e.location.startswith("../") == (k not in ("a", "c")), (k, e.location)
    out = zeros_like_state()
    out["a"] = torch.zeros(SIZES["a"], dtype=torch.int8)
    out["c"] = torch.zeros(2, SIZES["c"] // 2, dtype=torch.uint8)
    Snapshot(B).restore({"sd": out})
    for k in SIZES:
        assert torch.equal(out[k], sd2[k]), k


def test_chain_collapses_into_the_oldest_base(tmp_path, slab_threshold):
    A, B, C = (str(tmp_path / n) for n in "ABC")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    sd["b"][0] ^= 1
    sd["d"][0] ^= 1
    Snapshot.take(B, {"sd": sd}, base=A)
    sd["b"][1] ^= 1
    sd["d"][1] ^= 1
    c = Snapshot.take(C, {"sd": sd}, base=Snapshot(B))
    real_a = os.path.realpath(A)
    reused = [e for e in leaf_entries(C).values() if e.location.startswith("../")]
    assert len(reused) == len(SIZES) - 2
    for e in reused:  # straight into A, no hop through B
        assert os.path.normpath(os.path.join(os.path.realpath(C), e.location)) \
            .startswith(real_a + os.sep), e.location
    assert c.dependencies() == [real_a]
    shutil.rmtree(B)
    assert_restores(C, sd)
    assert Snapshot(C).verify().ok


def test_materialize(tmp_path, slab_threshold):
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    sd["a"][3] ^= 1
    sd["e"][3] ^= 1
    b = Snapshot.take(B, {"sd": sd}, base=A)
    assert b.dependencies() == [os.path.realpath(A)]
    b.materialize()
    assert b.dependencies() == [] and Snapshot(B).dependencies() == []
    assert not os.path.exists(os.path.join(B, ".snapshot_bases"))
    shutil.rmtree(A)
    assert not any(e.location.startswith("../") for e in leaf_entries(B).values())
    assert_restores(B, sd)
    rep = Snapshot(B).verify()
    assert rep.ok and rep.checked == rep.blobs, rep.as_dict()
    # still a full-value base: its content file follows the moved blobs
    sd["c"][0] ^= 1
    Snapshot.take(str(tmp_path / "C"), {"sd": sd}, base=B)
    assert TakeStats.last["leaves_reused"] == len(SIZES) - 1
    assert_restores(str(tmp_path / "C"), sd)


def test_cli_deps_and_materialize(tmp_path, capsys):
    from hipsnapshot.__main__ import main

    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    Snapshot.take(B, {"sd": sd}, base=A)
    assert main(["deps", B]) == 0
    assert capsys.readouterr().out.split() == [os.path.realpath(A)]
    assert main(["materialize", B]) == 0
    capsys.readouterr()
    assert main(["deps", B]) == 0
    assert capsys.readouterr().out.strip() == ""


def test_checksum_fallback_for_a_base_without_content(tmp_path):
    """A base taken without content digests: whole-file raw leaves match
    through their blob checksum, slab members have no digest and are
    rewritten."""
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    with knobs.override_slab_size_threshold_bytes(8 << 10):
        Snapshot.take(A, {"sd": sd})
        assert not os.path.exists(os.path.join(A, ".snapshot_content"))
        Snapshot.take(B, {"sd": sd}, base=A)
    entries = leaf_entries(B)
    for k in ("c", "d", "e"):
        assert entries[k].location.startswith("../"), k
    for k in ("a", "b", "odd"):
        assert not entries[k].location.startswith("../"), k
    assert TakeStats.last["bytes_reused"] == SIZES["c"] + SIZES["d"] + SIZES["e"]
    assert_restores(B, sd)
    assert Snapshot(B).verify().ok


def test_bad_bases_raise_before_anything_is_written(tmp_path):
    A = str(tmp_path / "A")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    with pytest.raises(ValueError):  # base == path (the committed A stays as it is)
        Snapshot.take(os.path.join(str(tmp_path), ".", "A"), {"sd": sd}, base=A)
    assert_restores(A, sd)
    uncommitted = tmp_path / "U"
    uncommitted.mkdir()
    cases = [str(uncommitted), str(tmp_path / "missing"), "memory://bucket/base"]
    for i, base in enumerate(cases):
        new = tmp_path / f"N{i}"
        with pytest.raises(ValueError):
            Snapshot.take(str(new), {"sd": sd}, base=base)
        assert not new.exists(), base
    with pytest.raises(ValueError):  # the new snapshot is not on the fs plugin either
        Snapshot.take("memory://bucket/new", {"sd": sd}, base=A)


def test_async_take_has_no_base():
    import inspect

    assert "base" not in inspect.signature(Snapshot.async_take).parameters


def test_plain_take_after_an_incremental_one(tmp_path):
    """Neither the plan cache nor the entry objects carry rewritten locations
    into a later plain take."""
    A, B, P = (str(tmp_path / n) for n in "ABP")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    Snapshot.take(B, {"sd": sd}, base=A)
    Snapshot.take(P, {"sd": sd})
    assert not any(e.location.startswith("../") for e in leaf_entries(P).values())
    assert "../" not in (tmp_path / "P" / ".snapshot_metadata").read_text()
    assert blob_bytes(P) >= sum(SIZES.values())
    assert_restores(P, sd)


def test_no_side_files_by_default(tmp_path):
    assert not knobs.content_digests_enabled()
    P = tmp_path / "P"
    Snapshot.take(str(P), {"sd": make_state()})
    assert sorted(f for f in os.listdir(P) if f.startswith(".snapshot")) == \
        [".snapshot_checksums", ".snapshot_metadata"]
    assert "bytes_reused" not in TakeStats.last
    assert Snapshot(str(P)).dependencies() == []


def test_knob_turns_content_digests_on(tmp_path):
    P = tmp_path / "P"
    with knobs.override_knob("CONTENT_DIGESTS", True):
        Snapshot.take(str(P), {"sd": make_state()})
    assert (P / ".snapshot_content" / "0").exists()
    assert not (P / ".snapshot_bases").exists()


def test_plain_retake_removes_stale_side_files(tmp_path):
    """A plain take over an incremental snapshot must not leave the old
    content digests (they would describe blobs that were replaced)."""
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    Snapshot.take(B, {"sd": sd}, base=A)
    sd["a"][0] ^= 1
    Snapshot.take(B, {"sd": sd})
    assert not os.path.exists(os.path.join(B, ".snapshot_content"))
    assert not os.path.exists(os.path.join(B, ".snapshot_bases"))
    assert Snapshot(B).dependencies() == []
    assert_restores(B, sd)


def test_failed_coalesce_keeps_an_incremental_snapshot_whole(tmp_path, monkeypatch):
    """A take that fails in the coalesce gather has written nothing: the
    incremental snapshot at its path keeps its side files, so
    ``dependencies()`` still guards the base."""
    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    sd["a"][0] ^= 1
    Snapshot.take(B, {"sd": sd}, base=A)
    content = (tmp_path / "B" / ".snapshot_content" / "0").read_text()

    def boom(*a, **k):
        raise RuntimeError("coalesce failed")

    monkeypatch.setattr(Snapshot, "_coalesce", classmethod(boom))
    for kw in ({}, {"content_digests": True}, {"base": A}):
        with pytest.raises(RuntimeError, match="coalesce failed"):
            Snapshot.take(B, {"sd": make_state(1)}, **kw)
        assert Snapshot(B).dependencies() == [os.path.realpath(A)], kw
        assert (tmp_path / "B" / ".snapshot_content" / "0").read_text() == content, kw
    monkeypatch.undo()
    assert_restores(B, sd)
    assert Snapshot(B).verify().ok
    Snapshot(B).materialize()
    assert sorted(os.listdir(os.path.join(B, "external"))) == ["0"]


def test_interrupted_materialize_still_verifies_and_reruns(tmp_path, monkeypatch):
    from hipsnapshot.storage.fs import FSStoragePlugin

    A, B = str(tmp_path / "A"), str(tmp_path / "B")
    sd = make_state()
    Snapshot.take(A, {"sd": sd}, content_digests=True)
    sd["a"][0] ^= 1
    Snapshot.take(B, {"sd": sd}, base=A)

    async def crash(self, path, buf):
        raise OSError("interrupted before the commit")

    monkeypatch.setattr(FSStoragePlugin, "commit_metadata", crash)
    with pytest.raises(OSError, match="interrupted"):
        Snapshot(B).materialize()
    monkeypatch.undo()
    assert Snapshot(B).dependencies() == [os.path.realpath(A)]
    assert_restores(B, sd)
    assert Snapshot(B).verify().ok  # the old locations still have their checksums
    Snapshot(B).materialize()
    shutil.rmtree(A)
    assert Snapshot(B).dependencies() == []
    assert_restores(B, sd)
    rep = Snapshot(B).verify()
    assert rep.ok and rep.checked == rep.blobs
    for side in (".snapshot_checksums", ".snapshot_content"):
        assert "../" not in (tmp_path / "B" / side / "0").read_text(), side


def test_content_files_of_ranks_that_are_gone_are_removed(tmp_path):
    P = tmp_path / "P"
    sd = make_state()
    Snapshot.take(str(P), {"sd": sd}, content_digests=True)
    (P / ".snapshot_content" / "3").write_text('{"algo": "hs64", "leaves": {}}')
    Snapshot.take(str(P), {"sd": sd}, content_digests=True)
    assert os.listdir(P / ".snapshot_content") == ["0"]


def test_owning_root(tmp_path):
    A = str(tmp_path / "A")
    Snapshot.take(A, {"sd": make_state()})
    blob = os.path.join(A, "batched", "x")
    assert incremental.owning_root(blob, [A]) == A
    assert incremental.owning_root(blob, []) == A  # the directory with the metadata
    with pytest.raises(RuntimeError):
        incremental.owning_root(str(tmp_path / "nowhere" / "0" / "x"), [A])


@pytest.mark.multiproc
def test_two_ranks_replicated_state(tmp_path):
    run_distributed(W.ddp_incremental, 2, str(tmp_path))


@pytest.mark.multiproc
def test_two_ranks_mismatched_bases(tmp_path):
    run_distributed(W.mismatched_bases, 2, str(tmp_path))
