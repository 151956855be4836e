"""Incremental takes: leaves unchanged since a base snapshot are not written.

Not in the reference.  ``Snapshot.take(path, app_state, base=B)`` hashes every
eligible leaf tensor of the take where it lives -- HBM leaves of a device by
ONE ``hs_hash64_batch`` launch (csrc/hshash.hip), host leaves by the C++ hasher
-- *before* anything is staged, and compares each digest with the one the base
recorded for the same leaf.  A leaf whose digest, byte count, dtype and shape
all match is neither staged, copied nor written: its manifest entry points at
the base's blob through a relative ``location`` (``../B/0/model/w``), which the
storage plugin and the native restore resolve like any other location.  Only
the leaves that remain are packed into slabs, compressed and written.

Matching is per leaf, not per blob file: with the default 128 MiB slab
threshold almost every tensor of a training state is a slab member, so the
blob checksums of ``.snapshot_checksums`` would match almost nothing.

Side files of a snapshot (JSON, next to ``.snapshot_metadata``):

``.snapshot_content/<rank>``
    ``{"algo": "hs64", "leaves": {key: hex}}`` -- hs64 of each eligible leaf's
    raw logical bytes (C order, before any HSZ1 encoding).  ``key`` is the
    leaf's final ``TensorEntry.location``, plus ``#<start>-<end>`` when the
    entry has a ``byte_range``.  Reused leaves are recorded under their
    rewritten location, so an incremental snapshot is a full-value base.
``.snapshot_bases``
    JSON list of the snapshot directories (relative to this one) this
    snapshot's entries point into; absent when it is self-contained.

hs64 is a 64-bit, non-cryptographic hash: ``mix64`` is a bijection and every
word is keyed by its index, so a change confined to one 8-byte word always
changes the sum; wider changes collide with probability 2^-64.
"""

from __future__ import annotations

import fnmatch
import json
import os
import shutil
import time
from typing import Any, Dict, List, Optional, Tuple

import torch

from ..format.manifest import (
    ChunkedTensorEntry,
    Entry,
    ShardedTensorEntry,
    SnapshotMetadata,
    TensorEntry,
    iter_tensor_entries,
)
from ..format.serialization import SER
from ..io_types import WriteReq
from ..ops import checksum

CONTENT_DIR = ".snapshot_content"
BASES_FNAME = ".snapshot_bases"
METADATA_FNAME = ".snapshot_metadata"
EXTERNAL_DIR = "external"  # where ``materialize`` puts the blobs it brings in


def content_file(rank: int) -> str:
    return f"{CONTENT_DIR}/{rank}"


def content_key(entry: TensorEntry) -> str:
    if entry.byte_range is None:
        return entry.location
    return f"{entry.location}#{int(entry.byte_range[0])}-{int(entry.byte_range[1])}"


def is_external(location: str) -> bool:
    return location == ".." or location.startswith("../")


def fs_root(url: str) -> Optional[str]:
    """The real directory of an ``fs`` snapshot URL; None for other plugins."""
    from ..storage.registry import split_url

    protocol, root = split_url(url)
    return os.path.realpath(root) if protocol == "fs" else None


def resolve_base(base: Any, path: str) -> str:
    """The base's directory, checked: an ``fs`` snapshot that is committed and
    is not ``path`` itself (raises ``ValueError`` before the take writes)."""
    base_url = getattr(base, "path", base)
    if not isinstance(base_url, str):
        raise ValueError(f"base must be a Snapshot or a path string, got {type(base)!r}")
    root, base_root = fs_root(path), fs_root(base_url)
    if root is None or base_root is None:
        raise ValueError("an incremental take needs the base and the new snapshot on the "
                         f"local 'fs' storage plugin (base={base_url!r}, path={path!r})")
    if base_root == root:
        raise ValueError(f"base and path are the same snapshot: {root}")
    if not os.path.isfile(os.path.join(base_root, METADATA_FNAME)):
        raise ValueError(f"base {base_root} is not a committed snapshot "
                         f"(no {METADATA_FNAME})")
    if root in read_dependencies(base_root):
        raise ValueError(f"base {base_root} points into {root}: a take there would "
                         "overwrite blobs the base needs")
    return base_root


def _read_json(path: str) -> Optional[Any]:
    try:
        with open(path, "rb") as f:
            return json.loads(f.read().decode("utf-8"))
    except FileNotFoundError:
        return None


def read_dependencies(root: str) -> List[str]:
    doc = _read_json(os.path.join(root, BASES_FNAME)) or []
    return [os.path.normpath(os.path.join(root, d)) for d in doc]


def owning_root(target: str, roots: List[str]) -> str:
    """The snapshot directory that holds the blob ``target``: the longest of
    the known ``roots`` above it (a base nested in another's directory wins),
    else the nearest directory above it with a ``.snapshot_metadata``."""
    for r in sorted(roots, key=len, reverse=True):
        if target.startswith(r + os.sep):
            return r
    d = os.path.dirname(target)
    while d and d != os.path.dirname(d):
        if os.path.isfile(os.path.join(d, METADATA_FNAME)):
            return d
        d = os.path.dirname(d)
    raise RuntimeError(f"{target} lies in no snapshot directory")


class BaseIndex:
    """What a take needs of its base: the manifest, the content digests of
    all ranks (they are small, every rank loads them all), the blob checksums
    and the base's own bases."""

    def __init__(self, root: str) -> None:
        from ..snapshot import Snapshot

        self.root = root
        self.metadata: SnapshotMetadata = Snapshot(root).metadata
        ws = self.metadata.world_size
        self.content: Dict[str, int] = {}
        self.sums: Dict[str, int] = {}
        for r in range(ws):
            doc = _read_json(os.path.join(root, content_file(r)))
            if doc is not None:
                if doc.get("algo") != checksum.ALGO:
                    raise ValueError(f"unknown content digest algorithm {doc.get('algo')!r}")
                self.content.update((k, int(h, 16)) for k, h in doc["leaves"].items())
            doc = _read_json(os.path.join(root, checksum.rank_file(r)))
            if doc is not None and doc.get("algo") == checksum.ALGO:
                self.sums.update((k, int(h, 16)) for k, h in doc["blobs"].items())
        self.roots = [root] + read_dependencies(root)
        self._manifests: Dict[int, Dict[str, Entry]] = {}

    def manifest_for(self, rank: int) -> Dict[str, Entry]:
        m = self._manifests.get(rank)
        if m is None:
            from ..parallel.elasticity import get_manifest_for_rank

            local, merged = get_manifest_for_rank(self.metadata, rank)
            m = dict(merged)
            m.update(local)
            self._manifests[rank] = m
        return m

    def digest_of(self, be: TensorEntry) -> Optional[int]:
        d = self.content.get(content_key(be))
        if d is None and be.byte_range is None and be.codec is None \
                and be.serializer == SER.BUFFER_PROTOCOL:
            # a whole-file raw blob: its blob checksum is the content digest
            d = self.sums.get(be.location)
        return d


def _pieces(entry: Entry):
    """(tensor entry, piece id) of every blob descriptor of a leaf's entry."""
    if isinstance(entry, TensorEntry):
        yield entry, None
    elif isinstance(entry, ChunkedTensorEntry):
        for c in entry.chunks:
            yield c.tensor, ("chunk", tuple(c.offsets), tuple(c.sizes))
    elif isinstance(entry, ShardedTensorEntry):
        for s in entry.shards:
            yield s.tensor, ("shard", tuple(s.offsets), tuple(s.sizes))


def _base_piece(base_entry: Optional[Entry], entry: Entry, piece) -> Optional[TensorEntry]:
    """The base's tensor entry of the same piece of the same kind of leaf."""
    if base_entry is None or type(base_entry) is not type(entry):
        return None
    if isinstance(entry, ChunkedTensorEntry) and (
            base_entry.dtype != entry.dtype or list(base_entry.shape) != list(entry.shape)):
        return None
    for te, pid in _pieces(base_entry):
        if pid == piece:
            return te
    return None


def eligible(stager, logical: str, quantize: Optional[List[str]]) -> bool:
    from ..io.tensor import TensorBufferStager, is_uvm_like

    if not isinstance(stager, TensorBufferStager) or stager._tensor_prepare_func is not None:
        return False
    if stager.entry.serializer != SER.BUFFER_PROTOCOL:
        return False
    if quantize and any(fnmatch.fnmatch(logical, p) for p in quantize):
        return False
    t = stager.tensor
    if t.layout != torch.strided or not t.is_contiguous():
        return False
    if t.is_cuda:
        return not is_uvm_like(t)
    return t.device.type == "cpu"


class IncrementalTake:
    """One take's content digests and, with a base, its reuse decisions."""

    def __init__(self, path: str, base_root: Optional[str]) -> None:
        self.root = fs_root(path)
        self.base = BaseIndex(base_root) if base_root is not None else None
        self.digests: List[Tuple[TensorEntry, int]] = []  # every eligible leaf
        self.reused_sums: Dict[str, int] = {}  # rewritten location -> blob checksum
        self.bytes_reused = 0
        self.leaves_reused = 0
        self.digest_s = 0.0

    BASES_FNAME = BASES_FNAME

    @staticmethod
    def content_path(rank: int) -> str:
        return content_file(rank)

    # -- hashing ---------------------------------------------------------------

    @staticmethod
    def _hash(stagers) -> List[int]:
        from .scheduler import aux_pool
        from .staging import device_of

        out: List[Optional[int]] = [None] * len(stagers)
        by_dev: Dict[int, List[int]] = {}
        host: List[int] = []
        for i, st in enumerate(stagers):
            t = st.tensor
            if t.is_cuda:
                by_dev.setdefault(device_of(t), []).append(i)
            else:
                host.append(i)

        def host_hash(i: int) -> int:
            t = stagers[i].tensor
            nb = t.numel() * t.element_size()
            return checksum.hs64_host(t.data_ptr() if nb else 0, nb, 2)

        # the host leaves hash on the pool while the device launches run
        futs = [(i, aux_pool().submit(host_hash, i)) for i in host]
        for dev, idxs in by_dev.items():
            blobs = [(stagers[i].tensor.data_ptr(),
                      stagers[i].tensor.numel() * stagers[i].tensor.element_size())
                     for i in idxs]
            for i, h in zip(idxs, checksum.device_hash_batch(dev, blobs)):
                out[i] = h
        for i, f in futs:
            out[i] = f.result()
        return out  # type: ignore[return-value]

    # -- planning --------------------------------------------------------------

    def plan(self, object_entries: Dict[str, Entry], path_reqs: Dict[str, List[WriteReq]],
             rank: int, quantize: Optional[List[str]]) -> None:
        """Hash the eligible leaves this rank would write and, with a base,
        take the unchanged ones out of ``path_reqs`` (their entries are
        re-pointed at the base's blobs in place)."""
        from ..io.tensor import tensor_nbytes_from_entry

        t0 = time.perf_counter()
        found = []  # (logical, write request, top entry, piece id)
        for logical, wrs in path_reqs.items():
            top = object_entries.get(logical)
            if top is None:
                continue
            pid_of = {id(te): pid for te, pid in _pieces(top)}
            for wr in wrs:
                st = wr.buffer_stager
                if eligible(st, logical, quantize) and id(st.entry) in pid_of:
                    found.append((logical, wr, top, pid_of[id(st.entry)]))
        hashes = self._hash([wr.buffer_stager for _, wr, _, _ in found])
        self.digest_s = time.perf_counter() - t0
        base_manifest = self.base.manifest_for(rank) if self.base is not None else None
        dropped = set()
        for (logical, wr, top, pid), digest in zip(found, hashes):
            te = wr.buffer_stager.entry
            self.digests.append((te, digest))
            if base_manifest is None:
                continue
            be = _base_piece(base_manifest.get(logical), top, pid)
            if be is None or be.serializer != SER.BUFFER_PROTOCOL or be.dtype != te.dtype \
                    or list(be.shape) != list(te.shape) or be.quant is not None:
                continue
            t = wr.buffer_stager.tensor
            nbytes = t.numel() * t.element_size()
            if self.base.digest_of(be) != digest or tensor_nbytes_from_entry(be) != nbytes:
                continue
            target = os.path.normpath(os.path.join(self.base.root, be.location))
            te.location = os.path.relpath(target, self.root)
            te.byte_range = None if be.byte_range is None else [int(x) for x in be.byte_range]
            te.codec = None if be.codec is None else dict(be.codec)
            blob_sum = self.base.sums.get(be.location)
            if blob_sum is not None:
                self.reused_sums[te.location] = blob_sum
            self.bytes_reused += nbytes
            self.leaves_reused += 1
            dropped.add(id(wr))
        if dropped:
            for logical in list(path_reqs):
                path_reqs[logical] = [wr for wr in path_reqs[logical] if id(wr) not in dropped]

    # -- side files ------------------------------------------------------------

    def content_doc(self) -> bytes:
        leaves = {content_key(te): checksum.to_hex(h) for te, h in self.digests}
        return json.dumps({"algo": checksum.ALGO, "leaves": dict(sorted(leaves.items()))}
                          ).encode("utf-8")

    def bases_doc(self, manifest: Dict[str, Entry]) -> Optional[bytes]:
        """``.snapshot_bases`` of the committed manifest (rank 0): the base
        roots that some entry of some rank points into; None when none does."""
        if self.base is None:
            return None
        used = set()
        for e in manifest.values():
            for te in iter_tensor_entries(e):
                if is_external(te.location):
                    target = os.path.normpath(os.path.join(self.root, te.location))
                    used.add(owning_root(target, self.base.roots))
        if not used:
            return None
        return json.dumps(sorted(os.path.relpath(r, self.root) for r in used)).encode("utf-8")

    def drop_content_beyond(self, world_size: int) -> None:
        """Remove the content files of ranks an earlier, larger take at this
        path had (rank 0, after the commit; readers never look at them)."""
        d = os.path.join(self.root, CONTENT_DIR) if self.root is not None else None
        if d is None or not os.path.isdir(d):
            return
        for name in os.listdir(d):
            if name.isdigit() and int(name) >= world_size:
                try:
                    os.remove(os.path.join(d, name))
                except OSError:
                    pass


# -- retention -------------------------------------------------------------------

def _link_or_copy(src: str, dst: str) -> None:
    os.makedirs(os.path.dirname(dst), exist_ok=True)
    tmp = f"{dst}.tmp.{os.getpid()}"
    try:
        os.link(src, tmp)
    except OSError:
        shutil.copyfile(src, tmp)
    os.replace(tmp, dst)


def _rewrite_keys(path: str, field: str, moved: Dict[str, str], keep_old: bool) -> None:
    """Re-key a checksum / content file after blobs moved.  ``keep_old``: the
    records are kept under their old key as well (until the metadata that
    names the new locations is committed)."""
    doc = _read_json(path)
    if doc is None:
        return
    out = {}
    for k, v in doc[field].items():
        loc, sep, rng = k.partition("#")
        if loc in moved:
            out[moved[loc] + sep + rng] = v
            if not keep_old:
                continue
        out[k] = v
    doc[field] = out
    tmp = f"{path}.tmp.{os.getpid()}"
    with open(tmp, "wb") as f:
        f.write(json.dumps(doc).encode("utf-8"))
    os.replace(tmp, path)


def materialize(root: str, storage_options: Optional[Dict[str, Any]] = None) -> int:
    """Make the committed ``fs`` snapshot at ``root`` self-contained: bring
    every blob it references outside its directory in (hard link, or a copy
    where linking fails; whole files -- a base slab with one live member comes
    whole), re-point the metadata, checksum and content files at the local
    copies, commit the metadata atomically and remove ``.snapshot_bases``.
    Returns the number of blobs brought in.

    Every step leaves a snapshot that restores and verifies: the blobs come in
    first, the checksum and content files then carry each record under its old
    and its new key, the metadata commit switches the locations, and only
    then do the old keys and ``.snapshot_bases`` go.  After an interruption,
    run it again."""
    import asyncio

    from ..io_types import ReadIO, run_sync
    from ..storage.registry import url_to_storage_plugin_in_event_loop

    loop = asyncio.new_event_loop()
    storage = url_to_storage_plugin_in_event_loop(root, loop, storage_options)
    try:
        rio = ReadIO(path=METADATA_FNAME)
        storage.sync_read(rio, loop)
        md = SnapshotMetadata.from_json(bytes(rio.data()).decode("utf-8"))
        roots = read_dependencies(root)
        numbered = {r: i for i, r in enumerate(sorted(roots))}
        moved: Dict[str, str] = {}
        for e in md.manifest.values():
            for te in iter_tensor_entries(e):
                if not is_external(te.location):
                    continue
                new = moved.get(te.location)
                if new is None:
                    src = os.path.normpath(os.path.join(root, te.location))
                    owner = owning_root(src, roots)
                    k = numbered.setdefault(owner, len(numbered))
                    new = f"{EXTERNAL_DIR}/{k}/{os.path.relpath(src, owner)}"
                    _link_or_copy(src, os.path.join(root, new))
                    moved[te.location] = new
                te.location = new
        side = [(os.path.join(root, checksum.rank_file(r)), "blobs")
                for r in range(md.world_size)]
        side += [(os.path.join(root, content_file(r)), "leaves") for r in range(md.world_size)]
        if moved:
            for path, field in side:
                _rewrite_keys(path, field, moved, keep_old=True)
            run_sync(loop, storage.commit_metadata(METADATA_FNAME,
                                                   md.to_json().encode("utf-8")))
            for path, field in side:
                _rewrite_keys(path, field, moved, keep_old=False)
        try:
            os.remove(os.path.join(root, BASES_FNAME))
        except FileNotFoundError:
            pass
        return len(moved)
    finally:
        storage.sync_close(loop)
        loop.close()
