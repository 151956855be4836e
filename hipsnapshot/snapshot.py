"""``Snapshot`` / ``PendingSnapshot``: the public take / async_take / restore API.

Behavioural reference: `/root/reference/torchsnapshot/snapshot.py:66-947`
(API surface, replicated/sharded/per-rank semantics, RNG invariants, commit
protocol).  Orchestration differences on MI355X:

* path, replication globs, app-state keys, hostnames and a commit nonce are
  exchanged in ONE object all-gather (reference: broadcast + 2 all-gathers);
  replicated-path verification and write partitioning are single all-gathers
  whose result every rank computes identically (no follow-up broadcast), so a
  take issues 4 metadata collectives + K per-key barriers + 2 commit barriers
  (before rank 0 writes the metadata, and after, so that take() returns on
  every rank only once the snapshot is readable).  The K per-key barriers are
  skipped when no rank's ``state_dict()`` can run a collective
  (``knobs.get_state_dict_barriers``).
* ``async_take`` runs ONE collective before returning (the coalesce
  all-gather; DDP-replicated state adds the partition gathers): the manifest
  exchange moved into the commit thread, through the c10d store (rank 0
  assembles the metadata after the commit barrier), so the unblock path does
  not grow with the rank count.
* ``async_take`` freezes all HBM-resident state with ONE gather-kernel launch
  into a spare-HBM arena (enqueued on the trainer's stream, so no host sync
  is needed for consistency) and returns; D2H + storage writes drain in the
  background.  When HBM is short it falls back to staging into pinned host
  memory before returning (reference semantics).
* the commit (``.snapshot_metadata``) is written atomically (temp + rename on
  file systems) only after every rank finished writing.
"""

from __future__ import annotations

import asyncio
import copy
import fnmatch
import functools
import itertools
import json
import logging
import os
import socket
import sys
import threading
import time
import traceback
import uuid
import weakref
from datetime import timedelta
from typing import Any, Callable, Dict, List, Optional, Set, Tuple, TypeVar

import torch
import torch.distributed as dist
from torch.nn.parallel import DistributedDataParallel as DDP

from . import knobs
from .engine import memory, native_restore, restore_cache, staging
from .engine.scheduler import (
    PendingIOWork,
    get_process_memory_budget_bytes,
    _budget_cache,
    sync_execute_read_reqs,
    sync_execute_write_reqs,
)
from .format.flatten import flatten, inflate
from .format.manifest import (
    Entry,
    LazySnapshotMetadata,
    PrimitiveEntry,
    ShardedTensorEntry,
    SnapshotMetadata,
    entry_json,
    is_container_entry,
    is_replicated,
    metadata_json_from_parts,
)
from .io.batcher import batch_read_requests, batch_write_requests
from .io.preparer import prepare_read, prepare_write
from .io.sharded import is_sharded
from .io_types import ReadIO, ReadReq, StoragePlugin, WriteIO, WriteReq, run_sync
from .ops import checksum, native
from .parallel.comm import Comm
from .parallel.elasticity import get_manifest_for_rank, handle_sharded_tensor_elasticity
from .parallel.partitioner import (
    consolidate_replicated_entries,
    partition_write_reqs,
    replicated_chunk_bytes,
)
from .parallel.store import LinearBarrier, existing_store, get_or_create_store
from .stateful import AppState, RNGState, Stateful
from .storage.fs import FSStoragePlugin as _FSStoragePlugin
from .storage.registry import url_to_storage_plugin_in_event_loop
from .utils.tracing import paused_gc, roctx_range, timeline
from .version import __version__

logger = logging.getLogger(__name__)

SNAPSHOT_METADATA_FNAME = ".snapshot_metadata"
T = TypeVar("T")
PrepareFunc = Callable[[str, torch.Tensor, bool], torch.Tensor]


class TakeStats:
    """Timings of the last take on this process (for benchmarks/observability)."""

    last: Dict[str, float] = {}


def _state_dict_view(stateful: Any) -> Any:
    """``stateful.state_dict()`` for a take or a restore.

    For an ``nn.Module`` whose class keeps ``nn.Module.state_dict`` (FSDP2
    modules included) this is ``state_dict(keep_vars=True)`` with plain
    tensors detached afterwards: DTensor parameters are kept as they are (the
    snapshot only reads and writes their local tensors, which do not require
    grad), which skips one DTensor-dispatched ``detach`` per parameter --
    ~25 us each, 291 of them for Llama-3-8B, on every take and restore.  On
    restore the read consumers fill ``_local_tensor`` in place, and the final
    ``load_state_dict`` copies each DTensor parameter onto itself, which
    ``copy_`` skips (same tensor); plain tensors are detached views, so the
    worker threads can write into them without ``no_grad``.
    """
    import torch.nn as nn

    if not (isinstance(stateful, nn.Module) and type(stateful).state_dict is nn.Module.state_dict):
        return stateful.state_dict()
    from torch.distributed.tensor import DTensor

    sd = _plain_state_dict(stateful)
    if sd is None:
        sd = stateful.state_dict(keep_vars=True)
    for k, v in sd.items():
        if type(v) is not DTensor and isinstance(v, torch.Tensor) and v.requires_grad \
                and not isinstance(v, DTensor):
            sd[k] = v.detach()
    return sd


def _materialize_optimizer_state(optim: "torch.optim.Optimizer") -> bool:
    """Create a fresh optimizer's state tensors so sharded (DTensor) state can
    be restored into them.

    A snapshot's sharded optimizer state is read into tensors of the current
    layout, and a fresh optimizer has none: it creates them at its first
    step.  That step is run here with zero gradients and a zero learning
    rate. The parameters do not move (lr 0 scales every update and the
    decoupled weight decay to nothing), and the state appears in the
    parameters' own sharding, as after a training step.  The restore then
    overwrites every value.  Skipped, returning False, when a parameter
    already holds a gradient."""
    params = [p for g in optim.param_groups for p in g["params"]]
    if any(p.grad is not None for p in params):
        return False
    saved = []
    for g in optim.param_groups:
        lr = g.get("lr")
        saved.append(lr)
        if lr is not None:
            g["lr"] = torch.zeros_like(lr) if isinstance(lr, torch.Tensor) else 0.0
    try:
        with torch.no_grad():
            for p in params:
                if p.requires_grad:
                    p.grad = torch.zeros_like(p)
        # the class's own step, without the registered step hooks (an EMA or
        # a logger hooked on steps must not see this one)
        raw = getattr(type(optim).step, "__wrapped__", None)
        if raw is not None:
            raw(optim)
        else:
            optim.step()
    except Exception as e:  # noqa: BLE001 - e.g. an optimizer whose step needs a closure
        logger.warning(f"could not create {type(optim).__name__} state before restoring "
                       f"it: {e}")
        return False
    finally:
        for p in params:
            p.grad = None
        for g, lr in zip(optim.param_groups, saved):
            if lr is not None:
                g["lr"] = lr
    return True


_PLAIN_SD_CLASS: Dict[type, bool] = {}


def _plain_sd_class(cls: type) -> bool:
    hit = _PLAIN_SD_CLASS.get(cls)
    if hit is None:
        import torch.nn as nn

        M = nn.Module
        hit = _PLAIN_SD_CLASS[cls] = (
            cls.state_dict is M.state_dict and cls._save_to_state_dict is M._save_to_state_dict
            and getattr(cls, "get_extra_state", M.get_extra_state) is M.get_extra_state)
    return hit


def _tree_plain(root: Any) -> bool:
    stack = [root]
    while stack:
        m = stack.pop()
        if not _plain_sd_class(type(m)) or m._state_dict_hooks:
            return False
        stack.extend(c for c in m._modules.values() if c is not None)
    return True


_plain_roots: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _plain_state_dict(root: Any) -> Optional["OrderedDict"]:
    """``root.state_dict(keep_vars=True)`` built by one iterative walk, when
    every module in the tree keeps ``nn.Module``'s state_dict machinery (no
    overrides, no extra state, no post hooks -- FSDP2 registers pre hooks
    only, which run here as nn.Module runs them); None otherwise.  Same
    entries, order and ``_metadata``, without a Python call frame, metadata
    dict and hook loops per module (a Llama-3-8B has 389 modules).  Whether
    the tree qualifies is checked once per root; a module that stops
    qualifying later is caught during the walk."""
    from collections import OrderedDict

    ok = _plain_roots.get(root)
    if ok is None:
        ok = _plain_roots[root] = _tree_plain(root)
    if not ok:
        return None
    dest: "OrderedDict" = OrderedDict()
    meta: "OrderedDict" = OrderedDict()
    dest._metadata = meta  # type: ignore[attr-defined]
    stack = [(root, "")]
    while stack:
        m, prefix = stack.pop()
        if not _plain_sd_class(type(m)) or m._state_dict_hooks:
            _plain_roots[root] = False
            return None
        meta[prefix[:-1]] = {"version": m._version}
        hooks = m._state_dict_pre_hooks
        if hooks:
            for hook in hooks.values():
                hook(m, prefix, True)
        for name, p in m._parameters.items():
            if p is not None:
                dest[prefix + name] = p
        if m._buffers:
            npb = m._non_persistent_buffers_set
            for name, b in m._buffers.items():
                if b is not None and name not in npb:
                    dest[prefix + name] = b
        kids = m._modules
        if kids:
            stack.extend((c, f"{prefix}{n}.") for n, c in reversed(kids.items()) if c is not None)
    return dest


_module_local: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _state_dict_is_local(stateful: Any) -> bool:
    """True when ``stateful.state_dict()`` is known to issue no collective:
    StateDict / RNGState, optimizers, and modules that keep
    ``nn.Module.state_dict`` and contain no FSDP1 wrapper (whose full state
    dicts all-gather).  FSDP2 (``fully_shard``) and DDP modules qualify.
    A module's answer is kept (walking a Llama's modules costs ~0.4 ms of
    every take's unblock path; a job does not wrap submodules in FSDP1 after
    it started checkpointing)."""
    import torch.nn as nn

    from .stateful import StateDict

    if isinstance(stateful, RNGState):
        return True
    # a subclass that overrides state_dict (a sharded optimizer that gathers)
    # keeps the per-key barrier
    if isinstance(stateful, StateDict):
        return type(stateful).state_dict is StateDict.state_dict
    if isinstance(stateful, torch.optim.Optimizer):
        return type(stateful).state_dict is torch.optim.Optimizer.state_dict
    if isinstance(stateful, nn.Module) and type(stateful).state_dict is nn.Module.state_dict:
        hit = _module_local.get(stateful)
        if hit is not None:
            return hit
        try:
            from torch.distributed.fsdp import FullyShardedDataParallel as FSDP1
        except Exception:  # pragma: no cover
            return True
        local = not any(isinstance(m, FSDP1) for m in stateful.modules())
        _module_local[stateful] = local
        return local
    return False


# FSDP2's own load_state_dict hooks (torch/distributed/fsdp/_fully_shard/):
# the pre-hook reshards (a no-op once ``state_dict`` ran for the restore
# plan) and the post-hook re-points the sharded parameter at its local
# tensor (a no-op when that tensor is the one restored in place)
_NOOP_LOAD_HOOKS = ("FSDPParamGroup._register_state_dict_hooks.<locals>.to_sharded_hook",
                    "FSDPParam.__init__.<locals>.<lambda>")
_module_plain_load: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _inplace_load_noop(stateful: Any) -> bool:
    """True when ``stateful.load_state_dict`` of its own tensors is a no-op:
    a plain module (``_plain_module_load``) or a StateDict (whose
    load_state_dict only re-inserts the same objects)."""
    from .stateful import StateDict

    if isinstance(stateful, StateDict):
        return type(stateful).load_state_dict is StateDict.load_state_dict
    return _plain_module_load(stateful)


def _plain_module_load(module: Any) -> bool:
    """True when ``module.load_state_dict`` does nothing beyond copying each
    state-dict tensor into the module's own tensor: nn.Module's own
    load_state_dict / _load_from_state_dict / set_extra_state in every
    submodule and no load hooks other than FSDP2's no-op ones.  Kept per
    module like ``_module_local``."""
    import torch.nn as nn

    if not isinstance(module, nn.Module) or \
            type(module).load_state_dict is not nn.Module.load_state_dict:
        return False
    hit = _module_plain_load.get(module)
    if hit is not None:
        return hit

    def known(h) -> bool:
        h = getattr(h, "hook", h)  # _WrappedHook of _register_load_state_dict_pre_hook
        return getattr(h, "__module__", "").startswith("torch.distributed.fsdp._fully_shard") \
            and getattr(h, "__qualname__", "") in _NOOP_LOAD_HOOKS

    ok = True
    for m in module.modules():
        t = type(m)
        if t._load_from_state_dict is not nn.Module._load_from_state_dict or \
                t.set_extra_state is not nn.Module.set_extra_state or \
                not all(known(h) for h in m._load_state_dict_pre_hooks.values()) or \
                not all(known(h) for h in m._load_state_dict_post_hooks.values()):
            ok = False
            break
    _module_plain_load[module] = ok
    return ok


_avail_mem = [0, -1e9]  # [bytes available, time.monotonic() of the reading]


class Snapshot:
    """A persisted program state at one point in time.

    ::

        app_state = {"model": model, "optim": optim, "progress": StateDict(step=0)}
        snapshot = Snapshot.take(path="/ckpt/step_100", app_state=app_state)
        ...
        Snapshot(path="/ckpt/step_100").restore(app_state)

    Every persisted value is one of per-rank (default), replicated (glob
    hints via ``replicated=``; DDP modules are inferred), or sharded
    (ShardedTensor / DTensor).  Snapshots whose values are all replicated or
    sharded can be restored into a different world size.
    """

    def __init__(self, path: str, pg: Optional[dist.ProcessGroup] = None,
                 storage_options: Optional[Dict[str, Any]] = None,
                 trust_objects: Optional[bool] = None) -> None:
        self.path = path
        self.pg = pg
        self._storage_options = storage_options
        self._metadata: Optional[SnapshotMetadata] = None
        self.trust_objects = trust_objects

    # ------------------------------------------------------------------ take

    @classmethod
    def take(cls, path: str, app_state: AppState, pg: Optional[dist.ProcessGroup] = None,
             replicated: Optional[List[str]] = None,
             storage_options: Optional[Dict[str, Any]] = None,
             _custom_tensor_prepare_func: Optional[PrepareFunc] = None,
             quantize: Optional[List[str]] = None,
             compression: Optional[str] = None,
             base: Optional[Any] = None,
             content_digests: Optional[bool] = None) -> "Snapshot":
        """Take a snapshot of ``app_state`` at ``path`` (blocking).

        ``quantize``: optional glob patterns of logical paths whose floating
        tensors are stored as blockwise OCP-fp8 (hipsnapshot extension; lossy).
        ``compression``: ``"hsz1"`` stores GPU-resident floating-point blobs
        losslessly compressed (encoded on the GPU before D2H, ~0.67x for
        bf16, ~0.84x for fp32); default from ``HIPSNAPSHOT_COMPRESSION`` ("none").
        ``base``: a committed snapshot (``Snapshot`` or path) on the same
        local file system: eligible leaves whose content digest equals the
        base's are not written, their entries point into the base
        (engine/incremental.py; see ``dependencies`` / ``materialize``).
        ``content_digests``: record each eligible leaf's hs64 in
        ``.snapshot_content/<rank>`` so this snapshot is a full-value base
        later (default ``knobs.TUNING.content_digests``, off; forced on by
        ``base``).
        """
        torch._C._log_api_usage_once("hipsnapshot.Snapshot.take")
        base_root = None
        if base is not None:
            from .engine.incremental import resolve_base

            base_root = resolve_base(base, path)  # ValueError before anything is written
            content_digests = True
        elif content_digests is None:
            content_digests = knobs.content_digests_enabled()
        memory.op_begin(pg)
        try:
            with paused_gc(plan_gc=False):
                return cls._take(path, app_state, pg, replicated, storage_options,
                                 _custom_tensor_prepare_func, quantize, compression,
                                 base_root, bool(content_digests))
        finally:
            memory.op_end()

    @classmethod
    def _take(cls, path, app_state, pg, replicated, storage_options,
              _custom_tensor_prepare_func, quantize, compression,
              base_root=None, content_digests=False) -> "Snapshot":
        cls._validate_app_state(app_state)
        _numa_bind_once()
        loop = asyncio.new_event_loop()
        comm = Comm(pg)
        t0 = time.monotonic()
        path, rep, keys, nonce, storage = cls._open_and_coalesce(
            path, comm, app_state, replicated, loop, storage_options,
            incremental=(base_root,) if content_digests else None)
        progress: Dict[str, Any] = {}
        incr = None
        try:
            if content_digests:
                from .engine.incremental import IncrementalTake, resolve_base

                if base_root is not None:
                    resolve_base(base_root, path)  # against rank 0's path, which won
                incr = IncrementalTake(path, base_root)
            with roctx_range("hipsnapshot.take.plan_and_stage"):
                pending, metadata = cls._take_impl(path, app_state, rep, keys, comm, storage,
                                                   loop, False, _custom_tensor_prepare_func,
                                                   quantize, compression, progress=progress,
                                                   incr=incr)
            t_staged = time.monotonic()
            with roctx_range("hipsnapshot.take.drain_io"), timeline.span("drain_io"):
                pending.sync_complete(loop)
            if incr is not None:
                # blobs this take points at without writing them keep the
                # checksum their own take recorded: verify() reads them too
                pending.stats.checksums.update(incr.reused_sums)
                storage.sync_write(WriteIO(path=incr.content_path(comm.get_rank()),
                                           buf=incr.content_doc()), loop)
            _write_checksums(storage, loop, comm.get_rank(), comm.get_world_size(),
                             pending.stats.checksums)
            with roctx_range("hipsnapshot.take.commit"), timeline.span("commit"):
                with timeline.span("commit_barrier", "commit"):
                    comm.barrier()
                if comm.get_rank() == 0:
                    bases = incr.bases_doc(metadata.manifest) if incr is not None else None
                    if bases is not None:
                        storage.sync_write(WriteIO(path=incr.BASES_FNAME, buf=bases), loop)
                    with timeline.span("write_metadata", "commit"):
                        cls._write_snapshot_metadata(metadata, storage, loop)
                    if incr is not None:
                        incr.drop_content_beyond(comm.get_world_size())
                if not comm.solo():
                    # take() returns on every rank only once the snapshot is
                    # committed: a rank may read it right away (the reference
                    # returns before rank 0 has written the metadata)
                    with timeline.span("committed_barrier", "commit"):
                        comm.barrier()
        finally:
            _release_plan(progress)
            storage.sync_close(loop)
            loop.close()
        timeline.dump("take", comm.get_rank())
        TakeStats.last = {"stage_s": t_staged - t0, "total_s": time.monotonic() - t0,
                          "bytes": float(pending.stats.bytes_written)}
        if incr is not None:
            TakeStats.last.update(bytes_reused=float(incr.bytes_reused),
                                  leaves_reused=float(incr.leaves_reused),
                                  digest_s=incr.digest_s)
        snap = cls(path=path, pg=pg, storage_options=storage_options)
        snap._metadata = metadata
        return snap

    @classmethod
    def async_take(cls, path: str, app_state: AppState, pg: Optional[dist.ProcessGroup] = None,
                   replicated: Optional[List[str]] = None,
                   storage_options: Optional[Dict[str, Any]] = None,
                   _custom_tensor_prepare_func: Optional[PrepareFunc] = None,
                   quantize: Optional[List[str]] = None,
                   compression: Optional[str] = None) -> "PendingSnapshot":
        """Capture a consistent snapshot and persist it in the background.

        Changes to ``app_state`` after this returns do not affect the
        snapshot.  Waiting on the returned handle is optional: the snapshot is
        committed regardless.
        """
        torch._C._log_api_usage_once("hipsnapshot.Snapshot.async_take")
        from .utils.affinity import note_caller_cpu

        note_caller_cpu()  # the drain's threads keep off this thread's core
        deferred_gc: list = []
        memory.op_begin(pg)
        try:
            with paused_gc(deferred_gc):
                pending = cls._async_take(path, app_state, pg, replicated, storage_options,
                                          _custom_tensor_prepare_func, quantize, compression)
        finally:
            memory.op_end()
        # a new plan's one full GC pass runs in the commit thread after the
        # drain, not on the unblock path (utils/tracing.paused_gc)
        pending._gc_after = bool(deferred_gc)
        # the commit thread starts draining only now: its staging workers would
        # otherwise hold the GIL while this thread is still on its way out
        pending._go.set()
        return pending

    @classmethod
    def _async_take(cls, path, app_state, pg, replicated, storage_options,
                    _custom_tensor_prepare_func, quantize, compression) -> "PendingSnapshot":
        t_in = time.perf_counter()
        cls._validate_app_state(app_state)
        with timeline.span("first_use"):
            _numa_bind_once()
        loop = asyncio.new_event_loop()
        comm = Comm(pg)
        t0 = time.monotonic()
        tp0 = time.perf_counter()
        timeline.add("async_setup", "phase", t_in, tp0)
        path, rep, keys, nonce, storage = cls._open_and_coalesce(
            path, comm, app_state, replicated, loop, storage_options)
        progress: Dict[str, Any] = {}
        try:
            pending, metadata = cls._take_impl(path, app_state, rep, keys, comm, storage, loop,
                                               True, _custom_tensor_prepare_func, quantize,
                                               compression, progress=progress)
        except BaseException as e:
            _release_plan(progress)
            from .engine.hbm_staging import arena_done

            # no drain will read the arena this take froze into: a kept one
            # is free for later takes (stream-ordered after this freeze)
            arena_done(progress.get("arenas", []))
            if progress.get("collectives_done"):
                # peers that staged successfully are already in (or about to
                # start) their commit threads: fail their barrier now instead
                # of letting them wait DEFAULT_BARRIER_TIMEOUT
                _report_async_failure(comm, path, nonce, e)
            storage.sync_close(loop)
            loop.close()
            raise
        with timeline.span("pending_init"):
            ps = PendingSnapshot(path=path, pending_io_work=pending, comm=comm, metadata=metadata,
                                 storage=storage, event_loop=loop,
                                 storage_options=storage_options, nonce=nonce,
                                 plan=progress.get("plan"),
                                 plan_store=progress.get("plan_store"))
        TakeStats.last = {"unblock_s": time.monotonic() - t0}
        timeline.add("unblock", "phase", tp0, time.perf_counter())
        timeline.dump("async_take", comm.get_rank())
        return ps

    @classmethod
    def _open_and_coalesce(cls, path: str, comm: Comm, app_state: AppState,
                           replicated: Optional[List[str]], loop: asyncio.AbstractEventLoop,
                           storage_options: Optional[Dict[str, Any]],
                           incremental: Optional[Tuple[Optional[str]]] = None):
        """Commit rule (reference `snapshot.py:226-234`): a snapshot exists
        iff its ``.snapshot_metadata`` exists.  A take into a path that holds
        a committed snapshot overwrites its blobs, so rank 0 takes the old
        commit away (``_uncommit``) BEFORE it contributes to the coalesce
        gather: no rank can finish that collective -- and so write its first
        blob -- while the old metadata still names the blobs being rewritten.
        The old metadata is stashed, not deleted: if the coalesce fails (app
        states that do not match, a rank that never arrives) no rank has
        written anything, and rank 0 puts the old commit back.
        (Rank 0's path is the snapshot's path, so it can open storage first.)"""
        storage = None
        stash = None
        try:
            if comm.get_rank() == 0:
                with timeline.span("storage_open"):
                    storage = url_to_storage_plugin_in_event_loop(path, loop, storage_options)
                with timeline.span("uncommit"):
                    stash = cls._uncommit(storage, loop)
            with timeline.span("coalesce"):
                path, rep, keys, nonce = cls._coalesce(path, comm, app_state, replicated or [],
                                                       incremental)
            if storage is None:
                with timeline.span("storage_open"):
                    storage = url_to_storage_plugin_in_event_loop(path, loop, storage_options)
        except BaseException:
            if stash is not None:
                cls._recommit(storage, loop, stash)
            if storage is not None:
                storage.sync_close(loop)
            loop.close()
            raise
        if stash is not None and stash[0] == "renamed":
            try:  # the stashed commit is obsolete now that every rank agreed
                storage.sync_delete(stash[1], loop)
            except Exception as e:  # noqa: BLE001
                logger.debug(f"could not remove the stashed metadata: {e}")
        if comm.get_rank() == 0:
            # only now that the take goes ahead (a failed coalesce puts the
            # old commit back whole, side files included)
            cls._drop_stale_side_files(storage, keep_content=incremental is not None)
        return path, rep, keys, nonce, storage

    @staticmethod
    def _drop_stale_side_files(storage: StoragePlugin, keep_content: bool) -> None:
        """An earlier incremental take's side files describe blobs this take
        replaces: a take with content digests rewrites them, any other
        removes them (local file systems only: nothing else can hold them)."""
        root = getattr(storage, "root", None)
        if not (isinstance(storage, _FSStoragePlugin) and isinstance(root, str)):
            return
        from .engine import incremental

        try:
            os.remove(os.path.join(root, incremental.BASES_FNAME))
        except OSError:
            pass
        if not keep_content and os.path.isdir(os.path.join(root, incremental.CONTENT_DIR)):
            import shutil

            shutil.rmtree(os.path.join(root, incremental.CONTENT_DIR), ignore_errors=True)

    @staticmethod
    def _uncommit(storage: StoragePlugin, loop: asyncio.AbstractEventLoop):
        """A snapshot exists iff its metadata exists: take an older commit at
        this path away before its blobs get overwritten.  Returns how to put
        it back (``_recommit``): ``("renamed", stash path)`` where the plugin
        renames atomically (FS), ``("bytes", data)`` where the old metadata
        was read and deleted, or None when there was none."""
        stash = f"{SNAPSHOT_METADATA_FNAME}.stash.{uuid.uuid4().hex[:12]}"
        out = None
        try:
            run_sync(loop, storage.rename(SNAPSHOT_METADATA_FNAME, stash))
            out = ("renamed", stash)
        except (FileNotFoundError, KeyError):
            pass
        except NotImplementedError:
            try:
                rio = ReadIO(path=SNAPSHOT_METADATA_FNAME)
                storage.sync_read(rio, loop)
                data = bytes(rio.data())
                storage.sync_delete(SNAPSHOT_METADATA_FNAME, loop)
                out = ("bytes", data)
            except (FileNotFoundError, KeyError):
                pass
            except Exception as e:  # noqa: BLE001 - e.g. plugins without delete
                logger.debug(f"could not remove previous metadata: {e}")
        except Exception as e:  # noqa: BLE001
            logger.debug(f"could not remove previous metadata: {e}")
        # a take with checksums rewrites every rank's file (verify reads only
        # ranks < world size); one without them must not leave the previous
        # take's behind.  (Removing the directory on every take cost ~1.5 ms
        # of rank 0's critical path on an overlay filesystem.)
        if not knobs.checksum_enabled():
            try:
                run_sync(loop, storage.delete_dir(checksum.CHECKSUM_DIR))
            except (FileNotFoundError, KeyError, NotImplementedError):
                pass
            except Exception as e:  # noqa: BLE001
                logger.debug(f"could not remove previous checksums: {e}")
        return out

    @staticmethod
    def _recommit(storage: Optional[StoragePlugin], loop: asyncio.AbstractEventLoop,
                  stash) -> None:
        """Put back the commit ``_uncommit`` took away (the take failed
        before any rank wrote a blob)."""
        if storage is None or stash is None:
            return
        try:
            if stash[0] == "renamed":
                run_sync(loop, storage.rename(stash[1], SNAPSHOT_METADATA_FNAME))
            else:
                commit = getattr(storage, "commit_metadata", None)
                run_sync(loop, commit(SNAPSHOT_METADATA_FNAME, stash[1]) if commit is not None
                         else storage.write(WriteIO(path=SNAPSHOT_METADATA_FNAME,
                                                    buf=memoryview(stash[1]))))
        except Exception as e:  # noqa: BLE001 - the take's own error is the one raised
            logger.warning(f"could not restore the previous snapshot's metadata: {e}")

    @classmethod
    def _take_impl(cls, path: str, app_state: AppState, replicated: Set[str],
                   global_keys: List[str], comm: Comm, storage: StoragePlugin,
                   loop: asyncio.AbstractEventLoop, is_async: bool,
                   prepare_func: Optional[PrepareFunc], quantize: Optional[List[str]],
                   compression: Optional[str] = None,
                   progress: Optional[Dict[str, Any]] = None,
                   incr=None) -> Tuple[PendingIOWork, SnapshotMetadata]:
        app_state = dict(app_state)
        rng_item = cls._pop_rng_state(app_state)
        manifest: Dict[str, Entry] = {}
        flattened: Dict[str, Any] = {}
        rng_sd = None
        # RNG first so that .state_dict() side effects cannot leak into it
        if rng_item is not None:
            key, st = rng_item
            rng_sd = st.state_dict()
            m, f = flatten(rng_sd, prefix=key)
            manifest.update(m)
            flattened.update(f)
        for key in global_keys:
            if key in app_state:
                with timeline.span("state_dict", key=key):
                    m, f = flatten(_state_dict_view(app_state[key]), prefix=key)
                manifest.update(m)
                flattened.update(f)
            # user state_dict() implementations may run collectives: keep them
            # from interleaving across ranks (skipped when no rank's can:
            # ``_coalesce``)
            if getattr(comm, "state_dict_barriers", True):
                with timeline.span("barrier"):
                    comm.barrier()
        if rng_item is not None:
            rng_item[1].load_state_dict(rng_sd)

        with timeline.span("replicated_entries"):
            rep_paths = cls._calculate_replicated_entries(flattened, replicated, comm)
        from .engine import plan_cache
        from .format.serialization import Serializer
        from .io.compression import host_requested, plan_compression, resolve

        comp = resolve(compression)
        if is_async and comp != "none" and knobs.async_device_codec() == "raw" \
                and knobs.async_hbm_staging_enabled():
            # the frozen device state drains raw: encoding it would run the
            # codec kernels on the compute units beside the training step
            comp = "none"
        rank = comm.get_rank()
        # plan reuse (engine/plan_cache.py): device-resident leaves whose plan
        # from an earlier take still holds are not planned again
        plan = cache_key = None
        resident: Dict[str, Any] = {}
        # (never for a take with content digests or a base: cached entries and
        # their JSON must not carry locations rewritten into a base)
        if not rep_paths and prepare_func is None and incr is None and plan_cache.enabled():
            with timeline.span("plan_lookup"):
                resident = {k: v for k, v in flattened.items() if plan_cache.is_resident(v)}
                if resident:
                    everything = dict(app_state)
                    if rng_item is not None:
                        everything[rng_item[0]] = rng_item[1]
                    cache_key = plan_cache.settings_key(
                        everything, rank, comm.get_world_size(), is_async, quantize,
                        comp + ("+host" if host_requested(compression) else ""))
                    # an async take's HBM freeze re-points the plan's
                    # stagers itself: it resets only the others
                    plan = plan_cache.lookup(
                        cache_key, resident,
                        defer_reset=is_async and knobs.async_hbm_staging_enabled()
                        and native.gpu_available())
                    if progress is not None and plan is not None:
                        # owned by this take from here on: a failure anywhere
                        # below must release it (``_release_plan``)
                        progress["plan"] = plan
        to_plan = flattened if plan is None else \
            {k: v for k, v in flattened.items() if k not in resident}
        t_prep = time.perf_counter()
        object_entries: Dict[str, Entry] = {}
        path_reqs: Dict[str, List[WriteReq]] = {}
        primitives: Dict[str, PrimitiveEntry] = {}
        max_chunk, max_shard = knobs.get_max_chunk_size_bytes(), knobs.get_max_shard_size_bytes()
        rep_chunk = max_chunk
        if rep_paths and comm.get_world_size() > 1:
            # replicated tensors in units small enough to balance the ranks
            rep_chunk = replicated_chunk_bytes(
                sum(v.numel() * v.element_size() for k, v in to_plan.items()
                    if k in rep_paths and isinstance(v, torch.Tensor) and not is_sharded(v)),
                comm.get_world_size(), max_chunk, knobs.TUNING.replicated_units_per_rank)
        with staging.plan_scope():
            for logical, obj in to_plan.items():
                ser = None
                if quantize and any(fnmatch.fnmatch(logical, p) for p in quantize):
                    ser = Serializer.FP8_BLOCK.value
                entry, wrs = prepare_write(
                    obj=obj, logical_path=logical, rank=rank, replicated=logical in rep_paths,
                    is_async_snapshot=is_async,
                    _tensor_prepare_func=(
                        (lambda t, tracing, _p=logical: prepare_func(_p, t, tracing))
                        if prepare_func is not None else None),
                    serializer=ser,
                    max_chunk_size_bytes=rep_chunk if logical in rep_paths else max_chunk,
                    max_shard_size_bytes=max_shard)
                if isinstance(entry, PrimitiveEntry):
                    primitives[logical] = entry
                else:
                    object_entries[logical] = entry
                    path_reqs[logical] = wrs
        timeline.add("prepare_write", "phase", t_prep, time.perf_counter(), n=len(to_plan))
        if rep_paths:  # identical on every rank (result of a collective)
            with timeline.span("partition"):
                object_entries, path_reqs = partition_write_reqs(object_entries, path_reqs,
                                                                 comm)
        if incr is not None:
            # content digests of the leaves this rank would write; with a
            # base, the unchanged ones leave here: batching, compression
            # planning and rebalancing see only what remains
            with timeline.span("content_digests"):
                incr.plan(object_entries, path_reqs, rank, quantize)
        write_reqs = [wr for wrs in path_reqs.values() for wr in wrs]
        if not knobs.is_batching_disabled():
            with timeline.span("batch"):
                # with a reused plan, this take's own slabs get their own
                # prefix: they can never collide with the plan's slabs
                _, write_reqs = batch_write_requests(
                    list(object_entries.values()), write_reqs,
                    name_prefix=f"r{rank}" if plan is None else f"r{rank}v")
        if comp == "hsz1":
            with timeline.span("plan_compression"):
                plan_compression(write_reqs, include_host=host_requested(compression))
        if plan is not None:
            object_entries = {k: plan.entries[k] if k in plan.entries else object_entries[k]
                              for k in flattened
                              if k in plan.entries or k in object_entries}
            write_reqs = plan.write_reqs + write_reqs
        elif cache_key is not None:
            prefixes = {k: flat_prefix(k) for k in everything}
            owners = [everything[k] for k, pre in prefixes.items()
                      if any(r == pre or r.startswith(pre + "/") for r in resident)]
            if is_async:
                # stored by the commit thread, off the unblock path (~0.4 ms of
                # a cold async_take); the plan serves the NEXT take either way
                if progress is not None:
                    progress["plan_store"] = functools.partial(
                        plan_cache.store, cache_key, resident, object_entries, write_reqs,
                        owners)
            else:
                with timeline.span("plan_store"):
                    plan = plan_cache.store(cache_key, resident, object_entries, write_reqs,
                                            owners)
        if progress is not None:
            progress["plan"] = plan
        manifest.update(primitives)
        manifest.update(object_entries)
        metadata = None
        if is_async:
            # async: no metadata collective before returning.  The commit
            # thread publishes this rank's manifest through the c10d store
            # and rank 0 assembles it after the commit barrier
            # (``PendingSnapshot``), so nothing on the unblock path scales
            # with the rank count.  A rank whose staging fails after this
            # point reports the error through the commit barrier
            # (``_report_async_failure``): its peers' commit threads fail at
            # once instead of timing out.
            metadata = _DeferredMetadata(manifest, plan)
            if progress is not None:
                progress["collectives_done"] = True

        budget = get_process_memory_budget_bytes(comm)
        deferred: List[WriteReq] = []
        if is_async and knobs.async_hbm_staging_enabled():
            from .engine.hbm_staging import freeze_device_state, is_deferrable
            from .engine.uvm_capture import capture_host_uvm

            # host-resident UVM tables: copied by CPU threads while the
            # trainer's stream waits on a gate, not frozen over PCIe
            with timeline.span("uvm_capture"):
                captured = capture_host_uvm(write_reqs, budget)
            with timeline.span("hbm_freeze"):
                freeze_device_state(write_reqs, plan,
                                    keep={id(wr.buffer_stager) for wr in captured})
            if progress is not None:
                progress["arenas"] = list({
                    id(r[0]): r[0] for r in (getattr(wr.buffer_stager, "frozen_region", None)
                                             for wr in write_reqs) if r is not None}.values())
            with timeline.span("split_deferred"):
                now: List[WriteReq] = []
                for wr in write_reqs:
                    (deferred if is_deferrable(wr) else now).append(wr)
                write_reqs = now
        if not is_async and not comm.solo() and knobs.rebalance_enabled():
            # uneven device loads: move whole blobs to idle ranks over xGMI
            # (a collective: before the background metadata gather starts)
            from .parallel.rebalance import rebalance

            with timeline.span("rebalance"):
                write_reqs = rebalance(write_reqs, comm)
        # largest first: the writes still running after the last D2H -- the
        # take's tail -- are then the small ones (slabs), not a 100 MB chunk
        write_reqs.sort(key=lambda wr: wr.buffer_stager.get_staging_cost_bytes(), reverse=True)
        gather = None
        first_staged: Optional[threading.Event] = None
        if metadata is None:
            # sync take: entries are final since planning, so the metadata
            # gather (JSON encoding + one collective) runs on a helper thread
            # while the main thread stages: it leaves the path to the first
            # D2H and the post-staging tail alike
            first_staged = threading.Event()
            gather = _BackgroundGather(cls._gather_metadata, manifest, comm, plan,
                                       start=first_staged)
        try:
            with timeline.span("stage", n=len(write_reqs)):
                # async: whatever was not frozen in HBM is copied from the
                # LIVE tensors -- every such copy (and its hash) must have
                # finished before async_take returns and training resumes
                if write_reqs or not is_async:
                    pending = sync_execute_write_reqs(write_reqs, storage, budget, rank, loop,
                                                      wait_copies=is_async,
                                                      first_staged=first_staged)
                else:
                    from .engine.scheduler import empty_write_work

                    pending = empty_write_work(budget)
        except BaseException:
            if gather is not None:
                gather.join_quietly()  # the staging error is the one to report
            raise
        if gather is not None:
            metadata = gather.result()
        if deferred:
            from .engine.scheduler import DeferredIOWork

            with timeline.span("deferred_init"):
                pending = DeferredIOWork(pending, deferred, storage, budget, rank)
        return pending, metadata

    # --------------------------------------------------------------- restore

    def restore(self, app_state: AppState, verify: bool = False) -> None:
        """Restore ``app_state`` in place from this snapshot.

        ``verify``: check every blob read against the checksums the take
        recorded (engine/blob_verify.py) and raise ``CorruptBlobError``
        naming the first blob that does not match."""
        torch._C._log_api_usage_once("hipsnapshot.Snapshot.restore")
        memory.op_begin(self.pg)
        try:
            with paused_gc():
                self._restore(app_state, verify)
        finally:
            memory.op_end()
            # the pools keep their rings for the next restore only while the
            # trainer keeps its headroom (engine/memory.py)
            memory.settle_restore_pools()

    def _restore(self, app_state: AppState, verify: bool = False) -> None:
        self._validate_app_state(app_state)
        _numa_bind_once()
        loop = asyncio.new_event_loop()
        comm = Comm(self.pg)
        storage = url_to_storage_plugin_in_event_loop(self.path, loop, self._storage_options)
        try:
            verifier = None
            if verify:
                from .engine.blob_verify import RestoreVerifier

                verifier = run_sync(loop, RestoreVerifier.load(storage,
                                                               self.metadata.world_size))
            app_state = dict(app_state)
            rng_item = self._pop_rng_state(app_state)
            gathered: List[Any] = [None] * comm.get_world_size()
            comm.all_gather_object(gathered, (list(app_state.keys()), socket.gethostname()))
            keys = sorted(set(itertools.chain.from_iterable(g[0] for g in gathered)))
            knobs.set_local_ranks_hint([g[1] for g in gathered].count(socket.gethostname()))
            for key in keys:
                with timeline.span("load_stateful", key=key):
                    self._load_stateful(key, app_state.get(key), storage, comm, loop, verifier)
                comm.barrier()
            if rng_item is not None:
                self._load_stateful(rng_item[0], rng_item[1], storage, comm, loop, verifier)
        finally:
            storage.sync_close(loop)
            loop.close()
        timeline.dump("restore", comm.get_rank())

    def _load_stateful(self, key: str, stateful: Optional[Stateful], storage: StoragePlugin,
                       comm: Comm, loop: asyncio.AbstractEventLoop, verifier=None) -> None:
        if stateful is None:
            return
        with timeline.span("restore_plan_view"):
            with timeline.span("manifest_for_rank"):
                manifest, merged = get_manifest_for_rank(self.metadata, comm.get_rank())
            if isinstance(stateful, torch.optim.Optimizer) and not stateful.state:
                state_pre = flat_prefix(key) + "/state/"
                if any(k.startswith(state_pre) and isinstance(e, ShardedTensorEntry)
                       for k, e in manifest.items()):
                    _materialize_optimizer_state(stateful)
            with timeline.span("state_dict_view"):
                _, flat = flatten(_state_dict_view(stateful), prefix=key)
        with timeline.span("restore_filter"):
            n_leaves = len(flat)
            flat = {k: v for k, v in flat.items()
                    if isinstance(v, torch.Tensor) or is_sharded(v)}
            own = dict(flat) if len(flat) == n_leaves else None
            prefix = flat_prefix(key)
            manifest = {k: v for k, v in manifest.items()
                        if k == prefix or k.startswith(prefix + "/")}
            merged_here = {k: v for k, v in merged.items() if k.startswith(prefix + "/")}
            handle_sharded_tensor_elasticity(manifest, merged_here, list(flat.keys()))
        # the same snapshot restored into the same device tensors again: run
        # the recorded native job (engine/restore_cache.py)
        cache_key = None
        if own is not None and restore_cache.enabled() and _inplace_load_noop(stateful):
            with timeline.span("restore_cache_key"):
                cache_key = restore_cache.key_for(_local_metadata_key(self.path), key,
                                                  comm.get_rank(), comm.get_world_size(), own)
            plan = restore_cache.lookup(cache_key)
            if plan is not None:
                with timeline.span("read_pipeline", cached=True):
                    restore_cache.run(plan, get_process_memory_budget_bytes(comm), verifier)
                    if verifier is not None:
                        run_sync(loop, verifier.finish(storage,
                                                       get_process_memory_budget_bytes(comm)))
                return
        budget = get_process_memory_budget_bytes(comm)
        # the native job's pinned slots / device rings fill beside the planning
        native_restore.prewarm_for(flat.values(), manifest.values(), budget, storage)
        containers: Dict[str, Entry] = {}
        reads: List[ReadReq] = []
        futs = {}
        with timeline.span("prepare_read", n=len(manifest)), staging.plan_scope():
            for logical, entry in manifest.items():
                if is_container_entry(entry):
                    containers[logical] = entry
                    continue
                rrs, fut = prepare_read(entry, obj_out=flat.get(logical),
                                        trust_objects=self.trust_objects)
                reads += rrs
                futs[logical] = fut
                flat.pop(logical, None)
        with timeline.span("batch_reads", n=len(reads)):
            if not knobs.is_batching_disabled():
                reads = batch_read_requests(reads)
        native_jobs, py_reads = native_restore.split(reads, storage, budget)
        with timeline.span("read_pipeline", n=len(reads)):
            sync_execute_read_reqs(py_reads, storage, budget, comm.get_rank(), loop,
                                   native_jobs=native_jobs, verifier=verifier)
        native_restore.join_prewarm()
        with timeline.span("load_state_dict", n=len(futs)):
            objs = {k: f.obj for k, f in futs.items()}
            # every leaf was read into the module's own tensor: load_state_dict
            # would only copy each tensor onto itself (FSDP2: ~9 ms of DTensor
            # copy_ dispatch per Llama-3-8B restore), so it is skipped
            if own is not None and len(objs) == len(own) and \
                    all(objs.get(k) is v for k, v in own.items()) and \
                    _inplace_load_noop(stateful):
                if not py_reads:
                    restore_cache.store(cache_key, stateful, native_jobs, own)
                return
            state_dict = inflate(containers, objs, prefix=key)
            stateful.load_state_dict(state_dict)

    # ---------------------------------------------------------- inspection

    @property
    def metadata(self) -> SnapshotMetadata:
        if self._metadata is None:
            key = _local_metadata_key(self.path)
            hit = _metadata_cache.get(key) if key is not None else None
            if hit is not None:
                self._metadata = hit
                return hit
            loop = asyncio.new_event_loop()
            storage = url_to_storage_plugin_in_event_loop(self.path, loop, self._storage_options)
            try:
                self._metadata = self._read_snapshot_metadata(storage, loop)
            finally:
                storage.sync_close(loop)
                loop.close()
            if key is not None and key == _local_metadata_key(self.path):
                _metadata_cache[key] = self._metadata
                while len(_metadata_cache) > 4:
                    _metadata_cache.pop(next(iter(_metadata_cache)))
        return self._metadata

    def get_manifest(self) -> Dict[str, Entry]:
        return copy.deepcopy(self.metadata.manifest)

    def verify(self, concurrency: int = 4, distributed: bool = False):
        """Re-read every blob and check it against the hs64 checksum its take
        recorded (hipsnapshot extension; returns ``verify.VerifyReport``,
        ``.ok`` is True iff every blob matched).  ``distributed``: every rank
        of this snapshot's process group checks its share of the blobs (a
        collective call) and gets the merged report."""
        from .verify import verify_snapshot

        return verify_snapshot(self.path, self._storage_options, concurrency,
                               distributed=distributed, pg=self.pg)

    def dependencies(self) -> List[str]:
        """The snapshot directories (absolute paths) this snapshot's entries
        point into: the bases of an incremental take (``take(base=...)``),
        which must outlive it.  Empty for a self-contained snapshot."""
        from .engine import incremental

        root = incremental.fs_root(self.path)
        return [] if root is None else incremental.read_dependencies(root)

    def materialize(self) -> "Snapshot":
        """Make this snapshot self-contained: every blob it references in a
        base is hard-linked (copied where linking fails) into its own
        directory and its metadata, checksum and content files are re-pointed;
        afterwards ``dependencies()`` is empty and the bases may be deleted."""
        from .engine import incremental

        root = incremental.fs_root(self.path)
        if root is None:
            raise ValueError("materialize() needs a snapshot on the local 'fs' storage plugin")
        incremental.materialize(root, self._storage_options)
        self._metadata = None
        return self

    def read_object(self, path: str, obj_out: Optional[T] = None,
                    memory_budget_bytes: Optional[int] = None, verify: bool = False) -> T:
        """Read one persisted object by manifest path ``RANK/STATEFUL/KEY/...``.

        Tensor/ShardedTensor/DTensor ``obj_out`` are filled in place; with
        ``memory_budget_bytes`` large tensors are read in tiles that never
        exceed it.  ``verify``: as for ``restore``.  A sharded entry read
        without a tensor ``obj_out`` comes back whole, as a host tensor of its
        global shape (the reference requires an ``obj_out`` there).
        """
        torch._C._log_api_usage_once("hipsnapshot.Snapshot.read_object")
        memory.op_begin(self.pg)
        try:
            return self._read_object(path, obj_out, memory_budget_bytes, verify)
        finally:
            memory.op_end()
            memory.settle_restore_pools()

    def _read_object(self, path: str, obj_out: Optional[T], memory_budget_bytes: Optional[int],
                     verify: bool) -> T:
        rank_str, unranked = path.split("/", 1)
        manifest, merged = get_manifest_for_rank(self.metadata, int(rank_str))
        if unranked not in merged and unranked not in manifest:
            raise RuntimeError(
                f'The supplied path "{path}" does not exist in the snapshot\'s manifest. '
                "Please verify the available paths within the snapshot via "
                "`snapshot.get_manifest()`.")
        if not isinstance(obj_out, torch.Tensor) and not is_sharded(obj_out):
            if obj_out is not None:
                logger.warning(f"`obj_out` is of type {type(obj_out)}, which does not support "
                               "in-place load. The loaded object will be returned.")
        entry = merged.get(unranked) or manifest[unranked]
        if isinstance(entry, PrimitiveEntry):
            return entry.get_value()
        if isinstance(entry, ShardedTensorEntry) and entry.shards and \
                not isinstance(obj_out, torch.Tensor) and not is_sharded(obj_out):
            from .format.serialization import SUPPORTED_QUANTIZED_DTYPES, string_to_dtype

            dtype = string_to_dtype(entry.shards[0].tensor.dtype)
            if dtype not in SUPPORTED_QUANTIZED_DTYPES:  # (those need an obj_out)
                obj_out = torch.empty(entry.global_shape(), dtype=dtype)
        loop = asyncio.new_event_loop()
        storage = url_to_storage_plugin_in_event_loop(self.path, loop, self._storage_options)
        try:
            reads, fut = prepare_read(entry, obj_out=obj_out,
                                      buffer_size_limit_bytes=memory_budget_bytes,
                                      trust_objects=self.trust_objects)
            if not knobs.is_batching_disabled():
                reads = batch_read_requests(reads)
            verifier = None
            if verify:
                from .engine.blob_verify import RestoreVerifier

                verifier = run_sync(loop, RestoreVerifier.load(storage,
                                                               self.metadata.world_size))
            sync_execute_read_reqs(reads, storage,
                                   memory_budget_bytes or knobs.MAX_PER_RANK_MEMORY_BUDGET_BYTES,
                                   Comm(self.pg).get_rank(), loop, verifier=verifier)
        finally:
            storage.sync_close(loop)
            loop.close()
        return fut.obj

    # ----------------------------------------------------------- helpers

    @staticmethod
    def _validate_app_state(app_state: AppState) -> None:
        for key, value in app_state.items():
            if not isinstance(value, Stateful):
                raise TypeError(f"Expected Stateful in app_state for key {key}, "
                                f"got {type(value)}.")

    @staticmethod
    def _pop_rng_state(app_state: Dict[str, Any]) -> Optional[Tuple[str, RNGState]]:
        items = [(k, v) for k, v in app_state.items() if isinstance(v, RNGState)]
        if len(items) > 1:
            raise RuntimeError(f"Multiple RNGState objects in app state: {[k for k, _ in items]}")
        if not items:
            return None
        del app_state[items[0][0]]
        return items[0]

    @staticmethod
    def _infer_replicated(replicated: List[str], app_state: AppState) -> List[str]:
        out = list(replicated)
        if "**" in out:
            return out
        for key, val in app_state.items():
            if isinstance(val, DDP):
                ignored = set(getattr(val, "parameters_to_ignore", []) or [])
                if not ignored:
                    out.append(os.path.join(key, "**"))
                    continue
                # parameters_to_ignore holds names relative to the wrapped
                # module; state_dict keys carry DDP's "module." prefix
                inner = val.module
                for name, _ in itertools.chain(inner.named_parameters(), inner.named_buffers()):
                    if name not in ignored and f"module.{name}" not in ignored:
                        out.append(os.path.join(key, f"module.{name}"))
        return out

    @classmethod
    def _coalesce(cls, path: str, comm: Comm, app_state: AppState, replicated: List[str],
                  incremental: Optional[Tuple[Optional[str]]] = None
                  ) -> Tuple[str, Set[str], List[str], str]:
        """ONE all-gather: path (rank 0 wins), replication globs (intersection),
        app-state keys (sorted union), hostnames (local world size), nonce,
        and what an incremental take must agree on (the resolved base)."""
        rank, ws = comm.get_rank(), comm.get_world_size()
        mode = knobs.get_state_dict_barriers()
        local = mode == "never" or (mode == "auto" and all(
            _state_dict_is_local(v) for v in app_state.values()))
        mine = (path, cls._infer_replicated(replicated, app_state), list(app_state.keys()),
                socket.gethostname(), uuid.uuid4().hex, local, incremental)
        gathered: List[Any] = [None] * ws
        comm.all_gather_object(gathered, mine, frame=4096)
        if len({g[6] for g in gathered}) > 1:
            # every rank sees the same gathered values and raises
            raise ValueError("every rank of an incremental take must pass the same base= and "
                             f"content_digests=: {[g[6] for g in gathered]}")
        # per-key barriers only when some rank's state_dict() may run a
        # collective (every rank sees the same gathered flags)
        comm.state_dict_barriers = not comm.solo() and not all(g[5] for g in gathered)
        root_path = gathered[0][0]
        if root_path != path:
            logger.warning(f"Rank {rank} specified a path ({path}) different from rank 0 "
                           f"({root_path}). Using path specified by rank 0.")
        rep = set.intersection(*[set(g[1]) for g in gathered])
        if set(mine[1]) != rep:
            logger.warning(f"Rank {rank} specified replicated paths: {set(mine[1])} different "
                           f"from replicated paths verified across all ranks: {rep}")
        keys = sorted(set(itertools.chain.from_iterable(g[2] for g in gathered)))
        hostnames = [g[3] for g in gathered]
        knobs.set_local_ranks_hint(hostnames.count(socket.gethostname()))
        if knobs.get_memory_budget_override() is None:
            # seed the budget cache from this gather (no hostname collective
            # later); available memory is re-read at most every 10 s
            import psutil

            local_ws = hostnames.count(socket.gethostname())
            now = time.monotonic()
            if now - _avail_mem[1] > 10.0:
                _avail_mem[:] = [psutil.virtual_memory().available, now]
            budget = int(min(_avail_mem[0] * 0.6 / max(local_ws, 1),
                             knobs.MAX_PER_RANK_MEMORY_BUDGET_BYTES))
            _budget_cache[(id(getattr(comm, "pg", comm)), ws)] = budget
        return root_path, rep, keys, gathered[0][4]

    @staticmethod
    def _calculate_replicated_entries(flattened: Dict[str, Any], replicated: Set[str],
                                      comm: Comm) -> Set[str]:
        """Replicated = matches a glob on every rank, exists on every rank, not sharded."""
        mine = sorted(p for p, v in flattened.items()
                      if not is_sharded(v) and any(fnmatch.fnmatch(p, g) for g in replicated))
        ws = comm.get_world_size()
        if comm.solo() or not replicated:
            # ``replicated`` is the cross-rank intersection from _coalesce, so
            # every rank takes this early exit together (no collective needed)
            return set(mine)
        gathered: List[Any] = [None] * ws
        comm.all_gather_object(gathered, mine)
        return set.intersection(*[set(g) for g in gathered])

    @staticmethod
    def _metadata_payload(manifest: Dict[str, Entry], plan=None
                          ) -> Tuple[Dict[str, Entry], List[Tuple[str, str]]]:
        """This rank's part of the metadata: (replicated entries, pre-encoded
        JSON fragments of every other entry).  Entries of a reused take plan
        keep the JSON encoded by the first take."""
        rep = {k: e for k, e in manifest.items() if is_replicated(e)}
        if plan is None:
            return rep, [(k, entry_json(e)) for k, e in manifest.items() if k not in rep]
        cached, planned = plan.json, plan.entries
        frags = []
        for k, e in manifest.items():
            if k in rep:
                continue
            js = cached.get(k)
            if js is None:
                js = entry_json(e)
                if k in planned:
                    cached[k] = js
            frags.append((k, js))
        return rep, frags

    @staticmethod
    def _assemble_metadata(gathered: List[Any], ws: int) -> SnapshotMetadata:
        """Every rank's ``_metadata_payload`` -> the snapshot metadata: the
        committing rank only consolidates replicated entries and joins
        strings."""
        rank_reps = consolidate_replicated_entries([g[0] for g in gathered])
        parts = []
        for rank, (_, fr) in enumerate(gathered):
            for logical, js in fr:
                parts.append(json.dumps(f"{rank}/{logical}") + ":" + js)
            for logical, entry in rank_reps[rank].items():
                parts.append(json.dumps(f"{rank}/{logical}") + ":" + entry_json(entry))
        return LazySnapshotMetadata(metadata_json_from_parts(__version__, ws, parts),
                                    __version__, ws)

    @classmethod
    def _gather_metadata(cls, manifest: Dict[str, Entry], comm: Comm,
                         plan=None) -> SnapshotMetadata:
        """ONE all-gather of every rank's ``_metadata_payload``; each rank
        JSON-encodes its own entries in parallel (reference: all-gather of
        entry objects, then rank 0 encodes the whole manifest,
        `snapshot.py:842-853`)."""
        ws = comm.get_world_size()
        gathered: List[Any] = [None] * ws
        comm.all_gather_object(gathered, cls._metadata_payload(manifest, plan))
        return cls._assemble_metadata(gathered, ws)

    @staticmethod
    def _gather_manifest(manifest: Dict[str, Entry], comm: Comm) -> Dict[str, Entry]:
        gathered: List[Any] = [None] * comm.get_world_size()
        comm.all_gather_object(gathered, manifest)
        gathered = consolidate_replicated_entries(gathered)
        out: Dict[str, Entry] = {}
        for rank, m in enumerate(gathered):
            for logical, entry in m.items():
                out[f"{rank}/{logical}"] = entry
        return out

    @staticmethod
    def _write_snapshot_metadata(metadata: SnapshotMetadata, storage: StoragePlugin,
                                 loop: asyncio.AbstractEventLoop) -> None:
        with timeline.span("metadata_to_json", "commit"):
            buf = metadata.to_json().encode("utf-8")
        metadata.__dict__.pop("_json_async", None)  # later edits re-encode
        commit = getattr(storage, "commit_metadata", None)
        if commit is not None:
            run_sync(loop, commit(SNAPSHOT_METADATA_FNAME, buf))
        else:
            storage.sync_write(WriteIO(path=SNAPSHOT_METADATA_FNAME, buf=buf), loop)

    @staticmethod
    def _read_snapshot_metadata(storage: StoragePlugin, loop: asyncio.AbstractEventLoop
                                ) -> SnapshotMetadata:
        rio = ReadIO(path=SNAPSHOT_METADATA_FNAME)
        storage.sync_read(rio, loop)
        return SnapshotMetadata.from_json(bytes(rio.data()).decode("utf-8"))


# Parsed metadata of local-FS snapshots, keyed by the metadata file's
# identity (path, inode, size, mtime): a second ``Snapshot(path)`` of the same
# committed snapshot -- an eval loop, a restore after a failed step -- reuses
# the parsed manifest and its cached per-rank split instead of parsing the
# merged manifest again (~8 ms for an 8-rank FSDP Llama-3-8B).  A new take
# into the path replaces the file (new inode / mtime) and misses.  The
# metadata object is never mutated by the restore path (parallel/elasticity.py
# ``_fresh``), so sharing it is as safe as reusing one Snapshot object.
_metadata_cache: Dict[tuple, SnapshotMetadata] = {}


def _local_metadata_key(path: str) -> Optional[tuple]:
    from .storage.registry import split_url

    protocol, root = split_url(path)
    if protocol != "fs":
        return None
    f = os.path.join(os.path.abspath(root), SNAPSHOT_METADATA_FNAME)
    try:
        st = os.stat(f)
    except OSError:
        return None
    return (f, st.st_dev, st.st_ino, st.st_size, st.st_mtime_ns)


_numa_done = [False]


def _numa_bind_once() -> None:
    """``HIPSNAPSHOT_NUMA_BIND=1``: bind this process to the CPUs of its
    current GPU's NUMA node before the first I/O threads start (once)."""
    if _numa_done[0]:
        return
    _numa_done[0] = True
    # one commit thread up front: starting it in the first async_take cost
    # that take's unblock ~0.2 ms
    pool = _commit_pool()
    if torch.cuda.is_initialized():
        # the data plane's code object loads on that thread while this take
        # plans, not at its first kernel launch (~3 ms of a first async_take)
        native.prewarm_module(torch.cuda.current_device(), pool)
    else:
        pool.submit(int)
    if os.environ.get("HIPSNAPSHOT_NUMA_BIND") and torch.cuda.is_available():
        from .utils.affinity import maybe_bind_from_env

        rep = maybe_bind_from_env(torch.cuda.current_device())
        if rep is not None:
            logger.info(f"NUMA binding: {rep}")


def flat_prefix(key: str) -> str:
    from .format.flatten import encode_key

    return encode_key(key)


def _release_plan(progress: Dict[str, Any]) -> None:
    """The take that used a cached plan is over (its I/O completed or it
    failed): the plan may serve the next take."""
    from .engine import plan_cache

    plan_cache.release(progress.pop("plan", None))


class _BackgroundGather:
    """Runs ``fn(manifest, comm)`` (the metadata gather) on a helper thread.
    Every rank starts it at the same point of the take, so its collective
    pairs up across ranks whatever the main threads do meanwhile; the helper
    adopts the caller's HIP device (current device is per thread and RCCL
    object collectives stage their bytes on it)."""

    _pool: Dict[str, Any] = {"pid": None, "ex": None}

    def __init__(self, fn, manifest, comm: Comm, plan,
                 start: Optional[threading.Event] = None) -> None:
        self._out: Dict[str, Any] = {}
        dev = torch.cuda.current_device() if torch.cuda.is_initialized() else None

        def run() -> None:
            try:
                if start is not None:
                    # after the take's first copy is queued: its JSON encoding
                    # holds the GIL the staging threads need to get going
                    # (0.5 ms of a rank share's ~3 ms before the first DMA)
                    start.wait(0.05)
                if dev is not None:
                    torch.cuda.set_device(dev)
                with timeline.span("gather_manifest"):
                    self._out["v"] = fn(manifest, comm, plan)
            except BaseException as e:  # noqa: BLE001 - re-raised in result()
                self._out["e"] = e

        # one long-lived helper thread per process (a new thread per take
        # cost its start-up on the take's critical path)
        pool = _BackgroundGather._pool
        if pool["ex"] is None or pool["pid"] != os.getpid():
            from concurrent.futures import ThreadPoolExecutor

            pool["ex"] = ThreadPoolExecutor(max_workers=1,
                                            thread_name_prefix="hipsnapshot-manifest")
            pool["pid"] = os.getpid()
        self._fut = pool["ex"].submit(run)

    def join_quietly(self) -> None:
        self._fut.result()

    def result(self):
        self._fut.result()
        if "e" in self._out:
            raise self._out["e"]
        return self._out["v"]


def _write_checksums(storage: StoragePlugin, loop: asyncio.AbstractEventLoop, rank: int,
                     world_size: int, sums: Dict[str, int]) -> None:
    """This rank's blob checksums, ``.snapshot_checksums/<rank>`` (written
    before the commit barrier: a committed snapshot has all of them)."""
    if not knobs.checksum_enabled():
        return
    doc = {"algo": checksum.ALGO, "rank": rank, "world_size": world_size,
           "blobs": {p: checksum.to_hex(h) for p, h in sorted(sums.items())}}
    storage.sync_write(WriteIO(path=checksum.rank_file(rank),
                               buf=json.dumps(doc).encode("utf-8")), loop)


class _DeferredMetadata:
    """An async take's manifest; its metadata is assembled in the commit
    thread (``PendingSnapshot._complete_snapshot``), not on the unblock path."""

    __slots__ = ("manifest", "plan")

    def __init__(self, manifest: Dict[str, Entry], plan) -> None:
        self.manifest = manifest
        self.plan = plan


def _manifest_key(path: str, nonce: str, rank: int) -> str:
    return f"hipsnapshot_{nonce}_{path}/manifest/{rank}"


def _encode_payload(rep: Dict[str, Entry], frags: List[Tuple[str, str]]) -> bytes:
    return json.dumps({"rep": {k: e.to_dict() for k, e in rep.items()},
                       "frags": frags}).encode("utf-8")


def _decode_payload(raw: bytes) -> Tuple[Dict[str, Entry], List[Tuple[str, str]]]:
    from .format.manifest import entry_from_dict

    d = json.loads(bytes(raw).decode("utf-8"))
    return ({k: entry_from_dict(v) for k, v in d["rep"].items()},
            [(k, js) for k, js in d["frags"]])


def _commit_barrier(store, path: str, nonce: str, rank: int, world_size: int) -> LinearBarrier:
    return LinearBarrier(prefix=f"hipsnapshot_{nonce}_{path}", store=store, rank=rank,
                         world_size=world_size, leader_rank=0)


def _report_async_failure(comm: Comm, path: str, nonce: str, exc: BaseException) -> None:
    """A rank failed between the metadata gather and its commit thread:
    publish the error on the async commit barrier so the leader fails in
    ``arrive`` and every peer in ``depart``.  Only an EXISTING store is used
    (creating one is collective and the peers are not in a collective)."""
    if comm.solo():
        return
    store = existing_store(comm)
    if store is None:
        logger.warning("async_take failed on this rank and no store exists to report it; "
                       "peers will wait for the commit barrier timeout")
        return
    try:
        _commit_barrier(store, path, nonce, comm.get_rank(),
                        comm.get_world_size()).report_error(repr(exc))
    except Exception as e:  # noqa: BLE001 - never mask the original error
        logger.warning(f"could not report async_take failure to peers: {e}")


_commit = {"pid": None, "pool": None}
_commit_lock = threading.Lock()


def _commit_pool():
    """Threads that run async takes' commits (``PendingSnapshot``), kept
    between takes.  Non-daemon, like the dedicated thread each take used to
    start: the interpreter waits for a commit in flight before it exits."""
    pool = _commit["pool"]
    if pool is None or _commit["pid"] != os.getpid():
        from concurrent.futures import ThreadPoolExecutor

        with _commit_lock:
            if _commit["pool"] is None or _commit["pid"] != os.getpid():
                _commit["pool"] = ThreadPoolExecutor(max_workers=64,
                                                     thread_name_prefix="hipsnapshot-commit")
                _commit["pid"] = os.getpid()
            pool = _commit["pool"]
    return pool


class PendingSnapshot:
    """Handle of an in-flight ``async_take``; the commit happens in a thread
    that never issues collectives (store-based two-phase barrier)."""

    DEFAULT_BARRIER_TIMEOUT = timedelta(seconds=1800)

    def __init__(self, path: str, pending_io_work: PendingIOWork, comm: Comm,
                 metadata: SnapshotMetadata, storage: StoragePlugin,
                 event_loop: asyncio.AbstractEventLoop,
                 storage_options: Optional[Dict[str, Any]] = None, nonce: str = "",
                 plan=None, plan_store=None) -> None:
        self.path = path
        self.pg = comm.pg
        self.exc_info = None
        self._done = False
        self._storage_options = storage_options
        self.stats: Dict[str, float] = {}
        self._go = threading.Event()  # set by async_take once it is returning
        self._finished = threading.Event()
        self._gc_after = False  # run the new plan's full GC pass after the commit
        # the drain runs with the knobs of the async_take call, whatever the
        # environment says by the time it writes (knobs.pinned)
        self._env = knobs.env_snapshot()
        store = None if comm.solo() else get_or_create_store(comm)
        self._pending_io_work = pending_io_work
        # a pooled thread: starting one cost ~0.2 ms of every unblock
        _commit_pool().submit(
            self._run_commit, path=path, rank=comm.get_rank(),
            world_size=comm.get_world_size(), pending_io_work=pending_io_work,
            metadata=metadata, storage=storage, event_loop=event_loop, store=store,
            nonce=nonce, plan=plan, plan_store=plan_store)

    def _run_commit(self, **kwargs) -> None:
        try:
            with knobs.pinned(self._env):
                self._complete_snapshot(**kwargs)
        except BaseException:  # noqa: BLE001 - reported by wait()
            if self.exc_info is None:
                self.exc_info = sys.exc_info()
        finally:
            self._done = True
            self._finished.set()

    def _complete_snapshot(self, path: str, rank: int, world_size: int,
                           pending_io_work: PendingIOWork, metadata: SnapshotMetadata,
                           storage: StoragePlugin, event_loop: asyncio.AbstractEventLoop,
                           store, nonce: str, plan=None, plan_store=None) -> None:
        # WARNING: no collectives in this thread
        self._go.wait()
        if plan_store is not None:
            # a new take plan, cached here instead of on the unblock path
            from .engine import plan_cache

            try:
                with timeline.span("plan_store", "commit"):
                    plan = plan_store()
            except Exception as e:  # noqa: BLE001 - an uncached plan is only not reused
                logger.debug(f"take plan not cached: {e}")
                plan = None
            if isinstance(metadata, _DeferredMetadata):
                metadata.plan = plan
            if plan_cache.take_stored_flag() and knobs.gc_after_plan():
                self._gc_after = True  # its one full GC pass, after the commit
        barrier = None
        if store is not None:
            barrier = _commit_barrier(store, path, nonce, rank, world_size)
        try:
            if isinstance(metadata, _DeferredMetadata):
                # the metadata exchange happens here, through the store (not a
                # collective): every rank publishes its part before it
                # arrives at the commit barrier; rank 0 assembles them after
                try:
                    with timeline.span("manifest_payload", "commit"):
                        payload = Snapshot._metadata_payload(metadata.manifest, metadata.plan)
                        if store is None:
                            metadata = Snapshot._assemble_metadata([payload], world_size)
                        else:
                            store.set(_manifest_key(path, nonce, rank),
                                      _encode_payload(*payload))
                            metadata = None
                except BaseException:
                    # the drain must still be awaited (its threads read the
                    # frozen arena and use this event loop) before failing
                    try:
                        pending_io_work.sync_complete(event_loop)
                    except Exception:  # noqa: BLE001 -- the first error is reported
                        pass
                    raise
            pending_io_work.sync_complete(event_loop)
            _write_checksums(storage, event_loop, rank, world_size,
                             pending_io_work.stats.checksums)
            if barrier is not None:
                barrier.arrive(timeout=self.DEFAULT_BARRIER_TIMEOUT)
            if rank == 0:
                if metadata is None:
                    with timeline.span("manifest_assemble", "commit"):
                        keys = [_manifest_key(path, nonce, r) for r in range(world_size)]
                        raw = store.multi_get(keys) if hasattr(store, "multi_get") \
                            else [store.get(k) for k in keys]
                        metadata = Snapshot._assemble_metadata(
                            [_decode_payload(b) for b in raw], world_size)
                        for k in keys:
                            try:
                                store.delete_key(k)
                            except Exception:  # noqa: BLE001 - best effort cleanup
                                pass
                Snapshot._write_snapshot_metadata(metadata, storage, event_loop)
            if barrier is not None:
                barrier.depart(timeout=self.DEFAULT_BARRIER_TIMEOUT)
            self.stats = pending_io_work.stats.as_dict()
        except Exception as e:  # noqa: BLE001
            if barrier is not None:
                try:
                    barrier.report_error(str(e))
                except Exception:  # pragma: no cover
                    pass
            self.exc_info = sys.exc_info()
            logger.warning(f"Encountered exception while taking snapshot asynchronously:\n{e}")
        finally:
            self._pending_io_work = None
            _release_plan({"plan": plan})  # its stagers are idle again
            try:
                storage.sync_close(event_loop)
            finally:
                event_loop.close()
            if self._gc_after:
                import gc

                with timeline.span("gc_after_plan"):
                    gc.collect()
        self._done = True

    def wait(self) -> Snapshot:
        # nothing trains beside the drain while its caller blocks here: let
        # the native drain use all of its writers (engine/native_drain.py)
        boost = getattr(self._pending_io_work, "boost", None)
        if boost is not None and not self._done:
            boost()
        self._finished.wait()
        if self.exc_info is not None:
            formatted = "".join(traceback.format_exception(*self.exc_info))
            raise RuntimeError(
                f"Encountered exception while taking snapshot asynchronously:\n{formatted}")
        return Snapshot(path=self.path, pg=self.pg, storage_options=self._storage_options)

    def done(self) -> bool:
        return self._done
