"""Worker bodies of the multi-process incremental-take tests (module-level so
spawn can import them)."""

import os

import pytest
import torch
import torch.distributed as dist

from hipsnapshot import Snapshot, StateDict
from hipsnapshot.knobs import override_is_batching_disabled, override_max_chunk_size_bytes
from hipsnapshot.snapshot import TakeStats

N_REP = 8


def _rep_state():
    # the same values on every rank, as DDP keeps them
    return StateDict(**{f"w{i}": torch.full((1000 * (i + 1),), float(i)) for i in range(N_REP)})


def _nbytes(t):
    return t.numel() * t.element_size()


def ddp_incremental(root: str):
    rank = dist.get_rank()
    A, B = os.path.join(root, "A"), os.path.join(root, "B")
    sd = _rep_state()
    # per-rank state; "big" is written as 4 chunks of 4096 floats
    mine = StateDict(t=torch.full((64,), float(rank)),
                     big=torch.arange(16384, dtype=torch.float32) + rank)
    for batching_off in (True, False):
        a, b = A + str(batching_off), B + str(batching_off)
        with override_is_batching_disabled(batching_off), override_max_chunk_size_bytes(16384):
            sd["w3"][0], mine["big"][5000] = 3.0, 5000.0
            Snapshot.take(a, {"sd": sd, "mine": mine}, replicated=["sd/**"],
                          content_digests=True)
            sd["w3"][0] = -1.0
            mine["big"][5000] = -1.0  # chunk 1 of 4
            Snapshot.take(b, {"sd": sd, "mine": mine}, replicated=["sd/**"], base=a)
            stats = [None, None]
            dist.all_gather_object(stats, dict(TakeStats.last))
        # each replicated leaf was hashed by the one rank the partition plan
        # gave it to: together the ranks reused every unchanged byte once
        unchanged = sum(_nbytes(v) for k, v in sd.items() if k != "w3") \
            + 2 * (3 * 16384 + _nbytes(mine["t"]))
        assert sum(s["bytes_reused"] for s in stats) == unchanged, stats
        assert all(s["leaves_reused"] > 0 for s in stats), stats  # across the partition
        man = Snapshot(b).get_manifest()
        for i in range(N_REP):
            assert man[f"0/sd/w{i}"].location.startswith("../") == (i != 3), i
        chunks = sorted(man[f"{rank}/mine/big"].chunks, key=lambda c: c.offsets)
        assert [c.tensor.location.startswith("../") for c in chunks] == \
            [True, False, True, True]
        assert man[f"{rank}/mine/t"].location.startswith("../")
        out = StateDict(**{k: torch.zeros_like(v) for k, v in sd.items()})
        mine_out = StateDict(t=torch.zeros(64), big=torch.zeros(16384))
        Snapshot(b).restore({"sd": out, "mine": mine_out})
        for k, v in sd.items():
            assert torch.equal(out[k], v), k
        assert torch.equal(mine_out["t"], mine["t"]) and torch.equal(mine_out["big"], mine["big"])
        if rank == 0:
            assert Snapshot(b).verify().ok
            assert Snapshot(b).dependencies() == [os.path.realpath(a)]
        dist.barrier()


def mismatched_bases(root: str):
    rank = dist.get_rank()
    sd = _rep_state()
    bases = [os.path.join(root, "A0"), os.path.join(root, "A1")]
    for p in bases:
        Snapshot.take(p, {"sd": sd}, replicated=["sd/**"], content_digests=True)
    new = os.path.join(root, "N")
    with pytest.raises(ValueError, match="same base"):
        Snapshot.take(new, {"sd": sd}, replicated=["sd/**"], base=bases[rank])
    dist.barrier()
    assert not os.path.exists(os.path.join(new, ".snapshot_metadata"))
    assert not os.path.exists(new) or not os.listdir(new)


def dtensor_one_rank_mesh(root: str):
    """FSDP2's layout on one GPU: DTensor ``Shard(0)`` leaves over a one-rank
    mesh; unchanged shards are reused by their offsets and sizes."""
    from torch.distributed.device_mesh import init_device_mesh
    from torch.distributed.tensor import DTensor, Shard

    gpu = torch.device("cuda:0")
    A, B = os.path.join(root, "A"), os.path.join(root, "B")
    mesh = init_device_mesh("cuda", (1,))
    g = torch.Generator(device=gpu).manual_seed(5)
    local = {k: torch.randn(r, 256, device=gpu, generator=g)
             for k, r in (("w0", 48), ("w1", 96), ("w2", 7))}
    sd = StateDict(**{k: DTensor.from_local(v, mesh, [Shard(0)], run_check=False)
                      for k, v in local.items()})
    Snapshot.take(A, {"m": sd}, content_digests=True)
    local["w1"][95, 255] += 1.0
    Snapshot.take(B, {"m": sd}, base=A)
    assert TakeStats.last["bytes_reused"] == (48 + 7) * 256 * 4
    man = Snapshot(B).get_manifest()
    base_man = Snapshot(A).get_manifest()
    for k in local:
        shards, base_shards = man[f"0/m/{k}"].shards, base_man[f"0/m/{k}"].shards
        assert [(s.offsets, s.sizes) for s in shards] == \
            [(s.offsets, s.sizes) for s in base_shards]
        assert all(s.tensor.location.startswith("../") == (k != "w1") for s in shards), k
    outs = {k: torch.zeros_like(v) for k, v in local.items()}
    Snapshot(B).restore({"m": StateDict(**{
        k: DTensor.from_local(v, mesh, [Shard(0)], run_check=False)
        for k, v in outs.items()})})
    torch.cuda.synchronize()
    for k in local:
        assert torch.equal(outs[k], local[k]), k
    assert Snapshot(B).verify().ok
