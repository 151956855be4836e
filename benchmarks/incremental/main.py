"""Incremental takes against a plain take, in one process.

Builds a bf16 state with Llama-3-8B's parameter shapes on one GPU (cut off at
``--size-gb``), then times, each into a fresh directory:

* a plain ``Snapshot.take``;
* a take with ``content_digests=True`` (the base of what follows);
* ``take(base=...)`` with 0 %, 50 % and 100 % of the bytes changed since the
  base (whole tensors, in parameter order), and with ``--frozen-fraction`` of
  the bytes unchanged (the LoRA / frozen-backbone case);
* ``plain_after_base``: a plain take at the point of the sequence where the
  ``base=`` takes run, right after a full base was written -- the control that
  separates what the file system does then from what ``base=`` costs.

Every figure is compared with the plain take of the same process.
``digest_GBps`` is the state's bytes over ``digest_s`` (one ``hs_hash64_batch``
launch plus its table upload and read-back).

    python benchmarks/incremental/main.py --size-gb 16 --frozen-fraction 0.9
"""

from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size-gb", type=float, default=16.0)
    ap.add_argument("--frozen-fraction", type=float, default=0.9)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--compression", default="none", choices=["none", "hsz1"])
    ap.add_argument("--device", default="cuda:0", help="cuda:N, or cpu (host tensors)")
    ap.add_argument("--dir", default=os.environ.get("HSBENCH_DIR", "/tmp"))
    args = ap.parse_args()

    import torch

    from hipsnapshot import Snapshot, StateDict
    from hipsnapshot.models.llama import Llama, LlamaConfig
    from hipsnapshot.snapshot import TakeStats

    dev = torch.device(args.device)
    on_gpu = dev.type == "cuda"
    if on_gpu:
        torch.cuda.set_device(dev)
        from hipsnapshot.utils.affinity import bind_to_gpu_numa

        bind_to_gpu_numa(dev.index or 0)
    with torch.device("meta"):
        meta = Llama(LlamaConfig.llama3_8b())
    budget = int(args.size_gb * 1e9)
    gen = torch.Generator(device=dev).manual_seed(0)
    params, total = {}, 0
    for name, p in meta.named_parameters():
        nb = p.numel() * 2
        if total + nb > budget:
            if not params:  # a state smaller than the first parameter: a slice of it
                rows = max(1, budget // (2 * p.shape[1]))
                params[name] = (torch.randn(rows, p.shape[1], device=dev, generator=gen)
                                * 0.02).to(torch.bfloat16)
                total += params[name].numel() * 2
            continue
        params[name] = (torch.randn(tuple(p.shape), device=dev, generator=gen) * 0.02
                        ).to(torch.bfloat16)
        total += nb
    del meta
    app_state = {"model": StateDict(**params)}
    names = list(params)

    def sync() -> None:
        if on_gpu:
            torch.cuda.synchronize()

    def touch(fraction: float) -> int:
        """Change the leading tensors that make up ``fraction`` of the bytes."""
        done = 0
        for n in names:
            if done >= fraction * total:
                break
            params[n].view(-1)[:8].add_(0.5)
            done += params[n].numel() * 2
        sync()
        return done

    root = os.path.join(args.dir, "hipsnapshot_incremental")
    shutil.rmtree(root, ignore_errors=True)

    def timed(name: str, **kw) -> dict:
        path = os.path.join(root, name)
        shutil.rmtree(path, ignore_errors=True)
        sync()
        t0 = time.perf_counter()
        Snapshot.take(path, app_state, compression=args.compression, **kw)
        dt = time.perf_counter() - t0
        s = dict(TakeStats.last)
        return {"s": dt, "stage_s": s.get("stage_s", 0.0), "bytes_written": s.get("bytes", 0.0),
                "bytes_reused": s.get("bytes_reused", 0.0), "digest_s": s.get("digest_s", 0.0)}

    cases = [("changed_0", 0.0), ("changed_50", 0.5), ("changed_100", 1.0),
             ("frozen", 1.0 - args.frozen_fraction)]
    runs: dict = {k: [] for k in ["plain", "content_digests", "plain_after_base"]
                  + [c for c, _ in cases]}
    for step in range(args.warmup + args.steps):
        keep = step >= args.warmup
        r = timed("plain")
        if keep:
            runs["plain"].append(r)
        r = timed("base", content_digests=True)
        if keep:
            runs["content_digests"].append(r)
        base = os.path.join(root, "base")
        for i, (case, fraction) in enumerate(cases):
            if i:  # a fresh base of the current values: each case changes relative to it
                timed("base", content_digests=True)
            if case == "changed_100":
                # control: a plain take where the base= takes stand, right
                # after a full base was written (its pages are still dirty)
                r = timed("incr")
                if keep:
                    runs["plain_after_base"].append(r)
                timed("base", content_digests=True)
            touched = touch(fraction)
            r = dict(timed("incr", base=base), touched_bytes=touched)
            if keep:
                runs[case].append(r)
    shutil.rmtree(root, ignore_errors=True)

    def med(case: str, key: str) -> float:
        return statistics.median(r[key] for r in runs[case])

    plain = med("plain", "s")
    out = {"bench": "incremental", "device": args.device, "compression": args.compression,
           "state_bytes": total, "tensors": len(names), "steps": args.steps,
           "frozen_fraction": args.frozen_fraction,
           "plain_take_s": round(plain, 4), "plain_stage_s": round(med("plain", "stage_s"), 4),
           "plain_GBps": round(total / plain / 1e9, 2)}
    for case in runs:
        if case == "plain":
            continue
        d = med(case, "digest_s")
        out[case] = {"take_s": round(med(case, "s"), 4),
                     "stage_s": round(med(case, "stage_s"), 4),
                     "vs_plain": round(med(case, "s") / plain, 3),
                     "extra_s_over_plain": round(med(case, "s") - plain, 4),
                     "digest_s": round(d, 5),
                     "digest_GBps": round(total / d / 1e9, 1) if d else None,
                     "bytes_written": int(med(case, "bytes_written")),
                     "bytes_reused": int(med(case, "bytes_reused"))}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
