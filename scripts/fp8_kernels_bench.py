"""fp8 quantize / dequantize kernels alone on 512 Mi elements (1 GiB of bf16;
``--mi-elems M`` for another size;
for rocprofv3 --stats / --pmc passes): MX (E8M0 per 32), fp32 scale per 128,
MFMA Hadamard-32, MXFP4 (e2m1 nibbles, E8M0 per 32), Hadamard-rotated MXFP4,
MXFP6 (e2m3 codes, E8M0 per 32), two-level-scaled FP4 (e2m1 nibbles, e4m3 per
16 under one fp32 scale; its quantize is three launches and reads the source
twice, and ``traffic_bytes`` counts that), and the format probe of
``HIPSNAPSHOT_FP8_FORMAT=auto`` (``probe``: amax + probe + row sum, all four
candidates, the source read twice and nothing stored; ``probe_mx``: without the
two-level candidate, one read).
Prints one JSON line per
kernel with host-timed GB/s of HBM traffic (read + written bytes), the time
between device events around the call, and GB/s of the tensor alone (source
bytes of a quantize, destination bytes of a dequantize).

    fp8_kernels_bench.py [--dtype bf16|f32] [--offset] [--rounds R] [--mi-elems M] [mode ...]

Modes: ``mx_e8m0``, ``none``, ``hadamard32``, ``mxfp4``, ``mxfp4_hadamard32``,
``mxfp6``, ``nvfp4``, ``probe``, ``probe_mx``, ``regions`` (alone).  ``--rounds R`` goes
through the list of modes R times, so that two modes alternate and the spread
of one mode's repeats is seen beside the difference between the two.

``regions`` measures ``hs_dequant_regions`` on an 8192 x 8192 piece in the four
region-decodable formats: (a) the whole piece into a contiguous tensor beside
the streaming dequantizer, (b) a row half and (c) a column half beside the
two-pass of the existing entry points (stream-dequantize the whole piece into
scratch, then one ``hs_copy_nd`` of the region).

``--offset`` shifts the source and the restored tensor by one element, so
neither has the alignment of the vector loads and stores."""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from hipsnapshot.ops import native, quant  # noqa: E402


def timeit(fn, iters=10):
    """(host best, host median, event best, event median) seconds."""
    fn()
    torch.cuda.synchronize()
    ts, es = [], []
    for _ in range(iters):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
        es.append(start.elapsed_time(end) * 1e-3)
    return min(ts), sorted(ts)[len(ts) // 2], min(es), sorted(es)[len(es) // 2]


def regions_mode(dtype, rounds):
    dev, side = 0, 8192
    hs = int(torch.cuda.current_stream().cuda_stream)
    w = torch.empty(side, side, dtype=dtype, device="cuda:0").normal_()
    from hipsnapshot.format.manifest import TensorEntry
    from hipsnapshot.format.serialization import SER, dtype_to_string

    sets = {"whole": None, "rows": [(0, 0, side // 2)], "cols": [(1, 0, side // 2)]}
    blobs = {}  # quantized once per format, by the kernels, in HBM
    for fmt in ["mx", "mxfp4", "mxfp6", "nvfp4"]:
        info = quant.fp8_entry_quant_info(w, fmt=fmt)
        p, total = info["payload_bytes"], info["total_bytes"]
        blob = torch.zeros(total, dtype=torch.uint8, device="cuda:0")
        if fmt == "nvfp4":
            native.nvfp4_quantize(dev, w, blob[:p], blob[p: total - 4], blob[total - 4:], hs)
        else:
            quantize = {"mx": native.mx8_quantize, "mxfp4": native.mxfp4_quantize,
                        "mxfp6": native.mxfp6_quantize}[fmt]
            quantize(dev, w, blob[:p], blob[p:], hs)
        blobs[fmt] = (info, blob)
    torch.cuda.synchronize()
    for fmt in ["mx", "mxfp4", "mxfp6", "nvfp4"] * rounds:
        info, blob = blobs[fmt]
        entry = TensorEntry("w", SER.FP8_BLOCK, dtype_to_string(dtype), [side, side], False,
                            quant=info)
        p, total = info["payload_bytes"], info["total_bytes"]
        am = blob[total - 4: total] if fmt == "nvfp4" else None
        scratch = torch.empty_like(w)
        for name, narrows in sets.items():
            src = scratch
            for d, start, length in narrows or ():
                src = src.narrow(d, start, length)
            dst = torch.empty(src.shape, dtype=dtype, device="cuda:0")

            keep = []  # descriptor stages and workspaces, until timeit has synchronized

            def kernel():
                keep.append(native.dequant_regions(dev, info["format"], blob[:p],
                                                   blob[p: p + info["nblocks"]], am, entry.shape,
                                                   [(narrows, dst)], hs, sync=False))

            def two_pass():
                quant.dequantize_device(blob, entry, scratch)
                if narrows is not None:
                    batch = native.CopyBatch()
                    native.tensor_copy_descriptor(batch, src, dst)
                    batch.launch(dev, hs, sync=False)

            results = {}
            for what, fn in (("regions", kernel), ("streaming" if narrows is None else "two_pass",
                                                  two_pass)):
                dst.zero_()
                best, med, ev_best, ev_med = timeit(fn)
                results[what] = (scratch if what == "streaming" else dst).clone()
                # the two paths' outputs at the timed size, bit for bit
                same = all(torch.equal(r.view(torch.uint8), results["regions"].view(torch.uint8))
                           for r in results.values())
                print(json.dumps({"kernel": f"{what}_{name}_{fmt}", "dtype": str(dtype),
                                  "same_bits_as_regions": same,
                                  "ms_median": round(med * 1e3, 4),
                                  "event_ms_best": round(ev_best * 1e3, 4),
                                  "event_ms_median": round(ev_med * 1e3, 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", choices=("bf16", "f32"), default="bf16")
    ap.add_argument("--offset", action="store_true")
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--mi-elems", type=int, default=512)
    ap.add_argument("modes", nargs="*", default=["mx_e8m0", "none", "hadamard32"])
    args = ap.parse_args()
    dev = 0
    torch.cuda.set_device(dev)
    modes = args.modes * args.rounds
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if "regions" in args.modes:
        return regions_mode(dtype, args.rounds)
    off = 1 if args.offset else 0
    nw = args.mi_elems << 20
    w = torch.empty(nw + off, dtype=dtype, device="cuda:0").normal_()[off:]
    hs = int(torch.cuda.current_stream().cuda_stream)
    for mode in modes:
        if mode in ("probe", "probe_mx"):
            out = native.quant_probe_buffer(w.device)
            mask = 15 if mode == "probe" else 13
            reads = 2 if mode == "probe" else 1
            best, med, ev_best, ev_med = timeit(lambda: native.quant_probe(dev, w, mask, out, hs))
            tensor = nw * w.element_size()
            print(json.dumps({"kernel": mode, "ms_best": round(best * 1e3, 4),
                              "TBps_best": round(reads * tensor / best / 1e12, 3),
                              "TBps_median": round(reads * tensor / med / 1e12, 3),
                              "traffic_bytes": reads * tensor, "elems": nw,
                              "event_ms_best": round(ev_best * 1e3, 4),
                              "event_ms_median": round(ev_med * 1e3, 4),
                              "tensor_GBps_event_median": round(tensor / ev_med / 1e9, 1)}),
                  flush=True)
            continue
        if mode == "mx_e8m0":
            info = quant.fp8_entry_quant_info(w, rotation="none")
        elif mode in ("mxfp4", "mxfp4_hadamard32", "mxfp6", "nvfp4"):
            os.environ["HIPSNAPSHOT_FP8_FORMAT"] = mode
            info = quant.fp8_entry_quant_info(w, rotation=None if "hadamard" in mode else "none")
            del os.environ["HIPSNAPSHOT_FP8_FORMAT"]
        else:
            os.environ["HIPSNAPSHOT_FP8_FORMAT"] = "block"
            info = quant.fp8_entry_quant_info(w, rotation=mode)
            del os.environ["HIPSNAPSHOT_FP8_FORMAT"]
        blob = torch.zeros(info["total_bytes"], dtype=torch.uint8, device="cuda:0")
        p = info["payload_bytes"]
        e8m0 = mode in ("mx_e8m0", "mxfp4", "mxfp4_hadamard32", "mxfp6", "nvfp4")  # byte scales
        sc = blob[p:] if e8m0 else blob[p:].view(torch.float32)
        back = torch.empty(nw + off, dtype=dtype, device="cuda:0")[off:]
        if mode == "mx_e8m0":
            q = lambda: native.mx8_quantize(dev, w, blob[:p], sc, hs)  # noqa: E731
            dq = lambda: native.mx8_dequantize(dev, blob[:nw], sc, back, hs)  # noqa: E731
        elif mode == "mxfp4":
            q = lambda: native.mxfp4_quantize(dev, w, blob[:p], sc, hs)  # noqa: E731
            dq = lambda: native.mxfp4_dequantize(dev, blob[:p], sc, back, hs)  # noqa: E731
        elif mode == "nvfp4":
            sc, am = blob[p: -4], blob[-4:]
            q = lambda: native.nvfp4_quantize(dev, w, blob[:p], sc, am, hs)  # noqa: E731
            dq = lambda: native.nvfp4_dequantize(dev, blob[:p], sc, am, back, hs)  # noqa: E731
        elif mode == "mxfp6":
            q = lambda: native.mxfp6_quantize(dev, w, blob[:p], sc, hs)  # noqa: E731
            dq = lambda: native.mxfp6_dequantize(dev, blob[:p], sc, back, hs)  # noqa: E731
        elif mode == "mxfp4_hadamard32":
            q = lambda: native.mxfp4_hadamard_quantize(dev, w, blob[:p], sc, hs)  # noqa: E731
            dq = lambda: native.mxfp4_hadamard_dequantize(dev, blob[:p], sc, back, hs)  # noqa
        elif mode == "none":
            q = lambda: native.fp8_quantize(dev, w, blob[:p], sc, info["vpt"], hs)  # noqa: E731
            dq = lambda: native.fp8_dequantize(dev, blob[:nw], sc, back, info["vpt"], hs)  # noqa
        else:
            q = lambda: native.fp8_hadamard_quantize(dev, w, blob[:p], sc, hs)  # noqa: E731
            dq = lambda: native.fp8_hadamard_dequantize(dev, blob[:p], sc, back, hs)  # noqa
        for name, fn in (("quant", q), ("dequant", dq)):
            reads = 2 if (mode, name) == ("nvfp4", "quant") else 1
            traffic = reads * nw * w.element_size() + info["total_bytes"]
            best, med, ev_best, ev_med = timeit(fn)
            tensor = nw * w.element_size()
            print(json.dumps({"kernel": f"{name}_{mode}", "ms_best": round(best * 1e3, 4),
                              "TBps_best": round(traffic / best / 1e12, 3),
                              "TBps_median": round(traffic / med / 1e12, 3),
                              "traffic_bytes": traffic, "elems": nw,
                              "event_ms_best": round(ev_best * 1e3, 4),
                              "event_ms_median": round(ev_med * 1e3, 4),
                              "tensor_GBps_event_median": round(tensor / ev_med / 1e9, 1)}),
                  flush=True)
        del blob, back


if __name__ == "__main__":
    main()
