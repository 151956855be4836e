"""MXFP4 torch reference vs a float64 oracle; a host-tensor take / restore (CPU)."""

import math

import numpy as np
import pytest
import torch

import fp8_oracle as O
from hipsnapshot import Snapshot, StateDict, knobs
from hipsnapshot.ops import quant
from hipsnapshot.utils.test_utils import env

MAGS = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
SRC_DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DST_DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64]
QUIET_NAN = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00, torch.float32: 0x7FC00000,
             torch.float64: 0x7FF8 << 48}


def values(kind, n, dtype):
    """``fp8_oracle.build_values``, or "ties": per block 6 * 2^p (fixes k = p),
    then the 7 grid midpoints times 2^p, each with its two ``dtype`` neighbours."""
    if kind != "ties":
        return O.build_values(kind, n, dtype, 32)
    ps = [0, -3, 5, -8, 7, -10] if dtype == torch.float16 else [0, -3, 5, -20, 30, -100, 100]
    v = np.zeros(((n + 31) // 32, 32))
    for b in range(v.shape[0]):
        p = ps[b % len(ps)]
        v[b, 0] = math.ldexp(6.0, p) * (-1.0 if b % 3 == 2 else 1.0)
        for j, mid in enumerate((MAGS[:-1] + MAGS[1:]) / 2.0):
            v[b, 1 + 3 * j: 4 + 3 * j] = math.ldexp(mid, p) * (-1.0 if (b + j) % 2 else 1.0)
    t = torch.from_numpy(v).to(dtype)
    bits = t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    bits[:, 2:22:3] += 1  # away from zero
    bits[:, 3:23:3] -= 1  # toward zero
    return t.reshape(-1)[:n].contiguous()


def oracle_quant(x64, neg):
    """Exact float64: k by comparisons with 6 * 2^k, nearest magnitude, ties to even."""
    n, nb = x64.size, (x64.size + 31) // 32
    codes, sbytes = np.zeros(nb * 32, dtype=np.uint8), np.zeros(nb, dtype=np.uint8)
    xa, sign = np.zeros(nb * 32), np.zeros(nb * 32, dtype=np.uint8)
    xa[:n], sign[:n] = np.abs(x64), neg
    for b in range(nb):
        a = xa[b * 32: (b + 1) * 32]
        if np.isnan(a).any():
            sbytes[b] = 0xFF
            continue
        amax = float(np.where(np.isfinite(a), a, 0.0).max())
        k = math.frexp(amax)[1]
        while amax > 0.0 and amax <= math.ldexp(6.0, k - 1):
            k -= 1
        while amax > math.ldexp(6.0, k):
            k += 1
        k = max(-127, min(127, k)) if amax > 0.0 else 0
        sbytes[b] = k + 127
        d = np.abs(np.minimum(np.ldexp(a, -k), 6.0)[:, None] - MAGS[None, :])  # inf -> 6
        tie = d == d.min(axis=1)[:, None]
        even = tie & (np.arange(8) % 2 == 0)
        idx = np.where(even.any(axis=1), even.argmax(axis=1), tie.argmax(axis=1))
        codes[b * 32: (b + 1) * 32] = idx | (sign[b * 32: (b + 1) * 32] << 3)
    return codes[:n], sbytes


def oracle_restore_bits(codes, sbytes, dst):
    """Bits of float32(q * 2^k) rounded once to ``dst``; quiet NaN for 0xFF."""
    s = np.repeat(sbytes.astype(np.int64), 32)[: codes.size]
    q = np.where(codes & 8, -1.0, 1.0) * MAGS[codes & 7]
    with np.errstate(over="ignore"):
        f32 = np.ldexp(q, np.where(s == 0xFF, 0, s - 127)).astype(np.float32)
    return np.where(s == 0xFF, QUIET_NAN[dst], O.round_dst_bits(f32, dst))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4096 + 35])
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_reference_vs_float64_oracle(dtype, n):
    for kind in ("sweep", "special", "randn", "ties"):
        x = values(kind, n, dtype)
        payload, sbytes = quant.mxfp4_quantize_reference(x)
        want_codes, want_s = oracle_quant(*O.source_arrays(x))
        assert np.array_equal(sbytes.numpy(), want_s), (kind, sbytes, want_s)
        nibbles = np.stack([payload.numpy() & 0xF, payload.numpy() >> 4], axis=1).reshape(-1)
        bad = np.flatnonzero(nibbles[:n] != want_codes)
        assert bad.size == 0, (kind, int(bad[0]), x[int(bad[0])], want_codes[bad[0]])
        # the odd element's neighbour and the padding
        assert payload.numel() == ((n + 1) // 2 + 15) // 16 * 16 and not nibbles[n:].any(), kind
        for dst in DST_DTYPES:
            out = quant.mxfp4_dequantize_reference(payload, sbytes, n, dst)
            assert np.array_equal(O.bits_of(out), oracle_restore_bits(want_codes, want_s, dst)), \
                (kind, dst)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_host_take_and_restore(tmp_path, dtype):
    w = values("randn", 257 * 129, dtype).view(257, 129)
    w[3, :40], w[5, 7], w[9, 1] = 0.0, math.inf, math.nan
    path, n = tmp_path / "s", w.numel()
    with env(HIPSNAPSHOT_FP8_FORMAT="fp4"):  # unknown: the default
        assert knobs.fp8_format() == "mx"
    with env(HIPSNAPSHOT_FP8_FORMAT="mxfp4"):
        Snapshot.take(str(path), {"sd": StateDict(w=w)}, quantize=["sd/w"])
    e = Snapshot(str(path)).get_manifest()["0/sd/w"]
    total = ((n + 1) // 2 + 15) // 16 * 16 + (n + 31) // 32
    assert e.quant == {"format": "fp4_e2m1_mx", "block": 32, "scale": "e8m0", "rotation": "none",
                       "orig_dtype": str(dtype), "payload_bytes": total - (n + 31) // 32,
                       "nblocks": (n + 31) // 32, "total_bytes": total}
    assert (path / e.location).stat().st_size == total
    out = torch.zeros_like(w)
    Snapshot(str(path)).restore({"sd": StateDict(w=out)})
    ref = quant.mxfp4_dequantize_reference(*quant.mxfp4_quantize_reference(w), n, dtype)
    assert np.array_equal(O.bits_of(out), O.bits_of(ref))
    assert out.isnan().sum() == 32  # the NaN's whole block
