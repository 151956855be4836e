"""MXFP6 torch reference vs a float64 oracle; a host-tensor take / restore (CPU)."""

import math

import numpy as np
import pytest
import torch

import fp8_oracle as O
from hipsnapshot import Snapshot, StateDict
from hipsnapshot.ops import quant
from hipsnapshot.utils.test_utils import env
from test_mxfp4 import DST_DTYPES, QUIET_NAN, SRC_DTYPES

MAGS = np.concatenate([np.arange(16) / 8.0, 2.0 + np.arange(8) / 4.0, 4.0 + np.arange(8) / 2.0])
KINDS = ("sweep", "special", "randn", "ties")


def values(kind, n, dtype):
    """``fp8_oracle.build_values``, or "ties": element 0 of a block is 7.5 * 2^p
    (fixes k = p); the 31 grid midpoints times 2^p, each with its two ``dtype``
    neighbours, fill the other 31 elements of three consecutive blocks."""
    if kind != "ties":
        return O.build_values(kind, n, dtype, 32)
    ps = [0, -3, 5, -8, 7, -10] if dtype == torch.float16 else [0, -3, 5, -20, 30, -100, 100]
    mids = np.repeat((MAGS[:-1] + MAGS[1:]) / 2.0, 3) * np.where(np.arange(93) % 2, -1.0, 1.0)
    v = np.zeros(((n + 31) // 32, 32))
    for b in range(v.shape[0]):
        p = ps[(b // 3) % len(ps)]
        v[b, 0] = math.ldexp(7.5, p) * (-1.0 if b % 5 == 2 else 1.0)
        v[b, 1:] = np.ldexp(mids[31 * (b % 3): 31 * (b % 3) + 31], p)
    t = torch.from_numpy(v).to(dtype)
    bits = t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    step = (torch.arange(93) % 3).view(3, 31)[torch.arange(v.shape[0]) % 3]
    bits[:, 1:] += (step == 1).to(bits.dtype) - (step == 2).to(bits.dtype)  # away from / toward 0
    return t.reshape(-1)[:n].contiguous()


def oracle_quant(x64, neg):
    """Exact float64: k by comparisons with 7.5 * 2^k, nearest magnitude, ties to even."""
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
        k = -200
        while amax > math.ldexp(7.5, k):  # the smallest k with amax <= 7.5 * 2^k
            k += 1
        k = max(-127, min(127, k)) if amax > 0.0 else 0
        sbytes[b] = k + 127
        d = np.abs(np.minimum(np.ldexp(a, -k), 7.5)[:, None] - MAGS[None, :])  # inf -> 7.5
        tie = d == d.min(axis=1)[:, None]
        even = tie & (np.arange(32) % 2 == 0)
        idx = np.where(even.any(axis=1), even.argmax(axis=1), tie.argmax(axis=1))
        codes[b * 32: (b + 1) * 32] = idx | (sign[b * 32: (b + 1) * 32] << 5)
    return codes, sbytes


def unpack_codes(payload, nblocks):  # element j of block b: bits [6 j, 6 j + 6) of its 24 bytes
    bits = np.unpackbits(payload[: 24 * nblocks], bitorder="little").reshape(-1, 6)
    return (bits << np.arange(6)).sum(axis=1).astype(np.uint8)


def oracle_restore_bits(codes, sbytes, dst):  # float32(q * 2^k) rounded once; 0xFF: quiet NaN
    s = np.repeat(sbytes.astype(np.int64), 32)[: codes.size]
    q = np.where(codes & 32, -1.0, 1.0) * MAGS[codes & 31]
    with np.errstate(over="ignore"):
        f32 = np.ldexp(q, np.where(s == 0xFF, 0, s - 127)).astype(np.float32)
    return np.where(s == 0xFF, QUIET_NAN[dst], O.round_dst_bits(f32, dst))


@pytest.mark.parametrize("n", [1, 31, 32, 33, 4096 + 35])
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_reference_vs_float64_oracle(dtype, n):
    nb = (n + 31) // 32
    for kind in KINDS:
        x = values(kind, n, dtype)
        payload, sbytes = quant.mxfp6_quantize_reference(x)
        want_codes, want_s = oracle_quant(*O.source_arrays(x))
        assert np.array_equal(sbytes.numpy(), want_s), (kind, sbytes, want_s)
        got = unpack_codes(payload.numpy(), nb)
        bad = np.flatnonzero(got != want_codes)  # all 32 * nb: elements past n are code 0
        assert bad.size == 0, (kind, int(bad[0]), x[int(bad[0])], got[bad[0]], want_codes[bad[0]])
        assert payload.numel() == (24 * nb + 15) // 16 * 16 and not payload[24 * nb:].any(), kind
        for dst in DST_DTYPES:
            out = quant.mxfp6_dequantize_reference(payload, sbytes, n, dst)
            want = oracle_restore_bits(want_codes[:n], want_s, dst)
            assert np.array_equal(O.bits_of(out), want), (kind, dst)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_host_take_and_restore(tmp_path, dtype):
    w = values("randn", 257 * 129, dtype).view(257, 129)
    w[3, :40], w[5, 7], w[9, 1] = 0.0, math.inf, math.nan
    path, n = tmp_path / "s", w.numel()
    nb = (n + 31) // 32
    with env(HIPSNAPSHOT_FP8_FORMAT="mxfp6"):
        Snapshot.take(str(path), {"sd": StateDict(w=w)}, quantize=["sd/w"])
    e = Snapshot(str(path)).get_manifest()["0/sd/w"]
    payload = (24 * nb + 15) // 16 * 16
    assert e.quant == {"format": "fp6_e2m3_mx", "block": 32, "scale": "e8m0", "rotation": "none",
                       "orig_dtype": str(dtype), "nblocks": nb, "payload_bytes": payload,
                       "total_bytes": payload + nb}
    assert (path / e.location).stat().st_size == payload + nb
    out = torch.zeros_like(w)
    Snapshot(str(path)).restore({"sd": StateDict(w=out)})
    ref = quant.mxfp6_dequantize_reference(*quant.mxfp6_quantize_reference(w), n, dtype)
    assert np.array_equal(O.bits_of(out), O.bits_of(ref))
    assert out.isnan().sum() == 32  # the NaN's whole block
