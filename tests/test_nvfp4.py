"""Two-level-scaled FP4 (``nvfp4``): the torch reference vs a NumPy oracle that
applies the rules with explicit ``np.float32`` operations and exact e4m3 / e2m1
tables; a host-tensor take / restore (CPU)."""

import math

import numpy as np
import pytest
import torch

import fp8_oracle as O
from hipsnapshot import Snapshot, StateDict
from hipsnapshot.ops import quant
from hipsnapshot.utils.test_utils import env
from test_mxfp4 import DST_DTYPES, MAGS, QUIET_NAN, SRC_DTYPES

F32 = np.float32  # (its division and product are correctly rounded)
KINDS = ("sweep", "special", "randn", "ties", "peak")


def values(kind, n, dtype):
    """``fp8_oracle.build_values`` with blocks of 16, or "peak": N(0, 9) whose
    largest magnitude, -48, is the last element (the first blocks get scale
    bytes from the middle of the e4m3 range), or "ties": every scale is a power
    of two -- element 0 is 2688 * 2^q (ts = 2^q), every later block leads with
    6 * 2^p (s8 = 2^(p - q), d = 2^p) and goes on with five of the seven e2m1
    midpoints times 2^p, each with its two ``dtype`` neighbours."""
    if kind == "peak":
        t = O.build_values("randn", n, dtype, 16).clone()
        t[n - 1] = -48.0
        return t
    if kind != "ties":
        return O.build_values(kind, n, dtype, 16)
    q = 0 if dtype == torch.float16 else -20
    mids = (MAGS[:-1] + MAGS[1:]) / 2.0
    v = np.zeros(((n + 15) // 16, 16))
    v[0, 0] = math.ldexp(2688.0, q)
    for b in range(1, v.shape[0]):
        p = q + (0, -3, 5, -9, 8, -6)[b % 6]  # 2^(p - q) is an e4m3 value: 2^-9 .. 2^8
        v[b, 0] = math.ldexp(6.0, p) * (-1.0 if b % 3 == 2 else 1.0)
        for j in range(5):
            v[b, 1 + 3 * j: 4 + 3 * j] = math.ldexp(mids[(5 * b + j) % 7], p) * (-1.0) ** (b + j)
    t = torch.from_numpy(v).to(dtype)
    bits = t.view(torch.int16 if t.element_size() == 2 else torch.int32)
    bits[1:, 2:16:3] += 1  # away from zero
    bits[1:, 3:16:3] -= 1  # toward zero
    return t.reshape(-1)[:n].contiguous()


def tensor_scale(amax):
    return max(F32(amax) / F32(2688.0), F32(2.0 ** -117))


def oracle_quant(x):
    """(codes[16 nb], scale bytes[nb], A) by the rules, one np.float32 operation per step."""
    x64, neg = O.source_arrays(x)
    n, nb = x64.size, (x64.size + 15) // 16
    a, sign = np.zeros(nb * 16, dtype=F32), np.zeros(nb * 16, dtype=np.uint8)
    a[:n], sign[:n] = np.abs(x64).astype(F32), neg  # the widening of a source value is exact
    a = a.reshape(nb, 16)
    fa = np.where(np.isfinite(a), a, F32(0.0))
    amax = fa.max()
    ts = tensor_scale(amax)
    quot = np.minimum(fa.max(axis=1) / (F32(6.0) * ts), F32(448.0))
    s8 = O.encode_e4m3_rne(quot.astype(np.float64))
    d = O.E4M3[s8].astype(F32) * ts
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        y = np.minimum(a * (F32(1.0) / d)[:, None], F32(6.0))
    dist = np.abs(np.nan_to_num(y.astype(np.float64))[:, :, None] - MAGS)
    tie = dist == dist.min(axis=2)[:, :, None]
    even = tie & (np.arange(8) % 2 == 0)
    idx = np.where(even.any(axis=2), even.argmax(axis=2), tie.argmax(axis=2))
    idx = np.where((d > 0)[:, None], idx, 0)  # s8 == 0: the sign alone
    codes = idx.astype(np.uint8) | (sign.reshape(nb, 16) << 3)
    has_nan = np.isnan(a).any(axis=1)
    codes[has_nan] = 0
    return codes.reshape(-1), np.where(has_nan, 0x7F, s8).astype(np.uint8), amax


def oracle_restore_bits(codes, sbytes, amax, dst):  # f32(q * f32(f32(s8) * ts)), one rounding
    s = np.repeat(sbytes, 16)[: codes.size]
    nan = (s & 0x7F) == 0x7F
    d = O.E4M3[np.where(nan, 0, s)].astype(F32) * tensor_scale(amax)
    f32 = (np.where(codes & 8, -1.0, 1.0) * MAGS[codes & 7]).astype(F32) * d
    return np.where(nan, QUIET_NAN[dst], O.round_dst_bits(f32, dst))


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4096 + 35])
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_reference_vs_numpy_oracle(dtype, n):
    nb = (n + 15) // 16
    for kind in KINDS:
        x = values(kind, n, dtype)
        payload, sbytes, amax = quant.nvfp4_quantize_reference(x)
        want_codes, want_s, want_a = oracle_quant(x)
        assert amax.numpy().view(np.uint32) == want_a.view(np.uint32), (kind, amax, want_a)
        assert np.array_equal(sbytes.numpy(), want_s), (kind, sbytes, want_s)
        nibbles = np.stack([payload.numpy() & 0xF, payload.numpy() >> 4], axis=1).reshape(-1)
        bad = np.flatnonzero(nibbles[: 16 * nb] != want_codes)  # elements past n are code 0
        assert bad.size == 0, (kind, int(bad[0]), x[int(bad[0])], want_codes[bad[0]])
        assert payload.numel() == ((n + 1) // 2 + 15) // 16 * 16 and not nibbles[n:].any(), kind
        for dst in DST_DTYPES:
            out = quant.nvfp4_dequantize_reference(payload, sbytes, amax, n, dst)
            want = oracle_restore_bits(want_codes[:n], want_s, want_a, dst)
            assert np.array_equal(O.bits_of(out), want), (kind, dst)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_host_take_and_restore(tmp_path, dtype):
    w = values("peak", 257 * 129, dtype).view(257, 129)
    w[3, :60], w[5, 7], w[9, 1] = 0.0, math.inf, math.nan  # row 3 holds two all-zero blocks
    path, n = tmp_path / "s", w.numel()
    nb, payload = (n + 15) // 16, ((n + 1) // 2 + 15) // 16 * 16
    total = payload + (nb + 3) // 4 * 4 + 4
    with env(HIPSNAPSHOT_FP8_FORMAT="nvfp4"):
        Snapshot.take(str(path), {"sd": StateDict(w=w)}, quantize=["sd/w"])
    e = Snapshot(str(path)).get_manifest()["0/sd/w"]
    assert e.quant == {"format": "fp4_e2m1_nv", "block": 16, "scale": "e4m3+fp32",
                       "rotation": "none", "orig_dtype": str(dtype), "nblocks": nb,
                       "payload_bytes": payload, "total_bytes": total}
    q, sbytes, amax = quant.nvfp4_quantize_reference(w)
    assert amax.item() == 48.0 and (sbytes == 0).sum() >= 2 and (sbytes == 0x7F).sum() == 1
    blob = np.fromfile(path / e.location, dtype=np.uint8)
    pad = np.zeros(total - 4 - payload - nb, dtype=np.uint8)
    assert np.array_equal(blob, np.concatenate([q.numpy(), sbytes.numpy(), pad,
                                                amax.numpy().view(np.uint8)]))
    out = torch.zeros_like(w)
    Snapshot(str(path)).restore({"sd": StateDict(w=out)})
    ref = quant.nvfp4_dequantize_reference(q, sbytes, amax, n, dtype)
    assert np.array_equal(O.bits_of(out), O.bits_of(ref))
    assert out.isnan().sum() == 16  # the NaN's whole block
