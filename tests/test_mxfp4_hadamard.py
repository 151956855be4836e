"""Hadamard-rotated MXFP4 torch references against float64; a host take / restore (CPU)."""

import math

import numpy as np
import pytest
import torch

import fp8_oracle as O
from hipsnapshot import Snapshot, StateDict, knobs
from hipsnapshot.ops import quant
from hipsnapshot.utils.test_utils import env
from test_mxfp4 import DST_DTYPES, MAGS, QUIET_NAN, SRC_DTYPES, values

H64 = O.hadamard64()


def exact_sum(n, dtype, seed=0):
    """Multiples of 1/8 up to 31 (Student-t(2)): every sum of a rotation is exact in fp32."""
    t = np.random.default_rng(seed).standard_t(2, size=n)
    return torch.from_numpy(np.clip(np.round(16 * t) / 8, -31, 31)).to(dtype)


def edge_blob(nblocks=8):
    """Seeded codes; scale bytes 0, 1, 0xFE, 0xFF: subnormal products, overflow, NaN group."""
    payload = np.random.default_rng(1).integers(0, 256, 16 * nblocks, dtype=np.uint8)
    sbytes = np.array([0, 1, 0xFE, 0xFF, 127, 5, 250, 130][:nblocks], dtype=np.uint8)
    return torch.from_numpy(payload), torch.from_numpy(sbytes)


def oracle_restore_bits(payload, sbytes, n, dst):
    """float64 ``decode @ H * 2^(k - 5)``, rounded to fp32 and once to ``dst``."""
    p, s = payload.numpy(), sbytes.numpy().astype(np.int64)[:, None]
    codes = np.stack([p & 0xF, p >> 4], axis=1).reshape(-1, 32)
    z = (np.where(codes & 8, -1.0, 1.0) * MAGS[codes & 7]) @ H64
    with np.errstate(over="ignore"):
        f32 = np.ldexp(z, np.where(s == 0xFF, 0, s - 132)).astype(np.float32)
    bits = O.round_dst_bits(f32.reshape(-1), dst).reshape(-1, 32)
    return np.where(s == 0xFF, QUIET_NAN[dst], bits).reshape(-1)[:n]


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1024 + 35])
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_references_vs_float64(dtype, n):
    x = exact_sum(n, dtype)
    payload, sbytes = quant.mxfp4_hadamard_quantize_reference(x)
    x64 = np.zeros((n + 31) // 32 * 32)
    x64[:n] = x.double().numpy()
    want = quant.mxfp4_quantize_reference(torch.from_numpy(x64.reshape(-1, 32) @ H64).float())
    assert torch.equal(sbytes, want[1]) and torch.equal(payload, want[0])
    assert payload.numel() == 16 * sbytes.numel() == (n + 31) // 32 * 16
    for blob in ((payload, sbytes), edge_blob()):
        m = min(n, 32 * blob[1].numel())
        for dst in DST_DTYPES:
            out = quant.mxfp4_hadamard_dequantize_reference(*blob, m, dst)
            assert np.array_equal(O.bits_of(out), oracle_restore_bits(*blob, m, dst)), dst


def test_non_finite_groups():
    """Groups 1 (inf), 3 (NaN), 5 (rotation overflows): 0xFF, zeros, 32 NaNs; others untouched."""
    clean = exact_sum(7 * 32, torch.float32)
    x = clean.clone()
    x[32 + 3], x[3 * 32 + 7], x[5 * 32: 6 * 32] = -math.inf, math.nan, 3e38
    payload, sbytes = quant.mxfp4_hadamard_quantize_reference(x)
    ref_p, ref_s = quant.mxfp4_hadamard_quantize_reference(clean)
    out = quant.mxfp4_hadamard_dequantize_reference(payload, sbytes, x.numel(), torch.float32)
    odd = torch.arange(7) % 2 == 1
    assert (sbytes[odd] == 0xFF).all() and not payload.view(7, 16)[odd].any()
    assert torch.equal(sbytes[~odd], ref_s[~odd])
    assert torch.equal(payload.view(7, 16)[~odd], ref_p.view(7, 16)[~odd])
    assert torch.equal(out.isnan().view(7, 32), odd[:, None].expand(7, 32))


def test_rotation_lowers_heavy_tail_error():
    x = torch.from_numpy(np.random.default_rng(0).standard_t(2, size=1 << 16)).float()
    n = x.numel()
    plain = quant.mxfp4_dequantize_reference(*quant.mxfp4_quantize_reference(x), n, torch.float32)
    rot = quant.mxfp4_hadamard_dequantize_reference(
        *quant.mxfp4_hadamard_quantize_reference(x), n, torch.float32)
    assert (rot - x).norm() < (plain - x).norm()


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_host_take_and_restore(tmp_path, dtype):
    w = values("randn", 257 * 129, dtype).view(257, 129)
    w[5, 7] = math.inf
    path, n, nblocks = tmp_path / "s", w.numel(), (w.numel() + 31) // 32
    with env(HIPSNAPSHOT_FP8_FORMAT="mxfp4_hadamard32"):
        assert "mxfp4_hadamard32" in knobs.plan_settings()
        Snapshot.take(str(path), {"sd": StateDict(w=w)}, quantize=["sd/w"])
    e = Snapshot(str(path)).get_manifest()["0/sd/w"]
    assert e.quant == {"format": "fp4_e2m1_mx", "block": 32, "scale": "e8m0",
                       "rotation": "hadamard32", "orig_dtype": str(dtype),
                       "payload_bytes": 16 * nblocks, "nblocks": nblocks,
                       "total_bytes": 17 * nblocks}
    assert (path / e.location).stat().st_size == 17 * nblocks
    out = torch.zeros_like(w)
    Snapshot(str(path)).restore({"sd": StateDict(w=out)})
    ref = quant.mxfp4_hadamard_dequantize_reference(
        *quant.mxfp4_hadamard_quantize_reference(w), n, dtype)
    assert np.array_equal(O.bits_of(out), O.bits_of(ref))
    assert out.isnan().sum() == 32  # the inf's whole group
