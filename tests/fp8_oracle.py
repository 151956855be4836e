"""float64 oracle of the fp8 checkpoint formats (MX e8m0, blockwise fp32-scale,
Hadamard-rotated), independent of ``hipsnapshot.ops.quant`` and of torch's
float8 cast.  Imported by ``test_fp8_oracle.py`` (CPU) and
``test_gpu_fp8_oracle.py`` (GPU) the way ``dist_workers`` is.

Everything here runs on the CPU in float64 NumPy.  e4m3fn codes are decoded
through a table built from the bit fields, the exact round-to-nearest-even code
of a value comes from ``np.rint`` on the scaled mantissa, bf16 rounding is
integer arithmetic on the float32 bits and f16 / f32 rounding is NumPy's.

A ``check_*`` function raises ``AssertionError`` naming the first offending
element, its block and the bound it missed.  The bounds are derived, not tuned:

* ``h(c)`` is half the larger of the two e4m3 grid gaps next to the decoded
  code ``c`` (2^-10 in the subnormal range): what one correct rounding to the
  grid can cost.
* blockwise codes: ``x * fl(1 / s)`` carries two fp32 roundings (2 * 2^-24
  relative), so ``|c - clamp(x / s)| <= h(c) + 2^-22 |x / s|``.
* Hadamard: any-order fp32 summation of 32 exact products errs by at most
  ``31 u sum|x| (1 + O(u))`` with ``u = 2^-24``; ``delta_r = 32 u sum|x|`` bounds
  it with ``u sum|x|`` to spare, which also absorbs the second-order term
  ``2^-23 delta_r`` of the later fp32 roundings.  The float64 rotation here errs
  by ``2^-53 sum|x|``, 2^34 times below ``delta_r``.
"""

from __future__ import annotations

import math

import numpy as np
import torch

FP8_MAX = 448.0
MIN_SCALE = 2.0 ** -126  # floor of a blockwise fp32 scale (smallest normal float32)
MX_BLOCK = 32
GROUP = 32
HAD_BLOCK = 128


# ---------------------------------------------------------------------------
# e4m3fn
# ---------------------------------------------------------------------------

def _build_e4m3_table() -> np.ndarray:
    t = np.empty(256, dtype=np.float64)
    for b in range(256):
        sign = -1.0 if b & 0x80 else 1.0
        e, m = (b >> 3) & 0xF, b & 0x7
        if e == 0xF and m == 0x7:
            v = math.nan  # 0x7f / 0xff; the format has no infinities
        elif e == 0:
            v = m * 2.0 ** -9
        else:
            v = (1.0 + m / 8.0) * 2.0 ** (e - 7)
        t[b] = sign * v
    return t


E4M3 = _build_e4m3_table()
_GRID = np.sort(E4M3[:0x7F])  # the 127 non-negative finite values, 0 .. 448


def _build_half_gap() -> np.ndarray:
    h = np.empty(256, dtype=np.float64)
    for b in range(256):
        a = b & 0x7F
        if a == 0x7F:
            h[b] = math.nan
            continue
        below = _GRID[a] - _GRID[a - 1] if a > 0 else _GRID[1] - _GRID[0]
        above = _GRID[a + 1] - _GRID[a] if a < 0x7E else below
        h[b] = max(below, above) / 2.0
    return h


HALF_GAP = _build_half_gap()


def decode_e4m3(codes: np.ndarray) -> np.ndarray:
    return E4M3[np.asarray(codes, dtype=np.uint8)]


def encode_e4m3_rne(v: np.ndarray, neg: np.ndarray = None) -> np.ndarray:
    """Exact round-to-nearest-even e4m3fn code of finite float64 ``v``: spacing
    2^-9 below 2^-6, 3 mantissa bits above.  A magnitude that rounds past 448
    gives the NaN code (the cast does not saturate)."""
    v = np.asarray(v, dtype=np.float64)
    a = np.abs(v)
    neg = np.signbit(v) if neg is None else neg
    sub = np.rint(a * 2.0 ** 9)  # 0 .. 8; 8 is the code of 2^-6
    m, e = np.frexp(a)  # a = m * 2^e, m in [0.5, 1)
    r = np.rint(m * 16.0)  # 8 .. 16
    carry = r == 16.0
    r = np.where(carry, 8.0, r)
    e = e + carry
    biased = e + 6
    norm = biased * 8 + (r.astype(np.int64) - 8)
    code = np.where(a < 2.0 ** -6, sub.astype(np.int64), norm)
    code = np.where((a >= 2.0 ** -6) & (norm >= 0x7F), 0x7F, code)
    return (code | np.where(neg, 0x80, 0)).astype(np.uint8)


# ---------------------------------------------------------------------------
# source / destination number formats
# ---------------------------------------------------------------------------

def source_arrays(t: torch.Tensor):
    """(float64 values, sign bits) of a CPU bf16 / f16 / f32 tensor.  Widening
    is exact; the sign is read from the raw bits (a NaN keeps its own)."""
    t = t.detach().reshape(-1).contiguous()
    assert t.device.type == "cpu"
    if t.element_size() == 2:
        neg = t.view(torch.int16).numpy() < 0
    else:
        neg = t.view(torch.int32).numpy() < 0
    return t.double().numpy(), neg


def bits_of(t: torch.Tensor) -> np.ndarray:
    t = t.detach().reshape(-1).contiguous()
    view = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    return t.view(view).numpy()


def _round_bf16_bits(f32: np.ndarray) -> np.ndarray:
    b = f32.view(np.uint32).astype(np.uint64)
    r = (b + 0x7FFF + ((b >> 16) & 1)) >> 16  # RNE on the upper half; carries into inf
    return r.astype(np.uint16).view(np.int16)


def round_dst_bits(f32: np.ndarray, dst: torch.dtype) -> np.ndarray:
    """Bits of float32 ``f32`` rounded once more to ``dst`` (signed ints, as
    ``bits_of`` returns them).  Meaningless where ``f32`` is NaN."""
    f32 = np.ascontiguousarray(f32, dtype=np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        if dst == torch.bfloat16:
            return _round_bf16_bits(f32)
        if dst == torch.float16:
            return f32.astype(np.float16).view(np.int16)
        if dst == torch.float32:
            return f32.view(np.int32)
        if dst == torch.float64:
            return f32.astype(np.float64).view(np.int64)
    raise ValueError(dst)


def _to_f32(v64: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.asarray(v64, dtype=np.float64).astype(np.float32)


def _first(mask: np.ndarray) -> int:
    return int(np.flatnonzero(mask)[0])


def _pad(a: np.ndarray, n: int, fill=0) -> np.ndarray:
    out = np.full(n, fill, dtype=a.dtype)
    out[: a.size] = a
    return out


# ---------------------------------------------------------------------------
# MX: exact
# ---------------------------------------------------------------------------

def mx_exponent(amax: float) -> int:
    """Smallest integer k with amax <= 448 * 2^k, clamped to [-127, 127]; 0 for
    a zero or non-finite amax."""
    if not (amax > 0.0) or math.isinf(amax):
        return 0
    _, e = math.frexp(amax)
    k = e - 9
    while amax > math.ldexp(FP8_MAX, k):
        k += 1
    while amax <= math.ldexp(FP8_MAX, k - 1):
        k -= 1
    return max(-127, min(127, k))


def check_mx_quant(x64, neg, codes, scales) -> None:
    """``codes``: round_up(n, 16) payload bytes, ``scales``: ceil(n / 32) bytes."""
    x64 = np.asarray(x64, dtype=np.float64)
    n = x64.size
    nb = (n + MX_BLOCK - 1) // MX_BLOCK
    payload = (n + 15) // 16 * 16
    codes = np.asarray(codes, dtype=np.uint8)
    scales = np.asarray(scales, dtype=np.uint8)
    assert codes.size == payload and scales.size == nb, (codes.size, payload, scales.size, nb)
    finite = np.isfinite(x64)
    xa = _pad(np.where(finite, np.abs(x64), 0.0), nb * MX_BLOCK).reshape(nb, MX_BLOCK)
    k = np.array([mx_exponent(float(a)) for a in xa.max(axis=1)], dtype=np.int64)
    bad = scales.astype(np.int64) != k + 127
    if bad.any():
        b = _first(bad)
        raise AssertionError(f"mx scale: block {b} (elements {b * 32}..) stores byte {scales[b]}, "
                             f"bound: exactly k + 127 = {k[b] + 127} for amax {xa[b].max()!r}")
    kk = np.repeat(k, MX_BLOCK)[:n]
    want = encode_e4m3_rne(np.ldexp(np.where(finite, x64, 0.0), -kk), neg)
    want = np.where(finite, want, np.where(neg, 0xFF, 0x7F)).astype(np.uint8)
    bad = codes[:n] != want
    if bad.any():
        i = _first(bad)
        raise AssertionError(
            f"mx code: element {i} (block {i // 32}, k = {kk[i]}) x = {x64[i]!r} has code "
            f"0x{codes[i]:02x} = {E4M3[codes[i]]!r}, bound: exactly the RNE code 0x{want[i]:02x} = "
            f"{E4M3[want[i]]!r} of x * 2^-k = {math.ldexp(x64[i], -int(kk[i])) if finite[i] else x64[i]!r}")
    bad = codes[n:] != 0
    if bad.any():
        i = n + _first(bad)
        raise AssertionError(f"mx padding: element {i} (block {i // 32}) is 0x{codes[i]:02x}, "
                             f"bound: padding [{n}, {payload}) is zero")


def check_mx_dequant(codes, scales, out_bits, dst: torch.dtype) -> None:
    n = np.asarray(out_bits).size
    c = decode_e4m3(np.asarray(codes, dtype=np.uint8)[:n])
    k = np.repeat(np.asarray(scales, dtype=np.uint8).astype(np.int64) - 127, MX_BLOCK)[:n]
    with np.errstate(over="ignore", invalid="ignore"):
        f32 = _to_f32(np.ldexp(c, k))
    _compare_restored("mx", f32, out_bits, dst, MX_BLOCK)


def _compare_restored(what, f32, out_bits, dst, block) -> None:
    out_bits = np.asarray(out_bits)
    want = round_dst_bits(f32, dst)
    nan = np.isnan(f32)
    es = out_bits.dtype.itemsize
    fl = {2: np.float16, 4: np.float32, 8: np.float64}[es]
    if dst == torch.bfloat16:
        got_nan = ((out_bits.view(np.uint16) & 0x7F80) == 0x7F80) & \
            ((out_bits.view(np.uint16) & 0x7F) != 0)
    else:
        got_nan = np.isnan(out_bits.view(fl))
    bad = nan & ~got_nan
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what} restore: element {i} (block {i // block}) is bits "
                             f"{int(out_bits[i]):#x}, bound: a NaN code restores as NaN")
    bad = ~nan & (out_bits != want)
    if bad.any():
        i = _first(bad)
        raise AssertionError(
            f"{what} restore to {dst}: element {i} (block {i // block}) is bits {int(out_bits[i]):#x}, "
            f"bound: exactly round_dst(float32(c * s)) = bits {int(want[i]):#x} (float32 {f32[i]!r})")


# ---------------------------------------------------------------------------
# blockwise fp32 scale
# ---------------------------------------------------------------------------

def check_block_quant(x64, neg, codes, scales, block: int) -> None:
    x64 = np.asarray(x64, dtype=np.float64)
    n = x64.size
    nb = (n + block - 1) // block
    codes = np.asarray(codes, dtype=np.uint8)
    scales = np.asarray(scales, dtype=np.float32)
    assert codes.size == n and scales.size == nb, (codes.size, n, scales.size, nb)
    finite = np.isfinite(x64)
    amax = _pad(np.where(finite, np.abs(x64), 0.0), nb * block).reshape(nb, block).max(axis=1)
    quot = amax / FP8_MAX
    want_s = np.where(amax == 0.0, np.float32(1.0),
                      np.where(quot >= MIN_SCALE, _to_f32(quot), np.float32(MIN_SCALE)))
    bad = ~(scales == want_s)
    if bad.any():
        b = _first(bad)
        raise AssertionError(
            f"block scale: block {b} (elements {b * block}..) stores {scales[b]!r}, bound: exactly "
            f"{want_s[b]!r} = float32(max(amax / 448, 2^-126)) for amax {amax[b]!r} (1 if amax == 0)")
    s = np.repeat(scales.astype(np.float64), block)[:n]
    _check_codes("block", x64, finite, neg, codes, s, np.zeros(n), block)


def _check_codes(what, y64, finite, neg, codes, s, delta, block) -> None:
    """|c s - clamp(y, +-448 s)| <= s h(c) + delta + 2^-22 |y| for finite y;
    the NaN code with the input's sign (``neg``; None: either sign) otherwise."""
    n = y64.size
    is_nan_code = (codes & 0x7F) == 0x7F
    if neg is None:
        bad = ~finite & ~is_nan_code
    else:
        bad = ~finite & (codes != np.where(neg, 0xFF, 0x7F))
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what} code: element {i} (block {i // block}) is non-finite and has "
                             f"code 0x{codes[i]:02x}, bound: the NaN code 0x7f / 0xff by its sign")
    bad = finite & is_nan_code
    if bad.any():
        i = _first(bad)
        raise AssertionError(f"{what} code: element {i} (block {i // block}) y = {y64[i]!r} is finite "
                             f"and has the NaN code 0x{codes[i]:02x} (scale {s[i]!r}), bound: a finite code")
    c = np.where(finite, E4M3[codes], 0.0)
    y = np.where(finite, y64, 0.0)
    err = np.abs(c * s - np.clip(y, -FP8_MAX * s, FP8_MAX * s))
    bound = s * np.where(finite, HALF_GAP[codes], 0.0) + delta + 2.0 ** -22 * np.abs(y)
    bad = finite & ~(err <= bound)
    if bad.any():
        i = _first(bad)
        raise AssertionError(
            f"{what} code: element {i} (block {i // block}) y = {y64[i]!r}, scale {s[i]!r}: code "
            f"0x{codes[i]:02x} = {E4M3[codes[i]]!r} is {err[i]!r} from clamp(y), bound "
            f"s h(c) + delta + 2^-22 |y| = {bound[i]!r} (y / s = {y64[i] / s[i] if s[i] else math.nan!r})")


def check_block_dequant(codes, scales, block: int, out_bits, dst: torch.dtype) -> None:
    n = np.asarray(out_bits).size
    c = decode_e4m3(np.asarray(codes, dtype=np.uint8)[:n])
    s = np.repeat(np.asarray(scales, dtype=np.float32).astype(np.float64), block)[:n]
    with np.errstate(invalid="ignore"):
        f32 = _to_f32(c * s)  # a 4-bit by 24-bit product: exact in float64
    _compare_restored("block", f32, out_bits, dst, block)


# ---------------------------------------------------------------------------
# Hadamard-rotated
# ---------------------------------------------------------------------------

def hadamard64(n: int = GROUP) -> np.ndarray:
    i = np.arange(n)
    parity = np.zeros((n, n), dtype=np.int64)
    for b in range(n.bit_length()):
        parity ^= ((i[:, None] & i[None, :]) >> b) & 1
    return 1.0 - 2.0 * parity


def check_hadamard_quant(x64, codes, scales) -> None:
    """``codes``: n_pad = round_up(n, 32) bytes, ``scales``: ceil(n_pad / 128)."""
    x64 = np.asarray(x64, dtype=np.float64)
    n = x64.size
    n_pad = (n + GROUP - 1) // GROUP * GROUP
    nb = (n_pad + HAD_BLOCK - 1) // HAD_BLOCK
    codes = np.asarray(codes, dtype=np.uint8)
    scales = np.asarray(scales, dtype=np.float32)
    assert codes.size == n_pad and scales.size == nb, (codes.size, n_pad, scales.size, nb)
    rpb = HAD_BLOCK // GROUP
    rows = _pad(x64, nb * HAD_BLOCK).reshape(-1, GROUP)
    row_ok = np.isfinite(rows).all(axis=1)  # a non-finite input spoils its own row only
    clean = np.where(row_ok[:, None], rows, 0.0)
    sum_abs = np.abs(clean).sum(axis=1)
    assert sum_abs.max() < 2.0 ** 126, "test input: a row sum could overflow float32"
    y64 = clean @ hadamard64()
    delta_r = 32.0 * 2.0 ** -24 * sum_abs
    amax = np.abs(y64).reshape(nb, -1).max(axis=1)
    delta = delta_r.reshape(nb, rpb).max(axis=1)
    s64 = scales.astype(np.float64)
    slack = delta + 2.0 ** -22 * amax
    # the kernel's fp32 amax lies in amax +- delta: scale 1 if that can be 0,
    # the floor 2^-126 if that can be below 448 * 2^-126, amax / 448 otherwise
    ok = np.abs(FP8_MAX * s64 - amax) <= slack
    ok &= s64 >= MIN_SCALE
    ok |= (s64 == 1.0) & (amax - delta <= 0.0)
    ok |= (s64 == MIN_SCALE) & (amax - slack <= FP8_MAX * MIN_SCALE) & (amax + delta > 0.0)
    if not ok.all():
        b = _first(~ok)
        raise AssertionError(
            f"hadamard scale: block {b} (elements {b * HAD_BLOCK}..) stores {scales[b]!r}, 448 s = "
            f"{FP8_MAX * s64[b]!r}, bound: within delta + 2^-22 amax = {slack[b]!r} of amax(y64) = "
            f"{amax[b]!r}, floored at 2^-126 (1 for a zero block)")
    finite = np.repeat(row_ok, GROUP)[:n_pad]
    s = np.repeat(s64, HAD_BLOCK)[:n_pad]
    _check_codes("hadamard", y64.reshape(-1)[:n_pad], finite, None, codes, s,
                 np.repeat(delta_r, GROUP)[:n_pad], HAD_BLOCK)


def check_hadamard_dequant(codes, scales, out_bits, dst: torch.dtype) -> None:
    """x = float32(rowsum * (s / 32)): the row sums of e4m3 values (multiples
    of 2^-9 below 2^14) are exact; ``s / 32`` is the float32 quotient the
    restore forms first (exact unless s < 2^-121, where it is subnormal and
    rounds once); their product, at most 23 by 24 bits, is exact in float64."""
    n = np.asarray(out_bits).size
    codes = np.asarray(codes, dtype=np.uint8)
    rows = decode_e4m3(codes).reshape(-1, GROUP)
    row_nan = np.isnan(rows).any(axis=1)
    z = np.where(row_nan[:, None], 0.0, rows) @ hadamard64()
    s32 = np.asarray(scales, dtype=np.float32) * np.float32(1.0 / 32.0)
    s = np.repeat(s32.astype(np.float64), HAD_BLOCK // GROUP)[: rows.shape[0]]
    f32 = _to_f32(np.where(row_nan[:, None], math.nan, z * s[:, None])).reshape(-1)[:n]
    _compare_restored("hadamard", f32, out_bits, dst, HAD_BLOCK)


# ---------------------------------------------------------------------------
# value sets: built in float64, cast to the source dtype, shared by the CPU and
# GPU tests
# ---------------------------------------------------------------------------

VALUE_SETS = ("sweep", "decades", "ties", "special", "randn")

# exponents of the per-block sweep, the edges first so that a tensor of a few
# blocks still meets them: whole blocks below 1.3e-36 (2^-119.6), the floor's
# threshold amax = 448 * 2^-126 (2^-117.2), subnormals, and the top
_EDGE_EXP = [-122, 0, -130, -118, -149, 120, -126, -117, -133, -127, -140, -121, -125, 100,
             -119, -120, -60, 60, -20, 20]


def _sweep_exponents(dtype) -> list:
    if dtype == torch.float16:
        edge = [-20, 0, -24, 15, -14, -15, -10, 8]
        lo, hi = -24, 15
    else:
        edge, lo, hi = _EDGE_EXP, -149, 120
    return edge + [e for e in range(lo, hi + 1) if e not in edge]


def _neighbours(t: torch.Tensor, step: int) -> torch.Tensor:
    """Next representable value away from (step = 1) or toward (-1) zero."""
    view = torch.int16 if t.element_size() == 2 else torch.int32
    return (t.view(view) + step).view(t.dtype)


def build_values(kind: str, n: int, dtype: torch.dtype, blk: int, seed: int = 0) -> torch.Tensor:
    """CPU tensor of ``n`` values of ``dtype``; ``blk`` is the block size of
    the format under test (the sets place whole blocks)."""
    rng = np.random.default_rng(seed + 1000 * VALUE_SETS.index(kind))
    nblk = (n + blk - 1) // blk
    tot = nblk * blk
    f16 = dtype == torch.float16
    if kind == "sweep":
        exps = _sweep_exponents(dtype)
        e = np.array([exps[i % len(exps)] for i in range(nblk)], dtype=np.int64)
        m = rng.uniform(1.0, 2.0, size=(nblk, blk)) * rng.choice([-1.0, 1.0], size=(nblk, blk))
        m[rng.random((nblk, blk)) < 0.25] = 0.0  # exact zeros inside every block
        v = np.ldexp(m, e[:, None]).reshape(-1)
    elif kind == "decades":
        lo, hi = (-8.0, 4.5) if f16 else (-40.0, 20.0)  # 60 decades (f16: its whole range)
        v = 10.0 ** rng.uniform(lo, hi, size=tot) * rng.choice([-1.0, 1.0], size=tot)
    elif kind == "ties":
        # every 32: 448 * 2^p (sets the MX exponent to p), then e4m3 midpoints
        # times 2^p, each followed by its two neighbours in the source dtype
        mids = (_GRID[:-1] + _GRID[1:]) / 2.0
        ps = [0, -3, 5, -8, 7, -14] if f16 else [0, -3, 5, -20, 30, -100, 100]
        g = (tot + 31) // 32
        v = np.zeros((g, 32))
        for b in range(g):
            p = ps[b % len(ps)]
            v[b, 0] = math.ldexp(FP8_MAX, p) * (-1.0 if b % 5 == 4 else 1.0)
            for j in range(10):
                mid = mids[(b * 10 + j) % mids.size] * (-1.0 if (b + j) % 2 else 1.0)
                v[b, 1 + 3 * j: 4 + 3 * j] = math.ldexp(mid, p)
            v[b, 31] = math.ldexp(mids[(b * 7) % mids.size], p)
        t = torch.from_numpy(v.reshape(-1)[:tot].copy()).to(dtype)
        t2 = t.view(-1, 32).clone()
        for j in range(10):  # neighbours (the midpoints are exact in every source dtype)
            t2[:, 2 + 3 * j] = _neighbours(t2[:, 2 + 3 * j].contiguous(), 1)
            t2[:, 3 + 3 * j] = _neighbours(t2[:, 3 + 3 * j].contiguous(), -1)
        return t2.reshape(-1)[:n].contiguous()
    elif kind == "special":
        fi = torch.finfo(dtype)
        tiny_sub = fi.smallest_subnormal if hasattr(fi, "smallest_subnormal") else fi.tiny
        v = rng.standard_normal(tot) * 3.0
        head = [0.0, -0.0, math.inf, -math.inf, math.nan, math.nan, fi.max, -fi.max,
                tiny_sub, -tiny_sub, fi.tiny, -fi.tiny, fi.tiny * 0.75, 1.0, -1.0, fi.max / 2]
        v[: len(head)] = head[: min(len(head), tot)]
        if nblk > 1:
            v[blk: 2 * blk] = 0.0  # an all-zero block
        if nblk > 2:
            v[2 * blk: 3 * blk] = 0.0  # a single non-zero value
            v[2 * blk + blk // 2 + 1] = -0.3
        if nblk > 3:
            v[3 * blk: 4 * blk] = 0.0  # the only finite non-zero is tiny, next to an inf
            v[3 * blk + 3] = math.inf
            v[3 * blk + 4] = fi.tiny * 8 if f16 else 1e-36
        if nblk > 4:
            v[4 * blk: 5 * blk] = 0.0  # tiny block with a NaN in it
            v[4 * blk + 1] = -tiny_sub * 5
            v[4 * blk + blk - 1] = math.nan
        t = torch.from_numpy(v).to(dtype)
        if tot > 5:  # NaN of both signs, set by their bits (a cast picks its own)
            view = torch.int16 if t.element_size() == 2 else torch.int32
            quiet = {torch.float32: 0x7FC00000, torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}[dtype]
            bits = t.view(view)
            bits[4] = quiet
            bits[5] = quiet - (0x8000 if t.element_size() == 2 else 0x80000000)
        return t[:n].contiguous()
    elif kind == "randn":
        v = rng.standard_normal(tot) * 3.0
    else:
        raise ValueError(kind)
    with np.errstate(over="ignore"):
        return torch.from_numpy(np.ascontiguousarray(v[:n])).to(dtype).contiguous()


def hadamard_safe(t: torch.Tensor) -> torch.Tensor:
    """Zero the finite values of 2^121 and above, so that every row of 32 sums
    to less than 2^126 and no finite input overflows the rotation's float32
    sums (the non-finite values stay)."""
    x = t.double()
    drop = torch.isfinite(x) & (x.abs() >= 2.0 ** 121)
    return torch.where(drop, torch.zeros_like(t), t).contiguous()
