"""Integer oracle of the float conversions ``hs_copy_nd`` performs when a
snapshot is restored into tensors of another float type (f16, bf16, f32, f64),
independent of ``hipsnapshot.ops``, of ``fp8_oracle.py``, of NumPy's ``astype``
and of every torch cast.  Imported by ``test_cast_oracle.py`` (CPU) and
``test_gpu_cast_oracle.py`` (GPU) the way ``dist_workers`` is.

``convert`` works on raw bit patterns in NumPy integer arithmetic only: split
sign, exponent and mantissa, renormalise a subnormal source, shift to the
target's mantissa width with round-to-nearest-even and let the carry run into
the exponent.  Overflow gives +-inf, gradual underflow ends at +-0, the sign of
zero is kept and a widening is exact, subnormal sources included.  A format is a
name of ``FORMATS`` or an ``(exponent bits, mantissa bits)`` pair.

``expected_bits`` is the contract of the copy kernel as its comments state it:
one RNE rounding, except that f64 -> f16 and f64 -> bf16 round to f32 first and
then again (what a ``c10::Half`` / ``c10::BFloat16`` built from a ``float``
does).

NaN policy: a NaN source must give a NaN result, never +-inf and never a finite
value.  Sign and payload of that NaN are compared neither with this oracle nor
with torch: torch's own CPU and device paths canonicalise differently, and the
kernel's ``f32_to_bf16`` keeps the sign.  ``convert`` therefore returns an
``is_nan`` mask next to the bits, and ``check_cast`` compares bits only where
it is clear.

The value sets (``source_set``) hold source bit patterns: all 65 536 patterns
of a 16-bit source; for a narrowing to f16 / bf16 every non-negative finite
target value with the midpoint to its successor and that midpoint -+1 source
ulp, both signs (every tie, every subnormal target, the round-to-zero and the
overflow boundary); for f64 -> f16 / bf16 also the edges of every interval of
doubles that rounds to an f32 equal to such a midpoint, where one rounding and
two roundings part; for f64 -> f32 and the widenings every exponent times a
fixed list of mantissas; and a list of specials."""

from __future__ import annotations

import functools

import numpy as np
import torch

FORMATS = {"f16": (5, 10), "bf16": (8, 7), "f32": (8, 23), "f64": (11, 52)}
PAIRS = [(s, d) for s in FORMATS for d in FORMATS if s != d]

NP_UINT = {"f16": np.uint16, "bf16": np.uint16, "f32": np.uint32, "f64": np.uint64}
NP_FLOAT = {"f16": np.float16, "f32": np.float32, "f64": np.float64}  # NumPy has no bf16
TORCH_FLOAT = {"f16": torch.float16, "bf16": torch.bfloat16, "f32": torch.float32,
               "f64": torch.float64}
TORCH_INT = {"f16": torch.int16, "bf16": torch.int16, "f32": torch.int32, "f64": torch.int64}

_ONE = np.uint64(1)


def _fmt(f):
    return FORMATS[f] if isinstance(f, str) else f


def _u(x) -> np.uint64:
    return np.uint64(x)


def _bit_length(x: np.ndarray) -> np.ndarray:
    """Position of the highest set bit plus one (0 for 0), by binary search."""
    x = x.copy()
    n = np.zeros(x.shape, dtype=np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        big = (x >> _u(s)) != 0
        n += np.where(big, s, 0)
        x = np.where(big, x >> _u(s), x)
    return n + (x != 0)


def convert(bits, src, dst, rounding: str = "rne"):
    """``bits`` of format ``src`` as format ``dst``: ``(bits, is_nan)``, both
    of the input's shape, the bits as uint64.  NaNs come out as the positive
    quiet NaN with the sign of the source; compare them through ``is_nan``.

    ``rounding`` is "rne"; "trunc" and "away" (ties away from zero) exist for
    the mutants of ``test_cast_oracle.py`` only."""
    (se, sm), (de, dm) = _fmt(src), _fmt(dst)
    b = np.asarray(bits).astype(np.uint64)
    s_max, d_max = (1 << se) - 1, (1 << de) - 1
    s_bias, d_bias = (1 << (se - 1)) - 1, (1 << (de - 1)) - 1
    sign = (b >> _u(se + sm)) & _ONE
    exp = ((b >> _u(sm)) & _u(s_max)).astype(np.int64)
    man = b & _u((1 << sm) - 1)
    is_nan = (exp == s_max) & (man != 0)
    is_inf = (exp == s_max) & (man == 0)
    is_zero = (exp == 0) & (man == 0)

    # significand with its leading bit at position sm, and that bit's exponent
    sub = exp == 0
    lshift = np.where(sub, sm + 1 - _bit_length(man), 0)
    sig = np.where(sub, man << lshift.astype(np.uint64), man | (_ONE << _u(sm)))
    e = np.where(sub, 1 - lshift, exp) - s_bias

    # biased target exponent; below 1 the result is subnormal and loses
    # 1 - t more bits.  Past sm + 2 bits every value rounds to zero.
    t = np.minimum(e + d_bias, d_max + 1)
    shift = np.minimum((sm - dm) + np.where(t < 1, 1 - t, 0), sm + 2)
    rs = np.maximum(shift, 0).astype(np.uint64)
    ls = np.maximum(-shift, 0).astype(np.uint64)
    q = (sig >> rs) << ls
    rem = sig & ((_ONE << rs) - _ONE)
    half = (_ONE << rs) >> _ONE  # 0 when nothing is shifted out
    if rounding == "rne":
        up = (rem > half) | ((rem == half) & (rs > 0) & ((q & _ONE) == 1))
    elif rounding == "away":
        up = (rem >= half) & (rs > 0)
    elif rounding == "trunc":
        up = np.zeros(q.shape, dtype=bool)
    else:
        raise ValueError(rounding)
    q = q + up.astype(np.uint64)

    # q carries the implicit bit of a normal result: adding it to exponent
    # t - 1 gives exponent t, and a mantissa that rounded up to 2^(dm+1), or a
    # subnormal that rounded up to 2^dm, carries into the exponent by itself
    inf_bits = _u(d_max << dm)
    out = (np.maximum(t - 1, 0).astype(np.uint64) << _u(dm)) + q
    out = np.where(out >= inf_bits, inf_bits, out)
    out = np.where(is_zero, _u(0), out)
    out = np.where(is_inf, inf_bits, out)
    out = np.where(is_nan, inf_bits | _u(1 << (dm - 1)), out)
    return out | (sign << _u(de + dm)), is_nan


def expected_bits(src_bits, src: str, dst: str, rounding: str = "rne"):
    """What the copy kernel must store for ``src_bits``: ``(bits, is_nan)``."""
    if src == "f64" and dst in ("f16", "bf16"):
        mid, is_nan = convert(src_bits, "f64", "f32", rounding)
        return convert(mid, "f32", dst, rounding)[0], is_nan
    return convert(src_bits, src, dst, rounding)


def nan_mask(bits, fmt) -> np.ndarray:
    e, m = _fmt(fmt)
    b = np.asarray(bits).astype(np.uint64)
    return (((b >> _u(m)) & _u((1 << e) - 1)) == _u((1 << e) - 1)) & ((b & _u((1 << m) - 1)) != 0)


def check_cast(src_bits, got_bits, want_bits, is_nan, src: str, dst: str, what: str) -> None:
    """``got_bits`` equal ``want_bits`` wherever ``is_nan`` is clear and are a
    NaN of ``dst`` wherever it is set; otherwise an ``AssertionError`` that
    names the first failing input."""
    src_bits, got = np.asarray(src_bits).ravel(), np.asarray(got_bits).astype(np.uint64).ravel()
    want, is_nan = np.asarray(want_bits).ravel(), np.asarray(is_nan).ravel()
    assert src_bits.shape == got.shape == want.shape == is_nan.shape, what
    bad = ~is_nan & (got != want)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(
            f"{what}: {src} {int(src_bits[i]):#x} (element {i}) gave {dst} {int(got[i]):#x}, "
            f"expected {int(want[i]):#x}; {int(bad.sum())} of {bad.size} elements differ")
    bad = is_nan & ~nan_mask(got, dst)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(
            f"{what}: NaN {src} {int(src_bits[i]):#x} (element {i}) gave {dst} {int(got[i]):#x}, "
            f"which is no NaN; {int(bad.sum())} of {int(is_nan.sum())} NaNs lost")


# ---------------------------------------------------------------------------
# bit patterns <-> tensors, without a cast
# ---------------------------------------------------------------------------

def to_tensor(bits, fmt: str) -> torch.Tensor:
    """CPU tensor of ``fmt`` holding exactly ``bits``."""
    raw = np.ascontiguousarray(np.asarray(bits).astype(NP_UINT[fmt]))
    return torch.from_numpy(raw.view(raw.dtype.name[1:])).view(TORCH_FLOAT[fmt])


def bits_of(t: torch.Tensor) -> np.ndarray:
    """The bit patterns of a float tensor (any device, any strides), uint64."""
    ints = {2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]
    a = t.detach().contiguous().view(ints).cpu().numpy()
    return a.view("u" + a.dtype.name).astype(np.uint64)


# ---------------------------------------------------------------------------
# value sets
# ---------------------------------------------------------------------------

def _both_signs(mag: np.ndarray, fmt) -> np.ndarray:
    e, m = _fmt(fmt)
    return np.concatenate([mag, mag | _u(1 << (e + m))])


def _mantissas(m: int) -> np.ndarray:
    rng = np.random.default_rng(0x5EED + m)
    fixed = [0, 1, 2, 1 << (m - 1), (1 << m) - 2, (1 << m) - 1]
    return np.concatenate([np.array(fixed, dtype=np.uint64),
                           rng.integers(0, 1 << m, 26, dtype=np.uint64)])


def exponent_sweep(fmt, with_top: bool = True) -> np.ndarray:
    """Every exponent field (the subnormal one, and with ``with_top`` the
    inf / NaN one) times 32 mantissas; non-negative patterns."""
    e, m = _fmt(fmt)
    exps = np.arange((1 << e) - (0 if with_top else 1), dtype=np.uint64)
    return ((exps << _u(m))[:, None] | _mantissas(m)[None, :]).ravel()


def subnormal_ladder(fmt) -> np.ndarray:
    """Subnormals with their leading bit at every position: 2^k, 2^k + 1 and
    2^(k+1) - 1 in units of the smallest one."""
    _, m = _fmt(fmt)
    k = np.arange(m, dtype=np.uint64)
    return np.unique(np.concatenate([_ONE << k, (_ONE << k) + _ONE, (_ONE << (k + _ONE)) - _ONE]))


def finite_targets(fmt) -> np.ndarray:
    """Every non-negative finite pattern of a 16-bit format."""
    e, m = _fmt(fmt)
    return np.arange(((1 << e) - 1) << m, dtype=np.uint64)


def neighbourhoods(targets: np.ndarray, dst, src) -> np.ndarray:
    """For each non-negative finite ``dst`` pattern t, in format ``src``: t,
    the midpoint between t and its successor, and that midpoint -+1 ulp.  The
    midpoint of t and t + 1 is the pattern 2t + 1 of the format with one more
    mantissa bit, which widens exactly.  Behind the largest finite t come the
    midpoint to its would-be successor and, where ``src`` can hold it, that
    successor (the overflow boundary)."""
    de, dm = _fmt(dst)
    t = convert(targets, dst, src)[0]
    mid = convert(targets * _u(2) + _ONE, (de, dm + 1), src)[0]
    assert np.all(mid > t) and np.all(mid[:-1] < t[1:])  # strictly between, and positive
    return np.concatenate([t, mid, mid - _ONE, mid + _ONE, 2 * mid[-1:] - t[-1:]])


def double_rounding_traps(dst) -> np.ndarray:
    """f64 patterns around the edges of every interval of doubles that rounds
    to an f32 which is itself a midpoint M of two ``dst`` values: the f32
    ties M -+ half an f32 ulp, each -+1 f64 ulp.  Inside the interval the
    first rounding lands on M and the second breaks the tie to even, where a
    single rounding follows the side of M the double lies on."""
    de, dm = _fmt(dst)
    m32 = convert(finite_targets(dst) * _u(2) + _ONE, (de, dm + 1), "f32")[0]
    lo = convert(m32 * _u(2) - _ONE, (8, 24), "f64")[0]
    hi = convert(m32 * _u(2) + _ONE, (8, 24), "f64")[0]
    return np.concatenate([lo - _ONE, lo, lo + _ONE, hi - _ONE, hi, hi + _ONE])


SPECIALS = {
    # +-0, +-inf, +-max finite, +-min / max subnormal, +-min normal, +-1, quiet and
    # signalling NaNs of both signs, and NaNs whose payload lies only in the
    # bits a narrowing drops (a truncating conversion makes inf from these)
    "f32": [0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7f7fffff, 0xff7fffff,
            0x00000001, 0x80000001, 0x007fffff, 0x807fffff, 0x00800000, 0x80800000,
            0x3f800000, 0xbf800000,
            0x7fc00000, 0xffc00000, 0x7fa00000, 0xffa00000, 0x7fffffff, 0xffffffff,
            0x7f800001, 0xff80ffff, 0x7f801000],
    "f64": [0x0000000000000000, 0x8000000000000000, 0x7ff0000000000000, 0xfff0000000000000,
            0x7fefffffffffffff, 0xffefffffffffffff, 0x0000000000000001, 0x8000000000000001,
            0x000fffffffffffff, 0x800fffffffffffff, 0x0010000000000000, 0x8010000000000000,
            0x3ff0000000000000, 0xbff0000000000000,
            0x7ff8000000000000, 0xfff8000000000000, 0x7ff4000000000000, 0xfff4000000000000,
            0x7fffffffffffffff, 0xffffffffffffffff,
            0x7ff0000000000001, 0xfff000001fffffff],
}


def specials(fmt: str) -> np.ndarray:
    return np.array(SPECIALS[fmt], dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def source_set(src: str, dst: str) -> np.ndarray:
    """The source bit patterns (uint64, read-only) a ``src`` -> ``dst`` cast is
    tested on."""
    if src in ("f16", "bf16"):
        out = np.arange(1 << 16, dtype=np.uint64)
    else:
        mags = [exponent_sweep(src), subnormal_ladder(src)]
        if dst in ("f16", "bf16"):
            mags.append(neighbourhoods(finite_targets(dst), dst, src))
            if src == "f64":
                mags.append(double_rounding_traps(dst))
        elif (src, dst) == ("f64", "f32"):
            targets = np.concatenate([exponent_sweep("f32", with_top=False),
                                      subnormal_ladder("f32")])
            mags.append(neighbourhoods(np.unique(targets), "f32", "f64"))
        out = np.concatenate([_both_signs(np.concatenate(mags), src), specials(src)])
    out.setflags(write=False)
    return out
