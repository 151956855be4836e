"""Proves ``cast_oracle.py`` on the CPU: its single roundings against NumPy's
``astype``, the kernel's contract (``expected_bits``) against torch's CPU
``.to()``, and its power to tell a wrong converter from a right one: eight
kinds of mutant go through the comparison the GPU test uses
(``check_cast``), and each must fail on exactly the pairs where it can."""

import functools

import numpy as np
import pytest
import torch

import cast_oracle as C

NARROWING = {("f32", "f16"), ("f32", "bf16"), ("f64", "f16"), ("f64", "bf16"), ("f64", "f32"),
             ("f16", "bf16"), ("bf16", "f16")}
WIDENING = [p for p in C.PAIRS if p not in NARROWING]
NUMPY_PAIRS = [(s, d) for s, d in C.PAIRS if s in C.NP_FLOAT and d in C.NP_FLOAT]


def _ids(pairs):
    return ["->".join(p) for p in pairs]


@functools.lru_cache(maxsize=None)
def _expected(src, dst):
    return C.expected_bits(C.source_set(src, dst), src, dst)


def _first(mask):
    return int(np.flatnonzero(mask)[0])


# -- anchors that need no other implementation -----------------------------------

@pytest.mark.parametrize("src,dst,bits,want", [
    ("f32", "f16", 0x3f800000, 0x3c00),   # 1.0
    ("f32", "f16", 0x477ff000, 0x7c00),   # 65520, the overflow tie: even is inf
    ("f32", "f16", 0x477fefff, 0x7bff),   # just below it: 65504
    ("f32", "f16", 0x33800000, 0x0001),   # 2^-24, the smallest subnormal
    ("f32", "f16", 0x33000000, 0x0000),   # 2^-25, a tie with zero: even is zero
    ("f32", "f16", 0xb3000001, 0x8001),   # just past it, negative
    ("f32", "f16", 0xb3000000, 0x8000),   # -2^-25 keeps its sign
    ("f32", "f16", 0x387fe000, 0x0400),   # largest subnormal tie carries into the exponent
    ("f32", "bf16", 0x3f808000, 0x3f80),  # tie, even below
    ("f32", "bf16", 0x3f818000, 0x3f82),  # tie, even above
    ("f32", "bf16", 0x7f7f8000, 0x7f80),  # overflow tie
    ("f32", "bf16", 0x7f7f7fff, 0x7f7f),  # largest value that stays finite
    ("f16", "f32", 0x0001, 0x33800000),   # subnormal source widens exactly
    ("f16", "f64", 0x83ff, 0xbf0ff80000000000),
    ("bf16", "f32", 0x0001, 0x00010000),  # subnormal to subnormal
    ("f64", "f32", 0x36a0000000000000, 0x00000001),  # 2^-149
    ("f64", "f32", 0x3690000000000000, 0x00000000),  # 2^-150: tie with zero
    ("f64", "f32", 0x47efffffe0000000, 0x7f7fffff),  # max float
    ("f64", "f32", 0x47effffff0000000, 0x7f800000),  # the overflow tie
])
def test_known_conversions(src, dst, bits, want):
    got, is_nan = C.convert(np.array([bits], dtype=np.uint64), src, dst)
    assert not is_nan[0] and int(got[0]) == want, f"{int(got[0]):#x}"


def test_double_rounding_differs_where_the_contract_says():
    """1 + 2^-11 + 2^-40: above the f16 tie, so one rounding goes up to
    0x3c01; through f32 it first becomes the tie and then goes to even."""
    x = np.array([0x3ff0020000001000], dtype=np.uint64)
    assert int(C.convert(x, "f64", "f16")[0][0]) == 0x3c01
    assert int(C.expected_bits(x, "f64", "f16")[0][0]) == 0x3c00


@pytest.mark.parametrize("narrow,wide", WIDENING, ids=_ids(WIDENING))
def test_widening_is_exact(narrow, wide):
    """Narrowing a widened value gives the value back, subnormals included."""
    src = C.source_set(narrow, wide)
    up, is_nan = C.convert(src, narrow, wide)
    back, _ = C.convert(up, wide, narrow)
    bad = ~is_nan & (back != src)
    assert not bad.any(), f"{narrow} {int(src[_first(bad)]):#x} does not survive {wide}"


# -- against NumPy and torch -----------------------------------------------------

@pytest.mark.parametrize("src,dst", NUMPY_PAIRS, ids=_ids(NUMPY_PAIRS))
def test_single_rounding_matches_numpy(src, dst):
    bits = C.source_set(src, dst)
    got, is_nan = C.convert(bits, src, dst)
    with np.errstate(all="ignore"):
        ref = bits.astype(C.NP_UINT[src]).view(C.NP_FLOAT[src]).astype(C.NP_FLOAT[dst])
    ref_bits = ref.view(C.NP_UINT[dst]).astype(np.uint64)
    assert np.array_equal(is_nan, np.isnan(ref)), "NaN sources and NumPy's NaN results differ"
    C.check_cast(bits, ref_bits, got, is_nan, src, dst, f"numpy astype {src}->{dst}")


@pytest.mark.parametrize("src,dst", C.PAIRS, ids=_ids(C.PAIRS))
def test_contract_matches_torch_cpu(src, dst):
    bits = C.source_set(src, dst)
    want, is_nan = _expected(src, dst)
    ref = C.to_tensor(bits, src).to(C.TORCH_FLOAT[dst])
    assert np.array_equal(is_nan, ref.isnan().numpy()), "NaN sources and torch's NaN results differ"
    C.check_cast(bits, C.bits_of(ref), want, is_nan, src, dst, f"torch cpu {src}->{dst}")


def test_tensor_helpers_keep_every_bit():
    for fmt in C.FORMATS:
        bits = C.source_set(fmt, "f64" if fmt != "f64" else "f32")
        assert np.array_equal(C.bits_of(C.to_tensor(bits, fmt)), bits), fmt


# -- the sets ----------------------------------------------------------------------

def test_sets_hold_what_they_promise():
    for src, dst in C.PAIRS:
        bits = C.source_set(src, dst)
        if src in ("f16", "bf16"):
            assert bits.size == 1 << 16
            continue
        have = set(C.SPECIALS[src])
        assert have <= set(bits.tolist()), (src, dst)
        want, is_nan = _expected(src, dst)
        de, dm = C.FORMATS[dst]
        mag = want[~is_nan] & np.uint64((1 << (de + dm)) - 1)
        if dst in ("f16", "bf16"):
            # every target magnitude, inf included, is some element's result
            assert np.array_equal(np.unique(mag), np.arange((((1 << de) - 1) << dm) + 1)), (src, dst)
        elif dst == "f32":
            # every exponent field of the target is
            assert np.array_equal(np.unique(mag >> np.uint64(dm)), np.arange(1 << de)), (src, dst)
        assert is_nan.sum() >= 9, (src, dst)


@pytest.mark.parametrize("dst", ["f16", "bf16"])
def test_double_rounding_traps_discriminate(dst):
    """The f64 set keeps inputs on which one rounding and two roundings
    disagree: a set without them could not see the two ``fptrunc``s of
    ``store_from_f64`` folded into one."""
    bits = C.source_set("f64", dst)
    want, is_nan = _expected("f64", dst)
    single, _ = C.convert(bits, "f64", dst)
    differ = ~is_nan & (single != want)
    print(f"f64->{dst}: {int(differ.sum())} of {bits.size} inputs are double-rounding traps")
    assert differ.sum() > 0
    # at least one for every target midpoint, on either side of zero
    assert differ.sum() >= 2 * C.finite_targets(dst).size


# -- mutants -------------------------------------------------------------------------

def _exp_field(bits, fmt):
    e, m = C.FORMATS[fmt]
    return (bits >> np.uint64(m)) & np.uint64((1 << e) - 1)


def _sign_only(bits, fmt):
    e, m = C.FORMATS[fmt]
    return bits & np.uint64(1 << (e + m))


def _truncation(bits, src, dst):
    return C.expected_bits(bits, src, dst, rounding="trunc")[0]


def _half_away(bits, src, dst):
    return C.expected_bits(bits, src, dst, rounding="away")[0]


def _flush_subnormal_results(bits, src, dst):
    out = C.expected_bits(bits, src, dst)[0]
    return np.where(_exp_field(out, dst) == 0, _sign_only(out, dst), out)


def _flush_subnormal_sources(bits, src, dst):
    flushed = np.where(_exp_field(bits, src) == 0, _sign_only(bits, src), bits)
    return C.expected_bits(flushed, src, dst)[0]


def _saturate(bits, src, dst):
    out = C.expected_bits(bits, src, dst)[0]
    e, m = C.FORMATS[dst]
    se, sm = C.FORMATS[src]
    mag = np.uint64((1 << (e + m)) - 1)
    src_inf = (bits & np.uint64((1 << (se + sm)) - 1)) == np.uint64(((1 << se) - 1) << sm)
    overflowed = ((out & mag) == np.uint64(((1 << e) - 1) << m)) & ~src_inf
    return np.where(overflowed, out - np.uint64(1), out)


def _nan_payload_truncated(bits, src, dst):
    """The mantissa of a NaN cut to the target's width without setting a quiet
    bit: a payload in the dropped bits leaves inf."""
    out, is_nan = C.expected_bits(bits, src, dst)
    (se, sm), (de, dm) = C.FORMATS[src], C.FORMATS[dst]
    man = bits & np.uint64((1 << sm) - 1)
    man = man >> np.uint64(sm - dm) if sm > dm else man << np.uint64(dm - sm)
    nan = ((bits >> np.uint64(se + sm)) << np.uint64(de + dm)) | np.uint64(((1 << de) - 1) << dm) | man
    return np.where(is_nan, nan, out)


def _single_rounding(bits, src, dst):
    return C.convert(bits, src, dst)[0]


def _zero_sign_lost(bits, src, dst):
    out = C.expected_bits(bits, src, dst)[0]
    return np.where(out == _sign_only(out, dst), np.uint64(0), out)


_FROM_F16 = {("f16", d) for d in ("bf16", "f32", "f64")}
MUTANTS = {
    # mutant -> (converter, the pairs on which it computes something wrong)
    "truncation": (_truncation, NARROWING),
    "round_half_away": (_half_away, NARROWING),
    # no f16 is small enough for a subnormal bf16; bf16 subnormals widen to f32 subnormals
    "flush_subnormal_results": (_flush_subnormal_results,
                                NARROWING - {("f16", "bf16")} | {("bf16", "f32")}),
    # the other sources' subnormals are zero in the target anyway
    "flush_subnormal_sources": (_flush_subnormal_sources,
                                _FROM_F16 | {("bf16", "f32"), ("bf16", "f64"), ("f32", "f64"),
                                             ("f32", "bf16")}),
    "saturate_instead_of_inf": (_saturate, NARROWING - {("f16", "bf16")}),
    "nan_payload_truncated": (_nan_payload_truncated, NARROWING - {("bf16", "f16")}),
    "single_rounded_f64": (_single_rounding, {("f64", "f16"), ("f64", "bf16")}),
    "zero_sign_lost": (_zero_sign_lost, set(C.PAIRS)),
}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_mutant_is_rejected(name):
    mutant, wrong_on = MUTANTS[name]
    rejected = set()
    for src, dst in C.PAIRS:
        bits = C.source_set(src, dst)
        want, is_nan = _expected(src, dst)
        try:
            C.check_cast(bits, mutant(bits, src, dst), want, is_nan, src, dst, name)
        except AssertionError as e:
            print(e)
            assert "0x" in str(e)  # names the input bits
            rejected.add((src, dst))
    assert rejected, f"{name} passed on every set"
    assert rejected == wrong_on, (sorted(rejected - wrong_on), sorted(wrong_on - rejected))
