"""The float64 oracle of the fp8 formats (``fp8_oracle.py``) proved on the CPU:
every ``*_reference`` of ``ops/quant.py`` passes it on the whole input set, it
rejects each of a list of mutants, and a CPU snapshot of tiny second moments
restores zeros as zeros (the tiny-block bug: a subnormal block scale whose
reciprocal is inf)."""

import numpy as np
import pytest
import torch

import fp8_oracle as O
from hipsnapshot import Snapshot, StateDict
from hipsnapshot.ops import quant as Q
from hipsnapshot.utils.test_utils import env

SRC_DTYPES = [torch.float32, torch.bfloat16, torch.float16]
DST_DTYPES = [torch.bfloat16, torch.float16, torch.float32, torch.float64]
SIZES = [1, 31, 32, 33, 127, 128, 129, 1023, 1024, 1025, 1024 + 5, 2048 + 5, 2049, 8192 + 17,
         65536 + 77]
MESSAGE = r"(?s)(element.*block|block.*element).*bound"


def _u8(q: torch.Tensor) -> np.ndarray:
    return q.view(torch.uint8).numpy()


def _mx_payload(q: torch.Tensor) -> np.ndarray:
    n = q.numel()
    out = np.zeros((n + 15) // 16 * 16, dtype=np.uint8)
    out[:n] = _u8(q)
    return out


# ---------------------------------------------------------------------------
# the tables
# ---------------------------------------------------------------------------

def test_e4m3_table_and_rne_encoder():
    t = O.E4M3
    assert t[0x7E] == 448.0 and t[0xFE] == -448.0 and t[0x38] == 1.0
    assert t[0x01] == 2.0 ** -9 and t[0x07] == 7 * 2.0 ** -9 and t[0x08] == 2.0 ** -6
    assert np.isnan(t[0x7F]) and np.isnan(t[0xFF]) and not np.isinf(t).any()
    assert (np.diff(t[:0x7F]) > 0).all()
    finite = np.array([b for b in range(256) if b & 0x7F != 0x7F], dtype=np.uint8)
    assert (O.encode_e4m3_rne(t[finite]) == finite).all()  # -0 keeps its sign
    grid = t[:0x7F]
    mids = (grid[:-1] + grid[1:]) / 2
    lo = np.arange(0x7E)
    even = np.where(lo % 2 == 0, lo, lo + 1)
    assert (O.encode_e4m3_rne(mids) == even).all()  # ties to even
    assert (O.encode_e4m3_rne(-mids) == (even | 0x80)).all()
    assert (O.encode_e4m3_rne(np.nextafter(mids, 0.0)) == lo).all()
    assert (O.encode_e4m3_rne(np.nextafter(mids, 1e9)) == lo + 1).all()
    assert O.HALF_GAP[0] == 2.0 ** -10 and O.HALF_GAP[0x08] == 2.0 ** -10
    assert O.HALF_GAP[0x38] == 2.0 ** -4 and O.HALF_GAP[0x39] == 2.0 ** -4  # 1.0: gaps 1/16, 1/8
    assert O.HALF_GAP[0x7E] == 16.0


def test_bf16_rounding_is_rne():
    f = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20,
                  3.3895314e38, -2.0 ** -133, 2.0 ** -134, 3 * 2.0 ** -134], dtype=np.float32)
    want = torch.from_numpy(f).to(torch.bfloat16).view(torch.int16).numpy()
    assert (O.round_dst_bits(f, torch.bfloat16) == want).all()


# ---------------------------------------------------------------------------
# the references pass
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kind", O.VALUE_SETS)
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_mx_reference_passes_oracle(dtype, kind):
    for n in SIZES:
        x = O.build_values(kind, n, dtype, O.MX_BLOCK)
        x64, neg = O.source_arrays(x)
        q, s = Q.mx_quantize_reference(x)
        O.check_mx_quant(x64, neg, _mx_payload(q), s.numpy())
        for dst in DST_DTYPES:
            out = Q.mx_dequantize_reference(q, s, dst)
            O.check_mx_dequant(_u8(q), s.numpy(), O.bits_of(out), dst)


@pytest.mark.parametrize("kind", O.VALUE_SETS)
@pytest.mark.parametrize("vpt", [2, 4, 8, 16])
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_block_reference_passes_oracle(dtype, vpt, kind):
    block = 64 * vpt
    for n in SIZES:
        x = O.build_values(kind, n, dtype, block)
        x64, neg = O.source_arrays(x)
        q, s = Q.quantize_reference(x, block)
        O.check_block_quant(x64, neg, _u8(q), s.numpy(), block)
        for dst in DST_DTYPES:
            out = Q.dequantize_reference(q, s, block, dst)
            O.check_block_dequant(_u8(q), s.numpy(), block, O.bits_of(out), dst)


@pytest.mark.parametrize("kind", O.VALUE_SETS)
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_hadamard_reference_passes_oracle(dtype, kind):
    for n in SIZES:
        x = O.hadamard_safe(O.build_values(kind, n, dtype, O.HAD_BLOCK))
        x64, _ = O.source_arrays(x)
        q, s = Q.hadamard_quantize_reference(x, O.HAD_BLOCK)
        O.check_hadamard_quant(x64, _u8(q), s.numpy())
        for dst in DST_DTYPES:
            out = Q.hadamard_dequantize_reference(q, s, n, dst, O.HAD_BLOCK)
            O.check_hadamard_dequant(_u8(q), s.numpy(), O.bits_of(out), dst)


def test_value_sets_reach_the_edges():
    """The sweep holds whole blocks below 1.3e-36 with zeros inside, the ties
    set holds exact MX ties, the special set every special value."""
    for dtype in (torch.float32, torch.bfloat16):
        x = O.build_values("sweep", 2049, dtype, 128).double().view(-1)[:2048].view(-1, 128)
        amax = x.abs().amax(dim=1)
        tiny = (amax > 0) & (amax < 1.3e-36)
        assert tiny.sum() >= 4 and bool((x[tiny] == 0).any(dim=1).all())
        assert bool((amax / 448 >= 2.0 ** -126).any())
    for dtype in SRC_DTYPES:
        x = O.build_values("ties", 1024, dtype, 32).double().numpy().reshape(-1, 32)
        k = np.array([O.mx_exponent(a) for a in np.abs(x).max(axis=1)])
        v = np.abs(np.ldexp(x, -k[:, None]))
        grid = O.E4M3[:0x7F]
        mids = (grid[:-1] + grid[1:]) / 2
        assert np.isin(v, mids).sum() >= 300
        s = O.build_values("special", 1024, dtype, 128)
        assert s.isinf().sum() >= 3 and s.isnan().sum() >= 3
        bits = O.bits_of(s)
        assert (bits[s.isnan().numpy()] < 0).any() and (bits[s.isnan().numpy()] > 0).any()
        assert bool((s.view(-1, 128)[1] == 0).all())


# ---------------------------------------------------------------------------
# the oracle rejects mutants
# ---------------------------------------------------------------------------

def _encode_with(v, neg, rnd):
    """The oracle's encoder with another rounding of the scaled mantissa."""
    a = np.abs(v)
    sub = rnd(a * 2.0 ** 9)
    m, e = np.frexp(a)
    r = rnd(m * 16.0)
    carry = r == 16.0
    r = np.where(carry, 8.0, r)
    norm = (e + carry + 6) * 8 + (r.astype(np.int64) - 8)
    code = np.where(a < 2.0 ** -6, sub.astype(np.int64), norm)
    return (code | np.where(neg, 0x80, 0)).astype(np.uint8)


def _mx_case(kind, n=1024, dtype=torch.float32):
    x = O.build_values(kind, n, dtype, O.MX_BLOCK)
    x64, neg = O.source_arrays(x)
    q, s = Q.mx_quantize_reference(x)
    codes, scales = _mx_payload(q).copy(), s.numpy().copy()
    O.check_mx_quant(x64, neg, codes, scales)
    return x64, neg, codes, scales


def _mx_scaled(x64, scales):
    k = np.repeat(scales.astype(np.int64) - 127, 32)[: x64.size]
    return np.ldexp(x64, -k)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_mutant_truncation(dtype):
    x64, neg, codes, scales = _mx_case("randn", dtype=dtype)
    trunc = _encode_with(_mx_scaled(x64, scales), neg, np.floor)
    assert (trunc != codes).any()
    with pytest.raises(AssertionError, match=MESSAGE):
        O.check_mx_quant(x64, neg, trunc, scales)
    x = O.build_values("randn", 1024, dtype, 128)
    x64, neg = O.source_arrays(x)
    q, s = Q.quantize_reference(x, 128)
    sc = np.repeat(s.numpy().astype(np.float64), 128)
    trunc = _encode_with(np.clip(x64 / sc, -448, 448), neg, np.floor)
    with pytest.raises(AssertionError, match=MESSAGE):
        O.check_block_quant(x64, neg, trunc, s.numpy(), 128)


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_mutant_ties_away_from_even(dtype):
    x64, neg, codes, scales = _mx_case("ties", dtype=dtype)
    away = _encode_with(_mx_scaled(x64, scales), neg, lambda t: np.floor(t + 0.5))
    diff = away != codes
    assert 0 < diff.sum() < codes.size // 4  # only the real ties move
    with pytest.raises(AssertionError, match=MESSAGE):
        O.check_mx_quant(x64, neg, away, scales)


def test_mutant_one_grid_step():
    """One code one grid step past the value it rounds: MX, blockwise, Hadamard."""
    x64, neg, codes, scales = _mx_case("randn")
    v = np.abs(_mx_scaled(x64, scales))
    inner = (codes & 7 >= 2) & (codes & 7 <= 5) & (codes & 0x78 != 0)  # no binade edge next to it
    i = int(np.flatnonzero(inner)[7])
    step = -1 if v[i] >= abs(O.E4M3[codes[i]]) else 1
    bad = codes.copy()
    bad[i] = int(codes[i]) + step
    with pytest.raises(AssertionError, match=rf"element {i} \(block {i // 32}"):
        O.check_mx_quant(x64, neg, bad, scales)

    x = O.build_values("randn", 1024, torch.float32, 128)
    x64, neg = O.source_arrays(x)
    q, s = Q.quantize_reference(x, 128)
    codes = _u8(q).copy()
    v = np.abs(x64 / np.repeat(s.numpy().astype(np.float64), 128))
    inner = (codes & 7 >= 2) & (codes & 7 <= 5) & (codes & 0x78 != 0)
    i = int(np.flatnonzero(inner)[11])
    codes[i] = int(codes[i]) + (-1 if v[i] >= abs(O.E4M3[codes[i]]) else 1)
    with pytest.raises(AssertionError, match=rf"element {i} \(block {i // 128}\).*bound"):
        O.check_block_quant(x64, neg, codes, s.numpy(), 128)

    q, s = Q.hadamard_quantize_reference(x, 128)
    codes = _u8(q).copy()
    y = (x64.reshape(-1, 32) @ O.hadamard64()).reshape(-1)
    v = np.abs(y / np.repeat(s.numpy().astype(np.float64), 128))
    inner = (codes & 7 >= 2) & (codes & 7 <= 5) & (codes & 0x78 != 0)
    i = int(np.flatnonzero(inner)[13])
    codes[i] = int(codes[i]) + (-1 if v[i] >= abs(O.E4M3[codes[i]]) else 1)
    with pytest.raises(AssertionError, match=rf"element {i} \(block {i // 128}\).*bound"):
        O.check_hadamard_quant(x64, codes, s.numpy())


def test_mutant_neighbouring_block_scale():
    x64, neg, codes, scales = _mx_case("sweep")
    bad = scales.copy()
    bad[3] = scales[4]
    assert bad[3] != scales[3]
    with pytest.raises(AssertionError, match=r"(?s)block 3 \(elements 96.*bound"):
        O.check_mx_quant(x64, neg, codes, bad)

    x = O.build_values("sweep", 2049, torch.float32, 128)
    x64, neg = O.source_arrays(x)
    q, s = Q.quantize_reference(x, 128)
    bad = s.numpy().copy()
    bad[5] = bad[6]
    with pytest.raises(AssertionError, match=r"(?s)block 5 \(elements 640.*bound"):
        O.check_block_quant(x64, neg, _u8(q), bad, 128)

    q, s = Q.hadamard_quantize_reference(x, 128)
    bad = s.numpy().copy()
    bad[5] = bad[6]
    with pytest.raises(AssertionError, match=r"(?s)block 5 \(elements 640.*bound"):
        O.check_hadamard_quant(x64, _u8(q), bad)


def test_mutant_swap_across_block_boundary():
    x64, neg, codes, scales = _mx_case("decades")
    b = next(b for b in range(1, 30) if codes[32 * b - 1] != codes[32 * b])
    bad = codes.copy()
    bad[32 * b - 1], bad[32 * b] = codes[32 * b], codes[32 * b - 1]
    with pytest.raises(AssertionError, match=rf"(?s)element {32 * b - 1} \(block {b - 1},.*bound"):
        O.check_mx_quant(x64, neg, bad, scales)


def test_mutant_padding_byte():
    x64, neg, codes, scales = _mx_case("randn", n=33)
    assert codes.size == 48
    codes[40] = 1
    with pytest.raises(AssertionError, match=r"(?s)padding: element 40 \(block 1\).*bound"):
        O.check_mx_quant(x64, neg, codes, scales)


def _scale_and_quant_before_the_floor(blocks: torch.Tensor):
    """``ops/quant.py`` ``_scale_and_quant`` as it was: scale = amax / 448 with
    no floor, so a tiny block's reciprocal is inf."""
    finite = torch.isfinite(blocks)
    amax = torch.where(finite, blocks.abs(), torch.zeros_like(blocks)).amax(dim=1)
    scale = torch.where(amax > 0, amax / torch.full_like(amax, 448.0), torch.ones_like(amax))
    inv = torch.ones_like(scale) / scale
    q = torch.where(finite, (blocks * inv[:, None]).clamp(-448.0, 448.0),
                    blocks).to(torch.float8_e4m3fn)
    return q, scale


TINY_BLOCK = [0.0, 1e-36, -5e-37, 3.3e-37, 0.0]


def test_tiny_block_before_and_after_the_floor():
    x = torch.zeros(128)
    x[:5] = torch.tensor(TINY_BLOCK)
    x64, neg = O.source_arrays(x)
    q, s = _scale_and_quant_before_the_floor(x.view(1, 128))
    old = Q.dequantize_reference(q.view(-1), s, 128, torch.float32)
    assert old.isnan().sum() == 125  # the bug: every zero restores as NaN
    with pytest.raises(AssertionError, match=r"(?s)block 0 \(elements 0.*bound"):
        O.check_block_quant(x64, neg, _u8(q.view(-1)), s.numpy(), 128)
    with pytest.raises(AssertionError, match=r"(?s)element 0 \(block 0\).*bound"):
        # the codes alone, judged under the scale the format now stores
        O.check_block_quant(x64, neg, _u8(q.view(-1)), np.float32([2.0 ** -126]), 128)

    q, s = Q.quantize_reference(x, 128)
    assert s.item() == 2.0 ** -126
    O.check_block_quant(x64, neg, _u8(q), s.numpy(), 128)
    new = Q.dequantize_reference(q, s, 128, torch.float32)
    assert not new.isnan().any() and bool((new[x == 0] == 0).all())
    assert torch.allclose(new, x, rtol=2.0 ** -4, atol=0)

    # at amax = 1e-44 the stored scale used to be 0.0
    x = torch.zeros(128)
    x[7] = 1e-44
    q, s = Q.quantize_reference(x, 128)
    assert s.item() == 2.0 ** -126 and not _u8(q).any()  # below 2^-136: flushed to zero
    O.check_block_quant(*O.source_arrays(x), _u8(q), s.numpy(), 128)

    # the rotated format shares the rule
    x = torch.zeros(128)
    x[:5] = torch.tensor(TINY_BLOCK)  # rows 1..3 are all zero
    q, s = Q.hadamard_quantize_reference(x, 128)
    O.check_hadamard_quant(O.source_arrays(x)[0], _u8(q), s.numpy())
    new = Q.hadamard_dequantize_reference(q, s, 128, torch.float32)
    assert not new.isnan().any() and bool((new[32:] == 0).all())


def test_normal_blocks_keep_their_bytes():
    """Blocks with amax / 448 >= 2^-126 are encoded exactly as before the floor."""
    for kind in ("randn", "decades", "sweep"):
        x = O.build_values(kind, 8192 + 17, torch.float32, 128)
        blocks = torch.zeros(65 * 128)
        blocks[: x.numel()] = x
        q0, s0 = _scale_and_quant_before_the_floor(blocks.view(-1, 128))
        q1, s1 = Q._scale_and_quant(blocks.view(-1, 128))
        same = (s0 >= 2.0 ** -126) | (s0 == 1.0)
        assert same.sum() >= same.numel() // 2
        assert torch.equal(s0[same], s1[same])
        assert torch.equal(q0.view(torch.uint8)[same], q1.view(torch.uint8)[same])


# ---------------------------------------------------------------------------
# snapshot round trip on the CPU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", ["block", "hadamard32"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=str)
def test_snapshot_tiny_second_moments(tmp_path, dtype, fmt):
    """``exp_avg_sq`` of rarely touched rows: values around 1e-38, exact zeros
    among them, whole rows never touched.  Every zero restores as zero and
    nothing as NaN.  (Rotated format: the rotation spreads a group's rounding
    error over its 32 elements, so only a zero in an all-zero group of 32 is
    exactly zero again; before the floor those restored as NaN too.)"""
    g = torch.Generator().manual_seed(11)
    v = (torch.rand(64, 64, generator=g, dtype=torch.float64) * 3e-38 + 2e-39)
    v[1::2] = 0.0  # rows never touched: with row 2i they share a block of 128
    if fmt == "block":
        v[torch.rand(64, 64, generator=g) < 0.3] = 0.0
    big = torch.rand(64, 64, generator=g, dtype=torch.float64) * 1e-3
    big[::3] = 0.0
    app = {"optim": StateDict(tiny=v.to(dtype), big=big.to(dtype))}
    with env(HIPSNAPSHOT_FP8_FORMAT=fmt):
        Snapshot.take(str(tmp_path / "s"), app, quantize=["optim/*"])
    e = Snapshot(str(tmp_path / "s")).get_manifest()["0/optim/tiny"]
    assert e.quant["format"] == "fp8_e4m3fn_block"
    assert e.quant["rotation"] == ("hadamard32" if fmt == "hadamard32" else "none")
    out = {"optim": StateDict(tiny=torch.ones(64, 64, dtype=dtype),
                              big=torch.ones(64, 64, dtype=dtype))}
    Snapshot(str(tmp_path / "s")).restore(out)
    for name in ("tiny", "big"):
        src, got = app["optim"][name], out["optim"][name]
        assert not got.isnan().any(), name
        zero = src == 0
        if fmt == "hadamard32":
            zero = (src.view(-1, 32) == 0).all(dim=1, keepdim=True).expand(-1, 32).reshape(64, 64)
        assert zero.sum() >= 1000 and bool((got[zero] == 0).all()), name
        err = (got.double() - src.double()).abs()
        amax = src.double().abs().view(-1, 128).amax(dim=1, keepdim=True).expand(-1, 128)
        # a code c of y / s is within max(2^-4 |c|, 2^-10) of it and
        # |c| <= (1 + 2^-4) |y / s|; s = max(amax / 448, 2^-126).  Rotated, a
        # restored value averages 32 code errors of rotated values, each at
        # most 32 times the block's amax.  Plus the destination's own
        # rounding (2^-9 relative for bf16).
        spread = 32.0 if fmt == "hadamard32" else 1.0
        scale = (spread * amax / 448.0).clamp_min(2.0 ** -126)
        mag = spread * amax if fmt == "hadamard32" else src.double().abs().view(-1, 128)
        bound = mag * (2.0 ** -4 * 1.0625) + scale * 2.0 ** -10 + amax * 2.0 ** -8
        assert bool((err.view(-1, 128) <= bound).all()), name
