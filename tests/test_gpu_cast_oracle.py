"""``hs_copy_nd`` (``csrc/hscopy.hip``) against the integer oracle of
``cast_oracle.py`` (proved on the CPU by ``test_cast_oracle.py``), driven
through ``native.CopyBatch``.

Casts: each of the 12 pairs among f16, bf16, f32 and f64 converts its value set
(every 16-bit pattern, or every tie, subnormal, overflow boundary,
double-rounding trap and special of a wide source) in three layouts:

* aligned contiguous: ``copy_contig_cast``'s 8-per-lane body and its scalar
  tail for the pairs among f16 / bf16 / f32, ``copy_strided_cast<1>`` for the
  f64 pairs;
* offset contiguous, both views one element into their buffers: the scalar
  path, from unaligned tile starts;
* strided, a column-narrowed source into a window of a transposed padded
  buffer: ``copy_strided_cast<2>``, rows no multiple of the 8-element run.

Each must equal ``expected_bits`` wherever the source is no NaN, give a NaN
wherever it is one, agree with the other two bit for bit, and leave the 0xA5
fill around and between its destination elements alone.  torch's ``.to()`` on
the same device is a second reference for the non-NaN inputs.

Same-dtype copies must carry every bit pattern through, signalling NaNs and
payloads included: all 65 536 patterns of bf16 and f16 through the LDS
transpose, the rows mode and the generic strided copy, f32 through the
transpose, and complex128 (the only 16-byte element, never copied from a
strided view by another test) through ``copy_strided_same<ND, 16>``."""

import functools

import numpy as np
import pytest
import torch

import cast_oracle as C
from hipsnapshot.ops import native

pytestmark = pytest.mark.gpu

GUARD = 64   # bytes of fill in front of and behind every destination
ROW = 1003   # row length of the strided layout: odd, so no multiple of kRun = 8
FLAG_ROWS, FLAG_TRANSPOSE = 2, 4


@functools.lru_cache(maxsize=None)
def _expected(src, dst):
    return C.expected_bits(C.source_set(src, dst), src, dst)


def _fill_value(dtype):
    return int.from_bytes(b"\xa5" * torch.empty(0, dtype=dtype).element_size(), "little",
                          signed=True)


def _buffer(gpu, shape, int_dtype):
    return torch.full(tuple(shape), _fill_value(int_dtype), dtype=int_dtype, device=gpu)


def _assert_untouched_outside(big, window_of, what):
    chk = big.clone()
    window_of(chk).fill_(_fill_value(big.dtype))
    bad = (chk != _fill_value(big.dtype)).reshape(-1).nonzero()
    assert bad.numel() == 0, (f"{what}: element {int(bad[0])} of the destination buffer, outside "
                              f"the window, was overwritten ({bad.numel()} in all)")


def _launch(batch):
    batch.launch(0, int(torch.cuda.current_stream().cuda_stream), sync=True)


def _bits(int_tensor):
    a = int_tensor.contiguous().cpu().numpy().reshape(-1)
    return a.view("u" + a.dtype.name).astype(np.uint64)


def _cast(src_i, src, dst_i, dst, ndim):
    """One launch converting the ``src`` values held by int tensor ``src_i``
    into the ``dst`` values of int tensor ``dst_i`` (views of any strides)."""
    b = native.CopyBatch()
    b.add(src_i.data_ptr(), C.TORCH_FLOAT[src], src_i.stride(), dst_i.data_ptr(),
          C.TORCH_FLOAT[dst], dst_i.stride(), list(src_i.shape), src_i.element_size())
    (row,) = b.rows
    assert row[3] == ndim and row[6] == 0 and row[4] >= 10 and row[5] >= 10, row  # the cast path
    _launch(b)


@pytest.mark.parametrize("src,dst", C.PAIRS, ids=["->".join(p) for p in C.PAIRS])
def test_cast_vs_oracle(gpu, src, dst):
    bits = C.source_set(src, dst)
    want, is_nan = _expected(src, dst)  # one oracle call per pair
    n = bits.size
    n_lin = (n + 7) // 8 * 8 + 5  # whole vectors of 8, then a 5-element tail
    rows = -(-n // ROW)
    idx = np.arange(max(n_lin, rows * ROW)) % n  # the set, then its beginning again
    si, di = C.TORCH_INT[src], C.TORCH_INT[dst]
    base = C.to_tensor(bits[idx], src).view(si).to(gpu)  # the one upload
    g = GUARD // torch.empty(0, dtype=di).element_size()
    got = {}

    def run(layout, s, big, window_of, ndim):
        d = window_of(big)
        _cast(s, src, d, dst, ndim)
        what = f"{src}->{dst} {layout}"
        _assert_untouched_outside(big, window_of, what)
        got[layout] = out = _bits(d)
        k = idx[:out.size]
        print(f"{what}: {out.size} elements, {int(is_nan[k].sum())} NaN sources")
        C.check_cast(bits[k], out, want[k], is_nan[k], src, dst, what)

    s = base[:n_lin]
    big = _buffer(gpu, [g + n_lin + g], di)
    assert s.data_ptr() % 16 == 0 and big[g:].data_ptr() % 16 == 0
    run("aligned", s, big, lambda b: b[g: g + n_lin], 1)

    sbuf = _buffer(gpu, [1 + n_lin], si)
    sbuf[1:] = base[:n_lin]
    big = _buffer(gpu, [g + 1 + n_lin + g], di)
    assert sbuf[1:].data_ptr() % 16 and big[g + 1:].data_ptr() % 16
    run("offset", sbuf[1:], big, lambda b: b[g + 1: g + 1 + n_lin], 1)

    swide = _buffer(gpu, [rows, ROW + 7], si)
    swide[:, 3: 3 + ROW] = base[:rows * ROW].view(rows, ROW)
    big = _buffer(gpu, [ROW + 9, rows + 9], di)
    assert 5 * (rows + 9) * big.element_size() >= GUARD
    run("strided", swide[:, 3: 3 + ROW], big, lambda b: b.t()[3: 3 + rows, 5: 5 + ROW], 2)

    # the same blob restored through different layouts gives the same bytes
    for other in ("offset", "strided"):
        m = min(got["aligned"].size, got[other].size)
        bad = np.flatnonzero(got["aligned"][:m] != got[other][:m])
        assert bad.size == 0, (
            f"{src}->{dst}: {src} {int(bits[idx[bad[0]]]):#x} gives {int(got['aligned'][bad[0]]):#x} "
            f"aligned and {int(got[other][bad[0]]):#x} {other} ({bad.size} differ)")

    # the kernel's comments promise bit identity with torch's copy_
    ref = _bits(base[:n].view(C.TORCH_FLOAT[src]).to(C.TORCH_FLOAT[dst]).view(di))
    C.check_cast(bits, ref, want, is_nan, src, dst, f"{src}->{dst} torch on the device")


# -- same-dtype copies keep every bit ------------------------------------------------

def _contiguous(gpu, shape, trail, int_dtype):
    """A contiguous destination of ``shape`` between two guards."""
    n = int(np.prod(shape))
    g = GUARD // (torch.empty(0, dtype=int_dtype).element_size() * int(np.prod(trail or [1])))
    big = _buffer(gpu, [g + n + g, *trail], int_dtype)
    return big, lambda b: b[g: g + n].view(*shape, *trail)


def _window(lo, outer):
    """A destination that is the window starting at ``lo`` of a buffer of
    shape ``outer``."""
    def make(gpu, shape, trail, int_dtype):
        big = _buffer(gpu, [*outer, *trail], int_dtype)
        sl = tuple(slice(a, a + z) for a, z in zip(lo, shape))
        assert all(a + z < o for a, z, o in zip(lo, shape, outer))
        return big, lambda b: b[sl]
    return make


def _copy_keeps_bits(gpu, words, shape, typed, pick, make_dst, path, what):
    """Copy ``pick(source)`` into a destination made by ``make_dst`` with one
    launch and compare the words.  ``words`` is a CPU int tensor of the
    source's elements in C order, ``(numel,)`` or ``(numel, 2)`` for complex;
    ``typed`` turns an int tensor into the tensor type under test.  ``path``
    is ``(flags & 7, ndim, vector width or None)`` of the descriptor."""
    trail = list(words.shape[1:])
    src = pick(typed(words.view(*shape, *trail).to(gpu)))
    index = pick(torch.arange(words.shape[0]).view(*shape))  # source element of each output
    big, window_of = make_dst(gpu, list(index.shape), trail, words.dtype)
    dst = typed(window_of(big))
    b = native.CopyBatch()
    native.tensor_copy_descriptor(b, src, dst)
    (row,) = b.rows
    assert (row[6] & 7, row[3]) == path[:2] and row[4] == row[5] < 10, (what, row)
    assert path[2] is None or row[6] >> 8 == path[2], (what, row)
    _launch(b)
    out = window_of(big).cpu().reshape(-1, *trail)
    ref = words[index.reshape(-1)]
    bad = (out != ref).reshape(out.shape[0], -1).any(1).nonzero()
    assert bad.numel() == 0, (
        f"{what}: output element {int(bad[0])} holds {out[int(bad[0])].tolist()}, the source "
        f"{ref[int(bad[0])].tolist()} ({bad.numel()} differ)")
    _assert_untouched_outside(big, window_of, what)


def _all_patterns_16():
    return torch.from_numpy(np.arange(1 << 16, dtype=np.uint16).view(np.int16).copy())


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize("case", ["transpose", "rows", "generic"])
def test_16bit_copies_keep_every_pattern(gpu, dtype, case):
    pick, make_dst, path = {
        "transpose": (lambda t: t.t(), _contiguous, (FLAG_TRANSPOSE, 3, None)),
        "rows": (lambda t: t[:, 3:250], _contiguous, (FLAG_ROWS, 2, 2)),
        "generic": (lambda t: t[::2, 1::3], _window((5, 7), (140, 100)), (0, 2, None)),
    }[case]
    _copy_keeps_bits(gpu, _all_patterns_16(), (256, 256), lambda t: t.view(dtype), pick, make_dst,
                     path, f"{dtype} {case}")


def test_f32_transpose_keeps_every_pattern(gpu):
    p = np.arange(1 << 16, dtype=np.uint32)
    words = torch.from_numpy((p << 16 | p).view(np.int32).copy())
    _copy_keeps_bits(gpu, words, (256, 256), lambda t: t.view(torch.float32), lambda t: t.t(),
                     _contiguous, (FLAG_TRANSPOSE, 3, None), "float32 transpose")


def _complex_words(numel):
    """``(numel, 2)`` int64 words: the f64 specials, then random bits."""
    rng = np.random.default_rng(16)
    w = rng.integers(0, 1 << 64, 2 * numel, dtype=np.uint64)
    sp = C.specials("f64")
    w[:sp.size] = sp
    w[sp.size: 2 * sp.size] = sp[::-1]  # every special in a real and in an imaginary word
    return torch.from_numpy(w.view(np.int64).reshape(numel, 2).copy())


def _complex(t):
    return torch.view_as_complex(t.view(torch.float64))


@pytest.mark.parametrize("case", ["transpose", "narrowed", "into_window", "permuted",
                                  "permuted_into_window"])
def test_complex128_strided_copies_keep_every_bit(gpu, case):
    shape, pick, make_dst, ndim = {
        "transpose": ((65, 67), lambda t: t.t(), _contiguous, 2),
        "narrowed": ((65, 67), lambda t: t[3:60, 5:40], _contiguous, 2),
        "into_window": ((65, 67), lambda t: t, _window((7, 11), (80, 90)), 2),
        # [11, 5, 9] out of [5, 9, 11]: the last two dims merge on both sides
        "permuted": ((5, 9, 11), lambda t: t.permute(2, 0, 1), _contiguous, 2),
        "permuted_into_window": ((5, 9, 11), lambda t: t.permute(2, 0, 1),
                                 _window((1, 2, 2), (13, 8, 12)), 3),
    }[case]
    words = _complex_words(int(np.prod(shape)))
    assert words.shape[0] * 16 <= 8 << 20
    _copy_keeps_bits(gpu, words, shape, _complex, pick, make_dst, (0, ndim, None),
                     f"complex128 {case}")
