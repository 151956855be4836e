"""Blockwise OCP-fp8 (e4m3fn) quantized save / dequantized restore (K5/K9).

Opt-in (``Snapshot.take(..., quantize=["model/**"])``): floating tensors are
written as 1 byte/element plus one fp32 scale per 128-element block, halving
bf16 checkpoint bytes (quartering fp32).  The entry's ``dtype`` stays the
ORIGINAL dtype so restore targets match in place; ``quant`` records the
layout::

    {"format": "fp8_e4m3fn_block", "block": 128, "rotation": "hadamard32"|"none",
     "payload_bytes": P, "nblocks": B, "total_bytes": P + 4B, ...}

blob = ``[fp8 payload (P bytes)][B fp32 scales]``.

rotation ``"hadamard32"`` (opt-in, ``HIPSNAPSHOT_FP8_FORMAT=hadamard32``): the flat
tensor is cut into groups of 32 elements and each group is multiplied by the
32x32 Sylvester Hadamard matrix H (+-1 entries) before quantization; restore
computes ``(Y' H) / 32``.  The rotation spreads outliers over the group; for
e4m3 that only pays when a block's dynamic range exceeds the format's (see
``default_rotation``), so it is off by default.  On MI355X both directions run on the
matrix cores.  bf16 / f16 tensors are rotated by ``v_mfma_f32_32x32x16_{bf16,f16}``
(``hs_fp8_hadamard_quant16``: 2 MFMAs per 1024 elements; the MFMA sums 16 exact
products in its own order, so a code can differ from the fp32 reference by one
fp8 ulp -- tests bound it.  So a bf16 / f16 tensor's rotated blob is NOT
byte-reproducible across devices: quantized on the GPU and on the CPU it can
give different codes, blob bytes and checksums.  Nothing depends on the two
matching -- a checksum is of the bytes actually written, and replicated
entries are deduplicated by manifest, not by blob contents); fp32 tensors use ``v_mfma_f32_32x32x2_f32``
(exact f32 k-ordered FMA chains, ``hs_fp8_hadamard_quant``), bit-identical to
the torch reference below, which uses the same sequential k order.  Every
dequantization runs on ``v_mfma_f32_32x32x16_bf16`` over the codes widened to
bf16 (``hs_fp8_hadamard_dequant8``): the row sums of e4m3 values are exact, so
GPU and torch restores agree bit for bit.

rotation ``"none"`` (default): plain blockwise quantization (``hs_fp8_quant`` kernel:
one wave per block, 64-lane xor-shuffle amax, ``v_cvt_pk_fp8_f32`` -- gfx950
converts to OCP e4m3fn natively).

Scale rule (both): ``scale = max(amax / 448, 2^-126)`` (the quotient correctly
rounded; 1 when the block is all zeros), ``q = e4m3fn(clamp(y * (1 / scale)))``
with round-to-nearest-even.  The floor at the smallest normal float32 keeps
``1 / scale <= 2^126`` finite: without it a block whose ``amax`` is below about
1.3e-36 (Adam second moments of rarely touched rows) got a subnormal or zero
scale, ``1 / scale = inf``, every zero restored as NaN (``0 * inf``) and every
non-zero as ``+-amax``.  Inside a floored block ``|y| / scale < 448``, zeros
stay zeros and values below ``2^-136`` flush to zero: that is the format's
floor.  Blocks with ``amax / 448 >= 2^-126`` are unchanged, and a stored scale
means what it always did, so older snapshots decode as before.  The kernels
(``csrc/hsquant.hip`` ``fp8_block_scale``) apply the same rule.

MX layout (default for un-rotated tensors; ``HIPSNAPSHOT_FP8_FORMAT=block``
selects the fp32-scale layout above)::

    {"format": "fp8_e4m3fn_mx", "block": 32, "scale": "e8m0", "rotation": "none",
     "payload_bytes": P = round_up(n, 16), "nblocks": B = ceil(n / 32),
     "total_bytes": P + B}

blob = ``[fp8 payload (P bytes, zero padded)][B E8M0 scale bytes]`` -- the OCP
MX block format: one power-of-two scale ``2^k`` per 32 elements, byte
``k + 127``.  ``k`` is the smallest exponent with ``amax <= 448 * 2^k``
(``amax`` over the block's finite elements; inf / nan are stored as e4m3fn
NaN with their sign, as torch's cast does)
(``amax = m * 2^e`` by frexp: ``k = e - 9`` if ``m <= 0.875`` else ``e - 8``;
0 for all-zero / non-finite blocks, clamped to [-127, 127]), so ``x * 2^-k``
is EXACT: no division, no saturation, and restore ``q * 2^k`` is exact in
fp32.  That takes the per-element correctly rounded division off the GPU
(``hs_mx8_quant`` streams at the HBM roof) while the blob stays bit-identical
to the torch reference below.  Same 1/32 scale overhead as fp32 scales per
128 elements, at 4x finer granularity.

MXFP4 layout (opt-in, ``HIPSNAPSHOT_FP8_FORMAT=mxfp4``): 4.25 bits per element,
half of MX fp8::

    {"format": "fp4_e2m1_mx", "block": 32, "scale": "e8m0", "rotation": "none",
     "orig_dtype": ..., "payload_bytes": P = round_up(ceil(n / 2), 16),
     "nblocks": B = ceil(n / 32), "total_bytes": P + B}

blob = ``[P payload bytes][B E8M0 scale bytes]``.  Element ``2i`` is the low
nibble of byte ``i`` and element ``2i + 1`` the high one (the OCP /
``float4_e2m1fn_x2`` order); for odd ``n`` the last high nibble is zero, and
bytes ``[ceil(n / 2), P)`` are zero.  The rules, shared by ``hs_mxfp4_quant`` /
``hs_mxfp4_dequant`` (``csrc/hsquant.hip``) and the references below:

* a code is sign (bit 3) and an index (bits 0-2) into
  ``{0, 0.5, 1, 1.5, 2, 3, 4, 6}``;
* the scale is ``2^k``, stored as ``k + 127``, with ``k`` the smallest exponent
  such that ``amax <= 6 * 2^k`` over the block's finite elements (``amax =
  m * 2^e`` by frexp: ``k = e - 3`` if ``m <= 0.75`` else ``e - 2``; clamped to
  [-127, 127]; 0 for a block that is all zero or has no finite element), so
  ``x * 2^-k`` is exact and at most 6: no division, no clamp;
* round to nearest on the magnitude, ties to the even index (0.25 -> 0,
  0.75 -> 1, 1.25 -> 1, 1.75 -> 2, 2.5 -> 2, 3.5 -> 4, 5 -> 4); the source's
  sign bit is kept, also when the magnitude rounds to zero;
* ``+-inf`` becomes code ``+-6`` and does not set the scale;
* e2m1 has no NaN code.  Unlike the fp8 layouts, where a NaN keeps its own
  element, a block that holds a NaN stores the MX NaN scale ``0xFF`` and 16
  zero payload bytes, and every element of it restores as a positive quiet
  NaN;
* restore is ``q * 2^k``, exact in fp32, then one rounding to the target
  dtype.  Known edge, as in MX fp8: a finite ``|x| >= 0.875 * 2^128`` rounds
  to a code whose product overflows fp32 and restores as inf.

A CPU take and a GPU take of a tensor write identical bytes, and a restore on
either side equals ``mxfp4_dequantize_reference`` bit for bit.

Measured relative L2 error ``|restored - x| / |x|`` of the CPU references on
2^20 seeded values: N(0, 1): ``mxfp4`` 0.1155, ``mx`` 0.0266; Student-t(2):
``mxfp4`` 0.1239, ``mx`` 0.0262.

MXFP6 layout (opt-in, ``HIPSNAPSHOT_FP8_FORMAT=mxfp6``): the OCP MX element
format FP6 e2m3, 6.25 bits per element, between MX fp8 (8.25) and MXFP4
(4.25)::

    {"format": "fp6_e2m3_mx", "block": 32, "scale": "e8m0", "rotation": "none",
     "orig_dtype": ..., "nblocks": B = ceil(n / 32),
     "payload_bytes": P = round_up(24 * B, 16), "total_bytes": P + B}

blob = ``[P payload bytes][B E8M0 scale bytes]``.  Block ``b`` is payload bytes
``[24 b, 24 b + 24)`` read as a little-endian 192-bit string, and element ``j``
of the block is bits ``[6 j, 6 j + 6)`` of it (4 codes in 3 bytes).  Elements
past ``n`` in the last block are code 0 and bytes ``[24 B, P)`` are zero.  The
rules, shared by ``hs_mxfp6_quant`` / ``hs_mxfp6_dequant`` (``csrc/hsquant.hip``)
and the references below:

* a code is sign (bit 5), exponent (bits 4-3, bias 1) and mantissa (bits 2-0):
  the 32 magnitudes are ``0, 0.125 .. 0.875`` (subnormal), ``1 .. 1.875`` in
  steps of 0.125, ``2 .. 3.75`` in steps of 0.25 and ``4 .. 7.5`` in steps of
  0.5 (``E2M3_VALUES``);
* the scale is ``2^k``, stored as ``k + 127``, with ``k`` the smallest exponent
  such that ``amax <= 7.5 * 2^k`` over the block's finite elements (``amax =
  m * 2^e`` by frexp: ``k = e - 3`` if ``m <= 0.9375`` else ``e - 2``; clamped
  to [-127, 127]; 0 for a block that is all zero or has no finite element), so
  ``x * 2^-k`` is exact and at most 7.5: no division, no clamp;
* round to nearest on the magnitude, ties to the even index; the source's sign
  bit is kept, also when the magnitude rounds to zero;
* ``+-inf`` becomes code ``+-7.5`` (index 31) and does not set the scale;
* e2m3 has no NaN code: as in MXFP4 a block that holds a NaN stores the MX NaN
  scale ``0xFF`` and 24 zero payload bytes, and restores as 32 positive quiet
  NaNs;
* restore is ``q * 2^k``, exact in fp32, then one rounding to the target
  dtype.  Known edge, as in the other MX formats: a finite ``|x|`` that rounds
  up to a code whose product overflows fp32 restores as inf.

A CPU take and a GPU take of a tensor write identical bytes, and a restore on
either side equals ``mxfp6_dequantize_reference`` bit for bit; no matrix
instruction is involved.

Relative L2 error of a float64 model of the MX rule on 2^20 seeded values,
``mxfp4`` / ``mxfp6`` / ``mx``: N(0, 1) 0.1154 / 0.0283 / 0.0265; Student-t(2)
0.1327 / 0.0350 / 0.0245; Laplace 0.1321 / 0.0308 / 0.0266: the error of fp8
(+7 % on Gaussians) for 24 % fewer bytes.

Rotated MXFP4 layout (opt-in, ``HIPSNAPSHOT_FP8_FORMAT=mxfp4_hadamard32``):
MXFP4 whose blocks are Hadamard-rotated groups, the same 4.25 bits per
element::

    {"format": "fp4_e2m1_mx", "block": 32, "scale": "e8m0", "rotation": "hadamard32",
     "orig_dtype": ..., "payload_bytes": P = n_pad / 2, "nblocks": B = n_pad / 32,
     "total_bytes": P + B}      with n_pad = round_up(n, 32)

blob = ``[P payload bytes][B E8M0 bytes]``.  One outlier pushes the other 31
values of an e2m1 block to the bottom of an 8-magnitude grid; the rotation
spreads it over exactly the 32 elements that share the scale byte.  The rules,
shared by ``hs_mxfp4_hadamard_quant`` / ``hs_mxfp4_hadamard_dequant`` and the
references below (test ``is_mxfp4_hadamard`` before ``is_mxfp4``, which looks
at ``format`` only):

* the flat tensor, zero-padded to ``n_pad``, is cut into groups of 32 and group
  ``g`` is rotated, ``y = x_g H`` with ``H = hadamard_matrix()``, the sums in
  fp32 in ``HADAMARD_K_ORDER`` (``_rotate_sequential``);
* the 32 rotated values of a group are one MX block: scale and codes follow the
  ``mxfp4`` rules on ``y`` (``k``, clamp, ties to the even index, sign kept on
  zero, nibble order);
* stricter than ``mxfp4`` on non-finite values: if any rotated value of a group
  is inf or NaN -- an input inf (it makes every rotated value +-inf, and code
  +-6 would restore finite garbage), an input NaN, or an fp32 overflow of a
  sum -- the group stores scale byte ``0xFF`` and 16 zero bytes and restores
  as 32 positive quiet NaNs, as a non-finite input spoils its own row of 32 in
  the rotated fp8 format;
* restore is ``x = (Q H) * 2^(k - 5)``: a row sum of e2m1 values is a multiple
  of 0.5 of magnitude <= 192, exact in fp32 in any order, the product with the
  power of two is one fp32 operation, then one rounding to the target dtype.
  So a blob restores to the same bits on the CPU and on the GPU for every
  target dtype.

A CPU take and a GPU take of an fp32 tensor write identical bytes.  bf16 / f16
tensors go through the 16-bit MFMA, which sums in the hardware's order: a
rotated value can differ from the k-ordered reference in its last fp32 bit and
a code exactly on a rounding boundary can move -- the known gap of
``hadamard32`` (``docs/next_steps.md``), far rarer for e2m1 (other summation
orders on the CPU moved at most 1 code in 2^20 and no scale byte).

Measured relative L2 error of the CPU references on 2^20 seeded values,
``mxfp4`` / ``mxfp4_hadamard32``: N(0, 1) 0.1154 / 0.1184; Student-t(2) 0.1327 /
0.1011; Student-t(3) 0.1505 / 0.1129; Student-t(5) 0.1327 / 0.1151; Laplace
0.1322 / 0.1151; N(0, 1) with every 257th value x50: 0.1361 / 0.1050.  About a
quarter lower on heavy tails, 2.6 % higher on pure Gaussians.

Two-level-scaled FP4 layout (opt-in, ``HIPSNAPSHOT_FP8_FORMAT=nvfp4``): the
"NVFP4" layout that other tools read, 4.5 bits per element::

    {"format": "fp4_e2m1_nv", "block": 16, "scale": "e4m3+fp32", "rotation": "none",
     "orig_dtype": ..., "nblocks": B = ceil(n / 16),
     "payload_bytes": P = round_up(ceil(n / 2), 16),
     "total_bytes": P + round_up(B, 4) + 4}

blob = ``[P payload bytes][B e4m3fn scale bytes][zero pad to 4][fp32 A]``.  The
payload is ``mxfp4``'s: the same e2m1 codes, nibble order and zero fill from
element ``n`` on.  ``A`` is the tensor's amax over its finite elements, 0 when
it has no finite non-zero element.  An MX scale is a power of two shared by 32
elements, so a block's largest value lands anywhere in the top octave of the
grid; here a block of 16 has an e4m3 scale, which puts it within 1/16 of 6, and
``A`` places the e4m3 range.  Every step below is ONE fp32 operation, in
``hs_nvfp4_amax`` / ``hs_nvfp4_quant`` / ``hs_nvfp4_dequant`` and in the
references alike:

* tensor scale ``ts = max(A / 2688, 2^-117)`` (2688 = 448 * 6, the quotient
  correctly rounded), evaluated the same way by the quantizer and the restore.
  The floor keeps every non-zero block scale ``d >= 2^-126`` so that ``1 / d``
  is finite (the reason for the floor of the fp32 block scales above);
* block scale byte ``s8 = e4m3fn_rne(min(bamax / (6 * ts), 448))`` with
  ``bamax`` the block's amax over its finite elements and ``6 * ts`` an fp32
  product: one correctly rounded division per block.  Decoded: ``d = f32(s8) *
  ts``, an fp32 product;
* element ``y = clamp(x * (1 / d), -6, 6)``, then the e2m1 code, round to
  nearest with ties to the even index, the source's sign bit kept also on a
  zero result.  The clamp is part of the rule: ``s8`` is rounded to nearest, so
  ``bamax / d`` can exceed 6;
* ``s8 == 0`` (an all-zero block, or one whose amax is more than about 2^22
  below ``A``): every code of the block is its element's sign bit alone, an inf
  included, and the block restores as signed zeros.  That is the format's
  floor: a tensor whose magnitudes span a large range ACROSS blocks -- Adam
  second moments, whose rows differ by tens of octaves -- loses its small
  blocks entirely and should stay on ``mx``, whose scale is free per block;
* ``+-inf`` becomes code ``+-6`` (the clamp) and sets neither ``bamax`` nor
  ``A``;
* a block that holds a NaN stores the e4m3fn NaN byte ``0x7F`` and 8 zero
  payload bytes and restores as 16 positive quiet NaNs (the MXFP4 convention);
  the NaN takes no part in ``A`` (the block's finite elements do);
* restore is ``q * d``, one fp32 product, then one rounding to the target
  dtype.

A CPU take and a GPU take write identical bytes for bf16, f16 and fp32 sources,
and a restore on either side equals ``nvfp4_dequantize_reference`` bit for bit
for bf16, f16, fp32 and fp64 targets.

Relative L2 error of a float64 model of the rules on 2^20 seeded values,
``mxfp4`` / ``mxfp4_hadamard32`` / ``nvfp4``: N(0, 1) 0.1154 / 0.1184 / 0.0950;
Student-t(2) 0.1327 / 0.1011 / 0.0645; Laplace 0.1321 / 0.1151 / 0.0927: 18 to
50 % less error than ``mxfp4`` for 6 % more bytes.

Error-budgeted choice (opt-in, ``HIPSNAPSHOT_FP8_FORMAT=auto[:max_error[:formats]]``):
the figures above come from synthetic data, and one format per process is
wrong for a real state.  ``format_errors(t)`` measures what ``mxfp4`` (4.25
bits per element), ``nvfp4`` (4.5), ``mxfp6`` (6.25) and ``mx`` (8.25) would
lose on ``t`` itself -- the sums that ``format_errors_reference`` states, by
``hs_quant_probe`` in one read of a tensor in HBM (every element round-tripped
through the four formats in registers, f64 sums reduced in a fixed order, so
the report is a function of the tensor's bytes) -- and ``choose_format`` picks
the smallest candidate that spoils no finite element and whose relative L2
error is within ``knobs.quant_max_error()`` (default 0.03).  A take under
``auto`` does that for every tensor it writes (``io/tensor.py``), records the
measured ``rel_l2`` and ``"selected": "auto"`` in the entry's ``quant`` dict,
and writes a tensor that no candidate serves unquantized.  The rotated formats
and ``block`` are not candidates.  On an MI355X the probe of 512 Mi bf16
elements takes 0.99 ms with the amax pass of ``nvfp4`` and 0.66 ms without
``nvfp4`` among the candidates (f32: 1.35 / 0.79 ms), against 0.39 ms for an
``nvfp4`` quantization: it is bound by the vector ALU, not by HBM
(``docs/architecture.md`` section 4); a take of 300 tensors pays about 50 us
per tensor for it and its host wait.
"""

from __future__ import annotations

import os
from typing import Any, Dict

import torch

from ..format.manifest import TensorEntry
from ..format.serialization import FP8_QUANTIZABLE_DTYPES, dtype_to_string, string_to_dtype
from ..io_types import StagedBuffer

FP8_MAX = 448.0
FP8_MIN_SCALE = 2.0 ** -126  # smallest normal float32: floor of a block's fp32 scale
DEFAULT_VPT = 2
GROUP = 32


def block_elems(vpt: int = DEFAULT_VPT) -> int:
    return 64 * vpt


def default_rotation() -> str:
    # Measured (tests/test_quant.py::test_rotation_error_tradeoff): e4m3 is a
    # floating format, so an outlier only costs its own relative precision;
    # rotating spreads the outlier's absolute error over its whole group.  On
    # Student-t(2) weights the rotated L2 error is ~1.6x the plain one, so the
    # rotation is opt-in; it pays when a block's dynamic range exceeds e4m3's
    # ~2^15 (values far below amax would otherwise fall into subnormals).
    from .. import knobs

    return "hadamard32" if knobs.fp8_format() == "hadamard32" else "none"


def default_scale() -> str:
    """``e8m0`` (MX, default) or ``fp32`` (``HIPSNAPSHOT_FP8_FORMAT=block``)
    for un-rotated quantization."""
    from .. import knobs

    return "fp32" if knobs.fp8_format() == "block" else "e8m0"


MX_BLOCK = 32


def is_mx(info: Dict[str, Any]) -> bool:
    return info.get("format") == "fp8_e4m3fn_mx"


def is_mxfp4(info: Dict[str, Any]) -> bool:
    return info.get("format") == "fp4_e2m1_mx"


def is_mxfp4_hadamard(info: Dict[str, Any]) -> bool:
    """Test this before ``is_mxfp4``, which looks at ``format`` only."""
    return is_mxfp4(info) and info.get("rotation") == "hadamard32"


def mxfp4_payload_bytes(n: int) -> int:
    return _round_up((n + 1) // 2, 16)


def is_mxfp6(info: Dict[str, Any]) -> bool:
    return info.get("format") == "fp6_e2m3_mx"


def mxfp6_payload_bytes(n: int) -> int:
    """24 bytes per block of 32, rounded up to 16."""
    return _round_up(24 * ((n + MX_BLOCK - 1) // MX_BLOCK), 16)


NV_BLOCK = 16


def is_nvfp4(info: Dict[str, Any]) -> bool:
    return info.get("format") == "fp4_e2m1_nv"


def nvfp4_payload_bytes(n: int) -> int:
    """The ``mxfp4`` payload: two codes per byte, rounded up to 16."""
    return mxfp4_payload_bytes(n)


def fp8_supported(t: torch.Tensor) -> bool:
    return t.dtype in FP8_QUANTIZABLE_DTYPES and hasattr(torch, "float8_e4m3fn") \
        and t.numel() > 0


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def fp8_entry_quant_info(t: torch.Tensor, vpt: int = DEFAULT_VPT, rotation: str = None,
                         fmt: str = None) -> Dict[str, Any]:
    """The ``quant`` dict of ``t`` under format ``fmt`` (a value of
    ``knobs.fp8_format()``, which is the default)."""
    if fmt is None:
        from .. import knobs

        fmt = knobs.fp8_format()
    n = t.numel()
    if rotation in (None, "hadamard32") and fmt == "mxfp4_hadamard32":
        nblocks = _round_up(n, GROUP) // GROUP  # block = rotated group
        return {"format": "fp4_e2m1_mx", "block": MX_BLOCK, "scale": "e8m0",
                "rotation": "hadamard32", "orig_dtype": dtype_to_string(t.dtype),
                "payload_bytes": 16 * nblocks, "nblocks": nblocks, "total_bytes": 17 * nblocks}
    rotation = rotation or ("hadamard32" if fmt == "hadamard32" else "none")
    if rotation == "none" and fmt == "mxfp4":
        payload = mxfp4_payload_bytes(n)
        nblocks = (n + MX_BLOCK - 1) // MX_BLOCK
        return {"format": "fp4_e2m1_mx", "block": MX_BLOCK, "scale": "e8m0",
                "rotation": "none", "orig_dtype": dtype_to_string(t.dtype),
                "payload_bytes": payload, "nblocks": nblocks, "total_bytes": payload + nblocks}
    if rotation == "none" and fmt == "mxfp6":
        payload = mxfp6_payload_bytes(n)
        nblocks = (n + MX_BLOCK - 1) // MX_BLOCK
        return {"format": "fp6_e2m3_mx", "block": MX_BLOCK, "scale": "e8m0",
                "rotation": "none", "orig_dtype": dtype_to_string(t.dtype), "nblocks": nblocks,
                "payload_bytes": payload, "total_bytes": payload + nblocks}
    if rotation == "none" and fmt == "nvfp4":
        payload = nvfp4_payload_bytes(n)
        nblocks = (n + NV_BLOCK - 1) // NV_BLOCK
        return {"format": "fp4_e2m1_nv", "block": NV_BLOCK, "scale": "e4m3+fp32",
                "rotation": "none", "orig_dtype": dtype_to_string(t.dtype), "nblocks": nblocks,
                "payload_bytes": payload, "total_bytes": payload + _round_up(nblocks, 4) + 4}
    if rotation == "none" and fmt != "block":
        payload = _round_up(n, 16)
        nblocks = (n + MX_BLOCK - 1) // MX_BLOCK
        return {"format": "fp8_e4m3fn_mx", "block": MX_BLOCK, "scale": "e8m0",
                "rotation": "none", "orig_dtype": dtype_to_string(t.dtype),
                "payload_bytes": payload, "nblocks": nblocks, "total_bytes": payload + nblocks}
    if rotation == "hadamard32":
        block = 128
        n_q = _round_up(n, GROUP)
    else:
        block = block_elems(vpt)
        n_q = n
    payload = _round_up(n_q, 16)
    nblocks = (n_q + block - 1) // block
    return {"format": "fp8_e4m3fn_block", "block": block, "vpt": vpt, "rotation": rotation,
            "orig_dtype": dtype_to_string(t.dtype), "payload_bytes": payload,
            "nblocks": nblocks, "total_bytes": payload + 4 * nblocks}


# ---------------------------------------------------------------------------
# torch fp32 references
# ---------------------------------------------------------------------------

def _scale_and_quant(blocks: torch.Tensor):
    # over the finite elements: an inf / nan does not set its block's scale,
    # and its code is the e4m3fn NaN with its sign (torch's cast of inf / nan),
    # as in the MX format and the GPU kernels (``csrc/hsquant.hip`` fp8_pack4)
    finite = torch.isfinite(blocks)
    amax = torch.where(finite, blocks.abs(), torch.zeros_like(blocks)).amax(dim=1)
    # tensor/tensor division (correctly rounded; a Python-scalar divisor is
    # lowered to a reciprocal multiply by torch and differs by 1 ulp)
    # floored at the smallest normal float32 (module docstring, "Scale rule")
    scale = torch.where(amax > 0,
                        torch.maximum(amax / torch.full_like(amax, FP8_MAX),
                                      torch.full_like(amax, FP8_MIN_SCALE)),
                        torch.ones_like(amax))
    # one reciprocal per block, one multiply per element (the kernels' rule)
    inv = torch.ones_like(scale) / scale
    q = torch.where(finite, (blocks * inv[:, None]).clamp(-FP8_MAX, FP8_MAX),
                    blocks).to(torch.float8_e4m3fn)
    return q, scale


def quantize_reference(x: torch.Tensor, block: int):
    """Plain blockwise reference: returns (q[n] e4m3fn, scale[nblocks])."""
    flat = x.detach().reshape(-1).float()
    n = flat.numel()
    nblocks = (n + block - 1) // block
    padded = torch.zeros(nblocks * block, dtype=torch.float32, device=flat.device)
    padded[:n] = flat
    q, scale = _scale_and_quant(padded.view(nblocks, block))
    return q.reshape(-1)[:n], scale


def dequantize_reference(q: torch.Tensor, scale: torch.Tensor, block: int,
                         dtype: torch.dtype) -> torch.Tensor:
    n = q.numel()
    nblocks = scale.numel()
    padded = torch.zeros(nblocks * block, dtype=torch.float32, device=q.device)
    padded[:n] = q.float()
    return (padded.view(nblocks, block) * scale[:, None]).reshape(-1)[:n].to(dtype)


def pow2(e: torch.Tensor) -> torch.Tensor:
    """Exact float32 ``2**e`` for integer ``e`` in [-149, 127] (bit-built:
    normal exponents, or the subnormal bit below -126)."""
    e = e.to(torch.int32)
    normal = (e + 127).clamp(min=1) << 23
    sub = torch.ones_like(e) << (e + 149).clamp(0, 22)
    return torch.where(e >= -126, normal, sub).view(torch.float32)


def mx_exponents(amax: torch.Tensor) -> torch.Tensor:
    """Per-block ``k``: smallest exponent with ``amax <= 448 * 2^k``."""
    m, e = torch.frexp(amax)
    k = torch.where(m <= 0.875, e - 9, e - 8)
    ok = (amax > 0) & torch.isfinite(amax)
    return torch.where(ok, k, torch.zeros_like(k)).clamp(-127, 127).to(torch.int32)


def mx_quantize_reference(x: torch.Tensor):
    """MX reference: returns (q[n] e4m3fn, scale bytes[nblocks] uint8)."""
    flat = x.detach().reshape(-1).float()
    n = flat.numel()
    nblocks = (n + MX_BLOCK - 1) // MX_BLOCK
    blocks = torch.zeros(nblocks * MX_BLOCK, dtype=torch.float32, device=flat.device)
    blocks[:n] = flat
    blocks = blocks.view(nblocks, MX_BLOCK)
    a = blocks.abs()
    amax = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).amax(dim=1)  # finite only
    k = mx_exponents(amax)
    q = (blocks * pow2(-k)[:, None]).to(torch.float8_e4m3fn)
    return q.reshape(-1)[:n], (k + 127).to(torch.uint8)


def mx_dequantize_reference(q: torch.Tensor, sbytes: torch.Tensor,
                            dtype: torch.dtype) -> torch.Tensor:
    n = q.numel()
    nblocks = sbytes.numel()
    padded = torch.zeros(nblocks * MX_BLOCK, dtype=torch.float32, device=q.device)
    padded[:n] = q.float()
    k = sbytes.to(torch.int32) - 127
    return (padded.view(nblocks, MX_BLOCK) * pow2(k)[:, None]).reshape(-1)[:n].to(dtype)


E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
E8M0_NAN = 0xFF
_QUIET_NAN_BITS = {torch.bfloat16: (torch.int16, 0x7FC0), torch.float16: (torch.int16, 0x7E00),
                   torch.float32: (torch.int32, 0x7FC00000),
                   torch.float64: (torch.int64, 0x7FF8 << 48)}


def mxfp4_exponents(amax: torch.Tensor) -> torch.Tensor:
    """Per-block ``k``: smallest exponent with ``amax <= 6 * 2^k``."""
    m, e = torch.frexp(amax)
    k = torch.where(m <= 0.75, e - 3, e - 2)
    ok = (amax > 0) & torch.isfinite(amax)
    return torch.where(ok, k, torch.zeros_like(k)).clamp(-127, 127).to(torch.int32)


def _e2m1_index(y: torch.Tensor) -> torch.Tensor:
    """Index of the nearest ``E2M1_VALUES`` magnitude to ``y >= 0`` (uint8): the
    comparisons are with the midpoints of the grid; a tie goes to the even
    index."""
    return ((y > 0.25).to(torch.uint8) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5)
            + (y >= 3.5) + (y > 5.0))


def mxfp4_quantize_reference(x: torch.Tensor):
    """MXFP4 reference: returns (payload[round_up(ceil(n / 2), 16)] uint8 with
    element 2i in the low nibble of byte i and zeros from element n on, scale
    bytes[nblocks] uint8).  The rules are in the module docstring."""
    flat = x.detach().reshape(-1).float()
    n = flat.numel()
    nblocks = (n + MX_BLOCK - 1) // MX_BLOCK
    blocks = torch.zeros(nblocks * MX_BLOCK, dtype=torch.float32, device=flat.device)
    blocks[:n] = flat
    blocks = blocks.view(nblocks, MX_BLOCK)
    a = blocks.abs()
    amax = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).amax(dim=1)  # finite only
    k = mxfp4_exponents(amax)
    y = a * pow2(-k)[:, None]  # exact, at most 6 (inf stays inf: index 7)
    codes = _e2m1_index(y) | (torch.signbit(blocks).to(torch.uint8) << 3)
    has_nan = torch.isnan(blocks).any(dim=1)
    codes = torch.where(has_nan[:, None], torch.zeros_like(codes), codes).reshape(-1)
    sbytes = torch.where(has_nan, torch.full_like(k, E8M0_NAN), k + 127).to(torch.uint8)
    payload = torch.zeros(mxfp4_payload_bytes(n), dtype=torch.uint8, device=flat.device)
    payload[: (n + 1) // 2] = (codes[0::2] | (codes[1::2] << 4))[: (n + 1) // 2]
    return payload, sbytes


def _e2m1_decode(payload: torch.Tensor, n: int, nblocks: int, block: int) -> torch.Tensor:
    """The fp32 values of the nibbles of elements ``[0, n)`` as ``[nblocks,
    block]`` (zeros past ``n``)."""
    p = payload[: (n + 1) // 2]
    codes = torch.zeros(nblocks * block, dtype=torch.uint8, device=p.device)
    codes[0: 2 * p.numel(): 2] = p & 0xF
    codes[1: 2 * p.numel(): 2] = p >> 4
    mag = torch.tensor(E2M1_VALUES, dtype=torch.float32, device=p.device)[(codes & 7).long()]
    return torch.where((codes & 8) != 0, -mag, mag).view(nblocks, block)


def mxfp4_dequantize_reference(payload: torch.Tensor, sbytes: torch.Tensor, n: int,
                               dtype: torch.dtype) -> torch.Tensor:
    """``q * 2^k`` exact in fp32, then one rounding to ``dtype``; a block with
    the NaN scale byte restores as positive quiet NaNs."""
    nblocks = sbytes.numel()
    q = _e2m1_decode(payload, n, nblocks, MX_BLOCK)
    is_nan = sbytes == E8M0_NAN
    k = torch.where(is_nan, torch.zeros_like(sbytes), sbytes).to(torch.int32) - 127
    out = (q * pow2(k)[:, None]).reshape(-1)[:n].to(dtype)
    # the NaN by its bits: a cast of NaN picks its own sign and payload
    view, bits = _QUIET_NAN_BITS[dtype]
    out.view(view)[is_nan.repeat_interleave(MX_BLOCK)[:n]] = bits
    return out


NVFP4_TOP = 2688.0  # 448 * 6: the largest e4m3 scale times the largest e2m1 magnitude
NVFP4_MIN_TS = 2.0 ** -117  # floor of the tensor scale: ts * 2^-9 >= 2^-126
E4M3_NAN = 0x7F


def nvfp4_tensor_scale(amax: torch.Tensor) -> torch.Tensor:
    """``ts = max(A / 2688, 2^-117)`` in fp32 (tensor / tensor: correctly
    rounded, see ``_scale_and_quant``)."""
    return torch.maximum(amax / torch.full_like(amax, NVFP4_TOP),
                         torch.full_like(amax, NVFP4_MIN_TS))


def nvfp4_quantize_reference(x: torch.Tensor):
    """Two-level-scaled FP4 reference: returns (payload[round_up(ceil(n / 2),
    16)] uint8 in the ``mxfp4`` nibble order, scale bytes[ceil(n / 16)] uint8
    (e4m3fn), amax[1] float32).  The rules are in the module docstring; every
    line below is one fp32 operation of them."""
    flat = x.detach().reshape(-1).float()
    n = flat.numel()
    nblocks = (n + NV_BLOCK - 1) // NV_BLOCK
    blocks = torch.zeros(nblocks * NV_BLOCK, dtype=torch.float32, device=flat.device)
    blocks[:n] = flat
    blocks = blocks.view(nblocks, NV_BLOCK)
    a = blocks.abs()
    finite_a = torch.where(torch.isfinite(a), a, torch.zeros_like(a))
    amax = finite_a.amax().reshape(1)
    ts = nvfp4_tensor_scale(amax)
    quot = finite_a.amax(dim=1) / (torch.full_like(ts, 6.0) * ts)
    s8 = torch.minimum(quot, torch.full_like(quot, FP8_MAX)).to(torch.float8_e4m3fn)
    d = s8.float() * ts
    inv = torch.ones_like(d) / d  # inf where s8 == 0
    y = (a * inv[:, None]).clamp(max=6.0)  # on magnitudes: rounding is symmetric; inf -> 6
    idx = torch.where((d > 0)[:, None], _e2m1_index(y), torch.zeros_like(y, dtype=torch.uint8))
    codes = idx | (torch.signbit(blocks).to(torch.uint8) << 3)
    has_nan = torch.isnan(blocks).any(dim=1)
    codes = torch.where(has_nan[:, None], torch.zeros_like(codes), codes).reshape(-1)
    sbytes = torch.where(has_nan, torch.full_like(has_nan, E4M3_NAN, dtype=torch.uint8),
                         s8.view(torch.uint8))
    payload = torch.zeros(nvfp4_payload_bytes(n), dtype=torch.uint8, device=flat.device)
    payload[: (n + 1) // 2] = (codes[0::2] | (codes[1::2] << 4))[: (n + 1) // 2]
    return payload, sbytes, amax


def nvfp4_dequantize_reference(payload: torch.Tensor, sbytes: torch.Tensor, amax: torch.Tensor,
                               n: int, dtype: torch.dtype) -> torch.Tensor:
    """``q * d`` with ``d = f32(s8) * ts``, two fp32 products, then one rounding
    to ``dtype``; a block with the e4m3fn NaN byte restores as positive quiet
    NaNs."""
    nblocks = sbytes.numel()
    q = _e2m1_decode(payload, n, nblocks, NV_BLOCK)
    is_nan = (sbytes & 0x7F) == E4M3_NAN
    s8 = torch.where(is_nan, torch.zeros_like(sbytes), sbytes).view(torch.float8_e4m3fn)
    d = s8.float() * nvfp4_tensor_scale(amax.reshape(1).float())
    out = (q * d[:, None]).reshape(-1)[:n].to(dtype)
    view, bits = _QUIET_NAN_BITS[dtype]
    out.view(view)[is_nan.repeat_interleave(NV_BLOCK)[:n]] = bits
    return out


E2M3_VALUES = tuple(i * 0.125 for i in range(16)) + tuple(2.0 + i * 0.25 for i in range(8)) \
    + tuple(4.0 + i * 0.5 for i in range(8))


def mxfp6_exponents(amax: torch.Tensor) -> torch.Tensor:
    """Per-block ``k``: smallest exponent with ``amax <= 7.5 * 2^k``."""
    m, e = torch.frexp(amax)
    k = torch.where(m <= 0.9375, e - 3, e - 2)
    ok = (amax > 0) & torch.isfinite(amax)
    return torch.where(ok, k, torch.zeros_like(k)).clamp(-127, 127).to(torch.int32)


def mxfp6_quantize_reference(x: torch.Tensor):
    """MXFP6 reference: returns (payload[round_up(24 * nblocks, 16)] uint8 with
    element j of block b in bits [6 j, 6 j + 6) of bytes [24 b, 24 b + 24) and
    zeros from element n on, scale bytes[nblocks] uint8).  The rules are in the
    module docstring."""
    flat = x.detach().reshape(-1).float()
    n = flat.numel()
    nblocks = (n + MX_BLOCK - 1) // MX_BLOCK
    blocks = torch.zeros(nblocks * MX_BLOCK, dtype=torch.float32, device=flat.device)
    blocks[:n] = flat
    blocks = blocks.view(nblocks, MX_BLOCK)
    a = blocks.abs()
    amax = torch.where(torch.isfinite(a), a, torch.zeros_like(a)).amax(dim=1)  # finite only
    k = mxfp6_exponents(amax)
    y = a * pow2(-k)[:, None]  # exact, at most 7.5 (inf stays inf: index 31)
    # the grid's step is 1/8 below 2, 1/4 below 4 and 1/2 from there on; every
    # segment starts at an even index, so torch.round's ties-to-even on the
    # quotient (exact in fp32) is ties to the even index
    idx = torch.where(y < 2, (y * 8).round(),
                      torch.where(y < 4, 16 + ((y - 2) * 4).round(), 24 + ((y - 4) * 2).round()))
    codes = idx.clamp(max=31).to(torch.int32) | (torch.signbit(blocks).to(torch.int32) << 5)
    has_nan = torch.isnan(blocks).any(dim=1)
    codes = torch.where(has_nan[:, None], torch.zeros_like(codes), codes).view(-1, 4)
    sbytes = torch.where(has_nan, torch.full_like(k, E8M0_NAN), k + 127).to(torch.uint8)
    # 4 codes -> 24 bits -> 3 bytes, little endian
    w = codes[:, 0] | (codes[:, 1] << 6) | (codes[:, 2] << 12) | (codes[:, 3] << 18)
    packed = torch.stack([w & 0xFF, (w >> 8) & 0xFF, w >> 16], dim=1).to(torch.uint8)
    payload = torch.zeros(mxfp6_payload_bytes(n), dtype=torch.uint8, device=flat.device)
    payload[: 24 * nblocks] = packed.reshape(-1)
    return payload, sbytes


def mxfp6_dequantize_reference(payload: torch.Tensor, sbytes: torch.Tensor, n: int,
                               dtype: torch.dtype) -> torch.Tensor:
    """``q * 2^k`` exact in fp32, then one rounding to ``dtype``; a block with
    the NaN scale byte restores as positive quiet NaNs."""
    nblocks = sbytes.numel()
    b = payload[: 24 * nblocks].to(torch.int32).view(-1, 3)
    w = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
    codes = torch.stack([(w >> s) & 63 for s in (0, 6, 12, 18)], dim=1).reshape(-1)
    mag = torch.tensor(E2M3_VALUES, dtype=torch.float32, device=b.device)[(codes & 31).long()]
    q = torch.where((codes & 32) != 0, -mag, mag).view(nblocks, MX_BLOCK)
    is_nan = sbytes == E8M0_NAN
    k = torch.where(is_nan, torch.zeros_like(sbytes), sbytes).to(torch.int32) - 127
    out = (q * pow2(k)[:, None]).reshape(-1)[:n].to(dtype)
    view, bits = _QUIET_NAN_BITS[dtype]
    out.view(view)[is_nan.repeat_interleave(MX_BLOCK)[:n]] = bits
    return out


# ---------------------------------------------------------------------------
# error-budgeted choice of a format (``HIPSNAPSHOT_FP8_FORMAT=auto``)
# ---------------------------------------------------------------------------

# the candidates by size: (knob value, bits per element)
AUTO_FORMATS = (("mxfp4", 4.25), ("nvfp4", 4.5), ("mxfp6", 6.25), ("mx", 8.25))


def _restore_f32(flat: torch.Tensor, fmt: str) -> torch.Tensor:
    n = flat.numel()
    if fmt == "mxfp4":
        return mxfp4_dequantize_reference(*mxfp4_quantize_reference(flat), n, torch.float32)
    if fmt == "nvfp4":
        payload, sbytes, amax = nvfp4_quantize_reference(flat)
        return nvfp4_dequantize_reference(payload, sbytes, amax, n, torch.float32)
    if fmt == "mxfp6":
        return mxfp6_dequantize_reference(*mxfp6_quantize_reference(flat), n, torch.float32)
    if fmt == "mx":
        return mx_dequantize_reference(*mx_quantize_reference(flat), torch.float32)
    raise ValueError(f"{fmt!r} is not a candidate of the format probe")


def _candidates(candidates) -> tuple:
    names = tuple(name for name, _ in AUTO_FORMATS)
    if candidates is None:
        return names
    unknown = [c for c in candidates if c not in names]
    if unknown:
        raise ValueError(f"not candidates of the format probe: {unknown}")
    return tuple(name for name in names if name in candidates)


def _report(n: int, n_finite: int, sumsq: float, per_format: Dict[str, Any]) -> Dict[str, Any]:
    for f in per_format.values():
        f["rel"] = (f["err2"] / sumsq) ** 0.5 if sumsq > 0 else 0.0
    return {"n": n, "n_finite": n_finite, "sumsq": sumsq, "formats": per_format}


def format_errors_reference(x: torch.Tensor, candidates=None) -> Dict[str, Any]:
    """What each candidate format would lose on ``x`` (bf16, f16 or f32), from
    the references above with the differences and sums in float64.  With
    ``r_F`` the restore of the flat ``x`` under format ``F`` into fp32
    (``*_quantize_reference`` then ``*_dequantize_reference(..., float32)``)::

        {"n": n, "n_finite": ..., "sumsq": sum of x_i^2 over the finite x_i,
         "formats": {F: {"err2": sum of (x_i - r_F,i)^2 over the i where x_i and
                                 r_F,i are both finite,
                         "spoiled": number of i where x_i is finite and r_F,i is
                                    not (the finite neighbours of a NaN in a NaN
                                    block; the fp32-overflow edge of a code that
                                    rounds up),
                         "rel": sqrt(err2 / sumsq), 0 when sumsq == 0}}}

    An inf in ``x`` takes no part in any sum.  ``hs_quant_probe``
    (``csrc/hsquant.hip``) computes the same numbers in one read of a tensor in
    HBM; ``format_errors`` dispatches between the two."""
    flat = x.detach().reshape(-1)
    xd = flat.double()
    finite = torch.isfinite(xd)
    sumsq = float((torch.where(finite, xd, torch.zeros_like(xd)) ** 2).sum())
    per_format = {}
    for fmt in _candidates(candidates):
        r = _restore_f32(flat, fmt).double()
        both = finite & torch.isfinite(r)
        err = torch.where(both, xd - r, torch.zeros_like(xd))
        per_format[fmt] = {"err2": float((err ** 2).sum()),
                           "spoiled": int((finite & ~torch.isfinite(r)).sum())}
    return _report(flat.numel(), int(finite.sum()), sumsq, per_format)


def format_errors(t: torch.Tensor, candidates=None) -> Dict[str, Any]:
    """``format_errors_reference``'s report of ``t``: by ``hs_quant_probe`` for a
    tensor on the GPU (one read, on the current stream, then one host wait for
    88 bytes), by the reference for a host tensor.  The GPU report is a
    function of the tensor's bytes: the same on every rank and in every run."""
    names = _candidates(candidates)
    if not t.is_cuda:
        return format_errors_reference(t, names)
    from . import native

    src = t.detach()
    src = src if src.is_contiguous() else src.contiguous()
    mask = sum(1 << native.PROBE_FORMATS.index(name) for name in names)
    out = native.quant_probe_buffer(t.device)
    native.quant_probe(t.device.index or 0, src, mask, out,
                       int(torch.cuda.current_stream(t.device).cuda_stream))
    words = out[: native.PROBE_REPORT_WORDS].cpu()  # waits for the probe
    sums, counts = words[:5].view(torch.float64).tolist(), words[5:10].tolist()
    per_format = {name: {"err2": sums[1 + i], "spoiled": counts[1 + i]}
                  for i, name in enumerate(native.PROBE_FORMATS) if name in names}
    return _report(src.numel(), counts[0], sums[0], per_format)


def choose_format(report: Dict[str, Any], max_error: float, candidates=None):
    """The candidate with the fewest bits per element that spoils nothing
    (``spoiled == 0``) and whose ``rel`` is at most ``max_error``; ``None`` if
    there is none.  ``report`` is a ``format_errors`` result.

    The measure is a tensor-wide L2 error.  What is small beside the tensor's
    norm hardly shows in it: the blocks that ``nvfp4`` flushes to zero because
    they lie 2^22 below the tensor's amax -- whole rows of Adam second moments
    -- contribute only their own, tiny, squares.  That is why the candidate
    list is a knob (``knobs.quant_auto_formats``): leave ``nvfp4`` out for such
    states."""
    for name in _candidates(candidates):
        f = report["formats"].get(name)
        if f is not None and f["spoiled"] == 0 and f["rel"] <= max_error:
            return name
    return None


def auto_format(t: torch.Tensor):
    """``(format, measured rel)`` of ``t`` under the ``auto`` knobs, ``(None,
    None)`` when no candidate is within the budget."""
    from .. import knobs

    names = knobs.quant_auto_formats()
    report = format_errors(t, names)
    fmt = choose_format(report, knobs.quant_max_error(), names)
    return (fmt, report["formats"][fmt]["rel"]) if fmt is not None else (None, None)


def hadamard_matrix(n: int = GROUP, device=None) -> torch.Tensor:
    idx = torch.arange(n, device=device)
    bits = (idx[:, None] & idx[None, :])
    parity = torch.zeros_like(bits)
    for b in range(n.bit_length()):
        parity ^= (bits >> b) & 1
    return 1.0 - 2.0 * parity.float()


# k order of the GPU kernels' MFMA chain: step t contracts k = t (lanes of
# half 0) then k = 16 + t (half 1), the layout that lets each lane load its
# 16 elements of a row with 16-B vector loads (hs_fp8_hadamard_*)
HADAMARD_K_ORDER = [k for t in range(GROUP // 2) for k in (t, GROUP // 2 + t)]


def _rotate_sequential(rows: torch.Tensor) -> torch.Tensor:
    """rows[R, 32] @ H with a k-ordered fp32 FMA chain (= MFMA f32 semantics,
    in ``HADAMARD_K_ORDER``)."""
    h = hadamard_matrix(GROUP, rows.device)
    acc = torch.zeros_like(rows)
    for k in HADAMARD_K_ORDER:
        acc = acc + rows[:, k:k + 1] * h[k][None, :]  # x * +-1 is exact: one rounding
    return acc


def mxfp4_hadamard_quantize_reference(x: torch.Tensor):
    """Rotated MXFP4 reference: returns (payload[n_pad / 2] uint8, scale
    bytes[n_pad / 32] uint8), n_pad = round_up(n, 32).  Each group of 32 is
    rotated (fp32 sums in ``HADAMARD_K_ORDER``) and is one MX block under the
    ``mxfp4`` rules; a group with a non-finite rotated value stores ``0xFF`` and
    zeros (module docstring)."""
    flat = x.detach().reshape(-1).float()
    n = flat.numel()
    rows = torch.zeros(_round_up(n, GROUP) // GROUP, GROUP, dtype=torch.float32,
                       device=flat.device)
    rows.view(-1)[:n] = flat
    y = _rotate_sequential(rows)
    bad = ~torch.isfinite(y).all(dim=1)
    y[bad] = float("nan")  # the mxfp4 rule for a block with a NaN: 0xFF and zeros
    return mxfp4_quantize_reference(y)


def mxfp4_hadamard_dequantize_reference(payload: torch.Tensor, sbytes: torch.Tensor, n: int,
                                        dtype: torch.dtype) -> torch.Tensor:
    """``x = (Q H) * 2^(k - 5)``: the row sums of e2m1 values are multiples of
    0.5 of magnitude <= 192 (float64 matmul, exact in fp32), one fp32 product
    with the power of two, one rounding to ``dtype``; a group with the NaN
    scale byte restores as positive quiet NaNs."""
    nblocks = sbytes.numel()
    is_nan = sbytes == E8M0_NAN
    ones = torch.full_like(sbytes, 127)  # decode the codes alone: scale 2^0
    q = mxfp4_dequantize_reference(payload, ones, nblocks * GROUP, torch.float32)
    z = (q.view(nblocks, GROUP).double() @ hadamard_matrix(GROUP, q.device).double()).float()
    k = torch.where(is_nan, ones, sbytes).to(torch.int32) - 127 - 5
    out = (z * pow2(k)[:, None]).reshape(-1)[:n].to(dtype)
    view, bits = _QUIET_NAN_BITS[dtype]
    out.view(view)[is_nan.repeat_interleave(GROUP)[:n]] = bits
    return out


def hadamard_quantize_reference(x: torch.Tensor, block: int = 128):
    """Returns (q[n_pad] e4m3fn, scale[nblocks]) with n_pad = round_up(n, 32)."""
    flat = x.detach().reshape(-1).float()
    n = flat.numel()
    n_pad = _round_up(n, GROUP)
    nblocks = (n_pad + block - 1) // block
    rows = torch.zeros(nblocks * block // GROUP, GROUP, dtype=torch.float32, device=flat.device)
    rows.view(-1)[:n] = flat
    y = _rotate_sequential(rows).reshape(nblocks, block)
    q, scale = _scale_and_quant(y)
    return q.reshape(-1)[:n_pad], scale


def hadamard_dequantize_reference(q: torch.Tensor, scale: torch.Tensor, n: int,
                                  dtype: torch.dtype, block: int = 128) -> torch.Tensor:
    """x = (Q H) * (s / 32): the row sums of e4m3 codes are exact (multiples of
    2^-9 below 2^14, computed in float64 and exact in fp32), then ONE fp32
    rounding by the block scale -- the same arithmetic as the GPU kernel
    (``hs_fp8_hadamard_dequant8``, bf16 MFMA on the widened codes), so both
    are bit-identical."""
    n_pad = q.numel()
    rows = q.float().reshape(-1, GROUP).double()
    h = hadamard_matrix(GROUP, rows.device).double()
    z = (rows @ h).float()  # exact
    s = (scale.float() * (1.0 / GROUP)).repeat_interleave(block // GROUP)[:z.shape[0]]
    x = z * s[:, None]
    return x.reshape(-1)[:n].to(dtype)


# ---------------------------------------------------------------------------
# staging (save) and decoding (restore)
# ---------------------------------------------------------------------------

def stage_fp8(t: torch.Tensor, entry: TensorEntry, producer: int) -> StagedBuffer:
    """Quantize ``t`` and return the blob bytes in host memory."""
    info = entry.quant
    rot = info.get("rotation", "none")
    payload, nblocks, total = info["payload_bytes"], info["nblocks"], info["total_bytes"]
    if is_mx(info) or is_mxfp4(info) or is_mxfp6(info) or is_nvfp4(info):
        return _stage_mx(t, info, producer)
    if t.is_cuda:
        from ..engine import staging
        from . import native

        dev = staging.device_of(t)
        src = t if t.is_contiguous() else t.contiguous()
        blob = torch.zeros(total, dtype=torch.uint8, device=t.device)
        stream = torch.cuda.current_stream(t.device)
        if producer is not None and producer != stream.cuda_stream:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.default_stream(t.device) if producer == 0
                      else torch.cuda.ExternalStream(producer))
            stream.wait_event(ev)
        scales = blob[payload:].view(torch.float32)
        if rot == "hadamard32":
            native.fp8_hadamard_quantize(dev, src, blob[:payload], scales,
                                         int(stream.cuda_stream))
        else:
            native.fp8_quantize(dev, src, blob[:payload], scales, info["vpt"],
                                int(stream.cuda_stream))
        return staging.d2h_tensor(blob, int(stream.cuda_stream))
    if rot == "hadamard32":
        q, scale = hadamard_quantize_reference(t, info["block"])
    else:
        q, scale = quantize_reference(t, info["block"])
    blob = torch.zeros(total, dtype=torch.uint8)
    blob[: q.numel()] = q.view(torch.uint8)
    blob[payload:] = scale.view(torch.uint8)
    from ..format.serialization import contiguous_cpu_bytes_view

    return StagedBuffer(contiguous_cpu_bytes_view(blob), keepalive=blob)


def _stage_mx(t: torch.Tensor, info: Dict[str, Any], producer: int) -> StagedBuffer:
    """The E8M0 layouts: MX fp8, MXFP6, MXFP4 and rotated MXFP4 (same blob
    shape, other kernel), and the two-level-scaled FP4 one, whose scale bytes
    are padded to a multiple of 4 and followed by the fp32 amax."""
    payload, total = info["payload_bytes"], info["total_bytes"]
    nv = is_nvfp4(info)
    fp4h = is_mxfp4_hadamard(info)
    fp4 = is_mxfp4(info) and not fp4h
    fp6 = is_mxfp6(info)
    if t.is_cuda:
        from ..engine import staging
        from . import native

        dev = staging.device_of(t)
        stream = torch.cuda.current_stream(t.device)
        if producer is not None and producer != stream.cuda_stream:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.default_stream(t.device) if producer == 0
                      else torch.cuda.ExternalStream(producer))
            stream.wait_event(ev)
        src = t if t.is_contiguous() else t.contiguous()
        blob = torch.empty(total, dtype=torch.uint8, device=t.device)  # kernel writes all of it
        if nv:
            native.nvfp4_quantize(dev, src, blob[:payload], blob[payload: total - 4],
                                  blob[total - 4:], int(stream.cuda_stream))
            return staging.d2h_tensor(blob, int(stream.cuda_stream))
        quantize = (native.mxfp4_hadamard_quantize if fp4h else
                    native.mxfp4_quantize if fp4 else
                    native.mxfp6_quantize if fp6 else native.mx8_quantize)
        quantize(dev, src, blob[:payload], blob[payload:], int(stream.cuda_stream))
        return staging.d2h_tensor(blob, int(stream.cuda_stream))
    if nv:
        q, sbytes, amax = nvfp4_quantize_reference(t)
    else:
        q, sbytes = (mxfp4_hadamard_quantize_reference(t) if fp4h else
                     mxfp4_quantize_reference(t) if fp4 else
                     mxfp6_quantize_reference(t) if fp6 else mx_quantize_reference(t))
    blob = torch.zeros(total, dtype=torch.uint8)
    blob[: q.numel()] = q.view(torch.uint8)
    blob[payload: payload + sbytes.numel()] = sbytes
    if nv:
        blob[total - 4:] = amax.view(torch.uint8)
    from ..format.serialization import contiguous_cpu_bytes_view

    return StagedBuffer(contiguous_cpu_bytes_view(blob), keepalive=blob)


def _split_blob(raw: torch.Tensor, info: Dict[str, Any], n: int):
    rot = info.get("rotation", "none")
    nq = _round_up(n, GROUP) if rot == "hadamard32" else n
    q = raw[:nq]
    scale = raw[info["payload_bytes"]: info["payload_bytes"] + 4 * info["nblocks"]].view(
        torch.float32)
    return rot, q, scale


def dequantize_host_fp8(buf, entry: TensorEntry) -> torch.Tensor:
    """CPU decode of an fp8 blob into a tensor of the entry's original dtype."""
    info = entry.quant
    n = 1
    for s in entry.shape:
        n *= int(s)
    mv = memoryview(buf.view if isinstance(buf, StagedBuffer) else buf).cast("B")
    raw = torch.frombuffer(bytearray(mv[: info["total_bytes"]]), dtype=torch.uint8)
    dtype = string_to_dtype(entry.dtype)
    if is_nvfp4(info):
        p, total = info["payload_bytes"], info["total_bytes"]
        out = nvfp4_dequantize_reference(raw[:p], raw[p: p + info["nblocks"]],
                                         raw[total - 4: total].view(torch.float32), n, dtype)
        return out.view(list(entry.shape))
    if is_mxfp6(info):
        p = info["payload_bytes"]
        out = mxfp6_dequantize_reference(raw[:p], raw[p: p + info["nblocks"]], n, dtype)
        return out.view(list(entry.shape))
    if is_mxfp4(info):
        p = info["payload_bytes"]
        decode = (mxfp4_hadamard_dequantize_reference if is_mxfp4_hadamard(info)
                  else mxfp4_dequantize_reference)
        out = decode(raw[:p], raw[p: p + info["nblocks"]], n, dtype)
        return out.view(list(entry.shape))
    if is_mx(info):
        p = info["payload_bytes"]
        out = mx_dequantize_reference(raw[:n].view(torch.float8_e4m3fn),
                                      raw[p: p + info["nblocks"]], dtype)
        return out.view(list(entry.shape))
    rot, q, scale = _split_blob(raw, info, n)
    if rot == "hadamard32":
        out = hadamard_dequantize_reference(q.view(torch.float8_e4m3fn), scale, n, dtype,
                                            info["block"])
    else:
        out = dequantize_reference(q.view(torch.float8_e4m3fn), scale, info["block"], dtype)
    return out.view(list(entry.shape))


def dequantize_device(blob_dev: torch.Tensor, entry: TensorEntry, dst: torch.Tensor) -> None:
    """GPU decode straight into a contiguous CUDA ``dst`` of the original dtype."""
    from . import native

    info = entry.quant
    n = dst.numel()
    stream = int(torch.cuda.current_stream(dst.device).cuda_stream)
    dev = dst.device.index or 0
    if is_nvfp4(info):
        p, total = info["payload_bytes"], info["total_bytes"]
        native.nvfp4_dequantize(dev, blob_dev[:p], blob_dev[p: p + info["nblocks"]],
                                blob_dev[total - 4: total], dst, stream)
        return
    if is_mxfp6(info):
        p = info["payload_bytes"]
        native.mxfp6_dequantize(dev, blob_dev[:p], blob_dev[p: p + info["nblocks"]], dst, stream)
        return
    if is_mxfp4(info):
        p = info["payload_bytes"]
        decode = (native.mxfp4_hadamard_dequantize if is_mxfp4_hadamard(info)
                  else native.mxfp4_dequantize)
        decode(dev, blob_dev[:p], blob_dev[p: p + info["nblocks"]], dst, stream)
        return
    if is_mx(info):
        p = info["payload_bytes"]
        native.mx8_dequantize(dev, blob_dev[:n], blob_dev[p: p + info["nblocks"]], dst, stream)
        return
    rot, q, scale = _split_blob(blob_dev, info, n)
    if rot == "hadamard32":
        native.fp8_hadamard_dequantize(dev, q, scale, dst, stream)
    else:
        native.fp8_dequantize(dev, q, scale, dst, info["vpt"], stream)


def gpu_region_decodable(info: Dict[str, Any]) -> bool:
    """Whether ``dequantize_regions`` can decode a blob of this ``quant`` dict
    region by region: the formats whose element ``i`` is decodable on its own
    (``mx``, ``mxfp4``, ``mxfp6``, ``nvfp4``: its code and its scale byte sit at
    offsets computed from ``i``).  The rotated formats (``hadamard32``,
    ``mxfp4_hadamard32``) need whole groups of 32 through the matrix cores, and
    the fp32-scale ``block`` layout was left on its kernels: those are restored
    whole by ``dequantize_device``, or on the host."""
    from . import native

    return bool(info) and info.get("format") in native.DEQUANT_FORMATS \
        and info.get("rotation", "none") == "none"


def _whole_piece(entry: TensorEntry, narrows) -> bool:
    return all(start == 0 and length == int(entry.shape[d]) for d, start, length in narrows or ())


def dequantize_regions(blob_dev: torch.Tensor, entry: TensorEntry, regions, stream: int):
    """GPU decode of boxes of a quantized blob in HBM into CUDA views, on
    ``stream`` (a handle), which is not synchronized here: the caller does
    that and holds the returned object (or None) until then.  ``regions``: list
    of ``(narrows or None, dst_view)``, ``narrows`` a list of ``(dim, start,
    length)`` on the entry's ``shape`` (the regions of
    ``staging.scatter_host_regions``); ``dst_view`` has the box's shape, any
    strides, and dtype bf16, f16 or f32 (it need not be the entry's: the decode
    is fp32, then one rounding).  A single region that is the whole piece into
    a contiguous view of the entry's dtype goes to the streaming kernels
    (``dequantize_device``), everything else to ``hs_dequant_regions`` in one
    launch; the entry must be ``gpu_region_decodable`` then."""
    from . import native

    info = entry.quant
    if len(regions) == 1:
        narrows, dst = regions[0]
        if (_whole_piece(entry, narrows) and dst.is_contiguous()
                and dst.dtype == string_to_dtype(entry.dtype)):
            st = (torch.cuda.ExternalStream(stream, device=dst.device) if stream
                  else torch.cuda.default_stream(dst.device))
            with torch.cuda.stream(st):
                dequantize_device(blob_dev, entry, dst)
            return None
    if not gpu_region_decodable(info):
        raise ValueError(f"quantized format {info.get('format')!r} (rotation "
                         f"{info.get('rotation')!r}) is not decodable by regions")
    p, total = info["payload_bytes"], info["total_bytes"]
    dev = regions[0][1].device.index or 0
    amax = blob_dev[total - 4: total] if is_nvfp4(info) else None
    return native.dequant_regions(dev, info["format"], blob_dev[:p],
                                  blob_dev[p: p + info["nblocks"]], amax, entry.shape, regions,
                                  stream, sync=False)
