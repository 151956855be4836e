"""``hs_quant_probe`` through ``quant.format_errors`` against
``quant.format_errors_reference`` (float64 sums over the torch references), and
``HIPSNAPSHOT_FP8_FORMAT=auto`` takes of a device tensor.

Bound of the sums: a term is ``e = x - r`` rounded once to fp32 (2^-24
relative, twice that on its square), squared and added in f64, so the kernel
is within 3 * 2^-24 = 1.8e-7 of the reference for these sizes and within (32 +
3) * 2^-24 = 2.1e-6 for the scaled-domain variant the rule also allows; 4e-6
is that with a factor 2."""

import math

import pytest
import torch

from hipsnapshot import Snapshot, StateDict
from hipsnapshot.ops import native, quant
from hipsnapshot.utils.test_utils import env
from test_gpu_fp8_oracle import _to_gpu
from test_mxfp4 import SRC_DTYPES
from test_nvfp4 import KINDS, values

pytestmark = pytest.mark.gpu

REL = 4e-6
NAMES = {"mxfp4": "fp4_e2m1_mx", "nvfp4": "fp4_e2m1_nv", "mxfp6": "fp6_e2m3_mx",
         "mx": "fp8_e4m3fn_mx"}
# (wave chunks, elements more): partial block, block +-1, one chunk +-1, two chunks + 1,
# and one workgroup (4 waves) + 1: two rows for the second-stage sum
SIZES = [(0, 1), (0, 31), (0, 32), (0, 33), (1, -1), (1, 0), (1, 1), (2, 1), (4, 1)]


def _check(ctx, got, want):
    assert (got["n"], got["n_finite"]) == (want["n"], want["n_finite"]), ctx
    assert got["sumsq"] == pytest.approx(want["sumsq"], rel=REL, abs=0), ctx
    assert list(got["formats"]) == list(want["formats"]), ctx
    for name, w in want["formats"].items():
        g = got["formats"][name]
        print(ctx, name, g, w)
        assert g["spoiled"] == w["spoiled"], (ctx, name)
        assert g["err2"] == pytest.approx(w["err2"], rel=REL, abs=0), (ctx, name)


@pytest.mark.parametrize("chunks, more", SIZES)
@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_probe_vs_reference(gpu, dtype, chunks, more):
    n = chunks * native.quant_probe_workgroup_elems(dtype) // 4 + more
    for kind in KINDS:
        x = values(kind, n, dtype)
        _check(f"{dtype} n={n} {kind}", quant.format_errors(_to_gpu(x, gpu)),
               quant.format_errors_reference(x))


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_non_finite_floor_and_candidates(gpu, dtype):
    """A NaN spoils its block's finite neighbours in the three block-NaN formats
    and nothing in ``mx``; an inf spoils nothing and is in no sum; a block more
    than 2^23 below A restores as zeros under ``nvfp4`` and adds its own squares;
    a candidate list limits the report."""
    n = native.quant_probe_workgroup_elems(dtype) + 70
    x = values("randn", n, dtype).clone()
    x[100] = 48.0  # A
    x[512:528] = 48.0 * 2.0 ** -25
    for at, v in ((5, math.nan), (n - 3, math.nan), (33, math.inf), (200, -math.inf)):
        x[at] = v
    want = quant.format_errors_reference(x)
    f = want["formats"]
    assert want["n_finite"] == n - 4 and math.isfinite(want["sumsq"])
    assert f["mx"]["spoiled"] == 0 and f["nvfp4"]["spoiled"] == 15 + min(15, (n - 1) % 16)
    assert f["mxfp4"]["spoiled"] == f["mxfp6"]["spoiled"] == 31 + min(31, (n - 1) % 32)
    assert not quant._restore_f32(x, "nvfp4")[512:528].any()  # the floor: err2 has its squares
    _check(f"{dtype} non-finite", quant.format_errors(_to_gpu(x, gpu)), want)
    some = ("mxfp6", "mxfp4")
    _check(f"{dtype} two candidates", quant.format_errors(_to_gpu(x, gpu), some),
           quant.format_errors_reference(x, some))


@pytest.mark.parametrize("dtype", SRC_DTYPES, ids=str)
def test_repeatable_and_misaligned_view(gpu, dtype):
    """Two probes of one tensor give the same bits; a source one element off an
    aligned address takes the element path."""
    n = 3 * native.quant_probe_workgroup_elems(dtype) + 35
    x = values("peak", n, dtype)
    src = _to_gpu(x, gpu)
    first = quant.format_errors(src)
    assert quant.format_errors(src) == first
    _check(f"{dtype} src+1", quant.format_errors(_to_gpu(x, gpu, x.element_size())),
           quant.format_errors_reference(x))


BUDGETS = [(0.12, "mxfp4"), (0.10, "nvfp4"), (0.05, "mxfp6"), (0.027, "mx"), (0.01, None)]


@pytest.mark.parametrize("budget, fmt", BUDGETS)
def test_auto_take_gpu(gpu, tmp_path, budget, fmt):
    w = torch.randn(2 * 8192 + 5, generator=torch.Generator().manual_seed(90)).bfloat16()
    w = w.view(27, 607)
    rels = {k: f["rel"] for k, f in quant.format_errors_reference(w)["formats"].items()}
    assert all(abs(b - r) >= 0.03 * r for b, _ in BUDGETS for r in rels.values()), rels
    dev = w.to(gpu)
    with env(HIPSNAPSHOT_FP8_FORMAT=f"auto:{budget}"):
        Snapshot.take(str(tmp_path / "s"), {"sd": StateDict(w=dev)}, quantize=["sd/*"])
    e = Snapshot(str(tmp_path / "s")).get_manifest()["0/sd/w"]
    if fmt is None:
        assert e.quant is None
        ref = w
    else:
        assert (e.quant["format"], e.quant["selected"]) == (NAMES[fmt], "auto")
        assert e.quant["rel_l2"] == pytest.approx(rels[fmt], rel=REL)
        ref = quant._restore_f32(w.reshape(-1), fmt).to(w.dtype).view(w.shape)
    for out in (torch.zeros_like(dev), torch.zeros_like(w)):
        Snapshot(str(tmp_path / "s")).restore({"sd": StateDict(w=out)})
        assert torch.equal(out.cpu(), ref)
