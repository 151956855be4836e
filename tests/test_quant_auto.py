"""``HIPSNAPSHOT_FP8_FORMAT=auto`` on the host: ``quant.choose_format`` over a
hand-written report, and takes of host tensors that record the format the CPU
reference's errors select (CPU)."""

import pytest
import torch

from hipsnapshot import Snapshot, StateDict, knobs
from hipsnapshot.engine import plan_cache
from hipsnapshot.ops import quant
from hipsnapshot.utils.test_utils import env

NAMES = {"mxfp4": "fp4_e2m1_mx", "nvfp4": "fp4_e2m1_nv", "mxfp6": "fp6_e2m3_mx",
         "mx": "fp8_e4m3fn_mx"}
REPORT = {"formats": {"mxfp4": {"spoiled": 0, "rel": 0.11}, "nvfp4": {"spoiled": 3, "rel": 0.02},
                      "mxfp6": {"spoiled": 0, "rel": 0.03}, "mx": {"spoiled": 0, "rel": 0.025}}}


def gaussian(n=4096 + 35, seed=88):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).bfloat16()


@pytest.mark.parametrize("budget, candidates, want", [
    (0.2, None, "mxfp4"),            # the smallest that qualifies
    (0.05, None, "mxfp6"),           # nvfp4 is within the budget but spoils 3 elements
    (0.03, None, "mxfp6"),           # rel == budget qualifies
    (0.01, None, None),              # none qualifies
    (0.2, ("mx", "mxfp6"), "mxfp6"),  # the list is honoured, in order of size
    (0.026, ("mxfp4", "mxfp6"), None)])
def test_choose_format(budget, candidates, want):
    assert quant.choose_format(REPORT, budget, candidates) == want


def test_knobs_from_the_format_value():
    with env(HIPSNAPSHOT_FP8_FORMAT="auto"):
        assert (knobs.fp8_format(), knobs.quant_max_error()) == ("auto", 0.03)
        assert knobs.quant_auto_formats() == ("mxfp4", "nvfp4", "mxfp6", "mx")
    with env(HIPSNAPSHOT_FP8_FORMAT="auto:0.05:mx,mxfp4"):
        assert (knobs.fp8_format(), knobs.quant_max_error()) == ("auto", 0.05)
        assert knobs.quant_auto_formats() == ("mxfp4", "mx")
    with knobs.override_knob("QUANT_MAX_ERROR", 0.2):
        assert knobs.quant_max_error() == 0.2 and knobs.fp8_format() == "mx"


@pytest.mark.parametrize("budget, fmt", [(0.10, "nvfp4"), (0.05, "mxfp6"), (0.01, None)])
def test_host_take_records_the_choice(tmp_path, budget, fmt):
    w = gaussian().view(27, 153)
    rels = {k: f["rel"] for k, f in quant.format_errors_reference(w)["formats"].items()}
    assert all(abs(budget - r) > 0.03 * r for r in rels.values()), rels
    with env(HIPSNAPSHOT_FP8_FORMAT=f"auto:{budget}"):
        Snapshot.take(str(tmp_path / "s"), {"sd": StateDict(w=w)}, quantize=["sd/*"])
    e = Snapshot(str(tmp_path / "s")).get_manifest()["0/sd/w"]
    if fmt is None:
        assert e.quant is None
        want = w
    else:
        assert (e.quant["format"], e.quant["selected"]) == (NAMES[fmt], "auto")
        assert e.quant["rel_l2"] == rels[fmt]
        with env(HIPSNAPSHOT_FP8_FORMAT=fmt):
            assert {k: v for k, v in e.quant.items() if k not in ("rel_l2", "selected")} \
                == quant.fp8_entry_quant_info(w)
        want = quant._restore_f32(w.reshape(-1), fmt).to(w.dtype).view(w.shape)
    out = torch.zeros_like(w)
    Snapshot(str(tmp_path / "s")).restore({"sd": StateDict(w=out)})
    assert torch.equal(out, want)


def test_choice_follows_contents_and_skips_the_plan_cache(tmp_path, monkeypatch):
    """The same resident tensor, Gaussian and then with a heavy tail: the second
    take measures again and records another format."""
    monkeypatch.setattr(plan_cache, "is_resident", lambda obj: isinstance(obj, torch.Tensor))
    plan_cache.clear()
    before = dict(plan_cache.stats)
    w, formats = gaussian(), []
    with env(HIPSNAPSHOT_FP8_FORMAT="auto:0.12"):
        for i in range(2):
            Snapshot.take(str(tmp_path / f"s{i}"), {"sd": StateDict(w=w)}, quantize=["sd/*"])
            formats.append(Snapshot(str(tmp_path / f"s{i}")).get_manifest()["0/sd/w"].quant["format"])
            w[::32] *= 9.0  # one outlier per block: mxfp4's other 31 values lose their grid
    assert formats == [NAMES["mxfp4"], NAMES["nvfp4"]]
    assert plan_cache.stats == before and not plan_cache._plans
