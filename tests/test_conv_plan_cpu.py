"""The convolution host queries answer what tests/golden/conv_plans.json recorded (scripts/
record_conv_plans.py, run on the commit before the launch plans moved into ConvPlan / WgradPlan):
workspace sizes, BatchNorm statistics tiles, weight-gradient splits and the paired-backward gate,
for the train step's geometries and the shapes at each gate's boundary, under every precision
and the tuning keys that change a route.  Host code only: no GPU call is made."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "conv_plans.json")) as _f:
    GOLD = json.load(_f)

_spec = importlib.util.spec_from_file_location(
    "record_conv_plans", os.path.join(ROOT, "scripts", "record_conv_plans.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)


@pytest.fixture(scope="module")
def lib():
    from e2ep_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    return _lib.load()


def test_fixture_covers_the_recorders_lists():
    """The fixture holds every shape and setting the recorder lists (the 41 train-step
    geometries included), one row of every field each."""
    assert GOLD["fields"] == rec.FIELDS
    assert GOLD["shapes"] == rec.shapes()
    assert GOLD["settings"] == rec.settings()
    assert sum(s["name"].startswith("step") for s in GOLD["shapes"]) == 41
    for rows in rec.expand(GOLD).values():
        assert len(rows) == len(GOLD["shapes"]) and all(len(r) == len(rec.FIELDS) for r in rows)


@pytest.mark.parametrize("setting", GOLD["settings"], ids=[s["name"] for s in GOLD["settings"]])
def test_host_queries_match_recorded(lib, setting):
    before = (lib.e2ep_conv_precision(-1), lib.e2ep_conv_gemm_variant(-1),
              [lib.e2ep_tune(int(k), 0) for k in setting["tune"]])
    with rec.applied(lib, setting):
        got = [rec.query(lib, sh) for sh in GOLD["shapes"]]
    after = (lib.e2ep_conv_precision(-1), lib.e2ep_conv_gemm_variant(-1),
             [lib.e2ep_tune(int(k), 0) for k in setting["tune"]])
    assert after == before, "setting not restored"
    want = rec.expand(GOLD)[setting["name"]]
    bad = [(sh["name"], f, w, g) for sh, wr, gr in zip(GOLD["shapes"], want, got)
           for f, w, g in zip(rec.FIELDS, wr, gr) if w != g]
    assert not bad, f"{len(bad)} answers differ (shape, field, recorded, got): {bad[:8]}"
