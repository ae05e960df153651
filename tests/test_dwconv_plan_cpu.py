"""The depthwise-convolution host queries answer what tests/golden/dwconv_plans.json recorded
(scripts/record_dwconv_plans.py, run on the commit before the routing moved into DwPlan /
dw_plan() of csrc/dwconv.hip): BatchNorm statistics tiles, the paired-backward gate, the bf16
storage gate and the weight-gradient workspace, for the EfficientNet trunk's geometries, the GPU
tests' cases and the shapes at each gate's boundary, under the tuning keys that change a route.
Geometries outside the strip kernels' halo bound (not in the fixture: the bound is newer than
it) answer as the generic route does.  Host code only: no GPU call is made."""
import ctypes
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "dwconv_plans.json")) as _f:
    GOLD = json.load(_f)

_spec = importlib.util.spec_from_file_location(
    "record_dwconv_plans", os.path.join(ROOT, "scripts", "record_dwconv_plans.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

# (N, C, H, W, K, stride, (left, right, top, bottom)): a lane's window would start left of the
# staged row (pad_left 5 > the 4 halo columns), or end right of it (an output row of 20 from a
# 16-wide input: 5 columns of right pad); tests/test_nn_ops_gpu.py::test_depthwise runs both
HALO_LEFT = (2, 8, 16, 16, 3, 1, (5, 1, 1, 1))
HALO_RIGHT = (2, 8, 16, 16, 3, 1, (1, 5, 1, 1))


@pytest.fixture(scope="module")
def lib():
    from e2ep_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    return _lib.load()


def _cases(test_fn):
    """The `case` list of a parametrised test."""
    return [tuple(c) for m in test_fn.pytestmark if m.args[0] == "case" for c in m.args[1]]


def test_fixture_covers_the_recorders_lists():
    """The fixture holds every shape and setting the recorder lists, one row of every field
    each, and the recorder's copies of the GPU tests' case lists are those tests' lists (the
    halo cases aside)."""
    import test_nn_ops_gpu as t
    assert GOLD["fields"] == rec.FIELDS
    assert GOLD["shapes"] == rec.shapes()
    assert GOLD["settings"] == rec.settings()
    assert sum(s["name"].startswith("trunk") for s in GOLD["shapes"]) == 20
    for s in GOLD["settings"]:
        rows = GOLD["results"][s["name"]]
        assert len(rows) == len(GOLD["shapes"]) and all(len(r) == len(rec.FIELDS) for r in rows)
    halo = [HALO_LEFT, HALO_RIGHT]
    assert _cases(t.test_depthwise) == rec.TEST_DEPTHWISE + halo
    assert _cases(t.test_depthwise_bwd_pair_bitwise_equals_two_launches) == rec.TEST_BWD_PAIR


@pytest.mark.parametrize("setting", GOLD["settings"], ids=[s["name"] for s in GOLD["settings"]])
def test_host_queries_match_recorded(lib, setting):
    before = [lib.e2ep_tune(int(k), 0) for k in setting["tune"]]
    with rec.applied(lib, setting):
        got = [rec.query(lib, sh["dims"]) for sh in GOLD["shapes"]]
    after = [lib.e2ep_tune(int(k), 0) for k in setting["tune"]]
    assert after == before, "setting not restored"
    want = GOLD["results"][setting["name"]]
    bad = [(sh["name"], f, w, g) for sh, wr, gr in zip(GOLD["shapes"], want, got)
           for f, w, g in zip(rec.FIELDS, wr, gr) if w != g]
    assert not bad, f"{len(bad)} answers differ (shape, field, recorded, got): {bad[:8]}"


@pytest.mark.parametrize("setting", GOLD["settings"], ids=[s["name"] for s in GOLD["settings"]])
@pytest.mark.parametrize("case", [HALO_LEFT, HALO_RIGHT], ids=["left", "right"])
def test_outside_the_halo_bound_is_the_generic_route(lib, case, setting):
    """No statistics, no paired backward, no bf16 storage, and the generic weight gradient's
    slabs (min(ceil(1024 / C), N * P * Q / 2048) splits, at least one), whatever the tuning."""
    dims = rec.dims_of(case)
    N, C, _, _, K, P, Q = dims[:7]
    splits = max(1, min(-(-1024 // C), N * P * Q // 2048, 128))
    with rec.applied(lib, setting):
        got = rec.query(lib, dims)
    assert got == [0, 0, 0, C * splits * K * K * 4]


@pytest.mark.parametrize("pad", [(4, 2, 1, 1), (2, 4, 1, 1)], ids=["left", "right"])
def test_at_the_halo_bound_is_the_strip_route(lib, pad):
    """The same 16 -> 20 wide rows with the pad moved one column, so that the outermost window
    ends on the staged row's edge (pad_left 4; 4 columns of right pad): statistics are taken,
    one tile per sample and unit of 12 output rows."""
    dims = rec.dims_of((*HALO_LEFT[:6], pad))
    assert dims[5:7] == rec.dims_of(HALO_LEFT)[5:7] == [16, 20]
    assert lib.e2ep_dwconv_fwd_stats_tiles((ctypes.c_int * 10)(*dims)) == 2 * 2
