"""The BatchNorm host queries answer what tests/golden/bn_plans.json recorded
(scripts/record_bn_plans.py, run on the commit before the routing moved into BnPlan / bn_plan()
of csrc/bn.hip): the split workspace, the forward and backward single-launch gates and the fused
MBConv middle's gate, for the model's shapes, the GPU tests' shapes and the shapes at each gate's
boundary, under the switches and tuning keys that change a route.  The fused middle's gate is
also derived by hand at the layout switches: it takes its layout from the BatchNorm kernels'
(csrc/bns_layout.h), whose summation order it repeats.  Host code only: no GPU call is made."""
import ctypes
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "bn_plans.json")) as _f:
    GOLD = json.load(_f)

_spec = importlib.util.spec_from_file_location(
    "record_bn_plans", os.path.join(ROOT, "scripts", "record_bn_plans.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

SETTING_IDS = [s["name"] for s in GOLD["settings"]]


@pytest.fixture(scope="module")
def lib():
    from e2ep_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    return _lib.load()


def _shapes(test_fn):
    """The `shape` list of a parametrised test."""
    return [tuple(c) for m in test_fn.pytestmark if m.args[0] == "shape" for c in m.args[1]]


def _state(lib):
    """Every switch a setting can move.  e2ep_bn_small_limits cannot be read back: a channel of
    2048 float4, the clamp, takes the single launch in both directions only at (2048, 2048)."""
    keys = (rec.KEY_SPLIT_TARGET, rec.KEY_SPLIT_MIN, rec.KEY_WIDE, rec.KEY_WIDE_LO, rec.KEY_MID)
    small = lib.e2ep_bn_small(-1)
    prev = lib.e2ep_bn_small(1)
    limits = (lib.e2ep_bn_fwd_split(32, 3, 16, 16), lib.e2ep_bn_bwd_split(32, 3, 16, 16))
    lib.e2ep_bn_small(prev)
    return [lib.e2ep_tune(k, 0) for k in keys], small, limits


def test_fixture_covers_the_recorders_lists():
    """The fixture holds every shape and setting the recorder lists, one row of every field
    each, and the recorder's copies of the GPU tests' shape lists are those tests' lists."""
    import test_bf16_store_gpu as tb
    import test_nn_ops_gpu as t
    assert GOLD["fields"] == rec.FIELDS
    assert GOLD["shapes"] == rec.shapes()
    assert GOLD["settings"] == rec.settings()
    assert sum(s["name"].startswith("model") for s in GOLD["shapes"]) == 2 * len(rec.model_shapes())
    for s in GOLD["settings"]:
        rows = GOLD["results"][s["name"]]
        assert len(rows) == len(GOLD["shapes"]) and all(len(r) == len(rec.FIELDS) for r in rows)
    assert _shapes(t.test_bn_act) == rec.TEST_BN_ACT
    assert _shapes(t.test_bn_drop_connect_fused) == rec.TEST_BN_DROP_CONNECT
    assert _shapes(tb.test_bn_bwd_bf16_io_bitwise) == rec.TEST_BN_BWD_BF16
    assert _shapes(t.test_bn_act_layouts) == rec.LAYOUT_BOUNDARIES
    assert [s[0] * s[2] * s[3] // 4 for s in rec.LAYOUT_BOUNDARIES] == [256, 257, 512, 513, 1024, 1025,
                                                                       2048, 2049]


@pytest.mark.parametrize("setting", GOLD["settings"], ids=SETTING_IDS)
def test_host_queries_match_recorded(lib, setting):
    before = _state(lib)
    assert before[1:] == (1, (0, 0)), "the library is not at its defaults"
    with rec.applied(lib, setting):
        got = [rec.query(lib, sh["shape"]) for sh in GOLD["shapes"]]
    assert _state(lib) == before, "setting not restored"
    want = GOLD["results"][setting["name"]]
    bad = [(sh["name"], f, w, g) for sh, wr, gr in zip(GOLD["shapes"], want, got)
           for f, w, g in zip(rec.FIELDS, wr, gr) if w != g]
    assert not bad, f"{len(bad)} answers differ (shape, field, recorded, got): {bad[:8]}"


# The fused middle runs a channel of N x 16 x 16 elements = 64 N float4 on the layout the
# single-launch BatchNorm kernels give it, except 256 threads x 8 vectors, which it does not
# build.  per = ceil(64 N / 256) vectors a thread of a 256-thread block would hold; the layout is
# <threads x vectors per thread> under e2ep_tune (key 25, key 26), "-" = not taken.  Its channels
# grow 64 vectors at a time, so N + 1 is the first shape past each switch at N (per as for one
# vector more).  N = 33 is past the middle's own bound (N * 256 <= 8192 elements a channel).
#
#    N  float4  per | (1, 1)    (2, 1)    (1, 2)    (2, 2)
#    4     256    1 | 256 x 1   256 x 1   256 x 1   256 x 1
#    5     320    2 | 256 x 2   256 x 2   512 x 1   512 x 1
#    8     512    2 | 256 x 2   256 x 2   512 x 1   512 x 1
#    9     576    3 | 256 x 4   256 x 4   512 x 2   512 x 2
#   16    1024    4 | 256 x 4   256 x 4   512 x 2   512 x 2
#   17    1088    5 | -(256x8)  512 x 4   -(256x8)  512 x 4
#   32    2048    8 | -(256x8)  512 x 4   -(256x8)  512 x 4
#   33    2112    9 | -         -         -         -
MID_OK = {4: (1, 1, 1, 1), 5: (1, 1, 1, 1), 8: (1, 1, 1, 1), 9: (1, 1, 1, 1), 16: (1, 1, 1, 1),
          17: (0, 1, 0, 1), 32: (0, 1, 0, 1), 33: (0, 0, 0, 0)}


@pytest.mark.parametrize("K", [3, 5])
def test_mbconv_mid_takes_the_bn_kernels_layouts(lib, K):
    before = _state(lib)
    got = {}
    for N in MID_OK:
        row = []
        for wide, wide_lo in ((1, 1), (2, 1), (1, 2), (2, 2)):
            setting = {"tune": {str(rec.KEY_WIDE): wide, str(rec.KEY_WIDE_LO): wide_lo},
                       "bn_small": None, "limits": None}
            with rec.applied(lib, setting):
                row.append(lib.e2ep_mbconv_mid_ok((ctypes.c_int * 10)(*rec.mid_dims(N, 672, K))))
        got[N] = tuple(row)
    assert _state(lib) == before, "setting not restored"
    assert got == MID_OK
