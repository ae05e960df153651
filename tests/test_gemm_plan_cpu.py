"""The GEMM host queries answer what tests/golden/gemm_plans.json recorded
(scripts/record_gemm_plans.py, run on the commit before the routing moved into GemmPlan /
gemm_plan() of csrc/gemm.hip): e2ep_gemm_workspace and e2ep_gemm_rowsum_workspace for the model's
linears at B = 8 and B = 1, the GPU tests' shapes and the shapes at each gate's boundary, under
the forced plans, e2ep_gemm_split_min, e2ep_tune key 4, and the three settings that move a route
but no workspace (bf16 operands, e2ep_tune key 28, e2ep_gemm_skinny).  Host code only: no GPU
call is made."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

with open(os.path.join(ROOT, "tests", "golden", "gemm_plans.json")) as _f:
    GOLD = json.load(_f)

_spec = importlib.util.spec_from_file_location(
    "record_gemm_plans", os.path.join(ROOT, "scripts", "record_gemm_plans.py"))
rec = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rec)

SETTING_IDS = [s["name"] for s in GOLD["settings"]]


@pytest.fixture(scope="module")
def lib():
    from e2ep_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    return _lib.load()


def _shapes(test_fn, names):
    """The `names` list of a parametrised test."""
    return [tuple(c) for m in test_fn.pytestmark if m.args[0] == names for c in m.args[1]]


def _state(lib):
    """Every switch a setting can move.  e2ep_gemm_force cannot be read back: the automatic plan
    splits the 112 x 258 x 2048 product (12 blocks of 32 x 128, 64 K-steps) 8 ways, and every
    forced plan recorded here splits it 1, 3 or 64 ways."""
    keys = [lib.e2ep_tune(k, 0) for k in (rec.KEY_SPLIT_TARGET, rec.KEY_FOLD)]
    return (keys, lib.e2ep_gemm_split_min(0), lib.e2ep_gemm_precision(-1), lib.e2ep_gemm_skinny(-1),
            lib.e2ep_gemm_workspace(112, 258, 2048))


def test_fixture_covers_the_recorders_lists(lib):
    """The fixture holds every shape and setting the recorder lists, one row of every field
    each, and the recorder's copies of the GPU tests' shape lists are those tests' lists."""
    import test_gemm_gpu as t
    assert GOLD["fields"] == rec.FIELDS
    assert GOLD["shapes"] == rec.shapes()
    assert GOLD["settings"] == rec.settings(lib)
    assert sum(s["name"].startswith("model") for s in GOLD["shapes"]) == 2 * 3 * len(rec.model_linears())
    for s in GOLD["settings"]:
        rows = GOLD["results"][s["name"]]
        assert len(rows) == len(GOLD["shapes"]) and all(len(r) == len(rec.FIELDS) for r in rows)
    assert t.SHAPES == rec.TEST_SHAPES
    assert t.PAIR_SHAPES == rec.TEST_PAIR
    assert _shapes(t.test_gemm_epilogue_bias_add_relu, "M,N,K") == rec.TEST_EPILOGUE
    assert _shapes(t.test_gemm_rowsum_weight_and_bias_gradient, "rows,N,K") == rec.TEST_ROWSUM
    assert _shapes(t.test_gemm_bf16_operands_vs_rounded_fp64, "M,N,K") == rec.TEST_BF16
    rows = {M for _, M, _, _ in rec.model_linears()}
    widths = {d for _, _, N, K in rec.model_linears() for d in (N, K)}
    assert rows == {2048, 112} and widths == {258, 516, 774, 2048, 204}
    assert max(K for s in GOLD["shapes"] for K in s["shape"]) < 32 * rec.SPLITS_ABOVE_KSTEPS


@pytest.mark.parametrize("setting", GOLD["settings"], ids=SETTING_IDS)
def test_host_queries_match_recorded(lib, setting):
    before = _state(lib)
    assert before[1:] == (8, 0, 16, 8 * 112 * 258 * 4), "the library is not at its defaults"
    with rec.applied(lib, setting):
        got = [rec.query(lib, sh["shape"]) for sh in GOLD["shapes"]]
    assert _state(lib) == before, "setting not restored"
    want = GOLD["results"][setting["name"]]
    bad = [(sh["name"], f, w, g) for sh, wr, gr in zip(GOLD["shapes"], want, got)
           for f, w, g in zip(rec.FIELDS, wr, gr) if w != g]
    assert not bad, f"{len(bad)} answers differ (shape, field, recorded, got): {bad[:8]}"


def test_route_only_settings_changed_no_recorded_answer():
    """bf16 operands, the fold mode and the skinny limit choose kernels, not workspace sizes."""
    for name in ("precision_1", "key28_1", "key28_2", "skinny_0", "skinny_128"):
        assert GOLD["results"][name] == GOLD["results"]["default"], name
