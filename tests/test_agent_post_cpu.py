"""The agent's post-processing without a GPU: tests/agent_ref.py reproduces the results recorded
from the reference (tests/golden/agent_post.json), which ties the GPU expectations of
test_agent_post_gpu.py to the reference; the library exports the new entry points, and each
rejects bad arguments before any launch."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import agent_ref
from conftest import GOLDEN

EINVAL, ERANGE = -1, -2
DOC = json.load(open(os.path.join(GOLDEN, "agent_post.json")))
NEW = ("e2ep_decode_bgra", "e2ep_slot_stats_workspace", "e2ep_slot_partials", "e2ep_slot_finish",
       "e2ep_target_select")


@pytest.mark.parametrize("case", DOC["slot_cases"], ids=lambda c: c["name"])
def test_agent_ref_reproduces_reference_slot(case):
    a = agent_ref.decode_logits(case)
    got, exp = agent_ref.slot(a, DOC["meta"]["res"]), case["expect"]
    assert got["found"] == (exp["target"] is not None)
    if got["found"]:
        # the reference's Python floats, bit for bit (the sign of a zero included)
        assert agent_ref.bits64([got["x"], got["y"]]).tolist() == agent_ref.bits64(exp["target"]).tolist()
    img = agent_ref.seg_image(a)
    assert img.dtype == np.uint8 and img.shape == a.shape[1:]
    if "seg_image" in exp:
        assert img.reshape(-1).tolist() == exp["seg_image"]
    else:
        assert hashlib.sha256(img.tobytes()).hexdigest() == exp["seg_image_sha256"]


def test_golden_cases_cover_the_edges():
    names = {c["name"]: c for c in DOC["slot_cases"]}
    assert names["none_8x8"]["expect"]["target"] is None
    assert names["all_8x8"]["expect"]["target"] is not None
    assert names["nonsquare_5x7"]["shape"] == [3, 5, 7]
    s = agent_ref.slot(agent_ref.decode_logits(names["truncation_8x8"]))
    assert (s["count"], s["tx"], s["ty"]) == (3, 2, 4)  # means 2 + 2/3 and 4 + 1/3, truncated
    a = agent_ref.decode_logits(names["asymmetric_8x8"])
    assert agent_ref.slot(a)["tx"] != agent_ref.slot(a[:, ::-1].copy())["tx"]
    assert sum("gen" in c for c in DOC["slot_cases"]) == 2
    for n in ("nan_plane2_8x8", "nan_planes12_8x8", "inf_8x8"):
        assert not np.isfinite(agent_ref.decode_logits(names[n])).all()


def test_agent_ref_reproduces_reference_detokenize():
    tn = DOC["meta"]["token_nums"]
    toks = [c["tokens"] for c in DOC["detok_cases"]]
    got = agent_ref.detokenize(toks, tn)
    exp = np.asarray([[*c["expect"][:3], float(c["expect"][3])] for c in DOC["detok_cases"]])
    assert agent_ref.bits64(got).tolist() == agent_ref.bits64(exp).tolist()
    assert any(np.signbit(e[1]) and e[1] == 0.0 for e in exp)  # a recorded -0.0 brake
    from dataset.carla_dataset import detokenize  # the drop-in's own, same results
    for c in DOC["detok_cases"]:
        d = detokenize(list(c["tokens"]), tn)
        assert agent_ref.bits64(d[:3]).tolist() == agent_ref.bits64(c["expect"][:3]).tolist()
        assert d[3] is c["expect"][3]


def test_target_used():
    goal = [1.5, -2.25, 30.0]
    assert agent_ref.target_used(None, goal).tolist() == goal
    assert agent_ref.target_used((np.float32(0.5), np.float32(-0.0)), goal).tolist() == [0.5, -0.0, 30.0]


# ------------------------------------------------------------------------------------------
# the C ABI
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from e2ep_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libe2ep_hip.so not built; run __graft_entry__.build()")
    return _lib.load()


def test_library_exports_the_agent_entry_points(lib):
    from e2ep_amd import _lib
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, f"{name} not declared in include/e2ep.h"
    assert lib.e2ep_abi_version() == 4  # additive


# never dereferenced: every call below is rejected before a launch
P = ctypes.c_void_p(0x1000)
LUT = (ctypes.c_ubyte * 8)(0, 128, 255, 0, 0, 0, 0, 0)


def _partials(lib, logits=P, strides=(120000, 40000, 200, 1), B=1, C=3, X=200, Y=200, target=2,
              lut=LUT, image=None, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.e2ep_slot_stats_workspace(B, X)
    return lib.e2ep_slot_partials(logits, *strides, B, C, X, Y, target, lut, image, ws, ws_bytes, None)


def _finish(lib, ws=P, ws_bytes=None, B=1, X=200, Y=200, state=P, seq=None, stride=0, length=0,
            first=0, token_nums=204, controls=None, tokens_out=None):
    if ws_bytes is None:
        ws_bytes = lib.e2ep_slot_stats_workspace(B, X)
    return lib.e2ep_slot_finish(ws, ws_bytes, B, X, Y, 0.1, 0.1, state, None, None, seq, stride,
                                length, first, token_nums, controls, tokens_out, None)


def test_slot_workspace_query(lib):
    n = lib.e2ep_slot_stats_workspace(1, 200)
    assert n % 12 == 0 and 24 * 12 <= n <= 64 * 12  # a few dozen workgroups at the agent's shape
    assert lib.e2ep_slot_stats_workspace(3, 200) == 3 * n
    assert lib.e2ep_slot_stats_workspace(1, 5) == 5 * 12
    assert lib.e2ep_slot_stats_workspace(0, 200) == 0


def test_slot_partials_rejects_bad_arguments(lib):
    assert _partials(lib, logits=None) == EINVAL
    assert _partials(lib, ws=None) == EINVAL
    assert _partials(lib, C=1) == EINVAL
    assert _partials(lib, C=9) == EINVAL
    assert _partials(lib, target=3) == EINVAL
    assert _partials(lib, target=-1) == EINVAL
    assert _partials(lib, X=0) == EINVAL
    assert _partials(lib, strides=(120000, 40000, 200, 0)) == EINVAL
    assert _partials(lib, image=P, lut=None) == EINVAL
    assert _partials(lib, ws_bytes=lib.e2ep_slot_stats_workspace(1, 200) - 1) == EINVAL
    assert _partials(lib, X=2000, Y=2000) == ERANGE       # 8e9 > INT32_MAX
    assert _partials(lib, X=70000, Y=70000) == ERANGE     # X * Y alone overflows
    assert _partials(lib, B=70000, X=8, Y=8) == ERANGE
    assert b"e2ep_slot_partials" in lib.e2ep_last_error()


def test_slot_finish_rejects_bad_arguments(lib):
    assert _finish(lib, ws=None) == EINVAL
    assert _finish(lib, state=None) == EINVAL
    assert _finish(lib, B=0) == EINVAL
    assert _finish(lib, ws_bytes=8) == EINVAL
    assert _finish(lib, X=2000, Y=2000) == ERANGE
    seq = dict(seq=P, stride=4, length=4, first=1, controls=P)
    assert _finish(lib, **{**seq, "first": 2}) == EINVAL      # first + 3 > length
    assert _finish(lib, **{**seq, "stride": 3}) == EINVAL     # stride < length
    assert _finish(lib, **{**seq, "token_nums": 4}) == EINVAL
    assert _finish(lib, **{**seq, "controls": None}) == EINVAL  # a token row with no output
    assert b"e2ep_slot_finish" in lib.e2ep_last_error()


def test_decode_bgra_rejects_bad_arguments(lib):
    def call(bgra=P, N=4, H=300, W=400, crop=256, image=P, rgb=None):
        return lib.e2ep_decode_bgra(bgra, N, H, W, crop, image, rgb, None)
    assert call(bgra=None) == EINVAL
    assert call(image=None) == EINVAL
    assert call(crop=301) == EINVAL     # crop > H: the reference would return a smaller image
    assert call(H=600, crop=401) == EINVAL  # crop > W
    assert call(crop=0) == EINVAL
    assert call(N=0) == EINVAL
    assert call(bgra=ctypes.c_void_p(0x1001)) == EINVAL
    assert b"e2ep_decode_bgra" in lib.e2ep_last_error()


def test_target_select_rejects_bad_arguments(lib):
    assert lib.e2ep_target_select(None, P, 1, P, None) == EINVAL
    assert lib.e2ep_target_select(P, None, 1, P, None) == EINVAL
    assert lib.e2ep_target_select(P, P, 1, None, None) == EINVAL
    assert lib.e2ep_target_select(P, P, 0, P, None) == EINVAL


def test_agent_step_on_a_cpu_model_raises():
    from e2ep_amd import _lib, agent_step

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.zeros(1))
            self.cfg = None

    with pytest.raises(_lib.E2EPError, match="HIP device"):
        agent_step.AgentStep(Tiny())
    with pytest.raises(_lib.E2EPError, match="HIP device"):
        agent_step.decode_bgra(torch.zeros(1, 8, 8, 4, dtype=torch.uint8), 8)
    with pytest.raises(_lib.E2EPError, match="HIP device"):
        agent_step.slot_stats(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3), (0.1, 0.1))
    with pytest.raises(_lib.E2EPError, match="HIP device"):
        agent_step.target_select(torch.zeros(1, 3), torch.zeros(1, 3))
