"""The agent's pre- and post-processing kernels (csrc/agent.hip, k_decode_bgra of
csrc/decode.hip) against tests/agent_ref.py and the results recorded from the reference
(tests/golden/agent_post.json).  Every quantity is an integer or a bit pattern: no tolerances."""
import json
import os
import types

import numpy as np
import pytest
import torch

import agent_ref
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DOC = json.load(open(os.path.join(GOLDEN, "agent_post.json")))
RES = tuple(DOC["meta"]["res"])
TOKEN_NUMS = DOC["meta"]["token_nums"]


def _A():
    from e2ep_amd import agent_step
    return agent_step


def _offset_view(t):
    """The same values one float off a 16-byte boundary (the dword-load path)."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = flat[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


def _run(logits, state=None, image=True, **kw):
    """slot_stats on (B, C, X, Y) device logits -> dict of host results."""
    A = _A()
    B, C, X, Y = logits.shape
    dev = logits.device
    state = A.new_state(B, dev) if state is None else state
    found = torch.full((B,), -7, dtype=torch.int32, device=dev)
    stats = torch.full((B, 3), -7, dtype=torch.int64, device=dev)
    img = torch.full((B, X, Y), 77, dtype=torch.uint8, device=dev) if image else None
    A.slot_stats(logits, state, RES, class_image=img, found=found, stats=stats, **kw)
    torch.cuda.synchronize()
    return dict(state=state.cpu().numpy(), found=found.cpu().numpy(), stats=stats.cpu().numpy(),
                image=None if img is None else img.cpu().numpy())


def _expect(logits_np):
    """agent_ref per sample -> the arrays _run returns (state from a cleared start)."""
    B = logits_np.shape[0]
    state = np.zeros((B, 3), np.float32)
    found, stats, imgs = np.zeros(B, np.int32), np.zeros((B, 3), np.int64), []
    for b in range(B):
        s = agent_ref.slot(logits_np[b], RES)
        found[b], stats[b] = s["found"], (s["count"], s["tx"], s["ty"])
        if s["found"]:
            state[b] = (1.0, s["px"], s["py"])
        imgs.append(agent_ref.seg_image(logits_np[b]))
    return dict(state=state, found=found, stats=stats, image=np.stack(imgs))


def _same(got, exp):
    assert got["found"].tolist() == exp["found"].tolist()
    assert got["stats"].tolist() == exp["stats"].tolist()
    assert agent_ref.bits(got["state"]).tolist() == agent_ref.bits(exp["state"]).tolist()
    if got["image"] is not None:
        assert np.array_equal(got["image"], exp["image"])


@pytest.mark.parametrize("case", DOC["slot_cases"], ids=lambda c: c["name"])
def test_golden_slot_cases(case):
    a = agent_ref.decode_logits(case)
    t = torch.from_numpy(a)[None].cuda()
    got, exp = _run(t), _expect(a[None])
    _same(got, exp)
    # the reference's recorded Python floats, rounded as torch.tensor(..., dtype=float) does
    target = case["expect"]["target"]
    assert bool(got["found"][0]) == (target is not None)
    if target is not None:
        assert agent_ref.bits(got["state"][0, 1:]).tolist() == agent_ref.bits(np.float32(target)).tolist()
    else:
        assert got["stats"][0].tolist() == [0, -1, -1]
    # the class image is the flipped torch.argmax image through the lookup table
    lut = torch.tensor(agent_ref.LUT, dtype=torch.uint8, device="cuda")
    assert np.array_equal(got["image"][0], lut[torch.argmax(t[0], dim=0)].flip(0).cpu().numpy())
    if "seg_image" in case["expect"]:
        assert got["image"][0].reshape(-1).tolist() == case["expect"]["seg_image"]
    # the dword-load path on the same values: the same integers
    _same(_run(_offset_view(t)), exp)
    # another lookup table, and no class image at all
    other = _run(t, class_lut=(9, 8, 7))["image"][0]
    assert np.array_equal(other, np.asarray([9, 8, 7], np.uint8)[agent_ref.classes(a)][::-1])
    _same(_run(t, image=False), exp)


def _batch(X, Y, seed):
    """(3, 3, X, Y): sample 0 a class-2 blob in noise, sample 1 no class-2 pixel, sample 2
    pure noise (class 2 on about a third of the map)."""
    rs = np.random.RandomState(seed)
    a = rs.standard_normal((3, 3, X, Y)).astype(np.float32)
    a[0, 2] -= 4.0
    a[0, 2, X // 3:X // 3 + 3, Y // 2:Y // 2 + 2] += 9.0
    a[1, 2] = -10.0
    return a


@pytest.mark.parametrize("X,Y", [(10, 12), (200, 200), (49, 52), (7, 5)])
def test_batched_paths_agree(X, Y):
    a = _batch(X, Y, seed=X * 1000 + Y)
    exp = _expect(a)
    assert exp["found"].tolist() == [1, 0, 1]
    t = torch.from_numpy(a).cuda()
    _same(_run(t), exp)                      # 16-byte loads where Y % 4 == 0
    _same(_run(_offset_view(t)), exp)        # dword loads
    wide = torch.zeros(3, 3, X, 2 * Y, device="cuda")
    wide[..., ::2] = t
    assert wide[..., ::2].stride(3) == 2
    _same(_run(wide[..., ::2]), exp)         # strided along Y
    cl = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert cl.stride(1) == 1 and not cl.is_contiguous()
    _same(_run(cl), exp)                     # channels-last view
    sub = torch.zeros(5, 4, X, Y, device="cuda")
    sub[1:4, :3] = t
    _same(_run(sub[1:4, :3]), exp)           # a slice of a larger batch: 16-byte path, odd strides


def test_more_classes_and_target_class():
    rs = np.random.RandomState(5)
    a = rs.standard_normal((2, 8, 9, 16)).astype(np.float32)
    t = torch.from_numpy(a).cuda()
    A = _A()
    for target in (0, 5, 7):
        state = A.new_state(2, t.device)
        stats = torch.zeros((2, 3), dtype=torch.int64, device=t.device)
        A.slot_stats(t, state, RES, target_class=target, stats=stats)
        for b in range(2):
            s = agent_ref.slot(a[b], RES, target=target)
            assert stats[b].tolist() == [s["count"], s["tx"], s["ty"]]


def test_state_persists_per_sample_and_target_select():
    A = _A()
    a = _batch(10, 12, seed=3)
    t = torch.from_numpy(a).cuda()
    goal = torch.tensor([[1.0, 2.0, 30.0], [-3.0, 4.0, -60.0], [5.0, -6.0, 90.0]], device="cuda")
    state = A.new_state(3, t.device)
    assert torch.equal(A.target_select(state, goal), goal)  # nothing found yet: the goal
    first = _run(t, state=state)
    exp = _expect(a)
    _same(first, exp)
    used = A.target_select(state, goal).cpu().numpy()
    for b in range(3):
        prev = tuple(exp["state"][b, 1:]) if exp["found"][b] else None
        assert agent_ref.bits(used[b]).tolist() == agent_ref.bits(
            agent_ref.target_used(prev, goal[b].cpu().numpy())).tolist()
    assert used[0, 2] == 30.0 and used[1].tolist() == [-3.0, 4.0, -60.0]
    # a not-found call leaves the earlier (valid, px, py) untouched, sample by sample
    none = torch.from_numpy(np.repeat(a[1:2], 3, 0)).cuda()
    second = _run(none, state=state)
    assert second["found"].tolist() == [0, 0, 0]
    assert agent_ref.bits(second["state"]).tolist() == agent_ref.bits(first["state"]).tolist()
    # sample 1 finds one now; the others keep theirs
    mixed = none.clone()
    mixed[1] = t[2]
    third = _run(mixed, state=state)
    assert third["found"].tolist() == [0, 1, 0]
    assert agent_ref.bits(third["state"][[0, 2]]).tolist() == agent_ref.bits(first["state"][[0, 2]]).tolist()
    assert agent_ref.bits(third["state"][1]).tolist() == agent_ref.bits(exp["state"][2]).tolist()
    state.zero_()  # reset
    assert torch.equal(A.target_select(state, goal), goal)


def test_detokenize_cases_strided_rows():
    A = _A()
    cases = DOC["detok_cases"]
    B = len(cases)
    buf = torch.full((B, 7), 203, dtype=torch.int64, device="cuda")
    buf[:, 0] = TOKEN_NUMS - 3
    buf[:, 1:4] = torch.tensor([c["tokens"] for c in cases])
    seq = buf[:, :4]
    assert seq.stride(0) == 7 > seq.shape[1]
    logits = torch.zeros(B, 3, 8, 8, device="cuda")
    controls = torch.full((B, 4), -5.0, dtype=torch.float64, device="cuda")
    out = torch.zeros((B, 4), dtype=torch.int64, device="cuda")
    A.slot_stats(logits, A.new_state(B, "cuda"), RES, seq=seq, first=1, token_nums=TOKEN_NUMS,
                 controls=controls, tokens_out=out)
    exp = np.asarray([[*c["expect"][:3], float(c["expect"][3])] for c in cases])
    got = controls.cpu().numpy()
    assert agent_ref.bits64(got).tolist() == agent_ref.bits64(exp).tolist()  # -0.0 included
    assert np.signbit(exp[:, 1]).any()
    assert torch.equal(out, seq)
    assert agent_ref.bits64(agent_ref.detokenize(seq[:, 1:].cpu().numpy(), TOKEN_NUMS)).tolist() == \
        agent_ref.bits64(exp).tolist()


@pytest.mark.parametrize("N,H,W,crop", [(2, 10, 14, 8), (1, 8, 8, 8), (4, 300, 400, 256),
                                        (2, 9, 11, 7)])
def test_decode_bgra_equals_process_image(N, H, W, crop):
    from dataset.carla_dataset import ProcessImage
    A = _A()
    raw = np.random.RandomState(N * 100 + crop).randint(0, 256, (N, H, W, 4)).astype(np.uint8)
    raw[0, H // 2 - crop // 2, W // 2 - crop // 2] = (0, 255, 1, 9)  # the crop's first pixel
    proc = ProcessImage(crop)
    ref_img, ref_rgb = [], []
    for n in range(N):
        img, rgb = proc(types.SimpleNamespace(raw_data=raw[n].tobytes(), height=H, width=W))
        ref_img.append(img)
        ref_rgb.append(np.asarray(rgb))
    ref_img, ref_rgb = torch.cat(ref_img, 0), np.stack(ref_rgb)
    assert ref_img.shape == (N, 3, crop, crop)
    dev = torch.from_numpy(raw).cuda()
    image, rgb = A.decode_bgra(dev, crop, rgb=True)
    assert torch.equal(image.cpu().view(torch.int32), ref_img.view(torch.int32))  # bitwise
    assert np.array_equal(rgb.cpu().numpy(), ref_rgb)
    image2, none = A.decode_bgra(dev, crop)
    assert none is None and torch.equal(image2, image)
    from e2ep_amd import _lib
    with pytest.raises(_lib.E2EPError):
        A.decode_bgra(dev, H + 1)


def test_four_launches_captured_replay_equals_eager():
    from e2ep_amd import graphs
    A = _A()
    N, H, W, crop, X, Y = 2, 10, 14, 8, 10, 12
    a = _batch(X, Y, seed=9)
    feeds = []  # (logits sample index, goal, frames seed, tokens): found, not found, found
    for k, src in enumerate((0, 1, 2)):
        feeds.append(dict(
            logits=torch.from_numpy(a[src:src + 1]).cuda(),
            goal=torch.tensor([[1.0 + k, -2.0 * k, 10.0 * k]], device="cuda"),
            frames=torch.from_numpy(np.random.RandomState(k).randint(0, 256, (N, H, W, 4)).astype(np.uint8)).cuda(),
            seq=torch.tensor([[201, 30 + 70 * k, 100 + k, 99 + k]], device="cuda")))

    def buffers():
        return dict(state=A.new_state(1, "cuda"), ws=A.slot_workspace(1, X, "cuda"),
                    image=torch.zeros(N, 3, crop, crop, device="cuda"),
                    rgb=torch.zeros(N, crop, crop, 3, dtype=torch.uint8, device="cuda"),
                    used=torch.zeros(1, 3, device="cuda"),
                    seg=torch.zeros(1, X, Y, dtype=torch.uint8, device="cuda"),
                    found=torch.zeros(1, dtype=torch.int32, device="cuda"),
                    stats=torch.zeros(1, 3, dtype=torch.int64, device="cuda"),
                    controls=torch.zeros(1, 4, dtype=torch.float64, device="cuda"),
                    toks=torch.zeros(1, 4, dtype=torch.int64, device="cuda"))

    def chain(inp, o):
        A.decode_bgra(inp["frames"], crop, out_image=o["image"], out_rgb=o["rgb"])
        A.target_select(o["state"], inp["goal"], out=o["used"])
        A.slot_stats(inp["logits"], o["state"], RES, workspace=o["ws"], class_image=o["seg"],
                     found=o["found"], stats=o["stats"], seq=inp["seq"], first=1,
                     token_nums=TOKEN_NUMS, controls=o["controls"], tokens_out=o["toks"])

    static = {k: v.clone() for k, v in feeds[0].items()}
    cap, eager = buffers(), buffers()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain(static, cap)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    cap["state"].zero_()
    g, _, _ = graphs.capture(lambda: chain(static, cap))
    states = []
    for k, f in enumerate(feeds):
        for key in static:
            static[key].copy_(f[key])
        g.replay()
        chain(f, eager)
        torch.cuda.synchronize()
        for key in cap:
            if key != "ws":
                assert torch.equal(cap[key].view(torch.uint8), eager[key].view(torch.uint8)), (k, key)
        states.append(cap["state"].cpu().numpy().copy())
        exp = agent_ref.slot(a[k], RES)
        assert bool(cap["found"].item()) == exp["found"]
    # the state advances from replay to replay: found, kept, replaced
    assert states[0][0, 0] == 1.0
    assert agent_ref.bits(states[1]).tolist() == agent_ref.bits(states[0]).tolist()
    assert agent_ref.bits(states[2]).tolist() != agent_ref.bits(states[1]).tolist()
    # replay 2 used replay 1's point, replay 3 (its own goal's yaw) still that point
    assert agent_ref.bits(cap["used"].cpu().numpy()[0]).tolist() == agent_ref.bits(
        agent_ref.target_used(tuple(states[1][0, 1:]), feeds[2]["goal"][0].cpu().numpy())).tolist()
