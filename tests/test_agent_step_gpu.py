"""AgentStep (e2ep_amd/agent_step.py): the agent's whole tick on the device, full model, B = 1.

After each tick the expectation is computed on the host with tests/agent_ref.py from THAT
tick's own pred_segmentation and tokens, never from a second trajectory: a one-ulp logit
difference could flip a pixel and fork the two.  Everything compared is an integer or a bit
pattern."""
import types

import numpy as np
import pytest
import torch

import agent_ref

pytestmark = pytest.mark.gpu

H, W, N_CAMS = 300, 400, 4
TICKS = 4


def _model():
    """Seeded ParkingModel whose segmentation head's final bias lets class 2 win on part of the
    map: the class-2 bias is raised by the 15th percentile of (best other logit - class-2
    logit) of tick 0's frames, so roughly a seventh of that map is the target slot."""
    from e2ep_amd import agent_step
    from model.parking_model import ParkingModel
    from tool.config import default_cfg
    torch.manual_seed(0)
    m = ParkingModel(default_cfg()).cuda().eval()
    inp = _inputs(0)
    image, _ = agent_step.decode_bgra(torch.from_numpy(inp["frames"]).cuda(), m.cfg.image_crop)
    with torch.no_grad():
        seg = m.predict(_data(image, inp["goal"], inp), _noise())[1][0]
        gap = torch.maximum(seg[0], seg[1]) - seg[2]
        m.segmentation_head.segmentation_head[3].bias[2] += torch.quantile(gap.flatten(), 0.15)
    return m


def _rig():
    from e2ep_amd import synthetic
    K, E = synthetic.rig(N_CAMS, 256)
    return K[None], E[None]


RIG = None


def _inputs(k):
    """Tick k's host inputs: seeded raw frames, ego motion and goal."""
    global RIG
    from e2ep_amd import synthetic
    if RIG is None:
        RIG = _rig()
    b = synthetic.synthetic_batch(1, seed=100 + k)
    frames = np.random.RandomState(k).randint(0, 256, (N_CAMS, H, W, 4)).astype(np.uint8)
    return dict(frames=frames, ego=b["ego_motion"][0, 0].clone(), goal=b["target_point"][0].clone(),
                K=RIG[0], E=RIG[1])


def _noise():
    from e2ep_amd import synthetic
    return synthetic.target_noise(1, seed=0).cuda()


def _data(image, target, inp):
    bos = torch.tensor([[204 - 3]], dtype=torch.int64, device="cuda")
    return {"image": image.view(1, N_CAMS, 3, *image.shape[-2:]),
            "target_point": torch.as_tensor(target, dtype=torch.float32).view(1, 3).cuda(),
            "ego_motion": inp["ego"].view(1, 1, 3).cuda(), "gt_control": bos,
            "intrinsics": inp["K"], "extrinsics": inp["E"]}


def _tick(step, k, as_objects=False):
    inp = _inputs(k)
    frames = inp["frames"]
    if as_objects:  # CARLA sensor images: raw_data, height, width
        frames = [types.SimpleNamespace(raw_data=f.tobytes(), height=H, width=W) for f in frames]
    return step.tick(frames, inp["ego"], inp["goal"], inp["K"], inp["E"], noise=_noise().cpu())


@pytest.fixture(scope="module")
def model():
    return _model()


@pytest.fixture(scope="module")
def trajectory(model):
    """Four captured ticks, each checked against its own outputs; returns the step and the
    per-tick results for the comparisons below."""
    from e2ep_amd import agent_step
    from dataset.carla_dataset import detokenize
    step = agent_step.AgentStep(model, cam_hw=(H, W), n_cams=N_CAMS, display=True)
    prev, out = None, []
    for k in range(TICKS):
        inp = _inputs(k)
        r = _tick(step, k, as_objects=(k == 1))
        seg = step.pred_segmentation[0].cpu().numpy()
        exp = agent_ref.slot(seg, step.res)
        # the target this tick consumed is the expectation of the tick before
        used = agent_ref.target_used(prev, inp["goal"].numpy())
        assert agent_ref.bits(r.target_point_used).tolist() == agent_ref.bits(used).tolist(), k
        assert r.slot_found == exp["found"], k
        assert r.slot_stats == (exp["count"], exp["tx"], exp["ty"]), k
        if exp["found"]:
            prev = (exp["px"], exp["py"])
        if prev is None:
            assert r.next_target is None
        else:
            assert agent_ref.bits(r.next_target).tolist() == agent_ref.bits(prev).tolist(), k
        assert r.tokens == step.tokens[0].tolist() and r.tokens[0] == 201 and len(r.tokens) == 4
        ctl = agent_ref.detokenize(r.tokens[1:], 204)
        assert agent_ref.bits64(r.controls[:3]).tolist() == agent_ref.bits64(ctl[:3]).tolist()
        assert r.controls[3] is bool(ctl[3])
        host = detokenize(r.tokens[1:], 204)
        assert r.controls[:3] == host[:3] and r.controls[3] is host[3]
        # tokens = model.predict on the decoded image and the used target
        image, rgb = agent_step.decode_bgra(torch.from_numpy(inp["frames"]).cuda(), step.crop, rgb=True)
        assert torch.equal(image, step.image[0]) and torch.equal(rgb, step.rgb_crops)
        with torch.no_grad():
            toks, seg2, _, tb = model.predict(_data(image, r.target_point_used, inp), _noise())
        assert toks[0].tolist() == r.tokens, k
        assert torch.equal(tb, step.target_bev)
        assert np.array_equal(step.seg_image[0].cpu().numpy(), agent_ref.seg_image(seg))
        out.append(dict(r=r, goal=inp["goal"].numpy(), seg=seg))
    return step, out


def test_ticks_match_their_own_outputs(trajectory):
    step, out = trajectory
    assert any(o["r"].slot_found for o in out)  # not vacuous: a slot was found ...
    assert any(agent_ref.bits(o["r"].target_point_used).tolist() != agent_ref.bits(o["goal"]).tolist()
               for o in out)                    # ... and fed back
    assert all(o["r"].target_point_used[2] == float(np.float32(o["goal"][2])) for o in out)
    assert step.graph_memsets >= 0 and step._graph is not None


def test_captured_equals_eager_and_repeats(model, trajectory):
    from e2ep_amd import agent_step
    step, out = trajectory
    eager = agent_step.AgentStep(model, cam_hw=(H, W), n_cams=N_CAMS, capture=False)
    step.reset()
    for k in range(TICKS):
        e, c, first = _tick(eager, k), _tick(step, k), out[k]["r"]
        for a, b in ((e, c), (first, c)):  # eager == captured; the captured run repeats bitwise
            assert a.tokens == b.tokens, k
            assert agent_ref.bits64(a.controls[:3]).tolist() == agent_ref.bits64(b.controls[:3]).tolist()
            assert a.controls[3] is b.controls[3]
            assert a.slot_found == b.slot_found and a.slot_stats == b.slot_stats
            assert (a.next_target is None) == (b.next_target is None)
            if a.next_target is not None:
                assert agent_ref.bits(a.next_target).tolist() == agent_ref.bits(b.next_target).tolist()
            assert agent_ref.bits(a.target_point_used).tolist() == agent_ref.bits(b.target_point_used).tolist()
        assert np.array_equal(step.pred_segmentation[0].cpu().numpy(), out[k]["seg"])
    assert eager._graph is None and eager.seg_image is None and eager.rgb_crops is None


def test_reset_rig_and_noise_rules(trajectory):
    from e2ep_amd import _lib
    step, out = trajectory
    inp = _inputs(0)
    step.reset()
    r = _tick(step, 0)
    assert agent_ref.bits(r.target_point_used).tolist() == agent_ref.bits(inp["goal"].numpy()).tolist()
    K2 = inp["K"].clone()
    K2[0, 0, 0, 2] += 1.0
    with pytest.raises(_lib.E2EPError, match="rig"):
        step.tick(inp["frames"], inp["ego"], inp["goal"], K2, inp["E"], noise=_noise().cpu())
    with pytest.raises(_lib.E2EPError, match="noise"):
        step.tick(inp["frames"], inp["ego"], inp["goal"], inp["K"], inp["E"])
    with pytest.raises(_lib.E2EPError, match="frames"):
        step.tick(inp["frames"][:, :10], inp["ego"], inp["goal"], inp["K"], inp["E"],
                  noise=_noise().cpu())
    step.tick(inp["frames"], inp["ego"], inp["goal"], inp["K"].clone(), inp["E"].clone(),
              noise=_noise().cpu())  # an equal rig in other tensors is the same rig


def test_fp16_tick():
    from e2ep_amd import agent_step, precision
    m = _model()
    with precision.use("fp16"):
        step = agent_step.AgentStep(m, cam_hw=(H, W), n_cams=N_CAMS)
        r = _tick(step, 2)
        inp = _inputs(2)
        with torch.no_grad():
            toks = m.predict(_data(step.image[0], r.target_point_used, inp), _noise())[0]
    assert toks[0].tolist() == r.tokens
    exp = agent_ref.slot(step.pred_segmentation[0].cpu().numpy(), step.res)
    assert r.slot_found == exp["found"] and r.slot_stats == (exp["count"], exp["tx"], exp["ty"])
    if exp["found"]:
        assert agent_ref.bits(r.next_target).tolist() == agent_ref.bits([exp["px"], exp["py"]]).tolist()
    assert precision.get() == "fp32"


def test_attention_hook_refreshed_by_the_replay():
    """The agent's attention patch and hook (agent/parking_agent.py:71-91, :266-268): the
    hook's tensor is a static output of the captured tick, refreshed by every replay."""
    from e2ep_amd import agent_step
    m = _model()
    sa = m.feature_fusion.tf_encoder.layers[-1].self_attn
    forward_orig = sa.forward

    def wrap(*args, **kwargs):
        kwargs["need_weights"] = True
        kwargs["average_attn_weights"] = False
        return forward_orig(*args, **kwargs)
    sa.forward = wrap
    saved = []
    sa.register_forward_hook(lambda mod, i, o: saved.append(o[1]))
    step = agent_step.AgentStep(m, cam_hw=(H, W), n_cams=N_CAMS)
    r0 = _tick(step, 0)
    kept = saved[-1]  # the capture's
    assert tuple(kept.shape) == (1, 6, 256, 256)
    w0 = kept.clone()
    n = len(saved)
    r1 = _tick(step, 1)
    assert len(saved) == n  # a replay runs no Python
    assert not torch.equal(kept, w0)
    inp = _inputs(1)
    with torch.no_grad():  # the eager hooked predict of tick 1's inputs
        toks = m.predict(_data(step.image[0], r1.target_point_used, inp), _noise())[0]
    assert torch.equal(saved[-1], kept)
    assert toks[0].tolist() == r1.tokens and len(r0.tokens) == 4
