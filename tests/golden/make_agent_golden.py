"""Generate tests/golden/agent_post.json by running the REFERENCE agent's own post-processing
functions (agent/parking_agent.py, dataset/carla_dataset.py) on small and seeded inputs.

Run in the build container only (needs /root/reference):
    python tests/golden/make_agent_golden.py

agent/parking_agent.py is imported unmodified.  Its imports that are absent from this image
are stubbed in sys.modules: carla, pygame, the data_generation modules, loguru,
torchvision.transforms, pyquaternion, and model.parking_model (its ParkingModel is only named
by load_model, which is not called; importing the real one needs the timm / trunk shims of
make_golden.py and changes nothing recorded here).  The reference's functions are then called
unbound on a stand-in object that carries `cfg` and `pre_target_point`:
ParkingAgent.save_prev_target (with get_target_point_ego_coord), ParkingAgent.save_seg_img and
detokenize.  No reference source is copied: only the inputs (inline, or a RandomState seed plus
the generating rule of tests/agent_ref.py) and the recorded results are written.  Before
writing, the script asserts that tests/agent_ref.py reproduces every recorded result."""
import hashlib
import json
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = "/root/reference"
OUT = os.path.join(REPO, "tests", "golden", "agent_post.json")
sys.path.insert(0, os.path.join(REPO, "tests"))

import agent_ref  # noqa: E402

TOKEN_NUMS = 204


def install_stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    mod("carla", Image=type("Image", (), {}), VehicleControl=type("VehicleControl", (), {}))
    mod("pygame")
    mod("data_generation")
    mod("data_generation.network_evaluator", NetworkEvaluator=object)
    mod("data_generation.tools", encode_npy_to_pil=None)
    mod("loguru", logger=types.SimpleNamespace(info=lambda *a, **k: None))
    tvt = mod("torchvision.transforms", Compose=lambda fs: None, ToTensor=lambda: None,
              Normalize=lambda **k: None)
    mod("torchvision", transforms=tvt)
    mod("pyquaternion", Quaternion=object)
    pm = mod("model.parking_model", ParkingModel=object)
    mod("model", parking_model=pm)
    if not hasattr(np, "string_"):
        np.string_ = np.bytes_
    sys.path.insert(0, REF)


def base(X, Y):
    """Class 0 wins everywhere."""
    a = np.zeros((3, X, Y), dtype=np.float32)
    a[0], a[2] = 1.0, -1.0
    return a


def with_slot(a, pixels):
    for r, c in pixels:
        a[2, r, c] = 2.0
    return a


def slot_cases():
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    out = []
    for seed in (11, 12):
        out.append(dict(name=f"noise_blob_200_seed{seed}",
                        gen=dict(rule="noise_blob", seed=seed, shape=[3, 200, 200], boost=6.0)))
    out.append(dict(name="none_8x8", a=base(8, 8)))
    out.append(dict(name="one_corner_8x8", a=with_slot(base(8, 8), [(0, 7)])))
    a = base(8, 8)
    a[2] = 2.0
    out.append(dict(name="all_8x8", a=a))
    out.append(dict(name="nonsquare_5x7", a=with_slot(base(5, 7), [(0, 1), (1, 5), (4, 6), (2, 2)])))
    # flipped rows {2, 3, 3} (mean 2 + 2/3), columns {4, 4, 5} (mean 4 + 1/3)
    out.append(dict(name="truncation_8x8", a=with_slot(base(8, 8), [(5, 4), (4, 4), (4, 5)])))
    out.append(dict(name="asymmetric_8x8", a=with_slot(base(8, 8), [(0, 1), (1, 1), (0, 2)])))
    a = with_slot(base(8, 8), [(6, 6)])
    a[1, 2, 3] = a[2, 2, 3] = 3.0  # classes 1 and 2 tie: 1 wins
    a[1, 3, 3] = a[2, 3, 3] = 3.0
    out.append(dict(name="tie_1_2_8x8", a=a))
    a = with_slot(base(8, 8), [(1, 6)])
    a[0, 2, 3] = a[2, 2, 3] = 3.0  # classes 0 and 2 tie: 0 wins
    a[0, 5, 0] = a[2, 5, 0] = 3.0
    out.append(dict(name="tie_0_2_8x8", a=a))
    a = base(8, 8)
    a[2, 1, 2] = a[2, 6, 5] = nan
    out.append(dict(name="nan_plane2_8x8", a=a))
    a = with_slot(base(8, 8), [(7, 0)])
    a[1, 1, 2] = a[2, 1, 2] = nan  # the first NaN (class 1) wins
    a[2, 3, 4] = nan
    a[0, 4, 4] = a[1, 4, 4] = a[2, 4, 4] = nan
    out.append(dict(name="nan_planes12_8x8", a=a))
    a = base(8, 8)
    a[2, 0, 0] = inf
    a[0, 1, 1] = a[2, 1, 1] = inf     # tie at +inf: 0 wins
    a[:, 2, 2] = -inf                 # all -inf: 0 wins
    a[0, 3, 3] = a[1, 3, 3] = -inf    # class 2 is the only finite one
    a[1, 4, 4] = inf
    a[2, 5, 6] = inf
    out.append(dict(name="inf_8x8", a=a))
    return out


def detok_cases():
    toks = [[t, 100, 100] for t in (0, 99, 100, 101, 200)]
    toks += [[50, s, 100] for s in (0, 100, 200)]
    toks += [[150, 100, r] for r in (100, 101, 200)]
    for special in (201, 202, 203):
        for pos in range(3):
            t = [120, 80, 150]
            t[pos] = special
            toks.append(t)
    return toks


def main():
    install_stubs()
    from agent.parking_agent import ParkingAgent
    from dataset.carla_dataset import detokenize

    class StandIn:
        get_target_point_ego_coord = ParkingAgent.get_target_point_ego_coord

        def __init__(self):
            self.cfg = types.SimpleNamespace(bev_x_bound=[-10.0, 10.0, agent_ref.RES[0]],
                                             bev_y_bound=[-10.0, 10.0, agent_ref.RES[1]])
            self.pre_target_point = None

    cases = []
    for c in slot_cases():
        rec = dict(name=c["name"])
        if "gen" in c:
            rec["gen"] = c["gen"]
            a = agent_ref.generate(c["gen"])
        else:
            a = c["a"]
            rec["shape"] = list(a.shape)
            rec["logits"] = agent_ref.encode_logits(a)
            assert np.array_equal(agent_ref.decode_logits(rec), a, equal_nan=True)
        s = StandIn()
        seg = torch.from_numpy(a.copy())[None]
        ParkingAgent.save_prev_target(s, seg)
        ParkingAgent.save_seg_img(s, seg)
        img = np.ascontiguousarray(np.asarray(s.seg_bev)).astype(np.uint8)
        assert np.array_equal(img, np.asarray(s.seg_bev))
        target = None if s.pre_target_point is None else [float(v) for v in s.pre_target_point]
        rec["expect"] = dict(target=target)
        if img.size <= 64:
            rec["expect"]["seg_image"] = img.reshape(-1).tolist()
        else:
            rec["expect"]["seg_image_sha256"] = hashlib.sha256(img.tobytes()).hexdigest()
        # the vectorised restatement must reproduce the reference before anything is written
        mine = agent_ref.slot(a)
        assert mine["found"] == (target is not None), c["name"]
        if target is not None:
            assert agent_ref.bits64([mine["x"], mine["y"]]).tolist() == agent_ref.bits64(target).tolist()
        assert np.array_equal(agent_ref.seg_image(a), img), c["name"]
        cases.append(rec)

    detok = []
    for t in detok_cases():
        got = detokenize(list(t), TOKEN_NUMS)
        exp = [float(got[0]), float(got[1]), float(got[2]), bool(got[3])]
        mine = agent_ref.detokenize(t, TOKEN_NUMS)
        assert agent_ref.bits64(mine[:3]).tolist() == agent_ref.bits64(exp[:3]).tolist(), t
        assert bool(mine[3]) == exp[3]
        detok.append(dict(tokens=t, expect=exp))

    doc = dict(meta=dict(source="reference agent/parking_agent.py save_prev_target, "
                                "get_target_point_ego_coord, save_seg_img and "
                                "dataset/carla_dataset.py detokenize, imported under stubs",
                         pinned=True, res=list(agent_ref.RES), token_nums=TOKEN_NUMS,
                         numpy=np.__version__, torch=torch.__version__),
               slot_cases=cases, detok_cases=detok)
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=None, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {OUT}: {len(cases)} slot cases, {len(detok)} detokenize cases, "
          f"{os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
