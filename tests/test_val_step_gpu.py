"""ValStep (e2ep_amd.val) on MI355X: the eager chain against the reference's validation
scalars, the captured chain against the eager one bit for bit, the device accumulator against
the per-batch values, and no host synchronisation between construction and result()."""
import warnings

import numpy as np
import pytest
import torch

from helpers import golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
RIG = ("intrinsics", "extrinsics")


def _module():
    from trainer.pl_trainer import ParkingTrainingModule
    from tool.config import default_cfg
    from weights import make_state
    mod = ParkingTrainingModule(default_cfg(deterministic=True))
    mod.parking_model.load_state_dict(make_state(mod.parking_model.state_dict(), 1234))
    return mod.to(DEV).eval()


def _batch(b, seed):
    from e2ep_amd import synthetic
    d = synthetic.synthetic_batch(b, seed=seed)
    data = {k: (v if k in RIG else v.to(DEV)) for k, v in d.items()}
    return data, synthetic.target_noise(b, seed=seed).to(DEV)


@pytest.fixture(scope="module")
def module():
    return _module()


def test_b8_eager_epoch_of_one_batch_matches_reference(module):
    """The five means after one golden batch, each <= 1e-5 relative to the reference's
    validation_step: the bound test_model_b8_gpu holds validation_step itself to."""
    from e2ep_amd.val import KEYS, ValStep
    g = golden("validation_b8.npz")
    data, noise = _batch(8, 11)
    v = ValStep(module, data, noise=noise, graph=False)
    assert v.result()["batches"] == 0  # construction accumulates nothing
    loss = v()
    r = v.result()
    assert r["batches"] == 1 and set(KEYS) == set(g)
    for k in KEYS:
        e = abs(r[k] / float(g[k]) - 1)
        print("valstep_b8", k, r[k], float(g[k]), f"{e:.3e}")
        assert e < 1e-5, (k, r[k], float(g[k]))
    assert float(loss) == r["val_loss"]  # one batch: the mean is the value
    assert r["seg_confusion"].sum() == 8 * 200 * 200
    assert not module.training


def _torch_confusion(seg, target, C=3):
    pred = seg.argmax(1).reshape(-1)
    t = target.reshape(-1)
    return torch.bincount(t * C + pred, minlength=C * C).reshape(C, C).cpu().numpy()


@pytest.fixture(scope="module")
def captured(module):
    """A captured and an eager ValStep over the same module fed the same two batches (then the
    second batch once more): per call the value's bits of both, the four loss scalars and the
    eager segmentation's confusion matrix."""
    from e2ep_amd.val import KEYS, ValStep
    (b1, n1), (b2, n2) = _batch(2, 7), _batch(2, 8)
    vg = ValStep(module, b1, noise=n1, graph=True, warmup=2)
    ve = ValStep(module, b1, noise=n1, graph=False)
    assert vg._graph is not None and ve._graph is None
    assert vg.result()["batches"] == 0  # warm-up and capture accumulate nothing
    calls = []
    for b, n in ((b1, n1), (b2, n2), (b2, n2)):
        lg = vg(b, n).clone()
        le = ve(b, n).clone()
        calls.append(dict(graph=lg.cpu().numpy(), eager=le.cpu().numpy(),
                          values=[float(vg.values[k]) for k in KEYS[:4]] + [float(lg)],
                          conf=_torch_confusion(ve.pred[1], b["segmentation"])))
    return vg, ve, calls, (b1, n1), (b2, n2)


def test_b2_captured_equals_eager_bit_for_bit(captured):
    _, _, calls, _, _ = captured
    for c in calls:
        assert c["graph"].tobytes() == c["eager"].tobytes(), (c["graph"], c["eager"])
        assert np.isfinite(c["graph"])
    assert calls[0]["graph"] != calls[1]["graph"]  # the second batch really went in
    assert calls[1]["graph"].tobytes() == calls[2]["graph"].tobytes()  # same batch, same bits


def test_b2_result_is_the_float64_mean_of_the_batches(captured):
    from e2ep_amd.val import KEYS
    vg, ve, calls, _, _ = captured
    rg, re_ = vg.result(), ve.result()
    assert rg["batches"] == re_["batches"] == 3
    for i, k in enumerate(KEYS):
        s = 0.0
        for c in calls:
            s = s + c["values"][i]  # the device adds each fp32 value to a float64 sum in order
        assert rg[k] == s / 3, (k, rg[k], s / 3)
        assert re_[k] == rg[k]
    conf = sum(c["conf"] for c in calls)
    assert np.array_equal(rg["seg_confusion"], conf) and np.array_equal(re_["seg_confusion"], conf)
    inter, union = np.diag(conf), conf.sum(0) + conf.sum(1) - np.diag(conf)
    assert np.array_equal(rg["seg_iou"], inter / union)
    assert rg["seg_miou"] == float((inter / union).mean())


def test_b2_rig_and_noise_rules_then_reset(captured):
    from e2ep_amd import _lib
    vg, _, _, (b1, n1), _ = captured
    other = dict(b1)
    other["intrinsics"] = b1["intrinsics"].clone()
    other["intrinsics"][0, 0, 0, 2] += 1.0
    with pytest.raises(_lib.E2EPError, match="rig"):
        vg(other, n1)
    with pytest.raises(_lib.E2EPError, match="noise"):
        vg(b1)
    before = vg.result()["batches"]
    assert before >= 3  # neither refused call was accumulated
    vg.reset()
    r = vg.result()
    assert r["batches"] == 0 and r["seg_confusion"].sum() == 0 and np.isnan(r["val_loss"])
    vg(b1, n1)
    assert vg.result()["batches"] == 1


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_merge_over_a_world_of_one_changes_nothing(captured, backend):
    """result()'s data-parallel merge (one all-reduce of the packed buffer, the counts as
    float64; host-staged for gloo) in a world of one rank: the same epoch as without it."""
    import torch.distributed as dist
    from e2ep_amd.val import ValStep
    _, ve, _, (b1, n1), _ = captured
    ve(b1, n1)
    plain = ve.result()
    kw = dict(device_id=torch.device(DEV, 0)) if backend == "nccl" else {}
    dist.init_process_group(backend, store=dist.HashStore(), rank=0, world_size=1, **kw)
    try:
        merged = ValStep.finish(ve._merge())
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
    assert merged.keys() == plain.keys() and merged["batches"] == plain["batches"] >= 1
    for k, v in plain.items():
        assert np.array_equal(np.asarray(merged[k]), np.asarray(v), equal_nan=True), k


def test_calls_do_not_synchronise(captured, monkeypatch):
    """Between construction and result() a call reads nothing back: torch raises on any
    synchronising op (sync debug mode), and no device tensor sees .item() or .cpu()."""
    vg, ve, _, (b1, n1), (b2, n2) = captured
    reads = []
    for name in ("item", "cpu", "tolist", "numpy"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, _name=name, **k):
            if self.is_cuda:
                reads.append(_name)
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)
    vg.reset()
    ve.reset()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")  # torch: "sync debug mode is a prototype feature"
        torch.cuda.set_sync_debug_mode("error")
    try:
        vg(b1, n1)
        vg(b2, n2)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    ve(b1, n1)  # the eager chain: the same calls, launch by launch
    ve(b2, n2)
    assert reads == []
    assert vg.result()["batches"] == ve.result()["batches"] == 2
