"""ValStep(depth_metrics=True) on MI355X: the feature leaves every other result of the step as
it is, its numbers are tests/depth_ref.py's on the step's own pred_depth and the batch's depth
(counts and maps exact; sums within 1e-9 relative, the bound derived in
test_depth_metrics_gpu.py), the captured chain equals the eager one bit for bit, a call reads
nothing back, and the data-parallel merge in a world of one rank changes nothing."""
import warnings

import numpy as np
import pytest
import torch

import depth_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
RIG = ("intrinsics", "extrinsics")
RATIOS = ("depth_bin_acc", "depth_bin_within1", "depth_bin_mae", "depth_delta125", "depth_abs_err",
          "depth_rmse", "depth_abs_rel", "depth_exp_abs_err", "depth_exp_rmse",
          "depth_true_bin_prob")


def _batch(b, seed):
    from e2ep_amd import synthetic
    d = synthetic.synthetic_batch(b, seed=seed)
    data = {k: (v if k in RIG else v.to(DEV)) for k, v in d.items()}
    return data, synthetic.target_noise(b, seed=seed).to(DEV)


def _host(ts):
    return [t.cpu().numpy().copy() for t in ts]


@pytest.fixture(scope="module")
def steps():
    """A captured and an eager ValStep with the depth metrics and an eager one without, over
    one module, fed the same three calls (two batches, the second twice)."""
    from trainer.pl_trainer import ParkingTrainingModule
    from tool.config import default_cfg
    from weights import make_state
    from e2ep_amd.val import ValStep
    mod = ParkingTrainingModule(default_cfg(deterministic=True))
    mod.parking_model.load_state_dict(make_state(mod.parking_model.state_dict(), 1234))
    mod = mod.to(DEV).eval()
    (b1, n1), (b2, n2) = _batch(2, 7), _batch(2, 8)
    vg = ValStep(mod, b1, noise=n1, graph=True, warmup=2, depth_metrics=True, depth_maps=True)
    ve = ValStep(mod, b1, noise=n1, graph=False, depth_metrics=True, depth_maps=True)
    v0 = ValStep(mod, b1, noise=n1, graph=False)
    assert vg._graph is not None and ve._graph is None
    r = vg.result()
    assert r["batches"] == 0 and r["depth_cells"] == 0  # warm-up and capture accumulate nothing
    assert ValStep.unpack_depth(vg.packed_depth.cpu().numpy())[2] == 0
    calls = []
    for b, n in ((b1, n1), (b2, n2), (b2, n2)):
        c = dict(loss_graph=vg(b, n).clone().cpu().numpy())
        c["out_graph"], c["maps_graph"] = vg.depth_out.cpu().numpy().copy(), _host(vg.depth_maps)
        c["loss_eager"] = ve(b, n).clone().cpu().numpy()
        c["out_eager"], c["maps_eager"] = ve.depth_out.cpu().numpy().copy(), _host(ve.depth_maps)
        c["prob"] = ve.pred[2].cpu().numpy().copy()
        c["depth"] = b["depth"].cpu().numpy().copy()
        c["loss_plain"] = v0(b, n).clone().cpu().numpy()
        calls.append(c)
    return mod, vg, ve, v0, calls, (b1, n1), (b2, n2)


def test_the_feature_leaves_the_other_results_as_they_are(steps):
    from e2ep_amd.val import KEYS
    _, vg, ve, v0, calls, _, _ = steps
    for c in calls:
        assert c["loss_eager"].tobytes() == c["loss_plain"].tobytes()
        assert np.isfinite(c["loss_plain"])
    assert ve.packed.cpu().numpy().tobytes() == v0.packed.cpu().numpy().tobytes()
    assert vg.packed.cpu().numpy().tobytes() == v0.packed.cpu().numpy().tobytes()
    with_, without = ve.result(), v0.result()
    assert without["batches"] == with_["batches"] == 3
    for k in KEYS + ("seg_miou",):
        assert with_[k] == without[k], k
    assert np.array_equal(with_["seg_confusion"], without["seg_confusion"])
    # off: no depth key beyond the loss, no second buffer, nothing kept
    assert [k for k in without if k.startswith("depth")] == ["depth_val_loss"]
    assert set(with_) - set(without) == set(RATIOS) | {"depth_cells", "depth_per_camera"}
    assert v0.packed_depth is None and v0.depth_out is None and v0.depth_maps is None
    assert v0._buf.numel() == v0.packed.numel() == 48 + 8 * 9


def _rel(got, want):
    return abs(got - want) / abs(want)


def test_depth_results_equal_the_reference_on_the_steps_own_tensors(steps):
    from e2ep_amd.val import ValStep
    mod, _, ve, _, calls, _, _ = steps
    d_bound, down = mod.cfg.d_bound, mod.cfg.bev_down_sample
    total_s, total_c = np.zeros((4, 6)), np.zeros((4, 5), dtype=np.int64)
    for i, c in enumerate(calls):
        B, N, H, W = c["depth"].shape
        assert (B, N) == (2, 4) and c["prob"].shape == (8, 48, H // down, W // down)
        ref = depth_ref.depth_metrics(c["prob"], c["depth"].reshape(B * N, H, W), d_bound, down, N)
        assert (ref["counts"][:, 0] >= 2 * 100).all()  # every image has foreground cells
        sums, counts, batches = ValStep.unpack_depth(c["out_eager"])
        assert batches is None
        assert np.array_equal(counts, ref["counts"]), (counts, ref["counts"])
        rel = np.abs(sums - ref["sums"]) / np.abs(ref["sums"])
        print(f"call {i}: cells {counts[:, 0].tolist()} hits {counts[:, 1].tolist()}, largest "
              f"relative error of a sum {rel.max():.3e}")
        assert (rel < 1e-9).all(), (sums, ref["sums"])
        pm, gm, cls = c["maps_eager"]
        assert pm.tobytes() == ref["pred_map"].tobytes()
        assert gm.tobytes() == ref["gt_map"].tobytes()
        assert np.array_equal(cls, ref["cls"])
        total_s, total_c = total_s + ref["sums"], total_c + ref["counts"]
    r = ve.result()
    pc = r["depth_per_camera"]
    assert np.array_equal(pc["depth_cells"], total_c[:, 0])
    assert r["depth_cells"] == total_c[:, 0].sum()
    cells = total_c[:, 0].astype(np.float64)
    assert np.array_equal(pc["depth_bin_acc"], total_c[:, 1] / cells)
    assert np.array_equal(pc["depth_bin_within1"], total_c[:, 2] / cells)
    assert np.array_equal(pc["depth_bin_mae"], total_c[:, 3] / cells)
    assert np.array_equal(pc["depth_delta125"], total_c[:, 4] / cells)
    want = {"depth_abs_err": total_s[:, 0] / cells, "depth_rmse": np.sqrt(total_s[:, 1] / cells),
            "depth_abs_rel": total_s[:, 2] / cells, "depth_exp_abs_err": total_s[:, 3] / cells,
            "depth_exp_rmse": np.sqrt(total_s[:, 4] / cells),
            "depth_true_bin_prob": total_s[:, 5] / cells}
    for k, v in want.items():
        assert (np.abs(pc[k] - v) / np.abs(v) < 1e-9).all(), (k, pc[k], v)
    assert r["depth_bin_acc"] == total_c[:, 1].sum() / cells.sum()
    assert _rel(r["depth_abs_err"], total_s[:, 0].sum() / cells.sum()) < 1e-9
    assert _rel(r["depth_exp_rmse"], np.sqrt(total_s[:, 4].sum() / cells.sum())) < 1e-9


def test_captured_equals_eager_bit_for_bit(steps):
    _, vg, ve, _, calls, _, _ = steps
    for c in calls:
        assert c["loss_graph"].tobytes() == c["loss_eager"].tobytes()
        assert c["out_graph"].tobytes() == c["out_eager"].tobytes()
        for a, b in zip(c["maps_graph"], c["maps_eager"]):
            assert a.tobytes() == b.tobytes()
    assert calls[0]["out_graph"].tobytes() != calls[1]["out_graph"].tobytes()
    assert calls[1]["out_graph"].tobytes() == calls[2]["out_graph"].tobytes()
    assert vg.packed_depth.cpu().numpy().tobytes() == ve.packed_depth.cpu().numpy().tobytes()
    rg, re_ = vg.result(), ve.result()
    assert rg.keys() == re_.keys()
    for k in rg:
        if k == "depth_per_camera":
            assert rg[k].keys() == re_[k].keys()
            for kk in rg[k]:
                assert rg[k][kk].tobytes() == re_[k][kk].tobytes(), kk
        else:
            assert np.array_equal(np.asarray(rg[k]), np.asarray(re_[k]), equal_nan=True), k


def test_merge_over_a_world_of_one_changes_nothing(steps):
    import torch.distributed as dist
    from e2ep_amd.val import ValStep
    _, _, ve, _, _, _, _ = steps
    plain = ve.result()
    dist.init_process_group("gloo", store=dist.HashStore(), rank=0, world_size=1)
    try:
        packed, packed_depth = ve._merge_all()
        assert ve._merge().tobytes() == packed.tobytes()
    finally:
        torch.cuda.synchronize()
        dist.destroy_process_group()
    assert packed_depth.tobytes() == ve.packed_depth.cpu().numpy().tobytes()
    merged = ValStep.finish(packed)
    merged.update(ValStep.finish_depth(packed_depth))
    assert merged.keys() == plain.keys() and merged["batches"] == plain["batches"] >= 3
    for k, v in plain.items():
        if k == "depth_per_camera":
            for kk in v:
                assert merged[k][kk].tobytes() == v[kk].tobytes(), kk
        else:
            assert np.array_equal(np.asarray(merged[k]), np.asarray(v), equal_nan=True), k


def test_calls_do_not_synchronise_and_reset_zeroes_both_buffers(steps, monkeypatch):
    """Runs last: it resets the fixture's steps."""
    from e2ep_amd.val import ValStep
    _, vg, ve, _, _, (b1, n1), (b2, n2) = steps
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
    monkeypatch.undo()
    rg, re_ = vg.result(), ve.result()
    assert rg["batches"] == re_["batches"] == 2
    assert rg["depth_cells"] == re_["depth_cells"] > 0
    assert ValStep.unpack_depth(vg.packed_depth.cpu().numpy())[2] == 2
    vg.reset()
    r = vg.result()
    assert r["batches"] == 0 and r["depth_cells"] == 0 and np.isnan(r["depth_rmse"])
    assert not vg._buf.cpu().numpy().any()
