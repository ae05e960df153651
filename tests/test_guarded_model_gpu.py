"""The whole model in guard-banded, poisoned buffers (tests/guard.py): two eager TrainStep calls
of the B = 2 deterministic module of test_train_step_gpu.py in fp32 and bf16, and one fp32
predict with the incremental decoder on.  Each runs unguarded, under fill A (0xFF) and under
fill B (0x7F); under the guard the parameters and buffers, the flat optimizer buffers and the
batch live in arenas, as does everything the step allocates.  Every band must stay clean, and the
loss, every parameter after each step, every BatchNorm running statistic and every parameter
gradient of the first step must be bitwise equal across the three runs: each launch of the step
is checked at the argument set the model really gives it.  The second call takes Adam's
second-step path and updates running statistics that are no longer at their initial values."""
import pytest
import torch

import guard
from test_guarded_ops_gpu import STATS, _put, run_guarded

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _report(family):
    n, nbytes = STATS[family]
    print(f"guarded {family}: {n} allocations, {nbytes} payload bytes over the fill A and B passes")


def _module():
    import test_train_step_gpu as tts
    from e2ep_amd import synthetic
    noise = _put(synthetic.target_noise(2, seed=7))
    mod = tts._module(noise)  # under the guard its .to("cuda") lands every tensor in an arena
    if guard.active() is not None:
        assert all(guard.owns(t) for t in list(mod.parameters()) + list(mod.buffers()))
    return mod, tts._batch(2), noise


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_two_train_steps(prec):
    from e2ep_amd import precision
    from e2ep_amd.train import TrainStep

    def fn():
        mod, batch, _ = _module()
        out = {}
        with precision.use(prec):
            step = TrainStep(mod, batch, graph=False)
            if guard.active() is not None:
                opt = step.opt
                assert all(guard.owns(t) for t in (opt.flat, opt.exp_avg, opt.exp_avg_sq, opt.step_count))
                assert all(guard.owns(p) for p in step.params)  # views of the guarded flat buffer
                assert all(guard.owns(v) for v in batch.values() if torch.is_tensor(v) and v.is_cuda)
            for k in range(2):
                out[f"loss{k}"] = step().clone()
                if k == 0:
                    out["grads"] = {n: p.grad.clone() for n, p in mod.named_parameters() if p.grad is not None}
                    assert len(out["grads"]) > 100
                out[f"params{k}"] = {n: p.detach().clone() for n, p in mod.named_parameters()}
                out[f"buffers{k}"] = {n: b.detach().clone() for n, b in mod.named_buffers()}
            out["exp_avg"], out["exp_avg_sq"] = step.opt.exp_avg, step.opt.exp_avg_sq
        torch.cuda.synchronize()
        assert torch.isfinite(out["loss0"]).item() and torch.isfinite(out["loss1"]).item()
        assert float(out["loss0"]) != float(out["loss1"])
        assert any("running_mean" in n for n in out["buffers1"])
        return out

    run_guarded(fn, f"model_train_{prec}", strict_owns=False)
    _report(f"model_train_{prec}")


def test_predict_with_incremental_decoder():
    from e2ep_amd import ar_decode

    def fn():
        mod, batch, noise = _module()
        m = mod.parking_model.eval()
        data = {**batch, "gt_control": batch["gt_control"][:, :1]}
        old, ar_decode._DECODE_CACHE[0] = ar_decode._DECODE_CACHE[0], True
        try:
            n0 = ar_decode.LAUNCHES[0]
            with torch.no_grad():
                tok, seg, depth, tgt = m.predict(data, noise)
            assert ar_decode.LAUNCHES[0] > n0  # the incremental path ran
        finally:
            ar_decode._DECODE_CACHE[0] = old
        torch.cuda.synchronize()
        assert tok.shape == (2, 4)
        return {"tokens": tok, "segmentation": seg, "depth": depth, "target": tgt}

    run_guarded(fn, "model_predict", strict_owns=False)
    _report("model_predict")
