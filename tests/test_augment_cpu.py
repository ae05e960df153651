"""The photometric augmentation's statement (tests/augment_ref.py) and its host side
(e2ep_amd/augment.py PhotoAugment, the config keys): properties that need no GPU."""
import dataclasses

import numpy as np
import pytest
import torch

import augment_ref as R

STRONG = dict(B=0.8, C=0.8, S=0.8, noise=0.3, gray_p=0.5)


def _frame(seed, side=12):
    g = np.random.default_rng(seed)
    f = g.integers(0, 256, (side, side, 3), dtype=np.uint8)
    f.reshape(-1)[:256] = np.arange(256, dtype=np.uint8)   # every byte value occurs
    return f


def test_mix64_constant():
    from e2ep_amd import augment
    assert int(R.mix64(0)) == 0xE220A8397B1DCDAF
    assert augment.mix64(0) == 0xE220A8397B1DCDAF
    for z in (1, 2 ** 63, 2 ** 64 - 1, 0x0123456789ABCDEF):
        assert augment.mix64(z) == int(R.mix64(np.uint64(z)))


def test_host_base_equals_reference():
    from e2ep_amd.augment import PhotoAugment
    for seed, epoch in ((0, 0), (42, 3), (-1, 7), (2 ** 40 + 5, 2 ** 33)):
        assert PhotoAugment(seed=seed).base(epoch) == int(R.base_of(seed, epoch))


def test_zero_strength_is_normalise_image():
    from dataset.carla_dataset import normalise_image
    f = _frame(0, side=20)
    for key in (0, 5, -3):
        got = R.augment_frame(f, key, seed=9, epoch=2)
        assert np.array_equal(got.view(np.uint32), normalise_image(f).numpy().view(np.uint32))


@pytest.mark.parametrize("per_frame", [(0, 0, 0), (255, 255, 255), (200, 30, 90)])
def test_zero_strength_constant_frames(per_frame):
    from dataset.carla_dataset import normalise_image
    f = np.broadcast_to(np.array(per_frame, dtype=np.uint8), (4, 4, 3)).copy()
    got = R.augment_frame(f, 1)
    assert np.array_equal(got.view(np.uint32), normalise_image(f).numpy().view(np.uint32))


def test_factor_ranges():
    B, C, S = 0.8, 0.5, 0.25
    fac = np.array([R.factors(3, 1, k, B, C, S, 0.) for k in range(500)], dtype=np.float64)
    for col, v in enumerate((B, C, S)):
        lo, hi = np.float32(1) - np.float32(v), np.float32(1) + np.float32(v)
        assert fac[:, col].min() >= lo and fac[:, col].max() <= hi
        assert fac[:, col].min() < 1 - v / 2 and fac[:, col].max() > 1 + v / 2  # they do spread
    grey = np.array([R.factors(3, 1, k, B, C, S, 0.5)[2] for k in range(500)])
    assert 150 < (grey == 0).sum() < 350
    assert all(R.factors(3, 1, k, B, C, S, 1.0)[2] == 0 for k in range(20))


def test_output_range():
    lo, hi = (np.float32(0) - R.MEAN) / R.STD, (np.float32(1) - R.MEAN) / R.STD
    for key in range(6):
        out = R.augment_frame(_frame(key), key, seed=1, epoch=0, **STRONG)
        assert out.dtype == np.float32 and np.isfinite(out).all()
        for c in range(3):
            assert out[c].min() >= lo[c] and out[c].max() <= hi[c]
    # the clamps do fire at these strengths
    out = np.stack([R.augment_frame(_frame(k), k, **STRONG) for k in range(6)])
    assert (out[:, 0] == lo[0]).any() and (out[:, 0] == hi[0]).any()


def test_draws_depend_on_key_epoch_seed():
    a = R.factors(1, 2, 3, 0.8, 0.8, 0.8)
    assert a == R.factors(1, 2, 3, 0.8, 0.8, 0.8)
    assert a != R.factors(1, 2, 4, 0.8, 0.8, 0.8)
    assert a != R.factors(1, 3, 3, 0.8, 0.8, 0.8)
    assert a != R.factors(2, 2, 3, 0.8, 0.8, 0.8)
    f = _frame(0)
    x = R.augment_frame(f, 3, seed=1, epoch=2, noise=0.3)
    assert np.array_equal(x, R.augment_frame(f, 3, seed=1, epoch=2, noise=0.3))
    assert not np.array_equal(x, R.augment_frame(f, 3, seed=1, epoch=3, noise=0.3))


def test_per_camera_keys():
    from e2ep_amd.augment import PhotoAugment
    idx = torch.tensor([5, 0, 9])
    own = PhotoAugment(brightness=0.5).frame_keys(idx, 4)
    assert own.dtype == torch.int64
    assert own.tolist() == [20, 21, 22, 23, 0, 1, 2, 3, 36, 37, 38, 39]
    shared = PhotoAugment(brightness=0.5, per_camera=False).frame_keys(idx, 4)
    assert shared.tolist() == [20] * 4 + [0] * 4 + [36] * 4
    fac = [R.factors(0, 0, int(k), 0.8, 0.8, 0.8, 0.5) for k in shared]
    assert fac[0] == fac[1] == fac[2] == fac[3] and fac[4] == fac[7] and fac[0] != fac[4]
    fac = [R.factors(0, 0, int(k), 0.8, 0.8, 0.8, 0.5) for k in own]
    assert len(set(fac)) == 12


def test_photo_augment_validates_and_is_immutable():
    from e2ep_amd._lib import E2EPError
    from e2ep_amd.augment import PhotoAugment
    a = PhotoAugment()
    assert dataclasses.asdict(a) == dict(brightness=0., contrast=0., saturation=0., noise=0.,
                                         gray_p=0., per_camera=True, seed=0)
    assert not a.active and PhotoAugment(noise=0.1).active and PhotoAugment(gray_p=1).active
    with pytest.raises(dataclasses.FrozenInstanceError):
        a.brightness = 0.5
    PhotoAugment(brightness=1, contrast=1., saturation=1., noise=0.5, gray_p=1.)
    for bad in (dict(brightness=-0.1), dict(brightness=1.01), dict(contrast=2), dict(saturation=-1),
                dict(noise=0.51), dict(noise=-0.01), dict(gray_p=1.5), dict(gray_p=-0.5),
                dict(brightness=float("nan")), dict(contrast="0.5"), dict(noise=True),
                dict(seed=1.5)):
        with pytest.raises(E2EPError):
            PhotoAugment(**bad)


def test_config_keys_build_the_augment():
    from dataset.dataloader import ParkingDataModule
    from tool.config import default_cfg
    assert ParkingDataModule(default_cfg(data_dir="x"))._augment() is None
    cfg = default_cfg(data_dir="x", augment_brightness=0.4, augment_gray_p=0.1,
                      augment_per_camera=False)
    aug = ParkingDataModule(cfg)._augment()
    assert (aug.brightness, aug.contrast, aug.gray_p, aug.per_camera) == (0.4, 0., 0.1, False)
