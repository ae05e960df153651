"""The augmented frame decode (csrc/decode.hip k_decode_frames_aug, e2ep_frame_gray_mean) and
GpuFrameLoader(augment=...) against the NumPy statement tests/augment_ref.py.

Bit-exact bar: every step of the augmentation is an integer hash or one IEEE-rounded fp32
operation in a fixed order, and the pivot an exact integer sum rounded once from float64, so
the kernel's image must equal the reference's bit for bit; depth is the plain decode's."""
import numpy as np
import pytest
import torch

import augment_ref as R
import carla_fixture
import guard

pytestmark = pytest.mark.gpu
DEV = "cuda"

STRONG = dict(brightness=0.8, contrast=0.8, saturation=0.8, noise=0.3, gray_p=0.5)
ALONE = [dict(brightness=0.8), dict(contrast=0.8), dict(saturation=0.8), dict(noise=0.3),
         dict(gray_p=1.0), dict(noise=0.5, gray_p=0.5)]


def _ref_kw(aug, epoch):
    return dict(seed=aug.seed, epoch=epoch, B=aug.brightness, C=aug.contrast, S=aug.saturation,
                noise=aug.noise, gray_p=aug.gray_p)


def _frames(frames, side, seed):
    g = np.random.default_rng(seed)
    rgb = g.integers(0, 256, (frames, side, side, 3), dtype=np.uint8)
    drgb = g.integers(0, 256, (frames, side, side, 3), dtype=np.uint8)
    return rgb, drgb


def _bits(a, b):
    """Bitwise equality of two tensors (torch.equal on the raw words: a NaN or a -0 counts)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(
        a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _decode(rgb, drgb, src, keys, aug, epoch, exact_outputs=False):
    """The augmented decode of numpy frames; inputs through guard.put (a plain copy outside a
    guard context), outputs from torch.empty at exact size when asked."""
    from e2ep_amd import decode
    F = len(src) if src is not None else rgb.shape[0]
    H, W = rgb.shape[1:3]
    out = {}
    if exact_outputs:
        out = dict(out_image=torch.empty(F, 3, H, W, device=DEV),
                   out_depth=torch.empty(F, H, W, dtype=torch.float64, device=DEV))
    img, dep = decode.decode_frames(guard.put(torch.from_numpy(rgb)),
                                    guard.put(torch.from_numpy(drgb)),
                                    src_frame=None if src is None else torch.tensor(src),
                                    augment=aug, epoch=epoch,
                                    frame_key=None if keys is None else torch.tensor(keys), **out)
    return img, dep


def _check_case(rgb, drgb, src, keys, aug, epoch):
    from e2ep_amd import decode
    img, dep = _decode(rgb, drgb, src, keys, aug, epoch)
    sel = rgb if src is None else rgb[src]
    ref_keys = keys if keys is not None else (src if src is not None else range(len(rgb)))
    want = torch.from_numpy(R.augment_frames(sel, ref_keys, **_ref_kw(aug, epoch)))
    assert img.dtype == torch.float32 and _bits(img.cpu(), want)
    _, plain = decode.decode_frames(None, torch.from_numpy(drgb).to(DEV),
                                    src_frame=None if src is None else torch.tensor(src))
    assert _bits(dep, plain)


# (frames, side, source table, keys): one quad; a ragged last block with several frames in
# one block; a gathered table with repeats and keys that are negative and beyond 2^32; many
# blocks per frame
SHAPES = [
    (3, 2, None, None),
    (3, 20, None, [7, 1, 2 ** 40 + 3]),
    (12, 64, [11, 0, 5, 5, 3], None),
    (12, 64, [11, 0, 5, 5, 3], [100, -7, 2 ** 40, 5, 6]),
    (5, 512, None, None),
]


@pytest.mark.parametrize("frames,side,src,keys", SHAPES)
def test_augmented_decode_bitwise(frames, side, src, keys):
    from e2ep_amd.augment import PhotoAugment
    rgb, drgb = _frames(frames, side, frames * side)
    _check_case(rgb, drgb, src, keys, PhotoAugment(seed=3, **STRONG), epoch=2)


@pytest.mark.parametrize("strengths", ALONE, ids=lambda d: "+".join(d))
def test_each_effect_alone_bitwise(strengths):
    from e2ep_amd.augment import PhotoAugment
    rgb, drgb = _frames(6, 20, 11)
    keys = list(range(4, 10))     # at seed 1, epoch 0, gray_p 0.5: keys 6, 7, 8 draw grey
    assert [float(R.factors(1, 0, k, gray_p=0.5)[2]) for k in keys] == [1, 1, 0, 0, 0, 1]
    _check_case(rgb, drgb, None, keys, PhotoAugment(seed=1, **strengths), epoch=0)


def test_constant_frames_bitwise():
    """All 0 (pivot 0), all 255 (pivot 1) and one constant colour (saturation a no-op)."""
    from e2ep_amd.augment import PhotoAugment
    rgb, drgb = _frames(3, 20, 5)
    rgb[0], rgb[1], rgb[2] = 0, 255, np.array([200, 30, 90], dtype=np.uint8)
    for epoch in (0, 1):
        _check_case(rgb, drgb, None, None, PhotoAugment(**STRONG), epoch)
    _check_case(rgb, drgb, None, None, PhotoAugment(contrast=1.0), 0)
    _check_case(rgb, drgb, None, None, PhotoAugment(saturation=1.0, gray_p=0.5), 0)


@pytest.mark.parametrize("frames,side,src", [(3, 2, None), (3, 20, None),
                                             (12, 64, [11, 0, 5, 5, 3]), (3, 256, [2, 0, 2])])
def test_frame_gray_mean_exact(frames, side, src):
    from e2ep_amd import decode
    rgb, _ = _frames(frames, side, 17 * side)
    rgb[0] = 255                     # the largest sums a frame of this size can have
    if frames > 2:
        rgb[2] = 0
    sums, mean = decode.frame_gray_mean(torch.from_numpy(rgb).to(DEV),
                                        None if src is None else torch.tensor(src))
    sel = rgb if src is None else rgb[src]
    assert sums.dtype == torch.int64 and mean.dtype == torch.float32
    assert torch.equal(sums.cpu(), torch.from_numpy(R.channel_sums(sel)))
    assert _bits(mean.cpu(), torch.from_numpy(R.gray_mean(sel)))
    if side == 256:
        assert sums[1].tolist() == [255 * 256 * 256] * 3 and float(mean[1]) == 1.0


@pytest.mark.parametrize("frames,side,src", [(3, 20, None), (12, 64, [11, 0, 5, 5, 3])])
def test_zero_strength_is_plain_decode(frames, side, src):
    from e2ep_amd import decode
    from e2ep_amd.augment import PhotoAugment
    rgb, drgb = _frames(frames, side, 23)
    rgb[0, 0, :4] = [[0, 0, 0], [255, 255, 255], [0, 255, 0], [1, 254, 128]]
    t, d = torch.from_numpy(rgb).to(DEV), torch.from_numpy(drgb).to(DEV)
    s = None if src is None else torch.tensor(src)
    img0, dep0 = decode.decode_frames(t, d, src_frame=s)
    for epoch in (0, 5):
        img, dep = decode.decode_frames(t, d, src_frame=s, augment=PhotoAugment(seed=4),
                                        epoch=epoch)
        assert _bits(img, img0) and _bits(dep, dep0)


@pytest.mark.parametrize("fill", [guard.FILL_A, guard.FILL_B], ids=["ff", "7f"])
def test_augmented_decode_in_guarded_buffers(fill):
    from e2ep_amd import decode
    from e2ep_amd.augment import PhotoAugment
    aug = PhotoAugment(seed=3, **STRONG)
    cases = [s for s in SHAPES if s[1] <= 64]
    plain = [_decode(*_frames(f, side, f * side), src, keys, aug, 2)
             for f, side, src, keys in cases]
    with guard.allocations(fill) as g:
        got = [_decode(*_frames(f, side, f * side), src, keys, aug, 2, exact_outputs=True)
               for f, side, src, keys in cases]
        rgb, _ = _frames(3, 20, 9)
        gm = decode.frame_gray_mean(guard.put(torch.from_numpy(rgb)), torch.tensor([2, 0]))
        assert all(guard.owns(t) for pair in got for t in pair) and guard.owns(gm[0])
        g.check()
    for (img, dep), (img0, dep0) in zip(got, plain):
        assert _bits(img, img0) and _bits(dep, dep0)
    assert torch.equal(gm[0].cpu(), torch.from_numpy(R.channel_sums(rgb[[2, 0]])))
    assert _bits(gm[1].cpu(), torch.from_numpy(R.gray_mean(rgb[[2, 0]])))


def test_bad_arguments_raise_before_any_launch():
    from e2ep_amd import _lib, decode
    from e2ep_amd.augment import PhotoAugment
    aug = PhotoAugment(brightness=0.5)
    rgb = torch.zeros(2, 6, 6, 3, dtype=torch.uint8, device=DEV)
    bad = [
        dict(rgb=rgb, augment=aug, frame_key=torch.tensor([0, 1, 2])),          # wrong length
        dict(rgb=rgb, augment=aug, src_frame=torch.tensor([1]), frame_key=torch.tensor([0, 1])),
        dict(rgb=rgb, augment=aug, frame_key=torch.tensor([0, 1], device=DEV)),  # device table
        dict(rgb=rgb, augment=aug, frame_key=torch.tensor([0., 1.])),            # not int64
        dict(depth_rgb=rgb, augment=aug),                                        # no rgb
        dict(rgb=rgb, frame_key=torch.tensor([0, 1])),                           # no augment
        dict(rgb=rgb, augment=dict(brightness=0.5)),                             # not a PhotoAugment
    ]
    for kw in bad:
        with pytest.raises(_lib.E2EPError):
            decode.decode_frames(**kw)
    for kw in (dict(brightness=1.5), dict(contrast=-0.1), dict(saturation=2), dict(noise=0.6),
               dict(gray_p=1.1)):
        with pytest.raises(_lib.E2EPError):
            PhotoAugment(**kw)
    # the C entry point checks the ranges itself, before its launch
    img = torch.empty(2, 3, 6, 6, device=DEV)
    key = torch.zeros(2, dtype=torch.int64, device=DEV)
    mean = torch.zeros(2, device=DEV)
    for strengths in ((1.5, 0, 0, 0, 0), (0, -0.5, 0, 0, 0), (0, 0, 0, 0.6, 0),
                      (0, 0, 0, 0, float("nan"))):
        with pytest.raises(_lib.E2EPError):
            _lib.call("e2ep_decode_frames_aug", _lib.ptr(rgb), None, None, _lib.ptr(key), 2, 36,
                      _lib.ptr(mean), 0, *strengths, _lib.ptr(img), None, _lib.stream())


# ---- the loader ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mini(tmp_path_factory):
    from dataset.carla_dataset import CarlaDataset
    from dataset.frame_cache import build_frame_cache
    d = str(tmp_path_factory.mktemp("carla"))
    carla_fixture.make_dataset(d, frames=16)
    cfg = carla_fixture.config(d, batch_size=4)
    ds = CarlaDataset(d, 1, cfg)
    cache = build_frame_cache(ds, str(tmp_path_factory.mktemp("fc")))
    return ds, cache


def _aug():
    from e2ep_amd.augment import PhotoAugment
    return PhotoAugment(brightness=0.4, contrast=0.4, saturation=0.4, noise=0.05, gray_p=0.25,
                        seed=7)


def _images(cache, batch_size, epoch=0, augment="default", **kw):
    """sample index -> that sample's (4, 3, C, C) image on the host, over one epoch."""
    from dataset.frame_cache import GpuFrameLoader
    loader = GpuFrameLoader(cache, batch_size, drop_last=False, seed=5,
                            augment=_aug() if augment == "default" else augment, **kw)
    loader.set_epoch(epoch)
    out = {}
    for batch, idx in zip(loader, loader.batches()):   # the loader first: zip exhausts it
        for i, img in zip(idx.tolist(), batch["image"].cpu()):
            out[i] = img
    return out


@pytest.fixture(scope="module")
def base_images(mini):
    return _images(mini[1], 4, shuffle=False, resident=False)


def _same(a, b):
    return sorted(a) == sorted(b) and all(_bits(a[i], b[i]) for i in a)


def test_loader_images_equal_the_reference(mini, base_images):
    _, cache = mini
    aug = _aug()
    assert sorted(base_images) == list(range(len(cache)))
    for i in (0, len(cache) - 1):
        want = R.augment_frames(np.asarray(cache.arrays["rgb"][i]), [4 * i + c for c in range(4)],
                                **_ref_kw(aug, 0))
        assert _bits(base_images[i], torch.from_numpy(want))


@pytest.mark.parametrize("kw", [dict(batch_size=3, shuffle=False, resident=False),
                                dict(batch_size=4, shuffle=True, resident=False),
                                dict(batch_size=4, shuffle=False, resident=True),
                                dict(batch_size=3, shuffle=True, resident=True)],
                         ids=["batch3", "shuffled", "resident", "all"])
def test_loader_images_depend_on_the_sample_alone(mini, base_images, kw):
    assert _same(_images(mini[1], **kw), base_images)


def test_loader_images_across_ranks(mini, base_images):
    _, cache = mini
    assert len(cache) % 2 == 0       # no padded duplicate on either rank
    halves = [_images(cache, 4, shuffle=True, resident=False, rank=r, world=2) for r in (0, 1)]
    assert not set(halves[0]) & set(halves[1])
    assert _same({**halves[0], **halves[1]}, base_images)
    assert _same(_images(cache, 4, shuffle=True, resident=False, rank=0, world=1), base_images)


def test_loader_epochs_differ_and_per_camera(mini, base_images):
    from e2ep_amd.augment import PhotoAugment
    _, cache = mini
    e1 = _images(cache, 4, epoch=1, shuffle=False, resident=False)
    assert all(not torch.equal(e1[i], base_images[i]) for i in base_images)
    assert _same(_images(cache, 4, epoch=0, shuffle=False, resident=True), base_images)
    shared = PhotoAugment(brightness=0.4, per_camera=False, seed=7)
    got = _images(cache, 4, augment=shared, shuffle=False, resident=True)
    want = R.augment_frames(np.asarray(cache.arrays["rgb"][3]), [12] * 4, **_ref_kw(shared, 0))
    assert _bits(got[3], torch.from_numpy(want))


@pytest.mark.parametrize("resident", [False, True])
def test_loader_leaves_everything_else_alone(mini, resident):
    from dataset.frame_cache import GpuFrameLoader
    _, cache = mini
    kw = dict(shuffle=True, drop_last=False, seed=5, resident=resident)
    plain = GpuFrameLoader(cache, 3, **kw)
    jit = GpuFrameLoader(cache, 3, augment=_aug(), **kw)
    n = 0
    jit_it = iter(jit)
    for a in plain:
        b = next(jit_it)
        assert sorted(a) == sorted(b)
        for k in a:
            assert b[k].is_cuda == (k not in ("intrinsics", "extrinsics")), k  # rig on the host
            assert b[k].dtype == a[k].dtype and b[k].shape == a[k].shape, k
            if k == "image":
                assert not torch.equal(a[k], b[k])
            else:
                assert torch.equal(a[k], b[k]), k
        n += 1
    assert next(jit_it, None) is None and n == len(plain)


def test_augmented_batch_trains_a_step(mini):
    from dataset.frame_cache import GpuFrameLoader
    from trainer.pl_trainer import ParkingTrainingModule
    ds, cache = mini
    it = iter(GpuFrameLoader(cache, 2, shuffle=False, augment=_aug()))
    batch = next(it)
    it.close()
    module = ParkingTrainingModule(ds.cfg).to(DEV)
    module.train()
    loss = module.training_step(batch, 0)
    assert torch.isfinite(loss)
    loss.backward()
