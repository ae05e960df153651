"""Photometric augmentation of the GPU frame decode (csrc/decode.hip k_decode_frames_aug).

PhotoAugment names the strengths of a per-frame colour jitter that the decode kernel applies
in registers between the / 255 and the ImageNet normalisation: brightness, contrast,
saturation (or full grey with probability gray_p) and per-pixel uniform noise.  Every draw is
a splitmix64 hash of (seed, epoch, frame key, pixel), so a sample's augmented image depends
on (augment, epoch, sample index) alone: not on batch size, shuffle order, resident or
streamed loading, rank or world size.  The rig, the depth and every label are untouched.

Deviation from torchvision.transforms.ColorJitter: the contrast pivot is the grey mean of the
*unjittered* source frame (torchvision pivots on the brightness-adjusted image), which makes
it an exact, order-free integer reduction (e2ep_frame_gray_mean); and the four effects are
always applied in the order brightness, contrast, saturation, noise (torchvision permutes
them and has no noise)."""
import dataclasses
import numbers

from ._lib import E2EPError

_M64 = (1 << 64) - 1


def mix64(z):
    """The splitmix64 finaliser of csrc/mix64.h on Python ints; mix64(0) == 0xE220A8397B1DCDAF."""
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


@dataclasses.dataclass(frozen=True)
class PhotoAugment:
    """brightness / contrast / saturation in [0, 1]: the factor is uniform on [1 - v, 1 + v].
    noise in [0, 0.5]: amplitude of uniform per-pixel, per-channel noise on the [0, 1] image.
    gray_p in [0, 1]: probability that a frame loses all saturation.  per_camera: every camera
    of a sample draws its own factors (False: one sample's cameras share them).  seed: the
    stream of draws."""
    brightness: float = 0.
    contrast: float = 0.
    saturation: float = 0.
    noise: float = 0.
    gray_p: float = 0.
    per_camera: bool = True
    seed: int = 0

    def __post_init__(self):
        for name, hi in (("brightness", 1.), ("contrast", 1.), ("saturation", 1.),
                         ("noise", .5), ("gray_p", 1.)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, numbers.Real) or not 0. <= v <= hi:
                raise E2EPError(f"PhotoAugment: {name} must lie in [0, {hi}], got {v!r}")
            object.__setattr__(self, name, float(v))
        if isinstance(self.seed, bool) or not isinstance(self.seed, numbers.Integral):
            raise E2EPError(f"PhotoAugment: seed must be an int, got {self.seed!r}")
        object.__setattr__(self, "per_camera", bool(self.per_camera))

    @property
    def active(self):
        """False when every strength is zero (the augmented decode is then the plain one)."""
        return any((self.brightness, self.contrast, self.saturation, self.noise, self.gray_p))

    def base(self, epoch):
        """mix64(seed ^ mix64(epoch)) as the uint64 the kernel adds each frame's key to."""
        return mix64((self.seed & _M64) ^ mix64(int(epoch) & _M64))

    def frame_keys(self, sample_index, cams):
        """int64 keys of the cams frames of each sample, sample-major: sample * cams + cam, or
        sample * cams for all of a sample's cameras when per_camera is off."""
        import torch
        idx = torch.as_tensor(sample_index, dtype=torch.int64).reshape(-1, 1) * cams
        if self.per_camera:
            return (idx + torch.arange(cams)).reshape(-1)
        return idx.expand(-1, cams).reshape(-1)
