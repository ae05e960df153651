"""NumPy statement of the photometric augmentation of the frame decode (test infrastructure).

The function the kernel csrc/decode.hip k_decode_frames_aug restates, of
(seed, epoch, frame key, pixel, bytes):

  Draws.  mix64 is the splitmix64 finaliser (csrc/mix64.h).  base = mix64(seed ^ mix64(epoch)).
  A frame with int64 key `key` has fh = mix64(base + key); parameter j draws
  u_j = float(mix64(fh + j) >> 40) * 2^-24 (j = 0 brightness, 1 contrast, 2 saturation, 3 grey).
  Factors, fp32, every operation rounded: b = 1 + B (2 u0 - 1), c = 1 + C (2 u1 - 1),
  s = 1 + S (2 u2 - 1), s = 0 when u3 < gray_p.
  Pivot.  m = float32((0.299 sumR + 0.587 sumG + 0.114 sumB) / (255 hw)) from the exact integer
  channel sums of the *unjittered* frame, evaluated in float64, rounded once.
  Per pixel, fp32, no contraction, x_c = float(byte_c) / 255, clamp(x) = min(max(x, 0), 1):
    1. x_c = clamp(x_c b)
    2. x_c = clamp(c x_c + k),  k = (1 - c) m
    3. g = (0.299 x_R + 0.587 x_G) + 0.114 x_B;  x_c = clamp(s x_c + (1 - s) g)
    4. h = mix64(fh ^ mix64(p)), p the pixel's index within its frame; channel c draws
       u = float((h >> 21 c) & 0x1FFFFF) * 2^-21;  x_c = clamp(x_c + a (2 u - 1))
    5. (x_c - mean_c) / std_c, the ImageNet normalisation of dataset.carla_dataset.

Deviation from torchvision's ColorJitter: the contrast pivot is the grey mean of the source
frame, not of the brightness-adjusted one."""
import numpy as np

MEAN = np.array([0.485, 0.456, 0.406], dtype=np.float32)
STD = np.array([0.229, 0.224, 0.225], dtype=np.float32)
F32 = np.float32


def mix64(z):
    """splitmix64 finaliser on uint64 scalars or arrays (wrapping arithmetic)."""
    z = np.asarray(z).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def _u64(v):
    return np.uint64(int(v) & 0xFFFFFFFFFFFFFFFF)


def base_of(seed, epoch):
    return mix64(_u64(seed) ^ mix64(_u64(epoch)))


def frame_hash(seed, epoch, key):
    with np.errstate(over="ignore"):
        return mix64(base_of(seed, epoch) + _u64(key))


def factors(seed, epoch, key, B=0., C=0., S=0., gray_p=0.):
    """(b, c, s) of one frame as np.float32."""
    fh = frame_hash(seed, epoch, key)
    with np.errstate(over="ignore"):
        u = [F32(int(mix64(fh + np.uint64(j))) >> 40) * F32(2.0 ** -24) for j in range(4)]
    one, two = F32(1), F32(2)
    b = one + F32(B) * (two * u[0] - one)
    c = one + F32(C) * (two * u[1] - one)
    s = one + F32(S) * (two * u[2] - one)
    if u[3] < F32(gray_p):
        s = F32(0)
    return F32(b), F32(c), F32(s)


def channel_sums(rgb):
    """(F, ..., 3) uint8 -> (F, 3) int64 exact sums."""
    rgb = np.asarray(rgb)
    return rgb.reshape(rgb.shape[0], -1, 3).astype(np.int64).sum(1)


def gray_mean(rgb):
    """(F, ..., 3) uint8 -> (F,) fp32: the contrast pivot."""
    s = channel_sums(rgb).astype(np.float64)
    hw = np.asarray(rgb).reshape(rgb.shape[0], -1, 3).shape[1]
    return (((0.299 * s[:, 0] + 0.587 * s[:, 1]) + 0.114 * s[:, 2]) / (255.0 * hw)).astype(F32)


def _clamp(x):
    return np.minimum(np.maximum(x, F32(0)), F32(1))


def augment_frame(rgb, key, seed=0, epoch=0, B=0., C=0., S=0., noise=0., gray_p=0.):
    """One (H, W, 3) uint8 frame -> (3, H, W) fp32, augmented and normalised."""
    rgb = np.asarray(rgb)
    H, W = rgb.shape[:2]
    b, c, s = factors(seed, epoch, key, B, C, S, gray_p)
    m = gray_mean(rgb[None])[0]
    one, two = F32(1), F32(2)
    x = rgb.reshape(-1, 3).astype(F32) / F32(255)
    x = _clamp(x * b)
    k = (one - c) * m
    x = _clamp(c * x + k)
    g = (F32(0.299) * x[:, 0] + F32(0.587) * x[:, 1]) + F32(0.114) * x[:, 2]
    x = _clamp(s * x + ((one - s) * g)[:, None])
    fh = frame_hash(seed, epoch, key)
    h = mix64(fh ^ mix64(np.arange(H * W, dtype=np.uint64)))
    for ch in range(3):
        u = ((h >> np.uint64(21 * ch)) & np.uint64(0x1FFFFF)).astype(F32) * F32(2.0 ** -21)
        x[:, ch] = _clamp(x[:, ch] + F32(noise) * (two * u - one))
    x = (x - MEAN) / STD
    assert x.dtype == np.float32
    return np.ascontiguousarray(x.reshape(H, W, 3).transpose(2, 0, 1))


def augment_frames(rgb, keys, **kw):
    """(F, H, W, 3) uint8 and F keys -> (F, 3, H, W) fp32."""
    return np.stack([augment_frame(f, int(k), **kw) for f, k in zip(rgb, keys)])
