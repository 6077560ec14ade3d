"""Shared inputs of the face-alignment tests (tests/test_align_cpu.py, tests/test_hip_align.py): a synthetic mean face,
similarity matrices, image-like and noise sources, plans built from explicit matrices, and exact float64 bilinear
sampling.  No reference file is involved: the reference's mean face is not in its checkout."""
import numpy as np

from dfd_clip_amd import align as AL


def mean_face(canvas=256):
    """68 distinct points spread over the middle of a `canvas` x `canvas` square: a jaw arc (0..16), brows, nose, eyes and a
    mouth ring.  Only its role matters: 8 stable points that are not collinear and a crop centroid near the middle."""
    k = np.arange(68, dtype=np.float64)
    ang = np.pi * (0.1 + 0.8 * k / 16.0)
    jaw = np.stack([0.5 - 0.34 * np.cos(ang), 0.42 + 0.40 * np.sin(ang)], 1)[:17]
    rest = np.stack([0.5 + 0.26 * np.cos(2.399963 * k) * np.sqrt(((k - 16) / 52.0).clip(0, 1)),
                     0.50 + 0.24 * np.sin(2.399963 * k) * np.sqrt(((k - 16) / 52.0).clip(0, 1))], 1)[17:]
    return np.concatenate([jaw, rest]) * canvas


def similarity(scale, theta, tx=0.0, ty=0.0):
    c, s = scale * np.cos(theta), scale * np.sin(theta)
    return np.array([[c, -s, tx], [s, c, ty]], dtype=np.float64)


def centred(scale, theta, src_hw, canvas=256, shift=(0.0, 0.0)):
    """The similarity that puts the source's centre on the canvas' centre (plus `shift`)."""
    M = similarity(scale, theta)
    ctr = np.array([(src_hw[1] - 1) / 2.0, (src_hw[0] - 1) / 2.0])
    M[:, 2] = np.array([(canvas - 1) / 2.0, (canvas - 1) / 2.0]) + np.asarray(shift, dtype=np.float64) - M[:, :2] @ ctr
    return M


def apply_affine(M, pts):
    return np.asarray(pts, dtype=np.float64) @ M[:, :2].T + M[:, 2]


def plan_from(forward, origins, crop=150, canvas=256, border=0, valid=None):
    """An AlignPlan from explicit forward matrices [F,2,3] and crop origins [F,2] (x0, y0)."""
    forward = np.asarray(forward, dtype=np.float64).reshape(-1, 2, 3)
    F = len(forward)
    valid = np.ones(F, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    return AL.AlignPlan(forward, AL.invert_affine(forward), np.asarray(origins).reshape(F, 2), valid, crop, canvas, border)


def smooth_hwc(n, h, w, seed):
    """Image-like uint8 frames [n,h,w,3]: low-frequency content plus mild noise, full range."""
    rng = np.random.default_rng(seed)
    gy, gx = max(2, h // 16), max(2, w // 16)
    low = rng.uniform(0, 255, (n, gy, gx, 3))
    yy = np.linspace(0, gy - 1, h)
    xx = np.linspace(0, gx - 1, w)
    y0, x0 = np.minimum(yy.astype(int), gy - 2), np.minimum(xx.astype(int), gx - 2)
    fy, fx = (yy - y0)[None, :, None, None], (xx - x0)[None, None, :, None]
    a, b = low[:, y0][:, :, x0], low[:, y0][:, :, x0 + 1]
    c, d = low[:, y0 + 1][:, :, x0], low[:, y0 + 1][:, :, x0 + 1]
    img = (a * (1 - fx) + b * fx) * (1 - fy) + (c * (1 - fx) + d * fx) * fy + rng.normal(0, 3, (n, h, w, 3))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def noise_hwc(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)


def exact_bilinear(frame_hwc, inverse, origin, out_h, out_w):
    """float64 bilinear sampling of the zero-padded source under the UNROUNDED inverse matrix -> ([3,out_h,out_w] values,
    source x, source y)."""
    H, W, _ = frame_hwc.shape
    img = np.zeros((H + 4, W + 4, 3))
    img[2:-2, 2:-2] = frame_hwc
    X = origin[0] + np.arange(out_w, dtype=np.float64)[None, :]
    Y = origin[1] + np.arange(out_h, dtype=np.float64)[:, None]
    x = inverse[0, 0] * X + inverse[0, 1] * Y + inverse[0, 2]
    y = inverse[1, 0] * X + inverse[1, 1] * Y + inverse[1, 2]
    xi, yi = np.floor(x), np.floor(y)
    fx, fy = (x - xi)[..., None], (y - yi)[..., None]
    xi = np.clip(xi.astype(np.int64), -2, W) + 2  # everything further out is zero as well
    yi = np.clip(yi.astype(np.int64), -2, H) + 2
    v = (img[yi, xi] * (1 - fx) + img[yi, xi + 1] * fx) * (1 - fy) + (img[yi + 1, xi] * (1 - fx) + img[yi + 1, xi + 1] * fx) * fy
    far = (x < -1) | (x > W) | (y < -1) | (y > H)
    v[far] = 0.0
    return v.transpose(2, 0, 1), x, y


def largest_step(img_hwc):
    """G: the largest absolute difference between horizontally or vertically adjacent pixels."""
    a = img_hwc.astype(np.int64)
    return int(max(np.abs(np.diff(a, axis=0)).max(), np.abs(np.diff(a, axis=1)).max()))
