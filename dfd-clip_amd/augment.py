"""Device-side training augmentation: the reference's `normal` and `frame` presets on uint8 device clips.

The reference augments every training clip on the host (`src/datasets.py:288-399`): albumentations RGBShift,
HueSaturationValue, RandomBrightnessContrast, ImageCompression (JPEG) and HorizontalFlip, per frame (`frame`) and per
clip with one draw replayed over its frames (`normal`).  Here the draws are made on the host by a seeded NumPy generator
and applied by one kernel launch per preset (`csrc/augment.hip`, `include/dfdclip_augment.h`):

  ClipAugment(spec, seed)   spec = the reference's `augmentation` config string
      .draw(n_clips, n_frames) -> AugmentParams     plain host data: parameter sets + one set index per frame
      .apply(clips_u8, params) -> new tensor        [B,T,3,H,W] uint8 on the device; the same params on a second tensor
                                                    is the reference's `replay` (paired clips)
      (clips_u8)                                    draw, then apply
  augment_reference(frames_u8, params)              NumPy int64 restatement of the kernel's arithmetic; the GPU tests
                                                    demand equality with it bit for bit, and the CPU tests hold its JPEG
                                                    stage against libjpeg

What is kept from albumentations' uint8 paths: RGBShift and RandomBrightnessContrast are 256-entry tables
(`clip(i + shift)`, `clip(i*alpha + 255*beta)`, truncated); HueSaturationValue adds through tables too, which truncates a
fractional shift: the reference's limits of +-0.3 and +-0.05 therefore act as -1 or 0 on the integer scales, a quirk of
the reference that is kept.  Parity with albumentations / OpenCV pixel values is not pinned (neither is a dependency);
the HSV conversion is this module's own integer one.
"""
import numpy as np

from . import capi

FLAG_RGB_LUT, FLAG_HSV, FLAG_TONE_LUT, FLAG_FLIP = capi.AUG_RGB_LUT, capi.AUG_HSV, capi.AUG_TONE_LUT, capi.AUG_FLIP

# dfd_augment_set_t as a NumPy record
SET_DTYPE = np.dtype([("flags", "<u4"), ("hue", "<i4"), ("sat", "<i4"), ("val", "<i4"), ("quality", "<i4"),
                      ("reserved", "<i4", (3,)), ("rgb_lut", "u1", (3, 256)), ("tone_lut", "u1", (256,))])
assert SET_DTYPE.itemsize == capi.AUGMENT_SET_BYTES

# (limit, p) per transform; jpeg = (lowest quality, highest, p); reference src/datasets.py:297-363
_PRESETS = {
    "normal": dict(rgb=(20.0, 0.3), hsv=(0.3, 0.3), tone=(0.3, 0.3), jpeg=(40, 100, 0.5), flip=0.5),
    "frame": dict(rgb=(5.0, 0.3), hsv=(0.05, 0.3), tone=(0.05, 0.3), jpeg=(80, 100, 0.5), flip=0.0),
    "force-rgb": dict(rgb=(20.0, 1.0)),
    "force-hue": dict(hsv=(0.3, 1.0)),
    "force-bright": dict(tone=(0.3, 1.0)),
}


def new_sets(n):
    """`n` parameter sets that change nothing: flags 0, quality 0, identity tables."""
    sets = np.zeros(n, dtype=SET_DTYPE)
    sets["rgb_lut"][:] = np.arange(256, dtype=np.uint8)
    sets["tone_lut"][:] = np.arange(256, dtype=np.uint8)
    return sets


class AugmentParams:
    """What `draw` returns: `stages` = [(name, sets, set_of_frame)] in the order they are applied, for clips of
    `n_clips` x `n_frames` frames.  Host data only; device copies are made on first use and kept."""

    def __init__(self, stages, n_clips, n_frames):
        self.stages = [(str(name), np.ascontiguousarray(sets, dtype=SET_DTYPE), np.ascontiguousarray(idx, dtype=np.int32))
                       for name, sets, idx in stages]
        self.n_clips, self.n_frames = int(n_clips), int(n_frames)
        for name, _, idx in self.stages:
            if idx.shape != (self.n_clips * self.n_frames,):
                raise ValueError(f"stage {name}: {idx.shape} set indices for {self.n_clips} x {self.n_frames} frames")
        self._device = {}

    def on(self, device):
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = [(torch.from_numpy(sets.view(np.uint8).reshape(len(sets), -1).copy()).to(device),
                                  torch.from_numpy(idx.copy()).to(device)) for _, sets, idx in self.stages]
        return self._device[key]


class ClipAugment:
    def __init__(self, spec, seed=None):
        self.spec = str(spec)
        parts = self.spec.split("+")
        self.frame, self.sequence = None, None
        if self.spec != "none":
            if "dev-mode" in parts:
                for k in ("force-rgb", "force-hue", "force-bright"):
                    if k in parts:
                        self.sequence = _PRESETS[k]
                        break
            else:
                if "normal" in parts:
                    self.sequence = _PRESETS["normal"]
                if "frame" in parts:
                    self.frame = _PRESETS["frame"]
            if self.frame is None and self.sequence is None:
                raise NotImplementedError(f"augmentation {self.spec!r}: none of normal, frame, dev-mode+force-rgb|force-hue|force-bright")
        self.rng = np.random.default_rng(seed)

    # ---- draws ----------------------------------------------------------------------------------------------------
    def _draw_sets(self, n, preset):
        rng, sets = self.rng, new_sets(n)
        flags = np.zeros(n, dtype=np.uint32)
        i = np.arange(256, dtype=np.float64)
        if "rgb" in preset:
            lim, p = preset["rgb"]
            fire = rng.random(n) < p
            shift = rng.uniform(-lim, lim, (n, 3))
            lut = np.clip(i[None, None, :] + shift[:, :, None], 0, 255).astype(np.uint8)
            sets["rgb_lut"][fire] = lut[fire]
            flags[fire] |= FLAG_RGB_LUT
        if "hsv" in preset:
            lim, p = preset["hsv"]
            fire = rng.random(n) < p
            shift = np.floor(rng.uniform(-lim, lim, (n, 3))).astype(np.int32)  # what the uint8 table path applies
            fire &= (shift != 0).any(axis=1)  # all three 0: the image is returned untouched
            for k, name in enumerate(("hue", "sat", "val")):
                sets[name][fire] = shift[fire, k]
            flags[fire] |= FLAG_HSV
        if "tone" in preset:
            lim, p = preset["tone"]
            fire = rng.random(n) < p
            alpha = 1.0 + rng.uniform(-lim, lim, n)
            beta = rng.uniform(-lim, lim, n)
            lut = np.clip(i[None, :] * alpha[:, None] + 255.0 * beta[:, None], 0, 255).astype(np.uint8)
            sets["tone_lut"][fire] = lut[fire]
            flags[fire] |= FLAG_TONE_LUT
        if "jpeg" in preset:
            lo, hi, p = preset["jpeg"]
            fire = rng.random(n) < p
            q = rng.integers(lo, hi + 1, n)
            sets["quality"][fire] = q[fire]
        if preset.get("flip", 0.0) > 0:
            fire = rng.random(n) < preset["flip"]
            flags[fire] |= FLAG_FLIP
        sets["flags"] = flags
        return sets

    def draw(self, n_clips, n_frames):
        """One draw per frame for `frame`, one per clip for the sequence presets; `frame` is applied first."""
        stages = []
        n = n_clips * n_frames
        if self.frame is not None:
            stages.append(("frame", self._draw_sets(n, self.frame), np.arange(n, dtype=np.int32)))
        if self.sequence is not None:
            stages.append(("sequence", self._draw_sets(n_clips, self.sequence), np.repeat(np.arange(n_clips, dtype=np.int32), n_frames)))
        return AugmentParams(stages, n_clips, n_frames)

    # ---- application ----------------------------------------------------------------------------------------------
    @staticmethod
    def apply(clips_u8, params):
        """[B,T,3,H,W] uint8 device clips -> a new tensor; one launch per stage of `params`."""
        import torch
        if not (torch.is_tensor(clips_u8) and clips_u8.is_cuda and clips_u8.dtype == torch.uint8):
            raise TypeError("ClipAugment.apply works on uint8 device clips (augment before the conversion to float, on the GPU)")
        if clips_u8.dim() != 5 or clips_u8.shape[2] != 3:
            raise ValueError(f"clips must be [B,T,3,H,W], got {tuple(clips_u8.shape)}")
        B, T = clips_u8.shape[:2]
        if (B, T) != (params.n_clips, params.n_frames):
            raise ValueError(f"params were drawn for {params.n_clips} x {params.n_frames} frames, the clips are {B} x {T}")
        x = clips_u8.contiguous().view(B * T, *clips_u8.shape[2:])
        if not params.stages:
            return x.clone().view_as(clips_u8)
        for sets, idx in params.on(clips_u8.device):
            x = capi.augment_u8(x, torch.empty_like(x), sets, idx)
        return x.view(clips_u8.shape)

    def __call__(self, clips_u8):
        return self.apply(clips_u8, self.draw(clips_u8.shape[0], clips_u8.shape[1]))


# ---- the integer restatement ------------------------------------------------------------------------------------------

def rgb_to_hsv(r, g, b):
    """OpenCV's 8-bit scales (H in [0,180), S, V in [0,255]) in integers with round-to-nearest divisions."""
    r, g, b = (np.asarray(c, dtype=np.int64) for c in (r, g, b))
    v = np.maximum(r, np.maximum(g, b))
    d = v - np.minimum(r, np.minimum(g, b))
    s = np.where(v > 0, (d * 255 + (v >> 1)) // np.maximum(v, 1), 0)
    num = np.where(v == r, (g - b) * 30, np.where(v == g, (b - r) * 30 + 60 * d, (r - g) * 30 + 120 * d))
    num = np.where(num < 0, num + 180 * d, num)
    h = np.where(d > 0, (num + (d >> 1)) // np.maximum(d, 1), 0)
    return np.where(h >= 180, h - 180, h), s, v


def hsv_to_rgb(h, s, v):
    h, s, v = (np.asarray(c, dtype=np.int64) for c in (h, s, v))
    sector = h // 30
    f = h - 30 * sector
    p = (v * (255 - s) + 127) // 255
    q = (v * (7650 - s * f) + 3825) // 7650
    t = (v * (7650 - s * (30 - f)) + 3825) // 7650
    pick = lambda c: np.choose(sector, c)
    return pick([v, q, p, p, t, v]), pick([t, v, v, q, p, p]), pick([p, p, t, v, v, q])


def hsv_shift(r, g, b, hue, sat, val):
    h, s, v = rgb_to_hsv(r, g, b)
    h = (h + int(hue)) % 180
    sat, val = min(max(int(sat), -255), 255), min(max(int(val), -255), 255)  # as the kernel reads them
    return hsv_to_rgb(h, np.clip(s + sat, 0, 255), np.clip(v + val, 0, 255))


_QUANT_BASE = np.array([
    [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
     14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
     49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99],
    [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32], dtype=np.int64).reshape(2, 8, 8)


def quant_tables(quality):
    """The Annex-K tables scaled the libjpeg way (baseline: entries clipped to 1..255) -> int64 [2, 8, 8]."""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((_QUANT_BASE * scale + 50) // 100, 1, 255)


_F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069,
          f2053=16819, f2562=20995, f3072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct8(d, first):
    """libjpeg's slow-integer forward DCT over a list of 8 int64 arrays (13-bit constants, 2 pass-1 bits)."""
    F = _F
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = 11 if first else 15
    o = [None] * 8
    o[0] = (tmp10 + tmp11) << 2 if first else _descale(tmp10 + tmp11, 2)
    o[4] = (tmp10 - tmp11) << 2 if first else _descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * F["f0541"]
    o[2] = _descale(z1 + tmp13 * F["f0765"], sh)
    o[6] = _descale(z1 - tmp12 * F["f1847"], sh)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F["f1175"]
    t4, t5, t6, t7 = tmp4 * F["f0298"], tmp5 * F["f2053"], tmp6 * F["f3072"], tmp7 * F["f1501"]
    z1, z2 = z1 * -F["f0899"], z2 * -F["f2562"]
    z3, z4 = z3 * -F["f1961"] + z5, z4 * -F["f0390"] + z5
    o[7], o[5], o[3], o[1] = (_descale(t4 + z1 + z3, sh), _descale(t5 + z2 + z4, sh), _descale(t6 + z2 + z3, sh),
                              _descale(t7 + z1 + z4, sh))
    return o


def _idct8(d, first):
    F = _F
    sh = 11 if first else 18
    z2, z3 = d[2], d[6]
    z1 = (z2 + z3) * F["f0541"]
    tmp2, tmp3 = z1 - z3 * F["f1847"], z1 + z2 * F["f0765"]
    tmp0, tmp1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F["f1175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F["f0298"], tmp1 * F["f2053"], tmp2 * F["f3072"], tmp3 * F["f1501"]
    z1, z2 = z1 * -F["f0899"], z2 * -F["f2562"]
    z3, z4 = z3 * -F["f1961"] + z5, z4 * -F["f0390"] + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    pairs = ((tmp10, tmp3), (tmp11, tmp2), (tmp12, tmp1), (tmp13, tmp0))
    return [_descale(a + b, sh) for a, b in pairs] + [_descale(a - b, sh) for a, b in reversed(pairs)]


def _along(fn, x, axis, first):
    return np.stack(fn([np.take(x, k, axis=axis) for k in range(8)], first), axis=axis)


def _block_round_trip(plane, table):
    """[H, W] int64 samples (H, W multiples of 8) -> the samples after DCT, quantisation and inverse DCT."""
    H, W = plane.shape
    x = plane.reshape(H // 8, 8, W // 8, 8).transpose(0, 2, 1, 3) - 128
    x = _along(_fdct8, _along(_fdct8, x, 3, True), 2, False)  # rows, then columns
    level = (np.abs(x) + 4 * table) // (8 * table)            # round half away from zero; the DCT output is scaled by 8
    x = np.sign(x) * level * table
    x = _along(_idct8, _along(_idct8, x, 2, True), 3, False)  # columns, then rows
    return np.clip(x + 128, 0, 255).transpose(0, 2, 1, 3).reshape(H, W)


def jpeg_round_trip(frame, quality):
    """[3, h, w] -> [3, h, w] int64: libjpeg's baseline 4:2:0 encode and decode at `quality`, in its fixed point."""
    frame = np.asarray(frame, dtype=np.int64)
    _, h, w = frame.shape
    ph, pw = -(-h // 16) * 16, -(-w // 16) * 16
    R, G, B = np.pad(frame, ((0, 0), (0, ph - h), (0, pw - w)), mode="edge")
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    ch, cw = (h + 1) // 2, (w + 1) // 2
    tables = quant_tables(quality)

    def down(c):
        s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
        out = (s + 1 + (np.arange(pw // 2) & 1)) >> 2
        out[ch:] = out[ch - 1]  # libjpeg pads the downsampled plane with its last real row
        return out

    Y = _block_round_trip(Y, tables[0])[:h, :w]
    y, x = np.arange(h), np.arange(w)
    cy, cx = y >> 1, x >> 1
    ny = np.where(y & 1, np.minimum(cy + 1, ch - 1), np.maximum(cy - 1, 0))
    nx = np.where(x & 1, np.minimum(cx + 1, cw - 1), np.maximum(cx - 1, 0))
    up = []
    for c in (Cb, Cr):
        c = _block_round_trip(down(c), tables[1])
        colsum = 3 * c[cy] + c[ny]                                              # [h, pw/2]
        up.append(((3 * colsum[:, cx] + colsum[:, nx] + np.where(x & 1, 7, 8)) >> 4) - 128)
    cb, cr = up
    return np.stack([np.clip(Y + ((91881 * cr + 32768) >> 16), 0, 255),
                     np.clip(Y + ((-22554 * cb - 46802 * cr + 32768) >> 16), 0, 255),
                     np.clip(Y + ((116130 * cb + 32768) >> 16), 0, 255)])


def augment_frame(frame, s):
    """One frame [3, h, w] under one parameter set (a SET_DTYPE record), stage by stage as the kernel does."""
    x = np.asarray(frame, dtype=np.int64)
    flags = int(s["flags"])
    if flags & FLAG_RGB_LUT:
        x = np.stack([s["rgb_lut"][c].astype(np.int64)[x[c]] for c in range(3)])
    if flags & FLAG_HSV:
        x = np.stack(hsv_shift(x[0], x[1], x[2], s["hue"], s["sat"], s["val"]))
    if flags & FLAG_TONE_LUT:
        x = s["tone_lut"].astype(np.int64)[x]
    q = min(max(int(s["quality"]), 0), 100)
    if q > 0:
        x = jpeg_round_trip(x, q)
    if flags & FLAG_FLIP:
        x = x[:, :, ::-1]
    return x.astype(np.uint8)


def augment_sets_reference(frames_u8, sets, set_of_frame):
    """`dfd_augment_u8` in NumPy: frames [n, 3, h, w] uint8; an index outside the table copies the frame."""
    frames = np.asarray(frames_u8)
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[1] == 3 and len(set_of_frame) == len(frames)
    out = np.empty_like(frames)
    for f, si in enumerate(np.asarray(set_of_frame)):
        out[f] = augment_frame(frames[f], sets[si]) if 0 <= si < len(sets) else frames[f]
    return out


def augment_reference(frames_u8, params):
    """What `ClipAugment.apply` computes, in NumPy int64: frames [n, 3, h, w] or clips [B, T, 3, h, w] uint8."""
    frames = np.asarray(frames_u8)
    x = frames.reshape(-1, *frames.shape[-3:])
    for _, sets, idx in params.stages:
        x = augment_sets_reference(x, sets, idx)
    return x.reshape(frames.shape).copy()
