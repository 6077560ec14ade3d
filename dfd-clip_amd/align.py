"""Face-aligned crops on the device: from full video frames and 68-point landmarks to the 150x150 crops `Detector` takes.

The reference runs this stage on the host with OpenCV in front of every video (`pipeline.py:114-182`, again in
`preprocessing/extract_faces.py:55-125`): `affine_transform` fits a similarity from 8 stable landmarks onto a mean face
and warps the frame onto a 256x256 canvas, `cut_patch` cuts a 150x150 patch centred on landmarks 15..67, `crop_patch`
loops over the frames.  Here the fit and the crop origin are host arithmetic in float64 and the pixels are one kernel
launch (`csrc/align.hip`, `include/dfdclip_align.h`) that computes only the cut, never the canvas:

  FaceAligner(reference, canvas=256, crop=150, stable_points=..., start_idx=15, stop_idx=68, smooth=0, border=0)
      .plan(landmarks [F,68,2], transforms=None) -> AlignPlan    plain host data
      .apply(frames_u8, plan, layout="hwc", swap_rb=False)       -> [F,3,crop,crop] uint8 on the frames' device
      .apply_yuv(src, plan, matrix=None)                         the same from a 4:2:0 source (`yuv.Yuv420`: NV12, I420, ...)
  AlignPlan   .forward / .inverse [F,2,3], .origin [F,2] (x0, y0), .valid [F], .records (dfd_align_frame_t as a NumPy record)
      .window(margin, frame_size) -> ((win_h, win_w), origins [F,2])   one window size and per-frame origins that cover every
                                                                     tap of every valid frame: upload only the face region
                                                                     (`even=True`: even origins, for 4:2:0 sources)
      .with_window(origins, (win_h, win_w)) -> AlignPlan             the plan for frames sliced that way
  align_reference(frames, plan, ...)   NumPy int64 restatement of the kernel; the GPU tests demand equality bit for bit

Three things the reference does are NOT pinned here, because they cannot be checked in this project:
  * `cv2.warpAffine`'s pixel values.  The kernel keeps its structure (bilinear on a 1/32-pixel grid, 15-bit weights,
    constant border) but rounds the source coordinate once where OpenCV rounds each term; OpenCV is not a dependency.
    tests/test_align_cpu.py holds the restatement against exact float64 bilinear sampling and against PIL instead.
  * `cv2.estimateAffinePartial2D(method=LMEDS)`.  That is a randomised robust fit; `fit_similarity` is the closed-form
    least-squares similarity over the same points, which is what LMEDS converges to on outlier-free landmarks.  A caller
    who has OpenCV's matrices passes them as `transforms=`.
  * The mean face.  The reference loads `misc/20words_mean_face.npy`, which its checkout does not contain; `reference`
    is therefore the caller's [68,2] array and none is shipped.

Two quirks of the reference that are restated on purpose:
  * `crop_patch` overwrites its own `window_margin` (`pipeline.py:166`): it becomes min(12 // 2, 0, ...) = 0 at frame 0 and
    stays 0, so the reference never smooths.  `smooth=0` is the default and matches it; `smooth=k` gives the window
    min(k, i, F-1-i) that line was meant to compute, with the re-centring of `:170`.
  * `cut_patch`'s four "too much bias" raises cannot fire: each follows the clamp that makes its condition false
    (`pipeline.py:138-154`), so `plan` has nothing to raise.
"""
import numpy as np

from . import capi

STABLE_POINTS = (28, 33, 36, 39, 42, 45, 48, 54)

# dfd_align_frame_t as a NumPy record
REC_DTYPE = np.dtype([("q", "<i8", (6,)), ("x0", "<i4"), ("y0", "<i4"), ("win_x", "<i4"), ("win_y", "<i4"), ("border", "<i4"),
                      ("flags", "<u4")])
assert REC_DTYPE.itemsize == capi.ALIGN_FRAME_BYTES
FLAG_INVALID = capi.ALIGN_FRAME_INVALID
_LAYOUTS = {"hwc": capi.ALIGN_HWC, "chw": capi.ALIGN_CHW}
_Q_LIMIT = 2.0 ** 40  # |q| below this with canvas coordinates below 2^20 cannot overflow the kernel's 64-bit affine part


def fit_similarity(src, dst):
    """The least-squares similarity (scale, rotation, translation, no reflection) [[a, -b, tx], [b, a, ty]] taking the
    points `src` [N,2] onto `dst` [N,2], in closed form: the minimiser of sum |M(src) - dst|^2 over (a, b, tx, ty)."""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    if src.shape != dst.shape or src.ndim != 2 or src.shape[1] != 2 or len(src) < 2:
        raise ValueError(f"fit_similarity needs two [N,2] point sets with N >= 2, got {src.shape} and {dst.shape}")
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    s, d = src - ms, dst - md
    den = (s * s).sum()
    if not den > 0:
        raise ValueError("fit_similarity: the source points coincide")
    a = (s * d).sum() / den
    b = (s[:, 0] * d[:, 1] - s[:, 1] * d[:, 0]).sum() / den
    R = np.array([[a, -b], [b, a]])
    return np.concatenate([R, (md - R @ ms)[:, None]], axis=1)


def invert_affine(M):
    """The ordinary inverse of 2x3 affine maps [..., 2, 3]."""
    M = np.asarray(M, dtype=np.float64)
    a, b, c, d = M[..., 0, 0], M[..., 0, 1], M[..., 1, 0], M[..., 1, 1]
    det = a * d - b * c
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.stack([np.stack([d, -b], -1), np.stack([-c, a], -1)], -2) / det[..., None, None]
    t = -(A @ M[..., :, 2:3])
    return np.concatenate([A, t], axis=-1)


def smooth_landmarks(landmarks, k):
    """`crop_patch`'s temporal smoothing as it was meant (`pipeline.py:166-170`): frame i becomes the mean over frames
    i-w..i+w, w = min(k, i, F-1-i), shifted so that its centroid stays frame i's own.  Frames without a face (non-finite
    landmarks) stay as they are and are left out of their neighbours' means."""
    lm = np.asarray(landmarks, dtype=np.float64)
    k = int(k)
    if k <= 0:
        return lm.copy()
    F = len(lm)
    ok = np.isfinite(lm).all(axis=(1, 2))
    out = lm.copy()
    for i in range(F):
        w = min(k, i, F - 1 - i)
        if not ok[i] or w == 0:
            continue
        win = lm[i - w:i + w + 1][ok[i - w:i + w + 1]]
        sm = win.mean(axis=0)
        out[i] = sm + (lm[i].mean(axis=0) - sm.mean(axis=0))
    return out


class AlignPlan:
    """What `FaceAligner.plan` returns: per frame the forward and inverse matrices, the crop origin, the validity and the
    kernel's records.  Host data only; the device copy of the records is made on first use and kept."""

    def __init__(self, forward, inverse, origin, valid, crop, canvas, border=0, win_origin=None, win_size=None, landmarks=None):
        self.forward = np.asarray(forward, dtype=np.float64)
        self.inverse = np.asarray(inverse, dtype=np.float64)
        self.origin = np.asarray(origin, dtype=np.int64).reshape(-1, 2)
        self.valid = np.asarray(valid, dtype=bool).reshape(-1)
        self.crop, self.canvas, self.border = int(crop), int(canvas), int(border)
        self.landmarks = landmarks
        F = len(self.valid)
        if self.forward.shape != (F, 2, 3) or self.inverse.shape != (F, 2, 3) or self.origin.shape != (F, 2):
            raise ValueError("AlignPlan: forward / inverse must be [F,2,3] and origin [F,2] for F = len(valid)")
        if not 0 <= self.border <= 255:
            raise ValueError(f"border must lie in 0..255, got {border}")
        self.win_size = None if win_size is None else (int(win_size[0]), int(win_size[1]))
        self.win_origin = np.zeros((F, 2), dtype=np.int64) if win_origin is None else np.asarray(win_origin, dtype=np.int64).reshape(F, 2)
        rec = np.zeros(F, dtype=REC_DTYPE)
        q = np.where(self.valid[:, None], self.inverse.reshape(F, 6) * 65536.0, 0.0)
        if not (np.isfinite(q).all() and (np.abs(q) < _Q_LIMIT).all()):
            raise ValueError("AlignPlan: a valid frame's transform is singular or absurdly small (its inverse does not fit Q16)")
        rec["q"] = np.rint(q).astype(np.int64)
        rec["x0"], rec["y0"] = self.origin[:, 0], self.origin[:, 1]
        rec["win_x"], rec["win_y"] = self.win_origin[:, 0], self.win_origin[:, 1]
        rec["border"] = self.border
        rec["flags"] = np.where(self.valid, 0, FLAG_INVALID)
        self.records = rec
        self._device = {}

    def __len__(self):
        return len(self.valid)

    def on(self, device):
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = torch.from_numpy(self.records.view(np.uint8).reshape(len(self.records), REC_DTYPE.itemsize).copy()).to(device)
        return self._device[key]

    def footprint(self):
        """[F,4] int64 (x_min, y_min, x_max, y_max): the full-frame pixels the four taps of frame f's crop can touch, from
        the records' own integers.  The source coordinate is affine in the output pixel and the shifts are monotone, so the
        extremes sit at the crop's corners.  Rows of invalid frames are 0."""
        r = self.records
        q = r["q"].astype(np.int64)
        X = np.stack([r["x0"], r["x0"] + self.crop - 1], 1).astype(np.int64)
        Y = np.stack([r["y0"], r["y0"] + self.crop - 1], 1).astype(np.int64)
        out = np.zeros((len(r), 4), dtype=np.int64)
        for k, lo, hi in ((0, 0, 2), (3, 1, 3)):
            f = (q[:, k, None, None] * X[:, :, None] + q[:, k + 1, None, None] * Y[:, None, :] + q[:, k + 2, None, None]).reshape(len(r), 4)
            s = ((f + 1024) >> 11) >> 5
            out[:, lo], out[:, hi] = s.min(axis=1), s.max(axis=1) + 1
        out[~self.valid] = 0
        return out

    def window(self, margin=0, frame_size=None, even=False):
        """((win_h, win_w), origins [F,2] int64 as (x, y)): one window size and a per-frame origin in full-frame coordinates
        such that every tap of every valid frame lies inside its window (plus `margin` pixels on every side).  With
        `frame_size=(H, W)` the windows are kept inside the frame, which loses nothing: a tap outside the frame is `border`
        either way.  The caller slices `frame[y:y+win_h, x:x+win_w]` on the host, uploads the slices and applies
        `with_window(origins, (win_h, win_w))`.
        `even=True` (4:2:0 sources, `apply_yuv`): every origin is even, so that the chroma of a window is the chroma of its
        frame, and every tap is still covered; the sizes are even too, except along an odd `frame_size` dimension, where they
        are odd (no even-sized window at an even origin reaches an odd frame's last column)."""
        margin = int(margin)
        fp = self.footprint()
        v = self.valid
        if not v.any():
            return ((2, 2) if even else (1, 1)), np.zeros((len(v), 2), dtype=np.int64)
        if even:
            return self._even_window(fp, margin, frame_size)
        win_w = int((fp[v, 2] - fp[v, 0]).max()) + 1 + 2 * margin
        win_h = int((fp[v, 3] - fp[v, 1]).max()) + 1 + 2 * margin
        origins = np.where(v[:, None], fp[:, :2] - margin, 0)
        if frame_size is not None:
            H, W = int(frame_size[0]), int(frame_size[1])
            win_h, win_w = min(win_h, H), min(win_w, W)
            origins = np.stack([np.clip(origins[:, 0], 0, W - win_w), np.clip(origins[:, 1], 0, H - win_h)], axis=1)
        return (win_h, win_w), origins.astype(np.int64)

    def _even_window(self, fp, margin, frame_size):
        v = self.valid
        sizes, origins = [], []
        for axis in (0, 1):                                   # x, then y
            lo, hi = fp[:, axis] - margin, fp[:, axis + 2] + margin
            n = None if frame_size is None else int(frame_size[1 - axis])
            if n is not None:                                 # what lies outside the frame is border with or without a window
                lo, hi = np.clip(lo, 0, n - 1), np.clip(hi, 0, n - 1)
            lo = np.where(v, lo - (lo & 1), 0)                # down to the even neighbour (also for negative origins)
            size = int((hi - lo)[v].max()) + 1
            parity = 0 if n is None else n & 1                # n - size even: the last origin that fits is even as well
            size += (size & 1) ^ parity
            if n is not None:
                size = min(size, n)
                lo = np.minimum(lo, n - size)
            sizes.append(size)
            origins.append(lo)
        return (sizes[1], sizes[0]), np.stack(origins, axis=1).astype(np.int64)

    def with_window(self, origins, size):
        """The same plan for frames of which only the window `size` = (win_h, win_w) at `origins` [F,2] (x, y) is held."""
        return AlignPlan(self.forward, self.inverse, self.origin, self.valid, self.crop, self.canvas, self.border,
                         win_origin=origins, win_size=size, landmarks=self.landmarks)


class FaceAligner:
    def __init__(self, reference, canvas=256, crop=150, stable_points=STABLE_POINTS, start_idx=15, stop_idx=68, smooth=0,
                 reference_size=256, border=0):
        self.reference = np.array(reference, dtype=np.float64)
        if self.reference.ndim != 2 or self.reference.shape[1] != 2:
            raise ValueError(f"reference must be the mean face [68,2], got {self.reference.shape}")
        self.canvas, self.crop, self.smooth, self.border = int(canvas), int(crop), int(smooth), int(border)
        if self.crop <= 0 or self.crop % 2:
            raise ValueError(f"crop must be even (the reference cuts 2 * (crop // 2) pixels), got {crop}")
        if self.crop > self.canvas:
            raise ValueError(f"a {crop} crop does not fit a {canvas} canvas")
        self.stable_points = tuple(int(p) for p in stable_points)
        self.start_idx, self.stop_idx = int(start_idx), int(stop_idx)
        # the stable reference points, shifted as `affine_transform` shifts them (pipeline.py:121-123)
        self.stable_reference = self.reference[list(self.stable_points)] - (float(reference_size) - self.canvas) / 2.0

    def crop_origin(self, transformed):
        """`cut_patch` on transformed landmarks [start_idx:stop_idx] -> (x0, y0).  Its raises are unreachable (module
        docstring), so none is restated.  `round` is Python's: halves go to the even neighbour."""
        half = self.crop // 2
        cx, cy = transformed.mean(axis=0)
        out = []
        for c in (cx, cy):
            if c - half < 0:
                c = half
            if c + half > self.canvas:
                c = self.canvas - half
            out.append(int(round(c) - round(half)))
        return out

    def plan(self, landmarks, transforms=None):
        """landmarks [F,68,2] in full-frame pixels (x, y); a frame whose landmarks are not all finite has no face: it is
        marked invalid, its crop is all `border` and `plan.valid` is False for it (the frame mask `Detector` takes).
        `transforms` [F,2,3]: the caller's own forward matrices (frame -> canvas) instead of the fit."""
        lm = np.asarray(landmarks, dtype=np.float64)
        if lm.ndim != 3 or lm.shape[2] != 2 or lm.shape[1] < max(max(self.stable_points) + 1, self.stop_idx):
            raise ValueError(f"landmarks must be [F, points, 2] with the stable and crop points present, got {lm.shape}")
        F = len(lm)
        valid = np.isfinite(lm).all(axis=(1, 2))
        lm = smooth_landmarks(lm, self.smooth)
        if transforms is not None:
            transforms = np.asarray(transforms, dtype=np.float64)
            if transforms.shape != (F, 2, 3):
                raise ValueError(f"transforms must be [{F},2,3], got {transforms.shape}")
            valid = valid & np.isfinite(transforms).all(axis=(1, 2))
        forward = np.zeros((F, 2, 3))
        forward[:, 0, 0] = forward[:, 1, 1] = 1.0
        origin = np.zeros((F, 2), dtype=np.int64)
        for f in np.flatnonzero(valid):
            M = transforms[f] if transforms is not None else fit_similarity(lm[f, list(self.stable_points)], self.stable_reference)
            forward[f] = M
            moved = lm[f] @ M[:, :2].T + M[:, 2]
            origin[f] = self.crop_origin(moved[self.start_idx:self.stop_idx])
        return AlignPlan(forward, invert_affine(forward), origin, valid, self.crop, self.canvas, self.border, landmarks=lm)

    @staticmethod
    def apply(frames_u8, plan, layout="hwc", swap_rb=False):
        """uint8 device frames [F,H,W,3] (`layout="hwc"`, what decoders deliver) or [F,3,H,W] ("chw") -> a new tensor
        [F,3,crop,crop]; one launch.  `swap_rb`: BGR sources come out RGB.  A plan made by `with_window` takes the windows."""
        import torch
        if not (torch.is_tensor(frames_u8) and frames_u8.is_cuda and frames_u8.dtype == torch.uint8):
            raise TypeError("FaceAligner.apply works on uint8 device frames (upload the decoded frames, align on the GPU); got "
                            f"{getattr(frames_u8, 'dtype', type(frames_u8))} on {getattr(frames_u8, 'device', 'the host')}")
        if layout not in _LAYOUTS:
            raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
        hwc = layout == "hwc"
        if frames_u8.dim() != 4 or frames_u8.shape[3 if hwc else 1] != 3:
            raise ValueError(f"frames must be {'[F,H,W,3]' if hwc else '[F,3,H,W]'}, got {tuple(frames_u8.shape)}")
        F = frames_u8.shape[0]
        H, W = (frames_u8.shape[1], frames_u8.shape[2]) if hwc else (frames_u8.shape[2], frames_u8.shape[3])
        if F != len(plan):
            raise ValueError(f"the plan holds {len(plan)} frames, the tensor {F}")
        if plan.win_size is not None and plan.win_size != (H, W):
            raise ValueError(f"the plan was made for {plan.win_size[0]}x{plan.win_size[1]} windows, the frames are {H}x{W}")
        def strides(x):  # (usable as it lies, row stride, frame stride) in bytes
            st = x.stride()
            rs = st[1] if hwc else st[2]
            rows_ok = (st[3] == 1 and st[2] == 3 and rs >= 3 * W) if hwc else (st[3] == 1 and rs >= W and st[1] == H * rs)
            span = ((H if hwc else 3 * H) - 1) * rs + (3 * W if hwc else W)  # bytes one frame spans
            fs = st[0] if F > 1 else max(st[0], span)                          # a single frame's stride is never used
            return rows_ok and fs >= span, rs, fs

        x = frames_u8
        ok, rs, fs = strides(x)  # views with padded rows or frames (a slice of a larger upload) are read where they lie
        if not ok:
            x = x.contiguous()
            ok, rs, fs = strides(x)
        out = torch.empty(F, 3, plan.crop, plan.crop, dtype=torch.uint8, device=x.device)
        return capi.align_crop_u8(x, out, plan.on(x.device), _LAYOUTS[layout], rs, fs, H, W, swap_rb=swap_rb)

    @staticmethod
    def apply_yuv(src, plan, matrix=None):
        """A `yuv.Yuv420` (NV12 / NV21 / I420 / YV12 device planes, read where they lie) -> a new tensor [F,3,crop,crop]; one
        launch that converts tap by tap under `matrix` (`yuv.matrix(...)`, default BT.601 limited range): the bits of
        `apply(yuv.to_rgb(src, matrix), plan, layout="chw")` without the converted frames.  A plan made by `with_window` takes
        the windows; their origins must be even (`plan.window(..., even=True)`), or the window's chroma samples would not be
        the frame's."""
        import torch
        from . import yuv
        if not isinstance(src, yuv.Yuv420):
            raise TypeError(f"FaceAligner.apply_yuv takes a yuv.Yuv420 (device planes as the decoder delivered them), got {type(src).__name__}")
        if len(src) != len(plan):
            raise ValueError(f"the plan holds {len(plan)} frames, the source {len(src)}")
        if plan.win_size is not None and plan.win_size != (src.height, src.width):
            raise ValueError(f"the plan was made for {plan.win_size[0]}x{plan.win_size[1]} windows, the frames are {src.height}x{src.width}")
        if (plan.win_origin[plan.valid] & 1).any():
            raise ValueError("apply_yuv: a window starts on an odd full-frame coordinate, so its chroma samples are not the frame's; "
                             "make the windows with plan.window(..., even=True)")
        out = torch.empty(len(src), 3, plan.crop, plan.crop, dtype=torch.uint8, device=src.device)
        return capi.align_crop_yuv420(src.source(), src.height, src.width, out, plan.on(src.device), yuv._c_matrix(matrix))

    def __call__(self, frames_u8, landmarks, layout="hwc", swap_rb=False):
        plan = self.plan(landmarks)
        return self.apply(frames_u8, plan, layout=layout, swap_rb=swap_rb), plan


# ---- the integer restatement ------------------------------------------------------------------------------------------

def align_records_reference(frames_u8, records, out_h, out_w, layout="hwc", swap_rb=False):
    """`dfd_align_crop_u8` in NumPy int64: frames [F,H,W,3] ("hwc") or [F,3,H,W] ("chw") uint8, the windows the records'
    (win_x, win_y) place in their full frames; records REC_DTYPE [F] -> [F,3,out_h,out_w] uint8."""
    frames = np.asarray(frames_u8)
    if layout not in _LAYOUTS:
        raise ValueError(f"layout must be 'hwc' or 'chw', got {layout!r}")
    assert frames.dtype == np.uint8 and frames.ndim == 4 and frames.shape[3 if layout == "hwc" else 1] == 3, frames.shape
    assert len(records) == len(frames)
    planar = frames.transpose(0, 3, 1, 2) if layout == "hwc" else frames
    H, W = planar.shape[2:]
    out = np.empty((len(frames), 3, out_h, out_w), dtype=np.uint8)
    i, j = np.arange(out_h, dtype=np.int64)[:, None], np.arange(out_w, dtype=np.int64)[None, :]
    for f, r in enumerate(records):
        border = min(max(int(r["border"]), 0), 255)
        if int(r["flags"]) & FLAG_INVALID:
            out[f] = border
            continue
        q = r["q"].astype(np.int64)
        X, Y = np.int64(r["x0"]) + j, np.int64(r["y0"]) + i
        xf = q[0] * X + q[1] * Y + q[2]  # int64 arrays wrap like the kernel's 64-bit registers
        yf = q[3] * X + q[4] * Y + q[5]
        x5, y5 = (xf + 1024) >> 11, (yf + 1024) >> 11
        fx, fy = x5 & 31, y5 & 31
        rx, ry = (x5 >> 5) - np.int64(r["win_x"]), (y5 >> 5) - np.int64(r["win_y"])
        acc = np.full((3, out_h, out_w), 512, dtype=np.int64)
        img = planar[f].astype(np.int64)
        for dy in (0, 1):
            for dx in (0, 1):
                w = (fx if dx else 32 - fx) * (fy if dy else 32 - fy)
                tx, ty = rx + dx, ry + dy
                inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
                v = img[:, np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)]
                acc += w * np.where(inside, v, border)
        res = (acc >> 10).astype(np.uint8)
        out[f] = res[::-1] if swap_rb else res
    return out


def align_reference(frames_u8, plan, layout="hwc", swap_rb=False):
    """What `FaceAligner.apply` computes, in NumPy int64: [F,3,crop,crop] uint8."""
    return align_records_reference(frames_u8, plan.records, plan.crop, plan.crop, layout=layout, swap_rb=swap_rb)
