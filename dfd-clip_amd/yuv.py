"""8-bit YUV 4:2:0 sources on the device: NV12 / NV21 / I420 / YV12 surfaces, as decoders deliver them, in front of the two
places where frames enter (`csrc/yuv.hip`, `include/dfdclip_yuv.h`):

  matrix(standard="bt601" | "bt709", full_range=False) -> the Q16 conversion record (MATRIX_DTYPE = dfd_yuv_matrix_t)
  Yuv420              a description of device planes: views only, never a copy
      .nv12(y [F,H,W], uv [F,ceil(H/2),ceil(W/2),2], swap_uv=False)     swap_uv: NV21
      .i420(y, u, v)                                                    u, v [F,ceil(H/2),ceil(W/2)]; YV12 is the same call
      .packed_nv12(buf [F, H + ceil(H/2), pitch], height, width)        one allocation per surface: luma rows, then uv rows
  to_rgb(src, matrix=None)                  -> [F,3,H,W] uint8: what `Detector.predict`, `ClipAugment` and `SslFake` take
  FaceAligner.apply_yuv(src, plan, matrix)  -> [F,3,crop,crop] uint8 (align.py): the alignment gather with the conversion in
                                               its taps, so that only the pixels a crop touches are converted
  to_rgb_reference(y, u, v, matrix=None)    NumPy int64 restatement of the conversion; the GPU tests demand equality bit for bit
  align_reference(src, plan, matrix=None)   = align.align_reference(to_rgb_reference(src), plan, layout="chw"): by definition
                                               what the fused gather computes (a tap is converted first and blended second)

Arithmetic (the header has the full text): y = Y - y_off, u = U - 128, v = V - 128, then
R = clamp8((cy y + crv v + 32768) >> 16), G = clamp8((cy y + cgu u + cgv v + 32768) >> 16), B = clamp8((cy y + cbu u + 32768) >> 16),
in 32-bit integers; y is not clamped at 0.  Chroma is replicated: pixel (r, c) takes chroma sample (r >> 1, c >> 1); odd
sizes are legal (ceil(H/2) x ceil(W/2) samples).  The default matrix is BT.601 limited range, what ffmpeg assumes for
untagged video.

NOT pinned, because it cannot be checked in this project: the pixel values of swscale or `cv2.cvtColor`, neither of which
is a dependency.  OpenCV clamps Y - 16 at 0 and uses a 20-bit shift where this uses 16 bits; tests/test_yuv_cpu.py holds the
fixed point against exact float64 over all 2^24 triples of every preset, and against PIL's YCbCr tables, instead.
"""
import numpy as np

from . import capi

# dfd_yuv_matrix_t as a NumPy record
MATRIX_DTYPE = np.dtype([("y_off", "<i4"), ("cy", "<i4"), ("crv", "<i4"), ("cgu", "<i4"), ("cgv", "<i4"), ("cbu", "<i4"),
                         ("reserved", "<i4", (2,))])
assert MATRIX_DTYPE.itemsize == capi.YUV_MATRIX_BYTES
COEFFICIENTS = ("cy", "crv", "cgu", "cgv", "cbu")
_KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722)}


def exact_matrix(standard="bt601", full_range=False):
    """(y_off, {coefficient: exact float64}) from the standard's (Kr, Kb): R = cy y + crv v, G = cy y + cgu u + cgv v,
    B = cy y + cbu u; limited range scales luma by 255/219 and chroma by 255/224."""
    if standard not in _KR_KB:
        raise ValueError(f"standard must be 'bt601' or 'bt709', got {standard!r}")
    kr, kb = _KR_KB[standard]
    kg = 1.0 - kr - kb
    ys, cs = (1.0, 1.0) if full_range else (255.0 / 219.0, 255.0 / 224.0)
    return (0 if full_range else 16), {"cy": ys, "crv": 2.0 * (1.0 - kr) * cs, "cgu": -2.0 * kb * (1.0 - kb) / kg * cs,
                                       "cgv": -2.0 * kr * (1.0 - kr) / kg * cs, "cbu": 2.0 * (1.0 - kb) * cs}


def matrix(standard="bt601", full_range=False):
    """The conversion record of a standard: every coefficient rint(exact * 65536)."""
    y_off, exact = exact_matrix(standard, full_range)
    return custom_matrix(y_off, *[int(np.rint(exact[k] * 65536.0)) for k in COEFFICIENTS])


def custom_matrix(y_off, cy, crv, cgu, cgv, cbu):
    """A record from the caller's own Q16 integers; the limits are the entry points'."""
    m = np.zeros((), dtype=MATRIX_DTYPE)
    if not 0 <= int(y_off) <= 255:
        raise ValueError(f"y_off must lie in 0..255, got {y_off}")
    m["y_off"] = int(y_off)
    for k, c in zip(COEFFICIENTS, (cy, crv, cgu, cgv, cbu)):
        if abs(int(c)) > capi.YUV_COEF_MAX:
            raise ValueError(f"|{k}| must not exceed 2^21, got {c}")
        m[k] = int(c)
    return m


def _record(m):
    """-> a 0-d MATRIX_DTYPE array (None: BT.601 limited range)"""
    if m is None:
        return matrix()
    m = np.asarray(m)
    if m.dtype != MATRIX_DTYPE or m.size != 1:
        raise TypeError("matrix must be one record of yuv.MATRIX_DTYPE (yuv.matrix(...) or yuv.custom_matrix(...))")
    return m.reshape(())


def _c_matrix(m):
    return capi.YuvMatrix.from_buffer_copy(_record(m).tobytes())


def chroma_size(h, w):
    return (int(h) + 1) // 2, (int(w) + 1) // 2


class Yuv420:
    """Device planes of F frames of H x W pixels: `y` [F,H,W], `u` and `v` [F,ceil(H/2),ceil(W/2)], uint8 views whose last
    stride is 1 (y), and 1 or 2 (u and v alike: planar or interleaved), with rows and frames wherever they lie.  Nothing is
    copied: a view that the kernels cannot read as it lies is refused."""

    def __init__(self, y, u, v):
        import torch
        for name, t in (("y", y), ("u", u), ("v", v)):
            if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8):
                raise TypeError(f"Yuv420 describes uint8 device planes (upload the decoder's surfaces as they are); {name} is "
                                f"{getattr(t, 'dtype', type(t))} on {getattr(t, 'device', 'the host')}")
            if t.dim() != 3:
                raise ValueError(f"the {name} plane must be [F, rows, columns], got {tuple(t.shape)}")
        F, H, W = y.shape
        ch, cw = chroma_size(H, W)
        if H < 1 or W < 1:
            raise ValueError(f"frames of {H}x{W} pixels")
        for name, t in (("u", u), ("v", v)):
            if tuple(t.shape) != (F, ch, cw):
                raise ValueError(f"{F} frames of {H}x{W} pixels have {name} planes of [{F},{ch},{cw}], got {tuple(t.shape)}")
        if u.device != y.device or v.device != y.device:
            raise ValueError("the three planes must lie on one device")
        self.frames, self.height, self.width = int(F), int(H), int(W)
        self.y, self.u, self.v = y, u, v
        # strides are element = byte strides; a dimension of size 1 has no stride to speak of
        self.c_px_stride = int(u.stride(2)) if cw > 1 else (2 if abs(u.data_ptr() - v.data_ptr()) == 1 else 1)
        if self.c_px_stride not in (1, 2) or (cw > 1 and v.stride(2) != self.c_px_stride):
            raise ValueError(f"chroma samples must be 1 (planar) or 2 (interleaved) bytes apart in both planes, got {u.stride(2)} and {v.stride(2)}")
        if W > 1 and y.stride(2) != 1:
            raise ValueError(f"luma samples must be adjacent, got a stride of {y.stride(2)}")
        c_row = (cw - 1) * self.c_px_stride + 1
        self.y_row_stride = int(y.stride(1)) if H > 1 else W
        self.c_row_stride = int(u.stride(1)) if ch > 1 else c_row
        if ch > 1 and v.stride(1) != u.stride(1):
            raise ValueError(f"the u and v planes must share one row stride, got {u.stride(1)} and {v.stride(1)}")
        y_span, c_span = (H - 1) * self.y_row_stride + W, (ch - 1) * self.c_row_stride + c_row
        self.y_frame_stride = int(y.stride(0)) if F > 1 else y_span
        self.c_frame_stride = int(u.stride(0)) if F > 1 else c_span
        if F > 1 and v.stride(0) != u.stride(0):
            raise ValueError(f"the u and v planes must share one frame stride, got {u.stride(0)} and {v.stride(0)}")
        if self.y_row_stride < W or self.c_row_stride < c_row or self.y_frame_stride < y_span or self.c_frame_stride < c_span:
            raise ValueError("the planes' rows or frames overlap (strides smaller than what they step over): not a surface layout")

    @classmethod
    def nv12(cls, y, uv, swap_uv=False):
        """y [F,H,W] and the interleaved plane uv [F,ceil(H/2),ceil(W/2),2] (`swap_uv`: NV21, V first)."""
        if getattr(uv, "ndim", 0) != 4 or uv.shape[3] != 2 or uv.stride(3) != 1 or (uv.shape[2] > 1 and uv.stride(2) != 2):
            raise ValueError(f"uv must be [F,ceil(H/2),ceil(W/2),2] with its pairs adjacent in memory, got {tuple(getattr(uv, 'shape', ()))}")
        first, second = uv[..., 0], uv[..., 1]
        return cls(y, second, first) if swap_uv else cls(y, first, second)

    @classmethod
    def i420(cls, y, u, v):
        """Three planes of their own (I420, or YV12: only their order in memory differs)."""
        return cls(y, u, v)

    @classmethod
    def packed_nv12(cls, buf, height, width, swap_uv=False):
        """One allocation per surface, as decoders hand them out: buf [F, height + ceil(height/2), pitch] holds `height` luma
        rows of `width` bytes and under them ceil(height/2) rows of interleaved chroma, all `pitch` bytes apart."""
        H, W = int(height), int(width)
        ch, cw = chroma_size(H, W)
        if getattr(buf, "ndim", 0) != 3 or buf.shape[1] != H + ch or buf.shape[2] < max(W, 2 * cw) or buf.stride(2) != 1:
            raise ValueError(f"a packed {H}x{W} NV12 surface is [F,{H + ch},pitch >= {max(W, 2 * cw)}] with adjacent bytes, got "
                             f"{tuple(getattr(buf, 'shape', ()))}")
        return cls.nv12(buf[:, :H, :W], buf[:, H:, :2 * cw].unflatten(2, (cw, 2)), swap_uv=swap_uv)

    @property
    def device(self):
        return self.y.device

    def __len__(self):
        return self.frames

    def source(self):
        """The dfd_yuv420_t of these planes."""
        return capi.Yuv420Source(self.y.data_ptr(), self.u.data_ptr(), self.v.data_ptr(), self.y_row_stride, self.y_frame_stride,
                                 self.c_row_stride, self.c_frame_stride, self.c_px_stride, 0)

    def numpy(self):
        """(y, u, v) as host arrays: what the restatements take."""
        return self.y.cpu().numpy(), self.u.cpu().numpy(), self.v.cpu().numpy()


def to_rgb(src, matrix=None):
    """A `Yuv420` -> a new tensor [F,3,H,W] uint8 on its device; one launch."""
    import torch
    if not isinstance(src, Yuv420):
        raise TypeError(f"to_rgb takes a yuv.Yuv420 (device planes), got {type(src).__name__}")
    out = torch.empty(src.frames, 3, src.height, src.width, dtype=torch.uint8, device=src.device)
    return capi.yuv420_to_rgb_u8(src.source(), out, _c_matrix(matrix))


# ---- the integer restatement ------------------------------------------------------------------------------------------

def upsample_chroma(plane, h, w):
    """[..., ceil(h/2), ceil(w/2)] -> [..., h, w]: sample (r >> 1, c >> 1) for pixel (r, c)."""
    plane = np.asarray(plane)
    return plane[..., np.arange(h) >> 1, :][..., np.arange(w) >> 1]


def convert_reference(Y, U, V, matrix=None):
    """The fixed-point conversion of sample arrays of one shape -> (R, G, B) int64 arrays in 0..255."""
    m = _record(matrix)
    y = np.asarray(Y).astype(np.int64) - int(m["y_off"])
    u, v = np.asarray(U).astype(np.int64) - 128, np.asarray(V).astype(np.int64) - 128
    cy, crv, cgu, cgv, cbu = (int(m[k]) for k in COEFFICIENTS)
    l = cy * y
    return (np.clip((l + crv * v + 32768) >> 16, 0, 255), np.clip((l + cgu * u + cgv * v + 32768) >> 16, 0, 255),
            np.clip((l + cbu * u + 32768) >> 16, 0, 255))


def _planes(src):
    y, u, v = src.numpy() if isinstance(src, Yuv420) else src
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    assert y.dtype == np.uint8 and u.dtype == np.uint8 and v.dtype == np.uint8 and y.ndim == 3, (y.dtype, u.dtype, v.dtype, y.shape)
    F, H, W = y.shape
    assert u.shape == v.shape == (F,) + chroma_size(H, W), (y.shape, u.shape, v.shape)
    return y, u, v


def to_rgb_reference(y, u=None, v=None, matrix=None):
    """`dfd_yuv420_to_rgb_u8` in NumPy int64: y [F,H,W], u and v [F,ceil(H/2),ceil(W/2)] uint8 (or a `Yuv420`, or one
    (y, u, v) tuple, as `y`) -> [F,3,H,W] uint8."""
    y, u, v = _planes(y if u is None else (y, u, v))
    H, W = y.shape[1:]
    return np.stack(convert_reference(y, upsample_chroma(u, H, W), upsample_chroma(v, H, W), matrix), axis=1).astype(np.uint8)


def align_reference(src, plan, matrix=None):
    """What `FaceAligner.apply_yuv` computes, by definition: the alignment restatement on the converted frames."""
    from . import align as AL
    return AL.align_records_reference(to_rgb_reference(src, matrix=matrix), plan.records, plan.crop, plan.crop, layout="chw")
