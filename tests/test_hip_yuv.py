"""GPU tests of the 4:2:0 sources (`dfd_yuv420_to_rgb_u8`, `dfd_align_crop_yuv420`, csrc/yuv.hip): both kernels must equal the
integer restatements of dfd-clip_amd/yuv.py BIT FOR BIT (torch.equal): the converter on NV12, NV21, I420 and YV12 given as
pointers and strides, dense and padded, on even and odd base addresses, on odd sizes and single pixels, under the four
presets and matrices at the coefficient limit; the fused crop on what tests/test_hip_align.py runs the RGB crop on.  Then
the composition on the device (`apply_yuv` = `apply` of `to_rgb`), `infer_raw_video` on a `Yuv420`, and the refusals.

Every kernel call goes through `Surfaces`: each allocation of the source is an exactly sized image (it ends with the last
sample of the last row of its last plane) whose row and frame padding is poisoned, in front of a poisoned guard; the output
sits between guards; all of them are checked after the launch; and every comparison runs with poison 0 and with poison 255,
one of which changes the result if it is read."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from dfd_clip_amd import align as AL
from dfd_clip_amd import capi, yuv
from tests import align_cases as C
from tests.cases import make_config
from tests.guarded import guarded_1d

pytestmark = pytest.mark.gpu

FORMS = ("nv12", "nv21", "i420", "yv12")
LIMIT = capi.YUV_COEF_MAX


def planes_from(hwc):
    """[F,H,W,3] test frames -> (y [F,H,W], u, v [F,ceil(H/2),ceil(W/2)]): channel 0 as luma, channels 1 and 2 subsampled."""
    return tuple(np.ascontiguousarray(p) for p in (hwc[..., 0], hwc[:, ::2, ::2, 1], hwc[:, ::2, ::2, 2]))


class Surfaces:
    """The planes (y, u, v) laid out in device memory in one of four forms, each described to the kernels by three pointers:
      nv12   two allocations: luma; interleaved chroma rows (u = base, v = base + 1, pixel stride 2)
      nv21   ONE allocation per clip as decoders hand surfaces out: per frame H luma rows, then the interleaved rows, V first,
             all one pitch apart
      i420   three allocations, one per plane: a guard stands behind each of them
      yv12   ONE allocation: per frame the luma plane, the V plane, the U plane
    rows are `row_pad` bytes apart beyond their length, frames `frame_pad` bytes beyond their span; `lead` bytes of poison in
    front of every allocation put all its planes on odd addresses (the allocation itself is 16-byte aligned)."""

    def __init__(self, planes, form, row_pad=0, frame_pad=0, poison=255, lead=0):
        y, u, v = planes
        F, H, W = y.shape
        ch, cw = u.shape[1:]
        self.shape = (F, H, W)
        if form in ("nv12", "i420"):
            y_rs = W + row_pad
            y_fs = (H - 1) * y_rs + W + frame_pad
            px = 2 if form == "nv12" else 1
            c_rs = px * cw + row_pad
            c_fs = (ch - 1) * c_rs + px * cw + frame_pad
            # (allocation, offset) of each plane
            where = {"y": (0, 0), "u": (1, 0), "v": (1, 1) if form == "nv12" else (2, 0)}
        elif form == "nv21":
            px = 2
            y_rs = c_rs = max(W, 2 * cw) + row_pad
            y_fs = c_fs = (H + ch - 1) * y_rs + 2 * cw + frame_pad
            where = {"y": (0, 0), "v": (0, H * y_rs), "u": (0, H * y_rs + 1)}
        elif form == "yv12":
            px = 1
            y_rs, c_rs = W + row_pad, cw + row_pad
            y_fs = c_fs = H * y_rs + ch * c_rs + (ch - 1) * c_rs + cw + frame_pad
            where = {"y": (0, 0), "v": (0, H * y_rs), "u": (0, H * y_rs + ch * c_rs)}
        else:
            raise ValueError(form)
        layout = {"y": (y, y_rs, y_fs, 1), "u": (u, c_rs, c_fs, px), "v": (v, c_rs, c_fs, px)}
        sizes = {}
        for name, (data, rs, fs, step) in layout.items():
            a, off = where[name]
            R, Cn = data.shape[1:]
            sizes[a] = max(sizes.get(a, 0), lead + off + (F - 1) * fs + (R - 1) * rs + (Cn - 1) * step + 1)
        images = {a: np.full(n, poison, dtype=np.uint8) for a, n in sizes.items()}
        for name, (data, rs, fs, step) in layout.items():
            a, off = where[name]
            R, Cn = data.shape[1:]
            for f in range(F):
                for r in range(R):
                    o = lead + off + f * fs + r * rs
                    images[a][o:o + (Cn - 1) * step + 1:step] = data[f, r]
        self.allocations = [guarded_1d(img.size, torch.uint8, fill=poison, name=f"{form} allocation {a}").set(torch.from_numpy(img))
                            for a, img in sorted(images.items())]
        ptr = {name: self.allocations[where[name][0]].t.data_ptr() + lead + where[name][1] for name in layout}
        self.source = capi.Yuv420Source(ptr["y"], ptr["u"], ptr["v"], y_rs, y_fs, c_rs, c_fs, px, 0)

    def assert_untouched(self):
        for g in self.allocations:
            g.assert_untouched(view_too=True)


def same(got, want):
    if not torch.equal(torch.from_numpy(got), torch.from_numpy(want)):
        bad = np.argwhere(got != want)
        f, c, y, x = bad[0]
        raise AssertionError(f"{len(bad)} of {got.size} samples differ; first at frame {f} channel {c} ({y}, {x}): "
                             f"kernel {got[f, c, y, x]} restatement {want[f, c, y, x]}; frames {sorted(set(bad[:, 0].tolist()))}")


def run_convert(planes, form, matrix, out_fill=0xA5, **kw):
    F, H, W = planes[0].shape
    src = Surfaces(planes, form, **kw)
    out = guarded_1d(F * 3 * H * W, torch.uint8, fill=out_fill, name="out")
    capi.yuv420_to_rgb_u8(src.source, out.shaped(F, 3, H, W), yuv._c_matrix(matrix))
    torch.cuda.synchronize()
    out.assert_untouched()
    src.assert_untouched()
    return out.shaped(F, 3, H, W).cpu().numpy()


def check_convert(planes, form, matrix=None, **kw):
    """Kernel against restatement under two poisons and two output pre-fills; returns the result."""
    want = yuv.to_rgb_reference(*planes, matrix=matrix)
    same(run_convert(planes, form, matrix, poison=255, out_fill=0xA5, **kw), want)
    same(run_convert(planes, form, matrix, poison=0, out_fill=0x5A, **kw), want)
    return want


def run_crop(planes, records, out_h, out_w, form, matrix, out_fill=0xA5, **kw):
    F, H, W = planes[0].shape
    src = Surfaces(planes, form, **kw)
    out = guarded_1d(F * 3 * out_h * out_w, torch.uint8, fill=out_fill, name="out")
    rec = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(F, -1).copy()).cuda()
    capi.align_crop_yuv420(src.source, H, W, out.shaped(F, 3, out_h, out_w), rec, yuv._c_matrix(matrix))
    torch.cuda.synchronize()
    out.assert_untouched()
    src.assert_untouched()
    return out.shaped(F, 3, out_h, out_w).cpu().numpy()


def check_crop(planes, records, out_h, out_w, form, matrix=None, row_pad=5, frame_pad=77, **kw):
    want = AL.align_records_reference(yuv.to_rgb_reference(*planes, matrix=matrix), records, out_h, out_w, layout="chw")
    same(run_crop(planes, records, out_h, out_w, form, matrix, poison=255, out_fill=0xA5, row_pad=row_pad, frame_pad=frame_pad, **kw), want)
    same(run_crop(planes, records, out_h, out_w, form, matrix, poison=0, out_fill=0x5A, row_pad=row_pad, frame_pad=frame_pad, **kw), want)
    return want


# ---- converter -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def noise_planes(F, H, W, seed):
    return planes_from(C.noise_hwc(F, H, W, seed))


@pytest.mark.parametrize("form", FORMS)
def test_converter_on_every_form_size_stride_and_base(form):
    """37x50: both odd chroma roundings, a last run of two pixels, a last row without a partner, rows on every alignment; 1x1
    and 2x2: one lane, one chroma sample; 16x64: every access of the dense, aligned case is the wide one."""
    for k, (F, H, W) in enumerate(((3, 37, 50), (1, 1, 1), (2, 2, 2), (3, 16, 64))):
        planes = noise_planes(F, H, W, 40 + k)
        want = check_convert(planes, form)                                          # dense, aligned bases
        assert want.shape == (F, 3, H, W)
        check_convert(planes, form, row_pad=5, frame_pad=77)                        # padded: odd strides
        check_convert(planes, form, row_pad=8, frame_pad=64)                        # padded, strides that keep the alignment
        check_convert(planes, form, lead=1)                                         # an odd base address for every plane
        check_convert(planes, form, row_pad=3, frame_pad=10, lead=1)
    assert len(np.unique(want)) > 200


def cube_planes():
    """One frame holding the 8 corners and the 12 edge midpoints of the (Y, U, V) cube, each on a 2x2 block of pixels."""
    pts = [(a, b, c) for a in (0, 255) for b in (0, 255) for c in (0, 255)]
    for axis in range(3):
        for a in (0, 255):
            for b in (0, 255):
                p = [a, b]
                p.insert(axis, 128)
                pts.append(tuple(p))
    pts = np.array(pts, dtype=np.uint8)
    assert len(pts) == 20
    return np.repeat(np.repeat(pts[None, None, :, 0], 2, axis=1), 2, axis=2), pts[None, None, :, 1].copy(), pts[None, None, :, 2].copy()


MATRICES = [yuv.matrix("bt601"), yuv.matrix("bt601", True), yuv.matrix("bt709"), yuv.matrix("bt709", True),
            yuv.custom_matrix(0, LIMIT, LIMIT, LIMIT, LIMIT, LIMIT),          # the largest sums: 2^21 * (255 + 127 + 127)
            yuv.custom_matrix(255, LIMIT, LIMIT, LIMIT, LIMIT, LIMIT),        # the smallest: 2^21 * (-255 - 128 - 128)
            yuv.custom_matrix(128, 40000, -LIMIT, LIMIT, -LIMIT, -LIMIT)]


@pytest.mark.parametrize("k", range(len(MATRICES)))
def test_converter_under_presets_and_limit_matrices_on_the_cube(k):
    m = MATRICES[k]
    cube = cube_planes()
    for form in ("nv12", "i420"):
        got = check_convert(cube, form, m, row_pad=3, frame_pad=0)
    # both clamps fire: somewhere the unclamped value lies below 0, somewhere above 255
    y = cube[0][0, 0, ::2].astype(np.int64) - int(m["y_off"])
    u, v = cube[1][0, 0].astype(np.int64) - 128, cube[2][0, 0].astype(np.int64) - 128
    raw = np.stack([(int(m["cy"]) * y + int(m["crv"]) * v + 32768) >> 16, (int(m["cy"]) * y + int(m["cgu"]) * u + int(m["cgv"]) * v + 32768) >> 16,
                    (int(m["cy"]) * y + int(m["cbu"]) * u + 32768) >> 16])
    assert raw.min() < 0 and raw.max() > 255 and np.abs(raw).max() < 1 << 15      # nothing overflowed 32 bits before the shift
    assert np.array_equal(got[0, :, 0, ::2], np.clip(raw, 0, 255)) and got.min() == 0 and got.max() == 255
    check_convert(noise_planes(2, 9, 21, 50), "nv21", m, row_pad=1, frame_pad=5, lead=1)
    check_convert(noise_planes(2, 9, 21, 50), "yv12", m)


# ---- fused crop ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def three_similarities():
    """tests/test_hip_align.py's case: 3 frames of 64x48 and a plan: scale 0.4, scale 2.5 with rotation 0.5 rad, and a crop that
    leaves the source on two sides."""
    planes = planes_from(C.smooth_hwc(3, 48, 64, seed=31))
    plan = C.plan_from([C.centred(0.4, 0.0, (48, 64)), C.centred(2.5, 0.5, (48, 64)), C.centred(3.0, -0.2, (48, 64), shift=(-60.0, -45.0))],
                       [(53, 53), (53, 53), (41, 60)], border=9)
    return planes, plan


@pytest.mark.parametrize("form", ["nv12", "i420"])
def test_crop_three_similarities_on_padded_strides(form):
    planes, plan = three_similarities()
    m = yuv.matrix("bt709")
    want = check_crop(planes, plan.records, 150, 150, form, m)
    for f in range(3):   # every frame mixes source content with border
        assert (want[f] == 9).all(axis=0).any() and len(np.unique(want[f])) > 30, f
    assert (want[2, :, -1, :] == 9).all() and (want[2, :, :, -1] == 9).all() and not (want[2, :, 0, 0] == 9).all()
    assert not (want[:, 0] == want[:, 1]).all()                                     # colour came through
    same(run_crop(planes, plan.records, 150, 150, form, m, row_pad=0, frame_pad=0), want)            # and dense
    same(run_crop(planes, plan.records, 150, 150, form, m, row_pad=2, frame_pad=1, lead=1), want)    # and on odd addresses
    assert not np.array_equal(check_crop(planes, plan.records, 150, 150, form), want)                # the default matrix is another one


@pytest.mark.parametrize("form", ["nv12", "i420", "nv21", "yv12"])
def test_crop_odd_output_plane_takes_the_tail_path(form):
    planes = planes_from(C.smooth_hwc(3, 79, 95, seed=32))                          # odd source sizes: chroma planes of 40x48
    rec = C.plan_from([C.centred(1.3, 0.25, (79, 95)), C.centred(0.9, -0.4, (79, 95)), C.centred(2.0, 0.1, (79, 95))],
                      [(100, 110), (90, 95), (117, 101)], border=3).records
    want = check_crop(planes, rec, 37, 41, form)   # 37 * 41 = 1517: frames 1 and 2 start on odd addresses, each plane ends in one byte
    assert all(len(np.unique(want[f])) > 30 for f in range(3))
    check_crop(planes, rec, 41, 37, form)
    check_crop(tuple(p[:1] for p in planes), rec[:1], 1, 1, form)
    check_crop(tuple(p[:2] for p in planes), rec[:2], 3, 2, form)   # planes shorter than one group, a group across three rows


def test_crop_far_translations_give_border_and_do_not_wrap():
    planes = noise_planes(6, 48, 64, 33)
    fwd = [C.similarity(1.0, 0.0, 1e6, 0.0), C.similarity(1.0, 0.0, -1e6, 0.0), C.similarity(1.0, 0.0, 0.0, 1e6), C.similarity(0.7, 0.3, -1e6, -1e6)]
    rec = np.concatenate([C.plan_from(fwd, [(53, 53)] * 4, border=77).records] * 2)[:6]
    # 2^32 and 2^40 source pixels away: positions that a 32-bit coordinate would fold back onto the frame
    rec["q"][4] = [65536, 0, (1 << 32) * 65536, 0, 65536, 0]
    rec["q"][5] = [65536, 0, 0, 0, 65536, -(1 << 40) * 65536]
    rec["x0"][4:], rec["y0"][4:] = 0, 0
    for form in ("nv12", "i420"):
        assert (check_crop(planes, rec, 150, 150, form) == 77).all()
    near = rec.copy()
    near["q"][4][2] = 0                         # the same record without the offset does read the frame
    assert not (AL.align_records_reference(yuv.to_rgb_reference(*planes), near, 150, 150, layout="chw")[4] == 77).all()


def test_crop_even_windows_equal_the_full_frames():
    H, W = 120, 160
    planes = planes_from(C.smooth_hwc(3, H, W, seed=34))
    plan = C.plan_from([C.centred(5.0, 0.1, (H, W), shift=(40.0, -25.0)), C.centred(4.6, -0.15, (H, W), shift=(-260.0, 140.0)),
                        C.centred(5.5, 0.0, (H, W), shift=(330.0, 230.0))], [(53, 53), (20, 90), (106, 0)], border=5)
    full = yuv.align_reference(planes, plan)
    (wh, ww), org = plan.window(0, (H, W), even=True)
    assert wh <= 42 and ww <= 42 and wh % 2 == 0 and ww % 2 == 0 and not (org & 1).any() and len({tuple(o) for o in org}) == 3
    y, u, v = planes
    windows = (np.stack([y[f, oy:oy + wh, ox:ox + ww] for f, (ox, oy) in enumerate(org)]),
               np.stack([u[f, oy // 2:(oy + wh) // 2, ox // 2:(ox + ww) // 2] for f, (ox, oy) in enumerate(org)]),
               np.stack([v[f, oy // 2:(oy + wh) // 2, ox // 2:(ox + ww) // 2] for f, (ox, oy) in enumerate(org)]))
    windowed = plan.with_window(org, (wh, ww))
    for form in ("nv12", "i420"):
        same(check_crop(windows, windowed.records, 150, 150, form), full)
        check_crop(planes, plan.records, 150, 150, form)
    # the same through the Python surface, on strided views of the full planes for a single frame
    dev = [torch.from_numpy(p).cuda() for p in planes]
    for f, (ox, oy) in enumerate(org):
        src = yuv.Yuv420.i420(dev[0][f:f + 1, oy:oy + wh, ox:ox + ww], dev[1][f:f + 1, oy // 2:(oy + wh) // 2, ox // 2:(ox + ww) // 2],
                              dev[2][f:f + 1, oy // 2:(oy + wh) // 2, ox // 2:(ox + ww) // 2])
        one = AL.AlignPlan(plan.forward[f:f + 1], plan.inverse[f:f + 1], plan.origin[f:f + 1], plan.valid[f:f + 1], plan.crop, plan.canvas, plan.border)
        same(AL.FaceAligner.apply_yuv(src, one.with_window(org[f:f + 1], (wh, ww))).cpu().numpy(), full[f:f + 1])
        with pytest.raises(ValueError, match="odd full-frame coordinate"):
            AL.FaceAligner.apply_yuv(src, one.with_window(org[f:f + 1] + [1, 0], (wh, ww)))


@pytest.mark.parametrize("border", [0, 200])
def test_crop_identity_and_invalid_frames(border):
    planes = noise_planes(4, 170, 200, 35)
    plan = C.plan_from([C.similarity(1.0, 0.0), C.similarity(1.0, 0.0, 7.0, -3.0), C.similarity(1.0, 0.0), C.similarity(2.0, 0.3)],
                       [(40, 10), (30, 2), (0, 0), (53, 53)], border=border, valid=[True, True, False, False])
    rgb = yuv.to_rgb_reference(*planes)
    for form in ("nv12", "i420"):
        got = check_crop(planes, plan.records, 150, 150, form)
        assert np.array_equal(got[0], rgb[0, :, 10:160, 40:190])          # an integer translation copies converted pixels
        assert np.array_equal(got[1], rgb[1, :, 5:155, 23:173])
        assert (got[2:] == border).all()
    wild = plan.records.copy()                      # an invalid frame's other fields are never used
    wild["q"][2:] = -(1 << 62)
    wild["border"][3] = border + 1000 if border else -5   # clamped to 0..255
    got = check_crop(planes, wild, 150, 150, "nv12")
    assert (got[2] == border).all() and (got[3] == (255 if border else 0)).all()
    # invalid frames do not read the source: whatever it holds, from one poison to the other, the crop is the border
    none = plan.records.copy()
    none["flags"] = AL.FLAG_INVALID
    for poison in (0, 255):
        filled = tuple(np.full_like(p, poison) for p in planes)
        for form in ("nv12", "i420"):
            assert (run_crop(filled, none, 150, 150, form, None, poison=poison, row_pad=5, frame_pad=77) == border).all()


def test_crop_single_frame_and_no_frame():
    planes, plan = three_similarities()
    want = yuv.align_reference(planes, plan)
    for f in range(3):
        same(check_crop(tuple(p[f:f + 1] for p in planes), plan.records[f:f + 1], 150, 150, "nv12"), want[f:f + 1])
    for call in ("crop", "convert"):
        out = guarded_1d(3 * 150 * 150, torch.uint8, fill=0xA5, name="out")
        src = Surfaces(tuple(p[:1] for p in planes), "i420")
        rec = torch.zeros(0, capi.ALIGN_FRAME_BYTES, dtype=torch.uint8, device="cuda")
        if call == "crop":
            capi.align_crop_yuv420(src.source, 48, 64, out.shaped(1, 3, 150, 150)[:0], rec, yuv._c_matrix(None))
        else:
            capi.yuv420_to_rgb_u8(src.source, out.t[0, :0].view(0, 3, 48, 64), yuv._c_matrix(None))
        torch.cuda.synchronize()
        out.assert_untouched()
        assert bool((out.t == 0xA5).all())              # nothing was launched, nothing written
    dev = [torch.zeros(0, *p.shape[1:], dtype=torch.uint8, device="cuda") for p in planes]
    empty = yuv.Yuv420.i420(*dev)
    assert tuple(AL.FaceAligner.apply_yuv(empty, C.plan_from(np.zeros((0, 2, 3)), np.zeros((0, 2)))).shape) == (0, 3, 150, 150)
    assert tuple(yuv.to_rgb(empty).shape) == (0, 3, 48, 64)


def test_refusals_leave_the_output_alone():
    lib = capi.load_library()
    planes, plan = three_similarities()
    src = Surfaces(planes, "nv12", row_pad=5, frame_pad=77)
    out = guarded_1d(3 * 3 * 150 * 150, torch.uint8, fill=0xA5, name="out")
    rec = plan.on("cuda")
    good = yuv._c_matrix(None)
    base = src.source

    def source(**o):
        s = capi.Yuv420Source.from_buffer_copy(bytes(base))
        for k, val in o.items():
            setattr(s, k, val)
        return s

    def both(word, s=base, m=good, o=None):
        o = out.t.data_ptr() if o is None else o
        rc = lib.dfd_yuv420_to_rgb_u8(ctypes.byref(s), 48, 64, o, 3, ctypes.byref(m), None)
        assert rc == -1 and word in lib.dfd_last_error(), ("dfd_yuv420_to_rgb_u8", word, lib.dfd_last_error())
        rc = lib.dfd_align_crop_yuv420(ctypes.byref(s), 48, 64, o, 3, 150, 150, rec.data_ptr(), ctypes.byref(m), None)
        assert rc == -1 and word in lib.dfd_last_error(), ("dfd_align_crop_yuv420", word, lib.dfd_last_error())

    # which plane the message names depends on where the allocator put the buffers (out is 200 KB long); tests/test_yuv_cpu.py
    # pins the names on made-up addresses
    both(b"plane and out overlap", o=base.y + 100)
    both(b"plane and out overlap", o=base.u)
    both(b"plane and out overlap", o=base.v + 2 * base.c_frame_stride + 23 * base.c_row_stride + 62)   # out on the last V sample
    both(b"luma row stride", s=source(y_row_stride=63))
    both(b"chroma row stride", s=source(c_row_stride=62))
    both(b"luma frame stride", s=source(y_frame_stride=47 * 69 + 63))
    both(b"chroma pixel stride", s=source(c_px_stride=4))
    both(b"null pointer", s=source(v=None))
    both(b"y_off", m=capi.YuvMatrix(300, 65536, 0, 0, 0, 0))
    both(b"out of range", m=capi.YuvMatrix(16, 65536, 0, LIMIT + 1, 0, 0))
    assert lib.dfd_align_crop_yuv420(ctypes.byref(base), 48, 64, out.t.data_ptr(), 3, 150, 150, None, ctypes.byref(good), None) == -1
    assert b"no parameter records" in lib.dfd_last_error()
    assert lib.dfd_align_crop_yuv420(ctypes.byref(base), 48, 64, out.t.data_ptr(), 3, 150, 150, rec.data_ptr() + 4, ctypes.byref(good), None) == -1
    assert b"8-byte aligned" in lib.dfd_last_error()
    torch.cuda.synchronize()
    out.assert_untouched()
    src.assert_untouched()
    assert bool((out.t == 0xA5).all())
    with pytest.raises(capi.DfdError):
        capi.align_crop_yuv420(base, 48, 64, out.shaped(3, 3, 150, 150).cpu(), rec, good)
    # and the same calls without a fault in them run
    assert lib.dfd_align_crop_yuv420(ctypes.byref(base), 48, 64, out.t.data_ptr(), 3, 150, 150, rec.data_ptr(), ctypes.byref(good), None) == 0
    torch.cuda.synchronize()
    out.assert_untouched()
    same(out.shaped(3, 3, 150, 150).cpu().numpy(), yuv.align_reference(planes, plan))
    small = guarded_1d(3 * 3 * 48 * 64, torch.uint8, fill=0xA5, name="out")
    assert lib.dfd_yuv420_to_rgb_u8(ctypes.byref(base), 48, 64, small.t.data_ptr(), 3, ctypes.byref(good), None) == 0
    torch.cuda.synchronize()
    small.assert_untouched()
    same(small.shaped(3, 3, 48, 64).cpu().numpy(), yuv.to_rgb_reference(*planes))


# ---- through Yuv420, FaceAligner and infer_raw_video -----------------------------------------------------------------------

def _video(F, H, W, seed, missing=()):
    """Planes with a face drifting and turning slowly, its landmarks, and the aligner."""
    ref = C.mean_face()
    planes = planes_from(C.smooth_hwc(F, H, W, seed=seed))
    rng = np.random.default_rng(seed)
    lm = np.stack([C.apply_affine(AL.invert_affine(C.centred(1.4 + 0.02 * f, 0.03 * f - 0.1, (H, W), shift=(3.0 * f - 10, 6 - f))), ref) for f in range(F)])
    lm += rng.normal(0, 0.7, lm.shape)
    for f in missing:
        lm[f] = np.nan
    return planes, lm, AL.FaceAligner(ref, border=0)


@pytest.mark.parametrize("H,W", [(150, 190), (151, 189)])
def test_apply_yuv_is_apply_of_to_rgb_on_every_constructor(H, W):
    planes, lm, aligner = _video(5, H, W, seed=36, missing=(3,))
    y, u, v = planes
    ch, cw = u.shape[1:]
    plan = aligner.plan(lm)
    m = yuv.matrix("bt709", full_range=True)
    want_rgb, want = yuv.to_rgb_reference(*planes, matrix=m), yuv.align_reference(planes, plan, m)
    assert (want[3] == 0).all() and all(len(np.unique(want[f])) > 50 for f in (0, 1, 2, 4))
    dy, du, dv = (torch.from_numpy(p).cuda() for p in planes)
    uv = torch.stack([du, dv], dim=-1)
    # one allocation per surface with a pitch, as a decoder's; chroma rows under the luma rows
    pitch = 2 * cw + 14
    packed = torch.full((5, H + ch, pitch), 255, dtype=torch.uint8, device="cuda")
    packed[:, :H, :W] = dy
    packed[:, H:, :2 * cw] = uv.reshape(5, ch, 2 * cw)
    # planes that are views of larger uploads: rows and frames are padded by what surrounds them
    big_y = torch.full((5, H + 9, W + 13), 255, dtype=torch.uint8, device="cuda")
    big_c = torch.full((2, 5, ch + 3, cw + 7), 255, dtype=torch.uint8, device="cuda")
    big_y[:, 4:4 + H, 6:6 + W] = dy
    big_c[0, :, 1:1 + ch, 5:5 + cw], big_c[1, :, 1:1 + ch, 5:5 + cw] = du, dv
    sources = {"nv12": yuv.Yuv420.nv12(dy, uv), "nv21": yuv.Yuv420.nv12(dy, torch.stack([dv, du], dim=-1), swap_uv=True),
               "i420": yuv.Yuv420.i420(dy, du, dv), "packed": yuv.Yuv420.packed_nv12(packed, H, W),
               "views": yuv.Yuv420.i420(big_y[:, 4:4 + H, 6:6 + W], big_c[0, :, 1:1 + ch, 5:5 + cw], big_c[1, :, 1:1 + ch, 5:5 + cw])}
    assert sources["packed"].y_row_stride == pitch and sources["packed"].c_px_stride == 2 and sources["views"].c_row_stride == cw + 7
    keep = packed.clone()
    for name, src in sources.items():
        rgb = yuv.to_rgb(src, m)
        assert rgb.dtype == torch.uint8 and rgb.device == dy.device and tuple(rgb.shape) == (5, 3, H, W), name
        same(rgb.cpu().numpy(), want_rgb)
        fused = aligner.apply_yuv(src, plan, m)
        assert tuple(fused.shape) == (5, 3, 150, 150) and fused.dtype == torch.uint8
        assert torch.equal(fused, aligner.apply(rgb, plan, layout="chw")), name                    # the composition, on the device
        assert torch.equal(fused, aligner.apply(rgb.permute(0, 2, 3, 1).contiguous(), plan)), name
        same(fused.cpu().numpy(), want)
    assert torch.equal(packed, keep)
    swapped = yuv.Yuv420.nv12(dy, uv, swap_uv=True)
    assert not torch.equal(aligner.apply_yuv(swapped, plan, m), fused)
    with pytest.raises(ValueError, match="the plan holds"):
        aligner.apply_yuv(yuv.Yuv420.i420(dy[:4], du[:4], dv[:4]), plan)
    with pytest.raises(ValueError, match="planes of"):
        yuv.Yuv420.i420(dy, du[:, :-1], dv[:, :-1])
    with pytest.raises(ValueError, match="1 \\(planar\\) or 2"):
        yuv.Yuv420.i420(dy, torch.zeros(5, ch, cw, 3, dtype=torch.uint8, device="cuda")[..., 0], torch.zeros(5, ch, cw, 3, dtype=torch.uint8, device="cuda")[..., 1])
    with pytest.raises(ValueError, match="adjacent"):
        yuv.Yuv420.i420(torch.zeros(5, W, H, dtype=torch.uint8, device="cuda").permute(0, 2, 1), du, dv)
    with pytest.raises(ValueError, match="share one row stride"):
        yuv.Yuv420.i420(dy, du, big_c[1, :, 1:1 + ch, 5:5 + cw])


def test_infer_raw_video_on_yuv420_equals_predict_on_the_restatement_crops():
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.harness import infer_raw_video
    from dfd_clip_amd.weights import random_state_dict
    T = 4
    cfg = make_config("tiny", decode_mode="index", decode_indices=[0, 1])
    model = Detector(cfg, T, None, precision="fp32")
    model.load_state_dict(random_state_dict(cfg, T, seed=0))
    model = model.cuda().eval()
    F = 2 * T + 3
    planes, lm, aligner = _video(F, 150, 190, seed=37, missing=(5,))
    dy, du, dv = (torch.from_numpy(p).cuda() for p in planes)
    src = yuv.Yuv420.nv12(dy, torch.stack([du, dv], dim=-1))
    m = yuv.matrix("bt709")
    prob, clip_probs, logits = infer_raw_video(model, src, lm, aligner, with_logits=True, matrix=m)
    plan = aligner.plan(lm)
    crops = torch.from_numpy(yuv.align_reference(planes, plan, m)[:2 * T]).cuda().view(2, T, 3, 150, 150)
    mask = torch.from_numpy(plan.valid[:2 * T].copy()).view(2, T).cuda()
    assert mask.tolist() == [[True] * 4, [True, False, True, True]]
    with torch.no_grad():
        want = model.predict(crops, mask)[0][0].cpu()
    assert tuple(logits.shape) == (2, 2) and torch.equal(logits, want)
    assert torch.equal(clip_probs, want.softmax(dim=-1)) and torch.equal(prob, clip_probs.mean(dim=0)[1])
    # the default matrix is BT.601 limited range, and an RGB tensor of the converted frames takes today's path to the same verdict
    default = infer_raw_video(model, yuv.Yuv420.i420(dy, du, dv), lm, aligner, with_logits=True)[2]
    rgb = yuv.to_rgb(src)
    assert torch.equal(default, infer_raw_video(model, rgb, lm, aligner, layout="chw", with_logits=True)[2])
    assert not torch.equal(default, logits)
