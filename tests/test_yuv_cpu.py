"""CPU side of the 4:2:0 sources (include/dfdclip_yuv.h, dfd-clip_amd/yuv.py): the header against its ctypes table and record
sizes, the four preset matrices, the refusals of the entry points (no launch, no GPU), the fixed point against exact float64
over every (Y, U, V) triple, against PIL's YCbCr tables, replicated chroma, even windows, and the refusals of `Yuv420`,
`to_rgb`, `apply_yuv` and `infer_raw_video` on the host."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dfd_clip_amd import align as AL
from dfd_clip_amd import capi, harness, yuv
from tests import align_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dfdclip_yuv.h")

# standard, full range -> y_off, cy, crv, cgu, cgv, cbu
PRESETS = {("bt601", False): (16, 76309, 104597, -25675, -53279, 132201),
           ("bt601", True): (0, 65536, 91881, -22553, -46802, 116130),
           ("bt709", False): (16, 76309, 117489, -13975, -34925, 138438),
           ("bt709", True): (0, 65536, 103206, -12276, -30679, 121609)}


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI ------------------------------------------------------------------------------------------------------------

def test_yuv_header_ctypes_table_and_exports_agree():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    fns = sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", _header_text())))
    assert fns == sorted(capi.YUV_SIGNATURES) == ["dfd_align_crop_yuv420", "dfd_yuv420_to_rgb_u8"]
    others = (set(capi.SIGNATURES) | set(capi.EXT_SIGNATURES) | set(capi.EXPLAIN_SIGNATURES) | set(capi.AUGMENT_SIGNATURES) |
              set(capi.ALIGN_SIGNATURES) | set(capi.ELASTIC_SIGNATURES) | set(capi.HOOK_SIGNATURES))
    assert not set(fns) & others
    for name in fns:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == capi.YUV_SIGNATURES[name][1] and getattr(lib, name).restype is ctypes.c_int
        params = re.search(name + r"\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
        assert len(params.split(",")) == len(capi.YUV_SIGNATURES[name][1])
    assert lib.dfd_abi_version() == capi.ABI_VERSION == 17


def test_records_have_the_documented_sizes_and_layouts():
    text = open(HEADER).read()
    defs = {k: int(v) for k, v in re.findall(r"#define\s+DFD_(YUV[A-Z0-9_]+)\s+(\d+)\b", text)}
    assert defs == {"YUV_MATRIX_BYTES": 32, "YUV420_BYTES": 64, "YUV_COEF_MAX": 1 << 21}
    assert ctypes.sizeof(capi.YuvMatrix) == capi.YUV_MATRIX_BYTES == yuv.MATRIX_DTYPE.itemsize == 32
    assert ctypes.sizeof(capi.Yuv420Source) == capi.YUV420_BYTES == 64 and capi.YUV_COEF_MAX == 1 << 21
    for name, _ in capi.YuvMatrix._fields_:
        assert getattr(capi.YuvMatrix, name).offset == yuv.MATRIX_DTYPE.fields[name][1], name
    # the struct members of the header, in order, are the ctypes fields
    for struct, cls in (("dfd_yuv_matrix", capi.YuvMatrix), ("dfd_yuv420", capi.Yuv420Source)):
        body = re.search(r"typedef struct " + struct + r"\s*\{(.*?)\}", _header_text(), flags=re.S).group(1)
        names = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            members = re.match(r"(?:const\s+)?\w+\s*\**\s*(.*)$", decl, flags=re.S).group(1)   # without the type
            names += [re.sub(r"\[\d+\]", "", n).strip() for n in members.split(",")]
        assert names == [n for n, _ in cls._fields_], (struct, names)


def test_the_four_presets_are_the_pinned_integers():
    for (standard, full), want in PRESETS.items():
        m = yuv.matrix(standard, full_range=full)
        assert (int(m["y_off"]),) + tuple(int(m[k]) for k in yuv.COEFFICIENTS) == want, (standard, full)
        assert not m["reserved"].any()
        c = yuv._c_matrix(m)
        assert (c.y_off, c.cy, c.crv, c.cgu, c.cgv, c.cbu) == want
    d = yuv._record(None)                                            # the default: what ffmpeg assumes for untagged video
    assert (int(d["y_off"]),) + tuple(int(d[k]) for k in yuv.COEFFICIENTS) == PRESETS[("bt601", False)]
    with pytest.raises(ValueError, match="standard"):
        yuv.matrix("bt2020")
    with pytest.raises(ValueError, match="y_off"):
        yuv.custom_matrix(256, 65536, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="2\\^21"):
        yuv.custom_matrix(0, 65536, (1 << 21) + 1, 0, 0, 0)
    assert int(yuv.custom_matrix(255, -(1 << 21), 1 << 21, 0, 0, 0)["cy"]) == -(1 << 21)
    with pytest.raises(TypeError, match="MATRIX_DTYPE"):
        yuv.to_rgb_reference(np.zeros((1, 2, 2), np.uint8), np.zeros((1, 1, 1), np.uint8), np.zeros((1, 1, 1), np.uint8), matrix=(16, 1, 2, 3, 4, 5))


def test_refusals_return_an_error_without_launching():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    Y, U, V, OUT, REC = 1 << 30, 1 << 31, (1 << 31) + (1 << 20), 1 << 32, 1 << 33  # never dereferenced: every call returns at its checks
    good = yuv._c_matrix(None)

    def source(**o):   # 2 frames of 48x64, I420, dense
        a = dict(y=Y, u=U, v=V, yrs=64, yfs=64 * 48, crs=32, cfs=32 * 24, cpx=1)
        a.update(o)
        return capi.Yuv420Source(a["y"], a["u"], a["v"], a["yrs"], a["yfs"], a["crs"], a["cfs"], a["cpx"], 0)

    def refused(word, m=good, out=OUT, n=2, wh=48, ww=64, oh=150, ow=150, rec=REC, convert=True, crop=True, null_src=False, null_m=False, **o):
        s = None if null_src else ctypes.byref(source(**o))
        mm = None if null_m else ctypes.byref(m)
        calls = ([("dfd_yuv420_to_rgb_u8", lambda: lib.dfd_yuv420_to_rgb_u8(s, wh, ww, out, n, mm, None))] if convert else []) + \
                ([("dfd_align_crop_yuv420", lambda: lib.dfd_align_crop_yuv420(s, wh, ww, out, n, oh, ow, rec, mm, None))] if crop else [])
        for name, call in calls:
            rc = call()
            msg = lib.dfd_last_error()
            assert rc == -1 and word in msg and name.encode() in msg, (name, o, rc, msg)

    refused(b"bad frame count", n=-1)
    refused(b"bad window size", wh=0)
    refused(b"bad window size", ww=-3)
    refused(b"bad window size", wh=1 << 16, ww=1 << 15, yrs=1 << 15, crs=1 << 14, crop=False)   # a plane of 2^31 bytes
    refused(b"bad output size", oh=0, convert=False)
    refused(b"bad output size", ow=-1, convert=False)
    refused(b"null source description or matrix", null_src=True)
    refused(b"null source description or matrix", null_m=True)
    refused(b"chroma pixel stride", cpx=0)
    refused(b"chroma pixel stride", cpx=3)
    refused(b"y_off", m=capi.YuvMatrix(256, 65536, 0, 0, 0, 0))
    refused(b"y_off", m=capi.YuvMatrix(-1, 65536, 0, 0, 0, 0))
    for k in range(5):
        for c in ((1 << 21) + 1, -(1 << 21) - 1, -(1 << 31)):
            co = [65536, 0, 0, 0, 0]
            co[k] = c
            refused(b"out of range", m=capi.YuvMatrix(0, *co))
    refused(b"luma row stride", yrs=63)
    refused(b"chroma row stride", crs=31)
    refused(b"chroma row stride", cpx=2, crs=62)                   # an interleaved row of one plane spans 2 * 31 + 1 bytes
    refused(b"luma frame stride", yfs=47 * 64 + 63)
    refused(b"chroma frame stride", cfs=23 * 32 + 31)
    refused(b"null pointer", y=None)
    refused(b"null pointer", u=None)
    refused(b"null pointer", v=None)
    refused(b"null pointer", out=None)
    refused(b"no parameter records", rec=None, convert=False)
    refused(b"8-byte aligned", rec=REC + 4, convert=False)
    refused(b"the y plane and out overlap", out=Y + 2 * 64 * 48 - 1)   # out starting on the last luma byte
    refused(b"the u plane and out overlap", out=U)
    refused(b"the v plane and out overlap", out=V + 2 * 32 * 24 - 1)
    refused(b"the v plane and out overlap", v=OUT + 2 * 3 * 48 * 64 - 1, crop=False)     # a plane starting on out's last byte
    refused(b"the v plane and out overlap", v=OUT + 2 * 3 * 150 * 150 - 1, convert=False)
    # touching buffers, the coefficient limit itself and the exact strides are fine: only n == 0 gets this far without a GPU
    edge = capi.YuvMatrix(255, 1 << 21, -(1 << 21), 1 << 21, -(1 << 21), 1 << 21)
    s = source(cpx=2, crs=63, cfs=23 * 63 + 63)
    assert lib.dfd_yuv420_to_rgb_u8(ctypes.byref(s), 48, 64, None, 0, ctypes.byref(edge), None) == 0
    assert lib.dfd_align_crop_yuv420(ctypes.byref(s), 48, 64, None, 0, 150, 150, None, ctypes.byref(edge), None) == 0


# ---- the fixed point -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("standard,full", sorted(PRESETS))
def test_fixed_point_against_exact_float64_over_every_triple(standard, full):
    """|fixed point - clip(exact float64, 0, 255)| <= 0.5 + 511 / 2^17 over all 2^24 triples: a coefficient is off by at most
    2^-17 (rint of a Q16 value), |y| + |u| + |v| <= 255 + 128 + 128 = 511, clipping moves two numbers no further apart, and
    one rounding to an integer adds 0.5."""
    y_off, exact = yuv.exact_matrix(standard, full)
    m = yuv.matrix(standard, full)
    bound = 0.5 + 511.0 / 2 ** 17
    U, V = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    u, v = U - 128.0, V - 128.0
    chroma = (exact["crv"] * v, exact["cgu"] * u + exact["cgv"] * v, exact["cbu"] * u)
    worst, hit_low, hit_high = 0.0, False, False
    for Y in range(256):
        got = yuv.convert_reference(np.full_like(U, Y), U, V, m)
        for g, c in zip(got, chroma):
            want = exact["cy"] * (Y - y_off) + c
            hit_low, hit_high = hit_low or bool((want < 0).any()), hit_high or bool((want > 255).any())
            worst = max(worst, float(np.abs(g - np.clip(want, 0.0, 255.0)).max()))
    print(f"{standard} full_range={full}: max |fixed - exact| {worst:.5f}  bound {bound:.5f}")
    assert worst <= bound
    assert worst > 0.49 and hit_low and hit_high      # real rounding was seen and both clamps fired


def test_bt601_full_range_against_pil_tables():
    """A sanity check, not a parity claim: PIL's YCbCr -> RGB is JFIF (BT.601 full range) from coarser tables, so it may
    differ by one step; more would mean a wrong matrix."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    ycc = rng.integers(0, 256, (200, 300, 3), dtype=np.uint8)
    want = np.asarray(Image.frombytes("YCbCr", (300, 200), ycc.tobytes()).convert("RGB")).astype(np.int64)
    got = np.stack(yuv.convert_reference(ycc[..., 0], ycc[..., 1], ycc[..., 2], yuv.matrix("bt601", full_range=True)), axis=-1)
    d = np.abs(got - want)
    print(f"PIL: max |diff| {int(d.max())}, {100 * float((d > 0).mean()):.1f} % of samples differ")
    assert d.max() <= 1
    limited = np.stack(yuv.convert_reference(ycc[..., 0], ycc[..., 1], ycc[..., 2], yuv.matrix("bt601")), axis=-1)
    assert np.abs(limited - want).max() > 10          # the comparison can tell two matrices apart


# ---- replicated chroma -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", [(1, 1), (2, 2), (3, 5), (37, 50), (16, 64), (5, 4)])
def test_replicated_chroma_is_repeat_upsampling(h, w):
    rng = np.random.default_rng(h * 100 + w)
    ch, cw = yuv.chroma_size(h, w)
    assert (ch, cw) == (-(-h // 2), -(-w // 2))
    y = rng.integers(0, 256, (2, h, w), dtype=np.uint8)
    u, v = rng.integers(0, 256, (2, 2, ch, cw), dtype=np.uint8)
    up = lambda p: np.repeat(np.repeat(p, 2, axis=1), 2, axis=2)[:, :h, :w]
    assert np.array_equal(yuv.upsample_chroma(u, h, w), up(u))
    got = yuv.to_rgb_reference(y, u, v)
    assert got.shape == (2, 3, h, w) and got.dtype == np.uint8
    want = np.stack(yuv.convert_reference(y, up(u), up(v)), axis=1)
    assert np.array_equal(got, want)
    assert np.array_equal(yuv.to_rgb_reference((y, u, v)), got)
    # grey chroma and BT.601 full range: R = G = B = Y
    assert np.array_equal(yuv.to_rgb_reference(y, np.full_like(u, 128), np.full_like(v, 128), matrix=yuv.matrix(full_range=True)), np.stack([y] * 3, 1))


def test_align_reference_is_the_composition():
    rng = np.random.default_rng(3)
    y = rng.integers(0, 256, (2, 48, 64), dtype=np.uint8)
    u, v = rng.integers(0, 256, (2, 2, 24, 32), dtype=np.uint8)
    plan = C.plan_from([C.centred(0.4, 0.0, (48, 64)), C.centred(2.5, 0.5, (48, 64))], [(53, 53), (53, 53)], border=9)
    m = yuv.matrix("bt709")
    rgb = yuv.to_rgb_reference(y, u, v, m)
    got = yuv.align_reference((y, u, v), plan, m)
    assert np.array_equal(got, AL.align_reference(rgb, plan, layout="chw"))
    assert np.array_equal(got, AL.align_reference(np.ascontiguousarray(rgb.transpose(0, 2, 3, 1)), plan))
    assert not np.array_equal(got, yuv.align_reference((y, u, v), plan))       # the matrix matters


# ---- even windows --------------------------------------------------------------------------------------------------------

def _window_plan(H, W):
    fwd = [C.centred(1.6, 0.3, (H, W), shift=(-30, 12)), C.centred(2.2, -0.5, (H, W), shift=(55, -20)), C.centred(1.0, 0.0, (H, W)),
           C.centred(1.9, 0.1, (H, W), shift=(500, 0)), C.centred(1.7, -0.2, (H, W), shift=(-420, -330))]   # the last two look past the frame
    return C.plan_from(fwd, [(53, 53), (40, 60), (0, 106), (53, 53), (41, 47)], border=7, valid=[True, True, False, True, True])


@pytest.mark.parametrize("H,W", [(300, 420), (301, 419), (300, 419)])
def test_even_windows_have_even_origins_and_cover_every_tap(H, W):
    plan = _window_plan(H, W)
    fp, v = plan.footprint(), plan.valid
    frames = C.noise_hwc(len(v), H, W, seed=13)
    full = AL.align_reference(frames, plan)
    P = 500
    padded = np.full((len(v), H + 2 * P, W + 2 * P, 3), 7, dtype=np.uint8)
    padded[:, P:P + H, P:P + W] = frames
    for margin, frame_size in ((0, (H, W)), (3, (H, W)), (0, None), (2, None)):
        (wh, ww), org = plan.window(margin, frame_size, even=True)
        assert org.shape == (len(v), 2) and org.dtype == np.int64 and not (org & 1).any()
        if frame_size is None:
            assert wh % 2 == 0 and ww % 2 == 0
        else:                                            # even, except along an odd frame dimension
            assert wh % 2 == H % 2 and ww % 2 == W % 2 and wh < H and ww < W
            assert (org >= 0).all() and (org[:, 0] + ww <= W).all() and (org[:, 1] + wh <= H).all()
        lo, hi = fp[:, :2] - margin, fp[:, 2:] + margin  # every tap (and the margin) that lies in the frame lies in its window
        if frame_size is not None:
            lo, hi = np.clip(lo, 0, [W - 1, H - 1]), np.clip(hi, 0, [W - 1, H - 1])
        assert (org[v] <= lo[v]).all() and (org[v] + [ww, wh] > hi[v]).all()
        cut = np.stack([padded[f, P + y:P + y + wh, P + x:P + x + ww] for f, (x, y) in enumerate(org)])
        assert np.array_equal(AL.align_reference(cut, plan.with_window(org, (wh, ww))), full)
        # no more than one pixel per side larger than the plain window
        (ph, pw), porg = plan.window(margin, frame_size)
        assert wh <= ph + 2 and ww <= pw + 2
    # the default is what it was
    assert plan.window(0, (H, W))[0] == plan.window(0, (H, W), even=False)[0]
    assert np.array_equal(plan.window(1, None)[1], plan.window(1, None, even=False)[1])
    none = C.plan_from([C.similarity(1.0, 0.0)], [(0, 0)], valid=[False])
    assert none.window(0, (H, W), even=True)[0] == (2, 2) and none.window(0, (H, W))[0] == (1, 1)


# ---- refusals on the host -------------------------------------------------------------------------------------------------

def test_yuv420_and_apply_yuv_refuse_host_tensors_and_bad_arguments():
    y, u, v = torch.zeros(2, 48, 64, dtype=torch.uint8), torch.zeros(2, 24, 32, dtype=torch.uint8), torch.zeros(2, 24, 32, dtype=torch.uint8)
    with pytest.raises(TypeError, match="uint8 device planes"):
        yuv.Yuv420.i420(y, u, v)
    with pytest.raises(TypeError, match="uint8 device planes"):
        yuv.Yuv420.i420(y.numpy(), u.numpy(), v.numpy())
    with pytest.raises(TypeError, match="uint8 device planes"):
        yuv.Yuv420.nv12(y, torch.zeros(2, 24, 32, 2, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uv must be"):
        yuv.Yuv420.nv12(y, torch.zeros(2, 24, 64, dtype=torch.uint8))
    with pytest.raises(ValueError, match="uv must be"):
        yuv.Yuv420.nv12(y, torch.zeros(2, 24, 2, 32, dtype=torch.uint8).permute(0, 1, 3, 2))   # pairs not adjacent
    with pytest.raises(ValueError, match="packed"):
        yuv.Yuv420.packed_nv12(torch.zeros(2, 71, 64, dtype=torch.uint8), 48, 64)
    with pytest.raises(ValueError, match="packed"):
        yuv.Yuv420.packed_nv12(torch.zeros(2, 72, 63, dtype=torch.uint8), 48, 64)
    with pytest.raises(TypeError, match="uint8 device planes"):
        yuv.Yuv420.packed_nv12(torch.zeros(2, 72, 64, dtype=torch.uint8), 48, 64)               # the shape is right, the device is not
    plan = C.plan_from([C.similarity(1.0, 0.0)] * 2, [(0, 0)] * 2)
    for bad in (y, (y, u, v), np.zeros((2, 48, 64, 3), np.uint8)):
        with pytest.raises(TypeError, match="Yuv420"):
            AL.FaceAligner.apply_yuv(bad, plan)
        with pytest.raises(TypeError, match="Yuv420"):
            yuv.to_rgb(bad)


class _FakeSource(yuv.Yuv420):
    """A Yuv420 that skips the device check, to reach the checks behind it without a GPU."""

    def __init__(self, F, H, W):
        self.frames, self.height, self.width = F, H, W
        self.y = torch.zeros(0, dtype=torch.uint8)


def test_apply_yuv_refuses_odd_window_origins_and_wrong_sizes():
    plan = _window_plan(300, 420)
    src = _FakeSource(5, 300, 420)
    with pytest.raises(ValueError, match="the plan holds"):
        AL.FaceAligner.apply_yuv(_FakeSource(4, 300, 420), plan)
    (wh, ww), org = plan.window(0, (300, 420), even=True)
    with pytest.raises(ValueError, match="windows"):
        AL.FaceAligner.apply_yuv(src, plan.with_window(org, (wh, ww)))
    for shift in ([1, 0], [0, 1], [-1, 3]):
        with pytest.raises(ValueError, match="odd full-frame coordinate"):
            AL.FaceAligner.apply_yuv(_FakeSource(5, wh, ww), plan.with_window(org + shift, (wh, ww)))


def test_infer_raw_video_keeps_rgb_and_yuv_arguments_apart():
    class Model:
        num_frames = 4

        def eval(self):
            return self

    ref = C.mean_face()
    lm = np.repeat(C.apply_affine(AL.invert_affine(C.centred(1.2, 0.05, (120, 160))), ref)[None], 4, 0)
    with pytest.raises(ValueError, match="matrix="):
        harness.infer_raw_video(Model(), torch.zeros(4, 120, 160, 3, dtype=torch.uint8), lm, AL.FaceAligner(ref), matrix=yuv.matrix())
    with pytest.raises(ValueError, match="swap_rb"):
        harness.infer_raw_video(Model(), _FakeSource(4, 120, 160), lm, AL.FaceAligner(ref), swap_rb=True)
