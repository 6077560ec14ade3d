"""CPU side of the device augmentation: the augment header against its ctypes table, the integer restatement's JPEG stage
against libjpeg (through PIL), properties of the restatement, and `ClipAugment`'s draws."""
import ctypes
import io
import os
import re

import numpy as np
import pytest
import torch

from dfd_clip_amd import augment as A
from dfd_clip_amd import capi, harness
from tests.test_hip_preprocess import smooth_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dfdclip_augment.h")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI ------------------------------------------------------------------------------------------------------------

def test_augment_header_ctypes_table_and_exports_agree():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    fns = sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", _header_text())))
    assert fns == sorted(capi.AUGMENT_SIGNATURES) == ["dfd_augment_u8"]
    others = set(capi.SIGNATURES) | set(capi.EXT_SIGNATURES) | set(capi.EXPLAIN_SIGNATURES) | set(capi.HOOK_SIGNATURES)
    assert not set(fns) & others
    for name in fns:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == capi.AUGMENT_SIGNATURES[name][1]
        params = re.search(name + r"\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
        assert len(params.split(",")) == len(capi.AUGMENT_SIGNATURES[name][1])
    assert lib.dfd_abi_version() == capi.ABI_VERSION == 17


def test_set_struct_has_the_documented_size_and_layout():
    documented = int(re.search(r"#define\s+DFD_AUGMENT_SET_BYTES\s+(\d+)", open(HEADER).read()).group(1))
    assert ctypes.sizeof(capi.AugmentSet) == documented == capi.AUGMENT_SET_BYTES == A.SET_DTYPE.itemsize == 1056
    for name, _ in capi.AugmentSet._fields_:
        assert getattr(capi.AugmentSet, name).offset == A.SET_DTYPE.fields[name][1], name
    flags = dict(re.findall(r"#define\s+DFD_AUG_([A-Z_]+)\s+(\d+)u", open(HEADER).read()))
    assert {k: int(v) for k, v in flags.items()} == {"RGB_LUT": capi.AUG_RGB_LUT, "HSV": capi.AUG_HSV, "TONE_LUT": capi.AUG_TONE_LUT,
                                                     "FLIP": capi.AUG_FLIP}


def test_refusals_return_an_error_without_launching():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    p = [1 << 20, 1 << 21, 1 << 22, 1 << 23]  # never dereferenced: every call returns at its checks
    assert lib.dfd_augment_u8(p[0], p[0], 2, 16, 16, p[2], 1, p[3], None) == -1 and b"in place" in lib.dfd_last_error()
    assert lib.dfd_augment_u8(p[0], p[0] + 100, 2, 16, 16, p[2], 1, p[3], None) == -1 and b"overlap" in lib.dfd_last_error()
    assert lib.dfd_augment_u8(p[0], p[1], 2, 16, 16, p[2], 0, p[3], None) == -1 and b"no parameter set" in lib.dfd_last_error()
    assert lib.dfd_augment_u8(p[0], p[1], 2, 16, 16, None, 1, p[3], None) == -1 and b"no parameter set" in lib.dfd_last_error()
    assert lib.dfd_augment_u8(None, p[1], 2, 16, 16, p[2], 1, p[3], None) == -1 and b"null pointer" in lib.dfd_last_error()
    assert lib.dfd_augment_u8(p[0], p[1], 2, 0, 16, p[2], 1, p[3], None) == -1 and b"bad shape" in lib.dfd_last_error()
    assert lib.dfd_augment_u8(p[0], p[1], 0, 16, 16, None, 0, None, None) == 0  # nothing to do


# ---- the JPEG stage against libjpeg ---------------------------------------------------------------------------------

JPEG_SIZES = ((32, 48), (150, 150), (224, 224))
JPEG_QUALITIES = (40, 60, 80, 95, 100)
# Measured against PIL 12.2 (libjpeg-turbo) on these cases: the restatement equals libjpeg's decode BIT FOR BIT at every
# size and quality (mean 0, share 0 %, max 0); the run is deterministic.  Each bar is the measured value plus a quarter (of
# a level for the mean and the max, of a percent for the share), far inside the issue's caps (mean 0.7, 6 %, and the float
# prototype's max of 15).  The max is a whole number, so its bar demands 0: a single sample off by one level, which is what
# a wrong edge, padding or last-chroma-column rule would first show as, fails the test.
BAR_MEAN, BAR_SHARE, BAR_MAX = 0.25, 0.25e-2, 0.25
assert BAR_MEAN <= 0.7 and BAR_SHARE <= 6e-2 and BAR_MAX <= 15


@pytest.mark.parametrize("h,w", JPEG_SIZES)
def test_jpeg_stage_matches_libjpeg(h, w):
    Image = pytest.importorskip("PIL.Image")
    frame = smooth_u8(1, h, w, seed=11 + h)[0].numpy()
    sets = A.new_sets(len(JPEG_QUALITIES))
    sets["quality"] = JPEG_QUALITIES
    got = A.augment_sets_reference(np.repeat(frame[None], len(sets), 0), sets, np.arange(len(sets)))
    for q, mine in zip(JPEG_QUALITIES, got):
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(frame.transpose(1, 2, 0))).save(buf, format="JPEG", quality=q)
        want = np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB")).transpose(2, 0, 1)
        d = np.abs(mine.astype(np.int64) - want.astype(np.int64))
        mean, share, worst = d.mean(), (d > 2).mean(), int(d.max())
        print(f"{h}x{w} q{q}: mean |d| {mean:.4f}  >2 levels {100 * share:.3f} %  max {worst}")
        assert mean <= BAR_MEAN and share <= BAR_SHARE and worst <= BAR_MAX, (h, w, q, mean, share, worst)


# ---- properties of the restatement ------------------------------------------------------------------------------------

def _one(frame, **fields):
    s = A.new_sets(1)
    for k, v in fields.items():
        s[k] = v
    return A.augment_sets_reference(frame[None], s, np.zeros(1, np.int32))[0]


def test_nothing_to_do_is_the_identity():
    f = smooth_u8(2, 17, 33, seed=1).numpy()
    out = A.augment_sets_reference(f, A.new_sets(1), np.array([0, 5]))  # set 0 does nothing; index 5 is outside: a copy
    assert np.array_equal(out, f)
    assert np.array_equal(A.augment_reference(f, A.AugmentParams([], 1, 2)), f)


def test_hsv_properties():
    grey = np.arange(256)
    h, s, v = A.rgb_to_hsv(grey, grey, grey)
    assert not h.any() and not s.any() and np.array_equal(v, grey)
    frame = np.broadcast_to(grey.astype(np.uint8)[None, None, :], (3, 2, 256)).copy()
    assert np.array_equal(_one(frame, flags=A.FLAG_HSV, hue=37), frame)          # hue moves nothing on grey
    for k in (-300, -7, 0, 9, 300):
        out = _one(frame, flags=A.FLAG_HSV, val=k)
        assert np.array_equal(out, np.clip(frame.astype(np.int64) + k, 0, 255))  # val adds, saturating, and stays grey
    f = smooth_u8(1, 24, 40, seed=2)[0].numpy()
    assert np.array_equal(_one(f, flags=A.FLAG_HSV, hue=180), _one(f, flags=A.FLAG_HSV, hue=0))
    assert np.array_equal(_one(f, flags=A.FLAG_HSV, hue=-143), _one(f, flags=A.FLAG_HSV, hue=37))
    h, s, v = A.rgb_to_hsv(*f.astype(np.int64))
    assert h.min() >= 0 and h.max() < 180 and s.max() <= 255
    # the primaries and secondaries sit on the sector borders and survive the round trip
    prim = np.array([[255, 0, 0], [255, 255, 0], [0, 255, 0], [0, 255, 255], [0, 0, 255], [255, 0, 255]]).T
    h, s, v = A.rgb_to_hsv(*prim)
    assert h.tolist() == [0, 30, 60, 90, 120, 150] and (s == 255).all() and (v == 255).all()
    assert np.array_equal(np.stack(A.hsv_to_rgb(h, s, v)), prim)
    # with the flag off the stage is skipped whatever the shifts say
    assert np.array_equal(_one(f, flags=0, hue=20, sat=-30, val=9), f)
    # the round trip alone moves a sample by a few levels at the most (integer H has 180 steps)
    back = np.stack(A.hsv_to_rgb(*A.rgb_to_hsv(*f.astype(np.int64))))
    assert np.abs(back - f).max() <= 5


def test_flip_and_luts():
    f = smooth_u8(1, 17, 33, seed=3)[0].numpy()
    once = _one(f, flags=A.FLAG_FLIP)
    assert np.array_equal(once, f[:, :, ::-1]) and np.array_equal(_one(once, flags=A.FLAG_FLIP), f)
    lut = np.stack([np.clip(np.arange(256) + d, 0, 255) for d in (-20, 3, 250)]).astype(np.uint8)
    out = _one(f, flags=A.FLAG_RGB_LUT, rgb_lut=lut)
    assert np.array_equal(out, np.clip(f.astype(np.int64) + np.array([-20, 3, 250])[:, None, None], 0, 255))
    assert np.array_equal(_one(f, flags=0, rgb_lut=lut), f)
    tone = (255 - np.arange(256)).astype(np.uint8)
    assert np.array_equal(_one(f, flags=A.FLAG_TONE_LUT, tone_lut=tone), 255 - f)
    # flip comes after compression: mirroring the compressed frame, not compressing the mirrored one
    assert np.array_equal(_one(f, flags=A.FLAG_FLIP, quality=50), _one(f, quality=50)[:, :, ::-1])


def test_quality_scales_the_tables_the_libjpeg_way():
    t49, t50, t100, t1 = (A.quant_tables(q) for q in (49, 50, 100, 1))
    assert t49[0, 0, 0] == (16 * (5000 // 49) + 50) // 100 == 16 and t49[0, 0, 1] == (11 * 102 + 50) // 100 == 11
    assert t49[1, 0, 3] == (47 * 102 + 50) // 100 == 48 and t50[1, 0, 3] == 47      # the two branches differ here
    assert np.array_equal(t50, A._QUANT_BASE) and (t100 == 1).all() and t1.max() == 255 and t1.min() == 255
    f = smooth_u8(1, 32, 32, seed=4)[0].numpy()
    assert not np.array_equal(_one(f, quality=49), _one(f, quality=50))
    flat = np.full((3, 20, 28), 77, dtype=np.uint8)  # a flat grey frame is its DC terms: exact at quality 100 (all tables 1)
    assert np.array_equal(_one(flat, quality=100), flat)
    assert np.array_equal(_one(f, quality=140), _one(f, quality=100)) and np.array_equal(_one(f, quality=-3), f)


# ---- ClipAugment ------------------------------------------------------------------------------------------------------

def _same(p1, p2):
    return len(p1.stages) == len(p2.stages) and all(
        a[0] == b[0] and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) for a, b in zip(p1.stages, p2.stages))


def test_same_seed_same_draws_and_set_sharing():
    for spec in ("normal", "frame", "frame+normal", "dev-mode+force-rgb"):
        assert _same(A.ClipAugment(spec, seed=5).draw(3, 4), A.ClipAugment(spec, seed=5).draw(3, 4)), spec
        assert not _same(A.ClipAugment(spec, seed=5).draw(3, 4), A.ClipAugment(spec, seed=6).draw(3, 4)), spec
    p = A.ClipAugment("normal", seed=1).draw(3, 4)
    (name, sets, idx), = p.stages
    assert name == "sequence" and len(sets) == 3 and idx.tolist() == [0] * 4 + [1] * 4 + [2] * 4
    p = A.ClipAugment("frame", seed=1).draw(3, 4)
    (name, sets, idx), = p.stages
    assert name == "frame" and len(sets) == 12 and idx.tolist() == list(range(12))
    p = A.ClipAugment("frame+normal", seed=1).draw(3, 4)
    assert [s[0] for s in p.stages] == ["frame", "sequence"] and [len(s[1]) for s in p.stages] == [12, 3]
    assert A.ClipAugment("none").draw(3, 4).stages == []


def test_applied_fractions_and_ranges():
    n = 4000
    (_, s, _), = A.ClipAugment("normal", seed=12).draw(n, 1).stages
    (_, f, _), = A.ClipAugment("frame", seed=13).draw(n, 1).stages

    def near(count, p, what):
        sigma = (n * p * (1 - p)) ** 0.5
        assert abs(count - n * p) <= 4 * sigma, (what, count, n * p, sigma)

    ident = np.arange(256, dtype=np.uint8)
    for sets, qlo, flip_p, rgb_lim in ((s, 40, 0.5, 20), (f, 80, 0.0, 5)):
        near(int((sets["flags"] & A.FLAG_RGB_LUT > 0).sum()), 0.3, "rgb")
        near(int((sets["flags"] & A.FLAG_TONE_LUT > 0).sum()), 0.3, "tone")
        near(int((sets["quality"] > 0).sum()), 0.5, "jpeg")
        # HSV fires with p = 0.3, and stays flagged unless all three floor(shift) are 0: p * (1 - 1/8)
        near(int((sets["flags"] & A.FLAG_HSV > 0).sum()), 0.3 * 7 / 8, "hsv")
        if flip_p:
            near(int((sets["flags"] & A.FLAG_FLIP > 0).sum()), flip_p, "flip")
        else:
            assert not (sets["flags"] & A.FLAG_FLIP).any()
        q = sets["quality"][sets["quality"] > 0]
        assert q.min() == qlo and q.max() == 100
        for k in ("hue", "sat", "val"):
            assert set(np.unique(sets[k]).tolist()) == {-1, 0}, k   # the reference's fractional limits, truncated
            assert (sets[k][sets["flags"] & A.FLAG_HSV == 0] == 0).all(), k
        fired = sets["flags"] & A.FLAG_RGB_LUT > 0
        assert (sets["rgb_lut"][~fired] == ident).all() and (sets["tone_lut"][sets["flags"] & A.FLAG_TONE_LUT == 0] == ident).all()
        shift = sets["rgb_lut"][fired][:, :, 128].astype(int) - 128
        assert -rgb_lim <= shift.min() <= -rgb_lim + 1 and rgb_lim - 2 <= shift.max() <= rgb_lim
        mono = np.diff(sets["tone_lut"].astype(int), axis=1)
        assert (mono >= 0).all()
    (_, d, _), = A.ClipAugment("dev-mode+force-bright", seed=3).draw(50, 2).stages
    assert (d["flags"] == A.FLAG_TONE_LUT).all() and (d["quality"] == 0).all()
    (_, d, _), = A.ClipAugment("dev-mode+force-hue", seed=3).draw(400, 2).stages
    assert set(np.unique(d["flags"]).tolist()) == {0, A.FLAG_HSV}


def test_unknown_specs_raise():
    for spec in ("", "heavy", "dev-mode", "dev-mode+normal", "Normal"):
        with pytest.raises(NotImplementedError):
            A.ClipAugment(spec)
    A.ClipAugment("none")


def test_train_steps_refuse_float_or_host_frames_with_an_augment():
    a = A.ClipAugment("normal", seed=0)
    for frames in (torch.zeros(1, 2, 3, 8, 8), torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8)):
        with pytest.raises(TypeError, match="uint8 device frames"):
            harness.train_step(torch.nn.Linear(1, 1), None, [(frames, None, None, None, None, 0)], total_tasks=1, augment=a)
        with pytest.raises(TypeError, match="uint8 device frames"):
            harness.compinv_train_step(torch.nn.Linear(1, 1), None, [(frames, None)], augment=a)
        with pytest.raises(TypeError, match="uint8 device"):
            a(frames)
    with pytest.raises(ValueError, match="set indices"):
        A.AugmentParams([("sequence", A.new_sets(1), np.zeros(3, np.int32))], 2, 2)
