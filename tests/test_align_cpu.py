"""CPU side of the device face alignment: the align header against its ctypes table, the refusals, the integer restatement
against exact float64 bilinear sampling and against PIL's affine transform, the landmark fit, the crop origin, smoothing,
missing faces, windows, and `infer_raw_video`'s clip cutting."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dfd_clip_amd import align as AL
from dfd_clip_amd import capi, harness
from tests import align_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dfdclip_align.h")


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


# ---- ABI ------------------------------------------------------------------------------------------------------------

def test_align_header_ctypes_table_and_exports_agree():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    fns = sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", _header_text())))
    assert fns == sorted(capi.ALIGN_SIGNATURES) == ["dfd_align_crop_u8"]
    others = (set(capi.SIGNATURES) | set(capi.EXT_SIGNATURES) | set(capi.EXPLAIN_SIGNATURES) | set(capi.AUGMENT_SIGNATURES) |
              set(capi.HOOK_SIGNATURES))
    assert not set(fns) & others
    for name in fns:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == capi.ALIGN_SIGNATURES[name][1]
        params = re.search(name + r"\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
        assert len(params.split(",")) == len(capi.ALIGN_SIGNATURES[name][1])
    assert lib.dfd_abi_version() == capi.ABI_VERSION == 17


def test_frame_record_has_the_documented_size_and_layout():
    text = open(HEADER).read()
    documented = int(re.search(r"#define\s+DFD_ALIGN_FRAME_BYTES\s+(\d+)", text).group(1))
    assert ctypes.sizeof(capi.AlignFrame) == documented == capi.ALIGN_FRAME_BYTES == AL.REC_DTYPE.itemsize == 72
    for name, _ in capi.AlignFrame._fields_:
        assert getattr(capi.AlignFrame, name).offset == AL.REC_DTYPE.fields[name][1], name
    defs = {k: int(v) for k, v in re.findall(r"#define\s+DFD_ALIGN_([A-Z_]+)\s+(\d+)u?\b", text)}
    assert defs == {"HWC": capi.ALIGN_HWC, "CHW": capi.ALIGN_CHW, "SWAP_RB": capi.ALIGN_SWAP_RB,
                    "FRAME_INVALID": capi.ALIGN_FRAME_INVALID, "FRAME_BYTES": 72}


def test_refusals_return_an_error_without_launching():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    src, out, rec = 1 << 30, 1 << 31, 1 << 32  # never dereferenced: every call returns at its checks
    fn = lib.dfd_align_crop_u8

    def refused(word, **over):
        a = dict(src=src, layout=0, rs=64 * 3, fs=64 * 48 * 3, wh=48, ww=64, out=out, n=2, oh=150, ow=150, rec=rec, flags=0)
        a.update(over)
        rc = fn(a["src"], a["layout"], a["rs"], a["fs"], a["wh"], a["ww"], a["out"], a["n"], a["oh"], a["ow"], a["rec"], a["flags"], None)
        msg = lib.dfd_last_error()
        assert rc == -1 and word in msg, (over, rc, msg)

    refused(b"overlap", out=src)                                 # out on top of the input
    refused(b"overlap", out=src + 2 * 64 * 48 * 3 - 1)           # out starting on the input's last byte
    refused(b"overlap", src=out + 2 * 3 * 150 * 150 - 1)         # the input starting on out's last byte
    refused(b"bad frame count", n=-1)
    refused(b"bad window size", wh=0)
    refused(b"bad window size", ww=-3)
    refused(b"bad output size", oh=0)
    refused(b"bad output size", ow=-1)
    refused(b"smaller than a row", rs=64 * 3 - 1)
    refused(b"smaller than a row", layout=1, rs=63)
    refused(b"smaller than a frame", fs=47 * 64 * 3 + 64 * 3 - 1)
    refused(b"no parameter records", rec=None)
    refused(b"null pointer", src=None)
    refused(b"unknown layout", layout=2)
    refused(b"unknown flag", flags=2)
    refused(b"8-byte aligned", rec=rec + 4)
    # the planar row bound is a third of the interleaved one, and touching buffers are fine: only n == 0 gets this far without a GPU
    assert fn(src, 1, 64, 3 * 48 * 64, 48, 64, out, 0, 150, 150, None, 0, None) == 0
    assert fn(None, 0, 64 * 3, 0, 48, 64, None, 0, 150, 150, None, 1, None) == 0  # nothing to do


# ---- the restatement against exact bilinear sampling and against PIL ------------------------------------------------

def _random_cases(n=40, seed=2026):
    """scale 0.4-2.5, rotation +-0.6 rad, sources 120..400 a side, alternating image-like and uniform-noise content; the
    first cases are fixed so that the crop lies wholly inside the source."""
    rng = np.random.default_rng(seed)
    cases = [(0.5, 0.0, 400, 400, "smooth"), (0.5, 0.3, 400, 400, "noise")]
    while len(cases) < n:
        cases.append((float(np.exp(rng.uniform(np.log(0.4), np.log(2.5)))), float(rng.uniform(-0.6, 0.6)), int(rng.integers(120, 401)),
                      int(rng.integers(120, 401)), "smooth" if len(cases) % 2 == 0 else "noise"))
    return cases


def _case_inputs(k, case):
    scale, theta, h, w, kind = case
    frame = (C.smooth_hwc if kind == "smooth" else C.noise_hwc)(1, h, w, seed=100 + k)
    plan = C.plan_from([C.centred(scale, theta, (h, w), shift=(0.37 * k % 5, -0.21 * k % 3))], [(53, 53)])
    return frame, plan


def test_restatement_against_exact_bilinear():
    """|restatement - float64 bilinear of the zero-padded source under the unrounded inverse| <= 0.5 + 0.04 G, G = the largest
    step between adjacent pixels of the padded source: the coordinate is off by at most 1/64 px (the 1/32 grid) plus
    511 * 2^-17 px (Q16 entries times coordinates below 511), under 0.02 px per axis; bilinear interpolation is G-Lipschitz
    per axis; one rounding to an integer adds 0.5."""
    worst = 0.0
    for k, case in enumerate(_random_cases()):
        frame, plan = _case_inputs(k, case)
        got = AL.align_reference(frame, plan)[0].astype(np.float64)
        want, _, _ = C.exact_bilinear(frame[0], plan.inverse[0], plan.origin[0], 150, 150)
        G = C.largest_step(np.pad(frame[0], ((1, 1), (1, 1), (0, 0))))
        d = float(np.abs(got - want).max())
        print(f"case {k} {case}: max |d| {d:.3f}  bound {0.5 + 0.04 * G:.2f}")
        assert d <= 0.5 + 0.04 * G, (k, case, d, G)
        worst = max(worst, d)
    assert worst > 0.0  # the comparison saw real differences, not two copies of one computation


def test_restatement_against_pil_affine():
    """Against PIL's Image.transform(AFFINE, BILINEAR) per channel, on pixels whose source position lies in [1, W-2] x
    [1, H-2] (PIL's edge rule differs): |diff| <= 1 + 0.04 G, two roundings, G from the unpadded source.  PIL samples at
    pixel centres, hence the shift of the translation by 0.5 - 0.5 a - 0.5 b."""
    Image = pytest.importorskip("PIL.Image")
    covered = []
    for k, case in enumerate(_random_cases()):
        frame, plan = _case_inputs(k, case)
        got = AL.align_reference(frame, plan)[0].astype(np.int64)
        inv, (x0, y0) = plan.inverse[0], plan.origin[0]
        h, w = frame.shape[1:3]
        (a, b, c), (d, e, f) = inv
        c, f = a * x0 + b * y0 + c, d * x0 + e * y0 + f              # output pixel (j, i) is canvas pixel (x0 + j, y0 + i)
        data = (a, b, c + 0.5 - 0.5 * a - 0.5 * b, d, e, f + 0.5 - 0.5 * d - 0.5 * e)
        want = np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(frame[0, :, :, ch])).transform(
            (150, 150), Image.Transform.AFFINE, data, resample=Image.Resampling.BILINEAR)) for ch in range(3)]).astype(np.int64)
        _, x, y = C.exact_bilinear(frame[0], inv, (x0, y0), 150, 150)
        interior = (x >= 1) & (x <= w - 2) & (y >= 1) & (y <= h - 2)
        covered.append(float(interior.mean()))
        if not interior.any():
            continue
        G = C.largest_step(frame[0])
        dmax = int(np.abs(got - want)[:, interior].max())
        print(f"case {k} {case}: interior {100 * covered[-1]:.0f} %  max |d| {dmax}  bound {1 + 0.04 * G:.2f}")
        assert dmax <= 1 + 0.04 * G, (k, case, dmax, G)
    assert max(covered) > 0.9 and sum(c > 0.5 for c in covered) >= 5, covered  # the check did not pass empty


# ---- fit ---------------------------------------------------------------------------------------------------------------

def test_fit_recovers_a_known_similarity():
    rng = np.random.default_rng(0)
    pts = rng.uniform(0, 500, (8, 2))
    for scale, theta, tx, ty in ((1.0, 0.0, 0.0, 0.0), (0.37, 0.5, 12.5, -40.0), (2.5, -1.2, -300.0, 77.0), (1.1, 3.0, 5.0, 5.0)):
        M = C.similarity(scale, theta, tx, ty)
        assert np.abs(AL.fit_similarity(pts, C.apply_affine(M, pts)) - M).max() <= 1e-9
    assert np.abs(AL.invert_affine(M) @ np.vstack([M, [0, 0, 1]]) - np.eye(3)[:2]).max() <= 1e-12


def test_fit_with_noise_is_the_least_squares_solution():
    rng = np.random.default_rng(1)
    src = rng.uniform(0, 300, (8, 2))
    dst = C.apply_affine(C.similarity(0.8, 0.4, 20.0, -11.0), src) + rng.normal(0, 2.0, (8, 2))
    # u = a x - b y + tx, v = b x + a y + ty: linear in (a, b, tx, ty)
    A = np.zeros((16, 4))
    A[0::2] = np.stack([src[:, 0], -src[:, 1], np.ones(8), np.zeros(8)], 1)
    A[1::2] = np.stack([src[:, 1], src[:, 0], np.zeros(8), np.ones(8)], 1)
    a, b, tx, ty = np.linalg.lstsq(A, dst.reshape(-1), rcond=None)[0]
    M = AL.fit_similarity(src, dst)
    assert np.abs(M - np.array([[a, -b, tx], [b, a, ty]])).max() <= 1e-9
    assert M[0, 0] == M[1, 1] and M[0, 1] == -M[1, 0]  # a similarity without reflection


def test_plan_fits_the_stable_points_onto_the_shifted_reference():
    ref = C.mean_face(300)
    aligner = AL.FaceAligner(ref, canvas=256, crop=150, reference_size=300)
    want = C.similarity(0.6, 0.2, 30.0, -15.0)                       # frame -> 256 canvas
    lm = C.apply_affine(AL.invert_affine(want), ref - (300 - 256) / 2.0)[None]
    plan = aligner.plan(lm)
    assert np.abs(plan.forward[0] - want).max() <= 1e-9 and plan.valid.all()
    assert np.abs(plan.inverse[0] - AL.invert_affine(want)).max() <= 1e-9
    assert np.array_equal(plan.records["q"][0], np.rint(plan.inverse[0].reshape(-1) * 65536).astype(np.int64))
    assert np.array_equal(AL.FaceAligner(ref, canvas=256, reference_size=300).stable_reference, ref[list(AL.STABLE_POINTS)] - 22.0)
    mine = np.repeat(C.similarity(1.5, 0.0, 3.0, 4.0)[None], 1, 0)   # the caller's own matrix replaces the fit
    assert np.array_equal(aligner.plan(lm, transforms=mine).forward, mine)


# ---- crop origin -----------------------------------------------------------------------------------------------------

def _origin_for_centre(cx, cy, **kw):
    aligner = AL.FaceAligner(C.mean_face(), **kw)
    lm = np.zeros((1, 68, 2))
    lm[0, :15] = (-1000.0, 5000.0)      # points outside [start_idx, stop_idx) do not count
    lm[0, 15:] = (cx, cy)
    return tuple(aligner.plan(lm, transforms=np.array([[[1.0, 0, 0], [0, 1.0, 0]]])).origin[0])


def test_crop_origin_clamps_and_rounds_half_to_even():
    # crop 150 on a 256 canvas: half = 75, the centre is clamped to [75, 181], origin = round(centre) - 75
    assert _origin_for_centre(128.0, 128.0) == (53, 53)
    assert _origin_for_centre(10.0, 128.0) == (0, 53)       # left:   75 - 75
    assert _origin_for_centre(250.0, 128.0) == (106, 53)    # right:  181 - 75
    assert _origin_for_centre(128.0, -40.0) == (53, 0)      # top
    assert _origin_for_centre(128.0, 1e6) == (53, 106)      # bottom
    assert _origin_for_centre(74.99, 181.01) == (0, 106)
    assert _origin_for_centre(100.5, 101.5) == (25, 27)     # halves go to the even neighbour: 100 and 102
    assert _origin_for_centre(100.49, 100.51) == (25, 26)
    assert _origin_for_centre(180.5, 181.5) == (105, 106)   # 180.5 -> 180; 181.5 is clamped to 181 first
    assert _origin_for_centre(60.0, 70.0, canvas=128, crop=100) == (10, 20)
    assert _origin_for_centre(20.0, 120.0, canvas=128, crop=100) == (0, 28)
    with pytest.raises(ValueError, match="even"):
        AL.FaceAligner(C.mean_face(), crop=151)
    with pytest.raises(ValueError, match="does not fit"):
        AL.FaceAligner(C.mean_face(), canvas=100, crop=150)


def test_identity_with_an_integer_origin_copies_source_pixels():
    frame = C.noise_hwc(2, 220, 260, seed=3)
    plan = C.plan_from([C.similarity(1.0, 0.0), C.similarity(1.0, 0.0, 7.0, -3.0)], [(40, 30), (53, 53)])
    got = AL.align_reference(frame, plan)
    assert np.array_equal(got[0], frame[0, 30:180, 40:190].transpose(2, 0, 1))
    assert np.array_equal(got[1], frame[1, 56:206, 46:196].transpose(2, 0, 1))   # canvas (X, Y) is source (X - 7, Y + 3)
    assert np.array_equal(AL.align_reference(frame, plan, swap_rb=True), got[:, ::-1])
    assert np.array_equal(AL.align_reference(frame.transpose(0, 3, 1, 2), plan, layout="chw"), got)
    out = AL.align_reference(frame[:, :100, :120], plan)                           # the crop leaves a smaller source
    assert np.array_equal(out[0, :, :70, :80], got[0, :, :70, :80]) and not out[0, :, 70:].any() and not out[0, :, :, 80:].any()


# ---- smoothing and missing faces -------------------------------------------------------------------------------------

def test_smoothing_matches_the_intended_window():
    rng = np.random.default_rng(5)
    lm = rng.uniform(50, 200, (5, 68, 2))
    assert np.array_equal(AL.smooth_landmarks(lm, 0), lm)
    assert np.array_equal(AL.FaceAligner(C.mean_face()).plan(lm).landmarks, lm)    # the default is the reference: no smoothing
    want = lm.copy()
    for i, w in enumerate((0, 1, 2, 1, 0)):                                        # min(2, i, 4 - i)
        sm = np.mean([lm[x] for x in range(i - w, i + w + 1)], axis=0)
        want[i] = sm + (lm[i].mean(axis=0) - sm.mean(axis=0))
    got = AL.smooth_landmarks(lm, 2)
    assert np.abs(got - want).max() <= 1e-12 and not np.array_equal(got[2], lm[2])
    assert np.abs(AL.FaceAligner(C.mean_face(), smooth=2).plan(lm).landmarks - want).max() <= 1e-12


def test_missing_faces_are_invalid_and_come_out_as_border():
    ref = C.mean_face()
    lm = np.repeat(C.apply_affine(AL.invert_affine(C.centred(0.8, 0.1, (200, 240))), ref)[None], 4, 0)
    lm[1, 30, 0] = np.nan
    lm[3] = np.inf
    frames = C.smooth_hwc(4, 200, 240, seed=8)
    for border in (0, 200):
        plan = AL.FaceAligner(ref, border=border).plan(lm)
        assert plan.valid.tolist() == [True, False, True, False]
        assert (plan.records["flags"] == [0, 1, 0, 1]).all() and (plan.records["border"] == border).all()
        out = AL.align_reference(frames, plan)
        assert (out[1] == border).all() and (out[3] == border).all()
        assert np.array_equal(out[0], AL.align_reference(frames[:1], AL.FaceAligner(ref, border=border).plan(lm[:1]))[0])
        assert len(np.unique(out[0])) > 50
    smoothed = AL.FaceAligner(ref, smooth=1).plan(lm)      # a missing neighbour is left out of the mean, it does not spread
    assert smoothed.valid.tolist() == [True, False, True, False] and np.isfinite(smoothed.landmarks[[0, 2]]).all()


# ---- windows -------------------------------------------------------------------------------------------------------

def test_window_covers_every_tap_of_every_valid_frame():
    H, W = 300, 420
    frames = C.noise_hwc(4, H, W, seed=13)
    fwd = [C.centred(1.6, 0.3, (H, W), shift=(-30, 12)), C.centred(2.2, -0.5, (H, W), shift=(55, -20)), C.centred(1.0, 0.0, (H, W)),
           C.centred(1.9, 0.1, (H, W), shift=(500, 0))]              # the last one looks past the frame's left edge
    plan = C.plan_from(fwd, [(53, 53), (40, 60), (0, 106), (53, 53)], border=7, valid=[True, True, False, True])
    full = AL.align_reference(frames, plan)
    P = 400                                                    # unclamped windows may hang over the frame: what the full frame
    padded = np.full((4, H + 2 * P, W + 2 * P, 3), 7, dtype=np.uint8)  # gives as border there, the slice must hold as well
    padded[:, P:P + H, P:P + W] = frames

    def cut(org, wh, ww, x_off=0):
        return np.stack([padded[f, P + y:P + y + wh, P + x + x_off:P + x + ww] for f, (x, y) in enumerate(org)])

    for margin, frame_size in ((0, (H, W)), (3, (H, W)), (0, None)):
        (wh, ww), org = plan.window(margin, frame_size)
        assert wh < H and ww < W and org.shape == (4, 2)
        if frame_size is not None:                             # kept inside the frame: plain slices of the frames
            assert (org >= 0).all() and (org[:, 0] + ww <= W).all() and (org[:, 1] + wh <= H).all()
        assert np.array_equal(AL.align_reference(cut(org, wh, ww), plan.with_window(org, (wh, ww))), full)
    (wh, ww), org = plan.window(0, None)
    shrunk = plan.with_window(org + [1, 0], (wh, ww - 1))      # one column short on the left: the cover is tight for some frame
    assert not np.array_equal(AL.align_reference(cut(org, wh, ww, x_off=1), shrunk), full)


# ---- infer_raw_video ---------------------------------------------------------------------------------------------------

class _HostAligner(AL.FaceAligner):
    """The aligner with the restatement in place of the kernel, so that the clip cutting runs without a GPU."""

    @staticmethod
    def apply(frames_u8, plan, layout="hwc", swap_rb=False):
        return torch.from_numpy(AL.align_reference(frames_u8.numpy(), plan, layout=layout, swap_rb=swap_rb))


def _stub_score(x, m):
    """One number per clip from its pixels and its mask, in integers: the same whatever the chunking."""
    return ((x.to(torch.int64).sum(dim=(1, 2, 3, 4)) % 97) + 100 * m.to(torch.int64).sum(dim=1)).float() / 64.0


class _StubModel:
    num_frames = 4

    def __init__(self):
        self.calls = []

    def eval(self):
        return self

    def predict(self, x, m):
        self.calls.append((x.clone(), m.clone()))
        s = _stub_score(x, m)
        return [torch.stack([s, -s], dim=1), torch.stack([-s, 2 * s], dim=1)], {}


def test_infer_raw_video_cuts_clips_and_drops_the_ragged_tail():
    T, F = 4, 2 * 4 + 3
    ref = C.mean_face()
    frames = torch.from_numpy(C.smooth_hwc(F, 120, 160, seed=21))
    lm = np.repeat(C.apply_affine(AL.invert_affine(C.centred(1.2, 0.05, (120, 160))), ref)[None], F, 0)
    lm += np.random.default_rng(2).normal(0, 0.5, lm.shape)
    lm[5] = np.nan                                                  # no face in frame 5 = clip 1, position 1
    aligner = _HostAligner(ref)
    crops = AL.align_reference(frames.numpy(), aligner.plan(lm))
    for batch_size, calls in ((16, 1), (1, 2)):
        model = _StubModel()
        prob, clip_probs, logits = harness.infer_raw_video(model, frames, lm, aligner, batch_size=batch_size, task_index=1, with_logits=True)
        assert len(model.calls) == calls
        x = torch.cat([c[0] for c in model.calls])
        m = torch.cat([c[1] for c in model.calls])
        assert x.dtype == torch.uint8 and tuple(x.shape) == (2, T, 3, 150, 150) and tuple(m.shape) == (2, T) and m.dtype == torch.bool
        assert np.array_equal(x.numpy().reshape(2 * T, 3, 150, 150), crops[:2 * T])          # consecutive frames; 8, 9, 10 dropped
        assert m.tolist() == [[True] * 4, [True, False, True, True]]
        s = _stub_score(x, m)
        want = torch.stack([-s, 2 * s], dim=1)                                                # task 1's logits
        assert torch.equal(logits, want) and torch.equal(clip_probs, want.softmax(dim=-1))
        assert tuple(clip_probs.shape) == (2, 2) and torch.equal(prob, clip_probs.mean(dim=0)[1])
    assert len(harness.infer_raw_video(_StubModel(), frames, lm, aligner)) == 2
    with pytest.raises(ValueError, match="do not fill one clip"):
        harness.infer_raw_video(_StubModel(), frames[:3], lm[:3], aligner)


def test_apply_refuses_host_float_and_misshapen_frames():
    plan = C.plan_from([C.similarity(1.0, 0.0)], [(0, 0)])
    with pytest.raises(TypeError, match="uint8 device frames"):
        AL.FaceAligner.apply(torch.zeros(1, 64, 64, 3, dtype=torch.uint8), plan)
    with pytest.raises(TypeError, match="uint8 device frames"):
        AL.FaceAligner.apply(np.zeros((1, 64, 64, 3), np.uint8), plan)
    with pytest.raises(ValueError, match="singular"):
        C.plan_from([np.zeros((2, 3))], [(0, 0)])
