"""GPU tests of the device face alignment (`dfd_align_crop_u8`, csrc/align.hip): the kernel must equal the integer
restatement `align.align_records_reference` BIT FOR BIT (torch.equal) on padded strides in both layouts, on an output plane
whose size is no multiple of 4, far outside the source, on windows, on the identity, with swapped channels, on invalid
frames, on one frame and on none; and `infer_raw_video` must give the logits of `Detector.predict` on the restatement's crops.

Every kernel call goes through `run`: the source sits in an exactly sized image (the last frame ends with the last pixel of
its last row) whose row and frame padding is poisoned, in front of a poisoned guard; the output sits between guards; all of
them are checked after the launch, and the poison is a value that would change the result if it were read."""
import functools

import numpy as np
import pytest
import torch

from dfd_clip_amd import align as AL
from dfd_clip_amd import capi
from tests import align_cases as C
from tests.cases import make_config
from tests.guarded import guarded_1d

pytestmark = pytest.mark.gpu


def pack(frames, layout, row_pad, frame_pad, poison):
    """frames [F,H,W,3] / [F,3,H,W] -> (byte image, row stride, frame stride, win_h, win_w): rows `row_pad` bytes apart
    beyond their length, frames `frame_pad` bytes beyond their span, every byte that is no pixel = `poison`."""
    F = len(frames)
    H, W = frames.shape[1:3] if layout == "hwc" else frames.shape[2:4]
    rows, row_bytes = (H, 3 * W) if layout == "hwc" else (3 * H, W)
    rs = row_bytes + row_pad
    span = (rows - 1) * rs + row_bytes
    fs = span + frame_pad
    img = np.full((F - 1) * fs + span, poison, dtype=np.uint8)
    data = np.ascontiguousarray(frames).reshape(F, rows, row_bytes)
    for f in range(F):
        for r in range(rows):
            o = f * fs + r * rs
            img[o:o + row_bytes] = data[f, r]
    return img, rs, fs, H, W


def run(frames, records, out_h, out_w, layout="hwc", swap_rb=False, row_pad=5, frame_pad=77, poison=255, out_fill=0xA5):
    """-> the kernel's output as an ndarray [F,3,out_h,out_w]; guards, padding and the input itself checked."""
    F = len(frames)
    img, rs, fs, H, W = pack(frames, layout, row_pad, frame_pad, poison)
    inp = guarded_1d(img.size, torch.uint8, fill=poison, name="in").set(torch.from_numpy(img))
    out = guarded_1d(F * 3 * out_h * out_w, torch.uint8, fill=out_fill, name="out")
    rec = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(F, -1).copy()).cuda()
    capi.align_crop_u8(inp.t[0], out.shaped(F, 3, out_h, out_w), rec, AL._LAYOUTS[layout], rs, fs, H, W, swap_rb=swap_rb)
    torch.cuda.synchronize()
    out.assert_untouched()
    inp.assert_untouched(view_too=True)
    return out.shaped(F, 3, out_h, out_w).cpu().numpy()


def same(got, want):
    if not torch.equal(torch.from_numpy(got), torch.from_numpy(want)):
        bad = np.argwhere(got != want)
        f, c, y, x = bad[0]
        raise AssertionError(f"{len(bad)} of {got.size} samples differ; first at frame {f} channel {c} ({y}, {x}): "
                             f"kernel {got[f, c, y, x]} restatement {want[f, c, y, x]}; frames {sorted(set(bad[:, 0].tolist()))}")


def as_layout(frames_hwc, layout):
    return frames_hwc if layout == "hwc" else np.ascontiguousarray(frames_hwc.transpose(0, 3, 1, 2))


def check(frames_hwc, records, out_h, out_w, layout, swap_rb=False, **kw):
    """Kernel against restatement under two poisons and two output pre-fills; returns the result."""
    frames = as_layout(frames_hwc, layout)
    want = AL.align_records_reference(frames, records, out_h, out_w, layout=layout, swap_rb=swap_rb)
    same(run(frames, records, out_h, out_w, layout, swap_rb, poison=255, out_fill=0xA5, **kw), want)
    same(run(frames, records, out_h, out_w, layout, swap_rb, poison=0, out_fill=0x5A, **kw), want)
    return want


@functools.lru_cache(maxsize=None)
def three_similarities():
    """3 frames of 64x48 and a plan: scale 0.4, scale 2.5 with rotation 0.5 rad, and a crop that leaves the source on two
    sides (shifted towards the lower right)."""
    frames = C.smooth_hwc(3, 48, 64, seed=31)
    plan = C.plan_from([C.centred(0.4, 0.0, (48, 64)), C.centred(2.5, 0.5, (48, 64)), C.centred(3.0, -0.2, (48, 64), shift=(-60.0, -45.0))],
                       [(53, 53), (53, 53), (41, 60)], border=9)
    return frames, plan


# ---- 1: padded strides, both layouts, border taps -------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_three_similarities_on_padded_strides(layout):
    frames, plan = three_similarities()
    want = check(frames, plan.records, 150, 150, layout)
    for f in range(3):   # every frame mixes source content with border
        assert (want[f] == 9).all(axis=0).any() and len(np.unique(want[f])) > 30, f
    assert (want[2, :, -1, :] == 9).all() and (want[2, :, :, -1] == 9).all() and not (want[2, :, 0, 0] == 9).all()
    same(run(as_layout(frames, layout), plan.records, 150, 150, layout, row_pad=0, frame_pad=0), want)   # and dense


# ---- 2: an output plane of 1517 bytes --------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["hwc", "chw"])
def test_odd_output_plane_takes_the_tail_path(layout):
    frames = C.smooth_hwc(3, 80, 96, seed=32)
    rec = C.plan_from([C.centred(1.3, 0.25, (80, 96)), C.centred(0.9, -0.4, (80, 96)), C.centred(2.0, 0.1, (80, 96))],
                      [(100, 110), (90, 95), (117, 101)], border=3).records
    want = check(frames, rec, 37, 41, layout)   # 37 * 41 = 1517: frames 1 and 2 start on odd addresses, each plane ends in one byte
    assert all(len(np.unique(want[f])) > 30 for f in range(3))
    check(frames, rec, 41, 37, layout, swap_rb=True)
    check(frames[:1], rec[:1], 1, 1, layout)
    check(frames[:2], rec[:2], 3, 2, layout)    # planes shorter than one group, a group across three rows


# ---- 3: far outside ----------------------------------------------------------------------------------------------------

def test_far_translations_give_border_and_do_not_wrap():
    frames = C.noise_hwc(6, 48, 64, seed=33)
    fwd = [C.similarity(1.0, 0.0, 1e6, 0.0), C.similarity(1.0, 0.0, -1e6, 0.0), C.similarity(1.0, 0.0, 0.0, 1e6), C.similarity(0.7, 0.3, -1e6, -1e6)]
    rec = np.concatenate([C.plan_from(fwd, [(53, 53)] * 4, border=77).records] * 2)[:6]
    # 2^32 and 2^40 source pixels away: positions that a 32-bit coordinate would fold back onto the frame
    rec["q"][4] = [65536, 0, (1 << 32) * 65536, 0, 65536, 0]
    rec["q"][5] = [65536, 0, 0, 0, 65536, -(1 << 40) * 65536]
    rec["x0"][4:], rec["y0"][4:] = 0, 0
    for layout in ("hwc", "chw"):
        want = check(frames, rec, 150, 150, layout)
        assert (want == 77).all()
    near = rec.copy()
    near["q"][4][2] = 0                         # the same record without the offset does read the frame
    assert not (AL.align_records_reference(frames, near, 150, 150)[4] == 77).all()


# ---- 4: windows ---------------------------------------------------------------------------------------------------------

def test_windows_at_per_frame_origins_equal_the_full_frames():
    H, W = 120, 160
    frames = C.smooth_hwc(3, H, W, seed=34)
    plan = C.plan_from([C.centred(5.0, 0.1, (H, W), shift=(40.0, -25.0)), C.centred(4.6, -0.15, (H, W), shift=(-260.0, 140.0)),
                        C.centred(5.5, 0.0, (H, W), shift=(330.0, 230.0))], [(53, 53), (20, 90), (106, 0)], border=5)
    (wh, ww), org = plan.window(0, (H, W))
    assert wh <= 40 and ww <= 40 and len({tuple(o) for o in org}) == 3
    org = np.stack([np.minimum(org[:, 0], W - 40), np.minimum(org[:, 1], H - 40)], 1)        # 40x40 windows inside the frame
    windows = np.stack([frames[f, y:y + 40, x:x + 40] for f, (x, y) in enumerate(org)])
    windowed = plan.with_window(org, (40, 40))
    full = AL.align_reference(frames, plan)
    for layout in ("hwc", "chw"):
        same(check(windows, windowed.records, 150, 150, layout), full)
        check(frames, plan.records, 150, 150, layout)
    moved = plan.with_window(org + [9, -7], (40, 40))   # the same bytes declared elsewhere: part of each footprint now misses
    part = check(windows, moved.records, 150, 150, "hwc")  # its window (border there), the rest reads other pixels
    assert (part == 5).all(axis=1).any() and (part == full).mean() < 0.9


# ---- 5: identity, swapped channels, invalid frames ---------------------------------------------------------------------

@pytest.mark.parametrize("border", [0, 200])
def test_identity_swap_and_invalid_frames(border):
    frames = C.noise_hwc(4, 170, 200, seed=35)
    plan = C.plan_from([C.similarity(1.0, 0.0), C.similarity(1.0, 0.0, 7.0, -3.0), C.similarity(1.0, 0.0), C.similarity(2.0, 0.3)],
                       [(40, 10), (30, 2), (0, 0), (53, 53)], border=border, valid=[True, True, False, False])
    for layout in ("hwc", "chw"):
        got = check(frames, plan.records, 150, 150, layout)
        assert np.array_equal(got[0], frames[0, 10:160, 40:190].transpose(2, 0, 1))
        assert np.array_equal(got[1], frames[1, 5:155, 23:173].transpose(2, 0, 1))
        assert (got[2:] == border).all()
        same(check(frames, plan.records, 150, 150, layout, swap_rb=True), got[:, ::-1].copy())
    wild = plan.records.copy()                      # an invalid frame's other fields are never used
    wild["q"][2:] = -(1 << 62)
    wild["border"][3] = border + 1000 if border else -5   # clamped to 0..255
    got = check(frames, wild, 150, 150, "hwc")
    assert (got[2] == border).all() and (got[3] == (255 if border else 0)).all()


# ---- 6: one frame, no frame ------------------------------------------------------------------------------------------

def test_single_frame_and_no_frame():
    frames, plan = three_similarities()
    want = AL.align_reference(frames, plan)
    for f in range(3):
        same(check(frames[f:f + 1], plan.records[f:f + 1], 150, 150, "hwc"), want[f:f + 1])
    out = guarded_1d(3 * 150 * 150, torch.uint8, fill=0xA5, name="out")
    src = torch.from_numpy(frames[0]).cuda()
    rec = torch.zeros(0, capi.ALIGN_FRAME_BYTES, dtype=torch.uint8, device="cuda")
    capi.align_crop_u8(src, out.shaped(1, 3, 150, 150)[:0], rec, capi.ALIGN_HWC, 3 * 64, 3 * 64 * 48, 48, 64)
    torch.cuda.synchronize()
    out.assert_untouched()
    assert bool((out.t == 0xA5).all())              # nothing was launched, nothing written
    empty = AL.FaceAligner.apply(torch.zeros(0, 48, 64, 3, dtype=torch.uint8, device="cuda"), C.plan_from(np.zeros((0, 2, 3)), np.zeros((0, 2))))
    assert tuple(empty.shape) == (0, 3, 150, 150)


def test_refusals_leave_the_output_alone():
    lib = capi.load_library()
    frames, plan = three_similarities()
    src = torch.from_numpy(frames).cuda()
    out = torch.full((3, 3, 150, 150), 0xA5, dtype=torch.uint8, device="cuda")
    rec = plan.on("cuda")
    args = lambda **o: [o.get("src", src.data_ptr()), o.get("layout", 0), o.get("rs", 192), 192 * 48, 48, 64, o.get("out", out.data_ptr()), 3, 150, 150,
                        o.get("rec", rec.data_ptr()), o.get("flags", 0), None]
    for over, word in ((dict(out=src.data_ptr() + 100), b"overlap"), (dict(rs=191), b"smaller than a row"), (dict(layout=7), b"unknown layout"),
                       (dict(flags=4), b"unknown flag"), (dict(rec=None), b"no parameter records")):
        assert lib.dfd_align_crop_u8(*args(**over)) == -1 and word in lib.dfd_last_error(), over
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and torch.equal(src.cpu(), torch.from_numpy(frames))
    with pytest.raises(capi.DfdError):
        capi.align_crop_u8(src.cpu(), out, rec, 0, 192, 192 * 48, 48, 64)
    assert lib.dfd_align_crop_u8(*args()) == 0       # and the same call without a fault in it runs
    torch.cuda.synchronize()
    same(out.cpu().numpy(), AL.align_reference(frames, plan))


# ---- through FaceAligner and infer_raw_video -----------------------------------------------------------------------------

def _video(F, H, W, seed, missing=()):
    """Frames with a face drifting and turning slowly, its landmarks, and the aligner."""
    ref = C.mean_face()
    frames = C.smooth_hwc(F, H, W, seed=seed)
    rng = np.random.default_rng(seed)
    lm = np.stack([C.apply_affine(AL.invert_affine(C.centred(1.4 + 0.02 * f, 0.03 * f - 0.1, (H, W), shift=(3.0 * f - 10, 6 - f))), ref) for f in range(F)])
    lm += rng.normal(0, 0.7, lm.shape)
    for f in missing:
        lm[f] = np.nan
    return frames, lm, AL.FaceAligner(ref, border=0)


def test_apply_equals_the_restatement_on_views_and_layouts():
    frames, lm, aligner = _video(5, 150, 190, seed=36, missing=(3,))
    plan = aligner.plan(lm)
    assert plan.valid.tolist() == [True, True, True, False, True]
    want = AL.align_reference(frames, plan)
    assert (want[3] == 0).all() and all(len(np.unique(want[f])) > 50 for f in (0, 1, 2, 4))
    dev = torch.from_numpy(frames).cuda()
    keep = dev.clone()
    got = aligner.apply(dev, plan)
    assert got.dtype == torch.uint8 and got.device == dev.device and tuple(got.shape) == (5, 3, 150, 150) and torch.equal(dev, keep)
    same(got.cpu().numpy(), want)
    same(aligner.apply(dev, plan, swap_rb=True).cpu().numpy(), want[:, ::-1].copy())
    same(aligner.apply(dev.permute(0, 3, 1, 2).contiguous(), plan, layout="chw").cpu().numpy(), want)
    same(aligner.apply(dev.permute(0, 3, 1, 2), plan, layout="chw").cpu().numpy(), want)     # a permuted view is made dense first
    crops, plan2 = aligner(dev, lm)
    same(crops.cpu().numpy(), want)
    # a window of a larger upload, read where it lies: rows and frames are padded by what surrounds the view
    (wh, ww), org = plan.window(2, (150, 190))
    assert wh < 150 and ww < 190
    big = torch.full((5, wh + 9, ww + 13, 3), 255, dtype=torch.uint8, device="cuda")
    view = big[:, 4:4 + wh, 6:6 + ww]
    view.copy_(torch.stack([dev[f, y:y + wh, x:x + ww] for f, (x, y) in enumerate(org)]))
    assert not view.is_contiguous()
    same(aligner.apply(view, plan.with_window(org, (wh, ww))).cpu().numpy(), want)
    with pytest.raises(ValueError, match="windows"):
        aligner.apply(dev, plan.with_window(org, (wh, ww)))
    with pytest.raises(TypeError, match="uint8 device frames"):
        aligner.apply(dev.float(), plan)
    with pytest.raises(ValueError, match=r"\[F,H,W,3\]"):
        aligner.apply(dev.permute(0, 3, 1, 2), plan)
    with pytest.raises(ValueError, match="the plan holds"):
        aligner.apply(dev[:4], plan)


def test_infer_raw_video_equals_predict_on_the_restatement_crops():
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.harness import infer_raw_video
    from dfd_clip_amd.weights import random_state_dict
    T = 4
    cfg = make_config("tiny", decode_mode="index", decode_indices=[0, 1])
    model = Detector(cfg, T, None, precision="fp32")
    model.load_state_dict(random_state_dict(cfg, T, seed=0))
    model = model.cuda().eval()
    F = 2 * T + 3
    frames, lm, aligner = _video(F, 150, 190, seed=37, missing=(5,))
    dev = torch.from_numpy(frames).cuda()
    prob, clip_probs, logits = infer_raw_video(model, dev, lm, aligner, with_logits=True)
    plan = aligner.plan(lm)
    crops = torch.from_numpy(AL.align_reference(frames, plan)[:2 * T]).cuda().view(2, T, 3, 150, 150)
    mask = torch.from_numpy(plan.valid[:2 * T].copy()).view(2, T).cuda()
    assert mask.tolist() == [[True] * 4, [True, False, True, True]]
    with torch.no_grad():
        want = model.predict(crops, mask)[0][0].cpu()
        unmasked = model.predict(crops, torch.ones_like(mask))[0][0].cpu()
    assert tuple(logits.shape) == (2, 2) and torch.equal(logits, want)
    assert torch.equal(logits[0], unmasked[0]) and not torch.equal(logits[1], unmasked[1])   # the invalid frame is masked out
    assert torch.equal(clip_probs, want.softmax(dim=-1)) and torch.equal(prob, clip_probs.mean(dim=0)[1])
    one_by_one = infer_raw_video(model, dev, lm, aligner, batch_size=1, with_logits=True)[2]
    # chunking changes the batch a kernel sees, not the verdict: fp32 logits of norm 5, the bar smoke() holds fp32 to
    assert torch.allclose(one_by_one, want, atol=1e-3)
    bgr = infer_raw_video(model, dev.flip(-1), lm, aligner, swap_rb=True, with_logits=True)[2]
    assert torch.equal(bgr, want)                                                         # BGR frames with swap_rb are the RGB frames
