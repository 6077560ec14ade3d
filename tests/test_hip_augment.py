"""GPU tests of the device augmentation (`dfd_augment_u8`, csrc/augment.hip): the kernel must equal the integer
restatement `augment.augment_sets_reference` BIT FOR BIT (torch.equal), for every stage alone and together, at sizes that
are one MCU, smaller than an MCU, ragged both ways, the reference's 150x150 face crop, 224x224 and an odd multi-tile size;
mixed launches; guard bands around the output and behind the input; the refusals; and the train step with `augment=`.

Every kernel call goes through `run`, which puts the output between poisoned guards (pre-filled 0xA5) and the input in
front of a poisoned guard, and checks both after the launch."""
import copy
import functools

import numpy as np
import pytest
import torch

from dfd_clip_amd import augment as A
from dfd_clip_amd import capi
from tests.cases import make_config
from tests.guarded import guarded_1d
from tests.test_hip_preprocess import smooth_u8

pytestmark = pytest.mark.gpu

SIZES = [(1, 16, 16), (2, 8, 8), (3, 17, 33), (2, 150, 150), (2, 224, 224), (5, 97, 131)]
RAGGED = {(3, 17, 33), (2, 150, 150), (5, 97, 131)}


def run(frames, sets, idx, out_fill=0xA5, in_guard=255):
    """frames uint8 ndarray [n,3,h,w] -> the kernel's output as an ndarray; guards checked."""
    n, _, h, w = frames.shape
    inp = guarded_1d(frames.size, torch.uint8, fill=in_guard, name="in").set(torch.from_numpy(frames))
    out = guarded_1d(frames.size, torch.uint8, fill=out_fill, name="out")
    sets_d = torch.from_numpy(sets.view(np.uint8).reshape(len(sets), -1).copy()).cuda()
    idx_d = torch.from_numpy(np.asarray(idx, dtype=np.int32)).cuda()
    capi.augment_u8(inp.shaped(n, 3, h, w), out.shaped(n, 3, h, w), sets_d, idx_d)
    torch.cuda.synchronize()
    out.assert_untouched()
    inp.assert_untouched(view_too=True)
    return out.shaped(n, 3, h, w).cpu().numpy()


def same(got, want):
    if not torch.equal(torch.from_numpy(got), torch.from_numpy(want)):
        bad = np.argwhere(got != want)
        f, c, y, x = bad[0]
        raise AssertionError(f"{len(bad)} of {got.size} samples differ; first at frame {f} channel {c} ({y}, {x}): "
                             f"kernel {got[f, c, y, x]} restatement {want[f, c, y, x]}; frames {sorted(set(bad[:, 0].tolist()))}")


def _luts(sets, k, seed):
    rng = np.random.default_rng(seed)
    sets["rgb_lut"][k] = np.clip(np.arange(256)[None] + rng.uniform(-20, 20, (3, 1)), 0, 255).astype(np.uint8)


def _tone(sets, k, alpha, beta):
    sets["tone_lut"][k] = np.clip(np.arange(256) * alpha + 255.0 * beta, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def stage_sets(with_flip_quality):
    """Each stage alone, then together: (names, sets)."""
    spec = [("copy", dict()), ("rgb", dict(flags=A.FLAG_RGB_LUT))]
    spec += [(f"hsv{s}", dict(flags=A.FLAG_HSV, hue=s[0], sat=s[1], val=s[2])) for s in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (37, -60, 45))]
    spec += [("hsv-extreme", dict(flags=A.FLAG_HSV, hue=-2 ** 31, sat=2 ** 31 - 1, val=-2 ** 31))]  # no overflow on the way to the clamp
    spec += [("tone", dict(flags=A.FLAG_TONE_LUT))]
    spec += [(f"q{q}", dict(quality=q)) for q in (1, 40, 49, 50, 75, 100)]
    spec += [("flip", dict(flags=A.FLAG_FLIP))]
    if with_flip_quality:
        spec += [("flip+q60", dict(flags=A.FLAG_FLIP, quality=60))]
    spec += [("all", dict(flags=A.FLAG_RGB_LUT | A.FLAG_HSV | A.FLAG_TONE_LUT | A.FLAG_FLIP, hue=37, sat=-60, val=45, quality=75)),
             ("colour+flip", dict(flags=A.FLAG_RGB_LUT | A.FLAG_HSV | A.FLAG_TONE_LUT | A.FLAG_FLIP, hue=100, sat=25, val=-30))]
    sets = A.new_sets(len(spec))
    for k, (_, fields) in enumerate(spec):
        for name, v in fields.items():
            sets[name][k] = v
        if fields.get("flags", 0) & A.FLAG_RGB_LUT:
            _luts(sets, k, seed=k)
        if fields.get("flags", 0) & A.FLAG_TONE_LUT:
            _tone(sets, k, 1.23, -0.11)
    return [s[0] for s in spec], sets


@pytest.mark.parametrize("n,h,w", SIZES)
def test_each_stage_alone_and_together(n, h, w):
    names, sets = stage_sets((n, h, w) in RAGGED)
    base = smooth_u8(n, h, w, seed=100 + h).numpy()
    frames = np.repeat(base, len(sets), axis=0)             # every frame under every set
    idx = np.tile(np.arange(len(sets), dtype=np.int32), n)
    got = run(frames, sets, idx)
    want = A.augment_sets_reference(frames, sets, idx)
    for k, name in enumerate(names):
        try:
            same(got[k::len(sets)], want[k::len(sets)])
        except AssertionError as e:
            raise AssertionError(f"set {name!r} at {n}x{h}x{w}: {e}") from None
    changed = [name for k, name in enumerate(names) if not np.array_equal(want[k::len(sets)], base)]
    assert len(changed) >= len(names) - 1, changed  # the cases are not vacuous


def _mixed_sets():
    sets = A.new_sets(3)
    sets["flags"][0] = A.FLAG_RGB_LUT | A.FLAG_TONE_LUT   # colour only
    _luts(sets, 0, seed=9)
    _tone(sets, 0, 0.8, 0.1)
    sets["quality"][1] = 55                                # JPEG only
    sets["flags"][2] = A.FLAG_HSV | A.FLAG_FLIP            # everything
    sets["hue"][2], sets["sat"][2], sets["val"][2], sets["quality"][2] = 170, 40, -20, 88
    return sets


def test_mixed_launches_and_out_of_range_indices():
    sets = _mixed_sets()
    frames = smooth_u8(7, 70, 90, seed=21).numpy()
    idx = np.array([0, 1, 2, 2, 1, 0, 1], dtype=np.int32)                       # 7 frames over 3 sets
    same(run(frames, sets, idx), A.augment_sets_reference(frames, sets, idx))
    sets = np.concatenate([sets, A.new_sets(1)])                                  # set 3 does nothing: the copy path
    idx = np.array([3, 0, 1, -1, 4, 2, 3], dtype=np.int32)                       # -1 and n_sets lie outside: copies
    got = run(frames, sets, idx)
    same(got, A.augment_sets_reference(frames, sets, idx))
    for f in (0, 3, 4, 6):
        assert np.array_equal(got[f], frames[f])
    wild = np.array([2 ** 31 - 1, -2 ** 31, 1 << 20, -7, 4, 100, 5], dtype=np.int32)  # far outside: never read
    assert np.array_equal(run(frames, sets, wild), frames)


def test_extreme_content():
    h, w = 33, 47
    yy, xx = np.mgrid[0:h, 0:w]
    checker = np.broadcast_to((((yy + xx) & 1) * 255).astype(np.uint8), (3, h, w))
    prim = np.zeros((3, h, w), np.uint8)
    for c in range(3):
        prim[c, :, c * 16:(c + 1) * 16] = 255                                    # stripes of pure red, green, blue
    frames = np.stack([np.zeros((3, h, w), np.uint8), np.full((3, h, w), 255, np.uint8), checker, prim])
    names, sets = stage_sets(True)
    picks = [names.index(k) for k in ("hsv(0, 0, -1)", "hsv(37, -60, 45)", "q1", "q40", "q100", "flip+q60", "all")]
    fr = np.repeat(frames, len(picks), axis=0)
    idx = np.tile(np.array(picks, dtype=np.int32), len(frames))
    same(run(fr, sets, idx), A.augment_sets_reference(fr, sets, idx))


def test_every_output_byte_is_written_and_no_guard_is_read():
    sets = _mixed_sets()
    frames = smooth_u8(4, 37, 51, seed=5).numpy()
    idx = np.array([0, 1, 2, 7], dtype=np.int32)
    want = A.augment_sets_reference(frames, sets, idx)
    a = run(frames, sets, idx, out_fill=0xA5, in_guard=255)
    b = run(frames, sets, idx, out_fill=0x5A, in_guard=0)   # another pre-fill, another poison behind the input
    same(a, want)
    same(b, want)


def test_refusals_leave_the_output_alone():
    lib = capi.load_library()
    frames = torch.from_numpy(smooth_u8(2, 16, 16, seed=1).numpy()).cuda()
    out = torch.full_like(frames, 0xA5)
    sets = torch.from_numpy(_mixed_sets().view(np.uint8).reshape(3, -1).copy()).cuda()
    idx = torch.zeros(2, dtype=torch.int32, device="cuda")
    with pytest.raises(capi.DfdError, match="in place"):
        capi.augment_u8(frames, frames, sets, idx)
    keep = frames.clone()
    rc = lib.dfd_augment_u8(frames.data_ptr(), out.data_ptr(), 2, 16, 16, sets.data_ptr(), 0, idx.data_ptr(), None)
    assert rc == -1 and b"no parameter set" in lib.dfd_last_error()
    torch.cuda.synchronize()
    assert torch.equal(frames, keep) and bool((out == 0xA5).all())
    with pytest.raises(capi.DfdError):
        capi.augment_u8(frames.cpu(), out, sets, idx)


# ---- through ClipAugment and the train step ---------------------------------------------------------------------------

def test_apply_equals_the_restatement_and_replays():
    clips = smooth_u8(2 * 4, 40, 52, seed=8).view(2, 4, 3, 40, 52)
    a = A.ClipAugment("frame+normal", seed=3)
    params = a.draw(2, 4)
    assert [len(s[1]) for s in params.stages] == [8, 2]
    assert any(s[1]["flags"].any() or s[1]["quality"].any() for s in params.stages)
    dev = clips.cuda()
    keep = dev.clone()
    got = a.apply(dev, params)
    assert got.data_ptr() != dev.data_ptr() and torch.equal(dev, keep)            # a new tensor; the input is untouched
    want = A.augment_reference(clips.numpy(), params)
    same(got.cpu().numpy(), want)
    assert not np.array_equal(want, clips.numpy())
    assert torch.equal(a.apply(dev.clone(), params), got)                        # replay: same params, second tensor
    none = A.ClipAugment("none")
    assert torch.equal(none(dev), dev)


class _Recording:
    """An optimizer that keeps the gradients it stepped on."""

    def __init__(self, opt, model):
        self.opt, self.model, self.grads = opt, model, None

    def step(self):
        self.grads = {k: p.grad.detach().clone() for k, p in self.model.named_parameters() if p.grad is not None}
        self.opt.step()


def _tiny_model():
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    cfg = make_config("tiny", decode_mode="index", decode_indices=[0, 1])
    model = Detector(cfg, 4, None, precision="fp32")
    model.load_state_dict(random_state_dict(cfg, 4, seed=0))
    return model.cuda()


def test_train_step_with_an_augment():
    from dfd_clip_amd.harness import train_step
    base = _tiny_model()
    clips = smooth_u8(2 * 4, 40, 52, seed=13).view(2, 4, 3, 40, 52).cuda()
    m = torch.ones(2, 4, dtype=torch.bool, device="cuda")
    y = torch.tensor([0, 1], device="cuda")

    def step(frames, **kw):
        model = copy.deepcopy(base)
        opt = _Recording(model.configure_optimizers(0.05), model)
        out = train_step(model, opt, [(frames, y, m, None, None, 0)], **kw)
        torch.cuda.synchronize()
        return out, opt.grads, {k: v.detach().clone() for k, v in model.named_parameters()}

    def equal(a, b):
        (oa, ga, pa), (ob, gb, pb) = a, b
        return (torch.equal(oa["losses"][0], ob["losses"][0]) and torch.equal(oa["logits"][0], ob["logits"][0]) and
                ga.keys() == gb.keys() and all(torch.equal(ga[k], gb[k]) for k in ga) and all(torch.equal(pa[k], pb[k]) for k in pa))

    spec, seed = "frame+normal", 4
    by_hand = A.ClipAugment(spec, seed=seed)
    params = by_hand.draw(2, 4)
    assert any(s[1]["flags"].any() or s[1]["quality"].any() for s in params.stages)
    augmented = by_hand.apply(clips, params)
    assert not torch.equal(augmented, clips)
    inside = step(clips, augment=A.ClipAugment(spec, seed=seed))
    outside = step(augmented)
    assert len(inside[1]) > 0 and equal(inside, outside)
    plain = step(clips)
    assert not torch.equal(plain[0]["losses"][0], inside[0]["losses"][0])
    assert equal(plain, step(clips, augment=None))
    with pytest.raises(TypeError, match="uint8 device frames"):
        step(clips.float(), augment=A.ClipAugment(spec, seed=seed))


def test_compinv_train_step_refuses_float_frames():
    from dfd_clip_amd.harness import compinv_train_step
    with pytest.raises(TypeError, match="uint8 device frames"):
        compinv_train_step(torch.nn.Linear(1, 1), None, [(torch.zeros(1, 2, 3, 8, 8, device="cuda"), None)], augment=A.ClipAugment("normal", seed=0))
