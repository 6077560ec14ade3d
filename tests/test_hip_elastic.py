"""GPU tests of the device elastic warp (`dfd_elastic_field`, `dfd_elastic_remap_u8`, csrc/elastic.hip): both kernels must
equal the integer restatements of `dfd-clip_amd/elastic.py` BIT FOR BIT (torch.equal, no tolerance anywhere): the field
kernel at sizes below, at and above one tile and with blur radii below, at and above the image size; the remap kernel on
hand-made fields (zero, whole and fractional shifts, every fraction of the 1/32 grid, displacements of a thousand pixels,
random) at plane sizes that are and are not multiples of 4 and frame counts that do and do not fill a chunk; the copy path;
`SslFake` end to end and inside the train step.

Every kernel call puts the output and the field workspace between poisoned guards and the input in front of one, and
checks them after the launch."""
import copy
import functools

import numpy as np
import pytest
import torch

from dfd_clip_amd import augment as A
from dfd_clip_amd import capi
from dfd_clip_amd import elastic as E
from tests.cases import make_config
from tests.guarded import guarded_1d, guarded_bytes
from tests.test_hip_preprocess import smooth_u8

pytestmark = pytest.mark.gpu

FIELD_SIZES = [(1, 1), (7, 5), (17, 33), (24, 25), (97, 131), (150, 150), (224, 224)]
SIGMAS = (0.5, 6, 16)                                 # radii 2, 24, 64
FIELD_IDS = [0, 2 ** 63 - 1, 0x0123456789ABCDEF, 0]   # the first id again at another place
REMAP_SHAPES = [(1, 1, 1, 1), (2, 1, 7, 5), (3, 3, 17, 33), (2, 5, 97, 131), (2, 2, 150, 150), (1, 2, 224, 224)]
SEED = 0xFEDCBA9876543210


def same(got, want, what=""):
    if not torch.equal(torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(want))):
        bad = np.argwhere(got != want)
        first = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ; first at {first}: kernel {got[first]} restatement {want[first]}")


def run_field(ids, h, w, taps, alpha_q, seed=SEED):
    """-> the kernel's fields as an int16 ndarray [n, h, w, 2]; the workspace is exactly n*h*w*4 bytes between guards."""
    n = len(ids)
    ws = guarded_bytes(n * h * w * 4, name="field")
    field = ws.t.view(torch.int16).view(n, h, w, 2)
    capi.elastic_field(field, torch.tensor(ids, dtype=torch.int64).cuda(), seed, taps, alpha_q)
    torch.cuda.synchronize()
    ws.assert_untouched()
    return field.cpu().numpy()


def run_remap(clips, fields, foc, out_fill=0xA5, in_guard=255):
    """clips uint8 ndarray [B,T,3,h,w], fields int16 ndarray [n,h,w,2], foc int list -> the kernel's output; guards checked."""
    B, T, _, h, w = clips.shape
    inp = guarded_1d(clips.size, torch.uint8, fill=in_guard, name="in").set(torch.from_numpy(clips))
    out = guarded_1d(clips.size, torch.uint8, fill=out_fill, name="out")
    ws = guarded_bytes(fields.size * 2, name="field")
    if fields.size:
        ws.set(torch.from_numpy(np.ascontiguousarray(fields).view(np.uint8).reshape(-1)))
    field = ws.t.view(torch.int16).view(len(fields), h, w, 2) if fields.size else torch.empty(0, h, w, 2, dtype=torch.int16, device="cuda")
    capi.elastic_remap_u8(inp.shaped(*clips.shape), out.shaped(*clips.shape), field, torch.tensor(foc, dtype=torch.int32).cuda())
    torch.cuda.synchronize()
    out.assert_untouched()
    inp.assert_untouched(view_too=True)
    ws.assert_untouched(view_too=True)
    return out.shaped(*clips.shape).cpu().numpy()


def remap_want(clips, fields, foc):
    return np.stack([E.remap_reference(c, fields[i]) if 0 <= i < len(fields) else c for c, i in zip(clips, foc)])


# ---- the field kernel ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w", FIELD_SIZES)
def test_field_kernel_equals_the_restatement(h, w):
    for sigma in SIGMAS:
        taps = E.elastic_taps(sigma)
        alpha_q = 12800 if sigma != 16 else 12800 * 40  # the widest blur leaves little: scale it up so that the bits still count
        got = run_field(FIELD_IDS, h, w, taps, alpha_q)
        for k, fid in enumerate(FIELD_IDS):
            same(got[k], E.field_reference(SEED, fid, h, w, taps, alpha_q), f"{h}x{w} sigma {sigma} id {fid:#x} at place {k}")
        assert np.array_equal(got[0], got[3]) and not np.array_equal(got[0], got[1]) and got.any()


def test_field_kernel_seed_alpha_and_saturation():
    h, w = 24, 25
    taps = E.elastic_taps(6.0)
    a = run_field([7], h, w, taps, 12800, seed=1)
    same(a[0], E.field_reference(1, 7, h, w, taps, 12800), "seed 1")
    b = run_field([7], h, w, taps, 12800, seed=1 + (1 << 32))   # the high seed word enters
    same(b[0], E.field_reference(1 + (1 << 32), 7, h, w, taps, 12800), "high seed word")
    assert not np.array_equal(a, b)
    assert not run_field([7, 8], h, w, taps, 0).any()           # alpha 0: no displacement
    for alpha_q in (2 ** 31 - 1, -2 ** 31):                     # radius 0: the noise itself, saturated to int16
        got = run_field([7], h, w, [32768], alpha_q)
        same(got[0], E.field_reference(SEED, 7, h, w, [32768], alpha_q), f"alpha_q {alpha_q}")
        assert got.max() == 32767 and got.min() == -32768


# ---- the remap kernel ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hand_made_fields(h, w):
    """(names, int16 [n, h, w, 2])"""
    rng = np.random.default_rng(1000 * h + w)
    const = lambda dx, dy: np.broadcast_to(np.array([dx, dy], dtype=np.int16), (h, w, 2))
    y, x = np.mgrid[0:h, 0:w]
    spec = [("zero", const(0, 0)), ("shift +3,-2 px", const(96, -64)), ("shift -1/32, +31/32 px", const(-1, 31)),
            ("shift 2.5, -0.75 px", const(80, -24)), ("+32767", const(32767, 32767)), ("-32767", const(-32767, -32767)),
            ("+-32767", np.where(rng.random((h, w, 2)) < 0.5, -32767, 32767).astype(np.int16)),
            ("-32768", const(-32768, -32768)),
            ("every fraction", np.stack([(x % 32) + 64, (y % 32) - 32], axis=-1).astype(np.int16)),
            ("random", rng.integers(-32768, 32768, (h, w, 2)).astype(np.int16)),
            ("a few px", rng.integers(-300, 301, (h, w, 2)).astype(np.int16))]
    return [s[0] for s in spec], np.stack([s[1] for s in spec])


@pytest.mark.parametrize("B,T,h,w", REMAP_SHAPES)
def test_remap_kernel_equals_the_restatement(B, T, h, w):
    names, fields = hand_made_fields(h, w)
    rng = np.random.default_rng(h + w)
    base = np.concatenate([smooth_u8(B * T - B * T // 2, h, w, seed=50 + h).numpy(),
                           rng.integers(0, 256, (B * T // 2, 3, h, w), dtype=np.uint8)]).reshape(B, T, 3, h, w)
    clips = np.repeat(base, len(fields), axis=0)             # every clip under every field
    foc = np.tile(np.arange(len(fields)), B).tolist()
    got = run_remap(clips, fields, foc)
    want = remap_want(clips, fields, foc)
    for k, name in enumerate(names):
        same(got[k::len(fields)], want[k::len(fields)], f"field {name!r} at {B}x{T}x{h}x{w}")
    assert np.array_equal(want[0::len(fields)], base)        # the zero field is the identity
    if h * w > 1:
        changed = [name for k, name in enumerate(names) if not np.array_equal(want[k::len(fields)], base)]
        assert len(changed) >= len(names) - 2, changed       # the cases are not vacuous


def test_every_fraction_of_the_grid_on_one_image():
    h = w = 32
    y, x = np.mgrid[0:h, 0:w]
    field = np.stack([x - 32, y + 64], axis=-1).astype(np.int16)[None]   # pixel (y, x) has fx = x, fy = y
    clips = np.random.default_rng(3).integers(0, 256, (1, 1, 3, h, w), dtype=np.uint8)
    assert len({(int(a) & 31, int(b) & 31) for a, b in field.reshape(-1, 2)}) == 1024
    same(run_remap(clips, field, [0]), remap_want(clips, field, [0]), "32x32 fractions")


def test_clips_without_a_field_are_copied_and_fields_are_shared():
    B, T, h, w = 7, 5, 37, 51                                 # 1887 bytes a plane: odd addresses, a short last group
    clips = smooth_u8(B * T, h, w, seed=6).numpy().reshape(B, T, 3, h, w)
    clips[2:4] = clips[0:2]                                   # clips 2, 3 hold the frames of clips 0, 1
    rng = np.random.default_rng(8)
    fields = rng.integers(-400, 401, (2, h, w, 2)).astype(np.int16)
    foc = [0, -1, 0, 2, 1, 2 ** 31 - 1, -2 ** 31]
    want = remap_want(clips, fields, foc)
    for fill, guard in ((0xA5, 255), (0x5A, 0)):              # another pre-fill, another poison behind the input
        got = run_remap(clips, fields, foc, out_fill=fill, in_guard=guard)
        same(got, want, "mixed")
        for b in (1, 3, 5, 6):
            assert np.array_equal(got[b], clips[b]), b        # bit for bit
        assert np.array_equal(got[0], got[2]) and not np.array_equal(got[0], clips[0]) and not np.array_equal(got[4], clips[4])
    none = np.zeros((0, h, w, 2), np.int16)                   # no field at all: every index lies outside
    assert np.array_equal(run_remap(clips, none, [0, 1, -1, 5, 0, 0, 0]), clips)


def test_refusals_leave_the_output_alone():
    lib = capi.load_library()
    clips = smooth_u8(4, 16, 16, seed=1).view(2, 2, 3, 16, 16).cuda()
    out = torch.full_like(clips, 0xA5)
    field = torch.zeros(1, 16, 16, 2, dtype=torch.int16, device="cuda")
    foc = torch.zeros(2, dtype=torch.int32, device="cuda")
    keep = clips.clone()
    with pytest.raises(capi.DfdError, match="overlap"):
        capi.elastic_remap_u8(clips, clips, field, foc)
    rc = lib.dfd_elastic_remap_u8(clips.data_ptr(), out.data_ptr(), 2, 2, 16, 16, field.data_ptr() + 2, 1, foc.data_ptr(), None)
    assert rc == -1 and b"4-byte aligned" in lib.dfd_last_error()
    with pytest.raises(capi.DfdError, match="taps sum"):
        capi.elastic_field(field, torch.zeros(1, dtype=torch.int64, device="cuda"), 1, [1, 2, 3], 12800)
    torch.cuda.synchronize()
    assert torch.equal(clips, keep) and bool((out == 0xA5).all()) and not bool(field.any())
    with pytest.raises(capi.DfdError):
        capi.elastic_remap_u8(clips.cpu(), out, field, foc)


# ---- through SslFake and the train step ----------------------------------------------------------------------------------

@pytest.mark.parametrize("B,T,h,w", [(2, 3, 150, 150), (2, 2, 224, 224)])
def test_apply_equals_the_restatement_and_replays(B, T, h, w):
    clips = smooth_u8(B * T, h, w, seed=8).view(B, T, 3, h, w)
    ssl = E.SslFake(seed=3)
    drawn = ssl.draw(B)
    params = E.ElasticParams([True, False], drawn.field_ids, drawn.seed, drawn.taps, drawn.alpha_q)
    dev = clips.cuda()
    keep = dev.clone()
    got = ssl.apply(dev, params)
    assert got.data_ptr() != dev.data_ptr() and torch.equal(dev, keep)              # a new tensor; the input is untouched
    want = E.elastic_reference(clips.numpy(), params)
    same(got.cpu().numpy(), want, "apply")
    assert not np.array_equal(want[0], clips[0].numpy()) and np.array_equal(want[1], clips[1].numpy())
    assert torch.equal(ssl.apply(dev.clone(), params), got)                         # replay: same params, second tensor
    other = smooth_u8(B * T, h, w, seed=9).view(B, T, 3, h, w)                       # the paired clip: other frames, same warp
    same(ssl.apply(other.cuda(), params).cpu().numpy(), E.elastic_reference(other.numpy(), params), "replay")
    which = torch.tensor([0, 1], device="cuda")                                     # `which` overrides the coins
    same(ssl.apply(dev, params, which).cpu().numpy(), E.elastic_reference(clips.numpy(), params, [0, 1]), "which")
    nothing = E.ElasticParams([False, False], drawn.field_ids, drawn.seed, drawn.taps, drawn.alpha_q)
    assert torch.equal(ssl.apply(dev, nothing), dev)


def test_call_warps_the_real_clips_whose_coin_fired():
    B, T, h, w = 8, 2, 40, 52
    clips = smooth_u8(B * T, h, w, seed=10).view(B, T, 3, h, w)
    labels = torch.tensor([0, 1, 0, 0, 1, 1, 0, 0])
    params = E.SslFake(seed=5).draw(B)
    which = params.coins & (labels.numpy() == 0)
    assert which.any() and (params.coins & (labels.numpy() == 1)).any() and (~params.coins & (labels.numpy() == 0)).any()
    got, new = E.SslFake(seed=5)(clips.cuda(), labels.cuda())
    same(got.cpu().numpy(), E.elastic_reference(clips.numpy(), params, which), "__call__")
    assert torch.equal(new.cpu(), torch.where(torch.from_numpy(which), 1, labels)) and new.dtype == labels.dtype
    same_clips, same_labels = E.SslFake(p=0.0, seed=5)(clips.cuda(), labels.cuda())
    assert torch.equal(same_clips.cpu(), clips) and torch.equal(same_labels.cpu(), labels)


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


def test_train_step_with_ssl_fake():
    from dfd_clip_amd.harness import train_step
    base = _tiny_model()
    clips = smooth_u8(2 * 4, 40, 52, seed=13).view(2, 4, 3, 40, 52).cuda()
    m = torch.ones(2, 4, dtype=torch.bool, device="cuda")
    y = torch.tensor([0, 1], device="cuda")

    def step(frames, labels=y, **kw):
        model = copy.deepcopy(base)
        opt = _Recording(model.configure_optimizers(0.05), model)
        out = train_step(model, opt, [(frames, labels, m, None, None, 0)], **kw)
        torch.cuda.synchronize()
        return out, opt.grads, {k: v.detach().clone() for k, v in model.named_parameters()}

    def equal(a, b):
        (oa, ga, pa), (ob, gb, pb) = a, b
        return (torch.equal(oa["losses"][0], ob["losses"][0]) and torch.equal(oa["logits"][0], ob["logits"][0]) and
                ga.keys() == gb.keys() and all(torch.equal(ga[k], gb[k]) for k in ga) and all(torch.equal(pa[k], pb[k]) for k in pa))

    seed = 4
    by_hand = E.SslFake(p=1.0, seed=seed)
    params = by_hand.draw(2)
    which, flipped = by_hand.select(params, y)
    assert which.tolist() == [True, False] and flipped.tolist() == [1, 1]
    warped = by_hand.apply(clips, params, which)
    assert not torch.equal(warped[0], clips[0]) and torch.equal(warped[1], clips[1])
    inside = step(clips, ssl_fake=E.SslFake(p=1.0, seed=seed))
    outside = step(warped, labels=flipped)
    assert len(inside[1]) > 0 and equal(inside, outside)
    plain = step(clips)
    assert not torch.equal(plain[0]["losses"][0], inside[0]["losses"][0])
    assert equal(plain, step(clips, ssl_fake=None))
    # with an augment: the augmentation first, the fakes from its output
    spec, aug_seed = "frame+normal", 4
    aug = A.ClipAugment(spec, seed=aug_seed)
    augmented = aug.apply(clips, aug.draw(2, 4))
    assert not torch.equal(augmented, clips)
    both = step(clips, augment=A.ClipAugment(spec, seed=aug_seed), ssl_fake=E.SslFake(p=1.0, seed=seed))
    assert equal(both, step(by_hand.apply(augmented, params, which), labels=flipped)) and not equal(both, inside)
    with pytest.raises(TypeError, match="ssl_fake= needs uint8 device frames"):
        step(clips.float(), ssl_fake=E.SslFake(seed=seed))
    with pytest.raises(TypeError, match="ssl_fake= needs uint8 device frames"):
        step(clips.cpu(), ssl_fake=E.SslFake(seed=seed))
