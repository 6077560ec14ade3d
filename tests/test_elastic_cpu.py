"""CPU side of the device elastic warp (`ssl_fake`): the elastic header against its ctypes table and the built library, the
refusals, and the integer restatement of `dfd-clip_amd/elastic.py` against scipy (the Gaussian filter with boundary
`reflect`, bilinear sampling with boundary `mirror`), plus `SslFake`'s draws and selection."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi, harness
from dfd_clip_amd import elastic as E
from tests.test_hip_preprocess import smooth_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dfdclip_elastic.h")
NAMES = ["dfd_elastic_field", "dfd_elastic_remap_u8"]


def _header_text():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def _lib():
    from dfd_clip_amd.build import build
    build()
    return capi.load_library()


# ---- ABI ------------------------------------------------------------------------------------------------------------

def test_elastic_header_ctypes_table_and_exports_agree():
    lib = _lib()
    fns = sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", _header_text())))
    assert fns == sorted(capi.ELASTIC_SIGNATURES) == NAMES
    others = (set(capi.SIGNATURES) | set(capi.EXT_SIGNATURES) | set(capi.EXPLAIN_SIGNATURES) | set(capi.AUGMENT_SIGNATURES) |
              set(capi.ALIGN_SIGNATURES) | set(capi.HOOK_SIGNATURES))
    assert not set(fns) & others
    for name in fns:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == capi.ELASTIC_SIGNATURES[name][1]
        params = re.search(name + r"\s*\((.*?)\)\s*;", _header_text(), flags=re.S).group(1)
        assert len(params.split(",")) == len(capi.ELASTIC_SIGNATURES[name][1])
    assert lib.dfd_abi_version() == capi.ABI_VERSION == 17
    defines = dict(re.findall(r"#define\s+DFD_ELASTIC_([A-Z_]+)\s+(0x[0-9A-Fa-f]+|\d+)u?", open(HEADER).read()))
    assert int(defines["MAX_RADIUS"], 0) == capi.ELASTIC_MAX_RADIUS == 128
    assert int(defines["TAP_ONE"], 0) == capi.ELASTIC_TAP_ONE == 32768
    assert int(defines["SITE"], 0) == capi.ELASTIC_SITE
    main_header = open(os.path.join(ROOT, "include", "dfdclip.h")).read()
    assert "elastic" not in main_header


def _taps(values):
    return (ctypes.c_int32 * len(values))(*[int(v) for v in values])


def test_field_refusals_return_an_error_without_launching():
    lib = _lib()
    f, ids = 1 << 20, 1 << 21  # never dereferenced: every call returns at its checks
    good = _taps(E.elastic_taps(6.0))

    def refused(what, *args):
        assert lib.dfd_elastic_field(*args, None) == -1, what
        assert what.encode() in lib.dfd_last_error(), (what, lib.dfd_last_error())

    refused("null pointer", None, 1, 16, 16, ids, 1, good, 24, 12800)
    refused("null pointer", f, 1, 16, 16, None, 1, good, 24, 12800)
    refused("null pointer", f, 1, 16, 16, ids, 1, None, 24, 12800)
    refused("bad field count", f, -1, 16, 16, ids, 1, good, 24, 12800)
    refused("bad size", f, 1, 65536, 32768, ids, 1, good, 24, 12800)           # h * w = 2^31
    refused("bad size", f, 1, 0, 16, ids, 1, good, 24, 12800)
    refused("bad size", f, 1, 16, -3, ids, 1, good, 24, 12800)
    refused("bad radius", f, 1, 16, 16, ids, 1, good, 129, 12800)
    refused("bad radius", f, 1, 16, 16, ids, 1, good, -1, 12800)
    short = np.array(E.elastic_taps(6.0))
    short[3] += 1
    refused("taps sum to 32769", f, 1, 16, 16, ids, 1, _taps(short), 24, 12800)
    refused("taps sum to", f, 1, 16, 16, ids, 1, good, 23, 12800)              # two taps short
    refused("is negative", f, 1, 16, 16, ids, 1, _taps([-1, 32770, -1]), 1, 12800)
    refused("4-byte aligned", f + 2, 1, 16, 16, ids, 1, good, 24, 12800)
    refused("8-byte aligned", f, 1, 16, 16, ids + 4, 1, good, 24, 12800)
    assert lib.dfd_elastic_field(None, 0, 16, 16, None, 1, good, 24, 12800, None) == 0  # nothing to do
    assert lib.dfd_elastic_field(f, 0, 16, 16, ids, 1, _taps([32768]), 0, 0, None) == 0


def test_remap_refusals_return_an_error_without_launching():
    lib = _lib()
    a, b, f, foc = 1 << 20, 1 << 24, 1 << 28, 1 << 29

    def refused(what, *args):
        assert lib.dfd_elastic_remap_u8(*args, None) == -1, what
        assert what.encode() in lib.dfd_last_error(), (what, lib.dfd_last_error())

    refused("null pointer", None, b, 2, 3, 16, 16, f, 1, foc)
    refused("null pointer", a, None, 2, 3, 16, 16, f, 1, foc)
    refused("null pointer", a, b, 2, 3, 16, 16, f, 1, None)
    refused("null field pointer", a, b, 2, 3, 16, 16, None, 1, foc)
    refused("bad clip or frame count", a, b, -1, 3, 16, 16, f, 1, foc)
    refused("bad clip or frame count", a, b, 2, -3, 16, 16, f, 1, foc)
    refused("bad field count", a, b, 2, 3, 16, 16, f, -1, foc)
    refused("bad size", a, b, 2, 3, 32768, 65536, f, 1, foc)                   # h * w = 2^31
    refused("bad size", a, b, 2, 3, 16, 0, f, 1, foc)
    refused("overlap", a, a, 2, 3, 16, 16, f, 1, foc)
    refused("overlap", a, a + 2 * 3 * 3 * 256 - 1, 2, 3, 16, 16, f, 1, foc)    # the last byte of in is the first of out
    refused("overlap", a + 100, a, 2, 3, 16, 16, f, 1, foc)
    refused("4-byte aligned", a, b, 2, 3, 16, 16, f + 2, 1, foc)
    refused("out of range", a, b, 2 ** 31 - 1, 2 ** 31 - 1, 16384, 16384, f, 1, foc)
    assert lib.dfd_elastic_remap_u8(None, None, 0, 3, 16, 16, None, 0, None, None) == 0  # nothing to do
    assert lib.dfd_elastic_remap_u8(None, None, 2, 0, 16, 16, None, 0, None, None) == 0


# ---- the restatement's parts -------------------------------------------------------------------------------------------

def test_philox_equals_the_oracle():
    from oracle.dropout_mask import philox4x32_10
    rng = np.random.default_rng(0)
    for _ in range(4):
        c = [rng.integers(0, 2 ** 32, 1000, dtype=np.uint64) for _ in range(4)]
        k = [int(v) for v in rng.integers(0, 2 ** 32, 2, dtype=np.uint64)]
        got, want = E.philox4x32_10(c, k), philox4x32_10(*c, *k)
        assert all(np.array_equal(g, w) for g, w in zip(got, want))
    edge = [np.array([0, 2 ** 32 - 1], dtype=np.uint64)] * 4
    assert all(np.array_equal(g, w) for g, w in zip(E.philox4x32_10(edge, (2 ** 32 - 1, 0)), philox4x32_10(*edge, 2 ** 32 - 1, 0)))


@pytest.mark.parametrize("sigma", [0.5, 6, 16])
def test_taps(sigma):
    q = E.elastic_taps(sigma)
    assert len(q) == 2 * int(4 * sigma + 0.5) + 1 and q.sum() == 32768 == capi.ELASTIC_TAP_ONE
    assert np.array_equal(q, q[::-1]) and (q >= 0).all() and q[len(q) // 2] >= q.max() - len(q) // 2
    with pytest.raises(ValueError):
        E.elastic_taps(40)  # radius 160
    with pytest.raises(ValueError):
        E.elastic_taps(0)


def test_noise_layout():
    """Element e = (c h + y) w + x takes draw e & 7 of block e >> 3: a smaller field is a prefix of its component planes'
    flat order only where the sizes agree, and ids, seeds and the site constant all enter."""
    n = E.field_noise(3, 9, 6, 7)
    assert n.shape == (2, 6, 7) and n.min() >= -32768 and n.max() <= 32767
    flat = E.field_noise(3, 9, 1, 42)  # the same 84 elements in another shape
    assert np.array_equal(n.reshape(-1), flat.reshape(-1))
    assert not np.array_equal(n, E.field_noise(4, 9, 6, 7)) and not np.array_equal(n, E.field_noise(3, 10, 6, 7))
    assert not np.array_equal(n, E.field_noise(3 + (1 << 32), 9, 6, 7)) and not np.array_equal(n, E.field_noise(3, 9 + (1 << 32), 6, 7))
    big = E.field_noise(1, 2, 224, 224)
    assert abs(big.mean()) < 300 and abs(big.std() - 65536 / 12 ** 0.5) < 200  # uniform over 16 bits


# ---- the field against scipy ---------------------------------------------------------------------------------------------

def field_bound(sigma, alpha, taps, alpha_q):
    """Largest possible |restatement - exact| in 1/32-pixel steps, from the fixed point alone (|noise| <= 1):
      0.5                              the final rounding onto the 1/32 grid
      32 alpha * 0.5 / 32768           the horizontal result is rounded to 16 bits (then weighted by taps summing to 1)
      32 alpha * sum |q q' - g g'|     Q15 taps q against scipy's float64 kernel g, over the separable 2-D kernel
      32 |alpha_q / 256 - alpha|       alpha in 1/256
    plus float64 slack."""
    r = len(taps) // 2
    x = np.arange(-r, r + 1, dtype=np.float64)
    g = np.exp(-0.5 / (sigma * sigma) * x * x)
    g /= g.sum()
    q = np.asarray(taps, dtype=np.float64) / 32768
    return 0.5 + 32 * alpha * (0.5 / 32768 + np.abs(np.outer(q, q) - np.outer(g, g)).sum()) + 32 * abs(alpha_q / 256 - alpha) + 1e-6


@pytest.mark.parametrize("h,w", [(224, 224), (150, 150), (20, 33), (7, 5), (1, 1)])
def test_field_matches_scipy_gaussian_filter(h, w):
    ndimage = pytest.importorskip("scipy.ndimage")
    alpha, sigma = 50.0, 6.0
    ssl = E.SslFake(alpha, sigma, seed=0)
    bound = field_bound(sigma, alpha, ssl.taps, ssl.alpha_q)
    assert bound < 2.0  # of a 1/32-pixel step: a sixteenth of a pixel
    worst, biggest = 0.0, 0.0
    for fid in (0, 1, 2 ** 63 - 1, 123456789):
        noise = E.field_noise(ssl.seed, fid, h, w)
        got = E.field_reference(ssl.seed, fid, h, w, ssl.taps, ssl.alpha_q).astype(np.float64)
        for c in range(2):
            want = ndimage.gaussian_filter(noise[c] / 32768.0, sigma, mode="reflect") * alpha * 32
            worst = max(worst, np.abs(got[..., c] - want).max())
            biggest = max(biggest, np.abs(want).max())
    print(f"{h}x{w}: max |restatement - scipy| {worst:.3f} of a 1/32-px step (derived bound {bound:.3f}); largest displacement {biggest / 32:.2f} px")
    assert worst <= bound, (h, w, worst, bound)


def test_field_depends_on_its_id_not_on_its_place_and_alpha_zero_is_zero():
    ssl = E.SslFake(seed=1)
    a = E.field_reference(ssl.seed, 5, 20, 33, ssl.taps, ssl.alpha_q)
    assert a.dtype == np.int16 and a.shape == (20, 33, 2) and a.any()
    assert not np.array_equal(a, E.field_reference(ssl.seed, 6, 20, 33, ssl.taps, ssl.alpha_q))
    assert not np.array_equal(a, E.field_reference(ssl.seed + 1, 5, 20, 33, ssl.taps, ssl.alpha_q))
    assert not E.field_reference(ssl.seed, 5, 20, 33, ssl.taps, 0).any()
    # the same id at two places of a batch, on the same frames: the same warp
    clips = np.repeat(smooth_u8(2, 20, 33, seed=3).numpy()[None], 3, axis=0)          # [3, 2, 3, 20, 33], three equal clips
    params = E.ElasticParams([True, True, True], [5, 6, 5], ssl.seed, ssl.taps, ssl.alpha_q)
    out = E.elastic_reference(clips, params)
    assert np.array_equal(out[0], out[2]) and not np.array_equal(out[0], out[1]) and not np.array_equal(out[0], clips[0])
    swapped = E.elastic_reference(clips, E.ElasticParams([True, True, True], [6, 5, 5], ssl.seed, ssl.taps, ssl.alpha_q))
    assert np.array_equal(swapped[1], out[0]) and np.array_equal(swapped[0], out[1])
    # saturation instead of wrap-around
    assert np.abs(E.blur_reference(np.full((1, 4, 4), 32767), [32768], 2 ** 31 - 1)).max() == 32767
    assert E.blur_reference(np.full((1, 4, 4), -32768), [32768], 2 ** 31 - 1).min() == -32768


# ---- the remap against scipy ---------------------------------------------------------------------------------------------

def _noise_u8(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _fields(h, w):
    rng = np.random.default_rng(h * 1000 + w)
    ssl = E.SslFake(seed=2)
    return {"drawn": E.field_reference(ssl.seed, 1, h, w, ssl.taps, ssl.alpha_q),
            "random": rng.integers(-32768, 32768, (h, w, 2)).astype(np.int16),                # up to 1024 px: many image widths
            "far": np.where(rng.random((h, w, 2)) < 0.5, -32767, 32767).astype(np.int16),
            "few px": rng.integers(-200, 201, (h, w, 2)).astype(np.int16)}


@pytest.mark.parametrize("h,w", [(33, 47), (7, 5), (1, 9), (6, 1), (1, 1), (150, 150)])
def test_remap_matches_scipy_map_coordinates(h, w):
    ndimage = pytest.importorskip("scipy.ndimage")
    images = np.concatenate([_noise_u8(2, h, w, seed=h + w), smooth_u8(1, h, w, seed=7)[0].numpy()])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    for name, d5 in _fields(h, w).items():
        got = E.remap_reference(images, d5)
        coords = [y + d5[..., 1] / 32.0, x + d5[..., 0] / 32.0]      # exact: the positions lie on the 1/32 grid
        worst = 0.0
        for img, g in zip(images, got):
            exact = ndimage.map_coordinates(img.astype(np.float64), coords, order=1, mode="mirror")
            worst = max(worst, np.abs(g.astype(np.float64) - exact).max())
        print(f"{h}x{w} {name}: max |restatement - exact| {worst:.6f}")
        assert worst <= 0.5 + 1e-6, (h, w, name, worst)


def test_remap_identity_shifts_and_constant_images():
    h, w = 9, 11
    img = _noise_u8(3, h, w, seed=5)
    assert np.array_equal(E.remap_reference(img, np.zeros((h, w, 2), np.int16)), img)
    for kx, ky in ((3, -2), (-1, 0), (13, -25), (-40, 31), (1000, -1000)):  # the later ones lie beyond the image
        pad = max(abs(kx), abs(ky))
        padded = np.pad(img, ((0, 0), (pad, pad), (pad, pad)), mode="reflect")
        want = padded[:, pad + ky:pad + ky + h, pad + kx:pad + kx + w]
        d5 = np.broadcast_to(np.array([32 * kx, 32 * ky]), (h, w, 2))
        assert np.array_equal(E.remap_reference(img, d5), want), (kx, ky)
    half = E.remap_reference(img, np.broadcast_to(np.array([16, 0]), (h, w, 2)))   # half a pixel to the right: the mean, rounded up
    right = np.pad(img, ((0, 0), (0, 0), (0, 1)), mode="reflect")[:, :, 1:]
    assert np.array_equal(half, (img.astype(int) + right + 1) >> 1)
    rng = np.random.default_rng(1)
    for v in (0, 1, 127, 255):
        flat = np.full((2, h, w), v, np.uint8)
        assert np.array_equal(E.remap_reference(flat, rng.integers(-32768, 32768, (h, w, 2))), flat)


# ---- SslFake ---------------------------------------------------------------------------------------------------------------

def test_same_seed_same_params():
    a, b, c = (E.SslFake(seed=s).draw(40) for s in (5, 5, 6))
    assert a.same_as(b) and not a.same_as(c)
    assert a.coins.dtype == bool and a.field_ids.dtype == np.int64 and a.field_ids.min() >= 0 and len(set(a.field_ids.tolist())) == 40
    assert 0 <= a.seed < 2 ** 64 and a.alpha_q == 12800 and np.array_equal(a.taps, E.elastic_taps(6.0))
    ssl = E.SslFake(seed=5)
    first, second = ssl.draw(40), ssl.draw(40)
    assert first.same_as(a) and not second.same_as(first) and second.seed == first.seed
    n = 4000
    for p in (0.5, 0.2):
        fired = int(E.SslFake(p=p, seed=9).draw(n).coins.sum())
        assert abs(fired - n * p) <= 4 * (n * p * (1 - p)) ** 0.5
    with pytest.raises(ValueError):
        E.ElasticParams([True], [1, 2], 0, [32768], 0)


def _host_call(ssl, clips, labels):
    """What `SslFake.__call__` computes, through its host pieces: draw, `select` on host labels, the restatement."""
    params = ssl.draw(len(clips))
    which, new_labels = ssl.select(params, torch.from_numpy(labels))
    return params, which.numpy(), E.elastic_reference(clips, params, which.numpy()), new_labels.numpy()


def test_only_real_clips_whose_coin_fired_change():
    B = 12
    clips = smooth_u8(B * 2, 20, 24, seed=4).numpy().reshape(B, 2, 3, 20, 24)
    labels = np.array([0, 1, 0, 0, 1, 1, 0, 0, 1, 0, 2, 0], dtype=np.int64)
    params, which, out, new = _host_call(E.SslFake(seed=3), clips, labels)
    assert which.dtype == bool and np.array_equal(which, params.coins & (labels == 0))
    assert which.any() and (params.coins & (labels != 0)).any() and (~params.coins & (labels == 0)).any()  # every kind is present
    for b in range(B):
        assert np.array_equal(out[b], clips[b]) != which[b], b
    assert np.array_equal(new, np.where(which, 1, labels))
    # other labels for real and fake
    params, which, out, new = _host_call(E.SslFake(real_label=2, fake_label=7, p=1.0, seed=3), clips, labels)
    assert which.tolist() == (labels == 2).tolist() and new[10] == 7 and np.array_equal(np.delete(new, 10), np.delete(labels, 10))
    assert not np.array_equal(out[10], clips[10]) and np.array_equal(np.delete(out, 10, 0), np.delete(clips, 10, 0))
    # p = 0: nothing; p = 1: every real clip
    params, which, out, new = _host_call(E.SslFake(p=0.0, seed=3), clips, labels)
    assert not which.any() and np.array_equal(out, clips) and np.array_equal(new, labels)
    params, which, out, new = _host_call(E.SslFake(p=1.0, seed=3), clips, labels)
    assert np.array_equal(which, labels == 0) and all(not np.array_equal(out[b], clips[b]) for b in np.flatnonzero(labels == 0))
    assert np.array_equal(new, np.where(labels == 0, 1, labels))
    # `which` overrides the coins in the restatement, as in `apply`
    forced = E.elastic_reference(clips, params, np.arange(B) == 1)
    assert not np.array_equal(forced[1], clips[1]) and np.array_equal(np.delete(forced, 1, 0), np.delete(clips, 1, 0))


def test_host_or_float_frames_raise():
    ssl = E.SslFake(seed=0)
    y = torch.zeros(1, dtype=torch.int64)
    for frames in (torch.zeros(1, 2, 3, 8, 8), torch.zeros(1, 2, 3, 8, 8, dtype=torch.uint8)):
        with pytest.raises(TypeError, match="ssl_fake= needs uint8 device frames"):
            harness.train_step(torch.nn.Linear(1, 1), None, [(frames, y, None, None, None, 0)], total_tasks=1, ssl_fake=ssl)
        with pytest.raises(TypeError, match="uint8 device"):
            ssl(frames, y)
        with pytest.raises(TypeError, match="uint8 device"):
            ssl.apply(frames, ssl.draw(1))
