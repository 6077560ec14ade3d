"""Self-supervised fakes on the device: the reference's `ssl_fake` elastic warp of uint8 clips.

The reference builds half of its contrastive pairs out of real clips (`src/datasets.py:401-418`, `:538-544`, `:667-669`,
`:692`): one `alb.ElasticTransform(alpha=50, sigma=6, alpha_affine=0, p=1)` draw is replayed over every frame of a real
clip, and the result is labelled fake.  Here the draw is made on the host by a seeded NumPy generator and applied by two
kernel launches (`csrc/elastic.hip`, `include/dfdclip_elastic.h`): one makes the displacement fields, one samples the clips.

  SslFake(alpha, sigma, p, real_label, fake_label, seed)
      .draw(n_clips) -> ElasticParams               plain host data: a coin and a 63-bit field id per clip, the seed, the
                                                    blur taps and alpha_q
      .apply(clips_u8, params, which=None)          -> new [B,T,3,H,W] uint8 device tensor; `which` (device bool / int [B])
                                                    overrides the coins; the same params on a second tensor is the
                                                    reference's `replay` (paired raw / c23 clips)
      (clips_u8, labels) -> (clips, labels)         a clip is warped iff its coin fired AND its label is `real_label`
                                                    (decided on the device, no sync); its label becomes `fake_label`
  elastic_taps, field_reference, remap_reference, elastic_reference
                                                    NumPy int64 restatements of the kernels' arithmetic; the GPU tests demand
                                                    equality with them bit for bit, the CPU tests hold them against scipy

What the transform is: per clip two displacement planes of the frame size -- uniform noise in [-1, 1), filtered with
scipy's `gaussian_filter` (radius int(4 sigma + 0.5), boundary `reflect`), times alpha -- and every frame and channel
sampled bilinearly at (x + dx, y + dy) with the border `reflect_101`; with alpha_affine = 0 the affine part is the identity.
The fixed point: 16-bit noise, Q15 taps summing to 32768, a rounded 16-bit result of the horizontal pass, the vertical pass
and alpha_q = round(256 alpha) in one 64-bit product rounded onto a 1/32-pixel grid; sampling on that grid with four
weights summing to 1024, as the face alignment does.  A field depends on (seed, field id, size, taps, alpha_q) only, never
on its position in a batch.  Parity with albumentations / OpenCV pixel values is not pinned (neither is a dependency); the
filter is pinned against scipy.
"""
import numpy as np

from . import capi

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_U32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): `counter` = four arrays of 32-bit words, `key` = two 32-bit integers -> four
    uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _U32 for c in counter)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> _S32) ^ c1 ^ np.uint64(k0)) & _U32, p1 & _U32, ((p0 >> _S32) ^ c3 ^ np.uint64(k1)) & _U32, p0 & _U32
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def elastic_taps(sigma):
    """scipy's Gaussian kernel of `gaussian_filter(sigma)` (radius int(4 sigma + 0.5)) in Q15: int64 [2 radius + 1], symmetric,
    summing to exactly 32768 (the centre tap takes what rounding leaves over)."""
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError(f"sigma must be positive, got {sigma}")
    radius = int(4.0 * sigma + 0.5)
    if radius > capi.ELASTIC_MAX_RADIUS:
        raise ValueError(f"sigma {sigma} needs a radius of {radius}; the kernel takes at most {capi.ELASTIC_MAX_RADIUS}")
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    phi = np.exp(-0.5 / (sigma * sigma) * x * x)
    q = np.rint(phi / phi.sum() * capi.ELASTIC_TAP_ONE).astype(np.int64)
    q[radius] += capi.ELASTIC_TAP_ONE - q.sum()
    return q


def field_noise(seed, field_id, h, w):
    """The 16-bit noise of one field, centred: int64 [2, h, w] in [-32768, 32767]."""
    seed, fid = int(seed) & 0xFFFFFFFFFFFFFFFF, int(field_id) & 0xFFFFFFFFFFFFFFFF
    n = 2 * h * w
    g = np.arange((n + 7) // 8, dtype=np.uint64)
    words = philox4x32_10((g & _U32, g >> _S32, np.full(len(g), fid & 0xFFFFFFFF, np.uint64), np.full(len(g), fid >> 32, np.uint64)),
                          ((seed & 0xFFFFFFFF) ^ capi.ELASTIC_SITE, seed >> 32))
    draws = np.empty((len(g), 8), dtype=np.int64)
    for j in range(4):
        draws[:, 2 * j] = (words[j] & np.uint64(0xFFFF)).astype(np.int64)
        draws[:, 2 * j + 1] = (words[j] >> np.uint64(16)).astype(np.int64)
    return (draws.reshape(-1)[:n] - 32768).reshape(2, h, w)


def _reflect(i, n):
    """d c b a | a b c d | d c b a, any distance."""
    m = np.mod(np.asarray(i, dtype=np.int64), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _reflect_101(i, n):
    """d c b | a b c d | c b a, any distance; a dimension of 1 maps to 0."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    m = np.mod(i, 2 * n - 2)
    return np.where(m < n, m, 2 * n - 2 - m)


def blur_reference(noise, taps, alpha_q):
    """`dfd_elastic_field` after the draw: int64 noise [..., h, w] -> d5 int64 [..., h, w] (saturated to int16's range)."""
    noise = np.asarray(noise, dtype=np.int64)
    taps = np.asarray(taps, dtype=np.int64)
    radius = len(taps) // 2
    h, w = noise.shape[-2:]
    cols = noise[..., _reflect(np.arange(-radius, w + radius), w)]
    hor = (sum(int(q) * cols[..., k:k + w] for k, q in enumerate(taps)) + (1 << 14)) >> 15
    rows = hor[..., _reflect(np.arange(-radius, h + radius), h), :]
    ver = sum(int(q) * rows[..., k:k + h, :] for k, q in enumerate(taps))
    return np.clip((ver * int(alpha_q) + (1 << 32)) >> 33, -32768, 32767)


def field_reference(seed, field_id, h, w, taps, alpha_q):
    """`dfd_elastic_field` in NumPy: int16 [h, w, 2] = (dx5, dy5) in 1/32-pixel units."""
    return np.ascontiguousarray(blur_reference(field_noise(seed, field_id, h, w), taps, alpha_q).transpose(1, 2, 0)).astype(np.int16)


def remap_reference(frames_u8, d5):
    """`dfd_elastic_remap_u8` for planes that share one field: frames uint8 [..., h, w], d5 integer [h, w, 2] -> uint8."""
    frames = np.asarray(frames_u8)
    d5 = np.asarray(d5).astype(np.int64)
    h, w = frames.shape[-2:]
    assert frames.dtype == np.uint8 and d5.shape == (h, w, 2)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    x5, y5 = 32 * x + d5[..., 0], 32 * y + d5[..., 1]
    fx, fy = x5 & 31, y5 & 31
    xa, xb = _reflect_101(x5 >> 5, w), _reflect_101((x5 >> 5) + 1, w)
    ya, yb = _reflect_101(y5 >> 5, h), _reflect_101((y5 >> 5) + 1, h)
    p = frames.astype(np.int64)
    acc = ((32 - fx) * (32 - fy) * p[..., ya, xa] + fx * (32 - fy) * p[..., ya, xb] + (32 - fx) * fy * p[..., yb, xa] +
           fx * fy * p[..., yb, xb] + 512)
    return (acc >> 10).astype(np.uint8)


class ElasticParams:
    """What `SslFake.draw` returns: `coins` bool [n_clips], `field_ids` int64 [n_clips] in [0, 2^63), the 64-bit `seed`, the
    Q15 `taps` and `alpha_q`.  Host data only; device copies are made on first use and kept."""

    def __init__(self, coins, field_ids, seed, taps, alpha_q):
        self.coins = np.ascontiguousarray(coins, dtype=bool)
        self.field_ids = np.ascontiguousarray(field_ids, dtype=np.int64)
        if self.coins.ndim != 1 or self.coins.shape != self.field_ids.shape:
            raise ValueError(f"{self.coins.shape} coins for {self.field_ids.shape} field ids")
        self.n_clips = len(self.coins)
        self.seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self.taps = np.ascontiguousarray(taps, dtype=np.int64)
        self.alpha_q = int(alpha_q)
        self._device = {}

    def same_as(self, other):
        return (np.array_equal(self.coins, other.coins) and np.array_equal(self.field_ids, other.field_ids) and self.seed == other.seed and
                np.array_equal(self.taps, other.taps) and self.alpha_q == other.alpha_q)

    def on(self, device):
        """(coins bool [n], field_ids i64 [n]) on `device`."""
        import torch
        key = str(device)
        if key not in self._device:
            self._device[key] = (torch.from_numpy(self.coins.copy()).to(device), torch.from_numpy(self.field_ids.copy()).to(device))
        return self._device[key]


def _check_clips(clips_u8, params):
    import torch
    if not (torch.is_tensor(clips_u8) and clips_u8.is_cuda and clips_u8.dtype == torch.uint8):
        raise TypeError("SslFake works on uint8 device clips (warp before the conversion to float, on the GPU)")
    if clips_u8.dim() != 5 or clips_u8.shape[2] != 3:
        raise ValueError(f"clips must be [B,T,3,H,W], got {tuple(clips_u8.shape)}")
    if clips_u8.shape[0] != params.n_clips:
        raise ValueError(f"params were drawn for {params.n_clips} clips, there are {clips_u8.shape[0]}")


def _warp(clips_u8, params, candidates, field_of_clip):
    """Fields for the clips `candidates` (host indices, ascending), then one remap: clip b takes field `field_of_clip[b]`
    (device i32 [B], an index into `candidates`) or is copied."""
    import torch
    x = clips_u8.contiguous()
    H, W = x.shape[3:]
    field = torch.empty(len(candidates), H, W, 2, dtype=torch.int16, device=x.device)
    if len(candidates):
        ids = params.on(x.device)[1]
        ids = ids if len(candidates) == params.n_clips else ids[torch.from_numpy(np.asarray(candidates, dtype=np.int64)).to(x.device)]
        capi.elastic_field(field, ids.contiguous(), params.seed, params.taps, params.alpha_q)
    return capi.elastic_remap_u8(x, torch.empty_like(x), field, field_of_clip.to(torch.int32).contiguous())


def _slots(coins):
    """Host: (indices of the fired coins, i32 [n] = each clip's position among them or -1)."""
    fired = np.flatnonzero(coins)
    slot = np.full(len(coins), -1, dtype=np.int32)
    slot[fired] = np.arange(len(fired), dtype=np.int32)
    return fired, slot


class SslFake:
    def __init__(self, alpha=50.0, sigma=6.0, p=0.5, real_label=0, fake_label=1, seed=None):
        self.alpha, self.sigma, self.p = float(alpha), float(sigma), float(p)
        self.real_label, self.fake_label = int(real_label), int(fake_label)
        self.taps = elastic_taps(self.sigma)
        self.alpha_q = int(round(256.0 * self.alpha))
        if not -2 ** 31 <= self.alpha_q < 2 ** 31:
            raise ValueError(f"alpha {alpha} is out of range")
        self.rng = np.random.default_rng(seed)
        self.seed = int(self.rng.integers(0, 2 ** 64, dtype=np.uint64))

    def draw(self, n_clips):
        """One coin and one field id per clip."""
        coins = self.rng.random(n_clips) < self.p
        return ElasticParams(coins, self.rng.integers(0, 2 ** 63, n_clips, dtype=np.int64), self.seed, self.taps, self.alpha_q)

    @staticmethod
    def apply(clips_u8, params, which=None):
        """[B,T,3,H,W] uint8 device clips -> a new tensor: the clips whose coin fired (or, with `which`, the clips it marks)
        warped by their field, the others copied."""
        import torch
        _check_clips(clips_u8, params)
        dev = clips_u8.device
        if which is None:
            fired, slot = _slots(params.coins)
            return _warp(clips_u8, params, fired, torch.from_numpy(slot).to(dev))
        which = torch.as_tensor(which, device=dev).reshape(-1)
        if which.numel() != params.n_clips:
            raise ValueError(f"`which` has {which.numel()} entries for {params.n_clips} clips")
        every = torch.arange(params.n_clips, dtype=torch.int32, device=dev)
        return _warp(clips_u8, params, np.arange(params.n_clips), torch.where(which != 0, every, torch.full_like(every, -1)))

    def select(self, params, labels):
        """(which bool [B], new labels) on the labels' device, without a sync: a clip is chosen iff its coin fired and its
        label is `real_label`; its label becomes `fake_label`."""
        import torch
        if labels.dim() != 1 or labels.shape[0] != params.n_clips:
            raise ValueError(f"labels must be [{params.n_clips}], got {tuple(labels.shape)}")
        coins = params.on(labels.device)[0] if labels.is_cuda else torch.from_numpy(params.coins.copy())
        which = coins & (labels == self.real_label)
        return which, torch.where(which, torch.full_like(labels, self.fake_label), labels)

    def __call__(self, clips_u8, labels):
        """Draw, then warp the real clips whose coin fired and relabel them: -> (new clips, new labels)."""
        import torch
        params = self.draw(clips_u8.shape[0] if torch.is_tensor(clips_u8) and clips_u8.dim() else 0)
        _check_clips(clips_u8, params)
        if not (torch.is_tensor(labels) and labels.device == clips_u8.device):
            raise TypeError("SslFake needs the labels on the clips' device (the choice is made there, without a sync)")
        which, new_labels = self.select(params, labels)
        fired, slot = _slots(params.coins)  # fields are made for every fired coin; the labels decide on the device
        slot = torch.from_numpy(slot).to(clips_u8.device)
        return _warp(clips_u8, params, fired, torch.where(which, slot, torch.full_like(slot, -1))), new_labels


def elastic_reference(clips_u8, params, which=None):
    """What `SslFake.apply` computes, in NumPy int64: clips [B, T, 3, h, w] uint8."""
    clips = np.asarray(clips_u8)
    assert clips.dtype == np.uint8 and clips.ndim == 5 and len(clips) == params.n_clips
    which = params.coins if which is None else np.asarray(which).reshape(-1) != 0
    out = clips.copy()
    h, w = clips.shape[-2:]
    for b in np.flatnonzero(which):
        out[b] = remap_reference(clips[b], field_reference(params.seed, params.field_ids[b], h, w, params.taps, params.alpha_q))
    return out
