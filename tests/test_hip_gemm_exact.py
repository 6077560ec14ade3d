"""Bit-exact integer tests of the A^T.B and MFMA GEMM paths.

Small integers are exact in bf16 and f32, their products are exact in f32, and every partial sum is exact in any order
while it stays below 2^24.  A^T.B and A.W^T + bias (+ residual, + pos) then have exactly one correct f32 value, and a
bf16 store exactly one correct value too: round-to-nearest-even of that f32, rounded ONCE.  So nothing here has a
tolerance: every element is compared with `torch.equal` against an int64 matmul on the CPU, and any layout, pairing,
tail, split or rounding-count mistake fails.

Operands: one in [-3, 3], the other in [-2, 2] with +1 on every 7th contraction index (asymmetric in k); bias, residual
and pos are integers in [-40, 40].  `int(|ref|.max()) < 2^24` is asserted on the host before every GPU call.

Which kernel ran is asserted for every case (capi.gemm_at_b_last_path(), capi.gemm_last_path()): a case that lands on
another path than the one it names fails.
"""
import functools

import pytest
import torch

from tests.guarded import guarded, guarded_bytes

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
EXACT = 2 ** 24


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert c.load_library().dfd_device_check() == 0, c.load_library().dfd_last_error()
    return c


def assert_exact(got, want, what):
    """Every element equal (a NaN equals nothing); the message counts the wrong elements and names the first."""
    want = want.to(device=got.device, dtype=got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(got, want):
        return
    bad = ~(got == want)
    r, c = bad.nonzero()[0].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements wrong, first at (row {r}, column {c}): "
                         f"got {got[r, c].item()}, want {want[r, c].item()}")


def as_f32(ref_i64):
    """The int64 reference as f32, after the host-side check that it is exactly representable.  (Partial sums: |product|
    <= 9, or 9 * 32 with the column scales, and depth <= 4096 keep them below 2^24 in any order.)"""
    assert int(ref_i64.abs().max()) < EXACT, "the reference leaves the exact-integer range of f32: shrink the shape"
    return ref_i64.to(F32)


# ---- dfd_gemm_at_b ------------------------------------------------------------------------------------------------

def tn_plan(R, Ma, Nb):
    """(tile, steps, splits, steps_per_split) of the gemm_tn kernels: dfd_gemm_tn_splits / dfd_gemm_tn_launch in
    dfd-clip_amd/csrc/gemm_tn.hip, restated.  64 contraction rows per step; at least 4 steps per split."""
    tile = 256 if Ma % 256 == 0 and Nb % 256 == 0 else 128
    tiles = (Ma // tile) * (Nb // tile)
    steps = (R + 63) // 64
    splits = ((512 if tile == 128 else 256) + tiles - 1) // tiles
    if splits > steps // 4:
        splits = max(steps // 4, 1)
    splits = min(splits, 256)
    return tile, steps, splits, (steps + splits - 1) // splits


@functools.lru_cache(maxsize=None)
def at_b_operands(R, Ma, Nb):
    """(A [R, Ma] int64 in [-3, 3], B [R, Nb] int64 in [-2, 2] (+1 on every 7th contraction row), A^T.B int64)."""
    g = torch.Generator().manual_seed(R * 7919 + Ma * 31 + Nb)
    a = torch.randint(-3, 4, (R, Ma), generator=g)
    b = torch.randint(-2, 3, (R, Nb), generator=g)
    b[::7] += 1
    return a, b, a.T @ b


def col_scales(Ma, Nb):
    """Exact power-of-two column scales: every output column (and row) gets a magnitude of its own."""
    sa = 2.0 ** ((torch.arange(Ma) % 7) - 3).double()
    sb = 2.0 ** ((torch.arange(Nb) % 5) - 2).double()
    return sa, sb


def view_in(data, layout, name, wide_block=(0, 1)):
    """`data` [R, cols] as a guarded input view.  layout: "dense" (ld = cols), an int (ld = cols + that), "block"
    (column block `wide_block[0]` of a tensor `wide_block[1]` blocks wide; the other columns stay NaN poison), or
    ("offset", k): columns k .. k + cols of a [R, cols + 8] tensor.  Returns (Guarded, view)."""
    R, cols = data.shape
    if layout == "block":
        idx, n = wide_block
        g = guarded(R, n * cols, data.dtype, name=name)
        v = g.t[:, idx * cols:(idx + 1) * cols]
    elif isinstance(layout, tuple):
        g = guarded(R, cols + 8, data.dtype, name=name)
        v = g.t[:, layout[1]:layout[1] + cols]
    else:
        g = guarded(R, cols, data.dtype, ld=cols + (0 if layout == "dense" else layout), name=name)
        v = g.t
    v.copy_(data.cuda())
    g._snap = g.flat.clone()  # an input from here on: the poison around the block is part of the snapshot
    return g, v


def run_at_b(capi, a, b, dtype, layout_a, layout_b, expected_path, ref, what):
    """One guarded dfd_gemm_at_b call, twice on the same (re-poisoned) buffers: path, every element, no byte outside
    the views, the same bits both times.  Returns C."""
    R, Ma = a.shape
    Nb = b.shape[1]
    ga, va = view_in(a.to(dtype), layout_a, "A", wide_block=(1, 3))
    gb, vb = view_in(b.to(dtype), layout_b, "B", wide_block=(0, 2))
    gc = guarded(Ma, Nb, F32, name="C")
    ws = guarded_bytes(capi.gemm_at_b_workspace_bytes(R, Ma, Nb, dtype), name="workspace")
    outs = []
    for call in range(2):
        gc.flat.copy_(gc._snap)  # NaN poison again, C and workspace alike
        ws.flat.copy_(ws._snap)
        capi.gemm_at_b(va, vb, gc.t, ws.t.view(-1))
        assert capi.gemm_at_b_last_path() == expected_path, f"{what}: ran on path {capi.gemm_at_b_last_path()}, the case names {expected_path}"
        assert_exact(gc.t, ref, f"{what} (call {call})")
        ga.assert_untouched(view_too=True)
        gb.assert_untouched(view_too=True)
        gc.assert_untouched()
        ws.assert_untouched()
        outs.append(gc.t.clone())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{what}: the second call gave other bits"
    return outs[0]


TN_LAYOUTS = [("dense", "dense"), (8, 8), ("block", "block")]

# (R, Ma, Nb, expected path, last split empty)
TN_CASES = [
    (1, 128, 128, 128, False),     # one step, 63 of its rows from the zero constant
    (63, 128, 128, 128, False),
    (65, 128, 256, 128, False),    # two steps, the second holds one row; Nb % 256 == 0 but Ma is not
    (257, 128, 128, 128, False),   # 5 steps in 1 split: odd count, both LDS slots
    (513, 128, 384, 128, False),   # 2 splits of 5 and 4 steps
    (1600, 128, 128, 128, True),   # 25 steps, 6 splits x 5
    (1601, 384, 640, 128, False),  # 15 tiles, Ma != Nb, 26 steps
    (2049, 768, 128, 128, True),   # Ma % 256 == 0, Nb not; 33 steps, 8 x 5
    (4033, 128, 128, 128, False),  # 16 splits x 4 steps: even parity, all four reduce groups used
    (64, 256, 256, 256, False),    # one full step
    (1600, 256, 256, 256, True),   # the empty split on the 8-wave kernel
    (1537, 256, 512, 256, True),   # empty split and ragged last step
    (1999, 512, 768, 256, False),  # 6 tiles, 8 x 4
    (3000, 768, 256, 256, True),   # the adapter's own extents: 47 steps, 11 x 5
]


@pytest.mark.parametrize("R,Ma,Nb,path,last_split_empty", TN_CASES)
def test_gemm_at_b_tn_exact(capi, R, Ma, Nb, path, last_split_empty):
    """dfd_gemm_at_b, bf16, on the gemm_tn kernels: dense, ld = cols + 8, and column blocks of wider tensors whose other
    columns are poison.  The rows behind R, the row padding, C and the exactly sized workspace are NaN poison, so a load
    past R or outside the column block, or a slab that is reduced but was never written, poisons C."""
    tile, steps, splits, per = tn_plan(R, Ma, Nb)
    # a check on the inputs, not on the result: if the plan changes, this names the cases that need a new R
    assert tile == path and ((splits - 1) * per >= steps) == last_split_empty, (R, Ma, Nb, tile, steps, splits, per)
    a, b, ref = at_b_operands(R, Ma, Nb)
    ref = as_f32(ref)
    for la, lb in TN_LAYOUTS:
        run_at_b(capi, a, b, BF16, la, lb, path, ref, f"at_b tn R={R} Ma={Ma} Nb={Nb} layout {la}/{lb}")


@pytest.mark.parametrize("R,Ma,Nb,path", [(513, 128, 384, 128), (1600, 256, 256, 256), (1601, 384, 640, 128)])
def test_gemm_at_b_tn_exact_scaled_columns(capi, R, Ma, Nb, path):
    """Column m of A times 2^((m % 7) - 3), column n of B times 2^((n % 5) - 2): exact scalings, so every output row
    and column has a magnitude of its own and a swap of two of them cannot cancel."""
    a, b, ref = at_b_operands(R, Ma, Nb)
    as_f32(ref)
    sa, sb = col_scales(Ma, Nb)
    want = (ref.double() * sa[:, None] * sb[None, :]).to(F32)
    assert torch.equal(want.double(), ref.double() * sa[:, None] * sb[None, :])
    for la, lb in TN_LAYOUTS:
        run_at_b(capi, a.double() * sa, b.double() * sb, BF16, la, lb, path, want, f"at_b tn scaled R={R} Ma={Ma} Nb={Nb} layout {la}/{lb}")


@pytest.mark.parametrize("R,Ma,Nb,layout_a", [(40, 8, 12, "dense"), (40, 8, 12, 8), (777, 128, 32, "dense"), (777, 128, 32, 8),
                                              (513, 128, 384, 4), (513, 128, 384, ("offset", 4))])
def test_gemm_at_b_fallback_bf16_exact(capi, R, Ma, Nb, layout_a):
    """The transpose + general-kernel fallback (path 1): extents that are no multiples of 128, ld = cols + 4 (not a
    multiple of 8), and an A that starts 4 elements into a row of a wider tensor (base 8-byte aligned only).  The two
    (513, 128, 384) cases must also give, bit for bit, the C of the gemm_tn path: both compute the one exact result."""
    a, b, ref = at_b_operands(R, Ma, Nb)
    ref = as_f32(ref)
    layout_b = 4 if layout_a == 4 else "dense" if layout_a == "dense" else 8
    c = run_at_b(capi, a, b, BF16, layout_a, layout_b, 1, ref, f"at_b fallback bf16 R={R} Ma={Ma} Nb={Nb} layout {layout_a}")
    if (R, Ma, Nb) == (513, 128, 384):
        c_tn = run_at_b(capi, a, b, BF16, "dense", "dense", 128, ref, "at_b tn (513, 128, 384) beside the fallback")
        assert torch.equal(c.view(torch.int32), c_tn.view(torch.int32)), "fallback and gemm_tn differ in their bits"


@pytest.mark.parametrize("R,Ma,Nb", [(33, 8, 12), (777, 128, 32), (1600, 128, 128)])
@pytest.mark.parametrize("layout", ["dense", 4])
def test_gemm_at_b_fallback_f32_exact(capi, R, Ma, Nb, layout):
    a, b, ref = at_b_operands(R, Ma, Nb)
    run_at_b(capi, a, b, F32, layout, layout, 1, as_f32(ref), f"at_b f32 R={R} Ma={Ma} Nb={Nb} layout {layout}")


# ---- dfd_gemm ------------------------------------------------------------------------------------------------------

M_MAX = 256 * 9 + 8
T_CLIP = 3


@functools.lru_cache(maxsize=None)
def gemm_operands(N, K, M=M_MAX):
    """A [M, K] in [-3, 3], W [N, K] in [-2, 2] (+1 on every 7th k), A.W^T, and integer bias [N], residual [M, N],
    pos [T_CLIP, N] in [-40, 40]: all int64 on the CPU, computed once per (N, K) (fewer rows: the first rows)."""
    g = torch.Generator().manual_seed(N * 4099 + K)
    a = torch.randint(-3, 4, (M, K), generator=g)
    w = torch.randint(-2, 3, (N, K), generator=g)
    w[:, ::7] += 1
    bias = torch.randint(-40, 41, (N,), generator=g)
    res = torch.randint(-40, 41, (M, N), generator=g)
    pos = torch.randint(-40, 41, (T_CLIP, N), generator=g)
    acc = a @ w.T
    assert int(acc.abs().max()) + 120 < EXACT
    return a, w, acc, bias, res, pos


def nan_out(M, N, dtype):
    return torch.full((M, N), float("nan"), device="cuda", dtype=dtype)


class Gemm:
    """The epilogues of one (M, N, K, operand dtype) on one expected path."""

    def __init__(self, capi, M, N, K, ab_dtype, path, **kw):
        a, w, acc, bias, res, pos = gemm_operands(N, K)
        self.capi, self.M, self.N, self.K, self.path, self.kw = capi, M, N, K, path, kw
        self.acc, self.bias_i, self.res_i, self.pos_i = acc[:M], bias, res[:M], pos
        self.a, self.w = a[:M].to(ab_dtype).cuda(), w.to(ab_dtype).cuda()
        self.bias, self.pos = bias.to(F32).cuda(), pos.to(F32).cuda()
        self.what = f"gemm M={M} N={N} K={K} {ab_dtype} path {path} {kw}"

    def _ran(self, tag, c_dtype):
        got = self.capi.gemm_last_path()
        assert got == self.path, f"{self.what} {tag}: ran on path {got}"
        # path 256 is two kernels: gemm256p.hip has the bf16 C except RESIDUAL_POS, gemm256.hip the rest
        k = self.capi
        tile = c_dtype == F32 or tag == "residual_pos"
        want = {128: k.GEMM_GENERAL, 257: k.GEMM_PINGPONG, 256: k.GEMM_TILE if tile else k.GEMM_PERSISTENT}[self.path]
        assert k.gemm_last_kernel() == want, f"{self.what} {tag}: ran on kernel {k.gemm_last_kernel()}, not {want}"

    def bias_store(self, c_dtype):
        """EPI_BIAS: C = acc + bias in f32, a bf16 C its one rounding."""
        c = nan_out(self.M, self.N, c_dtype)
        self.capi.gemm(self.a, self.w, c, self.bias, self.capi.EPI_BIAS, **self.kw)
        self._ran("bias", c_dtype)
        assert_exact(c, as_f32(self.acc + self.bias_i).to(c_dtype), f"{self.what} bias -> {c_dtype}")

    def bias_residual(self):
        """EPI_BIAS_RESIDUAL: x0 + acc + bias, in f32, in place."""
        c = self.res_i.to(F32).cuda()
        self.capi.gemm(self.a, self.w, c, self.bias, self.capi.EPI_BIAS_RESIDUAL, **self.kw)
        self._ran("bias_residual", F32)
        assert_exact(c, as_f32(self.res_i + self.acc + self.bias_i), f"{self.what} bias_residual")

    def residual_pos(self, c_dtype, rows_per_frame, in_place):
        """EPI_RESIDUAL_POS: C = res + acc + pos[(row / rows_per_frame) % T]: the f32 sum, rounded once."""
        frame = (torch.arange(self.M) // rows_per_frame) % T_CLIP
        want = as_f32(self.res_i + self.acc + self.pos_i[frame]).to(c_dtype)
        res = self.res_i.to(c_dtype).cuda()
        c = res.clone() if in_place else nan_out(self.M, self.N, c_dtype)
        self.capi.gemm(self.a, self.w, c, None, self.capi.EPI_RESIDUAL_POS, pos=self.pos, tokens=rows_per_frame + 1, frames_per_clip=T_CLIP,
                       residual=None if in_place else res, **self.kw)
        self._ran("residual_pos", c_dtype)
        assert_exact(c, want, f"{self.what} residual_pos -> {c_dtype} in_place={in_place}")

    def qkv_export(self, c_dtype, tokens, first):
        """EPI_QKV_EXPORT on [q | k | v] (first = 0) or [k | v] (first = 1: the k|v rows of W into the k|v columns of C):
        C = acc + bias; exports = acc + bias + pos[frame % T] without the CLS rows, each rounded once from the f32 value
        (epilogue_elem in csrc/gemm.hip)."""
        M, N = self.M, self.N
        D = N // 3
        frames = M // tokens
        assert frames * tokens == M and N == 3 * D
        pos_i = self.pos_i[:, :D]
        v = (self.acc + self.bias_i).view(frames, tokens, 3, D)
        e = v[:, 1:] + pos_i[torch.arange(frames) % T_CLIP].view(frames, 1, 1, D)
        c = nan_out(M, N, c_dtype)
        ke, ve = nan_out(frames * (tokens - 1), D, c_dtype), nan_out(frames * (tokens - 1), D, c_dtype)
        self.capi.gemm(self.a, self.w[first * D:], c[:, first * D:], self.bias[first * D:], self.capi.EPI_QKV_EXPORT, pos=self.pos[:, :D].contiguous(),
                       k_export=ke, v_export=ve, tokens=tokens, frames_per_clip=T_CLIP, qkv_first=first, **self.kw)
        self._ran(f"qkv_export first={first}", c_dtype)
        what = f"{self.what} qkv_export -> {c_dtype} qkv_first={first}"
        assert_exact(c[:, first * D:], as_f32(self.acc + self.bias_i)[:, first * D:].to(c_dtype), what + " C")
        assert first == 0 or bool(torch.isnan(c[:, :D]).all()), what + ": the query block was written"
        assert_exact(ke, as_f32(e[:, :, 1].reshape(-1, D)).to(c_dtype), what + " k_export")
        assert_exact(ve, as_f32(e[:, :, 2].reshape(-1, D)).to(c_dtype), what + " v_export")


@pytest.mark.parametrize("M,N,K", [(300, 200, 64), (5, 8, 32)])
def test_gemm_general_exact(capi, M, N, K):
    """The general kernel (path 128): f32 operands, bf16 operands with a bf16 and an f32 C."""
    rpf = 10 if M == 300 else 2
    for ab, cs in ((F32, (F32,)), (BF16, (BF16, F32))):
        t = Gemm(capi, M, N, K, ab, 128)
        for c_dtype in cs:
            t.bias_store(c_dtype)
            for in_place in (False, True):
                t.residual_pos(c_dtype, rpf, in_place)
        t.bias_residual()


@pytest.mark.parametrize("N,K", [(256, 192), (768, 768)])
def test_gemm256_f32_out_exact(capi, N, K):
    """gemm256.hip: bf16 operands into an f32 C (path 256)."""
    t = Gemm(capi, 1120, N, K, BF16, 256)
    t.bias_store(F32)
    t.bias_residual()
    if N == 768:
        for first in (0, 1):
            t.qkv_export(F32, 7, first)


@pytest.mark.parametrize("N,K,variant", [(256, 320, 0), (768, 192, 0), (768, 768, 1)])
def test_gemm256p_exact(capi, N, K, variant):
    """gemm256p.hip (path 256 with a bf16 C): the K depths the ping-pong kernel declines (K / 64 odd or < 6), and
    (768, 768) with the ping-pong kernel switched off.  RESIDUAL_POS at these depths is gemm256.hip's (path 256 too)."""
    old = capi.gemm_set_variant(variant)
    try:
        t = Gemm(capi, 1120, N, K, BF16, 256)
        t.bias_store(BF16)
        for in_place in (False, True):
            t.residual_pos(BF16, 7, in_place)
        if N == 768:
            for first in (0, 1):
                t.qkv_export(BF16, 7, first)
    finally:
        capi.gemm_set_variant(old)


@pytest.mark.parametrize("tile_blocks", [7, 8])
@pytest.mark.parametrize("N,K", [(256, 384), (768, 768), (1024, 4096)])
@pytest.mark.parametrize("M", [1120, M_MAX])
def test_gemm256e_exact(capi, M, N, K, tile_blocks):
    """gemm256e.hip (path 257), tiles of 224 and of 256 rows; M = 256 * 9 + 8 ends in a tile of 8 rows."""
    t = Gemm(capi, M, N, K, BF16, 257, tile_blocks=tile_blocks)
    t.bias_store(BF16)
    for in_place in (False, True):
        t.residual_pos(BF16, 7, in_place)
    if N == 768 and M % 7 == 0:
        for first in (0, 1):
            t.qkv_export(BF16, 7, first)
