"""The c_fc -> c_proj pair with a fragment-blocked intermediate `u` (csrc/gemm_blocked.hpp, dfd-clip_amd/blocked.py).

c_fc stores its accumulator fragments as they are (output channels permuted once on the host, so that a lane's fragments
are 16 consecutive channels of its row) and c_proj's LDS-DMA loader restores the row image address by address.  The
values of `u` and every bit behind it are those of the row-major pair, so every comparison here is `torch.equal`
against the SAME kernel run row-major (`capi.gemm_pair_set_variant(1)`); the row-major runs are also held against fp64 on
the same bf16 operands (f32 accumulation order + one rounding: rtol 2^-8, as tests/test_hip_kernels.py does).

What the row-major reference at M = 96 .. 480 is and is not: a flagged call waives the ping-pong kernel's M >= 1024 rule
under variant 1 too, so the reference is that kernel with a row-major C / A — the right twin for a layout comparison, but
not the kernel an unflagged call of that size takes in production (those go to the one-workgroup-per-tile or the general
kernel).  The fp64 check is what ties the reference to the truth; the encoder test compares against the production path.

The map test runs on the CPU; the rest need the GPU."""
import pytest
import torch

from dfd_clip_amd import blocked

gpu = pytest.mark.gpu


# ---- the map (CPU) -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 16, 96, 224 + 32, 352])
@pytest.mark.parametrize("C", [64, 512, 3072])
def test_pack_unpack_and_index_map(M, C):
    x = torch.arange(M * C, dtype=torch.int32).view(M, C)
    b = blocked.pack(x, fill=-1)
    assert b.shape == (blocked.padded_rows(M), C) and b.is_contiguous()
    assert torch.equal(blocked.unpack(b, M), x)
    assert torch.equal(blocked.unpack(b)[M:], torch.full((blocked.padded_rows(M) - M, C), -1, dtype=torch.int32))
    # the index map, element by element on a sample: piece (s, er, eq) of unit (g, kt) holds channels 16 eq + 8 s .. + 7
    flat = b.view(-1)
    g = torch.Generator().manual_seed(M * 7 + C)
    for r, c in zip(torch.randint(0, M, (64,), generator=g).tolist(), torch.randint(0, C, (64,), generator=g).tolist()):
        assert int(flat[blocked.piece_offset(r, c, C)]) == r * C + c
    for r, c in ((0, 0), (M - 1, C - 1), (M - 1, 0), (0, C - 1)):
        assert int(flat[blocked.piece_offset(r, c, C)]) == r * C + c
    # a unit is 2 KB of 2-byte elements: 16 rows of one 64-channel K tile, and nothing else
    kt = C // 64 - 1
    unit = flat[blocked.piece_offset(0, 64 * kt, C):][:1024]
    assert sorted(unit.tolist()) == sorted(x[:16, 64 * kt:64 * kt + 64].reshape(-1).tolist() + [-1] * (max(0, 16 - M) * 64))


@pytest.mark.parametrize("C", [64, 512, 3072])
def test_channel_permutation_composed_with_the_lane_map(C):
    perm = blocked.fc_channel_perm(C)
    assert torch.equal(perm[perm], torch.arange(C)), "the permutation is its own inverse"
    assert sorted(perm.tolist()) == list(range(C))
    for base in range(0, C, 64):
        for j in range(4):
            for eq in range(4):
                for e in range(4):
                    # MFMA column 16 j + 4 eq + e of the group computes true channel 16 eq + 4 j + e
                    assert int(perm[base + 16 * j + 4 * eq + e]) == base + 16 * eq + 4 * j + e
    for eq in range(4):
        ch = blocked.lane_channels(eq)  # [j][e]: the lane's fragments acc[i][j][e]
        assert [c for row in ch for c in row] == list(range(16 * eq, 16 * eq + 16)), "16 consecutive channels per lane"
        for s in range(2):  # piece (s, er, eq) = acc[i][2s], acc[i][2s + 1] = chunk 2 eq + s of the row's K tile
            assert ch[2 * s] + ch[2 * s + 1] == list(range(8 * (2 * eq + s), 8 * (2 * eq + s) + 8))
            assert blocked.piece_offset(0, ch[2 * s][0], 64) == s * 512 + eq * 8


# ---- the kernels (GPU) ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert c.load_library().dfd_device_check() == 0, c.load_library().dfd_last_error()
    return c


def _close(got, want, atol, rtol, msg):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err, lim = (got - want).abs(), atol + rtol * want.abs()
    assert torch.isfinite(got).all(), f"{msg}: non-finite output"
    assert (err <= lim).all(), f"{msg}: max err {err.max().item():.3e}"


class _row_major:
    """The same calls on the same kernel with a row-major C / A."""

    def __init__(self, capi):
        self.capi = capi

    def __enter__(self):
        self.old = self.capi.gemm_pair_set_variant(1)

    def __exit__(self, *exc):
        self.capi.gemm_pair_set_variant(self.old)


# one ragged panel; a full panel + a ragged one; 224-row tiles with a last panel of 32 rows; and a last row group that
# is half inside M (the other three are multiples of 16)
MS = [96, 352, 480, 200]


@gpu
@pytest.mark.parametrize("epi", ["quickgelu", "gelu"])
@pytest.mark.parametrize("K", [384, 768])
@pytest.mark.parametrize("M", MS)
def test_c_fc_blocked_equals_row_major(capi, M, K, epi):
    from tests import guarded as G
    N = 512
    g = torch.Generator(device="cuda").manual_seed(M + K)
    a = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    e = capi.EPI_BIAS_QUICKGELU if epi == "quickgelu" else capi.EPI_BIAS_GELU
    ref = a.double() @ w.double().T + bias.double()
    ref = ref * torch.sigmoid(1.702 * ref) if epi == "quickgelu" else torch.nn.functional.gelu(ref)
    Mp = blocked.padded_rows(M)
    with _row_major(capi):
        want = torch.full((Mp, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        capi.gemm(a, w, want, bias, e, m=M, c_blocked=True)
        assert capi.gemm_last_path() == 257
    assert torch.isnan(want[M:].float()).all()
    want = want[:M]
    _close(want, ref, 1e-4, 2 ** -8, "row-major c_fc")
    idx = blocked.fc_channel_perm(N, device="cuda")
    wp, bp = w[idx].contiguous(), bias[idx].contiguous()
    for opts in (dict(), dict(tile_blocks=7), dict(tile_blocks=8, stream_out=True)):
        u = G.guarded(Mp, N, torch.bfloat16, name="u")  # poisoned: every element a NaN with the harness's payload
        n0 = capi.gemm_pair_launches()
        capi.gemm(a, wp, u.t, bp, e, m=M, c_blocked=True, **opts)
        assert capi.gemm_last_path() == 257 and capi.gemm_pair_launches() == n0 + 1
        u.assert_untouched()
        rows = blocked.unpack(u.t.contiguous())
        assert torch.equal(rows[:M], want), opts
        tail = rows[M:].view(torch.int16)
        assert bool((tail == G.nan_pattern(2)).all()), "pieces of the rows beyond M were written"


@gpu
@pytest.mark.parametrize("N", [256, 768])
@pytest.mark.parametrize("K", [512, 3072])
@pytest.mark.parametrize("M", MS)
def test_c_proj_from_blocked_equals_row_major(capi, M, K, N):
    from tests import guarded as G
    g = torch.Generator(device="cuda").manual_seed(M + K + N)
    u = torch.randn(M, K, device="cuda", generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device="cuda", generator=g) * 0.1
    ref = u.double() @ w.double().T + bias.double()
    ub = blocked.pack(u, fill=float("nan"))  # the pieces of the rows beyond M are never read
    up = blocked.unpack(ub)                  # row-major, rows rounded up to 16 like the blocked buffer
    for tb in (7, 8):
        with _row_major(capi):
            want = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
            capi.gemm(up, w, want, bias, capi.EPI_BIAS, m=M, tile_blocks=tb, a_blocked=True)
            assert capi.gemm_last_path() == 257
        _close(want, ref, 1e-4, 2 ** -8, f"row-major c_proj, tile blocks {tb}")
        c = G.guarded(M, N, torch.bfloat16, name="delta")
        n0 = capi.gemm_pair_launches()
        capi.gemm(ub, w, c.t, bias, capi.EPI_BIAS, m=M, tile_blocks=tb, a_blocked=True)
        assert capi.gemm_last_path() == 257 and capi.gemm_pair_launches() == n0 + 1
        c.assert_untouched()
        assert torch.equal(c.t, want), tb


@gpu
def test_a_flagged_call_that_the_kernel_cannot_serve_is_an_error(capi):
    a = torch.zeros(64, 320, device="cuda", dtype=torch.bfloat16)  # five K steps: not the ping-pong kernel's
    w = torch.zeros(256, 320, device="cuda", dtype=torch.bfloat16)
    c = torch.zeros(64, 256, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(capi.DfdError):
        capi.gemm(a, w, c, None, capi.EPI_BIAS_QUICKGELU, c_blocked=True)
    with pytest.raises(capi.DfdError):
        capi.gemm(a, w, c, None, capi.EPI_BIAS_QUICKGELU, a_blocked=True)  # blocked A: the plain epilogue only


def test_plan_query():
    """The plan is host arithmetic: both halves put to the ping-pong kernel's own eligibility check (the one the launcher
    applies), M >= 1024 unless variant 2."""
    from dfd_clip_amd import capi
    capi.load_library()
    assert capi.gemm_pair_plan(94560, 768, 3072) and capi.gemm_pair_plan(1024, 1024, 4096)
    assert not capi.gemm_pair_plan(394, 768, 3072), "below 1024 rows the pair stays row-major"
    assert not capi.gemm_pair_plan(94560, 128, 512), "K = 128 is not the ping-pong kernel's depth"
    assert not capi.gemm_pair_plan(94560, 768, 3072 + 64)
    old = capi.gemm_pair_set_variant(2)
    try:
        assert old == 0 and capi.gemm_pair_plan(394, 768, 3072) and not capi.gemm_pair_plan(394, 128, 512)
        capi.gemm_pair_set_variant(1)
        assert not capi.gemm_pair_plan(94560, 768, 3072)
        capi.gemm_pair_set_variant(0)
        capi.gemm_set_variant(1)  # without the ping-pong kernel nothing knows the layout
        assert not capi.gemm_pair_plan(94560, 768, 3072)
    finally:
        capi.gemm_set_variant(0)
        capi.gemm_pair_set_variant(0)


# ---- the encoder ---------------------------------------------------------------------------------------------------------

def _encoder(arch, precision="bf16", seed=0):
    from dfd_clip_amd.encoder import VisionTransformer
    from dfd_clip_amd.weights import ARCHS
    torch.manual_seed(seed)
    return VisionTransformer(*ARCHS[arch], precision=precision).cuda().eval()


def _taps(capi, enc, x, taps, variant):
    old = capi.gemm_pair_set_variant(variant)
    try:
        n0 = capi.gemm_pair_launches()
        with torch.no_grad():
            k, v = enc.extract_kv(x, taps, x.shape[0])
        torch.cuda.synchronize()
        return k.clone(), v.clone(), capi.gemm_pair_launches() - n0
    finally:
        capi.gemm_pair_set_variant(old)


@gpu
def test_encoder_taps_bit_identical_with_and_without_the_pair(capi):
    """ViT-B/16, 2 frames (394 rows: one full and one ragged row panel), pair forced on (variant 2: the plan says yes below
    1,024 rows too) against forced off (unflagged calls: the kernels production uses at that size); and the tiny tower,
    whose MLP (K = 128) the ping-pong kernel does not serve: the plan says no and the pair is the row-major one under every
    variant.  So the tiny half shows that the fallback is taken (0 blocked launches) and nothing else: the blocked path is
    NOT exercised on the tiny configuration, it cannot be; ViT-B/16 is the coverage of the blocked path at encoder level."""
    enc = _encoder("ViT-B/16")
    taps = [6, 7, 8, 9, 10, 11]
    x = torch.randn(2, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    k0, v0, n_off = _taps(capi, enc, x, taps, 1)
    k1, v1, n_on = _taps(capi, enc, x, taps, 2)
    assert n_off == 0 and n_on == 2 * 11, "11 MLPs run in an extraction that ends at layer 11's K | V projection"
    assert torch.isfinite(k1.float()).all() and torch.equal(k0, k1) and torch.equal(v0, v1)
    # the state dict is untouched, the permuted copies live beside the prepared ones
    bp = enc._prepare()["blocks"][0]
    idx = blocked.fc_channel_perm(3072, device="cuda")
    assert torch.equal(bp["w_fc"], enc.transformer.resblocks[0].mlp.c_fc.weight.to(torch.bfloat16))
    assert torch.equal(bp["w_fc_blk"], bp["w_fc"][idx]) and torch.equal(bp["b_fc_blk"], bp["b_fc"][idx])

    tiny = _encoder("tiny")
    xt = torch.randn(2, 3, 32, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2))
    a = _taps(capi, tiny, xt, [0, 1], 1)
    b = _taps(capi, tiny, xt, [0, 1], 2)
    assert a[2] == 0 and b[2] == 0 and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@gpu
@pytest.mark.parametrize("policy,blocked_layers", [("all", 0), ("proj-bf16", 0), ("none", 2)])
def test_fp8_and_u8_configurations_take_the_row_major_pair(capi, policy, blocked_layers):
    """An e4m3 c_fc writes `u8` (policy "all") or a row-major bf16 `u` ("proj-bf16"): neither is a blocked pair.  Policy
    "none" is the bf16 arithmetic and takes it.  Asserted through the plan (`_pair_blocked`) and the launch count."""
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    from tests.cases import make_config
    B, T = 3, 2  # 6 frames x 197 rows = 1,182 rows: the e4m3 kernels' smallest shape is 1,024
    cfg = make_config("ViT-B/16", decode_mode="index", decode_indices=[1, 2])
    det = Detector(cfg, T, None, precision="fp8")
    det.load_state_dict(random_state_dict(cfg, T, seed=0))
    det = det.cuda().eval()
    x = torch.randn(B, T, 3, 224, 224, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    det.calibrate_fp8(x)
    det.set_fp8_policy(policy)
    enc, M = det.encoder, B * T * 197
    plan = enc.fp8_policy()
    got = [enc._pair_blocked(bp, M, plan[bp["idx"]]) for bp in enc._prepare()["blocks"][:2]]
    assert got == [blocked_layers > 0] * 2
    n0 = capi.gemm_pair_launches()
    with torch.no_grad():
        k, _ = enc.extract_kv(x.flatten(0, 1), [1, 2], T)
    torch.cuda.synchronize()
    assert torch.isfinite(k.float()).all() and capi.gemm_pair_launches() - n0 == 2 * blocked_layers
