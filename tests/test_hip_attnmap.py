"""dfd_decoder_attn_map alone (include/dfdclip_explain.h): the per-key weight ½(softmax + CoDA) that dfd_decoder_attn_fwd
applied to v, against the float64 restatement of tests/attnmap_cases.py and against the forward's own `mix`.

Bar: the one the forward meets on `mix` for the same sums (test_hip_kernels.py::test_decoder_attention, atol 2e-5,
rtol 1e-4); every weight is <= 1 in magnitude (under attn_mode "frame+temporal" <= 1.5), so it is meaningful."""
import pytest
import torch

from tests.attnmap_cases import KERNEL_ATOL, KERNEL_RTOL, attention_branches, worst

pytestmark = pytest.mark.gpu

SHAPES = [(2, 4, 4, 2), (3, 3, 5, 4), (3, 3, 196, 4), (1, 5, 256, 16)]  # (3, 3, 5, 4): S = 15, no multiple of the rows per trip
SPLITS = 3
_cache = {}


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert c.load_library().dfd_device_check() == 0, c.load_library().dfd_last_error()
    return c


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def operands(B, T, P, heads, dtype):
    """Seeded q, k, v (k, v rounded to `dtype`), a padded tail on clip 1, and the float64 branches — computed once."""
    key = (B, T, P, heads, dtype)
    if key not in _cache:
        S = T * P
        k, v = rnd(B, S, heads * 64, seed=17).to(dtype), rnd(B, S, heads * 64, seed=18).to(dtype)
        q = rnd(B, heads, 128, seed=19)
        m = torch.ones(B, T, dtype=torch.bool)
        if B > 1:
            m[1, T - max(1, T // 4):] = False
        ws, wc = attention_branches(q, k.float(), m, T)
        _cache[key] = dict(q=q, k=k, v=v, m=m, ws=ws, wc=wc)
    return _cache[key]


def run_pair(capi, o, B, T, P, heads, branches=True):
    """forward, then the map from the stats it wrote -> (mix, aff, branches)"""
    S, D = T * P, heads * 64
    f32 = dict(device="cuda", dtype=torch.float32)
    q, k, v, m = o["q"].cuda(), o["k"].cuda(), o["v"].cuda(), o["m"].to(torch.uint8).cuda()
    ws = torch.empty(capi.decoder_attn_workspace_bytes(B, heads, 64, SPLITS) // 4, **f32)
    mix, stats = torch.empty(B, D, **f32), torch.empty(B, heads, 2, **f32)
    capi.decoder_attn_fwd(q, k, v, m, mix, stats, ws, SPLITS, B, T, P, heads)
    aff = torch.full((B, heads, S), float("nan"), **f32)
    br = torch.full((2, B, heads, S), float("nan"), **f32) if branches else None
    capi.decoder_attn_map(q, k, m, stats, aff, B, T, P, heads, branches=br)
    return mix, aff, br


@pytest.mark.parametrize("B,T,P,heads", SHAPES)
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_map_matches_restatement_and_forward(capi, B, T, P, heads, dtype):
    o = operands(B, T, P, heads, dtype)
    S = T * P
    mix, aff, br = run_pair(capi, o, B, T, P, heads)
    assert torch.isfinite(aff).all() and torch.isfinite(br).all(), "an element was not written"
    want = 0.5 * (o["ws"] + o["wc"])
    for name, got, ref in (("aff", aff, want), ("softmax branch", br[0], o["ws"]), ("CoDA branch", br[1], o["wc"])):
        err, over = worst(got, ref)
        print(f"{name}: worst |err| {err:.3e} (|w| <= {ref.abs().max().item():.3f})")
        assert over <= 0, f"{name}: worst error {err:.3e} exceeds atol {KERNEL_ATOL} + rtol {KERNEL_RTOL}"
    # consistency with the forward: the weights reproduce its mix
    vh = o["v"].double().view(B, S, heads, 64)
    remix = torch.einsum("bhs,bshc->bhc", aff.double().cpu(), vh).reshape(B, heads * 64)
    err, over = worst(mix, remix)
    print(f"mix from the kernel's aff vs the forward's mix: worst |err| {err:.3e}")
    assert over <= 0, f"forward mix differs from sum(aff * v): {err:.3e}"
    # padded keys are exactly 0.0 in every output (+0.0: all bits clear)
    pad = ~o["m"].repeat_interleave(P, dim=1)[:, None, :].expand(B, heads, S)
    for t in (aff, br[0], br[1]):
        assert (t.cpu().view(torch.int32)[pad] == 0).all()
    # the softmax branch is a distribution per (clip, head)
    sums = br[0].double().sum(-1).cpu()
    print(f"softmax branch sums: worst |sum - 1| {(sums - 1).abs().max().item():.3e}")
    assert (sums - 1).abs().max().item() <= 1e-5
    # aff = ½(softmax + CoDA) of the stored branches, within one f32 ulp
    half = 0.5 * (br[0].double() + br[1].double())
    ulp = torch.finfo(torch.float32).eps * half.abs().clamp_min(torch.finfo(torch.float32).tiny)
    assert ((aff.double() - half).abs() <= ulp).all()
    # launching twice gives equal bits, with and without the second output
    _, aff2, br2 = run_pair(capi, o, B, T, P, heads)
    assert torch.equal(aff.view(torch.int32), aff2.view(torch.int32)) and torch.equal(br.view(torch.int32), br2.view(torch.int32))
    _, aff3, _ = run_pair(capi, o, B, T, P, heads, branches=False)
    assert torch.equal(aff.view(torch.int32), aff3.view(torch.int32))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("modes", [0, 3])
def test_map_in_place_equals_dense(capi, dtype, modes):
    """K read through a [frames, tokens, 3D] view with `pos` added on the fly = the dense f32 k + pos, bit for bit (the
    construction of test_hip_kernels.py::test_decoder_attention_reads_keys_and_values_in_place); with modes = 3 the
    softmax branch is the grouped-softmax pass's `ext_weights`, bit for bit."""
    B, T, P, H = 3, 4, 20, 4
    D, tok, S = H * 64, P + 1, T * P
    qkv = rnd(B * T, tok, 3 * D, seed=51).to(dtype).cuda()
    pos = rnd(T, D, seed=52, scale=0.3).cuda()
    kview, vview = qkv[:, 1:, D:2 * D], qkv[:, 1:, 2 * D:]
    pb = pos.repeat(B, 1).view(B * T, 1, D)
    kd, vd = (kview.float() + pb).contiguous().view(B * S, D), (vview.float() + pb).contiguous().view(B * S, D)
    q = rnd(B, 2 * D, seed=53).cuda()
    m = torch.ones(B, T, dtype=torch.uint8)
    if not modes:  # "frame" groups of a padded frame are NaN in the forward's weights, as in the reference
        m[1, T - 1:] = 0
    m = m.cuda()
    f32 = dict(device="cuda", dtype=torch.float32)

    def run(k, v, p):
        ws = torch.empty(capi.decoder_attn_workspace_bytes(B, H, 64, 2) // 4, **f32)
        mix, stats = torch.empty(B, D, **f32), torch.empty(B, H, 2, **f32)
        aw = None
        if modes:
            sc, aw = torch.empty(B, H, S, **f32), torch.empty(B, H, S, **f32)
            capi.decoder_attn_modes_fwd(q, k, m, modes, sc, aw, B, T, P, H, pos=p)
        capi.decoder_attn_fwd(q, k, v, m, mix, stats, ws, 2, B, T, P, H, ext_weights=aw, pos=p)
        aff, br = torch.full((B, H, S), float("nan"), **f32), torch.full((2, B, H, S), float("nan"), **f32)
        capi.decoder_attn_map(q, k, m, None if modes else stats, aff, B, T, P, H, ext_weights=aw, branches=br, pos=p)
        return mix, aff, br, aw

    bits = lambda t: t.view(torch.int32)
    got, want = run(kview, vview, pos), run(kd, vd, None)
    for a, b in zip(got[:3], want[:3]):
        assert torch.isfinite(a).all() and torch.equal(bits(a), bits(b))
    got2 = run(kview.contiguous().view(B * S, D), vview.contiguous().view(B * S, D), pos)  # dense with `pos`: same path
    for a, b in zip(got2[:3], want[:3]):
        assert torch.equal(bits(a), bits(b))
    mix, aff, br, aw = got
    if modes:
        assert torch.equal(bits(br[0]), bits(aw)), "the softmax branch must be ext_weights itself"
    # and it is the weight of this forward
    ws_, wc_ = attention_branches(q.view(B, H, 128).cpu(), kd.view(B, S, D).cpu(), m.bool().cpu(), T,
                                  ("frame", "temporal") if modes else ())
    err, over = worst(aff, 0.5 * (ws_ + wc_))
    print(f"modes={modes}: aff worst |err| {err:.3e}")
    assert over <= 0
    remix = torch.einsum("bhs,bshc->bhc", aff.double().cpu(), vd.double().cpu().view(B, S, H, 64)).reshape(B, D)
    err, over = worst(mix, remix, atol=KERNEL_ATOL * max(1.0, remix.abs().max().item()))
    print(f"modes={modes}: mix worst |err| {err:.3e}")
    assert over <= 0


def test_map_refuses_bad_arguments(capi):
    B, T, P, H = 1, 2, 4, 2
    f32 = dict(device="cuda", dtype=torch.float32)
    q, k = torch.zeros(B, H, 128, **f32), torch.zeros(B, T * P, H * 64, **f32)
    m, stats, aff = torch.ones(B, T, dtype=torch.uint8, device="cuda"), torch.ones(B, H, 2, **f32), torch.empty(B, H, T * P, **f32)
    with pytest.raises(capi.DfdError, match="null pointer"):
        capi.decoder_attn_map(q, k, m, None, aff, B, T, P, H)  # neither stats nor ext_weights
    odd = torch.zeros(B * T, P + 1, 3 * H * 64 + 2, **f32)
    with pytest.raises(capi.DfdError, match="16-byte aligned"):
        capi.decoder_attn_map(q, odd[:, 1:, :H * 64], m, stats, aff, B, T, P, H)
