"""The decoder attention family through the C ABI (dfd_decoder_attn_fwd / _bwd / _modes_fwd / _modes_bwd / _map) over
the tables of tests/decoder_edge_cases.py: every padding pattern, split counts from 1 past S (one-key and empty
splits, the combine kernel's strided loops on a second and third trip), odd head counts, T = 1, P = 49 and P = 576,
bf16 dk / dv — against the float64 restatement there, at the project's own bars, plus three properties that hold bit
for bit (padded content is irrelevant, clips are independent, in-place + pos equals dense).

Every test prints its worst error per output (run with -s to see them)."""
import pytest
import torch

from tests import decoder_edge_cases as dec
from tests.attnmap_cases import KERNEL_ATOL, KERNEL_RTOL
from tests.decoder_edge_cases import BARS, MODES_BARS, SHAPES, deals, operands, policy_splits, reference, splits_for

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
NAN = float("nan")
_refs = {}


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert c.load_library().dfd_device_check() == 0, c.load_library().dfd_last_error()
    return c


def ref_for(shape, dtype, deal, attn_mode=()):
    """operands and the float64 reference of one (shape, dtype, mask-deal, attn_mode), computed once"""
    key = (shape, dtype, deal, attn_mode)
    if key not in _refs:
        B, T, P, H = shape
        o = operands(B, T, P, H, dtype)
        names, mask = deals(B, T)[deal]
        _refs[key] = (o, names, mask, reference(o, mask, T, attn_mode))
    return _refs[key]


def f32(*shape, fill=NAN):
    return torch.full(shape, fill, device="cuda", dtype=torch.float32)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def dev(o, mask):
    B = o["q"].shape[0]
    return o["q"].reshape(B, -1).cuda(), o["k"].cuda(), o["v"].cuda(), mask.to(torch.uint8).cuda(), o["dmix"].cuda()


def fwd(capi, q, k, v, m, splits, shape, ext=None, pos=None):
    B, T, P, H = shape
    ws = f32(capi.decoder_attn_workspace_bytes(B, H, 64, splits) // 4)
    mix, mix_s, stats = f32(B, H * 64), f32(B, H * 64), f32(B, H, 2)
    capi.decoder_attn_fwd(q, k, v, m, mix, stats, ws, splits, B, T, P, H, mix_softmax=mix_s, ext_weights=ext, pos=pos)
    return mix, mix_s, stats


def amap(capi, q, k, m, stats, shape, ext=None, pos=None):
    B, T, P, H = shape
    aff, br = f32(B, H, T * P), f32(2, B, H, T * P)
    capi.decoder_attn_map(q, k, m, stats, aff, B, T, P, H, ext_weights=ext, branches=br, pos=pos)
    return aff, br


def bwd(capi, q, k, v, m, dmix, mix_s, stats, shape, gdtype=torch.float32, ext=None, ext_ds=None, pos=None):
    B, T, P, H = shape
    S, D = T * P, H * 64
    ws = f32(capi.decoder_attn_bwd_workspace_bytes(B, T, H) // 4)
    dq, dpos = f32(B, 2 * D), f32(T, D)
    dk, dv = (torch.full((B, S, D), NAN, device="cuda", dtype=gdtype) for _ in range(2))
    capi.decoder_attn_bwd(q, k, v, m, dmix, mix_s, stats, dq, dpos, ws, B, T, P, H, dk=dk, dv=dv, ext_weights=ext, ext_dscores=ext_ds, pos=pos)
    return dq, dpos, dk, dv


def modes_chain(capi, q, k, v, m, dmix, modes, splits, shape, pos=None):
    """modes_fwd -> fwd through ext_weights -> modes_bwd -> bwd -> (scores, weights, mix, dscores, dq, dpos, dk, dv)"""
    B, T, P, H = shape
    sc, aw, dsc = f32(B, H, T * P), f32(B, H, T * P), f32(B, H, T * P)
    capi.decoder_attn_modes_fwd(q, k, m, modes, sc, aw, B, T, P, H, pos=pos)
    mix, _, _ = fwd(capi, q, k, v, m, splits, shape, ext=aw, pos=pos)
    capi.decoder_attn_modes_bwd(sc, v, dmix, modes, f32(B, H, T * P), dsc, B, T, P, H, pos=pos)
    dq, dpos, dk, dv = bwd(capi, q, k, v, m, dmix, None, None, shape, ext=aw, ext_ds=dsc, pos=pos)
    return sc, aw, mix, dsc, dq, dpos, dk, dv


class Worst:
    """the worst error per output over a test's cases; check() asserts the bar case by case"""

    def __init__(self):
        self.err = {}

    def check(self, name, got, want, atol, rtol, case):
        err, over = dec.worst(got, want, atol, rtol)
        if err >= self.err.get(name, (-1.0,))[0]:
            self.err[name] = (err, atol, rtol, case)
        assert over <= 0, f"{name} {case}: worst error {err:.3e} exceeds atol {atol:.1e} + rtol {rtol:.1e}"

    def report(self, title):
        for n, (e, a, r, case) in self.err.items():
            print(f"{title} {n}: worst |err| {e:.3e} (bar {a:.1e} + {r:.1e}|ref|) at {case}")


def padded_keys(mask, P, H):
    B = mask.shape[0]
    return (~mask).repeat_interleave(P, dim=1)[:, None, :].expand(B, H, mask.shape[1] * P)


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_forward_and_map(capi, shape, dtype):
    """Every mask-deal x split count: mix, mix_softmax, (max, sumexp) and, from those stats, aff and both branches against
    float64; the maximum is bit-equal across the split counts (a maximum does not depend on the merge order); padded
    keys weigh exactly +0.0; the softmax branch sums to 1."""
    B, T, P, H = shape
    S = T * P
    w = Worst()
    for deal in range(len(deals(B, T))):
        o, names, mask, ref = ref_for(shape, dtype, deal)
        q, k, v, m, _ = dev(o, mask)
        pad = padded_keys(mask, P, H)
        max_bits = None
        for splits in splits_for(B, S):
            case = f"masks {names} splits {splits}"
            if not dec.combine_fits(H, splits):  # past the entry point's ceiling: refused by name, nothing launched
                with pytest.raises(capi.DfdError, match="splits"):
                    fwd(capi, q, k, v, m, splits, shape)
                continue
            mix, mix_s, stats = fwd(capi, q, k, v, m, splits, shape)
            w.check("mix", mix, ref["mix"], *BARS["mix"], case)
            w.check("mix_softmax", mix_s, ref["mix_softmax"], *BARS["mix_softmax"], case)
            w.check("max", stats[..., 0], ref["max"], *BARS["max"], case)
            w.check("sumexp", stats[..., 1], ref["sumexp"], *BARS["sumexp"], case)
            if max_bits is None:
                max_bits = bits(stats[..., 0]).clone()
            assert torch.equal(bits(stats[..., 0]), max_bits), f"{case}: the row maximum depends on the split count"
            aff, br = amap(capi, q, k, m, stats, shape)
            w.check("aff", aff, 0.5 * (ref["ws"] + ref["wc"]), KERNEL_ATOL, KERNEL_RTOL, case)
            w.check("softmax branch", br[0], ref["ws"], KERNEL_ATOL, KERNEL_RTOL, case)
            w.check("CoDA branch", br[1], ref["wc"], KERNEL_ATOL, KERNEL_RTOL, case)
            for t in (aff, br[0], br[1]):
                assert (bits(t).cpu()[pad] == 0).all(), f"{case}: a padded key is not +0.0"
            sums = br[0].double().sum(-1).cpu()
            w.check("softmax branch sum", sums, torch.ones_like(sums), 1e-5, 0.0, case)
    w.report(f"{shape} {dtype}")


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_backward(capi, shape, dtype):
    """dq, dk, dv, dpos against float64 autograd for every mask-deal (stats of the forward at the production split count
    and at the largest count of the table that the forward accepts); dk / dv rows of padded frames are exactly +0.0;
    with dk / dv in bf16 the call returns the f32 dk / dv rounded once, and the same dq and dpos bits."""
    B, T, P, H = shape
    S = T * P
    w = Worst()
    for deal in range(len(deals(B, T))):
        o, names, mask, ref = ref_for(shape, dtype, deal)
        q, k, v, m, dmix = dev(o, mask)
        pad_rows = (~mask).repeat_interleave(P, dim=1)  # [B, S]
        for splits in (policy_splits(B, S), max(s for s in splits_for(B, S) if dec.combine_fits(H, s))):
            case = f"masks {names} splits {splits}"
            _, mix_s, stats = fwd(capi, q, k, v, m, splits, shape)
            dq, dpos, dk, dv = bwd(capi, q, k, v, m, dmix, mix_s, stats, shape)
            for n, t in (("dq", dq), ("dk", dk), ("dv", dv), ("dpos", dpos)):
                w.check(n, t, ref[n], *BARS[n], case)
            assert (bits(dk).cpu()[pad_rows] == 0).all() and (bits(dv).cpu()[pad_rows] == 0).all(), f"{case}: padded dk / dv rows are not +0.0"
            dq16, dpos16, dk16, dv16 = bwd(capi, q, k, v, m, dmix, mix_s, stats, shape, gdtype=torch.bfloat16)
            assert same_bits(dk16, dk.to(torch.bfloat16)) and same_bits(dv16, dv.to(torch.bfloat16)), f"{case}: bf16 dk / dv are not the f32 ones rounded once"
            assert same_bits(dq16, dq) and same_bits(dpos16, dpos), f"{case}: dq / dpos depend on the dk / dv dtype"
    w.report(f"{shape} {dtype}")


def poison(x, mask, P):
    """x [B, S, D] with the rows of padded frames overwritten: zeros, and +-1e4 (in bf16: +-9984)"""
    B, S, D = x.shape
    pad = (~mask).repeat_interleave(P, dim=1)[:, :, None].expand(B, S, D)
    big = torch.where(torch.arange(S * D).view(1, S, D) % 3 == 0, -1e4, 1e4).to(x.dtype).expand(B, S, D)
    return torch.where(pad, torch.zeros_like(x), x), torch.where(pad, big, x)


@pytest.mark.parametrize("in_place", [False, True], ids=["dense", "in_place_pos"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] > 1], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_padded_content_is_irrelevant(capi, shape, dtype, in_place):
    """k and v of padded frames set to +-1e4 instead of 0: every output of fwd, map, bwd and the "temporal" modes chain has
    the same bits (a masked score that leaked into a maximum or a sum would overflow) — for dense K/V and for the
    [frames, tokens, 3D] view read in place with `pos` added on the fly."""
    B, T, P, H = shape
    S, D = T * P, H * 64
    pos = dec.rnd(T, D, seed=52, scale=0.3).cuda() if in_place else None
    for deal in range(len(deals(B, T))):
        o, names, mask, _ = ref_for(shape, dtype, deal)
        if mask.all():
            continue
        q, _, _, m, dmix = dev(o, mask)
        outs = []
        for kk, vv in zip(poison(o["k"], mask, P), poison(o["v"], mask, P)):
            if in_place:
                qkv = torch.zeros(B * T, P + 1, 3 * D, dtype=dtype)
                qkv[:, 1:, D:2 * D], qkv[:, 1:, 2 * D:] = kk.view(B * T, P, D), vv.view(B * T, P, D)
                qkv = qkv.cuda()
                kd, vd = qkv[:, 1:, D:2 * D], qkv[:, 1:, 2 * D:]
            else:
                kd, vd = kk.cuda(), vv.cuda()
            got = []
            for splits in (3, policy_splits(B, S), S + 1):
                mix, mix_s, stats = fwd(capi, q, kd, vd, m, splits, shape, pos=pos)
                got += [mix, mix_s, stats, *amap(capi, q, kd, m, stats, shape, pos=pos)]
            got += bwd(capi, q, kd, vd, m, dmix, mix_s, stats, shape, pos=pos)
            got += bwd(capi, q, kd, vd, m, dmix, mix_s, stats, shape, gdtype=torch.bfloat16, pos=pos)[2:]
            got += modes_chain(capi, q, kd, vd, m, dmix, capi.ATTN_MODE_BITS["temporal"], 3, shape, pos=pos)
            outs.append(got)
        for i, (a, b) in enumerate(zip(*outs)):
            assert not torch.isnan(a).any(), f"masks {names}: output {i} has a NaN"  # the modes' scores are -inf on padded keys
            assert same_bits(a, b), f"masks {names}: output {i} depends on the content of padded frames"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_clips_are_independent(capi, shape, dtype):
    """Clip b's mix, stats, aff, dq, dk, dv from the batched call = a B = 1 call on that clip with the same split count,
    bit for bit (dpos sums over the clips and is left out)."""
    B, T, P, H = shape
    S = T * P
    one = (1, T, P, H)
    for deal in range(len(deals(B, T))):
        o, names, mask, _ = ref_for(shape, dtype, deal)
        q, k, v, m, dmix = dev(o, mask)
        for splits in dict.fromkeys((policy_splits(B, S), 3, 65, S + 1)):
            mix, mix_s, stats = fwd(capi, q, k, v, m, splits, shape)
            aff, br = amap(capi, q, k, m, stats, shape)
            dq, _, dk, dv = bwd(capi, q, k, v, m, dmix, mix_s, stats, shape)
            for b in range(B):
                s = slice(b, b + 1)
                qb, kb, vb, mb, db = q[s].contiguous(), k[s].contiguous(), v[s].contiguous(), m[s].contiguous(), dmix[s].contiguous()
                mix1, mix_s1, stats1 = fwd(capi, qb, kb, vb, mb, splits, one)
                aff1, br1 = amap(capi, qb, kb, mb, stats1, one)
                dq1, _, dk1, dv1 = bwd(capi, qb, kb, vb, mb, db, mix_s1, stats1, one)
                for n, a, a1 in (("mix", mix, mix1), ("mix_softmax", mix_s, mix_s1), ("stats", stats, stats1), ("aff", aff, aff1),
                                 ("branches", br[:, s], br1), ("dq", dq, dq1), ("dk", dk, dk1), ("dv", dv, dv1)):
                    a = a if n == "branches" else a[s]
                    assert torch.isfinite(a).all() and same_bits(a, a1), f"masks {names} splits {splits}: {n} of clip {b} depends on its batch"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_in_place_with_pos_equals_dense(capi, dtype):
    """The construction of test_hip_kernels.py::test_decoder_attention_reads_keys_and_values_in_place at (3, 7, 5, 4) with
    splits 1, 2, 3, 4, 9: a block's rows span up to seven frames of staged positional rows, and splits start mid-frame.
    Forward, map and backward (dk / dv included) equal the dense f32 k + pos bit for bit, and meet the float64 bars."""
    shape = B, T, P, H = 3, 7, 5, 4
    D, tok, S = H * 64, P + 1, T * P
    qkv = dec.rnd(B * T, tok, 3 * D, seed=51).to(dtype).cuda()
    pos = dec.rnd(T, D, seed=52, scale=0.3).cuda()
    kview, vview = qkv[:, 1:, D:2 * D], qkv[:, 1:, 2 * D:]
    pb = pos.repeat(B, 1).view(B * T, 1, D)
    kd, vd = (kview.float() + pb).contiguous().view(B, S, D), (vview.float() + pb).contiguous().view(B, S, D)
    names, mask = deals(B, T)[0]
    assert not mask.all()
    o = dict(q=dec.rnd(B, H, 128, seed=53), k=kd.cpu(), v=vd.cpu(), dmix=dec.rnd(B, D, seed=54))
    ref = reference(o, mask, T)
    q, m, dmix = o["q"].reshape(B, -1).cuda(), mask.to(torch.uint8).cuda(), o["dmix"].cuda()
    w = Worst()
    for splits in (1, 2, 3, 4, 9):
        def run(k, v, p):
            mix, mix_s, stats = fwd(capi, q, k, v, m, splits, shape, pos=p)
            return [mix, mix_s, stats, *amap(capi, q, k, m, stats, shape, pos=p), *bwd(capi, q, k, v, m, dmix, mix_s, stats, shape, pos=p)]
        got, want = run(kview, vview, pos), run(kd, vd, None)
        dense_pos = run(kview.contiguous().view(B, S, D), vview.contiguous().view(B, S, D), pos)
        for i, (a, b, c) in enumerate(zip(got, want, dense_pos)):
            assert torch.isfinite(a).all() and same_bits(a, b) and same_bits(c, b), f"splits {splits}: output {i} differs from the dense run"
        mix, mix_s, stats, aff, br, dq, dpos, dk, dv = got
        for n, t in (("mix", mix), ("mix_softmax", mix_s), ("max", stats[..., 0]), ("sumexp", stats[..., 1]), ("dq", dq), ("dk", dk),
                     ("dv", dv), ("dpos", dpos)):
            w.check(n, t, ref[n], *BARS[n], f"splits {splits}")
        w.check("aff", aff, 0.5 * (ref["ws"] + ref["wc"]), KERNEL_ATOL, KERNEL_RTOL, f"splits {splits}")
    w.report(f"in place {dtype}")


@pytest.mark.parametrize("splits", [1, 3, 65])
@pytest.mark.parametrize("shape", [(3, 3, 5, 4), (4, 7, 20, 12)], ids=str)
def test_fully_padded_clip_forward(capi, shape, splits):
    """A clip without a valid frame: its mix and mix_softmax are NaN and its stats (-inf, 0), as the reference's softmax
    over all -inf; the other clips' outputs are those of the batch without it, bit for bit."""
    B, T, P, H = shape
    o, _, mask, _ = ref_for(shape, torch.float32, 0)
    mask = mask.clone()
    mask[1] = False
    q, k, v, m, _ = dev(o, mask)
    mix, mix_s, stats = fwd(capi, q, k, v, m, splits, shape)
    assert torch.isnan(mix[1]).all() and torch.isnan(mix_s[1]).all()
    assert (stats[1, :, 0] == float("-inf")).all() and (bits(stats[1, :, 1]) == 0).all()
    keep = [b for b in range(B) if b != 1]
    mix2, mix_s2, stats2 = fwd(capi, q[keep].contiguous(), k[keep].contiguous(), v[keep].contiguous(), m[keep].contiguous(), splits,
                               (B - 1, T, P, H))
    for a, a2 in ((mix, mix2), (mix_s, mix_s2), (stats, stats2)):
        assert torch.isfinite(a2).all() and same_bits(a[keep], a2)


def check_modes(capi, w, shape, dtype, modes, deal, splits_list):
    B, T, P, H = shape
    S = T * P
    attn_mode = tuple(modes.split("+"))
    mbits = sum(capi.ATTN_MODE_BITS[a] for a in attn_mode)
    o, names, mask, ref = ref_for(shape, dtype, deal, attn_mode)
    q, k, v, m, dmix = dev(o, mask)
    fs, gs = max(1.0, ref["mix"].abs().max().item()), max(1.0, ref["dq"].abs().max().item())
    for splits in splits_list:
        case = f"{modes} masks {names} splits {splits}"
        sc, aw, mix, dsc, dq, dpos, dk, dv = modes_chain(capi, q, k, v, m, dmix, mbits, splits, shape)
        w.check("weights", aw, ref["ws"], KERNEL_ATOL, KERNEL_RTOL, case)
        want_sum = (T if "frame" in attn_mode else 0) + (P if "temporal" in attn_mode else 0)
        w.check("weights sum", aw.double().sum(-1), torch.full((B, H), float(want_sum), dtype=torch.float64), 1e-3 * want_sum, 0.0, case)
        assert (bits(aw).cpu()[padded_keys(mask, P, H)] == 0).all(), f"{case}: a padded key's weight is not +0.0"
        w.check("mix", mix, ref["mix"], MODES_BARS["mix"][0] * fs, MODES_BARS["mix"][1], case)
        for n, t in (("dq", dq), ("dk", dk), ("dv", dv), ("dpos", dpos)):
            w.check(n, t, ref[n], MODES_BARS[n][0] * gs, MODES_BARS[n][1], case)
        aff, br = amap(capi, q, k, m, None, shape, ext=aw)
        assert same_bits(br[0], aw), f"{case}: the map's softmax branch is not ext_weights itself"
        w.check("aff", aff, 0.5 * (ref["ws"] + ref["wc"]), KERNEL_ATOL, KERNEL_RTOL, case)


@pytest.mark.parametrize("modes", ["temporal", "frame", "frame+temporal"])
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[1] * s[2] <= 1728], ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_modes(capi, shape, dtype, modes):
    """op_mode.attn_mode: the grouped-softmax weights, the forward through `ext_weights`, modes_bwd and attn_bwd against
    float64 — "temporal" with every mask-deal; "frame" and "frame+temporal" with full clips only (a padded frame's
    "frame" group is NaN, in the reference as well: test_hip_backward.py::test_decoder_attention_modes)."""
    B, T, P, H = shape
    S = T * P
    w = Worst()
    for deal in range(len(deals(B, T))):
        if modes != "temporal" and not deals(B, T)[deal][1].all():
            continue
        check_modes(capi, w, shape, dtype, modes, deal, dict.fromkeys((3, policy_splits(B, S), 65, S + 1)))
    if modes != "temporal" and not any(mk.all() for _, mk in deals(B, T)):  # no deal is all `full`: a full batch of its own
        key = (shape, dtype, "full", tuple(modes.split("+")))
        if key not in _refs:
            o = operands(B, T, P, H, dtype)
            mask = torch.ones(B, T, dtype=torch.bool)
            _refs[key] = (o, ("full",) * B, mask, reference(o, mask, T, key[3]))
        check_modes(capi, w, shape, dtype, modes, "full", dict.fromkeys((3, policy_splits(B, S), 65, S + 1)))
    assert w.err, "no case ran"
    w.report(f"{shape} {dtype}")


def test_modes_at_the_lds_ceiling(capi):
    """(1, 50, 256, 2): S = 12,800, and modes_bwd's three floats per key are 150 KiB, the most the entry points accept: the
    raised dynamic-LDS launch at its limit."""
    shape = (1, 50, 256, 2)
    key = (shape, torch.bfloat16, "full", ("frame", "temporal"))
    o = operands(*shape, torch.bfloat16)
    mask = torch.ones(1, 50, dtype=torch.bool)
    _refs[key] = (o, ("full",), mask, reference(o, mask, 50, key[3]))
    w = Worst()
    check_modes(capi, w, shape, torch.bfloat16, "frame+temporal", "full", (policy_splits(1, 12800),))
    w.report(f"{shape}")
    del _refs[key]


def test_modes_refuse_what_does_not_fit_one_lds_pass(capi):
    """(1, 23, 576, 2): S = 13,248 is past the ceiling; both entry points say so instead of launching."""
    B, T, P, H = 1, 23, 576, 2
    S, D = T * P, H * 64
    q, k, dmix = f32(B, 2 * D, fill=0.0), f32(B, S, D, fill=0.0), f32(B, D, fill=0.0)
    m = torch.ones(B, T, dtype=torch.uint8, device="cuda")
    sc, aw, dsc = f32(B, H, S), f32(B, H, S), f32(B, H, S)
    for modes in (1, 2, 3):
        with pytest.raises(capi.DfdError, match="too large for one LDS pass"):
            capi.decoder_attn_modes_fwd(q, k, m, modes, sc, aw, B, T, P, H)
        with pytest.raises(capi.DfdError, match="too large for one LDS pass"):
            capi.decoder_attn_modes_bwd(sc, k, dmix, modes, f32(B, H, S), dsc, B, T, P, H)
    assert torch.isnan(sc).all() and torch.isnan(aw).all() and torch.isnan(dsc).all(), "a refused call wrote its outputs"


def test_split_ceiling(capi):
    """The combine kernel keeps heads x splits rescale weights in LDS: a count that cannot get them is refused by name,
    before the partial kernel runs (the workspace stays untouched); the largest accepted heads x splits runs and meets the
    forward bar at S = 16, where all but 16 of its splits are empty."""
    assert all(dec.combine_fits(H, s) for B, T, P, H in SHAPES for s in splits_for(B, T * P) if (H, s) != (16, 3459))
    T, P = 2, 8
    for B, H, splits in ((1, 16, 4096), (1, 16, 2559), (1, 1, 4097), (1, 16, 4097)):
        assert not dec.combine_fits(H, splits)
        q, k = f32(B, 2 * H * 64, fill=0.0), f32(B, T * P, H * 64, fill=0.0)
        m = torch.ones(B, T, dtype=torch.uint8, device="cuda")
        ws = f32(B * splits * H * 130)
        mix, stats = f32(B, H * 64), f32(B, H, 2)
        with pytest.raises(capi.DfdError, match="splits") as e:
            capi.decoder_attn_fwd(q, k, k, m, mix, stats, ws, splits, B, T, P, H)
        assert splits > 4096 or "heads" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert torch.isnan(ws).all() and torch.isnan(mix).all() and torch.isnan(stats).all(), "a refused call launched a kernel"
    w = Worst()
    # heads * splits = 40928: 160 KiB less the kernel's two static rows; 4 x 4096: the first count past the 64 KiB a launch
    # gets unasked, at the largest split count
    for H, splits in ((16, 2558), (4, 4096)):
        assert dec.combine_fits(H, splits)
        shape = (2, T, P, H)
        o = operands(*shape, torch.float32)
        mask = torch.stack([dec.frame_mask("full", T), dec.frame_mask("tail", T)])
        ref = reference(o, mask, T)
        q, k, v, m, _ = dev(o, mask)
        mix, mix_s, stats = fwd(capi, q, k, v, m, splits, shape)
        case = f"heads {H} splits {splits}"
        w.check("mix", mix, ref["mix"], *BARS["mix"], case)
        w.check("mix_softmax", mix_s, ref["mix_softmax"], *BARS["mix_softmax"], case)
        w.check("max", stats[..., 0], ref["max"], *BARS["max"], case)
        w.check("sumexp", stats[..., 1], ref["sumexp"], *BARS["sumexp"], case)
        _, _, stats1 = fwd(capi, q, k, v, m, 1, shape)
        assert same_bits(stats[..., 0], stats1[..., 0])
    w.report("split ceiling")
