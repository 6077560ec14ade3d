"""GPU parity of dfd_kv_gather_patches (include/dfdclip_kvgather.h, csrc/kv_gather.hip) against `detector.gather_reference`
on the same operands, BIT FOR BIT: the kernel only moves rows and adds one rounded value, so there is no tolerance.

Every case keeps its source, its index table and both outputs between poisoned guards (tests/guarded.py).  Of the source,
only the rows that the table names hold numbers: CLS rows, the Q third, rows of patches that were not kept and all padding
are NaN, so a load from anywhere else shows in the result, which must be finite.  Shapes are the smallest at which the
kernel can go wrong: row counts that are no multiple of the rows per block, several blocks, D on both sides of the 16-byte
rule, unsorted tables with a repeated entry, and one layer stride beyond 2^31 elements."""
import ctypes

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.detector import gather_reference
from tests.guarded import guarded, guarded_1d

pytestmark = pytest.mark.gpu

NAN = float("nan")
VEC = {torch.float32: 4, torch.bfloat16: 8}
GEOMETRIES = [(4, 1), (4, 2), (4, 4), (9, 5)]                 # (P, S)
BATCHES = [(3, 3), (6, 3), (5, 5)]                            # (frames, T): B=1 T=3, B=2 T=3, T=5
WIDTHS = [(128, torch.bfloat16), (768, torch.bfloat16), (1536, torch.bfloat16), (72, torch.bfloat16), (128, torch.float32),
          (100, torch.float32), (66, torch.bfloat16)]


def bits(t):
    return t.contiguous().view(torch.uint8)


def same(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def table(L, P, S, seed):
    """int32 [L, S]: unsorted rows, the last one with a repeated entry where it has two."""
    rng = np.random.RandomState(seed)
    rows = []
    for _ in range(L):
        r = rng.permutation(P)[:S]
        if S >= 2 and (np.diff(r) > 0).all():
            r = r[::-1].copy()
        rows.append(r)
    if S >= 2:
        rows[-1][-1] = rows[-1][0]
    return torch.as_tensor(np.stack(rows), dtype=torch.int32)


def host_source(L, F, P, D, dtype, index, layout, seed, extra_rows=()):
    """-> (buffers, k view, v view) on the host: NaN everywhere but in the K and V rows that `index` (and `extra_rows`) names."""
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(L, F, P, D, generator=g).to(dtype) for _ in range(2)]
    named = torch.zeros(L, P, dtype=torch.bool)
    for l in range(L):
        named[l, index[l].long().clamp(0, P - 1)] = True
        named[l, list(extra_rows)] = True
    mask = named[:, None, :, None].expand(L, F, P, D)
    if layout == "in_place":
        buf = torch.full((L, F, P + 1, 3 * D), NAN, dtype=dtype)
        bufs, k, v = [buf], buf[:, :, 1:, D:2 * D], buf[:, :, 1:, 2 * D:]
    else:
        bufs = [torch.full((L, F * P, D), NAN, dtype=dtype) for _ in range(2)]
        k, v = (b.view(L, F, P, D) for b in bufs)
    k[mask], v[mask] = vals[0][mask], vals[1][mask]
    return bufs, k, v


def make_pos(T, D, dtype, seed):
    pos = torch.randn(T, D, generator=torch.Generator().manual_seed(seed)) * 1.37
    pos[0, 0] = 1.0 + 2.0 ** -8  # a tie in bf16: rounds to 1 before the add
    if dtype == torch.bfloat16:
        assert (pos.bfloat16().float() != pos).any()
    return pos


def run(L, F, T, P, S, D, dtype, layout, with_pos, seed=0, index=None, raw=False, offset=0):
    """One guarded call -> (k_out, v_out, path, reference pair).  `raw`: through the C entry point, not `capi.kv_gather_patches`
    (a table with entries outside [0, P) only gets that far).  `offset`: the source starts that many elements into a plain
    allocation (no guards around it then)."""
    index = table(L, P, S, seed) if index is None else index
    bufs, hk, hv = host_source(L, F, P, D, dtype, index, layout, seed, extra_rows=(0, P - 1) if raw else ())
    pos = make_pos(T, D, dtype, seed + 1) if with_pos else None
    want = gather_reference(hk, hv, index.clamp(0, P - 1), pos, T)
    assert torch.isfinite(want[0].float()).all() and torch.isfinite(want[1].float()).all()
    guards = []
    if offset:
        dev = [torch.full((b.numel() + 16,), NAN, dtype=dtype, device="cuda") for b in bufs]
        for d, b in zip(dev, bufs):
            d[offset:offset + b.numel()] = b.reshape(-1).cuda()
        dev = [d[offset:offset + b.numel()].view(b.shape) for d, b in zip(dev, bufs)]
    else:
        guards = [guarded(b.numel() // b.shape[-1], b.shape[-1], dtype, name=f"source {i}").set(b) for i, b in enumerate(bufs)]
        dev = [g.shaped(*b.shape) for g, b in zip(guards, bufs)]
    if layout == "in_place":
        dk, dv = dev[0][:, :, 1:, D:2 * D], dev[0][:, :, 1:, 2 * D:]
    else:
        dk, dv = dev
    gi = guarded_1d(L * S * 4, torch.uint8, fill=255, name="index").set(index.view(torch.uint8))
    di = gi.shaped(L * S * 4).view(torch.int32).view(L, S)
    gk, gv = (guarded(L * F * S, D, dtype, name=n) for n in ("k_out", "v_out"))
    ko, vo = gk.shaped(L, F * S, D), gv.shaped(L, F * S, D)
    dpos = pos.cuda() if with_pos else None
    if raw:
        s = (dk.stride(0), dk.stride(1), dk.stride(2)) if layout == "in_place" else (F * P * D, P * D, D)
        rc = capi.load_library().dfd_kv_gather_patches(dk.data_ptr(), dv.data_ptr(), capi._DTYPE[dtype], *s, di.data_ptr(),
                                                       dpos.data_ptr() if with_pos else None, ko.data_ptr(), vo.data_ptr(), L, F, T, P, S,
                                                       D, capi._stream())
        assert rc == 0, capi.load_library().dfd_last_error().decode()
    elif layout == "in_place":
        capi.kv_gather_patches(dk, dv, di, dpos, ko, vo, T=T, index_host=index)
    else:
        capi.kv_gather_patches(dk, dv, di, dpos, ko, vo, T=T, P=P)  # (no host copy given: the binding reads the table back)
    path = capi.kv_gather_last_path()
    torch.cuda.synchronize()
    for g in guards + [gi]:
        g.assert_untouched(view_too=True)
    gk.assert_untouched(), gv.assert_untouched()
    assert torch.isfinite(ko.float()).all() and torch.isfinite(vo.float()).all(), "a byte outside the named rows was read"
    return ko.clone(), vo.clone(), path, want


def expect_path(D, dtype):
    return capi.KVGATHER_VEC16 if D % VEC[dtype] == 0 else capi.KVGATHER_ELEMENT


@pytest.mark.parametrize("layout", ["in_place", "dense"])
@pytest.mark.parametrize("n,width", list(enumerate(WIDTHS)), ids=[f"D{d}-{str(t)[6:]}" for d, t in WIDTHS])
@pytest.mark.parametrize("P,S", GEOMETRIES)
def test_every_width_and_form_matches_the_reference(layout, n, width, P, S):
    D, dtype = width
    L = 1 + (n + S) % 2
    F, T = BATCHES[(n + P + S) % 3]
    with_pos = (n + S + (layout == "dense")) % 2 == 0
    ko, vo, path, want = run(L, F, T, P, S, D, dtype, layout, with_pos, seed=100 * n + 10 * P + S)
    assert path == expect_path(D, dtype), (path, D, dtype)
    assert same(ko, want[0]) and same(vo, want[1])


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("F,T", BATCHES)
@pytest.mark.parametrize("L", [1, 2])
@pytest.mark.parametrize("P,S", GEOMETRIES)
def test_every_geometry_at_the_tiny_width(with_pos, F, T, L, P, S):
    """D = 128 in bf16 puts 16 rows into a block: L * F * S rows from 3 to 60 are mostly no multiple of it, and from 17 rows
    on there is more than one block per layer."""
    ko, vo, path, want = run(L, F, T, P, S, 128, torch.bfloat16, "in_place", with_pos, seed=7 * F + P + S + L)
    assert path == capi.KVGATHER_VEC16
    assert same(ko, want[0]) and same(vo, want[1])


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float32, 100), (torch.bfloat16, 768)])
@pytest.mark.parametrize("layout", ["in_place", "dense"])
@pytest.mark.parametrize("with_pos", [False, True])
def test_both_forms_are_bit_identical(dtype, D, layout, with_pos):
    """The same operands from a 16-byte aligned base (16-byte form) and from a base one element off (element by element)."""
    a = run(2, 6, 3, 9, 5, D, dtype, layout, with_pos, seed=31)
    b = run(2, 6, 3, 9, 5, D, dtype, layout, with_pos, seed=31, offset=1)
    assert a[2] == capi.KVGATHER_VEC16 and b[2] == capi.KVGATHER_ELEMENT
    assert same(a[0], b[0]) and same(a[1], b[1]) and same(a[0], a[3][0]) and same(b[1], b[3][1])


def test_pos_none_and_pos_of_one_frame():
    for with_pos in (False, True):
        ko, vo, path, want = run(2, 5, 1, 4, 2, 128, torch.bfloat16, "in_place", with_pos, seed=5)  # T = 1: one row for all frames
        assert same(ko, want[0]) and same(vo, want[1])


def test_pos_is_rounded_before_the_add():
    """bf16 source 2^-8, pos 1 + 2^-8: rounded first pos is 1 and the sum ties back to 1; one rounding of the f32 sum would
    give 1.0078125.  In both forms."""
    for off in (0, 1):
        src = torch.full((1, 3, 4, 16 + off), 2.0 ** -8, dtype=torch.bfloat16, device="cuda")[..., off:]
        pos = torch.full((3, 16), 1.0 + 2.0 ** -8, device="cuda")
        idx = torch.tensor([[2, 0]], dtype=torch.int32, device="cuda")
        ko, vo = capi.kv_gather_patches(src, src, idx, pos, T=3)
        assert capi.kv_gather_last_path() == (capi.KVGATHER_ELEMENT if off else capi.KVGATHER_VEC16)
        assert (ko.float() == 1.0).all() and (vo.float() == 1.0).all()
        want = gather_reference(src.cpu(), src.cpu(), idx.cpu(), pos.cpu(), 3)
        assert same(ko, want[0])


@pytest.mark.parametrize("layout", ["in_place", "dense"])
@pytest.mark.parametrize("D", [128, 66])
def test_a_bad_table_is_refused_by_the_binding_and_clamped_by_the_kernel(layout, D):
    L, F, T, P, S = 2, 6, 3, 9, 5
    index = table(L, P, S, 3)
    index[0, 1], index[1, 3] = P, -1
    src = torch.zeros(L, F, P, D, dtype=torch.bfloat16, device="cuda")
    with pytest.raises(capi.DfdError, match="outside"):
        capi.kv_gather_patches(src, src, index.cuda(), None, T=T, index_host=index)
    with pytest.raises(capi.DfdError, match="outside"):
        capi.kv_gather_patches(src, src, index.cuda(), None, T=T)  # ... and when it has to read the table back itself
    ko, vo, path, want = run(L, F, T, P, S, D, torch.bfloat16, layout, True, seed=3, index=index, raw=True)
    assert same(ko, want[0]) and same(vo, want[1])  # (`want` is the reference on the clamped table)


def test_a_layer_stride_beyond_two_to_the_31_elements():
    """bf16, L = 2, layer stride 2^31 + 64 elements: a 32-bit offset would wrap into layer 0.  One uninitialised byte buffer;
    only the rows that are read get written."""
    L, F, T, P, S, D = 2, 3, 3, 4, 2, 128
    sl = 2 ** 31 + 64
    raw = torch.empty(2 * L * sl, dtype=torch.uint8, device="cuda")
    flat = raw.view(torch.bfloat16)
    k = flat.as_strided((L, F, P, D), (sl, (P + 1) * 3 * D, 3 * D, 1), (3 + 1) * D)
    v = flat.as_strided((L, F, P, D), (sl, (P + 1) * 3 * D, 3 * D, 1), (3 + 2) * D)
    index = torch.tensor([[3, 1], [0, 2]], dtype=torch.int32)
    g = torch.Generator().manual_seed(9)
    hk, hv = (torch.randn(L, F, P, D, generator=g).bfloat16() for _ in range(2))
    for l in range(L):
        rows = index[l].long().cuda()
        k[l, :, rows] = hk[l, :, index[l].long()].cuda()
        v[l, :, rows] = hv[l, :, index[l].long()].cuda()
    hk[0, :, [0, 2]], hk[1, :, [1, 3]] = NAN, NAN  # (the reference must not need the other rows either)
    pos = make_pos(T, D, torch.bfloat16, 2)
    gk, gv = (guarded(L * F * S, D, torch.bfloat16, name=n) for n in ("k_out", "v_out"))
    capi.kv_gather_patches(k, v, index.cuda(), pos.cuda(), gk.shaped(L, F * S, D), gv.shaped(L, F * S, D), T=T, index_host=index)
    assert capi.kv_gather_last_path() == capi.KVGATHER_VEC16
    gk.assert_untouched(), gv.assert_untouched()
    want = gather_reference(hk, hv, index, pos, T)
    assert same(gk.shaped(L, F * S, D), want[0]) and same(gv.shaped(L, F * S, D), want[1])
    assert torch.isfinite(want[0].float()).all()


def test_stream_policy_does_not_change_a_bit():
    before = capi.stream_policy_get()
    try:
        outs = []
        for mask in (0, 1):
            capi.stream_policy_set(mask)
            for D, dtype in ((768, torch.bfloat16), (66, torch.bfloat16)):
                outs.append(run(2, 6, 3, 9, 5, D, dtype, "in_place", True, seed=13))
    finally:
        capi.stream_policy_set(before)
    for a, b in zip(outs[:2], outs[2:]):
        assert a[2] == b[2] and same(a[0], b[0]) and same(a[1], b[1]) and same(a[0], a[3][0]) and same(a[1], a[3][1])


def test_refusals_and_no_ops_on_the_device():
    k = torch.zeros(2, 4, 9, 64, dtype=torch.bfloat16, device="cuda")
    idx = torch.zeros(2, 5, dtype=torch.int32, device="cuda")
    lib = capi.load_library()

    def call(**over):
        a = dict(k=k.data_ptr(), v=k.data_ptr(), dtype=capi.BF16, sl=4 * 9 * 64, sf=9 * 64, sp=64, index=idx.data_ptr(), pos=None,
                 ko=k.data_ptr(), vo=k.data_ptr(), L=2, F=4, T=2, P=9, S=5, D=64)
        a.update(over)
        rc = lib.dfd_kv_gather_patches(a["k"], a["v"], a["dtype"], a["sl"], a["sf"], a["sp"], a["index"], a["pos"], a["ko"], a["vo"],
                                       a["L"], a["F"], a["T"], a["P"], a["S"], a["D"], capi._stream())
        return rc, lib.dfd_last_error().decode()

    for over in (dict(k=None), dict(dtype=capi.FP8), dict(S=10), dict(S=-1), dict(T=0), dict(T=3), dict(sp=63), dict(L=65536)):
        rc, msg = call(**over)
        assert rc == -1 and "dfd_kv_gather_patches" in msg, (over, rc, msg)
    for over in (dict(L=0), dict(F=0), dict(S=0)):
        assert call(**over)[0] == 0 and capi.kv_gather_last_path() == 0
    torch.cuda.synchronize()
    assert (k == 0).all()
    empty = capi.kv_gather_patches(k, k, idx[:, :0].contiguous(), None, T=2)
    assert tuple(empty[0].shape) == (2, 0, 64)
    with pytest.raises(AssertionError):
        capi.kv_gather_patches(k, k.float(), idx, None, T=2)  # all four tensors share one type
