"""GPU parity of dfd_kv_move_frames (include/dfdclip_kvframes.h, csrc/kv_frames.hip) against `stream.move_reference` on the
same operands, BIT FOR BIT: the kernel only moves rows, so there is no tolerance.

Every case keeps its source and both outputs between poisoned guards (tests/guarded.py).  Of the source, only the frames
that the table names hold numbers: CLS rows, the Q third, frames that are not named and all padding are NaN, so a load from
anywhere else shows in the result.  The outputs start as poison and are compared WHOLE with the reference applied to the
same poison: a destination frame that is not named keeps it.  Shapes are the smallest at which the kernel can go wrong:
row counts that are no multiple of the rows per block, several blocks, D on both sides of the 16-byte rule, tables that
reverse, repeat and wrap, and one layer stride beyond 2^31 elements."""
import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.stream import move_reference
from tests.guarded import guarded

pytestmark = pytest.mark.gpu

NAN = float("nan")
VEC = {torch.float32: 4, torch.bfloat16: 8}
WIDTHS = [(128, torch.bfloat16), (128, torch.float32), (12, torch.bfloat16), (20, torch.bfloat16), (7, torch.float32), (768, torch.bfloat16)]


def bits(t):
    return t.contiguous().view(torch.uint8)


def same(a, b):
    return torch.equal(bits(a.cpu()), bits(b.cpu()))


def i32(x):
    return None if x is None else torch.as_tensor(np.asarray(x), dtype=torch.int32)


def host_source(L, F, P, D, dtype, named, layout, seed):
    """-> (buffer list, k view, v view) on the host: NaN everywhere but in the K and V rows of the frames in `named`."""
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(L, F, P, D, generator=g).to(dtype) for _ in range(2)]
    if layout == "in_place":
        buf = torch.full((L, F, P + 1, 3 * D), NAN, dtype=dtype)
        bufs, k, v = [buf], buf[:, :, 1:, D:2 * D], buf[:, :, 1:, 2 * D:]
    else:
        bufs = [torch.full((L, F, P, D), NAN, dtype=dtype) for _ in range(2)]
        k, v = bufs
    for f in sorted(set(int(x) for x in named)):
        k[:, f], v[:, f] = vals[0][:, f], vals[1][:, f]
    return bufs, k, v


def run(L, P, D, dtype, src_layout, dst_layout, src_frames, dst_frames, src=None, dst=None, n=None, seed=0, offset=0, raw=False,
        src_once=False):
    """One guarded call -> (k_out, v_out, path, reference pair).  `src` / `dst`: the tables (None = identity).  `dst_layout`:
    "dense" (contiguous) or "padded" (dst_stride_patch = D + 8).  `raw`: through the C entry point, not `capi.kv_move_frames` (a
    table with entries outside its side only gets that far).  `offset`: the source starts that many elements into a plain
    allocation (no guards around it then)."""
    src, dst = i32(src), i32(dst)
    n = n if n is not None else (len(src) if src is not None else (len(dst) if dst is not None else src_frames))
    s_eff = (torch.arange(n) if src is None else src.long()).clamp(0, src_frames - 1)
    d_eff = (torch.arange(n) if dst is None else dst.long()).clamp(0, dst_frames - 1)
    bufs, hk, hv = host_source(L, src_frames, P, D, dtype, s_eff.tolist(), src_layout, seed)
    guards = []
    if offset:
        dev = [torch.full((b.numel() + 16,), NAN, dtype=dtype, device="cuda") for b in bufs]
        for d_, b in zip(dev, bufs):
            d_[offset:offset + b.numel()] = b.reshape(-1).cuda()
        dev = [d_[offset:offset + b.numel()].view(b.shape) for d_, b in zip(dev, bufs)]
    else:
        guards = [guarded(b.numel() // b.shape[-1], b.shape[-1], dtype, name=f"source {i}").set(b) for i, b in enumerate(bufs)]
        dev = [g.shaped(*b.shape) for g, b in zip(guards, bufs)]
    if src_layout == "in_place":
        dk, dv = dev[0][:, :, 1:, D:2 * D], dev[0][:, :, 1:, 2 * D:]
    else:
        dk, dv = dev
    ld = D + 8 if dst_layout == "padded" else D
    gk, gv = (guarded(L * dst_frames * P, D, dtype, ld=ld, name=nm) for nm in ("k_out", "v_out"))
    ko, vo = (g.t.unflatten(0, (L, dst_frames, P)) for g in (gk, gv))
    assert ko.stride() == (dst_frames * P * ld, P * ld, ld, 1)
    want = move_reference(hk, hv, s_eff, d_eff, ko.cpu().clone(), vo.cpu().clone())  # on the poison the outputs start as
    for w in want:
        assert torch.isfinite(w[:, d_eff].float()).all()
    ds, dd = (None if t is None else t.cuda() for t in (src, dst))
    if raw:
        rc = capi.load_library().dfd_kv_move_frames(dk.data_ptr(), dv.data_ptr(), ko.data_ptr(), vo.data_ptr(), capi._DTYPE[dtype],
                                                    dk.stride(0), dk.stride(1), dk.stride(2), ko.stride(0), ko.stride(1), ko.stride(2),
                                                    None if ds is None else ds.data_ptr(), None if dd is None else dd.data_ptr(),
                                                    L, n, src_frames, dst_frames, P, D, int(src_once), capi._stream())
        assert rc == 0, capi.load_library().dfd_last_error().decode()
    else:
        capi.kv_move_frames(dk, dv, ko, vo, ds, dd, src_once=src_once, src_host=src, dst_host=dst)
    path = capi.kv_move_last_path()
    torch.cuda.synchronize()
    for g in guards:
        g.assert_untouched(view_too=True)
    gk.assert_untouched(), gv.assert_untouched()
    return ko.clone(), vo.clone(), path, want


def check(out):
    ko, vo, _, want = out
    assert same(ko, want[0]) and same(vo, want[1])
    return out


def expect_path(D, dtype):
    return capi.KVFRAMES_VEC16 if D % VEC[dtype] == 0 else capi.KVFRAMES_ELEMENT


def ring(a, n, capacity):
    return [(a + i) % capacity for i in range(n)]


@pytest.mark.parametrize("use", ["ingest", "gather"])
@pytest.mark.parametrize("i,width", list(enumerate(WIDTHS)), ids=[f"D{d}-{str(t)[6:]}" for d, t in WIDTHS])
@pytest.mark.parametrize("L,P,n", [(1, 4, 1), (2, 3, 5), (2, 1, 9), (1, 4, 9), (2, 4, 5)])
def test_every_width_and_form_in_both_uses(use, i, width, L, P, n):
    """Ingest: in-place q|k|v views -> ring slots of a store with capacity > n (a wrap where n allows one).  Gather: a dense
    store -> a dense buffer through a table with repeated entries (overlapping windows)."""
    D, dtype = width
    seed = 100 * i + 10 * P + n
    if use == "ingest":
        cap = n + 3
        out = run(L, P, D, dtype, "in_place", "dense", n, cap, dst=ring(cap - 2, n, cap), seed=seed, src_once=True)
    else:
        cap = 7
        windows = [(w + j) % cap for w in range(n // 2 + 1) for j in range(2)][:n]  # hop 1, T 2: every frame but the ends twice
        out = run(L, P, D, dtype, "dense", "dense", cap, n, src=windows, seed=seed)
    assert out[2] == expect_path(D, dtype), (out[2], D, dtype)
    check(out)


@pytest.mark.parametrize("src_layout", ["in_place", "dense"])
@pytest.mark.parametrize("dst_layout", ["dense", "padded"])
@pytest.mark.parametrize("tables", ["identity", "reversed", "repeated-src", "both", "wrap"])
@pytest.mark.parametrize("D,dtype", [(128, torch.bfloat16), (20, torch.bfloat16), (7, torch.float32)])
def test_layouts_and_tables(src_layout, dst_layout, tables, D, dtype):
    """L = 2, P = 3 with D = 128 bf16 puts 16 rows into a block: 5 frames are 15 rows, 9 frames 27 (two blocks, the second ragged)."""
    L, P = 2, 3
    if tables == "identity":
        out = run(L, P, D, dtype, src_layout, dst_layout, 5, 5, seed=1)
    elif tables == "reversed":
        out = run(L, P, D, dtype, src_layout, dst_layout, 9, 9, src=list(range(9))[::-1], seed=2)
    elif tables == "repeated-src":
        out = run(L, P, D, dtype, src_layout, dst_layout, 6, 9, src=[0, 1, 2, 1, 2, 3, 2, 3, 4], seed=3)
    elif tables == "both":
        out = run(L, P, D, dtype, src_layout, dst_layout, 6, 11, src=[4, 4, 0, 5, 2], dst=[10, 0, 7, 3, 8], seed=4)
    else:
        out = run(L, P, D, dtype, src_layout, dst_layout, 9, 11, dst=ring(7, 9, 11), seed=5, src_once=True)
    want_path = capi.KVFRAMES_VEC16 if D % VEC[dtype] == 0 else capi.KVFRAMES_ELEMENT
    assert out[2] == want_path  # (the padding of 8 elements keeps every stride a multiple of 16 bytes)
    check(out)


@pytest.mark.parametrize("dtype,D", [(torch.bfloat16, 128), (torch.float32, 128), (torch.bfloat16, 768)])
@pytest.mark.parametrize("src_layout", ["in_place", "dense"])
def test_both_forms_are_bit_identical(dtype, D, src_layout):
    """The same operands from a 16-byte aligned base (16-byte form) and from a base one element off (element by element)."""
    kw = dict(src=[3, 0, 4, 4, 1], dst=[1, 6, 2, 0, 5], seed=31)
    a = run(2, 3, D, dtype, src_layout, "padded", 5, 7, **kw)
    b = run(2, 3, D, dtype, src_layout, "padded", 5, 7, offset=1, **kw)
    assert a[2] == capi.KVFRAMES_VEC16 and b[2] == capi.KVFRAMES_ELEMENT
    check(a), check(b)
    assert same(a[0], b[0]) and same(a[1], b[1])


@pytest.mark.parametrize("D", [128, 20])
def test_bad_tables_are_refused_by_the_binding_and_clamped_by_the_kernel(D):
    L, P, Fs, Fd = 2, 3, 5, 7
    k = torch.zeros(L, Fs, P, D, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(L, Fd, P, D, dtype=torch.bfloat16, device="cuda")
    bad_src, bad_dst, twice = i32([0, Fs, 2]), i32([1, -1, 3]), i32([1, 4, 1])
    ok = i32([0, 1, 2])
    with pytest.raises(capi.DfdError, match="src_frame has an entry outside"):
        capi.kv_move_frames(k, k, o, o.clone(), bad_src.cuda(), ok.cuda(), src_host=bad_src, dst_host=ok)
    with pytest.raises(capi.DfdError, match="dst_frame has an entry outside"):
        capi.kv_move_frames(k, k, o, o.clone(), ok.cuda(), bad_dst.cuda())  # ... and when it has to read the tables back itself
    with pytest.raises(capi.DfdError, match="twice"):
        capi.kv_move_frames(k, k, o, o.clone(), ok.cuda(), twice.cuda(), dst_host=twice)
    with pytest.raises(capi.DfdError, match="identity"):
        capi.kv_move_frames(k[:, :2], k[:, :2], o, o.clone(), None, ok.cuda(), dst_host=ok)
    torch.cuda.synchronize()
    assert (o == 0).all()
    # raw: -3 -> 0 and Fs + 2 -> Fs - 1 on the source side, Fd -> Fd - 1 and -1 -> 0 on the destination side (distinct after the clamp)
    check(run(L, P, D, torch.bfloat16, "in_place", "padded", Fs, Fd, src=[-3, Fs + 2, 2, 1], dst=[Fd, -1, 3, 4], seed=6, raw=True))


def test_a_layer_stride_beyond_two_to_the_31_elements():
    """bf16, L = 2, layer stride 2^31 + 64 elements on the SOURCE (in-place views) and on the DESTINATION (a store): a 32-bit
    offset would wrap into layer 0.  One uninitialised byte buffer each; only the rows that are read get written first."""
    L, P, D, Fs, Fd = 2, 4, 128, 3, 5
    sl = 2 ** 31 + 64
    g = torch.Generator().manual_seed(9)
    hk, hv = (torch.randn(L, Fs, P, D, generator=g).bfloat16() for _ in range(2))
    src, dst = i32([2, 0, 2]), i32([4, 1, 0])
    # source far apart, destination guarded and dense
    flat = torch.empty(2 * L * sl, dtype=torch.uint8, device="cuda").view(torch.bfloat16)
    k = flat.as_strided((L, Fs, P, D), (sl, (P + 1) * 3 * D, 3 * D, 1), (3 + 1) * D)
    v = flat.as_strided((L, Fs, P, D), (sl, (P + 1) * 3 * D, 3 * D, 1), (3 + 2) * D)
    k.copy_(hk.cuda()), v.copy_(hv.cuda())
    gk, gv = (guarded(L * Fd * P, D, torch.bfloat16, name=n) for n in ("k_out", "v_out"))
    ko, vo = gk.shaped(L, Fd, P, D), gv.shaped(L, Fd, P, D)
    want = move_reference(hk, hv, src, dst, ko.cpu().clone(), vo.cpu().clone())
    capi.kv_move_frames(k, v, ko, vo, src.cuda(), dst.cuda(), src_host=src, dst_host=dst)
    assert capi.kv_move_last_path() == capi.KVFRAMES_VEC16
    gk.assert_untouched(), gv.assert_untouched()
    assert same(ko, want[0]) and same(vo, want[1])
    # destination far apart (the same allocation, now the store), source dense
    del k, v
    sk = flat.as_strided((L, Fd, P, D), (sl, P * D, D, 1), 0)
    sv = flat.as_strided((L, Fd, P, D), (sl, P * D, D, 1), Fd * P * D)
    sk.fill_(NAN), sv.fill_(NAN)
    want = move_reference(hk, hv, src, dst, sk.cpu().clone(), sv.cpu().clone())
    capi.kv_move_frames(hk.cuda(), hv.cuda(), sk, sv, src.cuda(), dst.cuda(), src_once=True, src_host=src, dst_host=dst)
    assert capi.kv_move_last_path() == capi.KVFRAMES_VEC16
    torch.cuda.synchronize()
    assert same(sk, want[0]) and same(sv, want[1])
    assert torch.isfinite(sk[1, 4].float()).all() and not torch.isfinite(sk[1, 2].float()).any()


def test_stream_policy_does_not_change_a_bit():
    before = capi.stream_policy_get()
    try:
        outs = []
        for mask in (0, capi.STREAM_DECODER_KV):
            capi.stream_policy_set(mask)
            for once in (False, True):
                for D, dtype in ((768, torch.bfloat16), (20, torch.bfloat16)):
                    outs.append(check(run(2, 3, D, dtype, "in_place", "padded", 6, 9, src=[5, 1, 1, 0, 3], dst=[8, 2, 0, 5, 4], seed=13,
                                          src_once=once)))
    finally:
        capi.stream_policy_set(before)
    for o in outs[1:]:
        ref = outs[0] if o[0].shape == outs[0][0].shape else outs[1]
        assert same(o[0], ref[0]) and same(o[1], ref[1])


def test_refusals_and_no_ops_on_the_device():
    k = torch.zeros(2, 4, 9, 64, dtype=torch.bfloat16, device="cuda")
    o = torch.zeros(2, 6, 9, 64, dtype=torch.bfloat16, device="cuda")
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    lib = capi.load_library()

    def call(**over):
        a = dict(k=k.data_ptr(), v=k.data_ptr(), ko=o.data_ptr(), vo=o.data_ptr(), dtype=capi.BF16, ssl=4 * 9 * 64, ssf=9 * 64, ssp=64,
                 dsl=6 * 9 * 64, dsf=9 * 64, dsp=64, src=idx.data_ptr(), dst=None, L=2, n=4, Fs=4, Fd=6, P=9, D=64, flags=0)
        a.update(over)
        rc = lib.dfd_kv_move_frames(a["k"], a["v"], a["ko"], a["vo"], a["dtype"], a["ssl"], a["ssf"], a["ssp"], a["dsl"], a["dsf"], a["dsp"],
                                    a["src"], a["dst"], a["L"], a["n"], a["Fs"], a["Fd"], a["P"], a["D"], a["flags"], capi._stream())
        return rc, lib.dfd_last_error().decode()

    for over in (dict(k=None), dict(vo=None), dict(dtype=capi.FP8), dict(n=-1), dict(ssp=63), dict(dsp=63), dict(dsf=-1), dict(L=65536),
                 dict(Fs=0), dict(Fd=0), dict(flags=2), dict(n=1 << 29, P=8), dict(n=7)):
        rc, msg = call(**over)
        assert rc == -1 and "dfd_kv_move_frames" in msg, (over, rc, msg)
        assert capi.kv_move_last_path() == 0
    for over in (dict(L=0), dict(n=0), dict(P=0), dict(n=0, Fs=0, Fd=0)):
        assert call(**over)[0] == 0 and capi.kv_move_last_path() == 0
    torch.cuda.synchronize()
    assert (o == 0).all()
    empty = capi.kv_move_frames(k, k, o, o.clone(), idx[:0], None)
    assert empty[0] is o
    with pytest.raises(AssertionError):
        capi.kv_move_frames(k, k.float(), o, o, idx, None)  # all four tensors share one type
    torch.cuda.synchronize()
    assert (o == 0).all()
