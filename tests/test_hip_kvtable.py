"""Decoder attention over a frame store through the C ABI (include/dfdclip_kvtable.h: dfd_decoder_attn_fwd_frames /
dfd_decoder_attn_map_frames), with guard bands (tests/guarded.py) round mix, mix_softmax, stats, the workspace, aff and the
branches.

Two bars.  BIT IDENTITY with the untabled entry points run on `stream.table_reference` of the same store, under the same
layout strides, splits and pos: a derived bar, not a measured one — the same rows pass through the same arithmetic in the
same order, only their addresses differ.  And the ABSOLUTE bars of tests/decoder_edge_cases.py against its float64
restatement on the named rows.

Every frame of the store that no table entry names is NaN (in the in-place view the q third and the class-token rows as
well), so a row read from a wrong address poisons the result.  Per shape and dtype, every table x store layout x pos runs
every split count; the padding deals of `deals(B, T)` rotate over those combinations so that each is used."""
import ctypes

import pytest
import torch

from dfd_clip_amd.stream import table_reference
from tests import decoder_edge_cases as dec
from tests.attnmap_cases import KERNEL_ATOL, KERNEL_RTOL
from tests.decoder_edge_cases import BARS, deals, policy_splits, restate, rnd
from tests.guarded import guarded, guarded_1d, guarded_bytes

pytestmark = pytest.mark.gpu

# the first four: tests/decoder_edge_cases.py SHAPES; (2, 3, 5, 18): 576 threads, the only way into the 1024-thread form
SHAPES = [(2, 1, 1, 1), (3, 3, 5, 4), (2, 5, 7, 3), (4, 7, 20, 12), (2, 3, 5, 18)]
DTYPES = [torch.float32, torch.bfloat16]
TABLES = ("identity", "reversed", "wrapped", "overlapping", "one_frame")
NAN = float("nan")


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    assert c.load_library().dfd_device_check() == 0, c.load_library().dfd_last_error()
    return c


def make_table(name, B, T, C):
    """int32 [B*T]: the store frame of (clip b, frame tf), a = b*T + tf"""
    b = torch.arange(B).view(B, 1).expand(B, T)
    tf = torch.arange(T).view(1, T).expand(B, T)
    a = b * T + tf
    t = {"identity": a, "reversed": B * T - 1 - a, "wrapped": (a + C - 2) % C,  # a window crosses the ring's end
         "overlapping": b + tf,                                                  # window b starts at frame b
         "one_frame": (2 * b + 1) % C + 0 * tf}[name]                           # one frame named T times
    return t.reshape(-1).to(torch.int32)


def straddling_splits(S, P):
    """the smallest split count under which one workgroup's rows [s*per, (s+1)*per) lie in two frames, or None (T == 1)"""
    for splits in range(2, S + 1):
        per = (S + splits - 1) // splits
        if any(s * per < S and (s * per) // P != (min(S, (s + 1) * per) - 1) // P for s in range(splits)):
            return splits
    return None


def splits_of(B, S, P):
    out = []
    for s in (1, policy_splits(B, S), S + 1, straddling_splits(S, P)):  # S + 1: empty workgroups
        if s is not None and s not in out:
            out.append(s)
    return out


def make_store(C, P, D, dtype, named, view, seed):
    """One layer of a store: (k, v) [C, P, D] on the device, dense or as the in-place view of a [C, P + 1, 3D] buffer (row
    stride 3D, frame stride tokens*3D); frames outside `named` are NaN, and so is everything of the buffer that is no K or
    V row.  Also the host copies."""
    hk, hv = rnd(C, P, D, seed=seed).to(dtype), rnd(C, P, D, seed=seed + 1).to(dtype)
    dead = torch.ones(C, dtype=torch.bool)
    dead[torch.as_tensor(sorted(named), dtype=torch.long)] = False
    hk[dead], hv[dead] = NAN, NAN
    if not view:
        return hk.cuda(), hv.cuda(), hk, hv
    whole = torch.full((C, P + 1, 3 * D), NAN, dtype=dtype)
    whole[:, 1:, D:2 * D], whole[:, 1:, 2 * D:] = hk, hv
    whole = whole.cuda()
    k, v = whole[:, 1:, D:2 * D], whole[:, 1:, 2 * D:]
    assert k.stride() == ((P + 1) * 3 * D, 3 * D, 1) and not k.is_contiguous()
    return k, v, hk, hv


def as_layout(rows, P, D, view):
    """the dense [n, P, D] reference rows under the store's strides: as they are, or inside a [n, P + 1, 3D] buffer"""
    if not view:
        return rows
    whole = torch.full((rows.shape[0], P + 1, 3 * D), NAN, dtype=rows.dtype, device=rows.device)
    whole[:, 1:, D:2 * D] = rows
    return whole[:, 1:, D:2 * D]


class Out:
    """guarded outputs of one forward + map"""

    def __init__(self, capi, B, T, P, H, splits):
        S, D = T * P, H * 64
        self.mix, self.mix_s = guarded(B, D, torch.float32, name="mix"), guarded(B, D, torch.float32, name="mix_softmax")
        self.stats = guarded_1d(B * H * 2, torch.float32, name="stats")
        self.ws = guarded_bytes(capi.decoder_attn_workspace_bytes(B, H, 64, splits), name="workspace")
        self.aff = guarded_1d(B * H * S, torch.float32, name="aff")
        self.br = guarded_1d(2 * B * H * S, torch.float32, name="branches")
        self.B, self.H, self.S = B, H, S

    def tensors(self):
        B, H, S = self.B, self.H, self.S
        return self.mix.t, self.mix_s.t, self.stats.shaped(B, H, 2), self.aff.shaped(B, H, S), self.br.shaped(2, B, H, S)

    def untouched(self):
        for g in (self.mix, self.mix_s, self.stats, self.ws, self.aff, self.br):
            g.assert_untouched()


def bits(t):
    return t.contiguous().view(torch.int32)


def run_tabled(capi, q, k, v, table, m, splits, shape, pos, table_host=None):
    B, T, P, H = shape
    o = Out(capi, B, T, P, H, splits)
    mix, mix_s, stats, aff, br = o.tensors()
    capi.decoder_attn_fwd_frames(q, k, v, table, m, mix, stats, o.ws.t, splits, B, T, P, H, mix_softmax=mix_s, pos=pos, table_host=table_host)
    capi.decoder_attn_map_frames(q, k, table, m, stats, aff, B, T, P, H, branches=br, pos=pos, table_host=table_host)
    o.untouched()
    return dict(mix=mix, mix_softmax=mix_s, stats=stats, aff=aff, branches=br)


def run_plain(capi, q, k, v, m, splits, shape, pos):
    B, T, P, H = shape
    o = Out(capi, B, T, P, H, splits)
    mix, mix_s, stats, aff, br = o.tensors()
    capi.decoder_attn_fwd(q, k, v, m, mix, stats, o.ws.t, splits, B, T, P, H, mix_softmax=mix_s, pos=pos)
    capi.decoder_attn_map(q, k, m, stats, aff, B, T, P, H, branches=br, pos=pos)
    o.untouched()
    return dict(mix=mix, mix_softmax=mix_s, stats=stats, aff=aff, branches=br)


def assert_same(got, want, case):
    for n in want:
        assert got[n].shape == want[n].shape and torch.equal(bits(got[n]), bits(want[n])), f"{n} {case}: the tabled bits differ from the untabled ones"


def hold(name, got, want, atol, rtol, case, worst):
    err, over = dec.worst(got, want, atol, rtol)
    worst[name] = max(worst.get(name, 0.0), err)
    assert over <= 0, f"{name} {case}: worst error {err:.3e} exceeds atol {atol:.1e} + rtol {rtol:.1e}"


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_tabled_equals_untabled_on_the_named_rows(capi, shape, dtype):
    B, T, P, H = shape
    S, D, C = T * P, H * 64, B * T + 3
    q_host = rnd(B, H, 2 * 64, seed=3)
    q = q_host.reshape(B, -1).cuda()
    pos_host = rnd(T, D, seed=52, scale=0.3)
    all_deals = deals(B, T)
    splits_list = splits_of(B, S, P)
    if T > 1:
        st = straddling_splits(S, P)
        per = (S + st - 1) // st
        assert st in splits_list and any((s * per) // P != (min(S, (s + 1) * per) - 1) // P for s in range(st) if s * per < S)
    used, worst, combo = set(), {}, 0
    for ti, tname in enumerate(TABLES):
        table_host = make_table(tname, B, T, C)
        assert int(table_host.min()) >= 0 and int(table_host.max()) < C
        table = table_host.cuda()
        for view in (False, True):
            k, v, hk, hv = make_store(C, P, D, dtype, set(table_host.tolist()), view, seed=10 + ti)
            rk, rv = table_reference(k, v, table_host)
            assert rk.shape == (B * T, P, D) and torch.isfinite(rk.float()).all() and torch.isfinite(rv.float()).all()
            rk, rv = as_layout(rk, P, D, view), as_layout(rv, P, D, view)
            assert rk.stride() == k.stride()  # the same layout strides
            for with_pos in (False, True):
                deal = (combo + ti) % len(all_deals)  # (+ ti: a deal is not tied to one layout or one pos setting)
                names, mask = all_deals[deal]
                used.add(deal)
                combo += 1
                m = mask.to(torch.uint8).cuda()
                pos = pos_host.cuda() if with_pos else None
                # float64 restatement on the named rows (positional embedding added per window frame)
                idx = table_host.long()
                add = pos_host.double().view(1, T, 1, D) if with_pos else 0.0
                k64 = (hk[idx].double().view(B, T, P, D) + add).view(B, S, D)
                v64 = (hv[idx].double().view(B, T, P, D) + add).view(B, S, D)
                with torch.no_grad():
                    ref = restate(q_host, k64, v64, mask, T)
                for splits in splits_list:
                    case = f"table {tname} {'view' if view else 'dense'} pos {with_pos} masks {names} splits {splits}"
                    got = run_tabled(capi, q, k, v, table, m, splits, shape, pos, table_host=table_host)
                    want = run_plain(capi, q, rk, rv, m, splits, shape, pos)
                    assert_same(got, want, case)
                    hold("mix", got["mix"], ref["mix"], *BARS["mix"], case, worst)
                    hold("mix_softmax", got["mix_softmax"], ref["mix_softmax"], *BARS["mix_softmax"], case, worst)
                    hold("max", got["stats"][..., 0], ref["max"], *BARS["max"], case, worst)
                    hold("sumexp", got["stats"][..., 1], ref["sumexp"], *BARS["sumexp"], case, worst)
                    hold("aff", got["aff"], 0.5 * (ref["ws"] + ref["wc"]), KERNEL_ATOL, KERNEL_RTOL, case, worst)
                    hold("softmax branch", got["branches"][0], ref["ws"], KERNEL_ATOL, KERNEL_RTOL, case, worst)
                    hold("CoDA branch", got["branches"][1], ref["wc"], KERNEL_ATOL, KERNEL_RTOL, case, worst)
    assert used == set(range(len(all_deals)))
    print(f"{shape} {dtype}: worst |err| against float64 " + ", ".join(f"{n} {e:.2e}" for n, e in worst.items()))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_a_bad_table_is_clamped_by_the_kernel_and_refused_by_the_binding(capi, shape):
    """entries -3, C and C + 2 through the raw entry points equal the clamped table bit for bit, and the guards stay whole"""
    B, T, P, H = shape
    S, D, C = T * P, H * 64, B * T + 3
    dtype = torch.bfloat16
    good = make_table("wrapped", B, T, C)
    bad = good.clone()
    for i, e in zip(range(B * T), (-3, C, C + 2)):
        bad[i] = e
    clamped = bad.clamp(0, C - 1)
    assert not torch.equal(bad, clamped)
    q = rnd(B, H, 128, seed=3).reshape(B, -1).cuda()
    k, v, _, _ = make_store(C, P, D, dtype, set(clamped.tolist()), True, seed=21)
    m = deals(B, T)[0][1].to(torch.uint8).cuda()
    pos = rnd(T, D, seed=52, scale=0.3).cuda()
    splits = splits_of(B, S, P)[-1]
    want = run_tabled(capi, q, k, v, clamped.cuda(), m, splits, shape, pos, table_host=clamped)
    # the binding looks at the host copy, or reads the table back itself, and launches nothing
    o = Out(capi, B, T, P, H, splits)
    mix, mix_s, stats, aff, br = o.tensors()
    dbad = bad.cuda()
    for host in (bad, None):
        with pytest.raises(capi.DfdError, match=rf"decoder_attn_fwd_frames: the frame table has an entry outside \[0, {C}\)"):
            capi.decoder_attn_fwd_frames(q, k, v, dbad, m, mix, stats, o.ws.t, splits, B, T, P, H, mix_softmax=mix_s, pos=pos, table_host=host)
        with pytest.raises(capi.DfdError, match=rf"decoder_attn_map_frames: the frame table has an entry outside \[0, {C}\)"):
            capi.decoder_attn_map_frames(q, k, dbad, m, stats, aff, B, T, P, H, branches=br, pos=pos, table_host=host)
    for g in (o.mix, o.mix_s, o.stats, o.ws, o.aff, o.br):
        g.assert_untouched(view_too=True)
    # raw
    lib = capi.load_library()
    lay = capi.KvLayoutDesc(k.stride(1), k.stride(0), pos.data_ptr())
    rc = lib.dfd_decoder_attn_fwd_frames(q.data_ptr(), k.data_ptr(), v.data_ptr(), capi._DTYPE[dtype], ctypes.byref(lay), m.data_ptr(), None,
                                         mix.data_ptr(), mix_s.data_ptr(), stats.data_ptr(), o.ws.t.data_ptr(), splits, B, T, P, H, 64,
                                         dbad.data_ptr(), C, capi._stream())
    assert rc == 0, lib.dfd_last_error().decode()
    rc = lib.dfd_decoder_attn_map_frames(q.data_ptr(), k.data_ptr(), capi._DTYPE[dtype], ctypes.byref(lay), m.data_ptr(), stats.data_ptr(), None,
                                         aff.data_ptr(), br.data_ptr(), B, T, P, H, 64, dbad.data_ptr(), C, capi._stream())
    assert rc == 0, lib.dfd_last_error().decode()
    o.untouched()
    assert_same(dict(mix=mix, mix_softmax=mix_s, stats=stats, aff=aff, branches=br), want, f"{shape} raw call with a bad table")
    assert torch.isfinite(mix).all() and torch.isfinite(aff).all()


@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_the_stream_policy_leaves_the_bits_alone(capi, shape, dtype):
    B, T, P, H = shape
    S, D, C = T * P, H * 64, B * T + 3
    table_host = make_table("overlapping", B, T, C)
    q = rnd(B, H, 128, seed=3).reshape(B, -1).cuda()
    k, v, _, _ = make_store(C, P, D, dtype, set(table_host.tolist()), True, seed=31)
    m = deals(B, T)[-1][1].to(torch.uint8).cuda()
    pos = rnd(T, D, seed=52, scale=0.3).cuda()
    splits = policy_splits(B, S)
    keep = capi.stream_policy_get()
    try:
        want = None
        for mask in range(capi.STREAM_ALL + 1):
            capi.stream_policy_set(mask)
            got = run_tabled(capi, q, k, v, table_host.cuda(), m, splits, shape, pos, table_host=table_host)
            want = got if want is None else want
            assert_same(got, want, f"{shape} {dtype} stream policy {mask}")
    finally:
        capi.stream_policy_set(keep)


def test_refusals_and_the_empty_batch(capi):
    B, T, P, H = 2, 3, 5, 4
    S, D, C = T * P, H * 64, B * T + 3
    table_host = make_table("identity", B, T, C)
    table = table_host.cuda()
    q = rnd(B, H, 128, seed=3).reshape(B, -1).cuda()
    k, v, _, _ = make_store(C, P, D, torch.float32, set(table_host.tolist()), False, seed=41)
    m = torch.ones(B, T, dtype=torch.uint8, device="cuda")
    # the library's refusals, in check_decoder_attn's words, before any launch
    o = Out(capi, B, T, P, H, 2)
    mix, mix_s, stats, aff, br = o.tensors()
    lib = capi.load_library()

    def raw_fwd(**over):
        a = dict(q=q.data_ptr(), k=k.data_ptr(), v=v.data_ptr(), dt=capi._DTYPE[torch.float32], lay=None, m=m.data_ptr(), ext=None,
                 mix=mix.data_ptr(), mix_s=mix_s.data_ptr(), stats=stats.data_ptr(), ws=o.ws.t.data_ptr(), splits=2, B=B, T=T, P=P, H=H, d=64,
                 table=table.data_ptr(), C=C, st=capi._stream())
        a.update(over)
        rc = lib.dfd_decoder_attn_fwd_frames(*a.values())
        return rc, lib.dfd_last_error().decode()

    def raw_map(**over):
        a = dict(q=q.data_ptr(), k=k.data_ptr(), dt=capi._DTYPE[torch.float32], lay=None, m=m.data_ptr(), stats=stats.data_ptr(), ext=None,
                 aff=aff.data_ptr(), br=br.data_ptr(), B=B, T=T, P=P, H=H, d=64, table=table.data_ptr(), C=C, st=capi._stream())
        a.update(over)
        rc = lib.dfd_decoder_attn_map_frames(*a.values())
        return rc, lib.dfd_last_error().decode()

    for raw, name in ((raw_fwd, "dfd_decoder_attn_fwd_frames"), (raw_map, "dfd_decoder_attn_map_frames")):
        assert raw(table=None) == (-1, f"{name}: null frame table")
        assert raw(C=0)[0] == -1 and f"{name}: store_frames=0" in raw(C=0)[1]
        assert raw(C=-4)[0] == -1
        assert raw(k=None) == (-1, f"{name}: null pointer")
        assert raw(d=32) == (-1, f"{name}: head dim 32, only 64 is supported")
        assert raw(k=k.data_ptr() + 4) == (-1, f"{name}: pointers must be 16-byte aligned")
        assert raw(dt=capi.FP8)[0] == -1
    assert raw_fwd(splits=0) == (-1, "dfd_decoder_attn_fwd_frames: splits=0")
    assert raw_fwd(splits=4097) == (-1, "dfd_decoder_attn_fwd_frames: splits=4097")
    # B == 0 (an empty torch tensor has no address, so only a raw call gets there): success, nothing launched or written
    assert raw_fwd(B=0)[0] == 0 and raw_map(B=0)[0] == 0
    for g in (o.mix, o.mix_s, o.stats, o.ws, o.aff, o.br):
        g.assert_untouched(view_too=True)
    # the binding: a table of another length, another dtype, a store of another row width
    with pytest.raises(AssertionError):
        capi.decoder_attn_fwd_frames(q, k, v, table[:-1], m, mix, stats, o.ws.t, 2, B, T, P, H)
    with pytest.raises(AssertionError):
        capi.decoder_attn_fwd_frames(q, k, v, table.long(), m, mix, stats, o.ws.t, 2, B, T, P, H)
    with pytest.raises(AssertionError):
        capi.decoder_attn_map_frames(q, k[:, :, :D - 64], table, m, stats, aff, B, T, P, H)
    with pytest.raises(capi.DfdError, match="device tensors"):
        capi.decoder_attn_fwd_frames(q, k, v, table_host, m, mix, stats, o.ws.t, 2, B, T, P, H)
    # and after all that a plain call still runs
    got = run_tabled(capi, q, k, v, table, m, 2, (B, T, P, H), None, table_host=table_host)
    assert torch.isfinite(got["mix"]).all()
