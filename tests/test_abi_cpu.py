"""CPU checks of the drop-in boundary: the C-ABI library builds/loads and exports exactly the
symbols `include/dfdclip.h` declares; the ctypes table mirrors the header; the host side fails
loudly (no silent CPU fallback) when handed CPU tensors."""
import os
import re

import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.build import LIB_PATH, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    build()
    return capi.load_library()


def header_functions():
    text = open(os.path.join(ROOT, "include", "dfdclip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", text)))


def test_header_and_ctypes_table_agree():
    assert header_functions() == sorted(capi.SIGNATURES)


def test_library_exports_every_declared_symbol(lib):
    for name in header_functions():
        assert hasattr(lib, name), name
    assert lib.dfd_abi_version() == capi.ABI_VERSION
    assert os.path.exists(LIB_PATH)


def test_invalid_arguments_are_reported_not_launched(lib):
    # null pointers / bad shapes are rejected on the host before any launch (no GPU needed)
    rc = lib.dfd_layernorm(None, 0, None, None, None, 0, 0, 1, 8, 1e-5, 0.0, None)
    assert rc == -1 and b"null pointer" in lib.dfd_last_error()
    rc = lib.dfd_gemm(1 << 12, 48, 1 << 12, 48, capi.BF16, 1 << 12, 8, capi.BF16, None, capi.EPI_BIAS, None, 4, 8, 48, None)
    assert rc == -1 and b"multiple of 32" in lib.dfd_last_error()
    rc = lib.dfd_attention_fwd(1 << 12, 384, 1 << 12, 128, capi.F32, 1, 5, 2, 32, 0.1, None)
    assert rc == -1 and b"head_dim" in lib.dfd_last_error()
    assert lib.dfd_decoder_attn_workspace(16, 12, 64, 8) == 16 * 8 * 12 * 130 * 4


def test_decoder_attention_entry_points_refuse_the_same_arguments(lib):
    """The five decoder-attention entry points share one argument check (csrc/decoder_common.hpp check_decoder_attn):
    each refuses every bad argument of the table on the host, under its own name, and accepts the valid call with B = 0.
    No pointer is dereferenced."""
    import ctypes
    p = 1 << 12
    T, P, H = 2, 3, 2
    D = H * 64

    def call(name, B=2, d=64, heads=H, dt=capi.F32, kv=p, lay=None):
        lp = ctypes.byref(lay) if lay is not None else None
        args = {
            "dfd_decoder_attn_fwd": (p, kv, kv, dt, lp, p, None, p, None, p, p, 1, B, T, P, heads, d, None),
            "dfd_decoder_attn_modes_fwd": (p, kv, dt, lp, p, 3, p, p, B, T, P, heads, d, None),
            "dfd_decoder_attn_map": (p, kv, dt, lp, p, p, None, p, None, B, T, P, heads, d, None),
            "dfd_decoder_attn_bwd": (p, kv, kv, dt, lp, p, p, p, p, None, None, p, p, None, None, capi.F32, p, B, T, P, heads, d, None),
            "dfd_decoder_attn_modes_bwd": (p, kv, dt, lp, p, 3, p, p, B, T, P, heads, d, None),
        }[name]
        return getattr(lib, name)(*args)

    bad = {
        "d = 32": dict(d=32),
        "heads = 17": dict(heads=17),
        "kv_dtype = 7": dict(dt=7),
        "K / V pointer off by 8 bytes": dict(kv=p + 8),
        "row stride 127 < D": dict(lay=capi.KvLayoutDesc(127, 3 * 128, None)),
        "bf16 row stride 132: not a multiple of 8 elements": dict(dt=capi.BF16, lay=capi.KvLayoutDesc(132, 3 * 136, None)),
        "frame stride 0": dict(lay=capi.KvLayoutDesc(D, 0, None)),
        "pos off by 4 bytes": dict(lay=capi.KvLayoutDesc(D, P * D, p + 4)),
    }
    for name in ("dfd_decoder_attn_fwd", "dfd_decoder_attn_modes_fwd", "dfd_decoder_attn_map", "dfd_decoder_attn_bwd",
                 "dfd_decoder_attn_modes_bwd"):
        for what, kw in bad.items():
            assert call(name, **kw) == -1, f"{name}: {what} was accepted"
            assert lib.dfd_last_error().startswith(name.encode() + b":"), (name, what, lib.dfd_last_error())
        assert call(name, B=0) == 0, (name, lib.dfd_last_error())
        assert call(name, B=0, dt=capi.BF16, lay=capi.KvLayoutDesc(D + 8, (P + 1) * (D + 8), p)) == 0, (name, lib.dfd_last_error())


def test_layernorm_entry_points_refuse_the_same_arguments(lib):
    """The six LayerNorm entry points share one argument check (csrc/layernorm.hip ln_check): each refuses every bad
    argument of the table that applies to it on the host, under its own name and with the rule's key phrase, and accepts
    the valid call with rows = 0.  Fake aligned addresses; no pointer is dereferenced."""
    X, G, B, GA, BA, D, D2, Y, Y8 = ((i + 1) << 12 for i in range(9))
    F32, BF16, FP8 = capi.F32, capi.BF16, capi.FP8
    plain, two, add = ("dfd_layernorm", "dfd_layernorm_dual"), ("dfd_layernorm2", "dfd_layernorm2_dual"), ("dfd_add_layernorm", "dfd_add_layernorm_dual")
    single, dual = (plain[0], two[0], add[0]), (plain[1], two[1], add[1])
    everyone = plain + two + add

    def call(name, x=X, ldx=768, g=G, ga=GA, d=D, d2=D2, ldd=768, ddt=BF16, y=Y, ldy=768, ydt=BF16, y8=Y8, ldy8=768, rows=0, cols=768,
             scale=None):
        if scale is None:
            scale = 0.5 if name in dual or ydt == FP8 else 0.0
        front = {plain: (x, ldx, g, B), two: (x, ldx, ga, BA, g, B), add: (x, ldx, d, d2, ldd, ddt, 1, g, B)}[
            next(k for k in (plain, two, add) if name in k)]
        out = (y, ldy, y8, ldy8) if name in dual else (y, ldy, ydt)
        return getattr(lib, name)(*front, *out, rows, cols, 1e-5, scale, None)

    bad = [  # (what, arguments, key phrase, the entry points it applies to)
        ("null x", dict(x=None), "null pointer", everyone),
        ("cols = 6", dict(cols=6, ldx=8, ldy=8, ldy8=8, ldd=8), "multiple of 4", everyone),
        ("cols = 0", dict(cols=0), "multiple of 4", everyone),
        ("cols = 2052", dict(cols=2052, ldx=2052, ldy=2052, ldy8=2052, ldd=2052), "multiple of 4", two + add),
        ("cols = 4100", dict(cols=4100, ldx=4100, ldy=4100, ldy8=4100, ldd=4100), "multiple of 4", everyone),
        ("ldx < cols", dict(ldx=764), "bad leading dimension", everyone),
        ("ldx % 4 != 0", dict(ldx=770), "bad leading dimension", everyone),
        ("ldy < cols", dict(ldy=764), "bad leading dimension", everyone),
        ("ldy8 % 4 != 0", dict(ldy8=770), "bad leading dimension", dual),
        ("ldd < cols", dict(ldd=764), "bad leading dimension", add),
        ("x off by 8 bytes", dict(x=X + 8), "aligned", everyone),
        ("gamma off by 8 bytes", dict(g=G + 8), "aligned", everyone),
        ("gamma_a off by 8 bytes", dict(ga=GA + 8), "aligned", two),
        ("y off by 4 bytes", dict(y=Y + 4), "aligned", everyone),
        ("e4m3 y off by 2 bytes", dict(y=Y + 2, ydt=FP8), "aligned", single),
        ("y8 off by 2 bytes", dict(y8=Y8 + 2), "aligned", dual),
        ("delta off by 4 bytes", dict(d=D + 4), "aligned", add),
        ("delta2 off by 4 bytes", dict(d2=D2 + 4), "aligned", add),
        ("f32 delta off by 4 bytes", dict(d=D + 4, ddt=F32), "aligned", add),
        ("e4m3 without a scale", dict(ydt=FP8, scale=0.0), "inv_scale > 0", single),
        ("e4m3 with a negative scale", dict(ydt=FP8, scale=-1.0), "inv_scale > 0", single),
        ("dual without a scale", dict(scale=0.0), "inv_scale > 0", dual),
        ("y_dtype = 7", dict(ydt=7), "y_dtype", single),
        ("delta_dtype = 7", dict(ddt=7), "delta_dtype", add),
        ("y is x", dict(y=X), "must not alias", everyone[1:]),
        ("y8 is x", dict(y8=X), "must not alias", dual),
        ("y is delta", dict(y=D), "must not alias", add),
        ("y8 is delta2", dict(y8=D2), "must not alias", add[1:]),
        ("y16 is y8", dict(y8=Y), "must not alias", dual),
        ("rows = 2^34", dict(rows=1 << 34), "fit a grid", everyone),
        ("rows = 4 (2^31 - 1) + 1", dict(rows=4 * (2 ** 31 - 1) + 1), "fit a grid", everyone),
        ("rows = -1", dict(rows=-1), "rows=-1", everyone),
    ]
    for name in everyone:
        for what, kw, phrase, applies in bad:
            if name not in applies:
                continue
            assert call(name, **kw) == -1, f"{name}: {what} was accepted"
            err = lib.dfd_last_error()
            assert err.startswith(name.encode() + b":") and phrase.encode() in err, (name, what, err)
        assert call(name) == 0, (name, lib.dfd_last_error())
        # the widest row of each kind, padded rows, and the alignments that are enough: 8 bytes for an f32 y, 4 for e4m3
        wide = 4096 if name in plain else 2048
        assert call(name, cols=wide, ldx=wide + 4, ldy=wide + 8, ldy8=wide + 4, ldd=wide + 12) == 0, (name, lib.dfd_last_error())
        assert call(name, y8=Y8 + 4) == 0, (name, lib.dfd_last_error())
        if name in single:
            assert call(name, y=Y + 8, ydt=F32) == 0 and call(name, y=Y + 4, ydt=FP8) == 0, (name, lib.dfd_last_error())
        if name in add:
            assert call(name, d2=None) == 0 and call(name, ddt=F32, d=D + 8, d2=D2 + 8) == 0, (name, lib.dfd_last_error())
    # what dfd_layernorm alone accepts: f32 in place (encoder.py's use); and the plain kind's 16 slabs
    assert call("dfd_layernorm", y=X, ydt=F32) == 0, lib.dfd_last_error()
    for name in plain:
        assert call(name, cols=2052, ldx=2052, ldy=2052, ldy8=2052) == 0, (name, lib.dfd_last_error())


def test_adapter_norm_gelu_plan_table(lib):
    """The selection table of include/dfdclip_hooks.h (adp_plan in csrc/adapter.hip), through dfd_adapter_norm_gelu_plan, for
    both directions, every mode, aligned and misaligned bases: path, grid and block of the forward kernel or the backward's
    group pass, and the backward's affine slabs.  The numbers are written out by hand.  No device is touched."""
    c = capi
    REG, JOINT, R256, ROW = c.ADP_JOINT_REG, c.ADP_JOINT, c.ADP_ROW256, c.ADP_ROW
    F32, BF16 = torch.float32, torch.bfloat16
    table = {
        # (frames, patches, x): joint (aligned path, frames, slabs, groups per slab),
        #                       rows (aligned path, workgroups of four rows, rows, slabs, groups per slab)
        (5, 196, 256): ((REG, 5, 5, 1), (R256, 245, 980, 512, 2)),     # slab 50,176: 6 slabs wanted, 5 frames
        (3, 196, 256): ((REG, 3, 3, 1), (R256, 147, 588, 512, 2)),     # 588 rows in 512 slabs of 2: 294..511 stay empty
        (1, 224, 256): ((REG, 1, 1, 1), (R256, 56, 224, 224, 1)),      # slab 57,344: exactly the register limit
        (1, 225, 256): ((JOINT, 1, 1, 1), (R256, 57, 225, 225, 1)),    # one row past it
        (2, 7, 5): ((JOINT, 2, 2, 1), (ROW, 4, 14, 14, 1)),            # slab 35: not a multiple of 8
        (3, 49, 64): ((REG, 3, 3, 1), (ROW, 37, 147, 147, 1)),
        (2, 7, 40): ((REG, 2, 2, 1), (ROW, 4, 14, 14, 1)),
        (2, 3, 1024): ((REG, 2, 2, 1), (ROW, 2, 6, 6, 1)),
    }

    def plan(shape, mode, mis, bwd, adt=BF16, dt=BF16):
        p = c.adapter_norm_gelu_plan(*shape, mode, adt, dt, misaligned=mis, backward=bwd)
        return p.path, p.grid, p.block, p.slabs, p.groups_per_slab

    for shape, (jt, rw) in table.items():
        for adt, dt in ((F32, F32), (F32, BF16), (BF16, BF16)):
            for mis in (False, True):
                path = JOINT if mis else jt[0]
                assert plan(shape, 1, mis, False, adt, dt) == (path, jt[1], 1024, 0, 0), (shape, mis)
                assert plan(shape, 1, mis, True, adt, dt) == (path, jt[1], 1024, jt[2], jt[3]), (shape, mis)
                for mode in (0, 2):
                    if rw[0] == R256 and not mis:
                        fwd, bwd = (R256, rw[1], 256), (R256, rw[1], 256)
                    else:  # forward: four rows to a workgroup of 256; backward: a workgroup of 64 per row
                        fwd, bwd = (ROW, rw[1], 256), (ROW, rw[2], 64)
                    assert plan(shape, mode, mis, False, adt, dt) == fwd + (0, 0), (shape, mode, mis)
                    assert plan(shape, mode, mis, True, adt, dt) == bwd + (rw[3], rw[4]), (shape, mode, mis)
    # forward with no frames launches nothing; the backward refuses it, in its own words
    assert plan((0, 196, 256), 1, False, False) == (0, 0, 0, 0, 0)
    with pytest.raises(c.DfdError, match="dfd_adapter_norm_gelu_bwd: bad shape"):
        plan((0, 196, 256), 1, False, True)
    with pytest.raises(c.DfdError, match="dfd_adapter_norm_gelu: mode=3"):
        plan((1, 196, 256), 3, False, False)


def test_adapter_entry_points_refuse_the_same_arguments(lib):
    """dfd_adapter_norm_gelu and dfd_adapter_norm_gelu_bwd share one argument check (csrc/adapter.hip adp_check): each refuses
    every bad argument of the table that applies to it on the host, under its own name and with the rule's key phrase,
    before any launch; the forward accepts the valid call with frames = 0.  A second table holds the dropout-descriptor
    rule (csrc/adapter_common.hpp check_drop) of the adapter_structs.hip entry points that take a descriptor.  Fake
    aligned addresses; no pointer is dereferenced."""
    import ctypes
    A, Y, DY, W, B, DW, DB, WS = ((i + 1) << 12 for i in range(8))
    F32, BF16 = capi.F32, capi.BF16
    fwd, bwd = "dfd_adapter_norm_gelu", "dfd_adapter_norm_gelu_bwd"
    both = (fwd, bwd)

    def call(name, a=A, adt=BF16, out=Y, dy=DY, dt=BF16, w=W, ws=WS, frames=2, patches=7, x=40, mode=1):
        if name == fwd:
            return lib.dfd_adapter_norm_gelu(a, adt, out, dt, w, B, frames, patches, x, mode, 1e-5, None)
        return lib.dfd_adapter_norm_gelu_bwd(a, adt, dy, out, dt, w, B, DW, DB, ws, frames, patches, x, mode, 1e-5, None)

    bad = [  # (what, arguments, key phrase, the entry points it applies to)
        ("null a", dict(a=None), "null pointer", both),
        ("null weight", dict(w=None), "null pointer", both),
        ("null output", dict(out=None), "null pointer", both),
        ("null dy", dict(dy=None), "null pointer", (bwd,)),
        ("null workspace", dict(ws=None), "null pointer", (bwd,)),
        ("patches = 0", dict(patches=0), "bad shape", both),
        ("x = -1", dict(x=-1), "bad shape", both),
        ("frames = -1", dict(frames=-1), "bad shape", both),
        ("frames = 0", dict(frames=0), "bad shape", (bwd,)),
        ("dtype = 7", dict(dt=7, adt=7), "dtype=7", both),
        ("a_dtype = 7", dict(adt=7), "a_dtype=7", both),
        ("bf16 a beside f32", dict(adt=BF16, dt=F32), "must be dtype or f32", both),
        ("mode = 3", dict(mode=3), "mode=3", both),
        ("mode = -1", dict(mode=-1), "mode=-1", both),
        ("patches * x = 2^31", dict(patches=65536, x=32768), "below 2^31", both),
        ("patches * x = 2^31, per row", dict(patches=65536, x=32768, mode=0), "below 2^31", both),
        ("2^35 rows", dict(frames=2 ** 31 - 1, patches=16, x=8, mode=0), "fit a grid", both),
        ("2^35 rows, GELU first", dict(frames=2 ** 31 - 1, patches=16, x=8, mode=2), "fit a grid", both),
        ("2^34 rows of 256", dict(frames=2 ** 30, patches=16, x=256, mode=0), "fit a grid", both),
        ("2^32 rows, one workgroup each", dict(frames=2 ** 30, patches=4, x=8, mode=0), "fit a grid", (bwd,)),
        ("in place across dtypes", dict(out=A, adt=F32), "in place needs one dtype", (fwd,)),
        ("da is dy", dict(out=DY), "must not alias", (bwd,)),
        ("da is a", dict(out=A), "must not alias", (bwd,)),
    ]
    for name in both:
        for what, kw, phrase, applies in bad:
            if name not in applies:
                continue
            assert call(name, **kw) == -1, f"{name}: {what} was accepted"
            err = lib.dfd_last_error()
            assert err.startswith(name.encode() + b":") and phrase.encode() in err, (name, what, err)
    # what the forward accepts without a launch: no frames, in any mode, in place in one dtype, from any alignment
    for mode in (0, 1, 2):
        assert call(fwd, frames=0, mode=mode) == 0, lib.dfd_last_error()
    assert call(fwd, frames=0, out=A) == 0 and call(fwd, frames=0, a=A + 2, out=Y + 2) == 0, lib.dfd_last_error()
    assert call(fwd, frames=0, adt=F32) == 0 and call(fwd, frames=0, adt=F32, dt=F32, out=A) == 0, lib.dfd_last_error()

    def with_drop(name, drop, n=16):  # valid but for the descriptor; frames = 2, patches = 1, width = 8, T = 1
        d = ctypes.byref(drop) if drop is not None else None
        return {
            "dfd_adapter_bn_apply": lambda: lib.dfd_adapter_bn_apply(A, BF16, None, Y, BF16, None, None, None, None, d, n // 8, 1, 8, 1, None),
            "dfd_adapter_bn_bwd": lambda: lib.dfd_adapter_bn_bwd(A, DY, BF16, Y, BF16, W, B, DW, DB, d, WS, n // 8, 1, 8, 1, 1, None),
            "dfd_gelu_erf": lambda: lib.dfd_gelu_erf(A, BF16, Y, BF16, n, d, None),
            "dfd_gelu_erf_bwd": lambda: lib.dfd_gelu_erf_bwd(A, BF16, DY, BF16, Y, BF16, n, d, None),
        }[name]()

    bad_drops = {"p = -0.1": capi.DropoutDesc(WS, 3, -0.1), "p = 1": capi.DropoutDesc(WS, 3, 1.0), "p = 0.5 without a state": capi.DropoutDesc(None, 3, 0.5)}
    for name in ("dfd_adapter_bn_apply", "dfd_adapter_bn_bwd", "dfd_gelu_erf", "dfd_gelu_erf_bwd"):
        for what, drop in bad_drops.items():
            assert with_drop(name, drop) == -1, f"{name}: {what} was accepted"
            assert lib.dfd_last_error() == name.encode() + b": bad dropout", (name, what, lib.dfd_last_error())
        if name != "dfd_adapter_bn_bwd":  # the three that take an empty tensor: p = 0 needs no state, p > 0 has one
            assert with_drop(name, capi.DropoutDesc(None, 3, 0.0), n=0) == 0, (name, lib.dfd_last_error())
            assert with_drop(name, capi.DropoutDesc(WS, 3, 0.5), n=0) == 0 and with_drop(name, None, n=0) == 0, (name, lib.dfd_last_error())


def test_gemm_at_b_refuses_rows_the_fallback_cannot_launch(lib):
    """The transpose + general-kernel path of dfd_gemm_at_b puts one block of 32 rows on grid.y: more than 65535 blocks
    are refused on the host, under the function's name, before any launch.  No pointer is dereferenced and nothing is
    launched: the accepted R is stopped by the next argument check (a workspace that is not 256-byte aligned), which a
    refused R never reaches.  The gemm_tn path (bf16, extents multiples of 128) has no such limit."""
    p = 1 << 12
    path_before = lib.dfd_gemm_at_b_last_path()

    def call(R, dtype=capi.F32, Ma=8, Nb=12, ws=p + 16):
        return lib.dfd_gemm_at_b(p, Ma, p, Nb, dtype, p, R, Ma, Nb, ws, None)

    for dtype in (capi.F32, capi.BF16):
        assert call(65536 * 32, dtype) == -1
        err = lib.dfd_last_error()
        assert err.startswith(b"dfd_gemm_at_b:") and b"65535" in err and b"grid.y" in err, err
        assert call(65535 * 32 + 1, dtype) == -1 and b"65535" in lib.dfd_last_error()
        assert call(65535 * 32, dtype) == -1
        assert lib.dfd_last_error() == b"dfd_gemm_at_b: workspace must be 256-byte aligned", lib.dfd_last_error()
    # bf16 operands the gemm_tn kernels serve: the limit does not apply
    assert call(65536 * 32, capi.BF16, Ma=128, Nb=128) == -1
    assert lib.dfd_last_error() == b"dfd_gemm_at_b: workspace must be 256-byte aligned", lib.dfd_last_error()
    assert lib.dfd_gemm_at_b_last_path() == path_before  # set on success only


def test_encoder_attention_plan_table(lib):
    """The selection table of include/dfdclip_hooks.h (attn_plan in csrc/attention_common.hpp), through dfd_attention_plan:
    every row on both sides of every edge, with grid, block, LDS bytes and chunk.  No device: n_cu is given."""
    c = capi
    BF, F = torch.bfloat16, torch.float32

    def plan(tokens, n=43, heads=12, dtype=BF, variant=0, n_cu=256, **ld):
        assert c.attention_set_variant(variant) == 0
        try:
            p = c.attention_plan(dtype, n, tokens, heads, n_cu=n_cu, **ld)
        finally:
            c.attention_set_variant(0)
        return p.path, p.grid, p.block, p.lds, p.chunk

    def rows(tokens, items, esz, chunk=0):
        keys = chunk or tokens
        return (c.ATTN_ROWS_CHUNKED if chunk else c.ATTN_ROWS, items, 256, 2 * keys * 64 * esz, chunk)

    def persist(tokens, grid=256):
        return (c.ATTN_PERSIST7_SHORT if tokens <= 200 else c.ATTN_PERSIST7, grid, 512, 512 * tokens + 57344, 0)

    def stream(tokens, items):
        return (c.ATTN_STREAM, items * -(-tokens // 128), 256, 0, 0)

    item7 = lambda items: (c.ATTN_ITEM7, items, 256, 57856, 0)
    item9 = lambda items: (c.ATTN_ITEM9, items, 256, 74240, 0)
    xrow = lambda grid=256: (c.ATTN_XROW, grid, 512, 150528, 0)
    big = 43 * 12  # 516 items: enough for the persistent kernels

    # token edges at >= 512 items, variants 0 and 2 (2 only takes the streaming kernel away)
    for v in (0, 2):
        any_ = (lambda t: rows(t, big, 2)) if v == 2 else (lambda t: stream(t, big))
        assert plan(32, variant=v) == rows(32, big, 2)
        assert plan(33, variant=v) == any_(33)
        assert plan(192, variant=v) == any_(192)
        assert plan(193, variant=v) == persist(193) and plan(200, variant=v) == persist(200) and persist(200)[0] == c.ATTN_PERSIST7_SHORT
        assert plan(201, variant=v) == persist(201) and plan(208, variant=v) == persist(208) and persist(201)[0] == c.ATTN_PERSIST7
        assert persist(208)[3] == 163840
        assert plan(209, variant=v) == item7(big) and plan(224, variant=v) == item7(big)
        assert plan(225, variant=v) == any_(225) and plan(256, variant=v) == any_(256)
        assert plan(257, variant=v) == xrow()
        assert plan(258, variant=v) == item9(big) and plan(288, variant=v) == item9(big)
        assert plan(289, variant=v) == any_(289)
    # variant 1 only changes the rows kernel's staging
    assert plan(32, variant=1) == rows(32, big, 2, chunk=16) and plan(5, dtype=F, variant=1) == rows(5, big, 4, chunk=16)
    assert plan(50, variant=1) == stream(50, big) and plan(197, variant=1) == persist(197) and plan(257, variant=1) == xrow()
    assert plan(210, variant=1) == item7(big) and plan(288, variant=1) == item9(big)
    # 511 / 512 items in both windows
    for tokens, one, many in ((193, item7, persist(193)), (197, item7, persist(197)), (208, item7, persist(208)), (257, item9, xrow())):
        assert plan(tokens, n=511, heads=1) == one(511) and plan(tokens, n=512, heads=1) == many
        assert plan(tokens, n=32, heads=16) == many and plan(tokens, n=31, heads=16) == one(496)
    # compute units: a whole number of workgroups per XCD, at least one each
    for tokens, one, many in ((197, item7, persist), (257, item9, lambda t, g: xrow(g))):
        assert plan(tokens, n_cu=7) == one(big)
        assert plan(tokens, n_cu=8) == many(tokens, 8)
        assert plan(tokens, n_cu=255) == many(tokens, 248)
        assert plan(tokens, n_cu=256) == many(tokens, 256)
    # f32: always the rows kernel; whole-head staging up to 160 KiB of K and V, then 64 KiB chunks
    for tokens in (5, 32, 33, 197, 257, 320):
        assert plan(tokens, dtype=F) == rows(tokens, big, 4)
    assert rows(320, big, 4)[3] == 160 * 1024
    assert plan(321, dtype=F) == rows(321, big, 4, chunk=128) and plan(1370, dtype=F) == rows(1370, big, 4, chunk=128)
    assert plan(640, variant=2) == rows(640, big, 2) and rows(640, big, 2)[3] == 160 * 1024
    assert plan(641, variant=2) == rows(641, big, 2, chunk=256) and rows(641, big, 2, chunk=256)[3] == 65536
    assert plan(641) == stream(641, big) == (c.ATTN_STREAM, big * 6, 256, 0, 0)

    # 32-bit extents of the persistent kernels: the frame count at which a formula first passes 0xfffffff0, and the one before
    def extents(n, tokens, heads, ld_qkv, ld_out):
        return (n * tokens - 1) * ld_qkv * 2 + 3 * heads * 128, (n * tokens - 1) * ld_out * 2 + heads * 128

    def first_past(tokens, heads, ld_qkv, ld_out):
        n = 1
        while max(extents(n, tokens, heads, ld_qkv, ld_out)) <= 0xfffffff0:
            n += 1
        return n

    for tokens, one, many in ((197, item7, persist(197)), (208, item7, persist(208)), (257, item9, xrow())):
        heads = 12
        D = heads * 64
        n = first_past(tokens, heads, 3 * D, D)
        q, o = extents(n, tokens, heads, 3 * D, D)
        assert q > 0xfffffff0 >= o and extents(n - 1, tokens, heads, 3 * D, D)[0] <= 0xfffffff0 and (n - 1) * heads >= 512
        assert plan(tokens, n=n - 1) == many and plan(tokens, n=n) == one(n * heads)
        # a padded output whose extent binds before the input's does
        ld_out = 4 * D
        n = first_past(tokens, heads, 3 * D, ld_out)
        q, o = extents(n, tokens, heads, 3 * D, ld_out)
        assert o > 0xfffffff0 >= q and extents(n - 1, tokens, heads, 3 * D, ld_out)[1] <= 0xfffffff0 and (n - 1) * heads >= 512
        assert plan(tokens, n=n - 1, ld_out=ld_out) == many and plan(tokens, n=n, ld_out=ld_out) == one(n * heads)
    # the streaming kernel's grid: items * spans <= 2^31 - 1, else the rows kernel
    tokens, heads = 577, 1
    n = (2 ** 31 - 1) // 5
    assert plan(tokens, n=n, heads=heads) == (c.ATTN_STREAM, 5 * n, 256, 0, 0)
    assert plan(tokens, n=n + 1, heads=heads) == rows(tokens, n + 1, 2)
    # the guarded harness's ld + 8 takes the dense call's path
    for tokens in (5, 50, 197, 205, 210, 257, 288, 641):
        assert plan(tokens, ld_qkv=3 * 768 + 8, ld_out=768 + 8) == plan(tokens)
    # what dfd_attention_fwd refuses about a shape, the hook refuses in the same words
    with pytest.raises(capi.DfdError, match="dfd_attention_fwd: bad leading dimensions"):
        c.attention_plan(BF, 2, 50, 2, ld_qkv=3 * 128 + 4)
    with pytest.raises(capi.DfdError, match="dfd_attention_fwd: bad shape"):
        c.attention_plan(BF, 2, 0, 2)


def test_encoder_attention_refuses_items_that_do_not_fit_a_grid(lib):
    """2^31 (frame, head) items on a kernel whose grid is the item count (rows, ITEM7, ITEM9) are refused on the host, under
    the function's name, before any launch; 2^31 - 1 items are planned.  No pointer is dereferenced."""
    p = 1 << 12
    path_before = lib.dfd_attention_last_path()
    for dtype, tokens in ((capi.F32, 5), (capi.BF16, 5), (capi.BF16, 197), (capi.BF16, 288), (capi.BF16, 50)):
        heads, n = 16, 1 << 27
        D = heads * 64
        assert lib.dfd_attention_fwd(p, 3 * D, p, D, dtype, n, tokens, heads, 64, 0.125, None) == -1
        err = lib.dfd_last_error()
        assert err.startswith(b"dfd_attention_fwd:") and b"2147483648 (frame, head) items do not fit a grid" in err, err
        assert lib.dfd_attention_plan(dtype, n, tokens, heads, 3 * D, D, 256, None) == -1
        assert lib.dfd_last_error() == err
    assert lib.dfd_attention_plan(capi.F32, (1 << 31) - 1, 5, 1, 192, 64, 256, None) == capi.ATTN_ROWS
    assert lib.dfd_attention_plan(capi.BF16, (1 << 31) - 1, 197, 1, 192, 64, 256, None) == capi.ATTN_ITEM7
    assert lib.dfd_attention_last_path() == path_before  # set on success only


def test_cpu_tensors_fail_loudly(lib):
    x = torch.zeros(4, 8)
    with pytest.raises(capi.DfdError):
        capi.layernorm(x, torch.ones(8), torch.zeros(8), torch.empty(4, 8))


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(capi.DfdError):
        capi.load_library(str(tmp_path / "nope.so"))


def test_gemm_plan_table(lib):
    """The selection table of include/dfdclip_hooks.h (gemm_plan in csrc/gemm_plan.hpp), through dfd_gemm_plan: every row on
    both sides of every edge, with kernel, effective epilogue, tile height, row panels, grid and block.  No device: n_cu is
    given.  The expectations come from the table's words, modelled below, never from the library."""
    c = capi
    F, B, E = c.F32, c.BF16, c.FP8
    GEN, TILE, PERS, PING = c.GEMM_GENERAL, c.GEMM_TILE, c.GEMM_PERSISTENT, c.GEMM_PINGPONG
    BIAS, QGELU, BRES, PATCH, QKV, RPOS, GELU = (c.EPI_BIAS, c.EPI_BIAS_QUICKGELU, c.EPI_BIAS_RESIDUAL, c.EPI_PATCH_EMBED, c.EPI_QKV_EXPORT,
                                                  c.EPI_RESIDUAL_POS, c.EPI_BIAS_GELU)
    EXPORT, POS, RES = c.GEMM_PTR_EXPORT, c.GEMM_PTR_POS, c.GEMM_PTR_RESIDUAL
    LIM = 0xfffffff0
    ceil = lambda a, b: -(-a // b)

    def plan(ab, cd, epi, M, N, K, variant=0, pair=0, **kw):
        assert c.gemm_set_variant(variant) == 0 and c.gemm_pair_set_variant(pair) == 0
        kw.setdefault("frames_per_clip", 3)
        try:
            p = c.gemm_plan(ab, cd, epi, M, N, K, **kw)
        finally:
            c.gemm_set_variant(0)
            c.gemm_pair_set_variant(0)
        assert p.ntiles == p.tiles_m * (ceil(N, 128) if p.kernel == GEN else N // 256)
        return p.kernel, p.epilogue, p.tile_rows, p.tiles_m, p.grid, p.grid_y, p.block

    def refused(*a, match, **kw):
        with pytest.raises(capi.DfdError, match=match):
            plan(*a, **kw)

    # the table's launch rows
    general = lambda M, N, epi=BIAS: (GEN, epi, 128, ceil(M, 128), ceil(N, 128), ceil(M, 128), 256)
    tile = lambda M, N, epi=BIAS: (TILE, epi, 256, ceil(M, 256), ceil(M, 256) * (N // 256), 1, 512)
    rounds = lambda M, N, rows, cus: ceil(ceil(M, rows) * (N // 256), cus)
    height = lambda M, N, cus: 224 if 0.97 * rounds(M, N, 224, cus) < rounds(M, N, 256, cus) else 256

    def persistent(kernel, M, N, epi=BIAS, rows=None, cus=256):
        rows = rows or height(M, N, cus)
        return (kernel, epi, rows, ceil(M, rows), min(ceil(M, rows) * (N // 256), cus), 1, 512)

    ping = lambda *a, **kw: persistent(PING, *a, **kw)
    pers = lambda *a, **kw: persistent(PERS, *a, **kw)

    # ---- bf16 operands: M, N, K edges under variants 0 / 1 / 3, bf16 and f32 C -------------------------------------------
    Ks = (64, 96, 128, 192, 256, 320, 384, 512, 640, 768)
    for M in (1023, 1024):
        for N in (255, 256, 257, 512):
            for K in Ks:
                for v in (0, 1, 3):
                    tuned = M >= 1024 and N % 256 == 0 and K % 64 == 0
                    steps = K // 64
                    if tuned and v != 1 and steps % 2 == 0 and steps >= 6:
                        want = ping(M, N)
                    elif tuned and steps >= 2:
                        want = pers(M, N)
                    else:  # (with a bf16 C whatever the tile kernel serves a persistent kernel serves first)
                        want = general(M, N)
                    assert plan(B, B, BIAS, M, N, K, variant=v) == want, (M, N, K, v)
                    # an f32 C: the one-workgroup-per-tile kernel from K = 128, K % 64 == 0
                    assert plan(B, F, BIAS, M, N, K, variant=v) == (tile(M, N) if tuned and K >= 128 else general(M, N)), (M, N, K, v)
                    # f32 operands: the general kernel whatever the shape
                    assert plan(F, F, BIAS, M, N, K, variant=v) == general(M, N)
                    # RESIDUAL_POS: 224-row tiles on the ping-pong kernel, also at 4 steps; never the round-2 persistent kernel
                    if tuned and v != 1 and steps % 2 == 0 and (steps >= 6 or steps == 4):
                        want = ping(M, N, RPOS, rows=224)
                    else:
                        want = tile(M, N, RPOS) if tuned and K >= 128 else general(M, N, RPOS)
                    assert plan(B, B, RPOS, M, N, K, variant=v, tokens=17, has=POS | RES) == want, (M, N, K, v)
    # the dynamic hand-out: ping-pong, bf16, six steps and more, variant 3 only
    dyn = lambda v, K, epi=BIAS, ab=B: (c.gemm_set_variant(v), c.gemm_plan(ab, B, epi, 1024, 256, K, tokens=17).dynamic, c.gemm_set_variant(0))[1]
    assert (dyn(3, 384), dyn(0, 384), dyn(3, 320), dyn(3, 256, RPOS), dyn(3, 384, RPOS), dyn(3, 768, ab=E)) == (1, 0, 0, 0, 1, 0)
    # W rows that are no 128-byte multiple: the ping-pong kernel declines, the persistent one serves (dfd_gemm_last_path: 256)
    assert plan(B, B, BIAS, 1024, 768, 768, ldw=768 + 8) == pers(1024, 768) and plan(B, B, BIAS, 1024, 768, 768, ldw=768 + 64) == ping(1024, 768)
    # leading dimensions: 16-byte rows for the persistent kernels; the tile kernel takes ldc % 4; the entry point refuses lda % 8
    assert plan(B, B, BIAS, 1024, 256, 384, ldc=256 + 8) == ping(1024, 256) and plan(B, B, BIAS, 1024, 256, 384, ldc=256 + 4) == tile(1024, 256)
    assert plan(B, B, BIAS, 1024, 256, 384, ldc=256 + 2) == general(1024, 256)
    refused(B, B, BIAS, 1024, 256, 384, lda=384 + 4, match="dfd_gemm: lda=388 ldw=384 must be >= K and 16-byte multiples")
    # one misaligned pointer in turn
    every = EXPORT | POS | RES
    for bit in (c.GEMM_PTR_A, c.GEMM_PTR_W):
        refused(B, B, BIAS, 1024, 768, 384, misaligned=bit, match="dfd_gemm: A and W must be 16-byte aligned")
    for bit in (c.GEMM_PTR_C, c.GEMM_PTR_BIAS):
        assert plan(B, B, BIAS, 1024, 768, 384, misaligned=bit) == general(1024, 768)
        assert plan(B, F, BIAS, 1024, 768, 384, misaligned=bit) == general(1024, 768)
    for bit in (POS, c.GEMM_PTR_CLS, RES, c.GEMM_PTR_COL_SCALE, EXPORT):  # pointers the plain epilogue does not read
        assert plan(B, B, BIAS, 1024, 768, 384, has=every, misaligned=bit) == ping(1024, 768)
    assert plan(B, B, QKV, 1024, 768, 384, tokens=2, has=every, misaligned=POS) == general(1024, 768, QKV)
    assert plan(B, B, QKV, 1024, 768, 384, tokens=2, has=EXPORT, misaligned=POS) == ping(1024, 768, QKV)  # no pos: nothing to misalign
    assert plan(B, B, RPOS, 1024, 768, 384, tokens=2, has=every, misaligned=RES) == general(1024, 768, RPOS)
    assert plan(B, B, RPOS, 1024, 768, 384, tokens=2, has=every, misaligned=POS) == general(1024, 768, RPOS)
    assert plan(B, F, PATCH, 1024, 768, 384, tokens=3, has=POS, misaligned=c.GEMM_PTR_CLS) == general(1024, 768, PATCH)
    refused(E, B, BIAS, 1024, 768, 768, misaligned=c.GEMM_PTR_COL_SCALE, match="dfd_gemm_fp8: call not served: col_scale")

    # ---- epilogues, bf16 and f32 C, at a ping-pong depth (6 steps) and at one only the round-2 kernels serve (5) ---------
    M, N = 1024, 768
    for K, p16 in ((384, ping), (320, pers)):
        assert plan(B, B, BIAS, M, N, K) == p16(M, N) and plan(B, B, QGELU, M, N, K) == p16(M, N, QGELU)
        assert plan(B, B, QKV, M, N, K, tokens=2, has=EXPORT) == p16(M, N, QKV)
        assert plan(B, B, QKV, M, N, K, tokens=2, has=EXPORT, qkv_first=1) == general(M, N, QKV)  # N / 2 = 384: no whole tiles per block
        assert plan(B, B, QKV, M, 512, K, tokens=2, has=EXPORT, qkv_first=1) == p16(M, 512, QKV)
        assert plan(B, B, QKV, M, N, K, tokens=2) == p16(M, N, BIAS), "no export buffers: a plain biased store"
        for epi in (BIAS, QGELU):
            assert plan(B, F, epi, M, N, K) == tile(M, N, epi)
        assert plan(B, F, QKV, M, N, K, tokens=2) == tile(M, N, QKV) and plan(B, F, QKV, M, N, K, tokens=2, has=EXPORT) == tile(M, N, QKV)
        assert plan(B, F, BRES, M, N, K) == tile(M, N, BRES) and plan(B, F, PATCH, M, N, K, tokens=3, has=POS) == tile(M, N, PATCH)
        assert plan(B, F, RPOS, M, N, K, tokens=17) == general(M, N, RPOS) and plan(B, F, GELU, M, N, K) == general(M, N, GELU)
        refused(B, B, BRES, M, N, K, match="dfd_gemm: call not served: the epilogue needs an f32 C")
        refused(B, B, PATCH, M, N, K, tokens=3, has=POS, match="dfd_gemm: PATCH_EMBED writes an f32 token matrix")
        refused(B, B, 7, M, N, K, match="dfd_gemm: call not served: unknown epilogue")
    # BIAS_GELU with bf16 operands: the ping-pong kernel or the general one
    assert plan(B, B, GELU, M, N, 384) == ping(M, N, GELU) and plan(B, B, GELU, M, N, 320) == general(M, N, GELU)
    assert plan(B, B, GELU, M, N, 384, variant=1) == general(M, N, GELU)
    # RESIDUAL_POS: 224 rows whatever is asked; the tile kernel needs ldc % 8
    assert plan(B, B, RPOS, M, N, 384, tokens=17, flags=8 << 16) == ping(M, N, RPOS, rows=224)
    assert plan(B, B, RPOS, M, N, 320, tokens=17) == tile(M, N, RPOS) and plan(B, B, RPOS, M, N, 320, tokens=17, ldc=N + 4) == general(M, N, RPOS)
    # f32 operands: every epilogue on the general kernel
    for epi, kw in ((BIAS, {}), (QGELU, {}), (GELU, {}), (BRES, {}), (QKV, dict(tokens=2, has=EXPORT)), (RPOS, dict(tokens=17)), (PATCH, dict(tokens=3, has=POS))):
        assert plan(F, F, epi, M, N, 384, **kw) == general(M, N, epi)
    refused(F, B, BIAS, M, N, 384, match="dfd_gemm: f32 operands with bf16 output unsupported")

    # ---- e4m3 operands: a step is 128 elements.  K = 128: one step, refused; 256 and 512: two and four steps, the round-2
    # persistent kernel (the ping-pong loop starts at six); 768 and 1024: six and eight, the ping-pong kernel.  256-row tiles.
    M, N = 1024, 768
    for cd in (B, E):
        refused(E, cd, BIAS, M, N, 128, match="dfd_gemm_fp8: call not served: K is less than two 128-byte steps")
        for K, kernel in ((256, PERS), (512, PERS), (768, PING), (1024, PING)):
            for epi in (BIAS, QGELU, GELU):
                assert plan(E, cd, epi, M, N, K) == persistent(kernel, M, N, epi, rows=256), (cd, K, epi)
                assert plan(E, cd, epi, M, N, K, variant=1) == pers(M, N, epi, rows=256)
                assert plan(E, cd, epi, M, N, K, flags=7 << 16) == persistent(kernel, M, N, epi, rows=256), "no 224-row fp8 tiles"
        refused(E, cd, RPOS, M, N, 768, tokens=17, match="dfd_gemm_fp8: epilogue 5 not served")
    assert plan(E, B, QKV, M, N, 768, tokens=2, has=EXPORT) == ping(M, N, QKV, rows=256) and plan(E, B, QKV, M, N, 512, tokens=2, has=EXPORT) == pers(M, N, QKV, rows=256)
    refused(E, E, QKV, M, N, 768, tokens=2, match="dfd_gemm_fp8: fp8 output needs")
    refused(E, F, BIAS, M, N, 768, match="dfd_gemm_fp8: c_dtype=0")
    refused(E, B, BIAS, 1023, N, 768, match=r"dfd_gemm_fp8: call not served: M < 1024 \(epilogue 0, M=1023 N=768 K=768\)")
    refused(E, B, BIAS, M, 255, 768, match="dfd_gemm_fp8: call not served: N % 256 != 0")
    refused(E, B, BIAS, M, N, 768 + 64, match="dfd_gemm_fp8: call not served: a row of K is not a whole number of 128-byte steps")
    # what the package restates as constants: the row threshold of the fp8 path and the widths it is built for
    assert c.FP8_MIN_ROWS == 1024
    assert plan(E, B, BIAS, c.FP8_MIN_ROWS, 768, 768)[0] == PING
    refused(E, B, BIAS, c.FP8_MIN_ROWS - 1, 768, 768, match="not served")
    from dfd_clip_amd.dinov2 import ARCHS
    tiny, base = ARCHS["dino_tiny"][2], ARCHS["dinov2_vitb14"][2]
    assert (tiny, base) == (128, 768) and tiny % 256 != 0 and base % 256 == 0  # (dinov2.py refuses fp8 by width % 256)
    refused(E, B, BIAS, 4096, 3 * tiny, tiny, match="not served")
    refused(E, B, BIAS, 4096, tiny, 4 * tiny, match="not served")
    assert plan(E, B, BIAS, 4096, 3 * base, base)[0] == PING and plan(E, B, GELU, 4096, 4 * base, base)[0] == PING

    # ---- the c_fc -> c_proj pair: this kernel at any M, or an error; pair variant 1 keeps the kernel and clears the layout --
    CB, AB = c.GEMM_C_BLOCKED, c.GEMM_A_BLOCKED
    D, H = 768, 3072

    def flags_in_force(epi, N, K, flag, M, pv, **kw):
        assert c.gemm_pair_set_variant(pv) == 0
        try:
            p = c.gemm_plan(B, B, epi, M, N, K, flags=flag, **kw)
            return p.kernel, p.c_blocked, p.a_blocked, bool(c.gemm_pair_plan(M, D, H))
        finally:
            c.gemm_pair_set_variant(0)

    for M in (32, 1023, 1024):
        for pv in (0, 1, 2):
            fc = flags_in_force(QGELU, H, D, CB, M, pv)
            pr = flags_in_force(BIAS, D, H, AB, M, pv)
            assert fc[:3] == (PING, int(pv != 1), 0) and pr[:3] == (PING, 0, int(pv != 1)), (M, pv, fc, pr)
            # the pair's plan: both halves planned blocked, plus the policy of 1024 rows (variant 2 waives it)
            assert fc[3] == pr[3] == (fc[1] == 1 and pr[2] == 1 and (M >= 1024 or pv == 2)), (M, pv)
            assert plan(B, B, QGELU, M, H, D, flags=CB, pair=pv) == ping(M, H, QGELU) and plan(B, B, BIAS, M, D, H, flags=AB, pair=pv) == ping(M, D)
            assert flags_in_force(GELU, H, D, CB, M, pv)[:3] == fc[:3]
    pair_words = "dfd_gemm: DFD_GEMM_C_BLOCKED / DFD_GEMM_A_BLOCKED: the ping-pong kernel does not serve this call: "
    refused(B, B, QGELU, 1024, H, D, flags=CB, ldc=H + 8, match=pair_words + "the leading dimension of a fragment-blocked matrix")
    refused(B, B, BIAS, 1024, D, H, flags=AB, lda=H + 8, match=pair_words + r".*\(epilogue 0, M=1024 N=768 K=3072\)")
    assert plan(B, B, QGELU, 1024, H, D, flags=CB, ldc=H + 8, pair=1) == ping(1024, H, QGELU), "row-major: any 16-byte ldc"
    assert plan(B, B, QGELU, 1024, H, D, flags=CB, ldc=H + 64) == ping(1024, H, QGELU)
    refused(B, B, BIAS, 1024, H, D, flags=CB, match=pair_words + "DFD_GEMM_C_BLOCKED needs BIAS_QUICKGELU or BIAS_GELU")
    refused(B, B, QGELU, 1024, D, H, flags=AB, match=pair_words + "DFD_GEMM_A_BLOCKED needs BIAS")
    refused(B, B, QGELU, 1024, H, D, flags=CB, variant=1, match=pair_words + r"dfd_gemm_set_variant\(1\) skips the ping-pong kernel")
    refused(B, B, QGELU, 32, 512, 128, flags=CB, match=pair_words + "the ping-pong K loop needs")
    refused(B, F, QGELU, 1024, H, D, flags=CB, match=pair_words + "C must be bf16")
    refused(E, B, QGELU, 1024, H, D, flags=CB, match="dfd_gemm_fp8: DFD_GEMM_C_BLOCKED / DFD_GEMM_A_BLOCKED: .*the fragment-blocked layout is bf16")
    assert c.gemm_set_variant(1) == 0 and not c.gemm_pair_plan(94560, D, H) and c.gemm_set_variant(0) == 1

    # ---- the tile plan on 256 compute units (ViT-B/16: 480 frames of 197 tokens) -------------------------------------------
    M = 94560
    assert plan(B, B, BIAS, M, 768, 768) == (PING, BIAS, 224, 423, 256, 1, 512)      # 5 rounds either way: the cheaper tile
    assert plan(B, B, BIAS, M, 2304, 768) == (PING, BIAS, 256, 370, 256, 1, 512)     # 15 rounds of 224 rows against 14
    assert plan(B, B, QGELU, M, 3072, 768) == (PING, QGELU, 256, 370, 256, 1, 512)   # 20 against 18
    assert (rounds(M, 768, 224, 256), rounds(M, 768, 256, 256), rounds(M, 2304, 224, 256), rounds(M, 2304, 256, 256)) == (5, 5, 15, 14)
    assert (rounds(M, 3072, 224, 256), rounds(M, 3072, 256, 256)) == (20, 18)
    assert plan(B, B, BIAS, M, 2304, 768, flags=7 << 16) == ping(M, 2304, rows=224) and plan(B, B, BIAS, M, 768, 768, flags=8 << 16) == ping(M, 768, rows=256)
    refused(B, B, BIAS, M, 768, 768, flags=5 << 16, match="dfd_gemm: tile blocks must be 0, 7 or 8")
    for kernel, K in ((PING, 768), (PERS, 320)):
        for spare, cus in ((32, 224), (100, 156), (200, 128)):  # binding, floored at half the chip
            for N in (768, 2304):
                assert plan(B, B, BIAS, M, N, K, flags=spare << 8) == persistent(kernel, M, N, cus=cus), (kernel, spare, N)
    # DFD_GEMM_SPARE_IF_FREE: honoured where the cheaper height costs no more on the CUs left than on all of them (50,000 rows
    # of N = 768: three rounds of 224-row tiles on 224 CUs as on 256), else every CU (94,560 rows: five rounds of 256-row tiles
    # on 224 CUs, five cheaper ones of 224 rows on 256); the round-2 persistent kernel takes the request as given
    cost = lambda M, N, cus: min(0.97 * rounds(M, N, 224, cus), rounds(M, N, 256, cus))
    assert cost(50000, 768, 224) == cost(50000, 768, 256) == 0.97 * 3 and (cost(M, 768, 224), cost(M, 768, 256)) == (5, 0.97 * 5)
    assert cost(M, 2304, 224) > cost(M, 2304, 256)
    sif = (32 << 8) | c.GEMM_SPARE_IF_FREE
    assert plan(B, B, BIAS, 50000, 768, 3072, flags=sif) == ping(50000, 768, cus=224) == (PING, BIAS, 224, 224, 224, 1, 512)
    assert plan(B, B, BIAS, M, 768, 3072, flags=sif) == ping(M, 768, cus=256) == (PING, BIAS, 224, 423, 256, 1, 512)
    assert plan(B, B, BIAS, M, 2304, 768, flags=sif) == ping(M, 2304, cus=256)
    assert plan(B, B, BIAS, M, 2304, 320, flags=sif) == pers(M, 2304, cus=224)
    assert plan(E, B, BIAS, M, 2304, 768, flags=sif) == ping(M, 2304, rows=256, cus=256) and plan(E, B, BIAS, M, 2304, 768, flags=32 << 8) == ping(M, 2304, rows=256, cus=224)
    # fewer tiles than CUs; a small chip
    assert plan(B, B, BIAS, 1024, 256, 384) == (PING, BIAS, 224, 5, 5, 1, 512) and plan(B, B, BIAS, 1024, 256, 384, flags=8 << 16) == (PING, BIAS, 256, 4, 4, 1, 512)
    assert plan(B, B, BIAS, M, 768, 768, n_cu=8) == ping(M, 768, cus=8) and ping(M, 768, cus=8)[4] == 8
    assert plan(B, B, BIAS, M, 768, 768, n_cu=8, flags=6 << 8) == ping(M, 768, cus=4)

    # ---- 32-bit extents: the first M at which a rule trips, and the one before --------------------------------------------
    # (the persistent kernels address A, W and C through buffer descriptors; past them the tile kernel, which has no such
    # limit, serves the call.  The export's and RESIDUAL_POS's own limits cannot bind before C's: C is the larger matrix.)
    N, K = 256, 384
    for lda, ldc in ((K, N), (K, N + 4096), (K + 4096, N)):
        first = min(LIM // (lda * 2), LIM // (ldc * 2)) + 1
        assert max((first - 1) * lda, (first - 1) * ldc) * 2 <= LIM < max(first * lda, first * ldc) * 2
        assert plan(B, B, BIAS, first - 1, N, K, lda=lda, ldc=ldc) == ping(first - 1, N)
        assert plan(B, B, BIAS, first, N, K, lda=lda, ldc=ldc) == tile(first, N)
        assert plan(B, B, BIAS, first, N, 320, lda=lda if lda > K else 320, ldc=ldc)[0] == (TILE if lda == K + 4096 or ldc > N else PERS)
    first = LIM // 768 + 1  # e4m3: one byte per element, and no other kernel
    assert plan(E, B, BIAS, first - 1, N, 768) == ping(first - 1, N, rows=256)
    refused(E, B, BIAS, first, N, 768, match="dfd_gemm_fp8: call not served: A, W or C exceeds the 32-bit byte offsets")
    ldw = (LIM // (N * 2) // 64 + 1) * 64  # W: N rows of ldw elements
    assert N * (ldw - 64) * 2 <= LIM < N * ldw * 2
    assert plan(B, B, BIAS, 1024, N, K, ldw=ldw - 64) == ping(1024, N) and plan(B, B, BIAS, 1024, N, K, ldw=ldw) == tile(1024, N)
    # a blocked matrix keeps whole groups of 16 rows: the rounded-up M counts
    first = (LIM // (D * 2)) // 16 * 16 + 1
    assert (first - 1) * D * 2 <= LIM < (first + 15) * D * 2 and first * D * 2 <= LIM
    assert plan(B, B, BIAS, first - 1, 256, D, flags=AB) == ping(first - 1, 256) and plan(B, B, BIAS, first, 256, D) == ping(first, 256)
    refused(B, B, BIAS, first, 256, D, flags=AB, match=pair_words + "A, W or C exceeds")
    # the tile kernel: rows below 2^31, tiles within 2^31 - 1
    assert plan(B, F, BIAS, (1 << 31) - 1, 256, 128) == tile((1 << 31) - 1, 256) and plan(B, F, BIAS, 1 << 31, 256, 128) == general(1 << 31, 256)
    wide = 256 * 257
    first = 256 * ((2 ** 31 - 1) // 257) + 1
    assert ceil(first - 1, 256) * 257 <= 2 ** 31 - 1 < ceil(first, 256) * 257
    assert plan(B, F, BIAS, first - 1, wide, 128) == tile(first - 1, wide) and plan(B, F, BIAS, first, wide, 128) == general(first, wide)

    # ---- nothing to launch; the guarded harness's padded rows take the dense call's kernel ---------------------------------
    assert plan(B, B, BIAS, 0, 768, 768) == (0, BIAS, 0, 0, 0, 0, 0)
    for K in (192, 320, 384, 768):
        assert plan(B, B, QGELU, 2893, 768, K, lda=K + 8, ldw=K + 64, ldc=768 + 8) == plan(B, B, QGELU, 2893, 768, K)

    # ---- a refused call leaves the record of the last kernel alone, and the entry points refuse in the hook's words -------
    p = 1 << 12
    kernel_before, path_before = lib.dfd_gemm_last_kernel(), lib.dfd_gemm_last_path()
    ex = capi.GemmExtra(None, None, None, None, 0, 0, None, 0, None, 0, 0.0, CB)
    assert lib.dfd_gemm(p, D, p, D, B, p, H + 8, B, p, QGELU, ex, 1024, H, D, None) == -1
    err = lib.dfd_last_error()
    refused(B, B, QGELU, 1024, H, D, flags=CB, ldc=H + 8, match=re.escape(err.decode()))
    assert lib.dfd_gemm_fp8(p, 768, p, 768, p, 768, B, p, p, 0.0, BIAS, None, 1023, 768, 768, None) == -1
    assert lib.dfd_last_error() == b"dfd_gemm_fp8: call not served: M < 1024 (epilogue 0, M=1023 N=768 K=768)"
    assert lib.dfd_gemm(p, 48, p, 48, B, p, 8, B, None, BIAS, None, 4, 8, 48, None) == -1 and b"multiple of 32" in lib.dfd_last_error()
    assert lib.dfd_gemm(p, 64, p, 64, B, p, 8, B, None, BRES, None, 4, 8, 64, None) == -1 and b"needs an f32 C" in lib.dfd_last_error()
    assert lib.dfd_gemm(p, 64, p, 64, B, p, 8, B, None, BIAS, None, 0, 8, 64, None) == 0  # M = 0: accepted, nothing launched
    assert (lib.dfd_gemm_last_kernel(), lib.dfd_gemm_last_path()) == (kernel_before, path_before)
