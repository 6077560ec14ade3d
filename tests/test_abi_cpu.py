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
