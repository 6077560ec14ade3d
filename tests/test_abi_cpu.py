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


def test_cpu_tensors_fail_loudly(lib):
    x = torch.zeros(4, 8)
    with pytest.raises(capi.DfdError):
        capi.layernorm(x, torch.ones(8), torch.zeros(8), torch.empty(4, 8))


def test_missing_library_fails_loudly(tmp_path):
    with pytest.raises(capi.DfdError):
        capi.load_library(str(tmp_path / "nope.so"))
