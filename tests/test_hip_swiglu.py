"""GPU parity of dfd_swiglu_fwd (include/dfdclip_swiglu.h, csrc/swiglu.hip): hidden = silu(x12[:, :H]) * x12[:, H:] against
float64 on the same operands — dense, on strided views between poisoned guards (tests/guarded.py), from a base pointer one
element off (the element-wise form), on the fixed values where a careless silu overflows, and the refusals.

Bars (against float64 of the operands as the kernel reads them):
  f32   |d| <= 2e-5 * |ref| + 1e-30: exp through exp2 carries a relative error of about |x| * 2^-24 (6e-6 at |x| = 88), the
        reciprocal and two products a few roundings more; the floor covers results below the smallest normal f32
  bf16  |d| <= 2^-8 * |ref| + 1e-30: one rounding of that f32 result to 8 significant bits."""
import ctypes
import functools

import pytest
import torch

from dfd_clip_amd import capi
from tests.guarded import guarded

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8), (3, 5), (7, 37), (5, 344), (257, 344), (33, 4096), (1025, 64)]
DTYPES = [torch.float32, torch.bfloat16]
SPECIAL = [1e4, -1e4, 88.0, -88.0, 0.0, -0.0]
RTOL = {torch.float32: 2e-5, torch.bfloat16: 2.0 ** -8}
FLOOR = 1e-30
VEC = {torch.float32: 4, torch.bfloat16: 8}


def silu_gate_f64(x12, H):
    x1, x2 = x12[:, :H].double(), x12[:, H:].double()
    return x1 / (1 + torch.exp(-x1)) * x2  # exp(1e4) = inf in float64 too: -1e4 / inf = -0, the limit


@functools.lru_cache(maxsize=None)
def case(rows, H, dtype):
    """(x12 [rows, 2H], float64 reference, the dense call's result): computed once, shared, never written again."""
    g = torch.Generator(device="cuda").manual_seed(1000 * rows + H)
    x1 = 3 * torch.randn(rows, H, device="cuda", generator=g)
    x2 = 2 * torch.randn(rows, H, device="cuda", generator=g)
    n = rows * H
    for i in range(min(36, n)):  # every pair of fixed values where there is room, the gate's own fastest
        at = (i * 7) % n if n >= 36 * 7 else i
        x1.view(-1)[at], x2.view(-1)[at] = SPECIAL[i % 6], SPECIAL[(i // 6 + i) % 6]
    x12 = torch.cat([x1, x2], dim=1).to(dtype).contiguous()
    ref = silu_gate_f64(x12, H)
    assert torch.isfinite(ref).all()
    dense = torch.full((rows, H), float("nan"), device="cuda", dtype=dtype)
    capi.swiglu_fwd(x12, dense)
    path = capi.swiglu_last_path()
    torch.cuda.synchronize()
    return x12, ref, dense, path


def assert_within_bar(got, ref, dtype, what):
    assert not torch.isnan(got).any(), f"{what}: an output element was left NaN"
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    err = (got.double() - ref).abs()
    lim = RTOL[dtype] * ref.abs() + FLOOR
    print(f"{what}: max |d| {err.max().item():.3e}, worst |d| / limit {(err / lim).max().item():.3f}")
    assert (err <= lim).all(), f"{what}: |d| {err.max().item():.3e} beyond the bar at {int((err / lim).argmax())}"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,H", SHAPES)
def test_dense_against_float64(rows, H, dtype):
    x12, ref, dense, path = case(rows, H, dtype)
    assert path == (capi.SWIGLU_VEC16 if H % VEC[dtype] == 0 else capi.SWIGLU_ELEMENT)
    assert_within_bar(dense, ref, dtype, f"swiglu {rows}x{H} {dtype}")
    again = torch.full_like(dense, float("nan"))
    capi.swiglu_fwd(x12, again)
    assert torch.equal(again.view(torch.uint8), dense.view(torch.uint8))


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
def test_fixed_values(dtype):
    """x1 = -1e4 gives +-0 and never NaN, x1 = +1e4 gives x1 * x2, +-88 sit at the edge of exp's range, +-0 give +-0."""
    pairs = [(a, b) for a in SPECIAL for b in SPECIAL + [1.5, -2.25]]
    x1 = torch.tensor([p[0] for p in pairs], device="cuda").to(dtype)
    x2 = torch.tensor([p[1] for p in pairs], device="cuda").to(dtype)
    x12 = torch.cat([x1, x2]).view(1, -1).contiguous()
    out = torch.full((1, len(pairs)), float("nan"), device="cuda", dtype=dtype)
    capi.swiglu_fwd(x12, out)
    assert_within_bar(out, silu_gate_f64(x12, len(pairs)), dtype, f"fixed values {dtype}")
    o, a, b = out[0].double(), x1.double(), x2.double()
    assert (o[a < -1e3] == 0).all(), "silu(-1e4) * x2 must be +-0"
    big = a > 1e3
    assert torch.equal(o[big], (a[big] * b[big]).to(dtype).double()), "silu(+1e4) * x2 must be x1 * x2, rounded once"
    assert (o[a == 0] == 0).all()


@pytest.mark.parametrize("pad", [8, 3], ids=["pad8", "pad3"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,H", SHAPES)
def test_strided_views_between_guards(rows, H, dtype, pad):
    """ldx > 2H and ldh > H: padding of 8 elements keeps the 16-byte form where H allows it, of 3 forces the other."""
    x12, ref, dense, _ = case(rows, H, dtype)
    gx = guarded(rows, 2 * H, dtype, ld=2 * H + pad, name="x12").set(x12)
    gh = guarded(rows, H, dtype, ld=H + pad, name="hidden")
    capi.swiglu_fwd(gx.t, gh.t)
    want_vec = H % VEC[dtype] == 0 and pad % VEC[dtype] == 0
    assert capi.swiglu_last_path() == (capi.SWIGLU_VEC16 if want_vec else capi.SWIGLU_ELEMENT)
    gx.assert_untouched(view_too=True)
    gh.assert_untouched()
    assert_within_bar(gh.t, ref, dtype, f"guarded {rows}x{H} {dtype} pad {pad}")
    assert torch.equal(gh.t.contiguous().view(torch.uint8), dense.view(torch.uint8)), "the strided result is not the dense one bit for bit"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,H", SHAPES)
def test_base_pointer_one_element_off(rows, H, dtype):
    x12, ref, dense, _ = case(rows, H, dtype)
    xb = torch.full((rows * 2 * H + 1,), float("nan"), device="cuda", dtype=dtype)
    hb = torch.full((rows * H + 2,), float("nan"), device="cuda", dtype=dtype)
    xo, ho = xb[1:].view(rows, 2 * H), hb[1:1 + rows * H].view(rows, H)
    xo.copy_(x12)
    assert xo.data_ptr() % 16 != 0 and ho.data_ptr() % 16 != 0
    capi.swiglu_fwd(xo, ho)
    assert capi.swiglu_last_path() == capi.SWIGLU_ELEMENT
    assert torch.isnan(hb[0]) and torch.isnan(hb[-1]) and torch.isnan(xb[0])
    assert torch.equal(ho.contiguous().view(torch.uint8), dense.view(torch.uint8))
    assert_within_bar(ho, ref, dtype, f"offset base {rows}x{H} {dtype}")


def test_refusals_return_status_and_message_without_a_launch():
    lib = capi.load_library()
    H, rows = 8, 4
    x = torch.randn(rows, 2 * H, device="cuda")
    out = guarded(rows, H, torch.float32, name="hidden")
    stream = capi._stream()

    def call(xp, ldx, hp, ldh, dtype, r=rows, h=H):
        rc = lib.dfd_swiglu_fwd(ctypes.c_void_p(xp), ldx, ctypes.c_void_p(hp), ldh, dtype, r, h, stream)
        return rc, lib.dfd_last_error().decode()

    xp, hp = x.data_ptr(), out.t.data_ptr()
    for args, word in (((0, 2 * H, hp, H, capi.F32), "null"), ((xp, 2 * H, 0, H, capi.F32), "null"),
                       ((xp, 2 * H - 1, hp, H, capi.F32), "ldx"), ((xp, 2 * H, hp, H - 1, capi.F32), "ldh"),
                       ((xp, 2 * H, hp, H, capi.FP8), "dtype"), ((xp, 2 * H, hp, H, 7), "dtype")):
        rc, msg = call(*args)
        assert rc == -1 and "dfd_swiglu_fwd" in msg and word in msg, (args, rc, msg)
    rc, msg = call(xp, 2 * H, hp, H, capi.F32, r=-1)
    assert rc == -1 and "rows" in msg
    out.assert_untouched(view_too=True)  # nothing ran: the view still holds its poison
    assert torch.isnan(out.t).all()
    assert call(xp, 2 * H, hp, H, capi.F32, r=0)[0] == 0 and capi.swiglu_last_path() == 0  # rows == 0: a successful no-op
    out.assert_untouched(view_too=True)
    with pytest.raises(capi.DfdError, match="device tensors"):
        capi.swiglu_fwd(x.cpu(), out.t)
    with pytest.raises(AssertionError):
        capi.swiglu_fwd(x.to(torch.bfloat16), out.t)  # both tensors share one type
