"""Dual-output LayerNorm (include/dfdclip_ext.h): the bf16 and the e4m3 output of one pass are the bits the single-output
entry point writes for that type — all three forms, outlier included, both epsilons the towers use."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 0.02
# one slab / several slabs / a last slab that is not full (772 = 3 * 256 + 4); rows that are no multiple of a workgroup's 4
SHAPES = [(1000, 768), (257, 1024), (3, 128), (1025, 772)]


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    return c


def inputs(rows, cols):
    g = torch.Generator(device="cuda").manual_seed(rows * 7 + cols)
    x = torch.randn(rows, cols, device="cuda", generator=g) * 3 + 0.5
    if rows > 5:
        x[5, 7] = 500.0  # an outlier: its e4m3 value saturates
    gam, bet = 1 + 0.1 * torch.randn(cols, device="cuda", generator=g), 0.1 * torch.randn(cols, device="cuda", generator=g)
    return g, x, gam, bet


def outs(rows, cols):
    return (torch.full((rows, cols), float("nan"), device="cuda", dtype=torch.bfloat16),
            torch.full((rows, cols), 0x7f, device="cuda", dtype=torch.uint8))  # 0x7f: e4m3's NaN


def finite(y16, y8):
    return torch.isfinite(y16.float()).all() and torch.isfinite(y8.view(torch.float8_e4m3fn).float()).all()


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_layernorm_dual(capi, rows, cols, eps):
    _, x, gam, bet = inputs(rows, cols)
    w16, w8 = outs(rows, cols)
    capi.layernorm(x, gam, bet, w16, eps=eps)
    capi.layernorm(x, gam, bet, w8, eps=eps, out_inv_scale=1.0 / SCALE)
    y16, y8 = outs(rows, cols)
    capi.layernorm_dual(x, gam, bet, y16, y8, 1.0 / SCALE, eps=eps)
    assert finite(y16, y8), "an element was not written"
    assert torch.equal(y16, w16) and torch.equal(y8, w8)
    if rows > 5:
        assert y8.view(torch.float8_e4m3fn).float().abs().max().item() == 448.0


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_layernorm2_dual(capi, rows, cols, eps):
    g, x, ga, ba = inputs(rows, cols)
    gb, bb = 1 + 0.5 * torch.randn(cols, device="cuda", generator=g), 0.5 * torch.randn(cols, device="cuda", generator=g)
    w16, w8 = outs(rows, cols)
    x16, x8, xd = x.clone(), x.clone(), x.clone()
    capi.layernorm2(x16, ga, ba, gb, bb, w16, eps=eps)
    capi.layernorm2(x8, ga, ba, gb, bb, w8, eps=eps, out_inv_scale=1.0 / SCALE)
    y16, y8 = outs(rows, cols)
    capi.layernorm2_dual(xd, ga, ba, gb, bb, y16, y8, 1.0 / SCALE, eps=eps)
    assert finite(y16, y8), "an element was not written"
    assert torch.equal(xd, x16) and torch.equal(xd, x8), "x <- LayerNorm_a(x)"
    assert torch.equal(y16, w16) and torch.equal(y8, w8)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_add_layernorm_dual(capi, rows, cols, eps):
    g, x, gam, bet = inputs(rows, cols)
    d1 = torch.randn(rows, cols, device="cuda", generator=g).to(torch.bfloat16)
    d2 = torch.randn(rows, cols, device="cuda", generator=g).to(torch.bfloat16)
    for two in (False, True):
        for store_x in (True, False):
            kw = dict(eps=eps, delta2=d2 if two else None, store_x=store_x)
            w16, w8 = outs(rows, cols)
            x16, x8, xd = x.clone(), x.clone(), x.clone()
            capi.add_layernorm(x16, d1, gam, bet, w16, **kw)
            capi.add_layernorm(x8, d1, gam, bet, w8, out_inv_scale=1.0 / SCALE, **kw)
            y16, y8 = outs(rows, cols)
            capi.add_layernorm_dual(xd, d1, gam, bet, y16, y8, 1.0 / SCALE, **kw)
            msg = f"two={two} store_x={store_x}"
            assert finite(y16, y8), msg
            assert torch.equal(xd, x16) and torch.equal(xd, x8), msg
            assert torch.equal(xd, x) != store_x, msg
            assert torch.equal(y16, w16) and torch.equal(y8, w8), msg
