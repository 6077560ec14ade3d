"""Guard-band and strided-view runs of the entry points of include/dfdclip_ext.h, with the harness of
tests/test_hip_guarded.py (tests/guarded.py): leading dimensions > columns for both outputs, poisoned guards and row padding,
outputs poisoned inside.  Asserted: no byte outside a view changed, no element left unwritten, and each output is the bits
of the single-output entry point's dense run for that type.

Coverage (checked against include/dfdclip_ext.h by tests/test_fp8_policy_cpu.py):

    dfd_layernorm_dual                    test_layernorm_dual
    dfd_layernorm2_dual                   test_layernorm2_dual
    dfd_add_layernorm_dual                test_add_layernorm_dual
"""
import pytest
import torch

from tests.test_hip_guarded import BF16, E4M3, F32, _f, both, capi, same_bits  # noqa: F401  (capi: the module's fixture)

pytestmark = pytest.mark.gpu

SCALE = 0.02
SHAPES = [(1000, 768), (257, 1024), (3, 128), (1025, 772)]


def inputs(rows, cols):
    g = torch.Generator().manual_seed(rows * 7 + cols)
    x = torch.randn(rows, cols, generator=g) * 3 + 0.5
    if rows > 5:
        x[5, 7] = 500.0
    return g, x, 1 + 0.1 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)


def check(dense, got, want, msg):
    """dense / got: {"y16", "y8"[, "x"]} of the dual call on dense and on guarded buffers; want: the single-output calls'."""
    for run in (dense, got):
        for name, w in want.items():
            assert torch.isfinite(_f(run[name])).all(), f"{msg} {name}: an element was not written"
            same_bits(run[name], w, f"{msg} {name}")


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_layernorm_dual(capi, rows, cols, eps):
    _, x, gam, bet = inputs(rows, cols)
    xc, gc, bc = x.cuda(), gam.cuda(), bet.cuda()
    w16 = capi.layernorm(xc, gc, bc, torch.empty(rows, cols, device="cuda", dtype=BF16), eps=eps)
    w8 = capi.layernorm(xc, gc, bc, torch.empty(rows, cols, device="cuda", dtype=torch.uint8), eps=eps, out_inv_scale=1 / SCALE)

    def op(b):
        y16, y8 = b.out((rows, cols), BF16, pad=8, name="y16"), b.out((rows, cols), E4M3, pad=12, name="y8")
        capi.layernorm_dual(b.inp(x, pad=4, name="x"), b.inp(gam, name="gamma"), b.inp(bet, name="beta"), y16, y8, 1 / SCALE, eps=eps)
        return {"y16": y16, "y8": y8}
    check(*both(op), {"y16": w16, "y8": w8.view(E4M3)}, "layernorm_dual")


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_layernorm2_dual(capi, rows, cols, eps):
    g, x, ga, ba = inputs(rows, cols)
    gb, bb = 1 + 0.5 * torch.randn(cols, generator=g), 0.5 * torch.randn(cols, generator=g)
    dev = [t.cuda() for t in (ga, ba, gb, bb)]
    x16, x8 = x.cuda(), x.cuda()
    w16 = capi.layernorm2(x16, *dev, torch.empty(rows, cols, device="cuda", dtype=BF16), eps=eps)
    w8 = capi.layernorm2(x8, *dev, torch.empty(rows, cols, device="cuda", dtype=torch.uint8), eps=eps, out_inv_scale=1 / SCALE)

    def op(b):
        xx = b.out((rows, cols), F32, pad=4, init=x, name="x")
        y16, y8 = b.out((rows, cols), BF16, pad=12, name="y16"), b.out((rows, cols), E4M3, pad=4, name="y8")
        capi.layernorm2_dual(xx, b.inp(ga), b.inp(ba), b.inp(gb), b.inp(bb), y16, y8, 1 / SCALE, eps=eps)
        return {"x": xx, "y16": y16, "y8": y8}
    check(*both(op), {"x": x16, "y16": w16, "y8": w8.view(E4M3)}, "layernorm2_dual")
    assert torch.equal(x16, x8)


@pytest.mark.parametrize("eps", [1e-5, 1e-6])
@pytest.mark.parametrize("rows,cols", SHAPES)
def test_add_layernorm_dual(capi, rows, cols, eps):
    g, x, gam, bet = inputs(rows, cols)
    d1, d2 = torch.randn(rows, cols, generator=g).to(BF16), torch.randn(rows, cols, generator=g).to(BF16)
    gc, bc = gam.cuda(), bet.cuda()
    for two in (False, True):
        for store_x in (True, False):
            kw = dict(eps=eps, delta2=d2.cuda() if two else None, store_x=store_x)
            x16, x8 = x.cuda(), x.cuda()
            w16 = capi.add_layernorm(x16, d1.cuda(), gc, bc, torch.empty(rows, cols, device="cuda", dtype=BF16), **kw)
            w8 = capi.add_layernorm(x8, d1.cuda(), gc, bc, torch.empty(rows, cols, device="cuda", dtype=torch.uint8), out_inv_scale=1 / SCALE, **kw)

            def op(b):
                xx = b.out((rows, cols), F32, pad=4, init=x, name="x")
                y16, y8 = b.out((rows, cols), BF16, pad=8, name="y16"), b.out((rows, cols), E4M3, pad=20, name="y8")
                capi.add_layernorm_dual(xx, b.inp(d1, pad=12, name="delta"), b.inp(gam), b.inp(bet), y16, y8, 1 / SCALE, eps=eps,
                                        delta2=b.inp(d2, pad=12, name="delta2") if two else None, store_x=store_x)
                return {"x": xx, "y16": y16, "y8": y8}
            check(*both(op), {"x": x16, "y16": w16, "y8": w8.view(E4M3)}, f"add_layernorm_dual two={two} store_x={store_x}")
            assert torch.equal(x16.cpu(), x) != store_x
