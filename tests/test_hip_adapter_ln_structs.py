"""The five CompInvAdapter structs with a LayerNorm ("768-x-768-nln", "-ln", "-z0", "768-x-768", "legacy-768-x-768") on
the GPU against a float64 torch-autograd restatement of adapter.py's docstring (reference models.py:795-875), dropout masks
included, in f32 and in bf16, at the (patches, x) that select each kernel of csrc/adapter.hip:
    nln (196, 256)   register-resident joint forward / backward, 7th chunk of 1024 x 8 partly filled
    nln (256, 256)   slab 65,536 > 1024 * 8 * 7: the generic joint kernels, 1024 threads
    nln (49, 64)     register path, a single partial chunk
    ln, z0 (49, 256) the row256 kernels;  (49, 64) the generic row kernels, backward with 64-thread groups
    768-x-768, legacy-768-x-768 in bf16: a1 stays in f32 beside bf16 activations (the <float, bf16_t> instantiations)

bf16: k, v and the upstream gradients are rounded to bf16 and the restatement consumes the same rounded values in float64.
The bar of a tensor is max(3 s, 3 * 2^-8) in relative L2, where s is measured on the reference side alone: the distance
between the float64 restatement and the same restatement in float32 under torch.autocast(bfloat16) with the same masks;
2^-8 is bf16's rounding unit.  The HIP path and autocast are two bf16 realisations of one computation, each about one s
from it; the HIP path rounds a few more stored tensors (a2 again after the inner dropout, da1, da2, the masked dOut), at
most doubling the roundings on a path, and independent roundings add in quadrature, which 3x covers.

Measured on MI355X, per bf16 case and kind of tensor (out = adapter(kv) + pos; the others parameter gradients, over the two
layers and k / v): smallest s / largest error, and the largest error / bar of any tensor of the case:
    case (struct, patches, x, p)        out                W_in               ln.w               ln.b               W_out              largest err / bar
    768-x-768-nln    (196, 256) p 0.0   2.4e-03 / 2.5e-03  4.0e-03 / 3.2e-03  4.1e-03 / 3.4e-03  3.2e-03 / 2.8e-03  4.0e-03 / 3.1e-03  0.27
    768-x-768-nln    (196, 256) p 0.4   3.1e-03 / 3.0e-03  4.7e-03 / 4.0e-03  4.7e-03 / 4.2e-03  4.0e-03 / 3.7e-03  4.7e-03 / 3.9e-03  0.30
    768-x-768-nln    (256, 256) p 0.0   2.3e-03 / 2.5e-03  4.0e-03 / 3.2e-03  4.1e-03 / 3.4e-03  3.2e-03 / 2.7e-03  4.0e-03 / 3.1e-03  0.27
    768-x-768-nln    (256, 256) p 0.4   3.0e-03 / 3.0e-03  4.7e-03 / 4.0e-03  4.7e-03 / 4.2e-03  4.0e-03 / 3.6e-03  4.7e-03 / 3.9e-03  0.30
    768-x-768-nln    ( 49,  64) p 0.0   1.8e-03 / 2.2e-03  4.0e-03 / 3.2e-03  4.0e-03 / 3.6e-03  3.2e-03 / 2.8e-03  4.0e-03 / 3.1e-03  0.28
    768-x-768-nln    ( 49,  64) p 0.4   2.5e-03 / 2.6e-03  4.6e-03 / 4.0e-03  4.7e-03 / 4.4e-03  4.0e-03 / 3.8e-03  4.7e-03 / 4.0e-03  0.31
    768-x-768-ln     ( 49, 256) p 0.0   2.3e-03 / 2.5e-03  4.0e-03 / 3.2e-03  5.2e-03 / 3.5e-03  5.2e-03 / 3.1e-03  4.0e-03 / 3.1e-03  0.27
    768-x-768-ln     ( 49, 256) p 0.4   3.0e-03 / 3.0e-03  4.7e-03 / 4.1e-03  5.7e-03 / 4.2e-03  5.5e-03 / 3.8e-03  4.7e-03 / 3.9e-03  0.29
    768-x-768-ln     ( 49,  64) p 0.0   1.8e-03 / 2.2e-03  4.1e-03 / 3.3e-03  5.1e-03 / 4.9e-03  5.1e-03 / 3.5e-03  4.0e-03 / 3.1e-03  0.27
    768-x-768-ln     ( 49,  64) p 0.4   2.4e-03 / 2.6e-03  4.7e-03 / 4.1e-03  5.4e-03 / 4.8e-03  5.9e-03 / 3.8e-03  4.7e-03 / 4.0e-03  0.29
    768-x-768-z0     ( 49, 256) p 0.0   1.0e-04 / 1.7e-03  3.7e-03 / 2.9e-03  5.4e-03 / 3.6e-03  5.1e-03 / 2.6e-03  3.3e-03 / 2.4e-03  0.25
    768-x-768-z0     ( 49, 256) p 0.4   1.5e-04 / 1.7e-03  4.4e-03 / 3.8e-03  6.1e-03 / 4.3e-03  5.7e-03 / 3.7e-03  4.1e-03 / 3.4e-03  0.29
    768-x-768-z0     ( 49,  64) p 0.0   4.9e-05 / 1.7e-03  3.8e-03 / 3.0e-03  5.4e-03 / 4.4e-03  4.7e-03 / 2.4e-03  3.1e-03 / 2.4e-03  0.26
    768-x-768-z0     ( 49,  64) p 0.4   7.2e-05 / 1.7e-03  4.4e-03 / 3.8e-03  5.8e-03 / 5.1e-03  5.2e-03 / 3.4e-03  4.0e-03 / 3.4e-03  0.28
    768-x-768        ( 49, 256) p 0.0   3.1e-03 / 2.7e-03  4.1e-03 / 3.3e-03  5.7e-03 / 3.2e-03  4.3e-03 / 2.6e-03  4.1e-03 / 2.6e-03  0.27
    768-x-768        ( 49, 256) p 0.4   3.7e-03 / 3.2e-03  4.7e-03 / 4.1e-03  6.2e-03 / 3.9e-03  5.0e-03 / 3.6e-03  4.7e-03 / 3.5e-03  0.29
    768-x-768        ( 49,  64) p 0.0   2.5e-03 / 2.4e-03  4.3e-03 / 3.4e-03  5.5e-03 / 3.8e-03  4.7e-03 / 3.1e-03  4.0e-03 / 2.6e-03  0.27
    768-x-768        ( 49,  64) p 0.4   3.2e-03 / 2.9e-03  4.9e-03 / 4.2e-03  5.5e-03 / 4.4e-03  4.6e-03 / 4.4e-03  4.6e-03 / 3.5e-03  0.28
    legacy-768-x-768 ( 49, 256) p 0.0   3.1e-03 / 2.7e-03  4.1e-03 / 3.3e-03  5.7e-03 / 3.2e-03  4.3e-03 / 2.6e-03  4.1e-03 / 2.6e-03  0.27
    legacy-768-x-768 ( 49, 256) p 0.4   3.5e-03 / 2.9e-03  4.4e-03 / 3.7e-03  5.8e-03 / 3.5e-03  4.7e-03 / 3.0e-03  4.4e-03 / 3.1e-03  0.28
    legacy-768-x-768 ( 49,  64) p 0.0   2.5e-03 / 2.4e-03  4.3e-03 / 3.4e-03  5.5e-03 / 3.8e-03  4.7e-03 / 3.1e-03  4.0e-03 / 2.6e-03  0.27
    legacy-768-x-768 ( 49,  64) p 0.4   2.9e-03 / 2.6e-03  4.6e-03 / 3.8e-03  5.5e-03 / 4.2e-03  5.0e-03 / 3.4e-03  4.3e-03 / 3.1e-03  0.27
"""
import pytest
import torch
import torch.nn.functional as F

from dfd_clip_amd import capi
from tests.test_hip_adapter_structs import rel_err, stub_adapter

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
L, B, T, D = 2, 2, 2, 768
SHAPES = [("768-x-768-nln", 196, 256), ("768-x-768-nln", 256, 256), ("768-x-768-nln", 49, 64),
          ("768-x-768-ln", 49, 256), ("768-x-768-ln", 49, 64), ("768-x-768-z0", 49, 256), ("768-x-768-z0", 49, 64),
          ("768-x-768", 49, 256), ("768-x-768", 49, 64), ("legacy-768-x-768", 49, 256), ("legacy-768-x-768", 49, 64)]


def masks_of(ad, rng, rows):
    """The dropout masks (0 or 1 / (1 - p), f32 on the CPU) of every (layer, tensor), recovered with capi.dropout on ones
    at the sites `CompInvAdapter._drops` uses."""
    def one(site, p, shape):
        if rng is None or p == 0:
            return None
        ones = torch.ones(shape, device=DEV)
        return capi.dropout(ones, torch.empty_like(ones), capi.Dropout(rng, site, p)).cpu()

    out = {}
    for i in range(L):
        for jj in range(2):
            base = 1000 + 4 * (2 * i + jj)
            out[(i, jj)] = (one(base, ad.drop_inner, (rows, ad.inner)), one(base + 1, ad.drop_outer, (rows, D)))
    return out


def restated(ad, k, v, pos, masks, dtype):
    """adapter(kv) + pos in plain torch on the CPU, in `dtype`; returns ([k_out, v_out], parameter leaves)."""
    rows, P, x = k.shape[1], ad.patches, ad.inner
    ln_shape = (P, x) if ad.struct.endswith("nln") else (x,)
    leaves, outs = {}, []
    posr = pos.cpu().to(dtype)[None, :, None, :].expand(B, T, P, D).reshape(rows, D)
    for jj, src in enumerate((k, v)):
        o = []
        for i in range(L):
            name = f"l{i}_{'kv'[jj]}"
            prm = {n: t.detach().cpu().to(dtype).requires_grad_(True) for n, t in getattr(ad, name).named_parameters()}
            leaves.update({f"{name}.{n}": t for n, t in prm.items()})
            w0, lw, lb = prm["0.weight"], prm[f"{ad.ln_idx}.weight"], prm[f"{ad.ln_idx}.bias"]
            w4 = prm[f"{ad.out_idx}.weight"]
            X = src[i].cpu().to(dtype)
            a1 = F.linear(X, w0).view(rows // P, P, x)
            if ad.mode == 2:  # GELU first: 768-x-768, legacy-768-x-768
                h = F.layer_norm(F.gelu(a1), ln_shape, lw, lb, 1e-5)
            else:
                h = F.gelu(F.layer_norm(a1, ln_shape, lw, lb, 1e-5))
            h = h.reshape(rows, x)
            inner, outer = masks[(i, jj)]
            if inner is not None:
                h = h * inner.to(dtype)
            y = F.linear(h, w4)
            if outer is not None:
                y = y * outer.to(dtype)
            o.append(X + y + posr)
        outs.append(torch.stack(o))
    return outs, leaves


def l2(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    return ((got - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("struct,P,x", SHAPES)
def test_layernorm_adapter_matches_torch_restatement(struct, P, x, p, dtype):
    ad = stub_adapter(struct, D, P, T, p, layers=L, x=x).train()
    rows = B * T * P
    gen = torch.Generator(device=DEV).manual_seed(11)
    k, v, gk, gv = (torch.randn(L, rows, D, device=DEV, generator=gen).to(dtype) for _ in range(4))
    pos = 0.1 * torch.randn(T, D, device=DEV, generator=gen)
    rng = torch.tensor([99, 4], device=DEV, dtype=torch.int64) if p > 0 else None
    masks = masks_of(ad, rng, rows)
    if p > 0:
        inner, outer = masks[(1, 1)]
        assert (inner is None) == (struct == "legacy-768-x-768") and 0.3 < (outer == 0).float().mean().item() < 0.5
    ok, ov = ad.run(k, v, T, pos, rng)
    torch.autograd.backward((ok, ov), (gk, gv))
    torch.cuda.synchronize()
    assert ok.dtype == dtype and ov.dtype == dtype
    got = {"out.k": ok, "out.v": ov, **{n: prm.grad for n, prm in ad.named_parameters()}}
    assert all(t is not None and torch.isfinite(t).all() for t in got.values())

    (rk, rv), leaves = restated(ad, k, v, pos, masks, torch.float64)
    torch.autograd.backward((rk, rv), (gk.cpu().double(), gv.cpu().double()))
    ref = {"out.k": rk, "out.v": rv, **{n: t.grad for n, t in leaves.items()}}
    assert sorted(ref) == sorted(got)
    if dtype == torch.float32:  # the bars of test_adapter_matches_torch_restatement
        assert rel_err(ok.cpu(), rk) <= 1e-5 and rel_err(ov.cpu(), rv) <= 1e-5
        for n in leaves:
            assert rel_err(got[n].cpu(), ref[n]) <= 1e-4, (n, rel_err(got[n].cpu(), ref[n]))
        return
    with torch.autocast("cpu", dtype=torch.bfloat16):
        (ak, av), aleaves = restated(ad, k, v, pos, masks, torch.float32)
    torch.autograd.backward((ak, av), (gk.cpu().float(), gv.cpu().float()))
    auto = {"out.k": ak, "out.v": av, **{n: t.grad for n, t in aleaves.items()}}
    failures = []
    for n in ref:
        s, e = l2(auto[n], ref[n]), l2(got[n], ref[n])
        bar = max(3 * s, 3 * 2.0 ** -8)
        print(f"{struct} P{P} x{x} p{p} {n}: s {s:.3e} err {e:.3e} err/bar {e / bar:.2f}")
        if not e <= bar:
            failures.append((n, s, e, bar))
    assert not failures, failures
