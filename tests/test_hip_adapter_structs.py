"""The CompInvAdapter structs "768-bn", "768-xxx-768" and "linear" on the GPU: their kernels against float64 torch, the
adapter against a torch-autograd restatement (dropout masks included), `Detector` / `CompInvEncoder` against what the
reference's own classes computed (tests/golden/adapter_*.npz), HIP-graph replay and the BatchNorm's mode rules."""
import copy
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from dfd_clip_amd import capi
from tests.adapter_struct_cases import (CASES, COMPINV_CASES, COMPINV_LR, COMPINV_MAX_STEPS, build_case,
                                        build_compinv_case, load_golden)
from tests.cases import make_config

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FP32_TOL = 1e-3


def rel_err(got, ref):
    return ((got.double() - ref.double()).abs().max() / ref.double().abs().max().clamp_min(1e-30)).item()


# ---- kernels against float64 --------------------------------------------------------------------------------------

def bn_kernels(y, res, pos, gamma, beta, dout, rm, rv, nbt, B, T, P, mode, train_bwd):
    rows, D = y.shape
    frames = B * T
    f32 = dict(device=DEV, dtype=torch.float32)
    ws = torch.empty(capi.adapter_bn_workspace_bytes(frames, P, D) // 4 + 4, **f32)
    stats = torch.empty(2, T, **f32)
    capi.adapter_bn_stats(y, stats, ws, frames, P, T, mode, rm, rv, nbt)
    out = torch.empty_like(res)
    capi.adapter_bn_apply(y, out, frames, P, T, stats, gamma, beta, residual=res, pos=pos)
    dy, dg, db = torch.empty_like(y), torch.empty(T, **f32), torch.empty(T, **f32)
    capi.adapter_bn_bwd(y, dout, dy, stats, gamma, dg, db, ws, frames, P, T, train_bwd)
    torch.cuda.synchronize()
    return stats, out, dy, dg, db


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", [(2, 3, 5), (16, 30, 196)])
def test_batchnorm_kernels_against_f64(shape, dtype):
    B, T, P = shape
    D = 768
    gen = torch.Generator(device=DEV).manual_seed(B * T + P)
    y = (torch.randn(B * T * P, D, device=DEV, generator=gen) * 1.7 + 3.0).to(dtype)  # an offset: E[y²]-E[y]² would cancel
    res = torch.randn(B * T * P, D, device=DEV, generator=gen).to(dtype)
    dout = torch.randn(B * T * P, D, device=DEV, generator=gen).to(dtype)
    pos = torch.randn(T, D, device=DEV, generator=gen)
    gamma = 1 + 0.1 * torch.randn(T, device=DEV, generator=gen)
    beta = 0.1 * torch.randn(T, device=DEV, generator=gen)
    rm0, rv0 = 0.1 * torch.randn(T, device=DEV, generator=gen), 0.5 + torch.rand(T, device=DEV, generator=gen)
    for train in (True, False):
        rm, rv, nbt = rm0.clone(), rv0.clone(), torch.full((), 7, device=DEV, dtype=torch.int64)
        mode = capi.BN_TRAIN_UPDATE if train else capi.BN_EVAL
        stats, out, dy, dg, db = bn_kernels(y, res, pos, gamma, beta, dout, rm, rv, nbt, B, T, P, mode, train)
        # float64 torch: BatchNorm2d(T) on [B, T, P, D]
        yd = y.double().view(B, T, P, D).requires_grad_(True)
        g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        rm64, rv64 = rm0.double().clone(), rv0.double().clone()
        z = F.batch_norm(yd, rm64, rv64, g64, b64, training=train, momentum=0.1, eps=1e-5)
        ref = res.double().view(B, T, P, D) + z + pos.double().view(1, T, 1, D)
        ref.backward(dout.double().view(B, T, P, D))
        n = B * P * D
        mean = yd.detach().mean((0, 2, 3)) if train else rm0.double()
        var = yd.detach().var((0, 2, 3), unbiased=False) if train else rv0.double()
        assert rel_err(stats[0], mean) <= 1e-5 and rel_err(stats[1], (var + 1e-5).rsqrt()) <= 1e-5, train
        if train:
            assert rel_err(rm, rm64) <= 1e-5 and rel_err(rv, rv64) <= 1e-5 and nbt.item() == 8
            assert abs(rv64[0].item() - (0.9 * rv0[0].item() + 0.1 * var[0].item() * n / (n - 1))) < 1e-6
        else:
            assert torch.equal(rm, rm0) and torch.equal(rv, rv0) and nbt.item() == 7
        tol = 1e-5 if dtype == torch.float32 else 2.0 ** -7
        assert rel_err(out, ref.detach().view_as(out)) <= tol, (train, rel_err(out, ref.detach().view_as(out)))
        assert rel_err(dg, g64.grad) <= 1e-4 and rel_err(db, b64.grad) <= 1e-4, train
        assert rel_err(dy, yd.grad.view_as(dy)) <= (1e-4 if dtype == torch.float32 else 2.0 ** -7), train
        # a second run repeats every bit; the backward leaves the running statistics alone
        rm_a, rv_a = rm.clone(), rv.clone()
        again = bn_kernels(y, res, pos, gamma, beta, dout, rm0.clone(), rv0.clone(), nbt, B, T, P, mode, train)
        for a, b in zip((stats, out, dy, dg, db), again):
            assert torch.equal(a, b)
        if train:
            assert torch.equal(rm_a, rm) and torch.equal(rv_a, rv)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gelu_erf_kernels_against_f64(dtype):
    gen = torch.Generator(device=DEV).manual_seed(5)
    a = (3 * torch.randn(4096, 256, device=DEV, generator=gen)).to(dtype)
    dh = torch.randn(4096, 256, device=DEV, generator=gen).to(dtype)
    rng = torch.tensor([1234, 9], device=DEV, dtype=torch.int64)
    drop = capi.Dropout(rng, 77, 0.3)
    mask = capi.dropout(torch.ones(4096, 256, device=DEV), torch.empty(4096, 256, device=DEV), drop).double()
    assert 0.25 < (mask == 0).double().mean().item() < 0.35
    h = capi.gelu_erf(a, torch.empty_like(a), drop)
    da = capi.gelu_erf_bwd(a, dh, torch.empty_like(a), drop)
    ad = a.double().requires_grad_(True)
    hr = F.gelu(ad) * mask
    hr.backward(dh.double())
    tol = 2e-6 if dtype == torch.float32 else 2.0 ** -8
    assert rel_err(h, hr.detach()) <= tol and rel_err(da, ad.grad) <= max(tol, 1e-5)
    assert torch.equal(h, capi.gelu_erf(a, torch.empty_like(a), drop))


# ---- the adapter against a torch-autograd restatement (masks recovered with capi.dropout on ones) ------------------

def stub_adapter(struct, width, P, T, p, layers=2, x=64):
    from dfd_clip_amd.adapter import CompInvAdapter
    cfg = make_config("ViT-B/32", adapter__type="normal", adapter__struct={"type": struct, "x": x})
    cfg.dropout = p
    res = int(round(P ** 0.5)) * 32
    det = types.SimpleNamespace(encoder=types.SimpleNamespace(width=width, input_resolution=res, patch_size=32),
                                layer_indices=list(range(layers)))
    torch.manual_seed(3)
    ad = CompInvAdapter(cfg, det, num_frames=T)
    with torch.no_grad():
        for n, t in ad.named_parameters():
            t.add_(0.05 * torch.randn_like(t))
        for m in ad.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.1)
                m.running_var.uniform_(0.5, 1.5)
    return ad.to(DEV)


def restated(ad, k, v, pos, T, rng, training):
    """float64 torch restatement of adapter(kv) + pos; returns outputs and the parameter leaves."""
    L, rows, D = k.shape
    P = ad.patches
    B = rows // (T * P)
    base = lambda i, jj: 1000 + 4 * (2 * i + jj)  # noqa: E731

    def mask(site, p, shape):
        if rng is None or p == 0:
            return 1.0
        return capi.dropout(torch.ones(shape, device=DEV), torch.empty(shape, device=DEV), capi.Dropout(rng, site, p)).double()

    leaves, outs = {}, []
    for jj, src in enumerate((k, v)):
        o = []
        for i in range(L):
            seq = getattr(ad, f"l{i}_{'kv'[jj]}")
            P_ = {n: t.detach().double().requires_grad_(True) for n, t in seq.named_parameters()}
            leaves.update({f"l{i}_{'kv'[jj]}.{n}": t for n, t in P_.items()})
            X = src[i].double()
            mo = mask(base(i, jj) + 1, ad.drop_outer, (rows, D))
            if ad.struct == "768-bn":
                bn = seq[1]
                y = (X @ P_["0.weight"].t()).view(B, T, P, D)
                z = F.batch_norm(y, bn.running_mean.double().clone(), bn.running_var.double().clone(), P_["1.weight"],
                                 P_["1.bias"], training=training, momentum=0.1, eps=1e-5).view(rows, D)
                out = X + mo * z
            elif ad.struct == "768-xxx-768":
                h1 = F.gelu(X @ P_["0.weight"].t()) * mask(base(i, jj), ad.drop_inner, (rows, ad.inner))
                h2 = F.gelu(h1 @ P_["3.weight"].t()) * mask(base(i, jj) + 2, ad.drop_inner, (rows, ad.inner))
                out = X + mo * (h2 @ P_["6.weight"].t())
            else:
                out = mo * (X @ P_["0.weight"].t())
            o.append(out + pos.double()[None, :, None, :].expand(B, T, P, D).reshape(rows, D))
        outs.append(torch.stack(o))
    return outs, leaves


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.4])
@pytest.mark.parametrize("struct", ["768-bn", "768-xxx-768", "linear"])
def test_adapter_matches_torch_restatement(struct, p, training):
    B, T, P, D = 3, 4, 16, 768
    ad = stub_adapter(struct, D, P, T, p)
    ad.train(training)
    gen = torch.Generator(device=DEV).manual_seed(11)
    k = torch.randn(2, B * T * P, D, device=DEV, generator=gen)
    v = torch.randn(2, B * T * P, D, device=DEV, generator=gen)
    pos = 0.1 * torch.randn(T, D, device=DEV, generator=gen)
    gk, gv = torch.randn_like(k), torch.randn_like(v)
    rng = torch.tensor([99, 4], device=DEV, dtype=torch.int64) if p > 0 else None
    buf0 = {n: b.clone() for n, b in ad.named_buffers()}
    (rk, rv_), leaves = restated(ad, k, v, pos, T, rng, training)
    names = [n for n, _ in ad.named_parameters()]
    ok, ov = ad.run(k, v, T, pos, rng)
    torch.autograd.backward((ok, ov), (gk, gv))
    torch.autograd.backward((rk, rv_), (gk.double(), gv.double()))
    assert rel_err(ok, rk) <= 1e-5 and rel_err(ov, rv_) <= 1e-5
    for n, prm in zip(names, ad.parameters()):
        assert rel_err(prm.grad, leaves[n].grad) <= 1e-4, (n, rel_err(prm.grad, leaves[n].grad))
    for n, b in ad.named_buffers():  # running statistics: advanced once by a train-mode forward, never by the backward
        if n.endswith("num_batches_tracked"):
            assert b.item() == buf0[n].item() + (1 if training else 0), n
        elif not training:
            assert torch.equal(b, buf0[n]), n
        else:
            assert not torch.equal(b, buf0[n]), n


def test_frozen_batchnorm_adapter_in_train_mode_updates_its_statistics():
    ad = stub_adapter("768-bn", 768, 16, 2, 0.0)
    for prm in ad.parameters():
        prm.requires_grad = False
    ad.train()
    k = torch.randn(2, 2 * 2 * 16, 768, device=DEV)
    before = {n: b.clone() for n, b in ad.named_buffers()}
    ad.run(k, k.clone(), 2, None)  # grad mode on, nothing trainable: the in-place path
    for n, b in ad.named_buffers():
        if n.endswith("num_batches_tracked"):
            assert b.item() == before[n].item() + 1
        else:
            assert not torch.equal(b, before[n]), n
    ad.eval()
    before = {n: b.clone() for n, b in ad.named_buffers()}
    with torch.no_grad():
        ad.run(k, k.clone(), 2, None)
    assert all(torch.equal(b, before[n]) for n, b in ad.named_buffers())


# ---- Detector against the reference's own class ------------------------------------------------------------------

def make_detector(c, precision):
    from dfd_clip_amd.detector import Detector
    det = Detector(c["cfg"], c["T"], None, precision=precision)
    det.load_state_dict(c["sd"], strict=True)
    return det.to(DEV)


@pytest.mark.parametrize("name", list(CASES))
def test_detector_fp32_matches_reference(name):
    c, g = build_case(name), load_golden(name)
    det = make_detector(c, "fp32").eval()
    with torch.no_grad():
        losses, logits = det(c["x"].to(DEV), [c["y"].to(DEV)], c["m"].to(DEV), single_task=0)
    assert np.abs(logits[0].cpu().numpy() - g["logits"]).max() <= FP32_TOL
    assert np.abs(losses[0].cpu().numpy() - g["losses"]).max() <= FP32_TOL


# bf16 HIP logits against the reference's own bf16 autocast run: twice the error measured on MI355X, floor 5e-3 (the rule of
# tests/test_hip_detector.py; deterministic kernels, so the measured values repeat).  Where it exceeds that file's 5e-2
# ceiling (tiny "linear") the reference's own bf16 run is as far from its fp32 run (max|d| 3.7e-2; 3.5e-2 tiny xxx,
# 2.4e-2 ViT-B/32 bn, 5.8e-3 ViT-B/16 xxx): the spread is the toy's, not the kernels'.
BF16_MEASURED = {"adapter_tiny_xxx": 2.745e-2, "adapter_tiny_linear": 4.422e-2, "adapter_vitb16_xxx": 2.621e-3,
                 "adapter_vitb32_bn": 3.617e-2}
BF16_TOL = {k: max(2 * v, 5e-3) for k, v in BF16_MEASURED.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_detector_bf16_matches_reference_autocast(name):
    c, g = build_case(name), load_golden(name)
    det = make_detector(c, "bf16").eval()
    with torch.no_grad():
        _, logits = det(c["x"].to(DEV), [c["y"].to(DEV)], c["m"].to(DEV), single_task=0)
    err = float(np.abs(logits[0].float().cpu().numpy() - g["logits_bf16"]).max())
    print(f"{name} bf16: max|d logits| vs autocast {err:.3e}")
    assert err <= BF16_TOL[name], err


@pytest.mark.parametrize("name", list(CASES))
def test_train_step_contract_matches_reference(name):
    c, g = build_case(name), load_golden(name)
    det = make_detector(c, "fp32")
    det.train()
    x, m, y = c["x"].to(DEV), c["m"].to(DEV), c["y"].to(DEV)
    opt = det.configure_optimizers(0.01)
    step_losses = []
    for step in range(2):
        opt.zero_grad()
        task_losses, task_logits, other = det(x, [y], m, train=True, single_task=0)
        loss = task_losses[0].mean() + sum(other.values())
        loss.backward()
        if step == 0:
            if "train_logits0" in g.files:
                assert np.abs(task_logits[0].detach().cpu().numpy() - g["train_logits0"]).max() <= FP32_TOL
            for pn, p in det.named_parameters():
                if p.grad is None:
                    continue
                gr = p.grad.detach().float().cpu()
                if "grad0." + pn in g.files:
                    want = torch.from_numpy(g["grad0." + pn])
                    scale = max(want.abs().max().item(), 1e-6)
                    assert (gr - want).abs().max().item() <= 1e-3 * scale + 2e-7, (pn, (gr - want).abs().max().item(), scale)
                else:
                    np.testing.assert_allclose(gr.norm().item(), g["grad0." + pn + ".norm"], rtol=1e-3, err_msg=pn)
                    np.testing.assert_allclose(gr.flatten()[:64].numpy(), g["grad0." + pn + ".head"], rtol=2e-3,
                                               atol=2e-4 * max(float(g["grad0." + pn + ".norm"]), 1e-6) / gr.numel() ** 0.5)
        step_losses.append(loss.item())
        opt.step()
    np.testing.assert_allclose(step_losses, g["step_losses"], atol=2e-4)
    for pn, p in det.named_parameters():
        if not p.requires_grad:
            continue
        t = p.detach().float().cpu()
        if "after2." + pn in g.files:
            np.testing.assert_allclose(t.numpy(), g["after2." + pn], atol=2e-5, rtol=0, err_msg=pn)
        else:
            np.testing.assert_allclose(t.flatten()[:64].numpy(), g["after2." + pn + ".head"], atol=2e-5, rtol=0, err_msg=pn)
    if c["struct"] == "768-bn":
        for bn, b in det.named_buffers():
            if "adapter" not in bn:
                continue
            want = g["after2." + bn]
            if bn.endswith("num_batches_tracked"):
                assert b.item() == int(want) == int(c["sd"][bn]) + 2
            else:
                assert rel_err(b.cpu(), torch.from_numpy(want)) <= 1e-5, bn
        det.eval()
        with torch.no_grad():
            _, logits = det(x, [y], m, single_task=0)
        assert np.abs(logits[0].cpu().numpy() - g["logits_after2"]).max() <= FP32_TOL


# ---- graph replay and the BatchNorm's mode rules --------------------------------------------------------------------

@pytest.mark.parametrize("name", list(CASES))
def test_static_graphs_match_eager_training(name):
    from dfd_clip_amd import adapter as amod
    c = build_case(name)
    det_e = make_detector(c, "bf16")
    det_g = copy.deepcopy(det_e)
    det_g.static_graphs = True
    x, m, y = c["x"].to(DEV), c["m"].to(DEV), c["y"].to(DEV)
    opt_e, opt_g = det_e.configure_optimizers(0.01), det_g.configure_optimizers(0.01)
    for step in range(3):
        xs = x if step % 2 == 0 else x.flip(0)
        out = []
        for det, opt in ((det_e, opt_e), (det_g, opt_g)):
            det.train()
            opt.zero_grad(set_to_none=True)
            losses, logits, other = det(xs, [y], m, train=True, single_task=0)
            (losses[0].mean() + sum(other.values())).backward()
            out.append((logits[0].detach().clone(), {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None},
                        {n: b.clone() for n, b in det.named_buffers() if "adapter" in n}))
            opt.step()
        (le, ge, be), (lg, gg, bg) = out
        assert torch.equal(le, lg), step
        assert all(torch.equal(ge[n], gg[n]) for n in ge), step
        for n in be:  # the running statistics advance exactly once per replayed step
            assert torch.equal(be[n], bg[n]), (step, n)
            if n.endswith("num_batches_tracked"):
                assert bg[n].item() == int(c["sd"][n]) + step + 1
    assert len(amod._GRAPHS.get(det_g.adapter) or {}) >= 1 and not det_g.adapter._graphs_failed


def test_batchnorm_eval_is_per_clip_and_train_couples_the_batch():
    c = build_case("adapter_vitb32_bn")
    det = make_detector(c, "fp32").eval()
    x, m, y = c["x"].to(DEV), c["m"].to(DEV), c["y"].to(DEV)
    with torch.no_grad():
        both = det.predict(x, m)[0][0]
        alone = det.predict(x[:1], m[:1])[0][0]
        assert torch.equal(both[:1], alone), (both[:1] - alone).abs().max().item()
        det.train()
        both_t = det.predict(x, m)[0][0]
        alone_t = det.predict(x[:1], m[:1])[0][0]
    assert (both_t[:1] - alone_t).abs().max().item() > 1e-3


# ---- full size ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("struct", ["768-bn", "768-xxx-768", "linear"])
def test_full_size_bf16_train_step_is_finite(struct):
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    cfg = make_config("ViT-B/16", decode_mode="stride", decode_stride=2, adapter__type="normal", adapter__frozen=0,
                      adapter__struct={"type": struct, "x": 256})
    cfg.dropout = 0.5
    det = Detector(cfg, 30, None, precision="bf16")
    det.load_state_dict(random_state_dict(cfg, 30, seed=0))
    det = det.to(DEV).train()
    opt = det.configure_optimizers(0.01)
    x = torch.randn(16, 30, 3, 224, 224, device=DEV)
    m = torch.ones(16, 30, dtype=torch.bool, device=DEV)
    y = torch.arange(16, device=DEV) % 2
    losses, logits, other = det(x, [y], m, train=True, single_task=0)
    (losses[0].mean() + sum(other.values())).backward()
    opt.step()
    torch.cuda.synchronize()
    assert torch.isfinite(logits[0]).all()
    assert all(torch.isfinite(p).all() for p in det.adapter.parameters())
    assert all(torch.isfinite(b).all() for b in det.adapter.buffers())


@pytest.mark.parametrize("struct", ["768-xxx-768", "linear"])
def test_vitl14_runs(struct):
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    cfg = make_config("ViT-L/14", decode_mode="stride", decode_stride=2, adapter__type="normal", adapter__frozen=0,
                      adapter__struct={"type": struct, "x": 256})
    det = Detector(cfg, 4, None, precision="bf16")
    det.load_state_dict(random_state_dict(cfg, 4, seed=0))
    det = det.to(DEV).train()
    x = torch.randn(2, 4, 3, 224, 224, device=DEV)
    m = torch.ones(2, 4, dtype=torch.bool, device=DEV)
    losses, logits, other = det(x, [torch.arange(2, device=DEV)], m, train=True, single_task=0)
    (losses[0].mean() + sum(other.values())).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(logits[0]).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in det.adapter.parameters())


@pytest.mark.parametrize("name", list(COMPINV_CASES))
def test_compinv_batchnorm_matches_reference(name):
    from dfd_clip_amd.compinv import CompInvEncoder
    from dfd_clip_amd.harness import compinv_train_step, make_one_cycle
    c, g = build_compinv_case(name), load_golden(name)
    model = CompInvEncoder(c["cfg"], None, num_frames=c["T"], precision="fp32")
    model.load_state_dict(c["sd"], strict=True)
    model = model.to(DEV).eval()
    x = c["x"].to(DEV)
    with torch.no_grad():
        _, match = model(x, c["comp"])
    assert abs(match.item() - float(g["match"])) <= 1e-5 * float(g["match"])
    opt = model.configure_optimizers(COMPINV_LR / 25)
    sched = make_one_cycle(opt, COMPINV_LR, COMPINV_MAX_STEPS, num_processes=1)
    outs = [compinv_train_step(model, opt, [(x, c["labels"])], sched) for _ in range(2)]
    for s in range(2):
        assert abs(outs[s]["match"][0].item() - float(g["train_match"][s])) <= 1e-5 * float(g["train_match"][s]), s
    for bn, b in model.named_buffers():
        if "adapter" in bn:
            if bn.endswith("num_batches_tracked"):
                assert b.item() == int(g["after2." + bn])
            else:
                assert rel_err(b.cpu(), torch.from_numpy(g["after2." + bn])) <= 1e-5, bn
    for pn, p in model.named_parameters():
        if not p.requires_grad:  # the frozen encoder
            continue
        key = f"after2.{pn}"
        if key in g.files:
            assert (p.detach().cpu() - torch.from_numpy(g[key])).abs().max().item() <= 2e-4, pn
        else:
            assert abs(p.norm().item() - float(g[key + ".norm"])) <= 1e-4 * float(g[key + ".norm"]), pn
    model.eval()
    with torch.no_grad():
        _, match = model(x, c["comp"])
    assert abs(match.item() - float(g["match_after2"])) <= 1e-4 * float(g["match_after2"])
