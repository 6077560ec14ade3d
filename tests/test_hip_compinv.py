"""Adapter pre-training on the GPU: the pair-loss kernels (dfd_compinv_loss_fwd / _bwd) against float64 math, and
`CompInvEncoder` against what the reference's own class computed (tests/golden/compinv_*.npz)."""
import copy

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from tests.compinv_cases import CASES, LR, MAX_STEPS, build_case, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def loss_ref(k, v, B, T, P):
    """float64 restatement of the pair loss on packed [L, B*T*P, D] -> (M, match, dk, dv) for d match = 1."""
    k = k.detach().double().requires_grad_(True)
    v = v.detach().double().requires_grad_(True)
    L, _, D = k.shape
    w = B // 2
    s = 0
    for t in (k, v):
        a = t.view(L, B, T * P, D)
        s = s + (a[:, 0:2 * w:2] - a[:, 1:2 * w:2]).abs().sum((0, 1))
    M = (s / (w * L * 2)).view(P, T, D).mean(1)
    match = M.norm() / P
    match.backward()
    return M.detach(), match.detach(), k.grad, v.grad


def run_kernels(k, v, B, T, P, grad=1.0):
    D = k.shape[-1]
    f32 = dict(device=k.device, dtype=torch.float32)
    ws = torch.empty(-(-capi.compinv_loss_workspace_bytes(P, D) // 4), **f32)
    match, norm, recon = torch.empty((), **f32), torch.empty((), **f32), torch.full((), 7.0, **f32)
    capi.compinv_loss_fwd(k, v, B, T, P, ws, match, norm, recon)
    g = torch.full((1,), grad, **f32)
    dk, dv = torch.full_like(k, 3.0), torch.full_like(v, 3.0)
    capi.compinv_loss_bwd(k, v, B, T, P, ws, norm, g, dk, dv)
    torch.cuda.synchronize()
    return ws[:P * D].view(P, D).clone(), match, norm, recon, dk, dv


# (B, L, P, T, D): every value of B {2, 5, 10}, L {1, 6}, P {4, 196, 256}, T {1, 3, 50}, D {128, 768, 1024} appears
SHAPES = [(2, 1, 4, 1, 128), (5, 6, 196, 3, 768), (10, 1, 196, 50, 768), (5, 6, 4, 50, 1024), (2, 6, 256, 3, 128),
          (10, 6, 256, 1, 1024), (5, 1, 256, 50, 768)]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("shape", SHAPES)
def test_loss_kernels_against_f64(shape, dtype):
    B, L, P, T, D = shape
    gen = torch.Generator(device=DEV).manual_seed(sum(shape))
    k = torch.randn(L, B * T * P, D, device=DEV, generator=gen).to(dtype)
    v = torch.randn(L, B * T * P, D, device=DEV, generator=gen).to(dtype)
    # exact ties (sign 0) in a few places: copy one member of pair 0 onto the other in frame 0's first rows
    k.view(L, B, T * P, D)[:, 1, :2] = k.view(L, B, T * P, D)[:, 0, :2]
    M, match, norm, recon, dk, dv = run_kernels(k, v, B, T, P, grad=0.75)
    Mr, matchr, dkr, dvr = loss_ref(k, v, B, T, P)
    assert recon.item() == 0.0
    assert abs(match.item() - matchr.item()) <= 1e-5 * matchr.item()
    assert abs(norm.item() - matchr.item() * P) <= 1e-5 * matchr.item() * P
    assert (M.double() - Mr).abs().max().item() <= 1e-5 * Mr.abs().max().item()
    for got, ref in ((dk, dkr * 0.75), (dv, dvr * 0.75)):
        err = (got.double() - ref).abs()
        if dtype == torch.float32:
            assert err.max().item() <= 1e-5 * ref.abs().max().item()
        else:  # the gradient is stored in bf16: one rounding of the f64 value (2^-9 relative) plus the f32 path
            assert (err <= 2.0 ** -8 * ref.abs() + 1e-5 * ref.abs().max()).all()
        assert torch.equal(got == 0, ref == 0) or dtype == torch.bfloat16
    if B % 2:  # the odd last clip takes no part: zero rows
        for got in (dk, dv):
            assert torch.count_nonzero(got.view(L, B, -1)[:, B - 1]).item() == 0
    # bit-identical on a second call, and with the two members of every pair swapped
    M2, match2, _, _, dk2, dv2 = run_kernels(k, v, B, T, P, grad=0.75)
    assert torch.equal(M, M2) and torch.equal(match, match2) and torch.equal(dk, dk2) and torch.equal(dv, dv2)
    w = B // 2
    perm = list(range(B))
    for i in range(w):
        perm[2 * i], perm[2 * i + 1] = perm[2 * i + 1], perm[2 * i]
    ks = k.view(L, B, -1)[:, perm].reshape_as(k).contiguous()
    vs = v.view(L, B, -1)[:, perm].reshape_as(v).contiguous()
    M3, match3, _, _, dk3, dv3 = run_kernels(ks, vs, B, T, P, grad=0.75)
    assert torch.equal(M, M3) and torch.equal(match, match3)
    assert torch.equal(dk3, dk.view(L, B, -1)[:, perm].reshape_as(dk))
    assert torch.equal(dv3, dv.view(L, B, -1)[:, perm].reshape_as(dv))


def test_loss_kernels_zero_norm_gives_zero_gradient():
    k = torch.randn(2, 2 * 3 * 4, 128, device=DEV)
    k.view(2, 2, -1)[:, 1] = k.view(2, 2, -1)[:, 0]
    M, match, norm, _, dk, dv = run_kernels(k, k.clone(), 2, 3, 4)
    assert match.item() == 0.0 and norm.item() == 0.0
    assert torch.count_nonzero(dk).item() == 0 and torch.count_nonzero(dv).item() == 0
    assert not torch.isnan(dk).any()


# ---- the model against the reference's own class --------------------------------------------------------------------

def make_model(name, precision="fp32", mode=1):
    from dfd_clip_amd.compinv import CompInvEncoder
    case = build_case(name, mode)
    model = CompInvEncoder(case["cfg"], None, num_frames=case["T"], precision=precision)
    model.load_state_dict(case["sd"])
    return model.to(DEV), case


def grad_scale(g):
    return max(float(np.abs(g[k]).max()) for k in g.files if k.startswith("grad_m") and not k.endswith(".norm"))


def check_tensor(got, g, key, tol, floor):
    """`got` against the fixture entry `key` (whole tensor, or .norm + .head): |d| <= tol * max(|ref|max, floor)."""
    got = got.detach().float().cpu()
    if key in g.files:
        ref = torch.from_numpy(g[key])
        assert (got - ref).abs().max().item() <= tol * max(ref.abs().max().item(), floor), key
    else:
        ref_n = float(g[key + ".norm"])
        assert abs(got.norm().item() - ref_n) <= tol * max(ref_n, floor), key
        head = torch.from_numpy(g[key + ".head"])
        assert (got.flatten()[:64] - head).abs().max().item() <= tol * max(head.abs().max().item(), floor), key


def losses_and_grads(model, case, comp):
    model.zero_grad()
    model.eval()
    recon, match = model(case["x"].to(DEV), comp)
    (recon + match).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.requires_grad}
    return recon.detach(), match.detach(), grads


@pytest.mark.parametrize("name", list(CASES))
def test_model_fp32_matches_reference(name):
    g = load_golden(name)
    scale = grad_scale(g)
    results = {}
    for mode in (0, 1):
        model, case = make_model(name, "fp32", mode)
        for tag, comp in (("str", case["comp"]), ("lab", case["labels"])):
            recon, match, grads = losses_and_grads(model, case, comp)
            assert recon.item() == 0.0 == float(g[f"recon_m{mode}_{tag}"])
            ref = float(g[f"match_m{mode}_{tag}"])
            assert abs(match.item() - ref) <= 1e-5 * ref, (mode, tag, match.item(), ref)
            for n, t in grads.items():
                check_tensor(t, g, f"grad_m{mode}.{n}", 1e-3, 1e-2 * scale)
            results[(mode, tag)] = (match, grads)
    # mode 0 and mode 1, comp strings and the labels tensor: the same bits
    base_m, base_g = results[(1, "str")]
    for key, (m, gr) in results.items():
        assert torch.equal(m, base_m), key
        assert all(torch.equal(gr[n], base_g[n]) for n in base_g), key


# the reference's own bf16 autocast run against its fp32 run differs by ~1e-4 relative here; the bf16 HIP path against
# that autocast run: 2x the error measured on MI355X (tiny 1.82e-4, small 1.15e-5 relative; deterministic kernels)
BF16_MATCH_RTOL = {"compinv_tiny": 3.7e-4, "compinv_small": 2.3e-5}


@pytest.mark.parametrize("name", list(CASES))
def test_model_bf16_matches_reference_autocast(name):
    g = load_golden(name)
    model, case = make_model(name, "bf16")
    for mode in (0, 1):
        model.mode = mode
        with torch.no_grad():
            recon, match = model(case["x"].to(DEV), case["comp"])
        ref = float(g[f"match_bf16_m{mode}"])
        err = abs(match.item() - ref) / ref
        print(f"{name} bf16 mode {mode}: match {match.item():.6g} vs autocast {ref:.6g}: rel {err:.2e}")
        assert recon.item() == 0.0
        assert err <= BF16_MATCH_RTOL[name], (err, BF16_MATCH_RTOL[name])


def adapter_params(model):
    return {n: p.detach().clone() for n, p in model.named_parameters() if p.requires_grad}


def two_steps(model, case, graphs=False):
    from dfd_clip_amd.harness import compinv_train_step, make_one_cycle
    model.use_graphs = graphs
    opt = model.configure_optimizers(LR / 25)
    sched = make_one_cycle(opt, LR, MAX_STEPS, num_processes=1)
    x = case["x"].to(DEV)
    outs = [compinv_train_step(model, opt, [(x, case["labels"])], sched) for _ in range(2)]
    torch.cuda.synchronize()
    return outs


@pytest.mark.parametrize("name", list(CASES))
def test_two_train_steps_match_reference(name):
    g = load_golden(name)
    model, case = make_model(name, "fp32")
    before = adapter_params(model)
    outs = two_steps(model, case)
    for s in range(2):
        assert outs[s]["recon"][0].item() == 0.0
        assert abs(outs[s]["match"][0].item() - float(g["train_match"][s])) <= 1e-5 * float(g["train_match"][s])
    after = adapter_params(model)
    # AdamW moves an element by about the learning rate whatever its gradient's size, so where the gradient is rounding
    # noise in both runs (~1e-9 here: the GELU-first LayerNorm's affine parameters) the result may land anywhere within
    # 2 * (lr_1 + lr_2) of the reference.  Elements with a real gradient (above 1e-4 of the case's gradient scale,
    # first step's gradient from the fixture) agree to 1e-5.
    bound = 2 * 2 * LR / 25 * 1.1
    floor = 1e-4 * grad_scale(g)
    signal = total = 0
    for n, p in after.items():
        key, gkey = f"after2.{n}", f"grad_m1.{n}"
        ref = torch.from_numpy(g[key]) if key in g.files else torch.from_numpy(g[key + ".head"])
        gref = torch.from_numpy(g[gkey]) if gkey in g.files else torch.from_numpy(g[gkey + ".head"])
        got = p.flatten()[:ref.numel()].cpu().view_as(ref)
        d = (got - ref).abs()
        assert d.max().item() <= bound, (n, d.max().item())
        real = gref.abs() > floor
        assert (d[real] <= 1e-5).all(), (n, d[real].max().item())
        signal += int(real.sum())
        total += ref.numel()
        if key + ".norm" in g.files:
            assert abs(p.norm().item() - float(g[key + ".norm"])) <= 1e-4 * float(g[key + ".norm"]), n
        assert not torch.equal(p, before[n]), n
    assert signal >= total // 2, (signal, total)


@pytest.mark.parametrize("name", list(CASES))
def test_graph_replayed_steps_equal_eager_steps(name):
    eager, case = make_model(name, "bf16")
    graphed = copy.deepcopy(eager)
    oe = two_steps(eager, case)
    og = two_steps(graphed, case, graphs=True)
    assert graphed.adapter._graphs_failed is None
    for s in range(2):
        assert torch.equal(oe[s]["match"][0], og[s]["match"][0])
    pe, pg = adapter_params(eager), adapter_params(graphed)
    assert all(torch.equal(pe[n], pg[n]) for n in pe)


def test_evaluate_builds_no_graph_and_matches_forward():
    from dfd_clip_amd.harness import compinv_evaluate
    model, case = make_model("compinv_small", "fp32")
    x = case["x"].to(DEV)
    out = compinv_evaluate(model, [(x, case["comp"]), (x, case["labels"])])
    assert not model.training
    for t in out["recon"] + out["match"]:
        assert not t.requires_grad and t.grad_fn is None
    with torch.no_grad():
        _, match = model(x, case["comp"])
    assert torch.equal(out["match"][0], match) and torch.equal(out["match"][1], match)
    _, match_g = model(x, case["comp"])  # the autograd path (out-of-place adapter)
    assert abs(match_g.item() - match.item()) <= 1e-6 * match.item()
    assert float(load_golden("compinv_small")["match_m1_str"]) == pytest.approx(match.item(), rel=1e-5)


def test_predict_returns_the_adapted_kv_twice():
    model, case = make_model("compinv_tiny", "fp32")
    with torch.no_grad():
        kvs, _kvs = model.predict(case["x"].to(DEV))
    assert kvs is _kvs and len(kvs) == len(case["layer_indices"])
    assert tuple(kvs[0]["k"].shape) == (case["B"], case["T"], case["patches"], case["heads"], case["width"] // case["heads"])


def test_checkpoint_loads_into_detector_pretrain(tmp_path):
    from dfd_clip_amd.detector import Detector
    from tests.cases import make_config
    model, case = make_model("compinv_small", "fp32")
    two_steps(model, case)  # trained parameters, not the seed ones
    path = str(tmp_path / "compinv.pt")
    torch.save(model.state_dict(), path)
    cfg = make_config(case["arch"], decode_stride=case["cfg"].decode_stride, adapter__type="pretrain", adapter__path=path,
                      adapter__frozen=1, adapter__struct={"type": "768-x-768", "x": int(case["cfg"].adapter.struct.x)})
    det = Detector(cfg, case["T"], None, precision="fp32")
    want = model.adapter.state_dict()
    got = det.adapter.state_dict()
    assert list(got) == list(want)
    assert all(torch.equal(got[n].cpu(), want[n].cpu()) for n in want)
    det = det.to(DEV).eval()
    m = torch.ones(case["B"], case["T"], dtype=torch.bool, device=DEV)
    with torch.no_grad():
        logits, _ = det.predict(case["x"].to(DEV), m)
    torch.cuda.synchronize()
    assert torch.isfinite(logits[0]).all()
