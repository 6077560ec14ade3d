"""GPU parity of the DINOv2 foundation: the exact-erf GELU epilogue against float64, the tower against the reference's
own per-block results (tests/golden/dinov2_*.npz, tools/gen_golden_dinov2.py), and `Detector` with `foundation: dinov2`
— logits, loss, gradients, two SGD steps, graph replay, frame chunking, re-folding after a parameter change."""
import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from tests.dinov2_cases import BF16_MEASURED, build_case, load_golden

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3      # logits (tests/test_hip_detector.py)
FP32_LAYER_TOL = 2e-4  # per-block q / k / v / out (test_encoder_reference_api_per_layer)


def bf16_bar(key):
    """Twice what the case measured on MI355X (the kernels are deterministic, so the figure repeats), at least 5e-3."""
    return max(2 * BF16_MEASURED[key], 5e-3)


def assert_close(got, want, atol, rtol, msg):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    err = (got - want).abs()
    lim = atol + rtol * want.abs()
    assert torch.isfinite(got).all(), f"{msg}: non-finite output"
    print(f"{msg}: max err {err.max().item():.3e}, worst err / limit {(err / lim).max().item():.3f}")
    assert (err <= lim).all(), f"{msg}: max err {err.max().item():.3e} at {err.argmax().item()}"


def gelu_f64(u):
    return u * 0.5 * (1 + torch.erf(u / 2 ** 0.5))


def gelu_case(M, N, K, dtype, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    a = torch.randn(M, K, device="cuda", generator=g).to(dtype)
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5).to(dtype)
    # biases of large and small magnitude: acc ~ N(0, 1), so acc + bias covers [-8, 8] and the region around 0
    bias = torch.cat([torch.linspace(-7, 7, N // 2, device="cuda"), torch.randn(N - N // 2, device="cuda", generator=g) * 0.05])
    bias = bias[torch.randperm(N, device="cuda", generator=g)].contiguous()
    return a, w, bias


# bars: the QuickGELU epilogue's in tests/test_hip_kernels.py (test_gemm_epilogues / test_gemm_tuned_kernel_every_epilogue)
@pytest.mark.parametrize("M,N,K", [(5, 8, 32), (300, 200, 64), (514, 512, 128), (257 * 3, 3072, 768)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_gelu_epilogue_general_kernel(M, N, K, dtype):
    a, w, bias = gelu_case(M, N, K, dtype, seed=M + N)
    ref = gelu_f64(a.double() @ w.double().T + bias.double())
    c = torch.full((M, N), float("nan"), device="cuda", dtype=dtype)
    capi.gemm(a, w, c, bias, capi.EPI_BIAS_GELU)
    assert capi.gemm_last_path() == 128
    assert_close(c, ref, 1e-4, 1e-5 if dtype == torch.float32 else 2 ** -8, f"gelu {dtype} {M}x{N}x{K}")
    c2 = torch.empty_like(c)
    capi.gemm(a, w, c2, bias, capi.EPI_BIAS_GELU)
    assert torch.equal(c, c2)
    if dtype == torch.bfloat16:  # bf16 operands, f32 C: the same values before the output rounding
        cf = torch.full((M, N), float("nan"), device="cuda")
        capi.gemm(a, w, cf, bias, capi.EPI_BIAS_GELU)
        assert_close(cf, ref, 1e-4, 1e-5, "gelu, f32 out")
        assert torch.equal(cf.to(torch.bfloat16), c)


@pytest.mark.parametrize("M", [257 * 30 + 0, 257 * 16 * 30])  # ViT-B/14 fc1: one clip / the B16xT30 batch, ragged last row panel
def test_gelu_epilogue_tuned_kernel(M):
    N, K = 3072, 768
    assert M % 256 != 0 and M % 224 != 0
    a, w, bias = gelu_case(M, N, K, torch.bfloat16, seed=M)
    outs = {}
    for blocks in (8, 7, 0):  # 256-row tiles, 224-row tiles, the launcher's choice
        c = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        capi.gemm(a, w, c, bias, capi.EPI_BIAS_GELU, tile_blocks=blocks)
        assert capi.gemm_last_path() == 257, "the ViT-B/14 fc1 shape must run on the ping-pong kernel"
        outs[blocks] = c
    assert torch.equal(outs[8], outs[7]) and torch.equal(outs[8], outs[0]), "tile height changed the bits"
    again = torch.empty_like(outs[8])
    capi.gemm(a, w, again, bias, capi.EPI_BIAS_GELU, tile_blocks=8, stream_out=True)
    assert torch.equal(again, outs[8])
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = torch.cat([torch.randint(0, M, (1536,), device="cuda", generator=g), torch.arange(M - 300, M, device="cuda")])
    ref = gelu_f64(a[rows].double() @ w.double().T + bias.double())
    assert_close(outs[8][rows], ref, 1e-4, 2 ** -8, f"gelu tuned M={M}")
    # ... and the general kernel computes the same function of the same accumulator: agreement within one bf16 rounding
    # of a differently ordered f32 sum
    few = rows[:256]
    cg = torch.empty(256, N, device="cuda", dtype=torch.bfloat16)
    capi.gemm(a[few].contiguous(), w, cg, bias, capi.EPI_BIAS_GELU)
    assert capi.gemm_last_path() == 128
    assert_close(cg, ref[:256], 1e-4, 2 ** -8, "gelu general, same rows")


def make_detector(case, precision):
    from dfd_clip_amd.detector import Detector
    det = Detector(case["cfg"], case["T"], None, precision=precision)
    res = det.load_state_dict(case["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return det.to("cuda").eval()


@pytest.mark.parametrize("name", ["dinov2_tiny", "dinov2_vitb14"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_tower_matches_reference_per_block(name, precision):
    case, g = build_case(name), load_golden(name)
    det = make_detector(case, precision)
    frames = case["x"].flatten(0, 1).cuda()
    got = det.encoder(frames, feat_keys=["q", "k", "v", "out"])
    assert len(got) == case["layers"] and set(got[0]) == {"q", "k", "v", "out"}
    tokens = (case["res"] // case["patch"]) ** 2 + 1
    assert tuple(got[0]["k"].shape) == (frames.shape[0], tokens, case["heads"], 64)
    assert set(det.encoder(frames)[0]) == {"k", "v"}
    rows = g["stored_rows"].tolist() if "stored_rows" in g.files else list(range(tokens))
    worst, checked = 0.0, 0
    for l in range(case["layers"]):
        for key in ("q", "k", "v", "out"):
            if f"enc{l}_{key}" not in g.files:
                continue
            err = np.abs(got[l][key][:, rows].float().cpu().numpy() - g[f"enc{l}_{key}"]).max()
            worst, checked = max(worst, err), checked + 1
    print(f"{name}/{precision}: max |d| over {checked} per-block tensors = {worst:.3e}")
    assert checked >= 8
    assert worst <= (FP32_LAYER_TOL if precision == "fp32" else bf16_bar(name + "/tower"))


@pytest.mark.parametrize("name", ["dinov2_tiny", "dinov2_tiny_adapter", "dinov2_vitb14"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_detector_logits_match_reference(name, precision):
    case, g = build_case(name), load_golden(name)
    det = make_detector(case, precision)
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    with torch.no_grad():
        losses, logits = det(x, [y], m, single_task=0)
        plog, feats = det.predict(x, m, with_video_features=True)
    err = np.abs(logits[0].cpu().numpy() - g["logits"]).max()
    print(f"{name}/{precision}: max |dlogit| = {err:.3e}")
    tol = FP32_TOL if precision == "fp32" else bf16_bar(name + "/logits")
    assert err <= tol
    assert torch.equal(plog[0], logits[0])
    ftol = FP32_TOL if precision == "fp32" else 5e-2
    np.testing.assert_allclose(feats["video"].cpu().numpy(), g["video_feature"], atol=ftol * 2, rtol=0)
    np.testing.assert_allclose(losses[0].cpu().numpy(), g["losses"], atol=ftol * 2, rtol=0)
    # frame chunking (one clip per pass) and the export path do not change the result
    det.encoder.frame_chunk = case["T"]
    with torch.no_grad():
        chunked = det.predict(x, m)[0][0]
    assert torch.equal(chunked, logits[0])


@pytest.mark.parametrize("name", ["dinov2_tiny", "dinov2_tiny_adapter"])
def test_train_step_contract_matches_reference(name):
    """fp32: gradients of every trainable parameter, then two SGD steps (bars of tests/test_hip_backward.py)."""
    case, g = build_case(name), load_golden(name)
    det = make_detector(case, "fp32").train()
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    opt = det.configure_optimizers(0.01)
    step_losses = []
    for step in range(2):
        opt.zero_grad()
        task_losses, task_logits, other = det(x, [y], m, train=True, single_task=0)
        loss = task_losses[0].mean() + sum(other.values())
        loss.backward()
        if step == 0:
            checked = 0
            for pn, p in det.named_parameters():
                assert (p.grad is None) == pn.startswith("encoder."), pn
                if p.grad is None:
                    continue
                gr = p.grad.detach().float().cpu()
                if "grad0." + pn in g.files:
                    want = torch.from_numpy(g["grad0." + pn])
                    scale = max(want.abs().max().item(), 1e-6)
                    assert (gr - want).abs().max().item() <= 1e-3 * scale + 2e-7, (pn, (gr - want).abs().max().item(), scale)
                else:
                    np.testing.assert_allclose(gr.norm().item(), g["grad0." + pn + ".norm"], rtol=1e-3)
                    np.testing.assert_allclose(gr.flatten()[:64].numpy(), g["grad0." + pn + ".head"], rtol=2e-3,
                                               atol=2e-4 * max(float(g["grad0." + pn + ".norm"]), 1e-6) / gr.numel() ** 0.5)
                checked += 1
            assert checked > 20
        step_losses.append(loss.item())
        opt.step()
    np.testing.assert_allclose(step_losses, g["step_losses"], atol=2e-4)
    for pn, p in det.named_parameters():
        if p.requires_grad:
            t = p.detach().float().cpu()
            if "after2." + pn in g.files:
                np.testing.assert_allclose(t.numpy(), g["after2." + pn], atol=2e-5, rtol=0, err_msg=pn)
            else:
                np.testing.assert_allclose(t.flatten()[:64].numpy(), g["after2." + pn + ".head"], atol=2e-5, rtol=0, err_msg=pn)


@pytest.mark.parametrize("name", ["dinov2_tiny", "dinov2_tiny_adapter"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_static_graphs_match_eager_bit_for_bit(name, precision):
    case = build_case(name)
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    runs = []
    for graphs in (False, True):
        det = make_detector(case, precision).train()
        det.static_graphs = graphs
        opt = det.configure_optimizers(0.01)
        seen = []
        for step in range(3):  # the third step replays what the earlier ones captured
            opt.zero_grad()
            tl, tz, other = det(x, [y], m, train=True, single_task=0)
            (tl[0].mean() + sum(other.values())).backward()
            opt.step()
            seen.append(tz[0].detach().clone())
        with torch.no_grad():
            seen.append(det.eval().predict(x, m)[0][0].clone())
        runs.append(seen)
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_checkpoint_round_trip_and_refolding():
    case = build_case("dinov2_tiny")
    det = make_detector(case, "fp32")
    x, m = case["x"].cuda(), case["m"].cuda()
    with torch.no_grad():
        base = det.predict(x, m)[0][0].clone()
    sd = {k: v.cpu().clone() for k, v in det.state_dict().items()}
    assert not torch.equal(sd["encoder.backbone.blocks.0.ls1.gamma"], torch.ones(case["width"]))
    other = make_detector(dict(case, sd=sd), "fp32")
    with torch.no_grad():
        assert torch.equal(other.predict(x, m)[0][0], base)
        # a parameter written in place is picked up by the invalidation hook; stale folded weights would repeat `base`
        other.encoder.backbone.blocks[0].ls1.gamma.mul_(1.5)
        other.invalidate_caches()
        changed = other.predict(x, m)[0][0]
        assert (changed - base).abs().max().item() > 1e-4
        # load_state_dict re-folds by itself
        other.load_state_dict(sd, strict=True)
        assert torch.equal(other.predict(x, m)[0][0], base)


def test_uint8_frames_take_the_imagenet_statistics():
    case = build_case("dinov2_tiny")
    det = make_detector(case, "fp32")
    g = torch.Generator().manual_seed(3)
    raw = torch.randint(0, 256, (1, case["T"], 3, 40, 52), dtype=torch.uint8, generator=g).cuda()
    m = torch.ones(1, case["T"], dtype=torch.bool, device="cuda")
    with torch.no_grad():
        fused = det.predict(raw, m)[0][0]
        frames = det.transform(raw.flatten(0, 1))
        mean = torch.tensor((0.485, 0.456, 0.406), device="cuda").view(1, 3, 1, 1)
        std = torch.tensor((0.229, 0.224, 0.225), device="cuda").view(1, 3, 1, 1)
        assert frames.shape[-1] == case["res"] and ((frames * std + mean).min() > -1e-3) and ((frames * std + mean).max() < 1 + 1e-3)
        two_step = det.predict(frames.unflatten(0, (1, case["T"])), m)[0][0]
    assert (fused - two_step).abs().max().item() <= 1e-3


def test_fp8_is_refused_for_this_foundation():
    from dfd_clip_amd.detector import Detector
    case = build_case("dinov2_tiny")
    with pytest.raises(NotImplementedError, match="fp8"):
        Detector(case["cfg"], case["T"], None, precision="fp8")
