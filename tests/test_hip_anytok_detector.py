"""The whole chain at 577 tokens (24x24 patches of 14 px + cls): `small24` against the reference's own results
(tests/golden/small24.npz) with the bars of tests/test_hip_detector.py and tests/test_hip_backward.py, and
ViT-L/14@336px at its real width on random weights.  In fp32 the encoder's attention is the rows kernel with chunked
staging (295,424 B of K and V per head), in bf16 the streaming MFMA kernel."""
import numpy as np
import pytest
import torch

from tests.anytok_cases import build_case, load_golden

pytestmark = pytest.mark.gpu

FP32_TOL = 1e-3
BF16_TOL = 5e-2
KV_TOL = 5e-4


def make_detector(case, precision):
    from dfd_clip_amd.detector import Detector
    det = Detector(case["cfg"], case["T"], None, precision=precision)
    det.load_state_dict(case["sd"])
    return det.to("cuda").eval()


@pytest.fixture(scope="module")
def case():
    return build_case("small24")


def test_small24_fp32_logits_and_kv_slices(case):
    g = load_golden("small24")
    det = make_detector(case, "fp32")
    assert (det.encoder.input_resolution, det.encoder.patch_size, det.encoder.tokens) == (336, 14, 577)
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    with torch.no_grad():
        losses, logits = det(x, [y], m, single_task=0)
        plog, feats = det.predict(x, m, with_video_features=True)
    err = np.abs(logits[0].cpu().numpy() - g["logits"]).max()
    print(f"small24/fp32: max |dlogit| = {err:.3e}")
    assert err <= FP32_TOL
    assert torch.equal(plog[0], logits[0])
    np.testing.assert_allclose(feats["video"].cpu().numpy(), g["video_feature"], atol=2 * FP32_TOL, rtol=0)
    np.testing.assert_allclose(losses[0].cpu().numpy(), g["losses"], atol=2 * FP32_TOL, rtol=0)
    rows, n = list(g["slice_rows"]), case["B"] * case["T"]
    enc = det.encoder(case["x"].flatten(0, 1)[[0, n - 1]].cuda())
    for l in case["layer_indices"]:
        for key in ("k", "v"):
            for i, fr in enumerate((0, n - 1)):
                got = enc[l][key][i, rows].float().cpu().numpy()
                d = np.abs(got - g[f"enc{l}_{key}_f{fr}"]).max()
                print(f"small24/fp32: enc{l}_{key}_f{fr} max err {d:.3e}")
                assert d <= KV_TOL, (l, key, fr, d)


def test_small24_bf16_logits(case):
    g = load_golden("small24")
    det = make_detector(case, "bf16")
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    with torch.no_grad():
        _, logits = det(x, [y], m, single_task=0)
    got = logits[0].cpu().numpy()
    ref_dev = np.abs(g["logits_bf16"] - g["logits"]).max()
    d32 = np.abs(got - g["logits"]).max()
    print(f"small24/bf16: |hip - ref_fp32| = {d32:.3e}   |ref_bf16 - ref_fp32| = {ref_dev:.3e}")
    assert d32 <= BF16_TOL
    assert d32 <= ref_dev + 1e-2


def test_small24_train_step_contract(case):
    """fp32: every decoder gradient after backward(mean loss) and two SGD steps, within 1e-3 of each tensor's max."""
    g = load_golden("small24")
    det = make_detector(case, "fp32").train()
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    opt = det.configure_optimizers(0.01)
    step_losses = []
    for step in range(2):
        opt.zero_grad()
        task_losses, _, other = det(x, [y], m, train=True, single_task=0)
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
        if not p.requires_grad:
            continue
        t = p.detach().float().cpu()
        if "after2." + pn in g.files:
            np.testing.assert_allclose(t.numpy(), g["after2." + pn], atol=2e-5, rtol=0, err_msg=pn)
        else:
            np.testing.assert_allclose(t.flatten()[:64].numpy(), g["after2." + pn + ".head"], atol=2e-5, rtol=0, err_msg=pn)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_small24_kv_in_place_matches_the_export_path(case, precision):
    """Frame stride 577 * 3D of the in-place hand-over: the bars of test_kv_in_place_matches_the_export_path."""
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    outs = []
    for in_place in (True, False):
        det = make_detector(case, precision).train()
        det.seed_dropout(123)
        det.kv_in_place = in_place
        det.zero_grad(set_to_none=True)
        losses, logits, other = det(x, [y], m, train=True, single_task=0)
        (losses[0].mean() + sum(other.values())).backward()
        grads = {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None}
        outs.append((logits[0].detach(), grads))
    (la, ga), (lb, gb) = outs
    assert ga.keys() == gb.keys() and len(ga) > 10
    assert (la - lb).abs().max().item() <= (1e-5 if precision == "fp32" else 3e-2)
    for n in ga:
        scale = max(gb[n].abs().max().item(), 1e-6)
        assert (ga[n] - gb[n]).abs().max().item() <= (1e-4 if precision == "fp32" else 5e-2) * scale, n


def test_vitl14_336px_real_width_properties():
    """ViT-L/14@336px (width 1024, 24 layers, 16 heads, 577 tokens), random weights, 2 clips x 2 frames, bf16, eval."""
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    from tests.cases import make_config
    cfg = make_config("ViT-L/14@336px", decode_mode="stride", decode_stride=2)
    B, T = 2, 2
    det = Detector(cfg, T, None, precision="bf16")
    det.load_state_dict(random_state_dict(cfg, T, seed=0))
    det = det.cuda().eval()
    assert (det.encoder.width, det.encoder.layers, det.encoder.heads, det.encoder.tokens) == (1024, 24, 16, 577)
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(B, T, 3, 336, 336, device="cuda", generator=g)
    m = torch.ones(B, T, dtype=torch.bool, device="cuda")
    with torch.no_grad():
        base = det.predict(x, m)[0][0].clone()
        assert torch.isfinite(base).all()
        np.testing.assert_allclose(base.norm(dim=-1).cpu().numpy(), 5.0, atol=1e-4)
        perm = torch.tensor([1, 0], device="cuda")
        assert torch.equal(det.predict(x[perm].contiguous(), m[perm].contiguous())[0][0], base[perm]), "clips are not independent"
        for chunk in (1, 4):
            det.encoder.frame_chunk = chunk
            assert torch.equal(det.predict(x, m)[0][0], base), f"frame chunk {chunk} changed the result"
        det.encoder.frame_chunk = 0
