"""Decoder attention maps through the public interface: `Detector.predict(with_attention=True)`, `Detector.saliency`,
`harness.saliency_guide`, and training with `patch_mask.type: guide` against the reference."""
import numpy as np
import pytest
import torch

from dfd_clip_amd import harness
from tests.attnmap_cases import (ATTNMAP_CASES, GUIDE_CASE, KERNEL_ATOL, KERNEL_RTOL, attention_map, build_guide_case,
                                 load_attnmap_golden, worst)
from tests.cases import EXTRA_INPUTS, build_case, load_golden

pytestmark = pytest.mark.gpu


def make_detector(case, precision):
    from dfd_clip_amd.detector import Detector
    det = Detector(case["cfg"], case["T"], None, precision=precision)
    det.load_state_dict(case["sd"])
    return det.to("cuda").eval()


def record_map_calls(monkeypatch):
    """What each `capi.decoder_attn_map` launch of the decoder read: (q, the keys as f32 with `pos` added, ext_weights)."""
    from dfd_clip_amd import capi
    real, calls = capi.decoder_attn_map, []

    def spy(q, k, frame_mask, stats, aff, B, T, patches, heads, d=64, ext_weights=None, branches=None, pos=None):
        kk = k.float().reshape(B, T, patches, heads * d)
        if pos is not None:
            kk = kk + pos.view(1, T, 1, heads * d)
        calls.append((q.clone().view(B, heads, 2 * d).cpu(), kk.reshape(B, T * patches, heads * d).cpu(), k.is_contiguous()))
        return real(q, k, frame_mask, stats, aff, B, T, patches, heads, d, ext_weights=ext_weights, branches=branches, pos=pos)
    monkeypatch.setattr(capi, "decoder_attn_map", spy)
    return calls


@pytest.mark.parametrize("in_place", [True, False])
@pytest.mark.parametrize("name", ATTNMAP_CASES)
def test_predict_attention_fp32_matches_the_reference(name, in_place, monkeypatch):
    """fp32: the maps against the reference's own weights at 1e-5 (the bar of the tiny variants), on the in-place and the
    export path; the logits are the bits of the call without maps."""
    case, g = build_case(name), load_attnmap_golden(name)
    det = make_detector(case, "fp32")
    det.kv_in_place = in_place
    x, m = case["x"].cuda(), case["m"].cuda()
    calls = record_map_calls(monkeypatch)
    with torch.no_grad():
        plain, f0 = det.predict(x, m)
        logits, features = det.predict(x, m, with_attention=True)
    assert "attention" not in f0 and len(calls) == len(case["layer_indices"]) and all(c[2] != in_place for c in calls)
    assert torch.equal(plain[0].view(torch.int32), logits[0].view(torch.int32))
    B, T, H = case["B"], case["T"], case["heads"]
    att = features["attention"]
    assert len(att) == len(case["layer_indices"])
    for i, a in enumerate(att):
        assert a.shape == (B, H, T, g["aff"].shape[-1] // T) and a.dtype == torch.float32
        err = (a.reshape(B, H, -1).double().cpu() - torch.from_numpy(g["aff"][i]).double()).abs().max().item()
        print(f"{name} in_place={in_place} block {i}: worst |aff - reference| {err:.3e}")
        assert err <= 1e-5, (name, i, err)
    for a in att:  # padded frames weigh nothing
        assert (a.permute(0, 2, 1, 3)[~m] == 0).all()


@pytest.mark.parametrize("name", ATTNMAP_CASES)
def test_predict_attention_bf16(name, monkeypatch):
    """bf16: against the restatement on the bf16-rounded keys (and the q) the decoder read, at the kernel bar."""
    case = build_case(name)
    det = make_detector(case, "bf16")
    x, m = case["x"].cuda(), case["m"].cuda()
    calls = record_map_calls(monkeypatch)
    with torch.no_grad():
        plain, _ = det.predict(x, m)
        logits, features = det.predict(x, m, with_attention=True)
    assert torch.equal(plain[0].view(torch.int32), logits[0].view(torch.int32))
    modes = ("frame", "temporal") if name == "tiny_attnmode" else ()
    for i, (a, (q, kk, _)) in enumerate(zip(features["attention"], calls)):
        want = attention_map(q, kk, case["m"], case["T"], modes)
        err, over = worst(a.reshape(want.shape), want)
        print(f"{name} bf16 block {i}: worst |err| {err:.3e}")
        assert over <= 0, f"block {i}: {err:.3e} exceeds atol {KERNEL_ATOL} + rtol {KERNEL_RTOL}"


def test_saliency_shape_and_head_reduction():
    case = build_case("tiny")
    det = make_detector(case, "fp32")
    x, m = case["x"].cuda(), case["m"].cuda()
    with torch.no_grad():
        _, features = det.predict(x, m, with_attention=True)
    a = torch.stack(features["attention"], dim=1)  # [B, L, H, T, P]
    g = case["res"] // case["patch"]
    for reduce, want in (("mean", a.mean(dim=2)), ("max", a.amax(dim=2))):
        s = det.saliency(x, m, reduce=reduce)
        assert s.shape == (case["B"], len(case["layer_indices"]), case["T"], g, g)
        assert torch.equal(s.reshape(want.shape), want)
    with pytest.raises(ValueError):
        det.saliency(x, m, reduce="sum")


def test_saliency_guide_over_two_batches(tmp_path):
    case = build_case("tiny")
    det = make_detector(case, "fp32")
    x, m = case["x"].cuda(), case["m"].cuda()
    guide = harness.saliency_guide(det, [(x, m), (x.flip(0), m.flip(0))])
    v = guide["v"]
    g = case["res"] // case["patch"]
    assert v.dtype == np.float64 and v.shape == (case["layers"], g, g) and np.isfinite(v).all() and (v >= 0).all()
    assert np.allclose(v.reshape(len(v), -1).sum(1), 1.0, rtol=0, atol=1e-12)
    for l in range(case["layers"]):
        if l not in case["layer_indices"]:
            assert np.array_equal(v[l], np.full((g, g), 1.0 / (g * g)))
        np.random.choice(range(g * g), g * g // 2, replace=False, p=v[l].flatten())
    assert any(v[l].std() > 0 for l in case["layer_indices"])
    # both batches hold the same clips: the average over them is one batch's map
    one = harness.saliency_guide(det, [(x, m)])["v"]
    assert np.allclose(v, one, rtol=0, atol=1e-6)
    harness.save_guide(tmp_path / "g.npz", guide)
    assert np.array_equal(harness.load_guide(tmp_path / "g.npz")["v"], v)


def test_patch_mask_guide_training_matches_the_reference(tmp_path):
    """`tiny_pmask_guide` under the contract and at the tolerances of test_hip_backward.py's `tiny_pmask` case
    (test_training_extras_match_reference) and its two SGD steps (test_train_step_contract_matches_reference), NumPy
    seeded as the reference run was (np_seed + step)."""
    g = load_golden(GUIDE_CASE)
    path = tmp_path / "guide.npz"
    harness.save_guide(path, {"v": g["guide_v"]})
    case = build_guide_case(path)
    det = make_detector(case, "fp32")
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    with torch.no_grad():
        losses, logits = det(x, [y], m, single_task=0)
    np.testing.assert_allclose(logits[0].cpu().numpy(), g["logits"], atol=1e-4)
    np.testing.assert_allclose(losses[0].cpu().numpy(), g["losses"], atol=1e-4)
    det.train()
    opt = det.configure_optimizers(0.01)
    speed = torch.tensor(EXTRA_INPUTS["speed"], device="cuda")
    step_losses = []
    for step in range(2):
        opt.zero_grad()
        np.random.seed(EXTRA_INPUTS["np_seed"] + step)
        tl, tz, other = det(x, [y], m, EXTRA_INPUTS["comp"], speed, train=True, single_task=0)
        loss = tl[0].mean() + sum(other.values())
        loss.backward()
        if step == 0:
            np.testing.assert_allclose(tl[0].detach().cpu().numpy(), g["train_task_loss"], atol=1e-4)
            for k_, v_ in other.items():
                np.testing.assert_allclose(v_.item(), g["other." + k_], atol=1e-5, err_msg=k_)
            assert {("other." + k_) for k_ in other} == {f for f in g.files if f.startswith("other.")}
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
                checked += 1
            assert checked > 20
        step_losses.append(loss.item())
        opt.step()
    print("step losses", step_losses, "reference", g["step_losses"].tolist())
    np.testing.assert_allclose(step_losses, g["step_losses"], atol=2e-4)
    for pn, p in det.named_parameters():
        if not p.requires_grad:
            continue
        t = p.detach().float().cpu()
        if "after2." + pn in g.files:
            np.testing.assert_allclose(t.numpy(), g["after2." + pn], atol=2e-5, rtol=0, err_msg=pn)
        else:
            np.testing.assert_allclose(t.flatten()[:64].numpy(), g["after2." + pn + ".head"], atol=2e-5, rtol=0, err_msg=pn)
