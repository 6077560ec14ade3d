"""GPU parity of the DINOv2 towers beside ViT-B/14: `dino_tiny_swiglu`, `dino_s2` and `dino_g2` (ViT-g/14's width, heads,
SwiGLU feed-forward and 257 tokens, two layers) against the reference's own results (tests/golden/dinov2_family_*.npz,
tools/gen_golden_dinov2_family.py) — the tower's per-block q / k / v / out, `Detector` logits, losses, every decoder
gradient, two SGD steps — the bf16 path against the reference's own bf16 deviation, the invariants of the real-width
geometry, which GEMM kernels its feed-forward runs on, and ViT-L/14's width at bf16 and fp8."""
import copy

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from tests.dinov2_family_cases import CASES, build_case, load_golden

pytestmark = pytest.mark.gpu

TOWER_TOL = 5e-4   # per-block q / k / v / out, fp32 (the K/V bar of tests/test_hip_anytok_detector.py)
LOGIT_TOL = 1e-3   # fp32 logits (tests/test_hip_detector.py)
LOSS_TOL = 1e-4


@pytest.fixture(scope="module")
def cases():
    return {name: build_case(name) for name in CASES}


def make_detector(case, precision):
    from dfd_clip_amd.detector import Detector
    det = Detector(case["cfg"], case["T"], None, precision=precision)
    res = det.load_state_dict(case["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return det.to("cuda").eval()


@pytest.mark.parametrize("name", list(CASES))
def test_fp32_tower_logits_and_losses_match_reference(cases, name):
    case, g = cases[name], load_golden(name)
    det = make_detector(case, "fp32")
    frames = case["x"].flatten(0, 1).cuda()
    got = det.encoder(frames, feat_keys=["q", "k", "v", "out"])
    tokens = (case["res"] // case["patch"]) ** 2 + 1
    assert len(got) == case["layers"] and tuple(got[0]["k"].shape) == (frames.shape[0], tokens, case["heads"], 64)
    rows = g["stored_rows"].tolist() if "stored_rows" in g.files else list(range(tokens))
    worst = 0.0
    for l in range(case["layers"]):
        for key in ("q", "k", "v", "out"):
            err = np.abs(got[l][key][:, rows].float().cpu().numpy() - g[f"enc{l}_{key}"]).max()
            print(f"{name}/fp32: enc{l}_{key} max |d| = {err:.3e}")
            worst = max(worst, err)
    assert worst <= TOWER_TOL
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    with torch.no_grad():
        losses, logits = det(x, [y], m, single_task=0)
        plog, feats = det.predict(x, m, with_video_features=True)
    err = np.abs(logits[0].cpu().numpy() - g["logits"]).max()
    lerr = np.abs(losses[0].cpu().numpy() - g["losses"]).max()
    print(f"{name}/fp32: max |dlogit| = {err:.3e}, max |dloss| = {lerr:.3e}")
    assert err <= LOGIT_TOL and lerr <= LOSS_TOL
    assert torch.equal(plog[0], logits[0])
    np.testing.assert_allclose(feats["video"].cpu().numpy(), g["video_feature"], atol=2 * LOGIT_TOL, rtol=0)


@pytest.mark.parametrize("name", list(CASES))
def test_bf16_logits_within_the_references_own_bf16_deviation(cases, name):
    """|hip - ref_fp32| <= 2 * |ref_bf16 - ref_fp32|max + 1e-2: both reference figures are the fixture's (the reference under
    torch.autocast(bfloat16) on the CPU), none comes from the code under test."""
    case, g = cases[name], load_golden(name)
    det = make_detector(case, "bf16")
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    with torch.no_grad():
        _, logits = det(x, [y], m, single_task=0)
    got = logits[0].float().cpu().numpy()
    ref_dev = np.abs(g["logits_bf16"] - g["logits"]).max()
    d32 = np.abs(got - g["logits"]).max()
    print(f"{name}/bf16: |hip - ref_fp32| = {d32:.3e}   |ref_bf16 - ref_fp32| = {ref_dev:.3e}   bar = {2 * ref_dev + 1e-2:.3e}")
    assert np.isfinite(got).all()
    assert d32 <= 2 * ref_dev + 1e-2


@pytest.mark.parametrize("name", list(CASES))
def test_train_step_contract_matches_reference(cases, name):
    """fp32: the train-forward losses, every decoder gradient within 1e-3 of its tensor's max, then two SGD steps (the bars
    of tests/test_hip_dinov2.py / test_hip_backward.py)."""
    case, g = cases[name], load_golden(name)
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
            np.testing.assert_allclose(task_losses[0].detach().cpu().numpy(), g["train_task_loss"], atol=LOSS_TOL, rtol=0)
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
    print(f"{name}: step losses {step_losses} (reference {g['step_losses'].tolist()})")
    np.testing.assert_allclose(step_losses, g["step_losses"], atol=2e-4)
    for pn, p in det.named_parameters():
        if p.requires_grad:
            t = p.detach().float().cpu()
            if "after2." + pn in g.files:
                np.testing.assert_allclose(t.numpy(), g["after2." + pn], atol=2e-5, rtol=0, err_msg=pn)
            else:
                np.testing.assert_allclose(t.flatten()[:64].numpy(), g["after2." + pn + ".head"], atol=2e-5, rtol=0, err_msg=pn)


def test_adamw_step_on_the_swiglu_tower(cases):
    """The fused AdamW step serves a Detector on a SwiGLU tower as it does any other: finite, and the loss falls."""
    case = cases["dinov2_family_tiny_swiglu"]
    cfg = case["cfg"].clone()
    cfg.optimizer = "adamw"
    det = make_detector(dict(case, cfg=cfg), "fp32").train()
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    opt = det.configure_optimizers(0.01)
    seen = []
    for _ in range(3):
        opt.zero_grad()
        tl, _, other = det(x, [y], m, train=True, single_task=0)
        loss = tl[0].mean() + sum(other.values())
        loss.backward()
        opt.step()
        seen.append(loss.item())
    assert all(np.isfinite(seen)) and seen[-1] < seen[0], seen


# ---- dino_g2: ViT-g/14's real width ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g2(cases):
    """Two clips of two frames: 1028 rows, what the tuned GEMMs serve (M >= 1024)."""
    from dfd_clip_amd.weights import synthetic_clips
    case = cases["dinov2_family_g2"]
    x, m, y = synthetic_clips(2, case["T"], case["res"], seed=77, masked_tail=False)
    return dict(case=case, x=x.cuda(), m=m.cuda(), y=y.cuda())


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_g2_permutation_and_frame_chunking(g2, precision):
    det = make_detector(g2["case"], precision)
    x, m = g2["x"], g2["m"]
    with torch.no_grad():
        base = det.predict(x, m)[0][0].clone()
        assert torch.isfinite(base).all()
        perm = torch.tensor([1, 0], device="cuda")
        assert torch.equal(det.predict(x[perm].contiguous(), m[perm].contiguous())[0][0], base[perm]), "clips are not independent"
        for chunk in (1, 2):
            det.encoder.frame_chunk = chunk
            assert torch.equal(det.predict(x, m)[0][0], base), f"frame chunk {chunk} changed the result"
        det.encoder.frame_chunk = 0


@pytest.mark.parametrize("in_place", [True, False])
def test_g2_graph_replay_equals_eager(g2, in_place):
    """The pipelined encoder replayed as one HIP graph (x12 and hidden are workspace buffers the graph is guarded by)."""
    det = make_detector(g2["case"], "bf16")
    det.kv_in_place = in_place
    x, m = g2["x"], g2["m"]
    with torch.no_grad():
        want = det.predict(x, m)[0][0].clone()
    guard = det.encoder.graph_guard(x.shape[0] * x.shape[1])
    assert guard[2]["x12"].shape[1] == 8192 and guard[2]["hidden"].shape[1] == 4096 and guard[2]["u"] is None
    gdet = copy.deepcopy(det)
    gdet.pipeline_encoder, gdet.inputs_ready, gdet.static_graphs = True, True, True
    torch.cuda.synchronize()
    with torch.no_grad():
        for i in range(4):  # two K/V sets alternate: each (input, set) pair is captured at its second sighting
            assert torch.equal(gdet.predict(x, m)[0][0], want), f"in_place={in_place} pass {i}"
    assert gdet._enc_graphs_failed is None
    assert (len(gdet._enc_graphs) >= 1) == in_place, "the encoder pass is replayed as a graph exactly when K/V stay in place"


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_g2_kv_in_place_matches_the_export_path(g2, precision):
    """The bars of tests/test_hip_anytok_detector.py::test_small24_kv_in_place_matches_the_export_path."""
    x, m, y = g2["x"], g2["m"], g2["y"]
    outs = []
    for in_place in (True, False):
        det = make_detector(g2["case"], precision).train()
        det.seed_dropout(123)
        det.kv_in_place = in_place
        det.zero_grad(set_to_none=True)
        losses, logits, other = det(x, [y], m, train=True, single_task=0)
        (losses[0].mean() + sum(other.values())).backward()
        grads = {n: p.grad.clone() for n, p in det.named_parameters() if p.grad is not None}
        outs.append((logits[0].detach(), grads))
    (la, ga), (lb, gb) = outs
    assert ga.keys() == gb.keys() and len(ga) > 10
    print(f"g2/{precision}: in place vs export max |dlogit| = {(la - lb).abs().max().item():.3e}")
    assert (la - lb).abs().max().item() <= (1e-5 if precision == "fp32" else 3e-2)
    for n in ga:
        scale = max(gb[n].abs().max().item(), 1e-6)
        assert (ga[n] - gb[n]).abs().max().item() <= (1e-4 if precision == "fp32" else 5e-2) * scale, n


def test_g2_feed_forward_runs_on_the_tuned_gemms(g2, monkeypatch):
    """bf16, 1028 rows: w12 (N = 8192, K = 1536) and w3 (N = 1536, K = 4096) must not fall to the general kernel, and the gate
    between them takes its 16-byte form."""
    det = make_detector(g2["case"], "bf16")
    seen, gates = [], []
    real_gemm, real_gate = capi.gemm, capi.swiglu_fwd

    def gemm(a, w, c, *args, **kw):
        out = real_gemm(a, w, c, *args, **kw)
        seen.append((tuple(w.shape), capi.gemm_last_kernel()))
        return out

    def gate(x12, hidden):
        out = real_gate(x12, hidden)
        gates.append((tuple(x12.shape), tuple(hidden.shape), capi.swiglu_last_path()))
        return out

    monkeypatch.setattr(capi, "gemm", gemm)
    monkeypatch.setattr(capi, "swiglu_fwd", gate)
    frames = g2["x"].flatten(0, 1)
    det.encoder(frames)
    w12 = [k for shp, k in seen if shp == (8192, 1536)]
    w3 = [k for shp, k in seen if shp == (1536, 4096)]
    assert len(w12) == 2 and len(w3) == 2, seen
    assert all(k in (capi.GEMM_PINGPONG, capi.GEMM_PERSISTENT, capi.GEMM_TILE) for k in w12 + w3), (w12, w3)
    assert gates == [((1028, 8192), (1028, 4096), capi.SWIGLU_VEC16)] * 2, gates
    assert not any(shp[0] == 4 * 1536 for shp, _ in seen), "a SwiGLU layer has no fc1"


@pytest.mark.parametrize("precision", ["bf16", "fp8"])
def test_vitl14_width_two_layer_cut(monkeypatch, precision):
    """dinov2_vitl14's width, heads and 257 tokens with two of its 24 layers, seeded weights, 2 clips x 2 frames: finite,
    clips independent; fp8 and its policy go through the code ViT-B/14 uses."""
    from dfd_clip_amd import weights
    from dfd_clip_amd.detector import Detector
    from tests.dinov2_cases import make_config
    res, patch, width, layers, heads, od = weights.ARCHS["dinov2_vitl14"]
    monkeypatch.setitem(weights.ARCHS, "dino_l2", (res, patch, width, 2, heads, od))
    monkeypatch.setitem(weights.DINO_IMG_SIZE, "dino_l2", 518)
    monkeypatch.setitem(weights.DINO_FFN, "dino_l2", "mlp")
    cfg = make_config("dino_l2", decode_mode="index", decode_indices=[0, 1])
    B, T = 2, 2
    kw = dict(fp8_policy="kv-bf16") if precision == "fp8" else {}
    det = Detector(cfg, T, None, precision=precision, **kw)
    det.load_state_dict(weights.random_state_dict(cfg, T, seed=0), strict=True)
    det = det.cuda().eval()
    assert (det.encoder.width, det.encoder.heads, det.encoder.tokens, det.encoder.ffn) == (1024, 16, 257, "mlp")
    x, m, _ = weights.synthetic_clips(B, T, res, seed=5, masked_tail=False)
    x, m = x.cuda(), m.cuda()
    with torch.no_grad():
        if precision == "fp8":
            det.encoder.calibrate_fp8(x.flatten(0, 1))
            assert det.encoder.fp8_policy()[0]["qkv"] == "kv-bf16"
        base = det.predict(x, m)[0][0].clone()
        assert torch.isfinite(base).all()
        perm = torch.tensor([1, 0], device="cuda")
        assert torch.equal(det.predict(x[perm].contiguous(), m[perm].contiguous())[0][0], base[perm]), "clips are not independent"
