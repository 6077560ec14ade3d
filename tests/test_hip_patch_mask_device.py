"""Patch-masked training through `Detector.mask_gather = "device"` (one dfd_kv_gather_patches launch behind `_encode`)
against the `"torch"` arm (per-layer index_select / stack / add on the dense export): the `tiny` architecture (P = 4,
D = 128, two tapped layers), T = 4, B = 2, ratio 0.5, seeded weights and `synthetic_clips`, dropout 0.5 from one seed.

The K/V handed to the decoder or the adapter must be the same bits in both arms.  Logits and gradients must agree no worse
than two runs of the "torch" arm agree with each other on this machine — measured first; where that is zero, bit identity
is required.  The pipelined arm is held to the bar of test_hip_backward.py's pipelined tests: bit for bit."""
import copy
import functools

import numpy as np
import pytest
import torch

from dfd_clip_amd import harness
from dfd_clip_amd.weights import ARCHS, random_state_dict, resolve_layer_indices, synthetic_clips
from tests.attnmap_cases import GUIDE_CASE, build_guide_case
from tests.cases import load_golden, make_config

pytestmark = pytest.mark.gpu

B, T, NP_SEED, DROP_SEED = 2, 4, 11, 5
Z0 = {"type": "768-x-768-z0", "x": 64}


def build_case(kind, adapter):
    over = dict(decode_mode="index", decode_indices=[0, 1], dropout=0.5, train_mode__patch_mask={"type": kind, "ratio": 0.5})
    if adapter:
        over.update(adapter__type="normal", adapter__frozen=0, adapter__struct=dict(Z0))
    cfg = make_config("tiny", **over)
    res, _, width, layers, _, _ = ARCHS["tiny"]
    x, m, y = synthetic_clips(B, T, res, seed=1234, masked_tail=True)
    return dict(cfg=cfg, T=T, sd=random_state_dict(cfg, T, seed=0), x=x, m=m, y=y, width=width,
                layer_indices=resolve_layer_indices(cfg, layers))


def make_detector(case, precision, arm):
    from dfd_clip_amd.detector import Detector
    det = Detector(case["cfg"], case["T"], None, precision=precision)
    det.load_state_dict(case["sd"])
    det = det.to("cuda").train()
    det.mask_gather, det._keep_masked_kv = arm, True
    det.seed_dropout(DROP_SEED)
    return det


def one_step(case, precision, arm, in_place=True):
    """One seeded train forward + backward -> what the arms are compared on."""
    det = make_detector(case, precision, arm)
    det.kv_in_place = in_place
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    np.random.seed(NP_SEED)
    losses, logits, other = det(x, [y], m, train=True, single_task=0)
    (losses[0].mean() + sum(other.values())).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in det.named_parameters() if p.grad is not None}
    assert len(grads) > 20 and not any(n.startswith("encoder.") for n in grads)
    return dict(det=det, kv=tuple(t.detach().clone() for t in det._last_masked_kv), logits=logits[0].detach().clone(),
                loss=losses[0].detach().clone(), grads=grads, path=det.last_mask_path, src=det._last_masked_src)


@functools.lru_cache(maxsize=None)
def arms(kind, adapter, precision):
    """The "torch" arm twice and the "device" arm once: computed once per configuration, shared, never written again."""
    case = build_case(kind, adapter)
    return case, one_step(case, precision, "torch"), one_step(case, precision, "torch"), one_step(case, precision, "device")


def gap(a, b):
    return (a.double() - b.double()).abs().max().item()


CONFIGS = [(k, a, p) for k in ("batch", "sample") for a in (False, True) for p in ("fp32", "bf16")]
IDS = [f"{k}-{'z0' if a else 'noadapter'}-{p}" for k, a, p in CONFIGS]


@pytest.mark.parametrize("kind,adapter,precision", CONFIGS, ids=IDS)
def test_gathered_kv_is_bit_identical_between_the_arms(kind, adapter, precision):
    case, t1, _, dev = arms(kind, adapter, precision)
    assert t1["path"] == "torch" and dev["path"] == "device"
    for a, b in zip(t1["kv"], dev["kv"]):
        S = int(4 * 0.5)
        assert a.shape == b.shape == (2, B * T * S, case["width"]) and a.dtype == b.dtype
        assert a.dtype == (torch.float32 if precision == "fp32" else torch.bfloat16)
        assert torch.isfinite(b.float()).all()
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), f"max |d| {gap(a, b):.3e}"


@pytest.mark.parametrize("kind,adapter,precision", CONFIGS, ids=IDS)
def test_logits_and_gradients_agree_as_two_torch_runs_do(kind, adapter, precision):
    _, t1, t2, dev = arms(kind, adapter, precision)
    rows = [("logits", t1["logits"], t2["logits"], dev["logits"]), ("loss", t1["loss"], t2["loss"], dev["loss"])]
    rows += [("grad " + n, t1["grads"][n], t2["grads"][n], dev["grads"][n]) for n in t1["grads"]]
    assert set(dev["grads"]) == set(t1["grads"])
    worst = 0.0
    for name, a, a2, d in rows:
        bar, got = gap(a, a2), gap(a, d)
        worst = max(worst, bar)
        assert torch.isfinite(d.float()).all(), name
        if bar == 0.0:
            assert torch.equal(a, d), f"{name}: two torch runs agree bit for bit, the device arm is off by {got:.3e}"
        else:
            assert got <= bar, f"{name}: device vs torch {got:.3e} > torch vs torch {bar:.3e}"
    print(f"torch-vs-torch worst gap {worst:.3e} over {len(rows)} tensors")


@pytest.mark.parametrize("adapter", [False, True])
def test_the_device_arm_reads_the_in_place_buffer_and_writes_no_export(adapter):
    case, t1, _, dev = arms("sample", adapter, "bf16")
    det, (k, v) = dev["det"], dev["src"]
    D, L = case["width"], len(case["layer_indices"])
    assert dev["path"] == "device" and det.kv_in_place
    # the encoder's return is the pair of strided views of the persistent q|k|v set: no [L, N*P, D] pair exists
    buf = det._kv_static[1][0]
    assert tuple(buf.shape) == (L, B * T, 4 + 1, 3 * D)
    assert k.dim() == 4 and tuple(k.shape) == (L, B * T, 4, D) and k.stride() == v.stride() == (buf.stride(0), buf.stride(1), 3 * D, 1)
    assert k.data_ptr() == buf[:, :, 1:, D:2 * D].data_ptr() and v.data_ptr() == buf[:, :, 1:, 2 * D:].data_ptr()
    assert t1["src"] is None  # the "torch" arm never goes there
    # ... and from the dense export (`kv_in_place = False`) the same kernel gathers the same bits
    dense = one_step(case, "bf16", "device", in_place=False)
    assert dense["path"] == "device" and dense["src"][0].dim() == 3 and dense["src"][0].is_contiguous()
    for a, b in zip(dev["kv"], dense["kv"]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert torch.equal(dev["logits"], dense["logits"])


@pytest.mark.parametrize("adapter", [False, True])
def test_pipelined_device_arm_matches_the_unpipelined_one(adapter):
    """pipeline_encoder + inputs_ready (+ static_graphs without an adapter): three steps over two alternating static batches.
    The set's three events are recorded right behind the gather in this mode: the second pass into a set (step 2) must
    not overwrite rows that step 0's gather has yet to read, and must leave step 0's results alone."""
    case = build_case("sample", adapter)
    det_e = make_detector(case, "bf16", "device")
    det_p = copy.deepcopy(det_e)
    det_p.seed_dropout(DROP_SEED)
    det_p.pipeline_encoder, det_p.inputs_ready, det_p.static_graphs = True, True, not adapter
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    a, b = (x.contiguous(), m, y), ((x * 0.5).flip(0).contiguous(), m.flip(0).contiguous(), y.flip(0).contiguous())
    torch.cuda.synchronize()  # inputs_ready: both batches are complete in device memory before the loop
    opts = [d.configure_optimizers(0.01) for d in (det_e, det_p)]
    for step in range(3):
        xs, ms, ys = (a, b)[step % 2]
        res = []
        for det, opt in zip((det_e, det_p), opts):
            det.train()
            det.zero_grad()
            np.random.seed(NP_SEED + step)
            losses, _, other = det(xs, [ys], ms, train=True, single_task=0)
            (losses[0].mean() + sum(other.values())).backward()
            res.append((losses[0].detach().clone(), tuple(t.clone() for t in det._last_masked_kv)))
            opt.step()
            assert det.last_mask_path == "device"
        assert torch.equal(res[0][0], res[1][0]), f"step {step}: losses differ"
        for ke, kp in zip(res[0][1], res[1][1]):
            assert torch.equal(ke.view(torch.uint8), kp.view(torch.uint8)), f"step {step}: gathered K/V differ"
    for (n, pe), (_, pp) in zip(det_e.named_parameters(), det_p.named_parameters()):
        assert torch.equal(pe, pp), n
    assert len(det_p._kv_static[1]) == 2 and len(det_e._kv_static[1]) == 1  # two alternating sets against one
    if not adapter:  # the pass over the recurring (batch, set) pair of step 2 was captured and replayed as one graph
        assert det_p._enc_graphs_failed is None and len(det_p._enc_graphs) >= 1, (det_p._enc_graphs_failed, len(det_p._enc_graphs))
    assert not det_e._enc_graphs


def test_guide_masks_agree_between_the_arms(tmp_path):
    """`patch_mask.type: guide` with the fixture map of tests/attnmap_cases.py: one seeded step in each arm."""
    path = tmp_path / "guide.npz"
    harness.save_guide(path, {"v": load_golden(GUIDE_CASE)["guide_v"]})
    case = build_guide_case(path)
    t1, t2, dev = (one_step(case, "fp32", arm) for arm in ("torch", "torch", "device"))
    assert dev["path"] == "device" and t1["path"] == "torch"
    for a, b in zip(t1["kv"], dev["kv"]):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    for name, a, a2, d in [("logits", t1["logits"], t2["logits"], dev["logits"])] + \
            [("grad " + n, t1["grads"][n], t2["grads"][n], dev["grads"][n]) for n in t1["grads"]]:
        bar = gap(a, a2)
        assert torch.equal(a, d) if bar == 0.0 else gap(a, d) <= bar, (name, bar, gap(a, d))
