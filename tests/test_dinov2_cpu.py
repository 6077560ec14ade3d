"""CPU checks of the DINOv2 foundation: the state_dict schema against the reference's (stored in the fixtures), the
seeded state, the host-side folding / positional resampling against the reference's first block, and that `Detector`
accepts `foundation: dinov2` (it raised NotImplementedError before this tower existed)."""
import numpy as np
import pytest
import torch

from dfd_clip_amd.config import ConfigNode
from dfd_clip_amd.detector import Detector
from dfd_clip_amd.weights import random_state_dict
from tests.dinov2_cases import CASES, build_case, load_golden


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_schema_is_the_references(name):
    case, g = build_case(name), load_golden(name)
    want = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    assert {k: ",".join(map(str, t.shape)) for k, t in case["sd"].items()} == want  # (the seeded state lists them in schema order)
    enc_keys = [k for k in g["keys"].tolist() if k.startswith("encoder.")]
    assert [k for k in case["sd"] if k.startswith("encoder.")] == enc_keys and enc_keys[0] == "encoder.backbone.cls_token"
    if name == "dinov2_vitb14":
        return  # (constructing the real tower is the next test's business)
    det = Detector(case["cfg"], case["T"], None, precision="fp32")
    assert list(det.state_dict()) == g["keys"].tolist()  # the module itself: the reference's order too
    res = det.load_state_dict(case["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert not any(p.requires_grad for p in det.encoder.parameters())


def test_seeded_state_is_deterministic_and_exercises_the_folding():
    case = build_case("dinov2_tiny")
    again = random_state_dict(case["cfg"], case["T"], seed=0)
    assert all(torch.equal(case["sd"][k], again[k]) for k in again)
    other = random_state_dict(case["cfg"], case["T"], seed=1)
    assert not torch.equal(case["sd"]["encoder.backbone.pos_embed"], other["encoder.backbone.pos_embed"])
    gamma = case["sd"]["encoder.backbone.blocks.0.ls1.gamma"]
    assert (gamma - 1).abs().min() > 1e-4 and gamma.std() > 0.1, "LayerScale must be far from the identity"
    assert case["sd"]["encoder.backbone.patch_embed.proj.bias"].abs().max() > 1e-3
    # decoder blocks start from the tapped backbone block (reference src/models.py:192-229)
    assert torch.equal(case["sd"]["decoder.transformer.resblocks.1.mlp.c_fc.weight"], case["sd"]["encoder.backbone.blocks.1.mlp.fc1.weight"])
    assert torch.equal(case["sd"]["decoder.transformer.resblocks.0.ln_2.bias"], case["sd"]["encoder.backbone.blocks.0.norm2.bias"])


def test_folded_operands_reproduce_the_references_first_block():
    """The staging arithmetic (conv bias and cls_token folded into the patch-embedding operands, pos_embed resampled
    5x5 -> 2x2 with the reference's scale factor, LayerScale folded into attn.proj / mlp.fc2), run through a float64
    restatement of one block, against the reference's own first-block input and output."""
    case, g = build_case("dinov2_tiny"), load_golden("dinov2_tiny")
    det = Detector(case["cfg"], case["T"], None, precision="fp32")
    det.load_state_dict(case["sd"], strict=True)
    f = det.encoder.folded_operands()
    D, H, patch = case["width"], case["heads"], case["patch"]
    grid = case["res"] // patch
    x = case["x"].flatten(0, 1).double()
    n = x.shape[0]
    patches = x.view(n, 3, grid, patch, grid, patch).permute(0, 2, 4, 1, 3, 5).reshape(n, grid * grid, -1)
    tok = torch.cat([(f["cls"].double() + f["pos"][0].double()).expand(n, 1, -1), patches @ f["w_patch"].double().T + f["pos"][1:].double()], 1)
    assert tuple(f["pos"].shape) == (grid * grid + 1, D)
    np.testing.assert_allclose(tok.numpy(), g["enc_in"], atol=2e-5, rtol=0)
    b = f["blocks"][0]
    ln = lambda t, gb: torch.nn.functional.layer_norm(t, (D,), gb[0].double(), gb[1].double(), 1e-6)
    qkv = ln(tok, b["ln1"]) @ b["w_qkv"].double().T + b["b_qkv"].double()
    q, k, v = qkv.view(n, -1, 3, H, 64).unbind(2)
    for name, t in (("q", q), ("k", k), ("v", v)):
        np.testing.assert_allclose(t.numpy(), g["enc0_" + name], atol=2e-5, rtol=0)
    a = ((q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2)) * 64 ** -0.5).softmax(-1) @ v.transpose(1, 2)
    xx = tok + a.transpose(1, 2).reshape(n, -1, D) @ b["w_out"].double().T + b["b_out"].double()
    u = torch.nn.functional.gelu(ln(xx, b["ln2"]) @ b["w_fc"].double().T + b["b_fc"].double())
    xx = xx + u @ b["w_proj"].double().T + b["b_proj"].double()
    np.testing.assert_allclose(xx.numpy(), g["enc0_out"], atol=2e-5, rtol=0)
    # stale folding would show: with gamma = 1 the same restatement misses by far more than the bar
    det.encoder.backbone.blocks[0].ls2.gamma.data.fill_(1.0)
    f1 = det.encoder.folded_operands()
    assert (f1["blocks"][0]["w_proj"] - b["w_proj"]).abs().max() > 1e-3


def test_detector_constructs_with_the_dinov2_foundation():
    case = build_case("dinov2_tiny")
    det = Detector(case["cfg"], case["T"], None)
    enc = det.encoder
    assert (enc.width, enc.heads, enc.input_resolution, enc.patch_size, enc.block_num) == (128, 2, 28, 14, 2)
    assert len(enc.transformer.resblocks) == 2 and enc.precision == "bf16" and enc.ln_eps == 1e-6
    assert det.transform.mean == (0.485, 0.456, 0.406) and det.transform.std == (0.229, 0.224, 0.225)
    assert enc.pixel_mean == det.transform.mean and enc.pixel_std == det.transform.std
    with pytest.raises(NotImplementedError, match="fp8"):
        Detector(case["cfg"], case["T"], None, precision="fp8")


def test_architecture_key_under_the_dinov2_foundation():
    """A CLIP model name of the reference is ignored (ViT-B/14 is built, as the reference does); the name of a DINOv2
    geometry selects it; this project's CLIP test geometries are refused instead of being answered with ViT-B/14."""
    from dfd_clip_amd.weights import model_arch
    cfg = Detector.get_default_config()
    cfg.foundation = "dinov2"
    for name in ("ViT-B/16", "ViT-L/14", "RN50", "dinov2_vitb14"):
        cfg.architecture = name
        assert model_arch(cfg) == "dinov2_vitb14"
    cfg.architecture = "dino_tiny"
    assert model_arch(cfg) == "dino_tiny"
    for name in ("tiny", "small14", "dinov2_vitl14"):
        cfg.architecture = name
        with pytest.raises(NotImplementedError, match="architecture"):
            model_arch(cfg)
        with pytest.raises(NotImplementedError, match="architecture"):
            Detector(cfg, 4, None)
    cfg.foundation = "clip"
    assert model_arch(cfg) == "dinov2_vitl14"  # (the CLIP path resolves its own names)


# the model sections of the reference's configs/deepfake/dino/*.yaml (settings only), num_frames 20
_NLN = {"foundation": "dinov2", "adapter": {"frozen": 0, "struct": {"type": "768-x-768-nln", "x": 256}, "type": "normal"},
        "architecture": "ViT-B/16", "decode_indices": [6, 7, 8, 9, 10, 11], "decode_mode": "index", "decode_stride": 2, "dropout": 0.5,
        "losses": ["auc_roc"], "name": "Detector", "out_dim": [2], "train_mode": {}, "weight_decay": 0.01, "optimizer": "sgd"}
SHIPPED = {
    "sgd(0.9m)-pure": _NLN,
    "sgd(0.9m)-pure-all": _NLN,
    "sgd(0.9m)-pure-pm-all-ln": dict(_NLN, adapter={"frozen": 0, "struct": {"type": "768-x-768-ln", "x": 256}, "type": "normal"},
                                     train_mode={"patch_mask": {"type": "batch", "ratio": 0.75}}),
}


@pytest.mark.parametrize("name", list(SHIPPED))
def test_shipped_dino_configs_are_accepted(name):
    cfg = Detector.get_default_config()
    for k, v in SHIPPED[name].items():
        cfg[k] = ConfigNode(v) if isinstance(v, dict) else v
    det = Detector(cfg, 20, None)
    assert type(det.encoder).__name__ == "DINOv2" and det.encoder.width == 768 and len(det.encoder.transformer.resblocks) == 12
    assert det.layer_indices == [6, 7, 8, 9, 10, 11] and det.adapter is not None and det.adapter.patches == 256
    assert tuple(det.encoder.backbone.pos_embed.shape) == (1, 1370, 768)
    opt = det.configure_optimizers(0.005)
    assert isinstance(opt, torch.optim.SGD)
