"""CPU checks of the DINOv2 towers beside ViT-B/14 (ViT-S/14, ViT-L/14, ViT-g/14 with its SwiGLU feed-forward): the
state_dict schema against the names recorded from the reference's own factories, the SwiGLU width, the host-side folding
against the reference's per-block results, which names `model_arch` selects, what fp8 refuses, and the header of the gate
kernel against its ctypes table."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.detector import Detector
from dfd_clip_amd.weights import ARCHS, DINO_FFN, DINO_IMG_SIZE, dinov2_schema, model_arch, swiglu_hidden
from tests.dinov2_family_cases import CASES, REAL_TOWERS, build_case, load_golden, recorded_schema

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_TOL = 2e-5  # tests/test_oracle_golden.py: an fp32 torch restatement against the reference's fp32 results


def test_arch_rows_are_the_factories():
    assert ARCHS["dinov2_vits14"] == (224, 14, 384, 12, 6, 0)
    assert ARCHS["dinov2_vitl14"] == (224, 14, 1024, 24, 16, 0)
    assert ARCHS["dinov2_vitg14"] == (224, 14, 1536, 40, 24, 0)
    assert ARCHS["dino_tiny_swiglu"] == (28, 14, 128, 2, 2, 0) and ARCHS["dino_s2"] == (28, 14, 384, 2, 6, 0)
    assert ARCHS["dino_g2"] == (224, 14, 1536, 2, 24, 0)
    assert all(len(row) == 6 for row in ARCHS.values())
    assert {n: DINO_IMG_SIZE[n] for n in ("dinov2_vits14", "dinov2_vitl14", "dinov2_vitg14", "dino_g2", "dino_tiny_swiglu", "dino_s2")} == \
        {"dinov2_vits14": 518, "dinov2_vitl14": 518, "dinov2_vitg14": 518, "dino_g2": 518, "dino_tiny_swiglu": 70, "dino_s2": 70}
    assert set(DINO_FFN) == set(DINO_IMG_SIZE) and set(DINO_FFN.values()) == {"mlp", "swiglu"}
    assert sorted(n for n, k in DINO_FFN.items() if k == "swiglu") == ["dino_g2", "dino_tiny_swiglu", "dinov2_vitg14"]
    assert DINO_FFN["dinov2_vitb14"] == "mlp" and DINO_FFN["dino_tiny"] == "mlp"


def test_swiglu_hidden_is_the_fused_layers():
    assert swiglu_hidden(1536) == 4096 and swiglu_hidden(128) == 344
    s = dinov2_schema("dinov2_vitg14")
    assert s["backbone.blocks.39.mlp.w12.weight"] == (8192, 1536) and s["backbone.blocks.39.mlp.w12.bias"] == (8192,)
    assert s["backbone.blocks.0.mlp.w3.weight"] == (1536, 4096) and s["backbone.blocks.0.mlp.w3.bias"] == (1536,)
    assert dinov2_schema("dino_tiny_swiglu")["backbone.blocks.1.mlp.w3.weight"] == (128, 344)
    assert not any("fc1" in k or "fc2" in k for k in s)


@pytest.mark.parametrize("tower", list(REAL_TOWERS))
def test_schema_is_the_reference_factorys_name_for_name(tower):
    want = recorded_schema(tower)
    got = [(k[len("backbone."):], shp) for k, shp in dinov2_schema(tower).items()]
    assert len(want) > 100 and got == want  # names, shapes and order: an official checkpoint loads with strict=True


@pytest.mark.parametrize("tower", ["dinov2_vits14", "dinov2_vitl14"])
def test_backbone_loads_the_recorded_names_strictly(tower):
    """The module itself (ViT-g/14's 1.1 B parameters are not allocated in a test: its block is `dino_g2`'s, below)."""
    from dfd_clip_amd.dinov2 import CHECKPOINTS, DINOv2
    enc = DINOv2(tower, precision="fp32", checkpoint=None)
    want = recorded_schema(tower)
    assert [(k, tuple(v.shape)) for k, v in enc.backbone.state_dict().items()] == want
    res = enc.backbone.load_state_dict({k: torch.zeros(shp) for k, shp in want}, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert CHECKPOINTS[tower] == f"misc/{tower}_pretrain.pth" and CHECKPOINTS["dinov2_vitb14"] == "misc/dinov2_vitb14_pretrain.pth"
    assert enc.ffn == "mlp" and enc.ffn_hidden == 0


def test_vitg14_blocks_are_the_recorded_ones():
    """One block of ViT-g/14 at its real size (dino_g2 = two of its forty) against the recorded names of the factory."""
    from dfd_clip_amd.dinov2 import CHECKPOINTS, DINOv2
    enc = DINOv2("dino_g2", precision="fp32", checkpoint=None)
    assert enc.ffn == "swiglu" and enc.ffn_hidden == 4096 and CHECKPOINTS["dinov2_vitg14"] == "misc/dinov2_vitg14_pretrain.pth"
    want = dict(recorded_schema("dinov2_vitg14"))
    got = {k: tuple(v.shape) for k, v in enc.backbone.state_dict().items()}
    assert got == {k: s for k, s in want.items() if not k.startswith("blocks.") or int(k.split(".")[1]) < 2}
    order = [k for k, _ in recorded_schema("dinov2_vitg14") if k in got]
    assert list(got) == order


@pytest.mark.parametrize("name", list(CASES))
def test_detector_state_dict_schema_is_the_references(name):
    case, g = build_case(name), load_golden(name)
    want = dict(zip(g["keys"].tolist(), g["shapes"].tolist()))
    assert {k: ",".join(map(str, t.shape)) for k, t in case["sd"].items()} == want
    det = Detector(case["cfg"], case["T"], None, precision="fp32")
    assert list(det.state_dict()) == g["keys"].tolist()
    res = det.load_state_dict(case["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    assert not any(p.requires_grad for p in det.encoder.parameters())
    for prec in ("bf16",):
        assert Detector(case["cfg"], case["T"], None, precision=prec).encoder.precision == prec
    # the decoder starts from the tower's LayerNorms; an MLP tower's fc1 / fc2 too, a SwiGLU tower has none to give
    sd = case["sd"]
    assert torch.equal(sd["decoder.transformer.resblocks.1.ln_2.weight"], sd["encoder.backbone.blocks.1.norm2.weight"])
    if DINO_FFN[case["arch"]] == "mlp":
        assert torch.equal(sd["decoder.transformer.resblocks.1.mlp.c_fc.weight"], sd["encoder.backbone.blocks.1.mlp.fc1.weight"])
    else:
        assert tuple(sd["decoder.transformer.resblocks.1.mlp.c_fc.weight"].shape) == (4 * case["width"], case["width"])


def restate_tower(f, x, D, heads, patch, res, dtype=torch.float32):
    """fp32 torch restatement of the kernel sequence on `folded_operands()`: per block {q, k, v, out}, and the first input."""
    grid = res // patch
    n = x.shape[0]
    c = lambda t: t.to(dtype)
    patches = x.to(dtype).view(n, 3, grid, patch, grid, patch).permute(0, 2, 4, 1, 3, 5).reshape(n, grid * grid, -1)
    tok = torch.cat([(c(f["cls"]) + c(f["pos"][0])).expand(n, 1, -1), patches @ c(f["w_patch"]).T + c(f["pos"][1:])], 1)
    ln = lambda t, gb: torch.nn.functional.layer_norm(t, (D,), c(gb[0]), c(gb[1]), 1e-6)
    xx, out = tok, []
    for b in f["blocks"]:
        qkv = ln(xx, b["ln1"]) @ c(b["w_qkv"]).T + c(b["b_qkv"])
        q, k, v = qkv.view(n, -1, 3, heads, 64).unbind(2)
        a = ((q.transpose(1, 2) @ k.transpose(1, 2).transpose(-1, -2)) * 64 ** -0.5).softmax(-1) @ v.transpose(1, 2)
        xx = xx + a.transpose(1, 2).reshape(n, -1, D) @ c(b["w_out"]).T + c(b["b_out"])
        h = ln(xx, b["ln2"])
        if "w_12" in b:  # gate, then w3 with ls2 folded in
            x12 = h @ c(b["w_12"]).T + c(b["b_12"])
            H = x12.shape[-1] // 2
            x1, x2 = x12[..., :H], x12[..., H:]
            xx = xx + (x1 / (1 + torch.exp(-x1)) * x2) @ c(b["w_3"]).T + c(b["b_3"])
        else:
            xx = xx + torch.nn.functional.gelu(h @ c(b["w_fc"]).T + c(b["b_fc"])) @ c(b["w_proj"]).T + c(b["b_proj"])
        out.append(dict(q=q, k=k, v=v, out=xx))
    return tok, out


@pytest.mark.parametrize("name", ["dinov2_family_tiny_swiglu", "dinov2_family_s2"])
def test_folded_operands_reproduce_the_references_blocks(name):
    case, g = build_case(name), load_golden(name)
    det = Detector(case["cfg"], case["T"], None, precision="fp32")
    det.load_state_dict(case["sd"], strict=True)
    f = det.encoder.folded_operands()
    swiglu = DINO_FFN[case["arch"]] == "swiglu"
    assert set(f["blocks"][0]) == ({"ln1", "ln2", "w_qkv", "b_qkv", "w_out", "b_out"} |
                                   ({"w_12", "b_12", "w_3", "b_3"} if swiglu else {"w_fc", "b_fc", "w_proj", "b_proj"}))
    if swiglu:
        H = swiglu_hidden(case["width"])
        assert tuple(f["blocks"][0]["w_12"].shape) == (2 * H, case["width"]) and tuple(f["blocks"][0]["w_3"].shape) == (case["width"], H)
    with torch.no_grad():
        tok, blocks = restate_tower(f, case["x"].flatten(0, 1), case["width"], case["heads"], case["patch"], case["res"])
    np.testing.assert_allclose(tok.numpy(), g["enc_in"], atol=ORACLE_TOL, rtol=0)
    for l, d in enumerate(blocks):
        for key in ("q", "k", "v", "out"):
            err = np.abs(d[key].numpy() - g[f"enc{l}_{key}"]).max()
            print(f"{name}: block {l} {key}: max |d| = {err:.3e}")
            assert err <= ORACLE_TOL, (l, key, err)
    if swiglu:  # a stale or missing ls2 fold would show: with gamma = 1 the folded w3 moves by far more than the bar
        w3 = f["blocks"][0]["w_3"].clone()
        det.encoder.backbone.blocks[0].ls2.gamma.data.fill_(1.0)
        assert (det.encoder.folded_operands()["blocks"][0]["w_3"] - w3).abs().max() > 1e-3


def test_model_arch_selects_the_new_names():
    from dfd_clip_amd.weights import DINO_ALIASES
    cfg = Detector.get_default_config()
    cfg.foundation = "dinov2"
    for name in ("dinov2_vits14", "dinov2_vitg14", "dino_tiny_swiglu", "dino_s2", "dino_g2", "dino_tiny"):
        cfg.architecture = name
        assert model_arch(cfg) == name
    # ... and by the model cards' names, the one spelling that selects ViT-L/14: `architecture: dinov2_vitl14` was refused
    # before the tower existed, tests/test_dinov2_cpu.py pins that, and it stays refused (now naming the spelling to use)
    assert DINO_ALIASES == {"dinov2-small": "dinov2_vits14", "dinov2-base": "dinov2_vitb14", "dinov2-large": "dinov2_vitl14",
                            "dinov2-giant": "dinov2_vitg14"}
    for alias, name in DINO_ALIASES.items():
        cfg.architecture = alias
        assert model_arch(cfg) == name
    cfg.architecture = "dinov2_vitl14"
    with pytest.raises(NotImplementedError, match="architecture: 'dinov2-large'"):
        model_arch(cfg)
    for name in ("ViT-L/14", "ViT-L/14@336px", "RN50"):  # the reference's CLIP names are still ignored
        cfg.architecture = name
        assert model_arch(cfg) == "dinov2_vitb14"
    cfg.architecture = "tiny"
    with pytest.raises(NotImplementedError, match="architecture"):
        model_arch(cfg)


def test_detector_builds_on_vitl14_by_its_alias():
    cfg = Detector.get_default_config()
    cfg.foundation, cfg.architecture, cfg.out_dim, cfg.losses = "dinov2", "dinov2-large", [2], ["auc_roc"]
    cfg.decode_mode, cfg.decode_indices = "index", [22, 23]
    det = Detector(cfg, 4, None)
    assert (det.encoder.width, det.encoder.heads, det.encoder.layers, det.encoder.ffn) == (1024, 16, 24, "mlp")
    assert tuple(det.encoder.backbone.pos_embed.shape) == (1, 1370, 1024) and det.layer_indices == [22, 23]
    assert Detector(cfg, 4, None, precision="fp8", fp8_policy="kv-bf16").encoder.fp8_policy()[22]["qkv"] == "kv-bf16"


def test_fp8_refusals():
    from dfd_clip_amd.dinov2 import DINOv2
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        DINOv2("dino_g2", precision="fp8", checkpoint=None)
    case = build_case("dinov2_family_tiny_swiglu")
    with pytest.raises(NotImplementedError, match="SwiGLU"):
        Detector(case["cfg"], case["T"], None, precision="fp8")
    with pytest.raises(NotImplementedError, match="width 384"):
        DINOv2("dinov2_vits14", precision="fp8", checkpoint=None)


def test_width_768_adapter_structs_stay_refused_in_words():
    case = build_case("dinov2_family_s2")
    cfg = case["cfg"].clone()
    from dfd_clip_amd.config import ConfigNode
    cfg.adapter = ConfigNode({"type": "normal", "frozen": 0, "struct": {"type": "768-bn"}})
    with pytest.raises(NotImplementedError, match="768"):
        Detector(cfg, case["T"], None)
    cfg.adapter = ConfigNode({"type": "normal", "frozen": 0, "struct": {"type": "768-x-768-nln", "x": 32}})
    det = Detector(cfg, case["T"], None)  # the structs that only carry 768 in their name follow the tower's width
    assert det.adapter is not None and tuple(det.adapter.state_dict()["l0_k.0.weight"].shape) == (32, 384)


def test_header_matches_the_ctypes_table():
    text = open(os.path.join(ROOT, "include", "dfdclip_swiglu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\bint\s+(dfd_\w+)\s*\(([^)]*)\)\s*;", code)
    assert sorted(n for n, _ in protos) == sorted(capi.SWIGLU_SIGNATURES) == ["dfd_swiglu_fwd", "dfd_swiglu_last_path"]
    lib = capi.load_library()
    for name, params in protos:
        res, args = capi.SWIGLU_SIGNATURES[name]
        assert res is ctypes.c_int and getattr(lib, name).argtypes == args
        assert (0 if params.strip() == "void" else len(params.split(","))) == len(args)
    assert "DFD_ABI_VERSION" not in code.replace("WITHOUT a new DFD_ABI_VERSION", "")
    assert (capi.SWIGLU_VEC16, capi.SWIGLU_ELEMENT) == tuple(int(re.search(rf"#define {n} (\d+)", code).group(1))
                                                           for n in ("DFD_SWIGLU_VEC16", "DFD_SWIGLU_ELEMENT"))
    assert capi.ABI_VERSION == 17
