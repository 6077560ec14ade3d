"""The fp8 precision policy on the host: parsing, validation and the presets' per-layer forms (`encoder.expand_fp8_policy`,
`VisionTransformer.set_fp8_policy`, `Detector(..., fp8_policy=...)`); the DINOv2 tower constructs with precision="fp8"; and
the entry points of include/dfdclip_ext.h are bound, exported and covered by a guard-band test, as include/dfdclip.h's are."""
import ast
import os
import re

import pytest

from dfd_clip_amd import capi
from dfd_clip_amd.detector import Detector
from dfd_clip_amd.encoder import FP8_CONTRACT_POLICY, FP8_PRESETS, VisionTransformer, expand_fp8_policy
from tests.cases import make_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = {"qkv": "fp8", "fc": "fp8", "proj": "fp8"}
NONE = {"qkv": "bf16", "fc": "bf16", "proj": "bf16"}
TAPS12 = [6, 7, 8, 9, 10, 11]
TAPS24 = list(range(1, 24, 2))


def test_presets_12_layers_taps_6_to_11():
    assert expand_fp8_policy(None, 12, TAPS12) == expand_fp8_policy("all", 12, TAPS12) == [ALL] * 12
    assert expand_fp8_policy("none", 12, TAPS12) == [NONE] * 12
    assert expand_fp8_policy("proj-bf16", 12, TAPS12) == [{"qkv": "fp8", "fc": "fp8", "proj": "bf16"}] * 12
    kv = expand_fp8_policy("kv-bf16", 12, TAPS12)
    assert [e["qkv"] for e in kv] == ["fp8"] * 6 + ["kv-bf16"] * 5 + ["bf16"]  # untapped: fp8; the last tapped layer: bf16
    assert all(e["fc"] == "fp8" and e["proj"] == "fp8" for e in kv)
    kvp = expand_fp8_policy("kv+proj-bf16", 12, TAPS12)
    assert [e["qkv"] for e in kvp] == [e["qkv"] for e in kv] and all(e["fc"] == "fp8" and e["proj"] == "bf16" for e in kvp)
    assert expand_fp8_policy("edges-bf16", 12, TAPS12) == [NONE] * 2 + [ALL] * 8 + [NONE] * 2


def test_presets_24_layers_stride_2():
    kv = expand_fp8_policy("kv-bf16", 24, TAPS24)
    assert [e["qkv"] for e in kv] == [("fp8" if l % 2 == 0 else "bf16" if l == 23 else "kv-bf16") for l in range(24)]
    assert expand_fp8_policy("edges-bf16", 24, TAPS24) == [NONE] * 2 + [ALL] * 20 + [NONE] * 2
    assert expand_fp8_policy("kv+proj-bf16", 24, TAPS24)[5] == {"qkv": "kv-bf16", "fc": "fp8", "proj": "bf16"}
    assert set(FP8_PRESETS) == {"all", "proj-bf16", "kv-bf16", "kv+proj-bf16", "edges-bf16", "none"}
    assert FP8_CONTRACT_POLICY is None or FP8_CONTRACT_POLICY in FP8_PRESETS


def test_per_layer_lists_and_kv_bf16_normalisation():
    pol = [{} for _ in range(12)]
    pol[3] = {"qkv": "kv-bf16"}          # untapped: means fp8
    pol[6] = {"qkv": "kv-bf16"}
    pol[11] = {"qkv": "kv-bf16"}         # the last tapped layer computes K and V only: equals bf16
    pol[7] = {"proj": "bf16"}
    pol[8] = {"fc": "bf16", "proj": "bf16"}
    plan = expand_fp8_policy(pol, 12, TAPS12)
    assert plan[3] == ALL and plan[6]["qkv"] == "kv-bf16" and plan[11]["qkv"] == "bf16"
    assert plan[7] == {"qkv": "fp8", "fc": "fp8", "proj": "bf16"} and plan[8] == {"qkv": "fp8", "fc": "bf16", "proj": "bf16"}
    # without tap information every layer counts as tapped (the bare encoder returns K/V of every layer)
    assert [e["qkv"] for e in expand_fp8_policy("kv-bf16", 4)] == ["kv-bf16"] * 3 + ["bf16"]


def test_invalid_policies_are_refused():
    with pytest.raises(ValueError, match="proj 'fp8' requires fc 'fp8'"):
        expand_fp8_policy([{"fc": "bf16"}] + [{}] * 11, 12, TAPS12)  # proj defaults to fp8
    with pytest.raises(ValueError, match="requires fc"):
        expand_fp8_policy([{"fc": "bf16", "proj": "fp8"}] * 12, 12)
    with pytest.raises(ValueError, match="unknown preset"):
        expand_fp8_policy("most", 12)
    with pytest.raises(ValueError, match="12 layers"):
        expand_fp8_policy([{}] * 11, 12)
    with pytest.raises(ValueError, match="layer 2"):
        expand_fp8_policy([{}, {}, {"qkv": "q-bf16"}] + [{}] * 9, 12)
    with pytest.raises(ValueError, match="keys"):
        expand_fp8_policy([{"out": "bf16"}] * 12, 12)
    with pytest.raises(ValueError, match="tapped"):
        expand_fp8_policy("kv-bf16", 12, [12])


def test_policy_needs_the_fp8_precision():
    enc = VisionTransformer(32, 16, 128, 2, 2, 64, precision="bf16")
    with pytest.raises(ValueError, match="precision='fp8'"):
        enc.set_fp8_policy("all")
    assert enc.fp8_policy() is None
    cfg = make_config("tiny")
    with pytest.raises(ValueError, match="precision='fp8'"):
        Detector(cfg, 4, None, precision="bf16", fp8_policy="proj-bf16")
    Detector(cfg, 4, None, precision="bf16")  # no policy: as before


def test_encoder_and_detector_carry_the_policy():
    enc = VisionTransformer(32, 16, 128, 2, 2, 64, precision="fp8")
    assert enc.fp8_policy() == [ALL] * 2, "the default is 'all'"
    enc.set_fp8_policy("none")
    assert enc.fp8_policy() == [NONE] * 2
    enc.invalidate()
    enc.load_state_dict(enc.state_dict())
    enc = enc.to("cpu")
    assert enc.fp8_policy() == [NONE] * 2, "a policy survives what invalidates weight-derived state"
    with pytest.raises(ValueError, match="unknown preset"):
        enc.set_fp8_policy("some")
    assert enc.fp8_policy() == [NONE] * 2, "a refused policy changes nothing"
    enc.set_fp8_policy(None)
    assert enc.fp8_policy() == [ALL] * 2
    cfg = make_config("ViT-B/16", decode_mode="index", decode_indices=TAPS12)
    det = Detector(cfg, 8, None, precision="fp8", fp8_policy="kv+proj-bf16")
    assert det.encoder.fp8_policy() == expand_fp8_policy("kv+proj-bf16", 12, TAPS12)
    # buffers follow the policy: e4m3 h / u and the bf16 u only where a projection touches them (rows >= FP8_MIN_ROWS)
    assert det.encoder._fp8_needs(4096) == (True, False, True)
    det.set_fp8_policy("all")
    assert det.encoder._fp8_needs(4096) == (True, True, False)
    det.set_fp8_policy("none")
    assert det.encoder._fp8_needs(4096) == (False, False, True)
    det.set_fp8_policy("all")
    assert det.encoder._fp8_needs(4 * 197) == (False, False, True), "a chunk below the e4m3 kernel's shape runs bf16"


def test_dinov2_constructs_in_fp8():
    from dfd_clip_amd.dinov2 import DINOv2
    enc = DINOv2("dino_w768", precision="fp8", checkpoint=None)
    assert (enc.width, enc.heads, enc.tokens, enc.layers, enc.precision) == (768, 12, 5, 2, "fp8")
    assert enc.act_epilogue == capi.EPI_BIAS_GELU and enc.fp8_policy() == [ALL] * 2
    enc.set_fp8_policy("edges-bf16")
    assert enc.fp8_policy() == [NONE] * 2
    with pytest.raises(NotImplementedError, match="fp8"):
        DINOv2("dino_tiny", precision="fp8", checkpoint=None)  # width 128: no fp8 GEMM serves K = 128


# ---- include/dfdclip_ext.h: bound, exported, covered ---------------------------------------------------------------

def _ext_functions():
    text = open(os.path.join(ROOT, "include", "dfdclip_ext.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", text)))


def test_ext_header_and_ctypes_table_agree():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    fns = _ext_functions()
    assert fns == sorted(capi.EXT_SIGNATURES) == ["dfd_add_layernorm_dual", "dfd_layernorm2_dual", "dfd_layernorm_dual"]
    assert not set(fns) & set(capi.SIGNATURES)
    for name in fns:
        assert hasattr(lib, name), name
    rc = lib.dfd_layernorm_dual(None, 0, None, None, None, 0, None, 0, 1, 8, 1e-5, 1.0, None)
    assert rc == -1 and b"null pointer" in lib.dfd_last_error()
    rc = lib.dfd_add_layernorm_dual(1 << 12, 8, 1 << 13, None, 8, capi.BF16, 1, 1 << 14, 1 << 15, 1 << 16, 8, 1 << 17, 8, 1, 8, 1e-5, 0.0, None)
    assert rc == -1 and b"y8_inv_scale" in lib.dfd_last_error()
    rc = lib.dfd_layernorm2_dual(1 << 12, 8, 1 << 13, 1 << 13, 1 << 13, 1 << 13, 1 << 16, 8, 1 << 17, 6, 1, 8, 1e-5, 1.0, None)
    assert rc == -1 and b"leading dimension" in lib.dfd_last_error()


def test_every_ext_function_has_a_guarded_test():
    src = open(os.path.join(ROOT, "tests", "test_hip_guarded_dual.py")).read()
    tree = ast.parse(src)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    table = {}
    for line in ast.get_docstring(tree).splitlines():
        m = re.match(r"\s*(dfd_[a-z0-9_]+)\s+(test_[a-z0-9_, ]+)$", line)
        if m:
            table[m.group(1)] = [t.strip() for t in m.group(2).split(",") if t.strip()]
    assert sorted(table) == _ext_functions()
    for f, ts in table.items():
        assert ts and all(t in tests for t in ts), f
        assert re.search(r"\bcapi\.%s\(" % re.escape(f[len("dfd_"):]), src), f"{f}: no call through capi in the module"
