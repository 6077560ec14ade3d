"""The seeded DINOv2 parity cases shared by tools/gen_golden_dinov2.py (which ran the reference's own `DINOv2` wrapper
and `Detector` on them to produce tests/golden/dinov2_*.npz) and by tests/test_dinov2_cpu.py / test_hip_dinov2.py.
Inputs and weights are re-derived from seeds; the fixtures hold results only."""
import os

import numpy as np

from dfd_clip_amd.config import ConfigNode, default_detector_config
from dfd_clip_amd.weights import ARCHS, model_arch, random_state_dict, resolve_layer_indices, synthetic_clips

# name -> (dinov2 arch, B, T, config overrides, what the fixture stores of the tower)
CASES = {
    "dinov2_tiny": ("dino_tiny", 2, 4, dict(decode_mode="index", decode_indices=[0, 1]), "full"),
    "dinov2_tiny_adapter": ("dino_tiny", 2, 4, dict(decode_mode="index", decode_indices=[0, 1], adapter__type="normal", adapter__frozen=0,
                                                    adapter__struct={"type": "768-x-768-nln", "x": 32}), "none"),
    # the real geometry (what the reference wrapper hard-codes), 1 clip x 2 frames, layers 6..11 tapped as the shipped
    # configs/deepfake/dino/*.yaml do
    "dinov2_vitb14": ("dinov2_vitb14", 1, 2, dict(decode_mode="index", decode_indices=[6, 7, 8, 9, 10, 11]), "rows"),
}
# "rows": token rows kept, every frame (CLS, first patches, a middle one, the last ones), of the tapped blocks' k / v, the
# first tapped block's q and the last block's out: what fits the size cap of a committed fixture
STORED_ROWS = [0, 1, 2, 128, 255, 256]


# bf16 path against the reference's fp32 results, measured on MI355X (max |difference|; the kernels are deterministic,
# so the figures repeat): a case's bar is TWICE its measured value (tests/test_hip_dinov2.py `bf16_bar`)
# ("tower": the largest difference over every stored q / k / v / out of every block)
BF16_MEASURED = {"dinov2_tiny/tower": 3.422e-2, "dinov2_vitb14/tower": 8.039e-2, "dinov2_tiny/logits": 1.939e-3,
                 "dinov2_tiny_adapter/logits": 3.559e-2, "dinov2_vitb14/logits": 6.473e-3}


def make_config(arch, **over):
    cfg = default_detector_config()
    cfg.foundation = "dinov2"
    # the shipped dino configs carry `architecture: ViT-B/16`, which the reference ignores; a DINOv2 geometry's name selects it
    cfg.architecture = "ViT-B/16" if arch == "dinov2_vitb14" else arch
    cfg.out_dim = [2]
    cfg.losses = ["auc_roc"]
    for k, v in over.items():
        node = cfg
        parts = k.split("__")
        for p in parts[:-1]:
            if p not in node:
                node[p] = ConfigNode()
            node = node[p]
        node[parts[-1]] = v
    return cfg


def build_case(name):
    arch, B, T, over, store = CASES[name]
    cfg = make_config(arch, **over)
    assert model_arch(cfg) == arch
    res, patch, width, layers, heads, _ = ARCHS[arch]
    sd = random_state_dict(cfg, T, seed=0)
    x, m, y = synthetic_clips(B, T, res, seed=1234)
    return dict(name=name, arch=arch, B=B, T=T, cfg=cfg, sd=sd, x=x, m=m, y=y, res=res, patch=patch, width=width, layers=layers,
                heads=heads, store=store, layer_indices=resolve_layer_indices(cfg, layers))


def load_golden(name):
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False)
