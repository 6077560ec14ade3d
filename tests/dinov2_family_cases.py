"""The seeded parity cases of the DINOv2 towers beside ViT-B/14 (ViT-S/14, ViT-L/14, and ViT-g/14 with its SwiGLU
feed-forward), shared by tools/gen_golden_dinov2_family.py (which ran the reference's own factories, `DINOv2` wrapper and
`Detector` on them to produce tests/golden/dinov2_family_*.npz) and by tests/test_dinov2_family_cpu.py /
test_hip_dinov2_family.py.  Inputs and weights are re-derived from seeds; the fixtures hold results only."""
import os

import numpy as np

from dfd_clip_amd.weights import ARCHS, model_arch, random_state_dict, resolve_layer_indices, synthetic_clips
from tests.dinov2_cases import STORED_ROWS, make_config  # noqa: F401  (the row subset of the real-width fixture is dinov2_vitb14's)

# fixture name -> (dinov2 arch, B, T, config overrides, what the fixture stores of the tower)
CASES = {
    "dinov2_family_tiny_swiglu": ("dino_tiny_swiglu", 2, 4, dict(decode_mode="index", decode_indices=[0, 1]), "full"),
    "dinov2_family_s2": ("dino_s2", 2, 4, dict(decode_mode="index", decode_indices=[0, 1]), "full"),
    # ViT-g/14's width, heads, SwiGLU (H = 4096) and 257 tokens: every block's q / k / v / out at token rows STORED_ROWS
    "dinov2_family_g2": ("dino_g2", 1, 2, dict(decode_mode="index", decode_indices=[0, 1]), "rows"),
}
# the real towers, whose state_dict names and shapes tests/golden/dinov2_family_names.npz records from the reference's own
# factories (built on the meta device): tower -> (factory, ffn_layer)
REAL_TOWERS = {"dinov2_vits14": ("vit_small", "mlp"), "dinov2_vitl14": ("vit_large", "mlp"), "dinov2_vitg14": ("vit_giant2", "swiglufused")}
# the factory a test geometry is cut from (None: no factory has its width; the class itself is called, as
# tools/gen_golden_dinov2.py does for dino_tiny)
FACTORY = {"dino_tiny_swiglu": (None, "swiglufused"), "dino_s2": ("vit_small", "mlp"), "dino_g2": ("vit_giant2", "swiglufused")}


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


def recorded_schema(tower):
    """[(name, shape)] of the reference factory's state_dict, in its order."""
    g = load_golden("dinov2_family_names")
    return [(str(k), tuple(int(v) for v in s.split(",")) if s else ()) for k, s in zip(g[tower + ".keys"], g[tower + ".shapes"])]
