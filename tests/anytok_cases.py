"""The seeded parity case at a token count outside the two MFMA attention windows: `small24`, ViT-L/14@336px's token
geometry (24x24 patches of 14 px, K = 588, 577 tokens) at width 128.  Same recipe as `small14` in tests/cases.py;
tools/gen_golden_anytok.py ran the reference itself on it to produce tests/golden/small24.npz."""
from dfd_clip_amd.weights import ARCHS, random_state_dict, resolve_layer_indices, synthetic_clips
from tests.cases import load_golden, make_config, oracle_kwargs  # noqa: F401

# name -> (architecture, B, T, config overrides)
CASES = {
    "small24": ("small24", 2, 3, dict(decode_mode="index", decode_indices=[0, 1])),
}
STORE = "medium"  # what oracle/gen_golden.py keeps of the encoder: K / V row slices of the tapped layers, two frames


def build_case(name):
    arch, B, T, over = CASES[name]
    res, patch, width, layers, heads, _ = ARCHS[arch]
    cfg = make_config(arch, **over)
    sd = random_state_dict(cfg, T, seed=0)
    x, m, y = synthetic_clips(B, T, res, seed=1234, masked_tail=True)
    return dict(name=name, arch=arch, B=B, T=T, cfg=cfg, sd=sd, x=x, m=m, y=y, res=res, patch=patch,
                width=width, layers=layers, heads=heads, layer_indices=resolve_layer_indices(cfg, layers))
