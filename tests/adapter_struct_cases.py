"""Seeded cases of the CompInvAdapter structs without a LayerNorm ("768-bn", "768-xxx-768", "linear"), shared by the
fixture generator (`tools/gen_golden_adapter_structs.py`, which ran the reference's own classes on them) and the CPU /
GPU tests.  Fixtures: tests/golden/adapter_<case>.npz."""
import numpy as np

from dfd_clip_amd.config import default_compinv_config
from dfd_clip_amd.weights import ARCHS, random_compinv_state_dict, random_state_dict, resolve_layer_indices, synthetic_clips
from tests.cases import EXTRA_INPUTS, load_golden, make_config  # noqa: F401  (load_golden: shared fixture reader)


def _adapter(struct, x):
    return dict(decode_mode="index", adapter__type="normal", adapter__frozen=0, adapter__struct={"type": struct, "x": x})


# Detector cases: name -> (architecture, B, T, config overrides).  ViT-B/32 is the cheapest width-768 tower (49 patches);
# two clips make the BatchNorm's coupling of a batch visible.
CASES = {
    "adapter_tiny_xxx": ("tiny", 2, 4, dict(_adapter("768-xxx-768", 32), decode_indices=[0, 1])),
    "adapter_tiny_linear": ("tiny", 2, 4, dict(_adapter("linear", 32), decode_indices=[0, 1])),
    "adapter_vitb16_xxx": ("ViT-B/16", 1, 2, dict(_adapter("768-xxx-768", 256), decode_indices=[10, 11])),
    "adapter_vitb32_bn": ("ViT-B/32", 2, 2, dict(_adapter("768-bn", 32), decode_indices=[10, 11])),
}
# CompInvEncoder case: name -> (architecture, B, T, decode_stride, struct, x); trained in train mode (BatchNorm on batch
# statistics), the last two layers tapped by stride 6
COMPINV_CASES = {
    "adapter_compinv_bn": ("ViT-B/32", 2, 2, 6, "768-bn", 32),
}
COMP_STRINGS = ["raw", "c23"]
COMPINV_LR, COMPINV_MAX_STEPS = 0.01, 10


def build_case(name):
    arch, B, T, over = CASES[name]
    res, patch, width, layers, heads, _ = ARCHS[arch]
    cfg = make_config(arch, **over)
    sd = random_state_dict(cfg, T, seed=0)
    x, m, y = synthetic_clips(B, T, res, seed=1234, masked_tail=True)
    return dict(name=name, arch=arch, B=B, T=T, cfg=cfg, sd=sd, x=x, m=m, y=y, res=res, patch=patch, width=width,
                layers=layers, heads=heads, layer_indices=resolve_layer_indices(cfg, layers), struct=over["adapter__struct"]["type"])


def build_compinv_case(name):
    arch, B, T, stride, struct, x = COMPINV_CASES[name]
    res, patch, width, layers, heads, _ = ARCHS[arch]
    cfg = default_compinv_config()
    cfg.architecture = arch
    cfg.decode_stride = stride
    cfg.mode = 1
    cfg.adapter.struct = {"type": struct, "x": x}
    sd = random_compinv_state_dict(cfg, seed=0, num_frames=T)
    frames, _, labels = synthetic_clips(B, T, res, seed=1234, masked_tail=False)
    return dict(name=name, arch=arch, B=B, T=T, cfg=cfg, sd=sd, x=frames, labels=labels, comp=COMP_STRINGS[:B], res=res,
                patch=patch, width=width, heads=heads, patches=(res // patch) ** 2, layer_indices=resolve_layer_indices(cfg, layers))


def stored(t):
    """What a fixture keeps of a tensor: all of it up to 4096 elements, else its norm and the first 64."""
    t = t.detach().float()
    if t.numel() <= 4096:
        return {"": t.numpy().copy()}
    return {".norm": np.asarray(t.norm().item(), dtype=np.float32), ".head": t.flatten()[:64].numpy().copy()}
