"""Seeded cases of the adapter pre-training model (`CompInvEncoder`), shared by the fixture generator
(`tools/gen_golden_compinv.py`, which ran the reference's own class on them) and the CPU / GPU tests."""
import io
import os
import zipfile

import numpy as np
import torch

from dfd_clip_amd.config import default_compinv_config
from dfd_clip_amd.weights import ARCHS, random_compinv_state_dict, resolve_layer_indices, synthetic_clips

# name -> (architecture, B, T, decode_stride, adapter x); 768-x-768 (the shipped struct, GELU first) in every case.
# tiny: an odd batch (the last clip takes no part); small: 196 patches, width 256.
CASES = {
    "compinv_tiny": ("tiny", 5, 3, 1, 32),
    "compinv_small": ("small", 4, 3, 2, 32),
}
COMP_STRINGS = ["raw", "c23", "c23", "raw", "raw", "c23"]  # per clip; pair 1 has its raw member second
LR, MAX_STEPS = 0.01, 10  # CompInvTrainer: AdamW at LR / 25, OneCycleLR(max_lr=LR, total_steps=MAX_STEPS)


def make_config(arch, stride, x, mode=1):
    cfg = default_compinv_config()
    cfg.architecture = arch
    cfg.decode_stride = stride
    cfg.mode = mode
    cfg.adapter.struct = {"type": "768-x-768", "x": x}
    return cfg


def build_case(name, mode=1):
    arch, B, T, stride, x = CASES[name]
    res, patch, width, layers, heads, _ = ARCHS[arch]
    cfg = make_config(arch, stride, x, mode)
    sd = random_compinv_state_dict(cfg, seed=0)
    frames, _, labels = synthetic_clips(B, T, res, seed=1234, masked_tail=False)
    return dict(name=name, arch=arch, B=B, T=T, cfg=cfg, sd=sd, x=frames, labels=labels, comp=COMP_STRINGS[:B], res=res,
                patch=patch, width=width, heads=heads, patches=(res // patch) ** 2,
                layer_indices=resolve_layer_indices(cfg, layers))


def load_golden(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz")
    return np.load(path, allow_pickle=False)


def save_npz(path, arrays):
    """np.savez_compressed with fixed zip timestamps, so that regenerating a fixture reproduces it byte for byte."""
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                       compress_type=zipfile.ZIP_DEFLATED)


def stored_slices(t):
    """What a fixture keeps of a parameter-shaped tensor: all of it up to 4096 elements, else its norm and the first 64."""
    t = t.detach().float()
    if t.numel() <= 4096:
        return {"": t.numpy().copy()}
    return {".norm": np.asarray(t.norm().item(), dtype=np.float32), ".head": t.flatten()[:64].numpy().copy()}


def loss_f64(kvs_adapted, layer_count):
    """The reference's pair loss (models.py:1017-1051) restated in float64 on the adapted K/V (what both of its operands
    hold): kvs_adapted = per layer {"k", "v"} [B, T, P, h, d].  Returns (recon, match)."""
    b, t, p, h, d = kvs_adapted[0]["k"].shape
    w = b // 2
    diff = torch.zeros(t, p, h, d, dtype=torch.float64)
    for i in range(w):
        for layer in range(layer_count):
            for s in ("k", "v"):
                a = kvs_adapted[layer][s].double()
                diff = diff + (a[2 * i] - a[2 * i + 1]).abs()
    m = (diff / (w * layer_count * 2)).view(p, t, -1).mean(dim=1)
    return torch.zeros((), dtype=torch.float64), m.norm() / p
