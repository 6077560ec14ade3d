#!/usr/bin/env python3
"""Writes tests/golden/dinov2_{tiny,tiny_adapter,vitb14}.npz by running the reference's own `DINOv2` wrapper
(src/models.py) around its own `dinov2.models.vision_transformer`, and its `Detector` with `foundation: dinov2`, on the
seeded cases of tests/dinov2_cases.py, in fp32 on the CPU.  Needs the reference checkout, so it runs only where that
exists; the tests read the fixtures and never run this.  Nothing of the reference is copied: it is imported.

Two things stand in for what the reference expects around it, both only inside this process:
  * `xformers.ops` (the reference's MemEffAttention imports it): `memory_efficient_attention(q, k, v)` =
    softmax(q k^T d^-1/2) v on [B, N, H, d] tensors in plain torch, `unbind` = torch.unbind;
  * the checkpoint: the wrapper reads misc/dinov2_vitb14_pretrain.pth relative to the working directory, so the seeded
    backbone state is written there in a temporary directory.  For the tiny geometry the module's `vit_base` is
    replaced by a call of the same `DinoVisionTransformer` class at the tiny size, and the wrapper's hard-coded
    heads / width / input_resolution are set to match.

Stored per case (the layout of oracle/gen_golden.py's files):
  enc{l}_{q,k,v,out}        the tower's per-block results ("full": everything; "rows": token rows `stored_rows` of the
                            tapped blocks' k / v, the first tapped block's q, the last block's out)
  enc_in                    the first block's input (patch embedding + cls + resampled pos_embed), "full" only
  logits / losses / video_feature, layer_indices
  train_task_loss, grad0.<param>[.norm|.head], step_losses, after2.<param>[.head]   two SGD steps
  keys / shapes             the reference Detector's state_dict schema

usage: python tools/gen_golden_dinov2.py [case ...]
"""
import contextlib
import os
import sys
import tempfile
import types
from functools import partial

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import REF, load_reference  # noqa: E402
from dfd_clip_amd.weights import ARCHS, DINO_IMG_SIZE  # noqa: E402
from tests.compinv_cases import save_npz, stored_slices  # noqa: E402
from tests.dinov2_cases import CASES, STORED_ROWS, build_case  # noqa: E402


def stand_in_xformers():
    ops = types.ModuleType("xformers.ops")

    def memory_efficient_attention(q, k, v, attn_bias=None):
        assert attn_bias is None
        q, k, v = (t.transpose(1, 2) for t in (q, k, v))  # [B, H, N, d]
        return ((q @ k.transpose(-2, -1)) * q.shape[-1] ** -0.5).softmax(dim=-1).matmul(v).transpose(1, 2)

    ops.memory_efficient_attention = memory_efficient_attention
    ops.unbind = torch.unbind
    ops.fmha = types.SimpleNamespace()
    ops.scaled_index_add = ops.index_select_cat = None
    xf = types.ModuleType("xformers")
    xf.ops = ops
    sys.modules.update({"xformers": xf, "xformers.ops": ops})


@contextlib.contextmanager
def reference_wrapper_for(mm, arch, backbone_state):
    """`mm.DINOv2()` builds the tower of `arch` holding `backbone_state` while this is active."""
    import dinov2.models.vision_transformer as vt
    res, patch, width, layers, heads, _ = ARCHS[arch]
    orig_cls, orig_vit_base, cwd = mm.DINOv2, vt.vit_base, os.getcwd()

    def vit_at_size(img_size, patch_size, **kw):
        assert img_size == 518 and patch_size == 14
        return vt.DinoVisionTransformer(img_size=DINO_IMG_SIZE[arch], patch_size=patch, embed_dim=width, depth=layers, num_heads=heads,
                                        mlp_ratio=4, block_fn=partial(vt.Block, attn_class=vt.MemEffAttention), **kw)

    def build():
        enc = orig_cls()
        enc.heads, enc.width, enc.input_resolution = heads, width, res
        return enc

    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "misc"))
        torch.save(backbone_state, os.path.join(tmp, "misc", "dinov2_vitb14_pretrain.pth"))
        os.chdir(tmp)
        if arch != "dinov2_vitb14":
            vt.vit_base, mm.DINOv2 = vit_at_size, build
        try:
            yield
        finally:
            vt.vit_base, mm.DINOv2 = orig_vit_base, orig_cls
            os.chdir(cwd)


def run_case(name, mm, Acc, to_cn):
    c = build_case(name)
    B, T, x, m, y, sd = c["B"], c["T"], c["x"], c["m"], c["y"], c["sd"]
    cfg = c["cfg"].clone()
    backbone = {k[len("encoder.backbone."):]: v for k, v in sd.items() if k.startswith("encoder.backbone.")}
    torch.manual_seed(1)
    with reference_wrapper_for(mm, c["arch"], backbone):
        det = mm.Detector(to_cn(cfg), T, Acc())
    res = det.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    det.eval()
    out = {}
    with torch.no_grad():
        losses, logits = det(x, [y], m, single_task=0)
        plog, feats = det.predict(x, m, with_video_features=True)
        enc = det.encoder(x.flatten(0, 1), feat_keys=["q", "k", "v", "out"])
        enc_in = det.encoder.backbone.prepare_tokens_with_masks(x.flatten(0, 1))
    assert torch.equal(plog[0], logits[0]) and len(enc) == c["layers"]
    assert tuple(enc[0]["k"].shape) == (B * T, (c["res"] // c["patch"]) ** 2 + 1, c["heads"], 64)
    out["logits"], out["losses"], out["video_feature"] = logits[0].numpy(), losses[0].numpy(), feats["video"].numpy()
    out["layer_indices"] = np.asarray(det.layer_indices)
    if c["store"] == "full":
        out["enc_in"] = enc_in.numpy()
        for l, d in enumerate(enc):
            for key in ("q", "k", "v", "out"):
                out[f"enc{l}_{key}"] = d[key].numpy()
    elif c["store"] == "rows":
        out["stored_rows"] = np.asarray(STORED_ROWS)
        lidx = list(det.layer_indices)
        for l in lidx:
            for key in ("k", "v"):
                out[f"enc{l}_{key}"] = enc[l][key][:, STORED_ROWS].numpy()
        out[f"enc{lidx[0]}_q"] = enc[lidx[0]]["q"][:, STORED_ROWS].numpy()
        out[f"enc{c['layers'] - 1}_out"] = enc[-1]["out"][:, STORED_ROWS].numpy()
    full = det.state_dict()
    out["keys"] = np.asarray(list(full))
    out["shapes"] = np.asarray([",".join(map(str, t.shape)) for t in full.values()])
    # training contract (oracle/gen_golden.py): forward(train=True) -> backward(mean loss) -> two SGD steps on one batch
    det.train()
    opt = det.configure_optimizers(0.01)
    step_losses = []
    for step in range(2):
        opt.zero_grad()
        tl, tz, other = det(x, [y], m, train=True, single_task=0)
        loss = tl[0].mean() + sum(other.values())
        loss.backward()
        if step == 0:
            out["train_task_loss"] = tl[0].detach().numpy().copy()
            for pn, p in det.named_parameters():
                assert (p.grad is None) == pn.startswith("encoder."), pn
                if p.grad is not None:
                    for suffix, a in stored_slices(p.grad).items():
                        out[f"grad0.{pn}{suffix}"] = a
        step_losses.append(loss.item())
        opt.step()
    out["step_losses"] = np.asarray(step_losses)
    for pn, p in det.named_parameters():
        if p.requires_grad:
            t = p.detach()
            out["after2." + pn + ("" if t.numel() <= 4096 else ".head")] = (t if t.numel() <= 4096 else t.flatten()[:64]).numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    save_npz(path, out)
    print(f"{name}: logits={out['logits'].tolist()} step_losses={step_losses} -> {path} ({os.path.getsize(path) / 1e6:.3f} MB)")


if __name__ == "__main__":
    torch.set_num_threads(8)
    stand_in_xformers()
    sys.path.insert(0, REF)  # the reference imports its `dinov2` package by that name
    mm, Acc, to_cn = load_reference()
    for case in (sys.argv[1:] or list(CASES)):
        run_case(case, mm, Acc, to_cn)
