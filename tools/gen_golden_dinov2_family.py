#!/usr/bin/env python3
"""Writes tests/golden/dinov2_family_{tiny_swiglu,s2,g2,names}.npz by running the reference's own
`dinov2.models.vision_transformer` factories (`vit_small`, `vit_giant2` with `ffn_layer="swiglufused"`), its `DINOv2`
wrapper (src/models.py) and its `Detector` with `foundation: dinov2` on the seeded cases of tests/dinov2_family_cases.py,
on the CPU.  Needs the reference checkout, so it runs only where that exists; the tests read the fixtures and never run
this.  Nothing of the reference is copied: it is imported.

What stands in for what the reference expects around it, all only inside this process (the first two are
tools/gen_golden_dinov2.py's):
  * `xformers.ops`: softmax(q k^T d^-1/2) v in plain torch;
  * the checkpoint: the wrapper reads misc/dinov2_vitb14_pretrain.pth relative to the working directory, so the seeded
    backbone state is written there in a temporary directory;
  * the tower: the wrapper calls `vit_base`.  While a case is built that name is bound to the case's own factory, called on
    the meta device with the wrapper's arguments (plus `drop_path_uniform=True`, which only keeps the constructor from
    reading a number out of a meta tensor; the rate is 0 either way), CUT to the geometry's depth (`blocks[:layers]`) and
    only then given memory -- ViT-g/14's 40 blocks are never allocated.  `dino_tiny_swiglu`'s width is no factory's: the
    class is called at that size, as the other tool does for `dino_tiny`;
  * the decoder's start from the tower: `ResidualAttentionBlock._apply_reference` maps the names fc1 / fc2 only, so with a
    SwiGLU tower the reference cannot build its decoder at all.  For those cases the LayerNorms are copied as it does and
    the mlp keeps its own initialisation (what dfd_clip_amd.decoder does); every parameter is overwritten by the strict
    load of the seeded state right after, so the stand-in decides nothing that is stored.

Stored per case (the layout of tools/gen_golden_dinov2.py's files, plus the autocast logits):
  enc{l}_{q,k,v,out}        every block's results ("full": everything, and `enc_in`; "rows": token rows `stored_rows`)
  logits / losses / video_feature, layer_indices
  logits_bf16 / losses_bf16 the same eval forward under torch.autocast("cpu", bfloat16)
  train_task_loss, grad0.<param>[.norm|.head], step_losses, after2.<param>[.head]   two SGD steps
  keys / shapes             the reference Detector's state_dict schema
dinov2_family_names.npz: `<tower>.keys` / `<tower>.shapes` of the three real towers' factories on the meta device.

usage: python tools/gen_golden_dinov2_family.py [case ... | names]
"""
import contextlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import REF, load_reference  # noqa: E402
from dfd_clip_amd.weights import ARCHS, DINO_FFN, DINO_IMG_SIZE  # noqa: E402
from tests.compinv_cases import save_npz, stored_slices  # noqa: E402
from tests.dinov2_family_cases import CASES, FACTORY, REAL_TOWERS, STORED_ROWS, build_case  # noqa: E402
from tools.gen_golden_dinov2 import stand_in_xformers  # noqa: E402

MAX_BYTES = 1_000_000


def factory_tower(vt, factory, ffn_layer, arch, **wrapper_args):
    """The backbone of `arch` from the reference's own factory, on the meta device, cut to the geometry's depth."""
    from functools import partial
    res, patch, width, layers, heads, _ = ARCHS[arch]
    args = dict(wrapper_args, img_size=DINO_IMG_SIZE[arch], patch_size=patch, ffn_layer=ffn_layer, drop_path_uniform=True)
    with torch.device("meta"):
        if factory is None:
            bb = vt.DinoVisionTransformer(embed_dim=width, depth=layers, num_heads=heads, mlp_ratio=4,
                                          block_fn=partial(vt.Block, attn_class=vt.MemEffAttention), **args)
        else:
            bb = getattr(vt, factory)(**args)
    assert bb.embed_dim == width and bb.blocks[0].attn.num_heads == heads and not bb.chunked_blocks
    assert len(bb.blocks) >= layers
    bb.blocks = torch.nn.ModuleList(list(bb.blocks)[:layers])
    return bb


@contextlib.contextmanager
def reference_wrapper_for(mm, arch, backbone_state):
    """`mm.DINOv2()` builds the tower of `arch` holding `backbone_state` while this is active."""
    import dinov2.models.vision_transformer as vt
    res, patch, width, layers, heads, _ = ARCHS[arch]
    factory, ffn_layer = FACTORY[arch]
    orig_cls, orig_vit_base, orig_apply, cwd = mm.DINOv2, vt.vit_base, mm.ResidualAttentionBlock._apply_reference, os.getcwd()

    def tower(img_size, patch_size, ffn_layer="mlp", **kw):  # called by the wrapper in place of vit_base
        assert img_size == 518 and patch_size == 14 and ffn_layer == "mlp"
        return factory_tower(vt, factory, FACTORY[arch][1], arch, **kw).to_empty(device="cpu")

    def build():
        enc = orig_cls()
        enc.heads, enc.width, enc.input_resolution = heads, width, res
        return enc

    def apply_reference_swiglu(self, config, block_index, layer_indices, reference_layers):
        src = reference_layers[layer_indices[block_index]]
        self.ln_1.load_state_dict(src.norm1.state_dict())
        self.ln_2.load_state_dict(src.norm2.state_dict())

    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "misc"))
        torch.save(backbone_state, os.path.join(tmp, "misc", "dinov2_vitb14_pretrain.pth"))
        os.chdir(tmp)
        vt.vit_base, mm.DINOv2 = tower, build
        if DINO_FFN[arch] == "swiglu":
            assert ffn_layer == "swiglufused"
            mm.ResidualAttentionBlock._apply_reference = apply_reference_swiglu
        try:
            yield
        finally:
            vt.vit_base, mm.DINOv2, mm.ResidualAttentionBlock._apply_reference = orig_vit_base, orig_cls, orig_apply
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
    assert len(det.encoder.backbone.blocks) == c["layers"]
    if DINO_FFN[c["arch"]] == "swiglu":
        assert type(det.encoder.backbone.blocks[0].mlp).__name__ == "SwiGLUFFNFused"
    det.eval()
    out = {}
    with torch.no_grad():
        losses, logits = det(x, [y], m, single_task=0)
        plog, feats = det.predict(x, m, with_video_features=True)
        enc = det.encoder(x.flatten(0, 1), feat_keys=["q", "k", "v", "out"])
        enc_in = det.encoder.backbone.prepare_tokens_with_masks(x.flatten(0, 1))
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        losses_a, logits_a = det(x, [y], m, single_task=0)
    assert torch.equal(plog[0], logits[0]) and len(enc) == c["layers"]
    assert tuple(enc[0]["k"].shape) == (B * T, (c["res"] // c["patch"]) ** 2 + 1, c["heads"], 64)
    out["logits"], out["losses"], out["video_feature"] = logits[0].numpy(), losses[0].numpy(), feats["video"].numpy()
    out["logits_bf16"], out["losses_bf16"] = logits_a[0].float().numpy(), losses_a[0].float().numpy()
    out["layer_indices"] = np.asarray(det.layer_indices)
    if c["store"] == "full":
        out["enc_in"] = enc_in.numpy()
    else:
        out["stored_rows"] = np.asarray(STORED_ROWS)
    for l, d in enumerate(enc):
        for key in ("q", "k", "v", "out"):
            out[f"enc{l}_{key}"] = (d[key] if c["store"] == "full" else d[key][:, STORED_ROWS]).numpy()
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
    assert os.path.getsize(path) <= MAX_BYTES, (path, os.path.getsize(path))
    print(f"{name}: logits={out['logits'].tolist()} |bf16 - fp32|max={np.abs(out['logits_bf16'] - out['logits']).max():.3e} "
          f"step_losses={step_losses} -> {path} ({os.path.getsize(path) / 1e6:.3f} MB)")


def run_names():
    """Names and shapes of the three real towers' state_dicts, from the factories themselves (no memory: meta device)."""
    import dinov2.models.vision_transformer as vt
    out = {}
    for tower, (factory, ffn_layer) in REAL_TOWERS.items():
        res, patch, width, layers, heads, _ = ARCHS[tower]
        bb = factory_tower(vt, factory, ffn_layer, tower, block_chunks=0, init_values=1.0)
        assert len(bb.blocks) == layers, (tower, len(bb.blocks))
        sd = bb.state_dict()
        out[tower + ".keys"] = np.asarray(list(sd))
        out[tower + ".shapes"] = np.asarray([",".join(map(str, t.shape)) for t in sd.values()])
        print(f"{tower}: {len(sd)} tensors, {sum(t.numel() for t in sd.values()) / 1e6:.1f} M parameters")
    path = os.path.join(ROOT, "tests", "golden", "dinov2_family_names.npz")
    save_npz(path, out)
    print(f"-> {path} ({os.path.getsize(path) / 1e3:.1f} kB)")


if __name__ == "__main__":
    torch.set_num_threads(8)
    stand_in_xformers()
    sys.path.insert(0, REF)  # the reference imports its `dinov2` package by that name
    mm, Acc, to_cn = load_reference()
    for case in (sys.argv[1:] or list(CASES) + ["names"]):
        if case == "names":
            run_names()
        else:
            run_case(case, mm, Acc, to_cn)
