"""DINOv2 ViT-S/14, ViT-B/14, ViT-L/14 and ViT-g/14 as the frozen foundation (`config.foundation == "dinov2"`), on the CLIP
tower's HIP kernels.

Host-side mirror of the reference's `DINOv2` wrapper (reference `src/models.py:364-391`) around its modified
`dinov2.models.vision_transformer.vit_base(img_size=518, patch_size=14, block_chunks=0, init_values=1.0,
ffn_layer="mlp")`, and around the three other factories of that file (`vit_small`, `vit_large`, and `vit_giant2` with
`ffn_layer="swiglufused"`: the towers of `weights.ARCHS` / `DINO_IMG_SIZE` / `DINO_FFN`; the wrapper itself hard-codes
ViT-B/14, `config.architecture` names another): `.backbone` holds the parameters under the reference's state_dict
names, `.transformer.resblocks` are the backbone's blocks, and `forward(x, feat_keys)` returns one dict per block with `q` / `k` / `v`
`[N, tokens, heads, 64]` (bias included, un-scaled, CLS row kept) and `out` `[N, tokens, width]`.

At 224 px the tower has ViT-L/14's token geometry (14x14 patches, K = 588, 257 tokens, 64-wide heads) at ViT-B/16's
width, so it runs on `VisionTransformer`'s kernel sequence.  What differs, and where it is handled:

  conv bias, cls_token, pos_embed   folded into the operands of DFD_EPI_PATCH_EMBED when the weights are staged:
                                    pos'[0] = pos[0], pos'[1 + p] = resampled pos[1 + p] + conv bias, cls = cls_token.
                                    `pos_embed` is stored for the 518-px grid (37x37) and resampled bicubically to the
                                    grid of the run (16x16) with the reference's scale factor (16 + 0.1) / 37
                                    (`interpolate_pos_encoding`), once per staging, with torch
  no ln_pre                         `_stage` leaves its entry None
  LayerNorm eps = 1e-6              `ln_eps`
  nn.GELU() (erf) in the MLP        `act_epilogue` = DFD_EPI_BIAS_GELU (bf16 and e4m3 operands, bf16 and e4m3 output)
  LayerScale (ls1 / ls2 gamma)      the tower is frozen, so gamma is folded into the Linear before it:
                                    W' = diag(gamma) W, b' = gamma b for attn.proj and mlp.fc2, and the residual
                                    epilogues serve unchanged.  Re-folded whenever the parameters change
                                    (`load_state_dict`, `.to()`, `invalidate()`).
  SwiGLU feed-forward (ViT-g/14)    `mlp.w12` [2H, D] and `mlp.w3` [D, H], H = weights.swiglu_hidden(D) (4096 at D = 1536): the
                                    block's second half runs w12 (plain bias epilogue) -> dfd_swiglu_fwd
                                    (silu(x1) * x2, csrc/swiglu.hip) -> w3 (`VisionTransformer._block`); the staged
                                    block carries w_12 / b_12 / w_3 / b_3 instead of w_fc / b_fc / w_proj / b_proj, with
                                    ls2 folded into w3 as it is into fc2.  Never fragment-blocked, not built for fp8.
The final `norm` and `mask_token` are parameters only (nothing the detector reads passes through them).
"""
import logging
import os
import types

import torch
from torch import nn

from . import capi
from .encoder import VisionTransformer, _Holder, quantize_rows_e4m3
from .weights import ARCHS, DINO_FFN, DINO_IMG_SIZE, swiglu_hidden

CHECKPOINT = "misc/dinov2_vitb14_pretrain.pth"  # where the reference reads it, relative to the working directory
# ... and the published file names of the other towers beside it (test geometries have none: they fall back to ViT-B's
# path, where no file of their shapes can be, and load what the caller hands them)
CHECKPOINTS = {"dinov2_vits14": "misc/dinov2_vits14_pretrain.pth", "dinov2_vitb14": CHECKPOINT,
               "dinov2_vitl14": "misc/dinov2_vitl14_pretrain.pth", "dinov2_vitg14": "misc/dinov2_vitg14_pretrain.pth"}
# `Detector._transform` for this foundation (reference src/models.py:769-779): ImageNet statistics
PIXEL_MEAN = (0.485, 0.456, 0.406)
PIXEL_STD = (0.229, 0.224, 0.225)


class _DinoAttn(_Holder):
    def __init__(self, d):
        super().__init__()
        self.qkv = nn.Linear(d, 3 * d)
        self.proj = nn.Linear(d, d)


class _DinoMlp(_Holder):
    def __init__(self, d):
        super().__init__()
        self.fc1 = nn.Linear(d, 4 * d)
        self.fc2 = nn.Linear(4 * d, d)


class _DinoSwiGLU(_Holder):
    """`SwiGLUFFNFused` (reference dinov2/layers/swiglu_ffn.py:45-63): its two Linears, in its registration order."""

    def __init__(self, d):
        super().__init__()
        h = swiglu_hidden(d)
        self.w12 = nn.Linear(d, 2 * h)
        self.w3 = nn.Linear(h, d)


class _LayerScale(_Holder):
    def __init__(self, d, init_values=1.0):
        super().__init__()
        self.gamma = nn.Parameter(init_values * torch.ones(d))


class _DinoBlock(_Holder):
    def __init__(self, d, heads, ffn="mlp"):
        super().__init__()
        assert ffn in ("mlp", "swiglu"), ffn
        self.norm1 = nn.LayerNorm(d, eps=1e-6)
        self.attn = _DinoAttn(d)
        self.attn.num_heads = heads
        self.ls1 = _LayerScale(d)
        self.norm2 = nn.LayerNorm(d, eps=1e-6)
        self.mlp = _DinoSwiGLU(d) if ffn == "swiglu" else _DinoMlp(d)
        self.ls2 = _LayerScale(d)


class _PatchEmbed(_Holder):
    def __init__(self, d, patch):
        super().__init__()
        self.proj = nn.Conv2d(3, d, kernel_size=patch, stride=patch)


class _Backbone(_Holder):
    """Parameters of `DinoVisionTransformer` in its registration order (so `state_dict()` lists the same keys)."""

    def __init__(self, img_size, patch, d, layers, heads, ffn="mlp"):
        super().__init__()
        self.patch_embed = _PatchEmbed(d, patch)
        self.cls_token = nn.Parameter(1e-6 * torch.randn(1, 1, d))
        self.pos_embed = nn.Parameter(0.02 * torch.randn(1, (img_size // patch) ** 2 + 1, d).clamp_(-2, 2))
        self.blocks = nn.ModuleList([_DinoBlock(d, heads, ffn) for _ in range(layers)])
        self.norm = nn.LayerNorm(d, eps=1e-6)
        self.mask_token = nn.Parameter(torch.zeros(1, d))
        for m in self.modules():  # init_weights_vit_timm
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)


def resample_pos_embed(pos_embed, grid):
    """`interpolate_pos_encoding` (reference dinov2/models/vision_transformer.py:175-198): pos_embed [1, 1 + G*G, D] ->
    [1 + grid*grid, D] for a grid x grid run, the patch part resampled bicubically with scale factor (grid + 0.1) / G."""
    pos = pos_embed.detach().float()
    n = pos.shape[1] - 1
    if n == grid * grid:
        return pos[0]
    G = round(n ** 0.5)
    assert G * G == n, "pos_embed must hold a square grid"
    sf = (grid + 0.1) / G
    patch = torch.nn.functional.interpolate(pos[:, 1:].reshape(1, G, G, -1).permute(0, 3, 1, 2), scale_factor=(sf, sf), mode="bicubic")
    assert patch.shape[-2:] == (grid, grid)
    return torch.cat((pos[0, :1], patch.permute(0, 2, 3, 1).reshape(grid * grid, -1)), dim=0)


class DINOv2(VisionTransformer):
    ln_eps = 1e-6
    act_epilogue = capi.EPI_BIAS_GELU

    def __init__(self, arch="dinov2_vitb14", precision="bf16", checkpoint=CHECKPOINT):
        nn.Module.__init__(self)
        res, patch, width, layers, heads, _ = ARCHS[arch]
        if checkpoint == CHECKPOINT:  # the default follows the tower that was named (None still means: no file)
            checkpoint = CHECKPOINTS.get(arch, CHECKPOINT)
        self.ffn = DINO_FFN[arch]
        self.ffn_hidden = swiglu_hidden(width) if self.ffn == "swiglu" else 0
        if precision == "fp8" and self.ffn == "swiglu":
            raise NotImplementedError(f"precision='fp8' is not built for the SwiGLU feed-forward of {arch}: its w12 -> gate -> w3 runs "
                                      "on bf16 or f32 operands only (no e4m3 gate, no calibration of its activations); use 'bf16' or 'fp32'")
        if precision == "fp8" and width % 256 != 0:
            raise NotImplementedError(f"precision='fp8' is not built for a DINOv2 tower of width {width}: the fp8 GEMM serves "
                                      "N % 256 == 0, K % 128 == 0, K >= 256 (include/dfdclip.h); use 'bf16' or 'fp32'")
        self.backbone = _Backbone(DINO_IMG_SIZE[arch], patch, width, layers, heads, self.ffn)
        if checkpoint and os.path.isfile(checkpoint):
            self.backbone.load_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=True))
        else:
            logging.warning("no checkpoint at %s: the DINOv2 encoder uses its random initialisation", checkpoint)
        # interfaces (reference src/models.py:371-378)
        self.transformer = types.SimpleNamespace(resblocks=self.backbone.blocks)
        self._init_runtime(res, patch, width, layers, heads, precision)
        self.block_num = layers
        self.pixel_mean, self.pixel_std = PIXEL_MEAN, PIXEL_STD

    def _param_device(self):
        return self.backbone.cls_token.device

    def folded_operands(self):
        """f32 operands of the kernel sequence with everything the CLIP tower does not have folded in (module
        docstring): a dict shaped like `VisionTransformer._stage`'s, on the parameters' device (CPU included)."""
        bb = self.backbone
        f32 = lambda t: t.detach().to(torch.float32).contiguous()
        D = self.width
        grid = self.input_resolution // self.patch_size
        pos = resample_pos_embed(bb.pos_embed, grid).clone()
        pos[1:] += bb.patch_embed.proj.bias.detach().float()
        out = dict(w_patch=f32(bb.patch_embed.proj.weight).reshape(D, -1), cls=f32(bb.cls_token).reshape(D), pos=pos.contiguous(), blocks=[])
        for blk in bb.blocks:
            g1, g2 = blk.ls1.gamma.detach().float(), blk.ls2.gamma.detach().float()
            first, last, names = (blk.mlp.w12, blk.mlp.w3, ("w_12", "b_12", "w_3", "b_3")) if self.ffn == "swiglu" else \
                (blk.mlp.fc1, blk.mlp.fc2, ("w_fc", "b_fc", "w_proj", "b_proj"))
            ffn = dict(zip(names, (f32(first.weight), f32(first.bias), (g2[:, None] * last.weight.detach().float()).contiguous(),
                                   (g2 * last.bias.detach().float()).contiguous())))
            out["blocks"].append(dict(
                ffn, ln1=(f32(blk.norm1.weight), f32(blk.norm1.bias)), ln2=(f32(blk.norm2.weight), f32(blk.norm2.bias)),
                w_qkv=f32(blk.attn.qkv.weight), b_qkv=f32(blk.attn.qkv.bias),
                w_out=(g1[:, None] * blk.attn.proj.weight.detach().float()).contiguous(), b_out=(g1 * blk.attn.proj.bias.detach().float()).contiguous()))
        return out

    def _stage(self, dev):
        act = self.act_dtype
        f = self.folded_operands()
        kreal = f["w_patch"].shape[1]
        kpad = (kreal + 63) // 64 * 64  # multiple of the tuned GEMM's K step (588 -> 640); pad columns are zero
        wp = torch.zeros(self.width, kpad, device=dev, dtype=torch.float32)
        wp[:, :kreal] = f["w_patch"]
        p = dict(kpad=kpad, w_patch=wp.to(act).contiguous(), cls=f["cls"], pos=f["pos"], ln_pre=None, blocks=[])
        for i, b in enumerate(f["blocks"]):
            staged = dict(b, idx=i)
            staged.update({k: b[k].to(act).contiguous() for k in ("w_qkv", "w_out", "w_fc", "w_proj", "w_12", "w_3") if k in b})
            if "w_3" in b and b["w_3"].shape[1] % 32 != 0:
                # dfd_gemm takes K in steps of 32: zero columns up to the next one, against the zero pad columns of the
                # workspace's `hidden` (H = 344 -> 352 on the test geometry; ViT-g's 4096 needs none)
                H = b["w_3"].shape[1]
                w3 = torch.zeros(self.width, (H + 31) // 32 * 32, device=dev, dtype=act)
                w3[:, :H] = staged["w_3"]
                staged["w_3"] = w3
            if self.precision == "fp8":  # per output row, AFTER the LayerScale fold (fc2's rows carry their gamma)
                for w, w8, sc in (("w_qkv", "w_qkv8", "s_qkv"), ("w_fc", "w_fc8", "s_fc"), ("w_proj", "w_proj8", "s_proj")):
                    staged[w8], staged[sc] = quantize_rows_e4m3(b[w])
            p["blocks"].append(staged)
        return p

    @torch.no_grad()
    def forward(self, x, feat_keys=("k", "v"), **args):
        """Reference API: frames [N,3,R,R] -> list of per-block dicts with the requested keys of q, k, v, out."""
        if args:
            raise NotImplementedError(f"DINOv2.forward: backbone arguments {sorted(args)} are not built (masks are out of scope)")
        unknown = set(feat_keys) - {"q", "k", "v", "out"}
        if unknown:
            raise KeyError(f"DINOv2.forward: unknown feature keys {sorted(unknown)}")
        full = VisionTransformer.forward(self, x, with_out="out" in feat_keys, with_q="q" in feat_keys)
        return [{k: d[k] for k in feat_keys} for d in full]
