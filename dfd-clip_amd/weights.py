"""Weight schema, seeded random initialisation and device-side preparation.

The state_dict key names and shapes are the reference's (`Detector.state_dict()`, schema
listed in SURVEY.md §8b; producers: reference `src/clip/model.py:255-274`, `:176-181`,
`:203-213` and `src/models.py:130-131`, `:155-166`, `:287-318`), so a reference
`best_weights.pt` loads unchanged and a checkpoint written here loads into the reference.

Pretrained CLIP weights cannot be fetched offline (reference `src/clip/clip.py:30-40`), so
benchmarks and parity tests use `random_state_dict`: a numpy PCG64 stream (stable across
machines and library versions, unlike `torch.manual_seed` streams) scaled so that
activations stay O(1) through the stack.
"""
from collections import OrderedDict

import numpy as np
import torch

# name -> (input_resolution, patch_size, width, layers, heads, output_dim)
# (reference `src/clip/model.py:453-496` infers the same numbers from checkpoint shapes).
ARCHS = {
    "ViT-B/16": (224, 16, 768, 12, 12, 512),
    "ViT-B/32": (224, 32, 768, 12, 12, 512),
    "ViT-L/14": (224, 14, 1024, 24, 16, 768),
    "ViT-L/14@336px": (336, 14, 1024, 24, 16, 768),  # 24x24 patches: 577 tokens
    # test-only shapes: every layout rule of the real model at a fraction of the size
    "tiny": (32, 16, 128, 2, 2, 64),
    "small": (224, 16, 256, 3, 4, 64),
    "small14": (224, 14, 128, 2, 2, 64),  # ViT-L/14's token geometry: 14x14 patches (K = 588), 257 tokens
    "small24": (336, 14, 128, 2, 2, 64),  # ViT-L/14@336px's token geometry: 24x24 patches (K = 588), 577 tokens
    # DINOv2 towers (`config.foundation == "dinov2"`; dinov2.py): resolution of the RUN, no output projection.  The
    # reference wrapper hard-codes ViT-B/14 (src/models.py:368); `dino_tiny` is the test geometry
    "dinov2_vitb14": (224, 14, 768, 12, 12, 0),
    "dino_tiny": (28, 14, 128, 2, 2, 0),
    "dino_w768": (28, 14, 768, 2, 12, 0),  # dino_tiny's 5 tokens per frame at a width the fp8 GEMM serves (K % 256 == 0, K >= 768)
    # the other factories of the reference's dinov2/models/vision_transformer.py: vit_small, vit_large, vit_giant2 (whose
    # feed-forward is the SwiGLU of `DINO_FFN`), and their test geometries
    "dinov2_vits14": (224, 14, 384, 12, 6, 0),
    "dinov2_vitl14": (224, 14, 1024, 24, 16, 0),
    "dinov2_vitg14": (224, 14, 1536, 40, 24, 0),
    "dino_tiny_swiglu": (28, 14, 128, 2, 2, 0),  # dino_tiny with the SwiGLU feed-forward (H = 344: no multiple of 64)
    "dino_s2": (28, 14, 384, 2, 6, 0),  # ViT-S/14's width and heads, 5 tokens, two layers
    "dino_g2": (224, 14, 1536, 2, 24, 0),  # ViT-g/14's width, heads, feed-forward (H = 4096) and 257 tokens, two layers
}
# ... and the image size their `pos_embed` is stored for (518 px = a 37x37 grid, resampled to the run's grid; the test
# geometries 70 px = 5x5 -> 2x2)
DINO_IMG_SIZE = {"dinov2_vitb14": 518, "dino_tiny": 70, "dino_w768": 70, "dinov2_vits14": 518, "dinov2_vitl14": 518, "dinov2_vitg14": 518,
                 "dino_tiny_swiglu": 70, "dino_s2": 70, "dino_g2": 518}
# ... and their feed-forward: "mlp" = fc1 -> GELU -> fc2 with 4 x width hidden channels; "swiglu" = the reference's
# `ffn_layer="swiglufused"` (dinov2/layers/swiglu_ffn.py): w12 -> silu(x1) * x2 -> w3 with `swiglu_hidden(width)` channels
DINO_FFN = {name: "swiglu" if name in ("dinov2_vitg14", "dino_tiny_swiglu", "dino_g2") else "mlp" for name in DINO_IMG_SIZE}

# The towers by the names of the published model cards (facebook/dinov2-small / -base / -large / -giant): what a config may
# carry in `architecture` beside a key of `DINO_IMG_SIZE`.  For ViT-L/14 it is the ONLY spelling `model_arch` takes: that
# `architecture: dinov2_vitl14` is refused under this foundation is pinned behaviour from before the tower existed
# (tests/test_dinov2_cpu.py), and it stays.
DINO_ALIASES = {"dinov2-small": "dinov2_vits14", "dinov2-base": "dinov2_vitb14", "dinov2-large": "dinov2_vitl14", "dinov2-giant": "dinov2_vitg14"}
DINO_ALIAS_ONLY = ("dinov2_vitl14",)


def swiglu_hidden(width):
    """Hidden channels of `SwiGLUFFNFused(in_features=width, hidden_features=4 * width)`: two thirds of the MLP's, rounded up to
    a multiple of 8 (1536 -> 4096, 128 -> 344)."""
    return (int(4 * width * 2 / 3) + 7) // 8 * 8


# the model names the reference's `clip.load` knows (src/clip/clip.py:30-40): what a reference config carries in `architecture`
REFERENCE_CLIP_NAMES = ("RN50", "RN101", "RN50x4", "RN50x16", "RN50x64", "ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px")


def model_arch(config):
    """The `ARCHS` row a config runs on.  With `foundation: dinov2` the reference ignores `architecture` and builds
    ViT-B/14 (src/models.py:441-444), and its shipped dino configs still carry `architecture: ViT-B/16`.  So here: one
    of the reference's CLIP model names (or no entry) is ignored in the same way; the name of a DINOv2 geometry of
    `DINO_IMG_SIZE` or a model-card name of `DINO_ALIASES` selects it (`dino_tiny` for tests; ViT-L/14 by its alias only); anything else -- this project's CLIP test geometries such as
    "tiny" -- is refused, rather than answered with an 86 M-parameter ViT-B/14 nobody named."""
    if "foundation" in config and config.foundation == "dinov2":
        name = config.architecture if "architecture" in config else None
        if name in DINO_ALIASES:
            return DINO_ALIASES[name]
        if name in DINO_IMG_SIZE and name not in DINO_ALIAS_ONLY:
            return name
        if name is None or name in REFERENCE_CLIP_NAMES:
            return "dinov2_vitb14"
        if name in DINO_ALIAS_ONLY:
            alias = next(a for a, n in DINO_ALIASES.items() if n == name)
            raise NotImplementedError(f"foundation 'dinov2' with architecture {name!r}: that spelling has always been refused here and "
                                      f"stays so; the tower is built, name it architecture: {alias!r}")
        raise NotImplementedError(f"foundation 'dinov2' with architecture {name!r}: no DINOv2 tower of that geometry is built "
                                  f"(built: {sorted(n for n in DINO_IMG_SIZE if n not in DINO_ALIAS_ONLY) + sorted(DINO_ALIASES)}; "
                                  "the reference's CLIP model names are ignored, as in the reference)")
    return config.architecture


def dinov2_schema(arch):
    """`DINOv2.state_dict()` (reference src/models.py:364-391 around dinov2/models/vision_transformer.py): key -> shape."""
    res, patch, width, layers, heads, _ = ARCHS[arch]
    s = OrderedDict()
    s["backbone.cls_token"] = (1, 1, width)
    s["backbone.pos_embed"] = (1, (DINO_IMG_SIZE[arch] // patch) ** 2 + 1, width)
    s["backbone.mask_token"] = (1, width)
    s["backbone.patch_embed.proj.weight"] = (width, 3, patch, patch)
    s["backbone.patch_embed.proj.bias"] = (width,)
    for l in range(layers):
        p = f"backbone.blocks.{l}."
        s[p + "norm1.weight"] = (width,)
        s[p + "norm1.bias"] = (width,)
        s[p + "attn.qkv.weight"] = (3 * width, width)
        s[p + "attn.qkv.bias"] = (3 * width,)
        s[p + "attn.proj.weight"] = (width, width)
        s[p + "attn.proj.bias"] = (width,)
        s[p + "ls1.gamma"] = (width,)
        s[p + "norm2.weight"] = (width,)
        s[p + "norm2.bias"] = (width,)
        if DINO_FFN[arch] == "swiglu":
            H = swiglu_hidden(width)
            s[p + "mlp.w12.weight"] = (2 * H, width)
            s[p + "mlp.w12.bias"] = (2 * H,)
            s[p + "mlp.w3.weight"] = (width, H)
            s[p + "mlp.w3.bias"] = (width,)
        else:
            s[p + "mlp.fc1.weight"] = (4 * width, width)
            s[p + "mlp.fc1.bias"] = (4 * width,)
            s[p + "mlp.fc2.weight"] = (width, 4 * width)
            s[p + "mlp.fc2.bias"] = (width,)
        s[p + "ls2.gamma"] = (width,)
    s["backbone.norm.weight"] = (width,)
    s["backbone.norm.bias"] = (width,)
    return s


def encoder_schema(arch):
    res, patch, width, layers, heads, out_dim = ARCHS[arch]
    tokens = (res // patch) ** 2 + 1
    s = OrderedDict()
    s["class_embedding"] = (width,)
    s["positional_embedding"] = (tokens, width)
    s["proj"] = (width, out_dim)
    s["conv1.weight"] = (width, 3, patch, patch)
    s["ln_pre.weight"] = (width,)
    s["ln_pre.bias"] = (width,)
    for l in range(layers):
        p = f"transformer.resblocks.{l}."
        s[p + "attn.in_proj_weight"] = (3 * width, width)
        s[p + "attn.in_proj_bias"] = (3 * width,)
        s[p + "attn.out_proj.weight"] = (width, width)
        s[p + "attn.out_proj.bias"] = (width,)
        s[p + "ln_1.weight"] = (width,)
        s[p + "ln_1.bias"] = (width,)
        s[p + "mlp.c_fc.weight"] = (4 * width, width)
        s[p + "mlp.c_fc.bias"] = (4 * width,)
        s[p + "mlp.c_proj.weight"] = (width, 4 * width)
        s[p + "mlp.c_proj.bias"] = (width,)
        s[p + "ln_2.weight"] = (width,)
        s[p + "ln_2.bias"] = (width,)
    s["ln_post.weight"] = (width,)
    s["ln_post.bias"] = (width,)
    return s


def decoder_schema(arch, num_frames, n_blocks, out_dims, temporal_position=True,
                   aug_query=False, global_prediction=False, layer_indices=None):
    res, patch, width, layers, heads, _ = ARCHS[arch]
    s = OrderedDict()
    s["class_embedding"] = (width,)
    if temporal_position:
        s["positional_embedding"] = (num_frames, 1, heads, width // heads)
    s["ln_pre.weight"] = (width,)
    s["ln_pre.bias"] = (width,)
    if aug_query:
        for i in range(n_blocks - 1):
            s[f"transformer.augment_query_{i}"] = (width,)
    for b in range(n_blocks):
        p = f"transformer.resblocks.{b}."
        s[p + "attn.in_proj.weight"] = (2 * width, width)
        s[p + "attn.in_proj.bias"] = (2 * width,)
        s[p + "attn.out_proj.weight"] = (width, width)
        s[p + "attn.out_proj.bias"] = (width,)
        s[p + "ln_1.weight"] = (width,)
        s[p + "ln_1.bias"] = (width,)
        s[p + "mlp.c_fc.weight"] = (4 * width, width)
        s[p + "mlp.c_fc.bias"] = (4 * width,)
        s[p + "mlp.c_proj.weight"] = (width, 4 * width)
        s[p + "mlp.c_proj.bias"] = (width,)
        s[p + "ln_2.weight"] = (width,)
        s[p + "ln_2.bias"] = (width,)
    s["ln_post.weight"] = (width,)
    s["ln_post.bias"] = (width,)
    for i, od in enumerate(out_dims):
        if global_prediction:
            for l in layer_indices:
                s[f"proj{i}x{od}_L{l}"] = (width, od)
        else:
            s[f"proj{i}x{od}"] = (width, od)
    return s


def adapter_schema(arch, n_blocks, struct_type, x, num_frames=None):
    """`CompInvAdapter` state (reference `src/models.py:783-928`): parameters, and for "768-bn" its BatchNorm2d(num_frames)
    buffers (`running_mean` / `running_var` [T], `num_batches_tracked` [] int64)."""
    res, patch, width, layers, heads, _ = ARCHS[arch]
    patches = (res // patch) ** 2
    s = OrderedDict()
    for i in range(n_blocks):
        for j in ("k", "v"):
            p = f"l{i}_{j}."
            if struct_type == "768-x-768-nln":
                s[p + "0.weight"] = (x, width)
                s[p + "1.weight"] = (patches, x)
                s[p + "1.bias"] = (patches, x)
                s[p + "4.weight"] = (width, x)
            elif struct_type in ("768-x-768-ln", "768-x-768-z0"):
                s[p + "0.weight"] = (x, width)
                s[p + "1.weight"] = (x,)
                s[p + "1.bias"] = (x,)
                s[p + "4.weight"] = (width, x)
            elif struct_type in ("768-x-768", "legacy-768-x-768"):  # Linear, GELU, LayerNorm, [Dropout,] Linear
                s[p + "0.weight"] = (x, width)
                s[p + "2.weight"] = (x,)
                s[p + "2.bias"] = (x,)
                s[p + ("4.weight" if struct_type == "768-x-768" else "3.weight")] = (width, x)
            elif struct_type == "768-bn":  # Linear(768, 768), BatchNorm2d(num_frames), Dropout
                if num_frames is None:
                    raise ValueError("768-bn: the BatchNorm's channel count is num_frames")
                s[p + "0.weight"] = (768, 768)
                for k in ("1.weight", "1.bias", "1.running_mean", "1.running_var"):
                    s[p + k] = (num_frames,)
                s[p + "1.num_batches_tracked"] = ()
            elif struct_type == "768-xxx-768":  # Linear, GELU, Dropout, Linear, GELU, Dropout, Linear, Dropout
                s[p + "0.weight"] = (x, width)
                s[p + "3.weight"] = (x, x)
                s[p + "6.weight"] = (width, x)
            elif struct_type == "linear":
                s[p + "0.weight"] = (width, width)
            else:
                raise NotImplementedError(struct_type)
    return s


def _fill(rng, name, shape):
    """One tensor of the seed recipe.  Linear/conv weights ~ N(0, fan_in^-1) keep activations
    O(1); LayerNorm gains near 1 and all biases small but non-zero so that every gain/bias
    path is exercised by the parity tests."""
    leaf = name.split(".")[-1]
    if leaf == "num_batches_tracked":  # BatchNorm buffers: a few steps already taken, statistics well off (0, 1)
        return torch.tensor(int(rng.integers(1, 100)), dtype=torch.int64)
    if leaf == "running_mean":
        return torch.from_numpy(np.ascontiguousarray(0.1 * rng.standard_normal(shape), dtype=np.float32))
    if leaf == "running_var":
        return torch.from_numpy(np.ascontiguousarray(np.exp(0.3 * rng.standard_normal(shape)) * 0.8, dtype=np.float32))
    if leaf == "gamma":  # LayerScale: well off 1 and of both signs of deviation, so a folding error shows
        return torch.from_numpy(np.ascontiguousarray(np.exp(0.4 * rng.standard_normal(shape)) * 0.7, dtype=np.float32))
    if leaf in ("cls_token", "pos_embed", "mask_token"):
        return torch.from_numpy(np.ascontiguousarray((shape[-1] ** -0.5) * rng.standard_normal(shape), dtype=np.float32))
    is_ln = ".norm" in name or ".ln_" in name or name.startswith("ln_") or (name.split(".")[-2:-1] == ["1"]) or \
        (name.split(".")[-2:-1] == ["2"] and len(shape) == 1)
    if is_ln and leaf == "weight":
        a = 1.0 + 0.05 * rng.standard_normal(shape)
    elif leaf == "bias" or leaf.endswith("in_proj_bias"):
        a = 0.02 * rng.standard_normal(shape)
    elif "augment_query" in name:
        a = 0.02 * rng.standard_normal(shape)
    elif leaf in ("class_embedding", "positional_embedding", "proj") or leaf.startswith("proj"):
        width = shape[0] if leaf.startswith("proj") else shape[-1]
        if leaf == "positional_embedding" and len(shape) == 4:
            width = shape[2] * shape[3]
        a = (width ** -0.5) * rng.standard_normal(shape)
    else:  # linear / conv weight [out, in, ...]
        fan_in = int(np.prod(shape[1:]))
        a = (fan_in ** -0.5) * rng.standard_normal(shape)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def resolve_layer_indices(config, n_layers):
    """Reference `src/models.py:458-463`."""
    if config.decode_mode == "stride":
        return list(range(0, n_layers, config.decode_stride))
    if config.decode_mode == "index":
        return list(config.decode_indices)
    raise Exception(f"Unknown decode type: {config.decode_mode}")


def random_state_dict(config, num_frames, seed=0):
    """Seeded fp32 `Detector` state_dict (reference key names).  The decoder's ln_1 / ln_2 /
    mlp start as copies of encoder layer `layer_indices[i]`, as the reference's
    `_apply_reference` does (`src/models.py:226-229`, concat_ref == 0).  A SwiGLU tower has no fc1 / fc2 to copy (the
    reference's `fetch_mlp_params` maps those two names only, and a decoder block is always c_fc -> QuickGELU -> c_proj):
    there the decoder's mlp keeps its own seeded fill and only the two LayerNorms are copies."""
    arch = model_arch(config)
    dino = "foundation" in config and config.foundation == "dinov2"
    res, patch, width, layers, heads, _ = ARCHS[arch]
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k, shp in (dinov2_schema(arch) if dino else encoder_schema(arch)).items():
        sd["encoder." + k] = _fill(rng, k, shp)
    lidx = resolve_layer_indices(config, layers)
    op = config.op_mode
    dsch = decoder_schema(
        arch, num_frames, len(lidx), list(config.out_dim),
        temporal_position=bool("temporal_position" in op and op.temporal_position),
        aug_query=bool("aug_query" in op and op.aug_query),
        global_prediction=bool("global_prediction" in op and op.global_prediction),
        layer_indices=lidx)
    for k, shp in dsch.items():
        sd["decoder." + k] = _fill(rng, k, shp)
    if not ("concat_ref" in config and config.concat_ref):
        for b, l in enumerate(lidx):
            for part in ("ln_1.weight", "ln_1.bias", "ln_2.weight", "ln_2.bias", "mlp.c_fc.weight",
                         "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias"):
                src = f"encoder.transformer.resblocks.{l}.{part}"
                if dino and DINO_FFN[arch] == "swiglu" and part.startswith("mlp."):
                    continue
                if dino:  # norm1 / norm2 / mlp.fc1 / mlp.fc2 of the backbone's block (reference src/models.py:192-209)
                    theirs = part
                    for a_, b_ in (("ln_1", "norm1"), ("ln_2", "norm2"), ("c_fc", "fc1"), ("c_proj", "fc2")):
                        theirs = theirs.replace(a_, b_)
                    src = f"encoder.backbone.blocks.{l}.{theirs}"
                sd[f"decoder.transformer.resblocks.{b}.{part}"] = sd[src].clone()
    if "temporal" in config.train_mode and config.train_mode.temporal == "ranking":
        sd["ranking_transform_param"] = _fill(rng, "proj", (width, 1))
    if config.adapter.type != "none":
        st = config.adapter.struct
        for k, shp in adapter_schema(arch, len(lidx), st.type, int(st.x) if "x" in st else 0, num_frames).items():
            sd["adapter." + k] = _fill(rng, k, shp)
    return sd


def random_compinv_state_dict(config, seed=0, num_frames=None):
    """Seeded fp32 `CompInvEncoder` state_dict (reference key names): `encoder.*` as in `random_state_dict`, then
    `adapter.l{i}_{k|v}.*` for the tapped layers."""
    arch = config.architecture
    layers = ARCHS[arch][3]
    rng = np.random.default_rng(seed)
    sd = OrderedDict()
    for k, shp in encoder_schema(arch).items():
        sd["encoder." + k] = _fill(rng, k, shp)
    st = config.adapter.struct
    for k, shp in adapter_schema(arch, len(resolve_layer_indices(config, layers)), st.type, int(st.x) if "x" in st else 0,
                                 num_frames).items():
        sd["adapter." + k] = _fill(rng, k, shp)
    return sd


def synthetic_clips(b, t, res, seed=1234, masked_tail=True):
    """Synthetic post-`Normalize` frames and padding mask: x ~ N(0,1) fp32;
    with `masked_tail`, clip 1 has its last ceil(T/4) frames marked as padding."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.standard_normal((b, t, 3, res, res), dtype=np.float32))
    m = torch.ones(b, t, dtype=torch.bool)
    if masked_tail and b > 1:
        m[1, t - (t + 3) // 4:] = False
    y = torch.arange(b) % 2
    return x, m, y
