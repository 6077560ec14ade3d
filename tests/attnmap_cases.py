"""Shared by the attention-map tests and tools/gen_golden_attnmap.py: a float64 restatement of the decoder's two attention
branches, the kernel bar, and the `patch_mask.type: guide` case.

The per-key weight of one decoder block (one query per clip, S = T*P keys, head width 64), in this project's words:
  score_s  = q_s·k / 8                      the softmax branch's score; -inf on keys of padded frames
  w_softmax = softmax over the S keys of score_s; under attn_mode the sum of softmaxes over each frame's P keys
              ("frame") and over the T keys at each patch position ("temporal"); 0 on padded keys
  w_coda   = tanh(q_c·k / 8) · 2·sigmoid(−‖q_c − k‖₁ / 8); 0 on padded keys
  aff      = ½ (w_softmax + w_coda)         what multiplies the key's value row
"""
import os

import numpy as np
import torch

from tests.cases import CASES, make_config
from dfd_clip_amd.weights import ARCHS, random_state_dict, resolve_layer_indices, synthetic_clips

HD = 64
# the bar the forward meets on `mix` for the same sums (tests/test_hip_decoder.py::test_decoder_attention)
KERNEL_ATOL, KERNEL_RTOL = 2e-5, 1e-4
ATTNMAP_CASES = ("tiny", "tiny_attnmode")
GUIDE_CASE = "tiny_pmask_guide"
GUIDE_SEED = 5


def attention_branches(q, k, mask, T, attn_modes=()):
    """q [B, H, 128] (softmax query | CoDA query per head), k [B, S, H*64] (positional embedding already added),
    mask [B, T] bool -> float64 (w_softmax, w_coda), each [B, H, S]."""
    B, H, _ = q.shape
    S = k.shape[1]
    P = S // T
    assert S == T * P and k.shape[2] == H * HD
    q = q.double()
    kh = k.double().view(B, S, H, HD).permute(0, 2, 1, 3)           # [B, H, S, 64]
    qs, qc = q[..., :HD], q[..., HD:]
    valid = mask.bool().repeat_interleave(P, dim=1)[:, None, :]     # [B, 1, S]
    score = torch.einsum("bhsc,bhc->bhs", kh, qs) / 8.0
    score = score.masked_fill(~valid, float("-inf"))
    if not attn_modes:
        ws = score.softmax(dim=-1)
    else:
        grid = score.view(B, H, T, P)
        ws = torch.zeros_like(grid)
        if "frame" in attn_modes:
            ws = ws + grid.softmax(dim=-1)
        if "temporal" in attn_modes:
            ws = ws + grid.softmax(dim=-2)
        ws = ws.reshape(B, H, S)
    ws = torch.where(valid, ws, torch.zeros_like(ws))               # a padded key weighs nothing (also where its group is all -inf)
    gate = 2.0 * torch.sigmoid(-(qc[:, :, None, :] - kh).abs().sum(-1) / 8.0)
    wc = torch.tanh(torch.einsum("bhsc,bhc->bhs", kh, qc) / 8.0) * gate
    wc = torch.where(valid, wc, torch.zeros_like(wc))
    return ws, wc


def attention_map(q, k, mask, T, attn_modes=()):
    ws, wc = attention_branches(q, k, mask, T, attn_modes)
    return 0.5 * (ws + wc)


def worst(got, want, atol=KERNEL_ATOL, rtol=KERNEL_RTOL):
    """-> (largest |got - want|, largest excess over atol + rtol·|want|) in float64"""
    got, want = got.double().cpu(), want.double().cpu()
    err = (got - want).abs()
    return err.max().item(), (err - (atol + rtol * want.abs())).max().item()


def load_attnmap_golden(name):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + "_attnmap.npz")
    return np.load(path, allow_pickle=False)


# ---- patch_mask.type: guide ---------------------------------------------------------------------------------------------

def guide_map(layers, grid, seed=GUIDE_SEED):
    """A seeded, clearly non-uniform map [layers, grid, grid], each layer summing to 1 (float64)."""
    rng = np.random.RandomState(seed)
    v = rng.uniform(0.05, 1.0, size=(layers, grid, grid)) ** 2
    return v / v.reshape(layers, -1).sum(1)[:, None, None]


def build_guide_case(path):
    """tests/cases.py's `tiny_pmask` with `type: guide` and the map file at `path` (the caller writes it: an .npz here, a
    pickle for the reference)."""
    arch, B, T, over = CASES["tiny_pmask"]
    over = dict(over, train_mode__patch_mask={"type": "guide", "ratio": 0.5, "path": str(path)})
    res, patch, width, layers, heads, _ = ARCHS[arch]
    cfg = make_config(arch, **over)
    sd = random_state_dict(cfg, T, seed=0)
    x, m, y = synthetic_clips(B, T, res, seed=1234, masked_tail=True)
    return dict(name=GUIDE_CASE, arch=arch, B=B, T=T, cfg=cfg, sd=sd, x=x, m=m, y=y, res=res, patch=patch, width=width,
                layers=layers, heads=heads, layer_indices=resolve_layer_indices(cfg, layers), over=over)
