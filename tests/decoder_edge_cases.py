"""Shared by tests/test_decoder_edges_cpu.py and tests/test_hip_decoder_edges.py: a float64 restatement of the decoder's
single-query two-branch attention with its autograd gradients, and the case tables (shapes, padding patterns, split
counts) that take the five decoder-attention entry points off the one corner the older kernel tests sit on.  No GPU
code is imported here.

One decoder block, in this project's words (tests/attnmap_cases.py has the per-key weights):
  mix_softmax = Σ_s w_softmax[s] · v[s]
  mix         = Σ_s ½ (w_softmax[s] + w_coda[s]) · v[s]
  stats       = (max_s score_s[s], Σ_s exp(score_s[s] − max)) per (clip, head), over the keys of valid frames
k and v are `stored + pos[frame]`, so d/dpos[t] = Σ_{clip, patch} (dk + dv) of frame t.
"""
import torch

from tests.attnmap_cases import HD, attention_branches

# (B, T, P, heads): S = 1; odd S = 15 (no multiple of the rows per trip); heads = 3 and 5 (rows per block rounded up);
# P = 49 and P = 576 (the two untested patch counts); heads = 12 and 16 (768 and 1024 channels: the combine kernel's
# largest blocks); T = 1, 3, 5, 6, 7
SHAPES = [(2, 1, 1, 1), (3, 3, 5, 4), (2, 5, 7, 3), (3, 3, 49, 2), (2, 6, 64, 5), (4, 7, 20, 12), (2, 3, 576, 16)]
MASKS = ("full", "tail", "head", "hole", "only_first", "only_last", "alternate")
# the project's bars (tests/test_hip_kernels.py::test_decoder_attention, tests/test_hip_backward.py): (atol, rtol)
BARS = {"mix": (2e-5, 1e-4), "mix_softmax": (2e-5, 1e-4), "max": (1e-5, 1e-5), "sumexp": (1e-4, 1e-4),
        "dq": (2e-5, 2e-4), "dk": (2e-6, 2e-4), "dv": (2e-6, 2e-4), "dpos": (5e-5, 2e-4)}
# test_hip_backward.py::test_decoder_attention_modes: atol times max(1, |reference|max of mix for the forward, of dq for the gradients)
MODES_BARS = {"mix": (2e-5, 1e-4), "dq": (5e-5, 2e-4), "dk": (5e-6, 2e-4), "dv": (5e-6, 2e-4), "dpos": (1e-4, 2e-4)}


def frame_mask(name, T):
    """One clip's valid frames [T] bool under the pattern `name`; a pattern that T has no room for is `full`."""
    m = torch.ones(T, dtype=torch.bool)
    n = max(1, T // 4)
    if name == "full" or T < 2 or (name == "hole" and T < 3):
        return m
    if name == "tail":
        m[T - n:] = False
    elif name == "head":
        m[:n] = False
    elif name == "hole":
        m[1:1 + max(1, (T - 2) // 2)] = False
    elif name == "only_first":
        m[1:] = False
    elif name == "only_last":
        m[:T - 1] = False
    elif name == "alternate":
        m[1::2] = False
    else:
        raise KeyError(name)
    return m


def deals(B, T):
    """The MASKS dealt to batches of B clips, starting at clip 0: deal i gives clip b the pattern MASKS[i*B + b] (wrapping),
    so one batch holds different patterns and the deals together hold them all.  -> [(names, mask [B, T] bool)]"""
    if T < 2:
        return [(("full",) * B, torch.ones(B, T, dtype=torch.bool))]
    out = []
    for i in range((len(MASKS) + B - 1) // B):
        names = tuple(MASKS[(i * B + b) % len(MASKS)] for b in range(B))
        out.append((names, torch.stack([frame_mask(n, T) for n in names])))
    return out


def policy_splits(B, S):
    """Decoder._splits, restated (the CPU test holds the two together)"""
    return max(1, min(S // 64, max(1, 768 // max(B, 1))))


def splits_for(B, S):
    """SPLITS(S): 1, 2, 3, 7, the production policy's count, 65 and 130 (the combine kernel's 64-strided loops on a second
    and third trip), and S, S + 1, 2S + 3 (one-key splits and empty ones), duplicates removed, order kept."""
    out = []
    for s in (1, 2, 3, 7, policy_splits(B, S), 65, 130, S, S + 1, 2 * S + 3):
        if s not in out:
            out.append(s)
    return out


def combine_fits(heads, splits):
    """dfd_decoder_attn_fwd's ceiling: the merge keeps heads x splits floats in LDS beside two static rows of 16, 160 KiB in
    all; of the tables only (2, 3, 576, 16) with 2S + 3 = 3459 splits is past it, and must be refused by name"""
    return splits <= 4096 and heads * splits * 4 + 128 <= 160 * 1024


def empty_splits(S, splits):
    """how many of `splits` workgroups get no key: split * per >= S with per = ceil(S / splits)"""
    per = (S + splits - 1) // splits
    return sum(1 for s in range(splits) if s * per >= S)


def rows_per_block(heads):
    """csrc/decoder_common.hpp decoder_attn_block: key rows side by side in a workgroup of heads*8*R threads, whole waves"""
    tpr = heads * 8
    R = (256 + tpr - 1) // tpr
    while (tpr * R) % 64 != 0:
        R += 1
    return R


def rnd(*shape, seed=0, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def operands(B, T, P, heads, dtype, seed=0):
    """Seeded q [B, heads, 128], k, v [B, S, D] rounded to `dtype`, dmix [B, D] (all on the CPU)"""
    S, D = T * P, heads * HD
    return dict(q=rnd(B, heads, 2 * HD, seed=seed + 3), k=rnd(B, S, D, seed=seed + 1).to(dtype), v=rnd(B, S, D, seed=seed + 2).to(dtype),
                dmix=rnd(B, D, seed=seed + 4))


def restate(q, k, v, mask, T, attn_mode=()):
    """q [B, H, 128], k, v [B, S, H*64] (positional embedding already added), mask [B, T] bool -> dict of float64
    mix, mix_softmax [B, H*64], max, sumexp [B, H], ws, wc [B, H, S].  Differentiable in q, k, v."""
    B, H, _ = q.shape
    S = k.shape[1]
    P = S // T
    ws, wc = attention_branches(q, k, mask, T, attn_mode)
    vh = v.double().view(B, S, H, HD)
    mix_softmax = torch.einsum("bhs,bshc->bhc", ws, vh).reshape(B, H * HD)
    mix = torch.einsum("bhs,bshc->bhc", 0.5 * (ws + wc), vh).reshape(B, H * HD)
    with torch.no_grad():
        valid = mask.bool().repeat_interleave(P, dim=1)[:, None, :]
        kh = k.double().view(B, S, H, HD)
        score = (torch.einsum("bshc,bhc->bhs", kh, q.double()[..., :HD]) / 8.0).masked_fill(~valid, float("-inf"))
        mx = score.max(-1).values
        sumexp = torch.where(valid, (score - mx[..., None]).exp(), torch.zeros_like(score)).sum(-1)
    return dict(mix=mix, mix_softmax=mix_softmax, max=mx, sumexp=sumexp, ws=ws, wc=wc)


def reference(o, mask, T, attn_mode=(), dtype=torch.float64):
    """The restatement and its autograd gradients for operands `o` (k, v as rounded) evaluated in `dtype` (float64; the
    float32 evaluation measures what a bar asks of an f32 kernel): every entry of restate() plus dq [B, 2D],
    dk, dv [B, S, D] and dpos [T, D] of Σ mix·dmix, detached."""
    B, S, D = o["k"].shape
    P = S // T
    q = o["q"].detach().to(dtype).clone().requires_grad_(True)
    pos = torch.zeros(T, D, dtype=dtype, requires_grad=True)
    per_key = lambda x: (x.to(dtype).view(B, T, P, D) + pos[None, :, None, :]).view(B, S, D)
    k, v = per_key(o["k"]), per_key(o["v"])
    k.retain_grad(), v.retain_grad()
    if dtype == torch.float64:
        r = restate(q, k, v, mask, T, attn_mode)
    else:  # restate() widens to float64; the float32 evaluation runs the same formulas on float32 tensors
        r = _restate_in(dtype, q, k, v, mask, T, attn_mode)
    (r["mix"] * o["dmix"].to(dtype)).sum().backward()
    out = {n: t.detach() for n, t in r.items()}
    out.update(dq=q.grad.reshape(B, -1), dk=k.grad, dv=v.grad, dpos=pos.grad)
    return out


def _restate_in(dtype, q, k, v, mask, T, attn_mode):
    B, H, _ = q.shape
    S = k.shape[1]
    P = S // T
    kh, vh = k.view(B, S, H, HD), v.view(B, S, H, HD)
    qs, qc = q[..., :HD], q[..., HD:]
    valid = mask.bool().repeat_interleave(P, dim=1)[:, None, :]
    score = (torch.einsum("bshc,bhc->bhs", kh, qs) / 8.0).masked_fill(~valid, float("-inf"))
    if not attn_mode:
        ws = score.softmax(-1)
    else:
        grid = score.view(B, H, T, P)
        ws = torch.zeros_like(grid)
        if "frame" in attn_mode:
            ws = ws + grid.softmax(-1)
        if "temporal" in attn_mode:
            ws = ws + grid.softmax(-2)
        ws = ws.reshape(B, H, S)
    ws = torch.where(valid, ws, torch.zeros_like(ws))
    gate = 2.0 * torch.sigmoid(-(qc[:, None] - kh).abs().sum(-1).transpose(1, 2) / 8.0)
    wc = torch.where(valid, torch.tanh(torch.einsum("bshc,bhc->bhs", kh, qc) / 8.0) * gate, torch.zeros_like(ws))
    mx = score.detach().max(-1).values
    sumexp = torch.where(valid, (score.detach() - mx[..., None]).exp(), torch.zeros_like(ws)).sum(-1)
    return dict(mix=torch.einsum("bhs,bshc->bhc", 0.5 * (ws + wc), vh).reshape(B, H * HD),
                mix_softmax=torch.einsum("bhs,bshc->bhc", ws, vh).reshape(B, H * HD), max=mx, sumexp=sumexp, ws=ws, wc=wc)


def worst(got, want, atol, rtol):
    """-> (largest |got - want|, largest excess over atol + rtol·|want|) in float64; a non-finite `got` is an infinite error"""
    got, want = got.detach().double().cpu().reshape(want.shape), want.double()
    err = (got - want).abs()
    err = torch.where(torch.isfinite(got), err, torch.full_like(err, float("inf")))
    return err.max().item(), (err - (atol + rtol * want.abs())).max().item()
