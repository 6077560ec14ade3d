#!/usr/bin/env python3
"""Writes tests/golden/{tiny,tiny_attnmode}_attnmap.npz and tests/golden/tiny_pmask_guide.npz by running the reference's
own `Detector` (src/models.py) on the seeded cases of tests/cases.py, in fp32 on the CPU.  Needs the reference checkout,
so it runs only where that exists; the tests read the fixtures and never run this.  Nothing of the reference is copied:
it is imported.

*_attnmap.npz — the per-key weight each decoder block applied to its values.  The reference forms it inside
  `MultiheadAttention.forward` and drops it, so a forward pre-hook on each attention module records that call's
  (q, k, v, m), and the module's own `in_proj` and its own `activations` closures are called on them again:
    q        [L, B, heads, 128]   in_proj output per head: softmax query | CoDA query
    k, v     [L, B, S, heads*64]  as the block received them (temporal positional embedding added)
    mask     [B, T]
    branches [2, L, B, heads, S]  activations[0] (softmax / attn_mode) and activations[1] (CoDA), without the 1/n_act
    aff      [L, B, heads, S]     their mean: what multiplies v
    logits   [B, out_dim]         of the same forward

tiny_pmask_guide.npz — `tiny_pmask` with `patch_mask.type: guide`: the guide (tests/attnmap_cases.py: guide_map) goes to
  the reference as the pickle it expects, in a temporary directory; NumPy is seeded as oracle/gen_golden.py seeds it
  (np_seed + step).  Stored: the training contract of oracle/gen_golden.py (logits, losses, train_task_loss, other.*,
  grad0.*, step_losses, after2.*), the guide itself (`guide_v`) and the patch indices the seeded draws selected
  (`patch_indices` [steps, layers, num_select]).

usage: python tools/gen_golden_attnmap.py [tiny tiny_attnmode tiny_pmask_guide]
"""
import os
import pickle
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import EXTRA_INPUTS, load_reference  # noqa: E402
from tests.cases import build_case  # noqa: E402
from tests.attnmap_cases import ATTNMAP_CASES, GUIDE_CASE, build_guide_case, guide_map  # noqa: E402


def reference_detector(mm, Acc, to_cn, case):
    torch.manual_seed(1)
    det = mm.Detector(to_cn(case["cfg"]), case["T"], Acc())
    res = det.load_state_dict(case["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return det


def run_attnmap(name, mm, Acc, to_cn):
    case = build_case(name)
    det = reference_detector(mm, Acc, to_cn, case).eval()
    blocks = det.decoder.transformer.resblocks
    seen = []
    hooks = [blk.attn.register_forward_pre_hook(lambda mod, args: seen.append((mod, *[a.detach().clone() for a in args])))
             for blk in blocks]
    with torch.no_grad():
        logits, _ = det.predict(case["x"], case["m"])
    for h in hooks:
        h.remove()
    assert len(seen) == len(blocks)
    out = dict(logits=logits[0].numpy(), mask=case["m"].numpy(), layer_indices=np.asarray(det.layer_indices))
    qs_, ks_, vs_, br = [], [], [], ([], [])
    with torch.no_grad():
        for mod, q, k, v, m in seen:
            heads = mod.n_head
            proj = mod.in_proj(q).unflatten(-1, (heads, -1))           # [B, 1, heads, n_act * 64]
            parts = proj.split(mod.embed_dim // heads, dim=-1)
            keymask = m.unsqueeze(1).unsqueeze(-1)
            for i, act in enumerate(mod.activations):
                w = act(parts[i], k, keymask)                          # [B, 1, S, heads]
                br[i].append(w[:, 0].permute(0, 2, 1))                 # [B, heads, S]
            qs_.append(proj[:, 0])
            ks_.append(k.flatten(-2))
            vs_.append(v.flatten(-2))
            # the weights reproduce the block's own mix
            mix = torch.einsum("bhs,bshc->bhc", (br[0][-1] + br[1][-1]) / mod.n_act, v).flatten(-2)
            assert torch.allclose(mod.out_proj(mix), mod(q, k, v, m)[:, 0], atol=1e-6)
    out["q"], out["k"], out["v"] = (torch.stack(t).numpy() for t in (qs_, ks_, vs_))
    out["branches"] = torch.stack([torch.stack(br[0]), torch.stack(br[1])]).numpy()
    out["aff"] = out["branches"].mean(axis=0)
    path = os.path.join(ROOT, "tests", "golden", name + "_attnmap.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: aff {out['aff'].shape}, min {out['aff'].min():.4f} max {out['aff'].max():.4f} -> {path} "
          f"({os.path.getsize(path) / 1e3:.1f} KB)")


def run_guide(mm, Acc, to_cn):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "guide.pkl")
        case = build_guide_case(path)
        grid = case["res"] // case["patch"]
        v = guide_map(case["layers"], grid)
        with open(path, "wb") as f:  # for the reference only: it unpickles {'v': per-layer maps}
            pickle.dump({"v": v}, f)
        det = reference_detector(mm, Acc, to_cn, case)
    x, m, y = case["x"], case["m"], case["y"]
    out = dict(guide_v=v, layer_indices=np.asarray(det.layer_indices))
    det.eval()
    with torch.no_grad():
        losses, logits = det(x, [y], m, single_task=0)
    out["logits"], out["losses"] = logits[0].numpy(), losses[0].numpy()
    # the draws the seeded steps make (the reference's call, models.py:533-539), recorded as data
    num_select = int(grid * grid * case["cfg"].train_mode.patch_mask.ratio)
    picks = []
    for step in range(2):
        np.random.seed(EXTRA_INPUTS["np_seed"] + step)
        picks.append([np.random.choice(range(grid * grid), num_select, replace=False, p=v[l].flatten()) for l in det.layer_indices])
    out["patch_indices"] = np.asarray(picks)
    det.train()
    opt = det.configure_optimizers(0.01)
    speed = torch.tensor(EXTRA_INPUTS["speed"])
    step_losses = []
    for step in range(2):
        opt.zero_grad()
        np.random.seed(EXTRA_INPUTS["np_seed"] + step)
        tl, tz, other = det(x, [y], m, EXTRA_INPUTS["comp"], speed, train=True, single_task=0)
        if step == 0:
            out["train_task_loss"] = tl[0].detach().numpy().copy()
            for k_, v_ in other.items():
                out["other." + k_] = np.asarray(v_.detach().item())
        loss = tl[0].mean() + sum(other.values())
        loss.backward()
        if step == 0:
            for pn, p in det.named_parameters():
                assert (p.grad is None) == pn.startswith("encoder."), pn
                if p.grad is not None:
                    g = p.grad.detach()
                    if g.numel() <= 4096:
                        out["grad0." + pn] = g.numpy().copy()
                    else:
                        out["grad0." + pn + ".norm"] = np.asarray(g.norm().item())
                        out["grad0." + pn + ".head"] = g.flatten()[:64].numpy().copy()
        step_losses.append(loss.item())
        opt.step()
    out["step_losses"] = np.asarray(step_losses)
    for pn, p in det.named_parameters():
        if p.requires_grad:
            t = p.detach()
            out["after2." + pn + ("" if t.numel() <= 4096 else ".head")] = (t if t.numel() <= 4096 else t.flatten()[:64]).numpy().copy()
    path = os.path.join(ROOT, "tests", "golden", GUIDE_CASE + ".npz")
    np.savez_compressed(path, **out)
    print(f"{GUIDE_CASE}: picks {out['patch_indices'].tolist()} step_losses={step_losses} -> {path} ({os.path.getsize(path) / 1e3:.1f} KB)")


if __name__ == "__main__":
    torch.set_num_threads(8)
    mm, Acc, to_cn = load_reference()
    for c in (sys.argv[1:] or list(ATTNMAP_CASES) + [GUIDE_CASE]):
        if c == GUIDE_CASE:
            run_guide(mm, Acc, to_cn)
        else:
            run_attnmap(c, mm, Acc, to_cn)
