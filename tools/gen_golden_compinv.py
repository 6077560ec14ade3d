#!/usr/bin/env python3
"""Writes tests/golden/compinv_{tiny,small}.npz by running the reference's own `CompInvEncoder` (imported through
`oracle.gen_golden.load_reference`, whose stubs build the CLIP tower locally) on the seeded cases of
`tests/compinv_cases.py`, in fp32 on the CPU.  Needs the reference checkout, so it runs only where that exists;
the tests read the fixtures and never run this.

Stored per case:
  recon_m{0,1}_{str,lab} / match_m{0,1}_{str,lab}   losses for mode 0 / 1, comp as strings / as the labels tensor
  recon_bf16_m{0,1} / match_bf16_m{0,1}             the same under torch.autocast("cpu", bfloat16)
  grad_m{0,1}.<param>[.norm|.head]                  adapter gradients of recon + match
  train_recon / train_match                         the losses of two CompInvTrainer-shaped steps
  after2.<param>[.norm|.head]                       adapter parameters after them (AdamW lr/25 + OneCycleLR)
  keys / shapes                                     the reference's state_dict schema

usage: python tools/gen_golden_compinv.py [case ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import load_reference  # noqa: E402
from tests.compinv_cases import CASES, LR, MAX_STEPS, build_case, save_npz, stored_slices  # noqa: E402


def run_case(name, mm, Acc, to_cn):
    out = {}
    models = {}
    for mode in (0, 1):
        c = build_case(name, mode)
        torch.manual_seed(1)
        model = mm.CompInvEncoder(to_cn(c["cfg"]), Acc(), num_frames=c["T"])
        res = model.load_state_dict(c["sd"], strict=True)
        assert not res.missing_keys and not res.unexpected_keys
        model.eval()
        models[mode] = (model, c)
        for tag, comp in (("str", c["comp"]), ("lab", c["labels"])):
            model.zero_grad()
            recon, match = model(c["x"], comp)
            (recon + match).backward()
            out[f"recon_m{mode}_{tag}"] = np.asarray(recon.item(), dtype=np.float32)
            out[f"match_m{mode}_{tag}"] = np.asarray(match.item(), dtype=np.float32)
            grads = {pn: p.grad.detach().clone() for pn, p in model.named_parameters() if p.requires_grad}
            if tag == "str":
                for pn, g in grads.items():
                    for suffix, a in stored_slices(g).items():
                        out[f"grad_m{mode}.{pn}{suffix}"] = a
            else:  # the labels tensor as comp: the same numbers (the loss is symmetric within a pair)
                assert out[f"match_m{mode}_lab"] == out[f"match_m{mode}_str"], name
        model.zero_grad()
        with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
            recon, match = model(c["x"], c["comp"])
        out[f"recon_bf16_m{mode}"] = np.asarray(recon.float().item(), dtype=np.float32)
        out[f"match_bf16_m{mode}"] = np.asarray(match.float().item(), dtype=np.float32)
    # what the reference's aliasing implies, checked on the reference itself
    for mode in (0, 1):
        assert out[f"recon_m{mode}_str"] == 0.0
    assert out["match_m0_str"] == out["match_m1_str"]
    sd = models[1][0].state_dict()
    out["keys"] = np.asarray(list(sd))
    out["shapes"] = np.asarray([",".join(map(str, t.shape)) for t in sd.values()])
    # two CompInvTrainer steps (src/trainer.py:226-303), one training set, comp = the labels tensor as its call passes
    model, c = models[1]
    opt = model.configure_optimizers(LR / 25)
    sched = torch.optim.lr_scheduler.OneCycleLR(optimizer=opt, max_lr=LR, total_steps=MAX_STEPS)
    tr, tm = [], []
    for _ in range(2):
        model.zero_grad()
        model.train()
        recon, match = model(c["x"], c["labels"])
        (recon + match).backward()
        tr.append(recon.item())
        tm.append(match.item())
        opt.step()
        sched.step()
        model.zero_grad()
    out["train_recon"], out["train_match"] = np.asarray(tr, dtype=np.float32), np.asarray(tm, dtype=np.float32)
    for pn, p in model.named_parameters():
        if p.requires_grad:
            for suffix, a in stored_slices(p).items():
                out[f"after2.{pn}{suffix}"] = a
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    save_npz(path, out)
    print(f"{name}: match {float(out['match_m1_str']):.6g} (bf16 {float(out['match_bf16_m1']):.6g}), "
          f"train {out['train_match'].tolist()} -> {path} ({os.path.getsize(path) / 1e6:.3f} MB)")


if __name__ == "__main__":
    torch.set_num_threads(8)
    mm, Acc, to_cn = load_reference()
    for c in (sys.argv[1:] or list(CASES)):
        run_case(c, mm, Acc, to_cn)
