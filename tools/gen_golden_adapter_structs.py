#!/usr/bin/env python3
"""Writes tests/golden/adapter_*.npz by running the reference's own `Detector` / `CompInvEncoder` (imported through
`oracle.gen_golden.load_reference`) with the CompInvAdapter structs "768-bn", "768-xxx-768" and "linear" on the seeded
cases of `tests/adapter_struct_cases.py`, in fp32 on the CPU.  Needs the reference checkout, so it runs only where that
exists; the tests read the fixtures and never run this.

Stored per Detector case (as oracle/gen_golden.py's adapter cases):
  logits / losses, logits_bf16 / losses_bf16        eval mode, fp32 and under torch.autocast("cpu", bfloat16)
  grad0.<param>[.norm|.head]                         gradients of the first training step (train mode)
  step_losses, after2.<param>[.head]                 the two SGD steps (lr 0.01) and the parameters after them
  keys / shapes                                      the reference's state_dict schema
and for "768-bn" also
  train_logits0                                      train-mode logits of step 0 (batch statistics)
  after2.<buffer>                                    running_mean / running_var / num_batches_tracked after the steps
  logits_after2                                      eval-mode logits after the steps (running statistics)
The CompInvEncoder case (train mode, two CompInvTrainer-shaped steps):
  match / match_bf16 (eval), train_match, grad.<param>[...] (step 0), after2.<param|buffer>[...], match_after2 (eval),
  keys / shapes

usage: python tools/gen_golden_adapter_structs.py [case ...]
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import load_reference  # noqa: E402
from tests.adapter_struct_cases import (CASES, COMPINV_CASES, COMPINV_LR, COMPINV_MAX_STEPS, EXTRA_INPUTS,  # noqa: E402
                                        build_case, build_compinv_case, stored)
from tests.compinv_cases import save_npz  # noqa: E402


def _schema(out, model):
    sd = model.state_dict()
    out["keys"] = np.asarray(list(sd))
    out["shapes"] = np.asarray([",".join(map(str, t.shape)) for t in sd.values()])


def _buffers(out, model, prefix):
    for bn, b in model.named_buffers():
        if "adapter" in bn:
            out[f"{prefix}.{bn}"] = b.detach().numpy().copy()


def run_case(name, mm, Acc, to_cn):
    c = build_case(name)
    x, m, y, T = c["x"], c["m"], c["y"], c["T"]
    torch.manual_seed(1)
    det = mm.Detector(to_cn(c["cfg"]), T, Acc())
    res = det.load_state_dict(c["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    _schema(out := {}, det)
    det.eval()
    with torch.no_grad():
        losses, logits = det(x, [y], m, single_task=0)
    out["logits"], out["losses"] = logits[0].numpy(), losses[0].numpy()
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        losses_a, logits_a = det(x, [y], m, single_task=0)
    out["logits_bf16"], out["losses_bf16"] = logits_a[0].float().numpy(), losses_a[0].float().numpy()
    det.train()
    opt = det.configure_optimizers(0.01)
    speed = torch.tensor(EXTRA_INPUTS["speed"][:c["B"]])
    step_losses = []
    for step in range(2):
        opt.zero_grad()
        np.random.seed(EXTRA_INPUTS["np_seed"] + step)
        tl, tz, other = det(x, [y], m, EXTRA_INPUTS["comp"][:c["B"]], speed, train=True, single_task=0)
        if step == 0:
            out["train_logits0"] = tz[0].detach().numpy().copy()
        loss = tl[0].mean() + sum(other.values())
        loss.backward()
        if step == 0:
            for pn, p in det.named_parameters():
                if p.requires_grad and p.grad is not None:
                    for suffix, a in stored(p.grad).items():
                        out[f"grad0.{pn}{suffix}"] = a
        step_losses.append(loss.item())
        opt.step()
    out["step_losses"] = np.asarray(step_losses)
    for pn, p in det.named_parameters():
        if p.requires_grad:
            t = p.detach()
            if t.numel() <= 4096:
                out["after2." + pn] = t.numpy().copy()
            else:
                out["after2." + pn + ".head"] = t.flatten()[:64].numpy().copy()
    if c["struct"] == "768-bn":
        _buffers(out, det, "after2")
        det.eval()
        with torch.no_grad():
            _, logits2 = det(x, [y], m, single_task=0)
        out["logits_after2"] = logits2[0].numpy()
    else:
        del out["train_logits0"]
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    save_npz(path, out)
    print(f"{name}: logits {out['logits'].tolist()} steps {out['step_losses'].tolist()} -> {path} "
          f"({os.path.getsize(path) / 1e6:.3f} MB)")


def run_compinv_case(name, mm, Acc, to_cn):
    c = build_compinv_case(name)
    torch.manual_seed(1)
    model = mm.CompInvEncoder(to_cn(c["cfg"]), Acc(), num_frames=c["T"])
    res = model.load_state_dict(c["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    _schema(out := {}, model)
    model.eval()
    with torch.no_grad():
        _, match = model(c["x"], c["comp"])
        out["match"] = np.asarray(match.item(), dtype=np.float32)
        with torch.autocast("cpu", dtype=torch.bfloat16):
            _, match = model(c["x"], c["comp"])
        out["match_bf16"] = np.asarray(match.float().item(), dtype=np.float32)
    # two CompInvTrainer steps (src/trainer.py:226-303) in train mode: the BatchNorm normalises with batch statistics
    opt = model.configure_optimizers(COMPINV_LR / 25)
    sched = torch.optim.lr_scheduler.OneCycleLR(optimizer=opt, max_lr=COMPINV_LR, total_steps=COMPINV_MAX_STEPS)
    tm = []
    for step in range(2):
        model.zero_grad()
        model.train()
        recon, match = model(c["x"], c["labels"])
        (recon + match).backward()
        if step == 0:
            for pn, p in model.named_parameters():
                if p.requires_grad:
                    for suffix, a in stored(p.grad).items():
                        out[f"grad.{pn}{suffix}"] = a
        tm.append(match.item())
        opt.step()
        sched.step()
    out["train_match"] = np.asarray(tm, dtype=np.float32)
    for pn, p in model.named_parameters():
        if p.requires_grad:
            for suffix, a in stored(p).items():
                out[f"after2.{pn}{suffix}"] = a
    _buffers(out, model, "after2")
    model.eval()
    with torch.no_grad():
        _, match = model(c["x"], c["comp"])
    out["match_after2"] = np.asarray(match.item(), dtype=np.float32)
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    save_npz(path, out)
    print(f"{name}: match {float(out['match']):.6g}, train {out['train_match'].tolist()}, after {float(out['match_after2']):.6g} "
          f"-> {path} ({os.path.getsize(path) / 1e6:.3f} MB)")


if __name__ == "__main__":
    torch.set_num_threads(8)
    mm, Acc, to_cn = load_reference()
    for name in (sys.argv[1:] or list(CASES) + list(COMPINV_CASES)):
        (run_compinv_case if name in COMPINV_CASES else run_case)(name, mm, Acc, to_cn)
