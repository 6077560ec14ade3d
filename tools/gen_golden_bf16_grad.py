#!/usr/bin/env python3
"""Writes tests/golden/bf16grad_<case>.npz: step 0 of the training contract on the reference's own `Detector` (imported
through `oracle.gen_golden.load_reference`), once in fp32 and once with the forward and the loss under
`torch.autocast("cpu", dtype=torch.bfloat16)` (Accelerate's `mixed_precision: bf16`, the pin `logits_bf16` uses), same
weights, inputs, numpy seed and `comp` / `speed` extras.  What a file holds: tests/bf16_grad_cases.py.  Needs the reference
checkout, so it runs only where that exists; the tests read the fixtures and never run this.

It asserts, and tests/test_bf16_grad_cpu.py checks again from the files:
  * the fp32 gradients equal the `grad0.*` entries of the case's existing fixture exactly (no existing fixture is written)
  * at most 5 % of a case's parameters are excluded for a spread above 0.1
  * every bar that is applied, max(3 spread, 3 median spread), is at most 0.2
  * a file stays under 1 MB: else the case's sample size is halved (recorded as `sample`)

usage: python tools/gen_golden_bf16_grad.py [case ...]
"""
import contextlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden  # noqa: E402
from tests import bf16_grad_cases as bc  # noqa: E402
from tests import cases  # noqa: E402
from tests.compinv_cases import save_npz  # noqa: E402

MAX_BYTES = 1_000_000


def step0_grads(c, mm, Acc, to_cn, autocast):
    torch.manual_seed(1)
    det = mm.Detector(to_cn(c["cfg"]), c["T"], Acc())
    res = det.load_state_dict(c["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    det.train()
    comp, speed, np_seed = bc.extras(c)
    np.random.seed(np_seed)
    ctx = torch.autocast("cpu", dtype=torch.bfloat16) if autocast else contextlib.nullcontext()
    with ctx:
        tl, _, other = det(c["x"], [c["y"]], c["m"], comp, torch.tensor(speed), train=True, single_task=0)
        loss = tl[0].float().mean() + sum(v.float() for v in other.values())
    loss.backward()
    grads = {}
    for pn, p in det.named_parameters():
        assert (p.grad is None) == pn.startswith("encoder."), pn
        if p.grad is not None:
            assert p.grad.dtype == torch.float32, pn
            grads[pn] = p.grad.detach().clone()
    return grads


def check_against_existing(name, g32):
    g = cases.load_golden(name)
    seen = 0
    for pn, t in g32.items():
        if "grad0." + pn in g.files:
            assert np.array_equal(t.numpy(), g["grad0." + pn]), pn
        else:
            assert np.float32(t.norm().item()) == np.float32(g[f"grad0.{pn}.norm"]), pn
            assert np.array_equal(t.flatten()[:64].numpy(), g[f"grad0.{pn}.head"]), pn
        seen += 1
    assert seen == sum(1 for f in g.files if f.startswith("grad0.") and not f.endswith((".norm", ".head"))) + \
        sum(1 for f in g.files if f.startswith("grad0.") and f.endswith(".norm")), name


def fixture(g32, gac, sample):
    out = {"sample": np.asarray(sample, dtype=np.int64)}
    for pn, t in g32.items():
        a = bc.stored_elements(pn, t.flatten().numpy(), sample)
        b = bc.stored_elements(pn, gac[pn].flatten().numpy(), sample)
        out["g32." + pn] = a.astype(np.float32)
        out["numel." + pn] = np.asarray(t.numel(), dtype=np.int64)
        out["norm32." + pn] = np.asarray(t.double().norm().item(), dtype=np.float64)
        na = np.linalg.norm(a.astype(np.float64))
        d = np.linalg.norm(b.astype(np.float64) - a.astype(np.float64))
        out["spread." + pn] = np.asarray(d / na if na > 0 else 0.0, dtype=np.float64)
    return out


def run_case(name, mm, Acc, to_cn):
    c = bc.build_case(name)
    g32 = step0_grads(c, mm, Acc, to_cn, autocast=False)
    check_against_existing(name, g32)
    gac = step0_grads(c, mm, Acc, to_cn, autocast=True)
    assert list(gac) == list(g32)
    assert all(torch.isfinite(t).all() for t in gac.values())
    path = bc.fixture_path(name)
    sample = bc.SAMPLE
    while True:
        out = fixture(g32, gac, sample)
        bar = bc.bars(out)  # the conditions hold before a file is written
        excluded = [pn for pn, b in bar.items() if b is None]
        zero = [pn for pn, b in bar.items() if b == 0.0]
        assert len(excluded) <= bc.MAX_EXCLUDED * len(bar), (name, excluded)
        applied = [b for b in bar.values() if b]
        assert max(applied) <= bc.MAX_BAR, (name, max(applied))
        save_npz(path, out)
        if os.path.getsize(path) <= MAX_BYTES:
            break
        sample //= 2
    fx = out
    spreads = sorted(float(fx["spread." + pn]) for pn in bar if bar[pn])
    print(f"{name}: {len(bar)} parameters, sample {sample}, spread median {np.median(spreads):.3e} max {spreads[-1]:.3e}, "
          f"largest bar {max(applied):.3f}, excluded {[(pn, round(float(fx['spread.' + pn]), 2)) for pn in excluded]}, "
          f"zero gradient {zero} -> {path} ({os.path.getsize(path) / 1e6:.3f} MB)", flush=True)


if __name__ == "__main__":
    torch.set_num_threads(8)
    assert {k: v[:4] for k, v in gen_golden.CASES.items()} == cases.CASES  # one table of cases, mirrored for the tests
    mm, Acc, to_cn = gen_golden.load_reference()
    for name in (sys.argv[1:] or bc.ALL_CASES):
        run_case(name, mm, Acc, to_cn)
