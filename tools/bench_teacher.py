#!/usr/bin/env python3
"""Times teacher-mode training (`harness.train_step` with a teaching `EmaTeacher`) on its two paths, and the teacher's update
alone; prints one JSON line and writes it to profiles/teacher_bench.json.

Arms: "private" = EmaTeacher(model) — a deep copy of the whole model, a second encoder pass per batch for the soft labels,
the update as the torch loop over every parameter (the path before `share_encoder` / `fused` existed); "shared" =
EmaTeacher(model, share_encoder=True, fused=True) — one tower, one encoder pass per batch read by both, one `dfd_ema_step`
launch.  Configurations: ViT-B/16, bf16, B16 x T30, two tasks (the batch is labelled for task 0, task 1 learns from the teacher),
stride-2 taps (six layers) — once without an adapter, once with `768-x-768-z0`, x = 1024 and `patch_mask: {type: sample,
ratio: 0.25}`.  Each arm has a model, optimizer and teacher of its own from the same weights; both live in ONE process and
alternate (private, shared, private, ...), with bench.py's train-leg settings: `static_graphs`, `pipeline_encoder`,
`inputs_ready` on, FusedSGD, a static batch.  A series is `--steps` train steps between two device synchronisations on the
host clock; each arm is primed with four steps, then runs `--repeats` + 1 series of which the FIRST is dropped.  Reported per
arm: ms per step and clips/s as median / min / max over the kept series, and the peak of allocated memory above what was
allocated before the arm was built (model, teacher, optimizer, K/V sets, activations).

`update` alone, on the no-adapter pair: the torch loop over every parameter ("torch_all", the private arm's), the torch loop
over the pairs the kernel covers ("torch_same_pairs") and `dfd_ema_step` ("ema_step"), `--iters` updates between two device
synchronisations on the host clock (the loops are bound by the host).  GB/s of the kernel counts 2 reads + 1 write per element
+ the mirror write of the decoder's Linear weights, against `copy`, a device copy moving the same number of bytes.
Nothing is asserted.

usage: python tools/bench_teacher.py [--steps 20] [--repeats 5] [--iters 20] [--clips 16] [--frames 30]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ARCH, RATIO, PRIME_STEPS, EMA_RATIO = "ViT-B/16", 0.25, 4, 0.999
ARMS = {"private": dict(share_encoder=False, fused=False), "shared": dict(share_encoder=True, fused=True)}


def spread(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def build(adapter, T, device):
    from dfd_clip_amd.config import ConfigNode
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    cfg = Detector.get_default_config()
    cfg.architecture, cfg.out_dim, cfg.losses = ARCH, [2, 2], ["auc_roc", "auc_roc"]
    cfg.decode_mode, cfg.decode_stride = "stride", 2
    if adapter:
        cfg.train_mode.patch_mask = ConfigNode({"type": "sample", "ratio": RATIO})
        cfg.adapter = ConfigNode({"type": "normal", "frozen": 0, "struct": {"type": "768-x-768-z0", "x": 1024}})
    det = Detector(cfg, T, None, precision="bf16")
    det.load_state_dict(random_state_dict(cfg, T, seed=0))
    det = det.to(device).train()
    det.static_graphs, det.pipeline_encoder, det.inputs_ready = True, True, True  # bench.py's train leg
    return det


def make_arm(name, adapter, T, device):
    from dfd_clip_amd.harness import EmaTeacher
    det = build(adapter, T, device)
    teacher = EmaTeacher(det, EMA_RATIO, teach_at=0, **ARMS[name])
    return det, det.configure_optimizers(0.01 / 25), teacher


def train_legs(adapter, B, T, steps, repeats, device):
    from dfd_clip_amd.harness import train_step
    from dfd_clip_amd.weights import ARCHS
    res = ARCHS[ARCH][0]
    g = torch.Generator(device=device).manual_seed(1234)
    x = torch.randn(B, T, 3, res, res, device=device, generator=g)
    m = torch.ones(B, T, dtype=torch.bool, device=device)
    y = torch.arange(B, device=device) % 2
    batch = [(x, y, m, None, None, 0)]
    np.random.seed(0)
    arms, peak_gib = {}, {}
    for name in ARMS:
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        arms[name] = make_arm(name, adapter, T, device)
        for _ in range(PRIME_STEPS):
            train_step(*arms[name][:2], batch, teacher=arms[name][2])
        torch.cuda.synchronize()
        assert arms[name][2].teaching
        peak_gib[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 30, 3)

    def series(name):
        det, opt, teacher = arms[name]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            train_step(det, opt, batch, teacher=teacher)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    ms = {a: [] for a in ARMS}
    for _ in range(repeats + 1):
        for a in ARMS:
            ms[a].append(series(a))
            print(f"  {'z0 + patch mask' if adapter else 'no adapter'} {a}: {ms[a][-1]:.3f} ms/step", file=sys.stderr, flush=True)
    kept = {a: v[1:] for a, v in ms.items()}
    out = {"adapter": "768-x-768-z0 x=1024, patch_mask sample 0.25" if adapter else "none", "layers": len(arms["shared"][0].layer_indices),
           "dropped_first_series_ms": {a: round(v[0], 3) for a, v in ms.items()}}
    for a in ARMS:
        out[a] = {"ms_per_step": spread(kept[a]), "clips_per_s": spread([B * 1e3 / t for t in kept[a]], 1), "series_ms": [round(t, 3) for t in kept[a]],
                  "peak_allocated_gib_above_base": peak_gib[a]}
    out["shared_over_private"] = round(statistics.median(kept["shared"]) / statistics.median(kept["private"]), 4)
    out["shared_always_faster"] = max(kept["shared"]) < min(kept["private"])
    return out, arms


def update_leg(arms, iters, repeats, device):
    """`update` alone on the two arms' (model, teacher) pairs."""
    private, shared = arms["private"][2], arms["shared"][2]
    model_p, model_s = arms["private"][0], arms["shared"][0]
    plan = shared._plan
    covered = [(e[0], e[1]) for e in plan["entries"]]
    moved = sum(p.numel() * 4 * (3 + (m is not None)) for p, _, m in plan["entries"])
    src = torch.empty(moved // 8, device=device, dtype=torch.float32).normal_()
    dst = torch.empty_like(src)
    r = EMA_RATIO

    @torch.no_grad()
    def torch_same_pairs():
        for p1, p2 in covered:
            p1.data.copy_((1 - r) * p1.data + r * p2.data)  # (in place: the pairs stay the kernel's)

    calls = {"torch_all": lambda: private.update(model_p), "torch_same_pairs": torch_same_pairs, "ema_step": lambda: shared.update(model_s),
             "copy": lambda: dst.copy_(src)}

    def series(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / iters * 1e6

    us = {n: [] for n in calls}
    for fn in calls.values():
        for _ in range(3):
            fn()
    for _ in range(repeats):
        for n, fn in calls.items():
            us[n].append(series(fn))
    out = {"pairs_all": len(list(private.module.parameters())), "pairs_kernel": len(covered), "pairs_torch_rest": len(plan["rest"]),
           "mirrored": len(plan["written"]), "elements_all": sum(p.numel() for p in private.module.parameters()),
           "elements_kernel": sum(p.numel() for p, _ in covered), "bytes_moved_kernel": moved}
    for n in calls:
        out[n] = {"us": spread(us[n], 2)}
    for n in ("ema_step", "copy", "torch_same_pairs"):
        out[n]["gbs"] = round(moved / statistics.median(us[n]) / 1e3, 1)
    out["ema_step_over_copy"] = round(statistics.median(us["ema_step"]) / statistics.median(us["copy"]), 3)
    out["torch_all_over_ema_step"] = round(statistics.median(us["torch_all"]) / statistics.median(us["ema_step"]), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=30)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_teacher needs a GPU: a time taken anywhere else says nothing")
    from dfd_clip_amd import capi
    capi.load_library()
    device = torch.device("cuda", 0)
    B, T = args.clips, args.frames
    out = {"tool": "bench_teacher", "arch": ARCH, "dtype": "bf16", "clips": B, "frames": T, "tasks": 2, "ema_ratio": EMA_RATIO,
           "steps": args.steps, "repeats": args.repeats, "iters": args.iters}
    out["no_adapter"], arms = train_legs(False, B, T, args.steps, args.repeats, device)
    out["update"] = update_leg(arms, args.iters, args.repeats, device)
    del arms
    torch.cuda.synchronize()
    gc.collect()  # (a Detector holds reference cycles: its buffers and captured graphs go only now)
    torch.cuda.empty_cache()
    out["adapter_z0_patch_mask"], arms = train_legs(True, B, T, args.steps, args.repeats, device)
    del arms
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "teacher_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
