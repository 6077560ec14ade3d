#!/usr/bin/env python3
"""Times patch-masked training (`train_mode.patch_mask`) with `Detector.mask_gather = "torch"` and `"device"`, and the gather
kernel alone; prints one JSON line and writes it to profiles/patch_mask_bench.json.

Configurations: ViT-B/16, bf16, B16 x T30, `patch_mask: {type: sample, ratio: 0.25}`, stride-2 taps (six layers) — once without
an adapter, once with `768-x-768-z0`, x = 1024 (the reference's tune-all preset).  Both arms run in ONE process on ONE model,
alternating (torch, device, torch, device, ...), with bench.py's train-leg settings: `static_graphs`, `pipeline_encoder`,
`inputs_ready` on, FusedSGD, a static batch.  A series is `--steps` train steps between two device synchronisations on the
host clock; each arm is primed with four steps, then runs `--repeats` + 1 series of which the FIRST is dropped (it still pays
for captures and allocator growth).  Reported per arm: ms per step and clips/s as median / min / max over the kept series.
`device_always_faster` is the default-on rule: every kept series of "device" beats every kept series of "torch".

The kernel alone (`dfd_kv_gather_patches`, in-place source, with the positional add): `--iters` launches between one HIP-event
pair, `--repeats` series; GB/s counts the bytes of the kept rows read plus the bytes written, against `copy`, a device copy of
the same number of bytes timed the same way in the same process.  Nothing is asserted.

usage: python tools/bench_patch_mask.py [--steps 20] [--repeats 5] [--iters 20] [--clips 16] [--frames 30]
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

ARCH, RATIO, PRIME_STEPS = "ViT-B/16", 0.25, 4


def spread(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def build(adapter, T, device):
    from dfd_clip_amd.config import ConfigNode
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    cfg = Detector.get_default_config()
    cfg.architecture, cfg.out_dim, cfg.losses = ARCH, [2], ["auc_roc"]
    cfg.decode_mode, cfg.decode_stride = "stride", 2
    cfg.train_mode.patch_mask = ConfigNode({"type": "sample", "ratio": RATIO})
    if adapter:
        cfg.adapter = ConfigNode({"type": "normal", "frozen": 0, "struct": {"type": "768-x-768-z0", "x": 1024}})
    det = Detector(cfg, T, None, precision="bf16")
    det.load_state_dict(random_state_dict(cfg, T, seed=0))
    det = det.to(device).train()
    det.static_graphs, det.pipeline_encoder, det.inputs_ready = True, True, True  # bench.py's train leg
    return det


def train_legs(adapter, B, T, steps, repeats, device):
    from dfd_clip_amd.weights import ARCHS
    det = build(adapter, T, device)
    res = ARCHS[ARCH][0]
    g = torch.Generator(device=device).manual_seed(1234)
    x = torch.randn(B, T, 3, res, res, device=device, generator=g)
    m = torch.ones(B, T, dtype=torch.bool, device=device)
    y = torch.arange(B, device=device) % 2
    opt = det.configure_optimizers(0.01 / 25)
    np.random.seed(0)

    def step():
        det.zero_grad(set_to_none=True)
        losses, _, other = det(x, [y], m, train=True, single_task=0)
        (losses[0].mean() + sum(other.values())).backward()
        opt.step()

    def series():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    arms = ("torch", "device")
    ms = {a: [] for a in arms}
    peak_gb = {}
    for a in arms:
        det.mask_gather = a
        for _ in range(PRIME_STEPS):
            step()
        assert det.last_mask_path == a
    for _ in range(repeats + 1):
        for a in arms:
            det.mask_gather = a
            torch.cuda.reset_peak_memory_stats()
            ms[a].append(series())
            peak_gb[a] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)  # (of the last series; both arms' persistent buffers included)
            print(f"  {'z0' if adapter else 'no adapter'} {a}: {ms[a][-1]:.3f} ms/step, peak {peak_gb[a]} GiB, now "
                  f"{torch.cuda.memory_allocated() / 2 ** 30:.2f} GiB", file=sys.stderr, flush=True)
    kept = {a: v[1:] for a, v in ms.items()}
    out = {"adapter": "768-x-768-z0 x=1024" if adapter else "none", "layers": len(det.layer_indices),
           "encoder_graph": bool(det._enc_graphs) and not det._enc_graphs_failed, "dropped_first_series_ms": {a: round(v[0], 3) for a, v in ms.items()}}
    for a in arms:
        out[a] = {"ms_per_step": spread(kept[a]), "clips_per_s": spread([B * 1e3 / t for t in kept[a]], 1), "series_ms": [round(t, 3) for t in kept[a]],
                  "peak_allocated_gib": peak_gb[a]}
    out["device_over_torch"] = round(statistics.median(kept["device"]) / statistics.median(kept["torch"]), 4)
    out["device_always_faster"] = max(kept["device"]) < min(kept["torch"])
    del det, opt, x, step, series
    torch.cuda.synchronize()
    gc.collect()  # (a Detector holds reference cycles: its buffers and captured graphs go only now)
    torch.cuda.empty_cache()
    return out


def kernel_leg(B, T, iters, repeats, device):
    from dfd_clip_amd import capi
    L, P, D, frames = 6, 196, 768, B * T
    S = int(P * RATIO)
    buf = torch.empty(L, frames, P + 1, 3 * D, device=device, dtype=torch.bfloat16).normal_()
    k, v = buf[:, :, 1:, D:2 * D], buf[:, :, 1:, 2 * D:]
    rng = np.random.RandomState(0)
    host = torch.as_tensor(np.stack([rng.choice(P, S, replace=False) for _ in range(L)]), dtype=torch.int32)
    index, pos = host.to(device), torch.randn(T, D, device=device)
    ko, vo = (torch.empty(L, frames * S, D, device=device, dtype=torch.bfloat16) for _ in range(2))
    moved = 2 * 2 * L * frames * S * D * 2  # K and V, read + written, bf16
    src = torch.empty(moved // 4, device=device, dtype=torch.bfloat16).normal_()
    dst = torch.empty_like(src)
    calls = {"gather": lambda: capi.kv_gather_patches(k, v, index, pos, ko, vo, T=T, index_host=host), "copy": lambda: dst.copy_(src)}
    calls["gather"]()
    assert capi.kv_gather_last_path() == capi.KVGATHER_VEC16

    def series(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    us = {n: [] for n in calls}
    for n, fn in calls.items():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for n, fn in calls.items():
            us[n].append(series(fn))
    out = {"rows_per_tensor": L * frames * S, "row_bytes": D * 2, "bytes_moved": moved}
    for n in calls:
        out[n] = {"us": spread(us[n], 2), "gbs": round(moved / statistics.median(us[n]) / 1e3, 1)}
    out["gather_over_copy"] = round(statistics.median(us["gather"]) / statistics.median(us["copy"]), 3)
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
        raise SystemExit("bench_patch_mask needs a GPU: a time taken anywhere else says nothing")
    from dfd_clip_amd import capi
    capi.load_library()
    device = torch.device("cuda", 0)
    B, T = args.clips, args.frames
    out = {"tool": "bench_patch_mask", "arch": ARCH, "dtype": "bf16", "clips": B, "frames": T, "patch_mask": {"type": "sample", "ratio": RATIO},
           "steps": args.steps, "repeats": args.repeats, "iters": args.iters}
    out["no_adapter"] = train_legs(False, B, T, args.steps, args.repeats, device)
    out["adapter_z0"] = train_legs(True, B, T, args.steps, args.repeats, device)
    out["kernel"] = kernel_leg(B, T, args.iters, args.repeats, device)
    out["default_on_rule_met"] = bool(out["no_adapter"]["device_always_faster"] and out["adapter_z0"]["device_always_faster"])
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "patch_mask_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
