#!/usr/bin/env python3
"""Adapter pre-training step (`CompInvEncoder` + `harness.compinv_train_step`) at the shipped configuration
(configs/comp-inv-encoder/deepfake.yaml of the reference): ViT-B/16, 5 (raw, c23) pairs = 10 clips x 50 frames,
`768-x-768` adapter with x = 256 on every other layer (6 tapped), bf16, AdamW + OneCycleLR.

Prints one JSON line: pairs/s and ms per optimizer step (HIP events around `--steps` steps after `--warmup`), and the
in-situ time and achieved bandwidth of the two pair-loss kernels on the step's own adapted K/V (events around
`--kernel-iters` back-to-back launches), against the 6.29 TB/s copy ceiling DESIGN.md uses.

usage: python tools/bench_compinv.py [--steps 10] [--warmup 3] [--pairs 5] [--frames 50] [--x 256] [--graphs]
"""
import argparse
import json
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dfd_clip_amd import capi, default_compinv_config  # noqa: E402
from dfd_clip_amd.compinv import CompInvEncoder  # noqa: E402
from dfd_clip_amd.harness import compinv_train_step, make_one_cycle  # noqa: E402

COPY_CEILING_GBS = 6290.0


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--x", type=int, default=256)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--graphs", action="store_true", help="replay the adapter's kernels as HIP graphs")
    a = ap.parse_args()
    logging.getLogger().setLevel(logging.ERROR)  # the random-initialisation notice of the encoder

    cfg = default_compinv_config()
    cfg.mode = 1
    cfg.adapter.struct = {"type": "768-x-768", "x": a.x}
    dev = "cuda:0"
    torch.manual_seed(0)
    model = CompInvEncoder(cfg, None, num_frames=a.frames, precision="bf16").to(dev)
    model.use_graphs = a.graphs
    B, T = 2 * a.pairs, a.frames
    x = torch.randn(B, T, 3, 224, 224, device=dev)
    comp = ["raw", "c23"] * a.pairs
    opt = model.configure_optimizers(a.lr / 25)
    sched = make_one_cycle(opt, a.lr, a.warmup + a.steps + 1, num_processes=1)
    step = lambda: compinv_train_step(model, opt, [(x, comp)], sched)  # noqa: E731
    for _ in range(a.warmup):
        out = step()
    ms = timed(step, a.steps)
    match = out["match"][0].item()

    # the loss kernels in situ: on this step's adapted K/V, with its workspace
    with torch.no_grad():
        k, v = model._adapted(x)
    P, D, L = model.adapter.patches, k.shape[-1], k.shape[0]
    f32 = dict(device=dev, dtype=torch.float32)
    ws = torch.empty(-(-capi.compinv_loss_workspace_bytes(P, D) // 4), **f32)
    m_, n_, r_ = torch.empty((), **f32), torch.empty((), **f32), torch.empty((), **f32)
    g = torch.ones(1, **f32)
    dk, dv = torch.empty_like(k), torch.empty_like(v)
    fwd_ms = timed(lambda: capi.compinv_loss_fwd(k, v, B, T, P, ws, m_, n_, r_), a.kernel_iters)
    bwd_ms = timed(lambda: capi.compinv_loss_bwd(k, v, B, T, P, ws, n_, g, dk, dv), a.kernel_iters)
    used = 2 * (B // 2)
    fwd_bytes = 2 * L * used * T * P * D * k.element_size()  # k and v of every paired clip, read once
    bwd_bytes = 2 * fwd_bytes + 2 * L * (B - used) * T * P * D * k.element_size()  # read + write (+ the odd clip's zeros)
    fwd_gbs, bwd_gbs = fwd_bytes / fwd_ms / 1e6, bwd_bytes / bwd_ms / 1e6
    print(json.dumps({
        "workload": "compinv_train_step", "arch": "ViT-B/16", "pairs": a.pairs, "frames": T, "adapter_x": a.x, "layers": L,
        "precision": "bf16", "graphs": a.graphs, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(ms, 3), "pairs_per_s": round(a.pairs / ms * 1e3, 2), "match": match,
        "loss_fwd_us": round(fwd_ms * 1e3, 1), "loss_fwd_GBps": round(fwd_gbs, 1),
        "loss_fwd_pct_copy_ceiling": round(100 * fwd_gbs / COPY_CEILING_GBS, 1),
        "loss_bwd_us": round(bwd_ms * 1e3, 1), "loss_bwd_GBps": round(bwd_gbs, 1),
        "loss_bwd_pct_copy_ceiling": round(100 * bwd_gbs / COPY_CEILING_GBS, 1),
        "loss_fwd_bytes": fwd_bytes, "loss_bwd_bytes": bwd_bytes,
    }))


if __name__ == "__main__":
    main()
