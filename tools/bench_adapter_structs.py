#!/usr/bin/env python3
"""Train step of a `Detector` with each CompInvAdapter struct at the flagship shape (ViT-B/16, B16 x T30, bf16, every
other layer tapped = 6 layers x (k, v) = 12 adapter tensors, dropout 0.5, SGD), and the new kernels at that step's shapes.

Prints one JSON line per struct: clips/s and ms per step (HIP events around `--steps` steps after `--warmup`); for the
new structs also the time and achieved bandwidth of each new kernel on one (layer, tensor) of the step (events around
`--kernel-iters` back-to-back launches on tensors of the step's shapes), against the 6.29 TB/s copy ceiling DESIGN.md
uses.  "768-x-768-nln" (x = 256), measured in the same run, is the point of comparison.

With `--kernel` the train steps are left out and one JSON line per named kernel group holds the per-kernel figures alone:
"norm_gelu" (dfd_adapter_norm_gelu and its backward: modes 0, 1, 2 in bf16, mode 2 with an f32 `a`, mode 0 at x = 1024) or a
struct name for that struct's kernels as above.

usage: python tools/bench_adapter_structs.py [--steps 5] [--warmup 2] [--clips 16] [--frames 30] [--x 256] [--graphs]
                                             [--structs 768-x-768-nln,768-bn,768-xxx-768,linear]
                                             [--kernel norm_gelu,768-bn,768-xxx-768,linear] [--patches 196] [--kernel-iters 20]
"""
import argparse
import json
import logging
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dfd_clip_amd import capi  # noqa: E402
from dfd_clip_amd.detector import Detector  # noqa: E402
from tests.cases import make_config  # noqa: E402

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


def kernel_figures(struct, rows, P, T, x, iters, dev):
    """{kernel: (us, GB/s)} of the struct's new kernels on one (layer, tensor) of the step's shapes."""
    bf, f32 = dict(device=dev, dtype=torch.bfloat16), dict(device=dev, dtype=torch.float32)
    rng = torch.tensor([1, 2], device=dev, dtype=torch.int64)
    drop = capi.Dropout(rng, 1001, 0.5)
    frames = rows // P
    out = {}

    def rec(name, fn, nbytes):
        fn()  # the first launch of a kernel is not a steady-state one
        ms = timed(fn, iters)
        out[name + "_us"] = round(ms * 1e3, 1)
        out[name + "_GBps"] = round(nbytes / ms / 1e6, 1)
        out[name + "_pct_copy_ceiling"] = round(100 * nbytes / ms / 1e6 / COPY_CEILING_GBS, 1)

    if struct == "norm_gelu":
        for name, mode, a_kw, xw in (("mode0", 0, bf, x), ("mode1", 1, bf, x), ("mode2", 2, bf, x), ("mode2_f32a", 2, f32, x),
                                     ("mode0_x1024", 0, bf, 1024)):
            shape = (P, xw) if mode == 1 else (xw,)
            a, dy = torch.randn(frames, P, xw, **a_kw), torch.randn(frames, P, xw, **bf)
            y, da = torch.empty_like(dy), torch.empty_like(dy)
            w, b = torch.ones(*shape, **f32), torch.zeros(*shape, **f32)
            dw, db = torch.empty_like(w), torch.empty_like(b)
            ws = torch.empty(capi.adapter_norm_gelu_bwd_workspace_bytes(frames, P, xw, mode) // 4 + 4, **f32)
            na, n = a.numel() * a.element_size(), dy.numel() * 2
            rec(f"norm_gelu_fwd_{name}", lambda: capi.adapter_norm_gelu(a, y, w, b, frames, P, xw, mode), na + n)
            # the group pass reads a and dy and writes da; the affine pass reads a and dy again
            rec(f"norm_gelu_bwd_{name}", lambda: capi.adapter_norm_gelu_bwd(a, dy, da, w, b, dw, db, ws, frames, P, xw, mode),
                2 * na + 3 * n)
    elif struct == "768-bn":
        D = 768
        y, res, dout = (torch.randn(rows, D, **bf) for _ in range(3))
        stats, ws = torch.empty(2, T, **f32), torch.empty(capi.adapter_bn_workspace_bytes(frames, P, D) // 4 + 4, **f32)
        g, b, pos = torch.ones(T, **f32), torch.zeros(T, **f32), torch.zeros(T, D, **f32)
        dg, db, dy = torch.empty(T, **f32), torch.empty(T, **f32), torch.empty_like(y)
        n = rows * D * 2
        rec("bn_stats", lambda: capi.adapter_bn_stats(y, stats, ws, frames, P, T, capi.BN_TRAIN), n)
        rec("bn_apply", lambda: capi.adapter_bn_apply(y, res, frames, P, T, stats, g, b, residual=res, pos=pos, drop=drop), 3 * n)
        rec("bn_bwd", lambda: capi.adapter_bn_bwd(y, dout, dy, stats, g, dg, db, ws, frames, P, T, True, drop=drop), 5 * n)
    elif struct == "768-xxx-768":
        a, dh, h = (torch.randn(rows, x, **bf) for _ in range(3))
        n = rows * x * 2
        rec("gelu_erf", lambda: capi.gelu_erf(a, h, drop), 2 * n)
        rec("gelu_erf_bwd", lambda: capi.gelu_erf_bwd(a, dh, h, drop), 3 * n)
    elif struct == "linear":
        D = 768
        o, kv, pos = torch.randn(rows, D, **f32), torch.empty(rows, D, **bf), torch.zeros(T, D, **f32)
        rec("linear_drop_pos", lambda: capi.adapter_bn_apply(o, kv, frames, P, T, pos=pos, drop=drop), rows * D * 6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--x", type=int, default=256)
    ap.add_argument("--kernel-iters", type=int, default=20)
    ap.add_argument("--graphs", action="store_true", help="Detector.static_graphs (HIP-graph replay of decoder + adapter)")
    ap.add_argument("--structs", default="768-x-768-nln,768-bn,768-xxx-768,linear")
    ap.add_argument("--kernel", default="", help="per-kernel figures only: norm_gelu and / or struct names, comma-separated")
    ap.add_argument("--patches", type=int, default=196, help="patches per frame of the --kernel tensors")
    a = ap.parse_args()
    logging.getLogger().setLevel(logging.ERROR)
    dev = "cuda:0"
    B, T = a.clips, a.frames
    for group in filter(None, a.kernel.split(",")):
        line = {"workload": "adapter_kernels", "kernel": group, "frames": B * T, "patches": a.patches, "x": a.x, "iters": a.kernel_iters}
        line.update(kernel_figures(group, B * T * a.patches, a.patches, T, a.x, a.kernel_iters, dev))
        print(json.dumps(line), flush=True)
    if a.kernel:
        return
    for struct in a.structs.split(","):
        cfg = make_config("ViT-B/16", decode_mode="stride", decode_stride=2, adapter__type="normal", adapter__frozen=0,
                          adapter__struct={"type": struct, "x": a.x})
        cfg.dropout = 0.5
        torch.manual_seed(0)
        det = Detector(cfg, T, None, precision="bf16").to(dev).train()
        det.static_graphs = a.graphs
        opt = det.configure_optimizers(0.01)
        x = torch.randn(B, T, 3, 224, 224, device=dev)
        m = torch.ones(B, T, dtype=torch.bool, device=dev)
        y = torch.arange(B, device=dev) % 2

        def step():
            opt.zero_grad(set_to_none=True)
            losses, _, other = det(x, [y], m, train=True, single_task=0)
            (losses[0].mean() + sum(other.values())).backward()
            opt.step()

        for _ in range(a.warmup):
            step()
        ms = timed(step, a.steps)
        P = det.adapter.patches
        line = {"workload": "detector_train_step", "arch": "ViT-B/16", "struct": struct, "clips": B, "frames": T,
                "adapter_x": a.x if struct not in ("768-bn", "linear") else None, "adapter_tensors": 2 * len(det.layer_indices),
                "precision": "bf16", "graphs": a.graphs, "steps": a.steps, "warmup": a.warmup,
                "ms_per_step": round(ms, 2), "clips_per_s": round(B / ms * 1e3, 2)}
        line.update(kernel_figures(struct, B * T * P, P, T, a.x, a.kernel_iters, dev))
        print(json.dumps(line), flush=True)
        del det, opt
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
