#!/usr/bin/env python3
"""Times dfd_align_crop_u8 (csrc/align.hip) on the flagship clip batch and prints one JSON line.

Shape: B16 x T30 = 480 interleaved uint8 frames of 1080x1920 on the device, one similarity per frame (the face drifts and
turns a little from frame to frame), canvas 256, crop 150, at scale factors 0.5 (a face 300 px wide in the frame) and 2 (a
face 75 px wide).  A series is `iters` launches back to back between one HIP-event pair, divided by `iters`; `repeats`
series give median / min / max.  The kernel writes 480 x 3 x 150 x 150 = 32.4 MB and gathers its sources through the caches, so
GB/s counts OUTPUT bytes only and stands beside a device-to-device copy of the same 32.4 MB timed the same way in the same
process (a copy reads as much as it writes; the kernel reads up to four taps per byte, mostly from cache).  `window512` is
the same work on 512x512 windows per frame (`AlignPlan.window`): what a caller uploads who cuts the face region on the host.
`cpu_pil` times PIL's Image.transform(AFFINE, BILINEAR) of one 1080x1920 RGB frame to 150x150 on the host, per frame and
single-threaded: PIL, not OpenCV, which is not installed.  Nothing is asserted.

usage: python tools/bench_align.py [--iters 30] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, CANVAS, CROP = 1080, 1920, 256, 150


def series(fn, iters):
    """-> µs per launch: `iters` launches back to back between one event pair (the queue stays full, so the host's launch
    cost is hidden for all but the first)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def timed(fn, iters, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    runs = [series(fn, iters) for _ in range(repeats)]
    return statistics.median(runs), {"median": round(statistics.median(runs), 2), "min": round(min(runs), 2), "max": round(max(runs), 2)}


def make_plan(n, scale, seed):
    """One similarity per frame: source point (cx, cy), drifting over the middle of the frame, lands on the canvas centre."""
    from dfd_clip_amd import align as AL
    rng = np.random.default_rng(seed)
    f = np.arange(n)
    cx = W / 2 + 300 * np.sin(f / 37.0) + rng.normal(0, 2, n)
    cy = H / 2 + 150 * np.cos(f / 53.0) + rng.normal(0, 2, n)
    th = 0.15 * np.sin(f / 11.0)
    fwd = np.zeros((n, 2, 3))
    fwd[:, 0, 0] = fwd[:, 1, 1] = scale * np.cos(th)
    fwd[:, 1, 0] = scale * np.sin(th)
    fwd[:, 0, 1] = -fwd[:, 1, 0]
    ctr = np.stack([cx, cy], 1)
    fwd[:, :, 2] = (CANVAS - 1) / 2.0 - np.einsum("fij,fj->fi", fwd[:, :, :2], ctr)
    origin = np.full((n, 2), (CANVAS - CROP) // 2)
    return AL.AlignPlan(fwd, AL.invert_affine(fwd), origin, np.ones(n, bool), CROP, CANVAS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from dfd_clip_amd import align as AL
    from dfd_clip_amd import capi
    capi.load_library()
    B, T = 16, 30
    n = B * T
    out_bytes = n * 3 * CROP * CROP
    res = {"tool": "bench_align", "shape": {"B": B, "T": T, "frame": [H, W], "layout": "hwc", "canvas": CANVAS, "crop": CROP},
           "iters": args.iters, "repeats": args.repeats, "out_bytes": out_bytes}
    g = torch.Generator(device="cuda").manual_seed(0)
    frames = torch.randint(0, 256, (n, H, W, 3), dtype=torch.uint8, device="cuda", generator=g)
    a, b = torch.empty(out_bytes, dtype=torch.uint8, device="cuda"), torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    copy_us, res["copy_us"] = timed(lambda: b.copy_(a), args.iters, args.repeats)
    res["copy_gbs_written"] = round(out_bytes / copy_us / 1e3, 1)

    def row(us, spread):
        return {"us": spread, "gbs_out": round(out_bytes / us / 1e3, 1), "of_copy": round(copy_us / us, 3), "frames_per_s": round(n / us * 1e6)}

    for scale in (0.5, 2):
        plan = make_plan(n, scale, seed=int(scale * 10))
        out = torch.empty(n, 3, CROP, CROP, dtype=torch.uint8, device="cuda")
        rec = plan.on("cuda")
        us, spread = timed(lambda: capi.align_crop_u8(frames, out, rec, capi.ALIGN_HWC, 3 * W, 3 * W * H, H, W), args.iters, args.repeats)
        res[f"full_scale_{scale}"] = row(us, spread)
        (wh, ww), org = plan.window(0, (H, W))
        assert wh <= 512 and ww <= 512, (wh, ww)
        org = np.stack([np.minimum(org[:, 0], W - 512), np.minimum(org[:, 1], H - 512)], 1)
        windows = torch.stack([frames[f, y:y + 512, x:x + 512] for f, (x, y) in enumerate(org)]).contiguous()
        wplan = plan.with_window(org, (512, 512))
        assert torch.equal(AL.FaceAligner.apply(windows, wplan), AL.FaceAligner.apply(frames, plan))
        wrec = wplan.on("cuda")
        us, spread = timed(lambda: capi.align_crop_u8(windows, out, wrec, capi.ALIGN_HWC, 3 * 512, 3 * 512 * 512, 512, 512), args.iters, args.repeats)
        res[f"window512_scale_{scale}"] = dict(row(us, spread), footprint=[wh, ww], upload_bytes=int(windows.numel()))
        del windows
    try:
        from PIL import Image
        host = Image.fromarray(frames[0].cpu().numpy())
        cpu = {}
        for scale in (0.5, 2):
            inv = make_plan(1, scale, seed=1).inverse[0]
            data = tuple(inv.reshape(-1))
            t0 = time.perf_counter()
            for _ in range(50):
                host.transform((CROP, CROP), Image.Transform.AFFINE, data, resample=Image.Resampling.BILINEAR)
            dt = (time.perf_counter() - t0) / 50
            cpu[f"scale_{scale}"] = {"us_per_frame": round(dt * 1e6, 1), "frames_per_s": round(1 / dt)}
        res["cpu_pil"] = dict(cpu, what="PIL Image.transform(AFFINE, BILINEAR), one thread, one 1080x1920 RGB frame -> 150x150")
    except ImportError:
        res["cpu_pil"] = None
    print(json.dumps(res))


if __name__ == "__main__":
    main()
