#!/usr/bin/env python3
"""Times dfd_augment_u8 (csrc/augment.hip) on the flagship clip batch and prints one JSON line.

Shape: B16 x T30 uint8 frames at 224x224 and at 150x150 (the reference's face crop).  Four parameter tables per size:
`copy` (every frame's set does nothing), `colour` (RGB table + HSV shift + tone table on every frame), `jpeg` (quality 75
on every frame) and `normal` (one draw of the reference's `normal` preset per clip: each transform with its own
probability).  Each launch sits between one HIP-event pair; `repeats` series of `iters` launches give median / min / max
of the per-series medians.  The kernel moves 2 bytes per sample (one read, one write), so GB/s is 2 * bytes / time, set
against the copy ceiling DESIGN.md uses (6.29 TB/s); clips/s is B over the launch time.  Nothing is asserted.

usage: python tools/bench_augment.py [--iters 30] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_CEILING_TBS = 6.29


def series(fn, iters):
    """-> median per-launch µs"""
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ts)


def tables(B, T):
    from dfd_clip_amd import augment as A
    per_clip = np.repeat(np.arange(B, dtype=np.int32), T)
    copy = A.new_sets(B)
    colour = A.new_sets(B)
    colour["flags"] = A.FLAG_RGB_LUT | A.FLAG_HSV | A.FLAG_TONE_LUT
    colour["rgb_lut"] = np.clip(np.arange(256) + 7, 0, 255).astype(np.uint8)
    colour["tone_lut"] = np.clip(np.arange(256) * 1.1 - 9.0, 0, 255).astype(np.uint8)
    colour["hue"], colour["sat"], colour["val"] = 11, -20, 8
    jpeg = A.new_sets(B)
    jpeg["quality"] = 75
    (_, normal, idx), = A.ClipAugment("normal", seed=0).draw(B, T).stages
    assert np.array_equal(idx, per_clip)
    return {"copy": copy, "colour": colour, "jpeg": jpeg, "normal": normal}, per_clip


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from dfd_clip_amd import capi
    capi.load_library()
    B, T = 16, 30
    sets, per_clip = tables(B, T)
    idx = torch.from_numpy(per_clip).cuda()
    out = {"tool": "bench_augment", "shape": {"B": B, "T": T}, "iters": args.iters, "repeats": args.repeats,
           "copy_ceiling_tbs": COPY_CEILING_TBS,
           "normal_draw": {"jpeg_clips": int((sets["normal"]["quality"] > 0).sum()), "colour_clips": int((sets["normal"]["flags"] & 7 > 0).sum()),
                           "flipped_clips": int((sets["normal"]["flags"] & 8 > 0).sum())}}
    g = torch.Generator().manual_seed(0)
    for res in (224, 150):
        low = torch.rand(B * T, 3, res // 16, res // 16, generator=g) * 255
        x = torch.nn.functional.interpolate(low, size=(res, res), mode="bilinear") + 12 * torch.randn(B * T, 3, res, res, generator=g)
        x = x.round().clamp(0, 255).to(torch.uint8).cuda()
        y = torch.empty_like(x)
        nbytes = x.numel()
        row = {"bytes_per_launch": 2 * nbytes, "floor_us": round(2 * nbytes / (COPY_CEILING_TBS * 1e12) * 1e6, 2)}
        for name, table in sets.items():
            s = torch.from_numpy(table.view(np.uint8).reshape(len(table), -1).copy()).cuda()
            fn = lambda: capi.augment_u8(x, y, s, idx)
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            runs = [series(fn, args.iters) for _ in range(args.repeats)]
            med = statistics.median(runs)
            row[name] = {"us": {"median": round(med, 2), "min": round(min(runs), 2), "max": round(max(runs), 2)},
                         "gbs": round(2 * nbytes / med / 1e3, 1), "of_ceiling": round(2 * nbytes / med / 1e3 / (COPY_CEILING_TBS * 1e3), 3),
                         "clips_per_s": round(B / med * 1e6, 1)}
        out[f"{res}x{res}"] = row
    print(json.dumps(out))


if __name__ == "__main__":
    main()
