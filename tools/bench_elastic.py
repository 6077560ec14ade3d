#!/usr/bin/env python3
"""Times the elastic warp (`dfd_elastic_field`, `dfd_elastic_remap_u8`, csrc/elastic.hip) on the flagship clip batch, prints
one JSON line and writes it to profiles/elastic_bench.json.

Shape: B16 x T30 uint8 clips at 224x224 and at 150x150 (the reference's face crop), one field per clip, the reference's
alpha = 50 and sigma = 6 (49 taps).  Four lines per size: `field` (16 fields), `remap` (every clip warped by its own field),
`both` (the two launches back to back: what `SslFake.apply` costs with every coin fired) and `copy` (a device-to-device
copy of the same clips, timed the same way in the same process).  A series is `iters` launches back to back between one
HIP-event pair, divided by `iters`; `repeats` series give median / min / max.  GB/s counts the bytes a line must move: the
field's bytes for `field`, in + out + field for `remap` and `both`, in + out for `copy`.  `remap_over_copy` is the remap's
time over the copy's: its floor is the copy plus the re-read of the field.  `half` is the remap with every second clip
copied (an index of -1), the mix a training step sees at p = 0.5 on real clips.  Nothing is asserted.

usage: python tools/bench_elastic.py [--iters 30] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def series(fn, iters):
    """-> µs per call: `iters` calls back to back between one event pair"""
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
    med = statistics.median(runs)
    return med, {"median": round(med, 2), "min": round(min(runs), 2), "max": round(max(runs), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from dfd_clip_amd import capi
    from dfd_clip_amd import elastic as E
    capi.load_library()
    B, T = 16, 30
    ssl = E.SslFake(alpha=50.0, sigma=6.0, p=1.0, seed=0)
    params = ssl.draw(B)
    ids = params.on("cuda")[1]
    every = torch.arange(B, dtype=torch.int32, device="cuda")
    half = torch.where(every % 2 == 0, every, torch.full_like(every, -1))
    out = {"tool": "bench_elastic", "shape": {"B": B, "T": T}, "alpha": ssl.alpha, "sigma": ssl.sigma, "taps": len(ssl.taps),
           "iters": args.iters, "repeats": args.repeats}
    g = torch.Generator().manual_seed(0)
    for res in (224, 150):
        low = torch.rand(B * T, 3, res // 16, res // 16, generator=g) * 255
        x = torch.nn.functional.interpolate(low, size=(res, res), mode="bilinear") + 12 * torch.randn(B * T, 3, res, res, generator=g)
        x = x.round().clamp(0, 255).to(torch.uint8).view(B, T, 3, res, res).cuda()
        y = torch.empty_like(x)
        field = torch.empty(B, res, res, 2, dtype=torch.int16, device="cuda")
        clip_bytes, field_bytes = x.numel(), field.numel() * 2
        calls = {"field": (lambda: capi.elastic_field(field, ids, params.seed, params.taps, params.alpha_q), field_bytes),
                 "remap": (lambda: capi.elastic_remap_u8(x, y, field, every), 2 * clip_bytes + field_bytes),
                 "half": (lambda: capi.elastic_remap_u8(x, y, field, half), 2 * clip_bytes + field_bytes // 2),
                 "both": (lambda: (capi.elastic_field(field, ids, params.seed, params.taps, params.alpha_q),
                                   capi.elastic_remap_u8(x, y, field, every)), 2 * clip_bytes + field_bytes),
                 "copy": (lambda: y.copy_(x), 2 * clip_bytes)}
        row = {"clip_bytes": clip_bytes, "field_bytes": field_bytes}
        med = {}
        for name, (fn, nbytes) in calls.items():
            med[name], spread = timed(fn, args.iters, args.repeats)
            row[name] = {"us": spread, "gbs": round(nbytes / med[name] / 1e3, 1)}
        row["remap_over_copy"] = round(med["remap"] / med["copy"], 3)
        row["clips_per_s_both"] = round(B / med["both"] * 1e6, 1)
        out[f"{res}x{res}"] = row
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "elastic_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
