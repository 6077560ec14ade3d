#!/usr/bin/env python3
"""Times the SwiGLU gate (`dfd_swiglu_fwd`, csrc/swiglu.hip) at ViT-g/14's shapes, prints one JSON line and writes it to
profiles/swiglu_bench.json.

Shapes: bf16, H = 4096, rows = 123,360 (B16 x T30 x 257 tokens: one layer's gate of the flagship batch) and 61,680
(B8 x T30).  The kernel reads x12 [rows, 2H] once and writes hidden [rows, H]: 3 * rows * H elements moved.  It is judged
against `copy`: a device-to-device copy that moves the SAME number of bytes (read + written), i.e. of 1.5 * rows * H
elements, timed the same way in the same process.  A series is `iters` launches back to back between one HIP-event pair,
divided by `iters`; `repeats` series give median / min / max.  GB/s counts read + written bytes.  `swiglu_over_copy` is the
gate's median time over the copy's: 1.0 means the gate moves its bytes as fast as a copy does.  `element` times the
element-by-element form on the same shape (a base pointer one element off), for the record.  Nothing is asserted.

usage: python tools/bench_swiglu.py [--iters 20] [--repeats 5]
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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_swiglu needs a GPU: a time taken anywhere else says nothing")
    from dfd_clip_amd import capi
    capi.load_library()
    H, tokens, T = 4096, 257, 30
    out = {"tool": "bench_swiglu", "dtype": "bf16", "H": H, "iters": args.iters, "repeats": args.repeats}
    g = torch.Generator(device="cuda").manual_seed(0)
    for B in (16, 8):
        rows = B * T * tokens
        x12 = torch.empty(rows * 2 * H + 8, device="cuda", dtype=torch.bfloat16)
        x12.normal_(generator=g)
        hidden = torch.empty(rows * H + 8, device="cuda", dtype=torch.bfloat16)
        n_copy = rows * H * 3 // 2
        dst = torch.empty(n_copy, device="cuda", dtype=torch.bfloat16)
        moved = 3 * rows * H * 2
        xv, hv = x12[:rows * 2 * H].view(rows, 2 * H), hidden[:rows * H].view(rows, H)
        xo, ho = x12[1:1 + rows * 2 * H].view(rows, 2 * H), hidden[1:1 + rows * H].view(rows, H)
        capi.swiglu_fwd(xv, hv)
        assert capi.swiglu_last_path() == capi.SWIGLU_VEC16
        capi.swiglu_fwd(xo, ho)
        assert capi.swiglu_last_path() == capi.SWIGLU_ELEMENT
        calls = {"swiglu": lambda: capi.swiglu_fwd(xv, hv), "copy": lambda: dst.copy_(x12[:n_copy]),
                 "element": lambda: capi.swiglu_fwd(xo, ho)}
        row, med = {"rows": rows, "bytes_moved": moved}, {}
        for name, fn in calls.items():
            med[name], spread = timed(fn, args.iters, args.repeats)
            row[name] = {"us": spread, "gbs": round(moved / med[name] / 1e3, 1)}
        row["swiglu_over_copy"] = round(med["swiglu"] / med["copy"], 3)
        out[f"B{B}xT{T}"] = row
        del x12, hidden, dst, xv, hv, xo, ho
        torch.cuda.empty_cache()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "swiglu_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
