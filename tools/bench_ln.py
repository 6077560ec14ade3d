#!/usr/bin/env python3
"""Microbenchmark of the LayerNorm family (f32 rows in, bf16 rows out, bf16 deltas) through the C ABI.

    bench_ln.py [rows] [cols] [--kind plain|two|add1|add2|add1_nostore] [--dual] [--iters N]

Without options: dfd_layernorm, 480 * 197 rows of 768 columns."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dfd_clip_amd import capi  # noqa: E402

KINDS = ("plain", "two", "add1", "add2", "add1_nostore")
NAMES = {"plain": "layernorm", "two": "layernorm2", "add1": "add_layernorm", "add2": "add_layernorm(2 deltas)",
         "add1_nostore": "add_layernorm(no store)"}


def bench(kind="plain", dual=False, rows=480 * 197, cols=768, iters=20):
    """(label, microseconds per call, algorithmic GB/s) of one form of the family."""
    x = torch.randn(rows, cols, device="cuda")
    ga, ba, g, b = (torch.randn(cols, device="cuda") for _ in range(4))
    y = torch.empty(rows, cols, device="cuda", dtype=torch.bfloat16)
    n_deltas = 2 if kind == "add2" else int(kind.startswith("add"))
    deltas = [torch.randn(rows, cols, device="cuda").to(torch.bfloat16) for _ in range(n_deltas)]
    out = (y, torch.empty(rows, cols, device="cuda", dtype=torch.uint8), 0.25) if dual else (y,)
    if kind == "plain":
        fn = capi.layernorm_dual if dual else capi.layernorm
        call = lambda: fn(x, g, b, *out)
    elif kind == "two":  # (x is overwritten by its own LayerNorm each call: the values change, the traffic does not)
        fn = capi.layernorm2_dual if dual else capi.layernorm2
        call = lambda: fn(x, ga, ba, g, b, *out)
    else:
        fn = capi.add_layernorm_dual if dual else capi.add_layernorm
        kw = dict(delta2=deltas[1] if kind == "add2" else None, store_x=kind != "add1_nostore")
        call = lambda: fn(x, deltas[0], g, b, *out, **kw)
    # bytes per element: x read, x written (two; add unless no store), 2 per delta, y (2, or 2 + 1 for the dual forms)
    per_elem = 4 + 4 * (kind == "two" or (kind.startswith("add") and kind != "add1_nostore")) + 2 * len(deltas) + (3 if dual else 2)
    for _ in range(3):
        call()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / iters
    return NAMES[kind] + ("_dual" if dual else ""), ms * 1e3, rows * cols * per_elem / ms / 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("rows", nargs="?", type=int, default=480 * 197)
    ap.add_argument("cols", nargs="?", type=int, default=768)
    ap.add_argument("--kind", choices=KINDS, default="plain")
    ap.add_argument("--dual", action="store_true", help="the form that also writes y as e4m3")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    capi.load_library()
    label, us, gbs = bench(a.kind, a.dual, a.rows, a.cols, a.iters)
    print(f"{label} rows={a.rows} cols={a.cols}: {us:.1f} us  {gbs:.0f} GB/s")


if __name__ == "__main__":
    main()
