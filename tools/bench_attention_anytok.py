#!/usr/bin/env python3
"""The streaming bf16 MFMA attention kernel (csrc/attention_mfma_any.hip) against the rows kernel that served the same
token counts before it (`capi.attention_set_variant(2)`), through `capi.attention_fwd` on the same inputs.

Token counts 50, 226, 577 and 1370 at frames * heads >= 3840 items (50, 226, 1370: 320 frames x 12 heads; 577: 240 x 16).
Each of 5 runs times `--iters` back-to-back launches of one kernel with HIP events, the two kernels ALTERNATING run by
run; per token count the line carries {median, min, max} of the per-launch microseconds over the runs and the FLOP/s of
the median at 4 * tokens^2 * 64 FLOP per item.  `faster` is the bar of DESIGN §4: the streaming kernel's slowest run
against the rows kernel's fastest.  At 1370 tokens the rows kernel is not timed (bf16 had no kernel there before).

Beside them `attn_mfma_kernel<9>` — all scores in registers, no online rescale — at 257 tokens, 240 frames x 16 heads in
launches of 16 frames (256 items: below the persistent kernel's threshold), as the yardstick per (query, key) pair;
`pair_ratio` = streaming kernel's picoseconds per pair over the yardstick's.  Reported, not gated.

Prints one JSON line.  usage: python tools/bench_attention_anytok.py [--iters 3] [--runs 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dfd_clip_amd import capi  # noqa: E402

SHAPES = [(50, 320, 12), (226, 320, 12), (577, 240, 16), (1370, 320, 12)]  # tokens, frames, heads


def timed_us(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def spread(us):
    return {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    capi.load_library()
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"bench": "attention_anytok", "device": torch.cuda.get_device_name(0), "iters": args.iters, "runs": args.runs, "tokens": {}}

    def make(tokens, frames, heads):
        qkv = torch.randn(frames * tokens, 3 * heads * 64, device="cuda", generator=g).to(torch.bfloat16)
        return qkv, torch.empty(frames * tokens, heads * 64, device="cuda", dtype=torch.bfloat16)

    for tokens, frames, heads in SHAPES:
        qkv, out = make(tokens, frames, heads)

        def launch(variant):
            def fn():
                capi.attention_fwd(qkv, out, frames, tokens, heads)

            def run():
                capi.attention_set_variant(variant)
                try:
                    return timed_us(fn, args.iters)
                finally:
                    capi.attention_set_variant(0)
            return run
        kernels = {"mfma_any": launch(0)} if tokens > 640 else {"mfma_any": launch(0), "rows": launch(2)}
        for run in kernels.values():
            run()  # warm-up
        us = {k: [] for k in kernels}
        for _ in range(args.runs):
            for k, run in kernels.items():
                us[k].append(run())
        flop = 4.0 * tokens * tokens * 64 * frames * heads
        row = {"frames": frames, "heads": heads, "items": frames * heads}
        for k, v in us.items():
            row[k + "_us"] = spread(v)
            row[k + "_TFLOPs"] = round(flop / statistics.median(v) / 1e6, 1)
        if "rows" in us:
            row["faster"] = max(us["mfma_any"]) < min(us["rows"])
            row["speedup_median"] = round(statistics.median(us["rows"]) / statistics.median(us["mfma_any"]), 1)
        row["ps_per_pair"] = round(statistics.median(us["mfma_any"]) * 1e6 / (frames * heads * tokens * tokens), 3)
        res["tokens"][str(tokens)] = row
        del qkv, out

    tokens, frames, heads, step = 257, 240, 16, 16
    qkv, out = make(tokens, frames, heads)

    def yard():
        for f0 in range(0, frames, step):
            capi.attention_fwd(qkv[f0 * tokens:(f0 + step) * tokens], out[f0 * tokens:(f0 + step) * tokens], step, tokens, heads)
    timed_us(yard, 1)
    ys = [timed_us(yard, args.iters) for _ in range(args.runs)]
    ps = statistics.median(ys) * 1e6 / (frames * heads * tokens * tokens)
    res["yardstick_mfma9_257"] = {"frames": frames, "heads": heads, "frames_per_launch": step, "us": spread(ys),
                                  "TFLOPs": round(4.0 * tokens * tokens * 64 * frames * heads / statistics.median(ys) / 1e6, 1),
                                  "ps_per_pair": round(ps, 3)}
    for row in res["tokens"].values():
        row["pair_ratio"] = round(row["ps_per_pair"] / ps, 2)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
