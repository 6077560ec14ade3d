#!/usr/bin/env python3
"""Times dfd_decoder_attn_map beside dfd_decoder_attn_fwd on the flagship decoder shape and prints one JSON line.

Shape: B16 x T30 x 196 patches, 12 heads, bf16 keys / values; dense export and in place (a strided view of a
[frames, tokens, 3D] activation with the positional embedding added on the fly).  The map and the forward run in
ALTERNATING launches on the same inputs (one HIP-event pair per launch); `repeats` such series give median / min / max
of the per-series medians.  The map reads K only, half the forward's bytes, so its floor is K's bytes (plus the f32 map it
writes) over the copy ceiling DESIGN.md uses (6.29 TB/s).  Nothing is asserted.

usage: python tools/bench_attention_map.py [--iters 50] [--repeats 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_CEILING_TBS = 6.29


def series(fn_a, fn_b, iters):
    """-> per-launch µs of fn_a and fn_b, launched alternately"""
    ta, tb = [], []
    ev = lambda: torch.cuda.Event(enable_timing=True)
    for _ in range(iters):
        for fn, out in ((fn_a, ta), (fn_b, tb)):
            e0, e1 = ev(), ev()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(ta), statistics.median(tb)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from dfd_clip_amd import capi
    capi.load_library()
    B, T, P, H = 16, 30, 196, 12
    D, S, tok = H * 64, T * P, P + 1
    g = torch.Generator().manual_seed(0)
    f32 = dict(device="cuda", dtype=torch.float32)
    qkv = torch.randn(B * T, tok, 3 * D, generator=g).to(torch.bfloat16).cuda()
    pos = (0.3 * torch.randn(T, D, generator=g)).cuda()
    q = torch.randn(B, 2 * D, generator=g).cuda()
    m = torch.ones(B, T, dtype=torch.uint8, device="cuda")
    splits = 48
    ws = torch.empty(capi.decoder_attn_workspace_bytes(B, H, 64, splits) // 4, **f32)
    mix, stats, aff = torch.empty(B, D, **f32), torch.empty(B, H, 2, **f32), torch.empty(B, H, S, **f32)
    layouts = {
        "dense": (qkv[:, 1:, D:2 * D].contiguous().view(B * S, D), qkv[:, 1:, 2 * D:].contiguous().view(B * S, D), None),
        "in_place": (qkv[:, 1:, D:2 * D], qkv[:, 1:, 2 * D:], pos),
    }
    k_bytes, map_bytes = B * S * D * 2, B * H * S * 4
    out = {"tool": "bench_attention_map", "shape": {"B": B, "T": T, "patches": P, "heads": H, "kv": "bf16"}, "iters": args.iters,
           "repeats": args.repeats, "k_bytes": k_bytes, "map_bytes": map_bytes,
           "map_floor_us": round((k_bytes + map_bytes) / (COPY_CEILING_TBS * 1e12) * 1e6, 2)}
    for name, (k, v, p) in layouts.items():
        fwd = lambda: capi.decoder_attn_fwd(q, k, v, m, mix, stats, ws, splits, B, T, P, H, pos=p)
        amap = lambda: capi.decoder_attn_map(q, k, m, stats, aff, B, T, P, H, pos=p)
        for _ in range(5):
            fwd(), amap()
        torch.cuda.synchronize()
        runs = [series(amap, fwd, args.iters) for _ in range(args.repeats)]
        stat = lambda xs: {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}
        mp, fw = stat([r[0] for r in runs]), stat([r[1] for r in runs])
        out[name] = {"map_us": mp, "fwd_us": fw, "map_gbs": round((k_bytes + map_bytes) / mp["median"] / 1e3, 1),
                     "fwd_gbs": round(2 * k_bytes / fw["median"] / 1e3, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
