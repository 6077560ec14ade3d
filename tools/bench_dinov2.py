#!/usr/bin/env python3
"""`Detector` with `foundation: dinov2` (ViT-B/14) at the shipped dino configuration (configs/deepfake/dino/*.yaml of
the reference: layers 6..11 tapped, `768-x-768-nln` adapter with x = 256, SGD), bf16, B clips x T frames.

Prints one JSON line (and writes it to --out when given):
  forward_*   forward-only `Detector.predict` (eval, no_grad): per-step HIP-event times after `--warmup` steps —
              median, min, max, interquartile spread — and clips/s from the median
  train_*     `harness.train_step` (forward, backward, SGD step) the same way
  fc1_*       in situ, same process: the MLP's first GEMM (M = B*T*257, N = 3072, K = 768) with the exact-erf GELU
              epilogue AND the same shape with DFD_EPI_BIAS_QUICKGELU, alternating, median of `--kernel-iters` timed
              launches each; their ratio is the cost of the exact erf
  vitl14_forward_*  the CLIP ViT-L/14 forward at the same batch (the same 257-token geometry, 24 layers at width 1024):
              the sanity reference — ViT-B/14 does half the layers at 3/4 the width, so it must come out faster

usage: python tools/bench_dinov2.py [--clips 16] [--frames 30] [--steps 10] [--warmup 3] [--graphs] [--out profiles/dinov2_bench.json]
"""
import argparse
import json
import logging
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from dfd_clip_amd import capi  # noqa: E402
from dfd_clip_amd.config import ConfigNode, default_detector_config  # noqa: E402
from dfd_clip_amd.detector import Detector  # noqa: E402
from dfd_clip_amd.harness import train_step  # noqa: E402


def per_step_ms(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    evs = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    torch.cuda.synchronize()
    evs[0].record()
    for i in range(steps):
        fn()
        evs[i + 1].record()
    torch.cuda.synchronize()
    return [evs[i].elapsed_time(evs[i + 1]) for i in range(steps)]


def summary(prefix, ms, clips):
    q = statistics.quantiles(ms, n=4) if len(ms) >= 4 else [min(ms), statistics.median(ms), max(ms)]
    med = statistics.median(ms)
    return {f"{prefix}_ms_median": round(med, 3), f"{prefix}_ms_min": round(min(ms), 3), f"{prefix}_ms_max": round(max(ms), 3),
            f"{prefix}_ms_iqr": round(q[2] - q[0], 3), f"{prefix}_clips_per_s": round(clips / med * 1e3, 2)}


def make_detector(foundation, arch, frames, adapter, dev):
    cfg = default_detector_config()
    cfg.foundation, cfg.architecture = foundation, arch
    cfg.out_dim, cfg.losses = [2], ["auc_roc"]
    cfg.decode_mode, cfg.decode_indices = ("index", [6, 7, 8, 9, 10, 11]) if foundation == "dinov2" else ("stride", [])
    cfg.dropout = 0.5
    if adapter:
        cfg.adapter = ConfigNode({"type": "normal", "frozen": 0, "struct": {"type": "768-x-768-nln", "x": 256}})
    torch.manual_seed(0)
    return Detector(cfg, frames, None, precision="bf16").to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=30)
    ap.add_argument("--no-vitl14", action="store_true", help="skip the ViT-L/14 sanity line")
    ap.add_argument("--graphs", action="store_true", help="train step: replay the decoder's / adapter's kernels as HIP graphs (Detector.static_graphs)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    logging.getLogger().setLevel(logging.ERROR)  # the random-initialisation notices
    dev = "cuda:0"
    B, T = a.clips, a.frames
    res = {"workload": "dinov2_vitb14_detector", "clips": B, "frames": T, "precision": "bf16", "adapter": "768-x-768-nln x=256",
           "layers_tapped": [6, 7, 8, 9, 10, 11], "steps": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    x = torch.randn(B, T, 3, 224, 224, device=dev)
    m = torch.ones(B, T, dtype=torch.bool, device=dev)
    y = (torch.arange(B, device=dev) % 2)

    det = make_detector("dinov2", "ViT-B/16", T, True, dev).eval()
    with torch.no_grad():
        res.update(summary("forward", per_step_ms(lambda: det.predict(x, m), a.steps, a.warmup), B))
    det.static_graphs = a.graphs
    res["train_graphs"] = a.graphs
    opt = det.configure_optimizers(0.005)
    batch = [(x, y, m, None, None, 0)]
    res.update(summary("train", per_step_ms(lambda: train_step(det, opt, batch), a.steps, a.warmup), B))
    del det, opt
    torch.cuda.empty_cache()

    # the fc1 GEMM with the two activation epilogues, alternating launches in one process
    M, N, K = B * T * 257, 3072, 768
    g = torch.Generator(device=dev).manual_seed(1)
    h = torch.randn(M, K, device=dev, generator=g).to(torch.bfloat16)
    w = (torch.randn(N, K, device=dev, generator=g) * K ** -0.5).to(torch.bfloat16)
    bias = torch.randn(N, device=dev, generator=g) * 0.1
    u = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
    times = {capi.EPI_BIAS_GELU: [], capi.EPI_BIAS_QUICKGELU: []}
    for it in range(a.kernel_iters + 3):
        for epi in times:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            capi.gemm(h, w, u, bias, epi, stream_out=True)
            e1.record()
            torch.cuda.synchronize()
            assert capi.gemm_last_path() == 257
            if it >= 3:
                times[epi].append(e0.elapsed_time(e1) * 1e3)
    us_g, us_q = statistics.median(times[capi.EPI_BIAS_GELU]), statistics.median(times[capi.EPI_BIAS_QUICKGELU])
    flops = 2.0 * M * N * K
    res.update({"fc1_M": M, "fc1_gelu_us": round(us_g, 1), "fc1_gelu_TFLOPs": round(flops / us_g / 1e6, 1),
                "fc1_gelu_us_min_max": [round(min(times[capi.EPI_BIAS_GELU]), 1), round(max(times[capi.EPI_BIAS_GELU]), 1)],
                "fc1_quickgelu_us": round(us_q, 1), "fc1_quickgelu_TFLOPs": round(flops / us_q / 1e6, 1),
                "fc1_quickgelu_us_min_max": [round(min(times[capi.EPI_BIAS_QUICKGELU]), 1), round(max(times[capi.EPI_BIAS_QUICKGELU]), 1)],
                "fc1_gelu_over_quickgelu": round(us_g / us_q, 4)})
    del h, w, u
    torch.cuda.empty_cache()

    if not a.no_vitl14:
        vl = make_detector("clip", "ViT-L/14", T, False, dev).eval()
        with torch.no_grad():
            res.update(summary("vitl14_forward", per_step_ms(lambda: vl.predict(x, m), a.steps, a.warmup), B))
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
