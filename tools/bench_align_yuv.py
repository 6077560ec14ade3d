#!/usr/bin/env python3
"""Times the 4:2:0 entry points (csrc/yuv.hip) on the flagship clip batch and prints one JSON line.

Shape: B16 x T30 = 480 NV12 frames of 1080x1920 on the device (1.5 bytes per pixel: 1.49 GB), the crop geometry of
tools/bench_align.py (one similarity per frame, canvas 256, crop 150, scale factors 0.5 and 2).  Timed, each as `iters`
launches back to back between one HIP-event pair, divided by `iters`, `repeats` series, median / min / max in µs per launch:

  fused          dfd_align_crop_yuv420: NV12 frames -> crops, one launch
  two_step       dfd_yuv420_to_rgb_u8 of the whole frames, then dfd_align_crop_u8 on the planar RGB: what a caller without the
                 fused kernel runs
  rgb_crop       dfd_align_crop_u8 on planar RGB frames alone: the crop a caller pays who already has RGB
  convert        dfd_yuv420_to_rgb_u8 alone: reads 1.49 GB, writes 2.99 GB
  copy_out       a device-to-device copy of the crops' 32.4 MB (what `fused` and `rgb_crop` write)
  copy_convert   a device-to-device copy of as many bytes as `convert` moves in all (read + written), halved: a copy of N
                 bytes moves 2 N

The fused and the two-step crops are compared for equality before anything is timed.  Nothing is asserted about time.

usage: python tools/bench_align_yuv.py [--iters 20] [--repeats 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_align import CANVAS, CROP, H, W, make_plan, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    from dfd_clip_amd import align as AL
    from dfd_clip_amd import capi, yuv
    capi.load_library()
    B, T = 16, 30
    n = B * T
    out_bytes = n * 3 * CROP * CROP
    yuv_bytes, rgb_bytes = n * H * W * 3 // 2, n * H * W * 3
    res = {"tool": "bench_align_yuv", "shape": {"B": B, "T": T, "frame": [H, W], "source": "nv12", "canvas": CANVAS, "crop": CROP},
           "iters": args.iters, "repeats": args.repeats, "out_bytes": out_bytes, "yuv_bytes": yuv_bytes, "rgb_bytes": rgb_bytes}
    g = torch.Generator(device="cuda").manual_seed(0)
    surfaces = torch.randint(0, 256, (n, H + H // 2, W), dtype=torch.uint8, device="cuda", generator=g)   # packed NV12, pitch = W
    src = yuv.Yuv420.packed_nv12(surfaces, H, W)
    source, matrix = src.source(), yuv._c_matrix(None)
    rgb = torch.empty(n, 3, H, W, dtype=torch.uint8, device="cuda")
    out = torch.empty(n, 3, CROP, CROP, dtype=torch.uint8, device="cuda")

    a = torch.empty(out_bytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    copy_us, res["copy_out_us"] = timed(lambda: b.copy_(a), args.iters, args.repeats)
    half = (yuv_bytes + rgb_bytes) // 2
    big_a = rgb.view(-1)[:half]                       # `rgb` is scratch here; it is rewritten before it is read again
    big_b = torch.empty(half, dtype=torch.uint8, device="cuda")
    big_us, res["copy_convert_us"] = timed(lambda: big_b.copy_(big_a), args.iters, args.repeats)
    res["copy_convert_gbs_moved"] = round(2 * half / big_us / 1e3, 1)
    del big_b

    conv_us, res["convert_us"] = timed(lambda: capi.yuv420_to_rgb_u8(source, rgb, matrix), args.iters, args.repeats)
    res["convert_gbs_moved"] = round((yuv_bytes + rgb_bytes) / conv_us / 1e3, 1)
    res["convert_of_copy"] = round(big_us / conv_us, 3)

    for scale in (0.5, 2):
        plan = make_plan(n, scale, seed=int(scale * 10))
        rec = plan.on("cuda")
        fused = AL.FaceAligner.apply_yuv(src, plan)
        assert torch.equal(fused, AL.FaceAligner.apply(yuv.to_rgb(src), plan, layout="chw")), "fused and two-step crops differ"
        del fused

        def two_step():
            capi.yuv420_to_rgb_u8(source, rgb, matrix)
            capi.align_crop_u8(rgb, out, rec, capi.ALIGN_CHW, W, 3 * H * W, H, W)

        f_us, f = timed(lambda: capi.align_crop_yuv420(source, H, W, out, rec, matrix), args.iters, args.repeats)
        t_us, t = timed(two_step, args.iters, args.repeats)
        r_us, r = timed(lambda: capi.align_crop_u8(rgb, out, rec, capi.ALIGN_CHW, W, 3 * H * W, H, W), args.iters, args.repeats)
        res[f"scale_{scale}"] = {"fused_us": f, "two_step_us": t, "rgb_crop_us": r, "fused_of_two_step": round(t_us / f_us, 2),
                                 "fused_of_rgb_crop": round(r_us / f_us, 3), "fused_of_copy_out": round(copy_us / f_us, 3),
                                 "fused_frames_per_s": round(n / f_us * 1e6)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
