#!/usr/bin/env python3
"""One optimizer step of `FusedAdamW` (dfd-clip_amd/optim.py, csrc/optim.hip) against `torch.optim.AdamW(foreach=True)` on the
project's two AdamW parameter sets:

  detector  the ViT-B/16 `Detector`'s trainable parameters without an adapter (the decoder; its Linear weights mirrored:
            the fused launch also rewrites their transposed copies, which torch's step leaves to 20 transposes that are
            NOT in its figure)
  adapter   the shipped `768-x-768-nln` x = 256 adapter of the same model (6 tapped layers x (k, v)), no mirrors

Prints one JSON line.  Per set:
  fused_us / torch_us    one optimizer step, gradients in place, the fused step's gradient packing included: per-step HIP-event
                         times of `--steps` steps after `--warmup`, the two optimizers ALTERNATING in one window, as
                         {median, min, max}.  Steps run back to back, so a step that the host cannot enqueue as fast as the
                         device runs it shows its host time
  *_kernels_per_step     the device kernels a step launches (torch.profiler)
  kernel_us              the fused kernel alone: the last launch again (same table, same step count), per-launch event
                         times {median, min, max}.  Back-to-back launches re-read what the launch before left in L2 and the
                         256 MB Infinity Cache: the adapter set (166 MB a launch) fits it whole
  kernel_cold_us         the same launch after a 1 GiB fill has evicted both caches, which is how a training step finds them
                         after a forward and a backward pass
  kernel_GBps, kernel_cold_GBps, *_fraction_of_copy_ceiling
                         the bytes the step needs, 28 B per element (read p, g, m, v; write p, m, v) plus 4 B per mirrored
                         element, over the median, and that over the 6.29 TB/s copy ceiling DESIGN.md uses

usage: python tools/bench_adamw.py [--steps 100] [--warmup 5] [--out FILE]
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
from dfd_clip_amd.detector import Detector  # noqa: E402
from dfd_clip_amd.optim import FusedAdamW  # noqa: E402
from tests.cases import make_config  # noqa: E402

COPY_CEILING_GBS = 6290.0


def timed(fns, iters, before=None):
    """Per-call HIP-event times in us of each of `fns`, called in turn `iters` times; `before()` runs ahead of every call,
    outside its events."""
    evs = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)] for _ in fns]
    torch.cuda.synchronize()
    for i in range(iters):
        for fn, ev in zip(fns, evs):
            if before is not None:
                before()
            ev[i][0].record()
            fn()
            ev[i][1].record()
    torch.cuda.synchronize()
    return [[a.elapsed_time(b) * 1e3 for a, b in ev] for ev in evs]


def spread(us):
    return {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}


def kernels_per_step(fn):
    """Device kernels one call of `fn` launches, as torch.profiler sees them."""
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "memcpy" not in e.name.lower()
               and "memset" not in e.name.lower())


def measure(params, mirrors, steps, warmup):
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    for p, q in zip(params, twins):
        p.grad = torch.randn_like(p) * 1e-2
        q.grad = p.grad.clone()
    fused = FusedAdamW(params, lr=1e-4, weight_decay=0.01, mirrors=mirrors)
    plain = torch.optim.AdamW(twins, lr=1e-4, weight_decay=0.01, foreach=True)
    out = {"tensors": len(params), "elements": sum(p.numel() for p in params)}
    for opt in (fused, plain):
        for _ in range(warmup):
            opt.step()
    t_fused, t_torch = timed([fused.step, plain.step], steps)
    out.update(fused_us=spread(t_fused), torch_us=spread(t_torch), fused_kernels_per_step=kernels_per_step(fused.step),
               torch_kernels_per_step=kernels_per_step(plain.step))
    # the kernel alone: the last launch again (same table, same step count), outside the optimizer's host code
    seen, real = [], capi.sgd_step

    def recording(*a, **k):
        seen.append((a, k))
        return real(*a, **k)

    capi.sgd_step = recording
    try:
        fused.step()
    finally:
        capi.sgd_step = real
    assert len(seen) == 1, "one launch per steady-state step"
    a, k = seen[0]
    entries = fused._plans[0]["entries"]
    mirrored = sum(e["numel"] for e in entries if e["mirror"] is not None)
    nbytes = 28 * out["elements"] + 4 * mirrored
    evict = torch.empty(1 << 28, device=params[0].device, dtype=torch.float32)  # 1 GiB: four times the Infinity Cache
    warm, = timed([lambda: real(*a, **k)], steps)
    cold, = timed([lambda: real(*a, **k)], steps, before=evict.zero_)
    out.update(mirrored_elements=mirrored, kernel_bytes=nbytes, kernel_us=spread(warm), kernel_cold_us=spread(cold))
    for name, us in (("kernel", statistics.median(warm)), ("kernel_cold", statistics.median(cold))):
        out[name + "_GBps"] = round(nbytes / us / 1e3, 1)
        out[name + "_fraction_of_copy_ceiling"] = round(nbytes / us / 1e3 / COPY_CEILING_GBS, 3)
    out["fused_speedup_over_torch"] = round(out["torch_us"]["median"] / out["fused_us"]["median"], 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    logging.getLogger().setLevel(logging.ERROR)
    dev = "cuda:0"
    torch.manual_seed(0)
    line = {"workload": "adamw_step", "arch": "ViT-B/16", "steps": a.steps, "warmup": a.warmup, "copy_ceiling_GBps": COPY_CEILING_GBS,
            "device": torch.cuda.get_device_name(0)}
    cfg = make_config("ViT-B/16", decode_mode="stride", decode_stride=2)
    cfg.optimizer = "adamw"
    det = Detector(cfg, 30, None, precision="bf16").to(dev).train()
    assert isinstance(det.configure_optimizers(1e-4), FusedAdamW)
    line["detector"] = measure([p for p in det.parameters() if p.requires_grad], det.decoder, a.steps, a.warmup)
    del det
    cfg = make_config("ViT-B/16", decode_mode="stride", decode_stride=2, adapter__type="normal", adapter__frozen=0,
                      adapter__struct={"type": "768-x-768-nln", "x": 256})
    det = Detector(cfg, 30, None, precision="bf16").to(dev).train()
    line["adapter"] = measure(list(det.adapter.parameters()), None, a.steps, a.warmup)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
