"""Speed against accuracy of the fp8 precision policy (`encoder.set_fp8_policy`), one JSON line per preset.

ViT-L/14, random weights (tests/cases.py `vitl14`: every second layer tapped).  Per preset:
  clips_per_s   forward of B8 x T30 clips: median / min / max over 5 rounds, the presets ALTERNATING within a round (so a
                drift of the machine hits every preset alike), each sample = `--steps` passes after `--warmup`;
  auroc ...     the 256-clip set of tests/test_hip_fp8.py::test_fp8_auroc_parity_vitl14 (labels Bernoulli(0.5) seed 7,
                calibration on the first 16 clips): AUROC, |dAUROC| and Spearman of p(real) against the bf16 path, max and
                mean |dlogit|;
  ref_fp32_err  max |logit - the reference's fp32 logit| on the committed fixture tests/golden/vitl14.npz;
  c_fc_frac     the fp8 c_fc GEMMs' FLOP/s as a fraction of the 5 PFLOP/s dense e4m3 peak (HIP events around each launch,
                in a pass of their own; null where no c_fc runs on e4m3).
Not a test; prints to stdout.  `python tools/bench_fp8_policy.py > profiles/fp8_policy.jsonl`."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dfd_clip_amd import capi  # noqa: E402
from dfd_clip_amd.detector import Detector  # noqa: E402
from dfd_clip_amd.encoder import FP8_PRESETS  # noqa: E402
from dfd_clip_amd.harness import binary_auroc  # noqa: E402
from tests.cases import build_case, load_golden  # noqa: E402

PEAK_FP8_TFLOPS = 5000.0  # dense, block-scaled e4m3 (MI355X chip specification; bench.py)


def spearman(a, b):
    ra, rb = np.argsort(np.argsort(a)), np.argsort(np.argsort(b))
    return float(np.corrcoef(ra, rb)[0, 1])


def auroc(y, s):
    return float(binary_auroc(list(y) + [0, 1], list(s) + [0.0, 1.0]))  # dummy pair appended as the reference's inference does


def make(case, precision):
    det = Detector(case["cfg"], case["T"], None, precision=precision)
    det.load_state_dict(case["sd"])
    return det.cuda().eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--clips", type=int, default=8)
    ap.add_argument("--frames", type=int, default=30)
    args = ap.parse_args()
    capi.load_library()
    case = build_case("vitl14")
    T, res, n_clips = case["T"], case["res"], 256
    x = torch.from_numpy(np.random.default_rng(4321).standard_normal((n_clips, T, 3, res, res), dtype=np.float32))
    m = torch.ones(n_clips, T, dtype=torch.bool)
    m[3::7, T - 1:] = False
    y = np.random.default_rng(7).integers(0, 2, n_clips)
    gold = torch.from_numpy(load_golden("vitl14")["logits"]).float()

    def outputs(det):
        p, lg = [], []
        with torch.no_grad():
            for i in range(0, n_clips, 32):
                logits = det.predict(x[i:i + 32].cuda(), m[i:i + 32].cuda())[0][0]
                p.append(logits.softmax(dim=-1)[:, 1].cpu())
                lg.append(logits.float().cpu())
            g = det.predict(case["x"].cuda(), case["m"].cuda())[0][0].float().cpu()
        return torch.cat(p).numpy(), torch.cat(lg), (g - gold.view_as(g)).abs().max().item()

    det16 = make(case, "bf16")
    p16, l16, g16 = outputs(det16)
    a16 = auroc(y, p16)
    del det16
    torch.cuda.empty_cache()
    det = make(case, "fp8")
    det.calibrate_fp8(x[:16].cuda())
    rows = {}
    for preset in FP8_PRESETS:
        det.set_fp8_policy(preset)
        p, lg, g = outputs(det)
        d = (lg - l16).abs()
        a = auroc(y, p)
        rows[preset] = dict(preset=preset, auroc=round(a, 5), auroc_bf16=round(a16, 5), d_auroc=round(abs(a - a16), 6),
                            spearman=round(spearman(p16, p), 5), dlogit_max=round(d.max().item(), 4), dlogit_mean=round(d.mean().item(), 4),
                            ref_fp32_err=round(g, 4), ref_fp32_err_bf16=round(g16, 4))

    # throughput: one detector at the bench shape (the temporal positional embedding fixes T), policies alternating
    from dfd_clip_amd.weights import random_state_dict
    B, Tb = args.clips, args.frames
    big = Detector(case["cfg"], Tb, None, precision="fp8")
    big.load_state_dict(random_state_dict(case["cfg"], Tb, seed=0))
    big = big.cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(13)
    xb = torch.randn(B, Tb, 3, res, res, device="cuda", generator=gen)
    mb = torch.ones(B, Tb, dtype=torch.bool, device="cuda")
    big.calibrate_fp8(xb[:2])
    samples = {p: [] for p in FP8_PRESETS}
    with torch.no_grad():
        for _ in range(args.rounds):
            for preset in FP8_PRESETS:
                big.set_fp8_policy(preset)
                for _ in range(args.warmup):
                    big.predict(xb, mb)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    big.predict(xb, mb)
                torch.cuda.synchronize()
                samples[preset].append(B * args.steps / (time.perf_counter() - t0))
        for preset in FP8_PRESETS:  # the c_fc GEMMs alone, event-timed, in a pass of their own
            big.set_fp8_policy(preset)
            plan = big.encoder.fp8_policy()
            big.predict(xb, mb)
            torch.cuda.synchronize()
            capi.profile_gemm(big.encoder.act_epilogue)
            big.predict(xb, mb)
            torch.cuda.synchronize()
            spans = capi.profile_gemm_collect()
            last = max(big.layer_indices)  # the last tapped layer stops after its projection: c_fc runs in the layers below it
            f8 = [s for l, s in enumerate(spans) if l < last and plan[l]["fc"] == "fp8"] if len(spans) == last else []
            ms, flops = sum(e - b for b, e, _ in f8), sum(f for _, _, f in f8)
            rows[preset]["c_fc_frac"] = round(flops / (ms * 1e-3) / (PEAK_FP8_TFLOPS * 1e12), 4) if ms > 0 else None
            rows[preset]["c_fc_ms"] = round(ms / len(f8), 4) if f8 else None
    for preset in FP8_PRESETS:
        s = samples[preset]
        rows[preset]["clips_per_s"] = dict(median=round(statistics.median(s), 1), min=round(min(s), 1), max=round(max(s), 1))
        rows[preset]["shape"] = f"ViT-L/14 B{B}xT{Tb} forward, {args.rounds} rounds x {args.steps} steps"
        print(json.dumps(rows[preset]), flush=True)


if __name__ == "__main__":
    main()
