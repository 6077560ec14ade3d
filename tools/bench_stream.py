#!/usr/bin/env python3
"""Times overlapping-window and live verdicts over the per-frame K/V store (dfd_clip_amd/stream.py) beside the only means
there was before it (`predict` on materialised `crops[table]`); prints one JSON line and writes it to `--out`
(default profiles/stream_bench.json).

Setup: ViT-B/16, bf16, T = 30, layers 6..11 tapped (bench.py's model), no adapter, one synthetic video of 900 frames of
224 x 224 uint8 crops on the device, every frame valid.  All arms run in ONE process on ONE model, alternating.

(a) windows   hop 30 / 15 / 5 / 1.  "predict": per batch of 16 windows, `crops[table[i:i+16]]` is materialised and goes through
              `predict` (the tower re-encodes every frame T / hop times).  "store": a `StreamingVerdict` (encode_chunk 480 =
              16 clips, batch 16) is fed the video and flushed; every window batch is gathered into a dense buffer
              (`gather="copy"`).  "table": the same with `gather="table"`: the decoder reads the ring in place through the slot
              table.  All copy each batch's logits to the host.  A series is one video on the host clock between two device
              synchronisations; each arm is warmed with one video per hop, then 5 series per arm, alternating.  ms per video,
              windows/s, tower frames/s as median / min / max, and the peak of allocated device memory over the arm's
              series (above what was allocated when the series began).  The yardstick of "table" is "store" of the same run.
(b) harness   `infer_raw_video(hop=None)` beside `hop=30` and `hop=30, gather="table"` on 900 frames of 256 x 256 with landmarks
              (aligner crop 224): what the K/V copies per frame cost against the path that stays the default.
(c) kernel    `dfd_kv_move_frames` alone: ingest (480 frames, in-place q|k|v source -> ring slots, SRC_ONCE) and gather (W = 16
              windows, 480 frames, store -> dense): `--iters` launches between one HIP-event pair, 5 series; GB/s counts bytes
              read plus bytes written, against a device copy of as many bytes timed the same way in the same process.
(c2) attention  one layer's decoder attention at W = 16 windows over the ring, hop 5 and hop 1: the tabled launch alone
              (`decoder_attn_fwd_frames`) beside gather + untabled launch (`kv_move_frames` of that layer, then
              `decoder_attn_fwd` on the dense rows), alternating; the launches walk round the six layers of the store, as the
              decoder does, so that a layer is not re-read from cache by the next launch.  us per launch; GB/s of the bytes
              NAMED (2 * W * T * P * D * 2: what the decoder reads) and of the bytes DISTINCT (the frames the 16 windows share,
              once), for both arms.
(d) live      hop 1 / 5 / 30 with encode_chunk = hop on a warm ring: ms on the host clock from `push(hop frames)` to the
              logits on the host (push returns them), median / min / max over `--live` pushes, for `gather="copy"` and "table".

Nothing is asserted but that the arms of (a) and (b) give the same number of windows, and that "store" and "table" give the same
bits.

usage: python tools/bench_stream.py [--frames 900] [--repeats 5] [--iters 20] [--live 30] [--hops 30,15,5,1] [--out PATH]
"""
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

ARCH, T, BATCH, LAYERS = "ViT-B/16", 30, 16, [6, 7, 8, 9, 10, 11]


def spread(xs, nd=3):
    return {"median": round(statistics.median(xs), nd), "min": round(min(xs), nd), "max": round(max(xs), nd)}


def build(device):
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    cfg = Detector.get_default_config()
    cfg.architecture, cfg.out_dim, cfg.losses = ARCH, [2], ["auc_roc"]
    cfg.decode_mode, cfg.decode_indices = "index", list(LAYERS)
    det = Detector(cfg, T, None, precision="bf16")
    det.load_state_dict(random_state_dict(cfg, T, seed=0))
    return det.to(device).eval()


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def windows_leg(det, crops, hops, repeats):
    from dfd_clip_amd.stream import StreamingVerdict, window_table
    F = crops.shape[0]
    ones = torch.ones(BATCH, T, dtype=torch.bool, device=crops.device)

    def by_predict(hop):
        table = window_table(0, F, T, hop).to(crops.device)
        rows = []
        with torch.no_grad():
            for i in range(0, table.shape[0], BATCH):
                x = crops[table[i:i + BATCH]]
                rows.append(det.predict(x, ones[:x.shape[0]])[0][0].detach().to("cpu"))
        return torch.cat(rows)

    def by_store(hop, gather="copy"):
        sv = StreamingVerdict(det, hop, encode_chunk=BATCH * T, batch_size=BATCH, gather=gather)
        sv.push(crops)
        sv.flush()
        return sv.result(with_logits=True)[2]

    out = {}
    for hop in hops:
        arms = {"predict": by_predict, "store": by_store, "table": lambda h: by_store(h, "table")}
        first = {n: timed(lambda: fn(hop)) for n, fn in arms.items()}
        W = first["predict"][1].shape[0]
        assert first["store"][1].shape[0] == W and torch.equal(first["store"][1], first["table"][1])
        gap = (first["predict"][1].double() - first["store"][1].double()).abs().max().item()
        ms, peak = {n: [] for n in arms}, {n: 0 for n in arms}
        for _ in range(repeats):
            for n, fn in arms.items():
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                ms[n].append(timed(lambda: fn(hop))[0])
                peak[n] = max(peak[n], torch.cuda.max_memory_allocated() - base)
                print(f"  hop {hop} {n}: {ms[n][-1]:.1f} ms", file=sys.stderr, flush=True)
        tower = {"predict": W * T, "store": (W - 1) * hop + T, "table": (W - 1) * hop + T}
        leg = {"windows": W, "warm_ms": {n: round(first[n][0], 1) for n in arms}, "max_logit_gap_between_arms": gap,
               "table_bits_equal_store": True}
        for n in arms:
            leg[n] = {"ms_per_video": spread(ms[n], 2), "series_ms": [round(t, 2) for t in ms[n]],
                      "windows_per_s": spread([W * 1e3 / t for t in ms[n]], 1),
                      "tower_frames": tower[n], "tower_frames_per_s": spread([tower[n] * 1e3 / t for t in ms[n]], 0),
                      "peak_allocated_mb_above_start": round(peak[n] / 2**20, 1)}
        leg["store_over_predict"] = round(statistics.median(ms["store"]) / statistics.median(ms["predict"]), 4)
        leg["table_over_predict"] = round(statistics.median(ms["table"]) / statistics.median(ms["predict"]), 4)
        leg["table_over_store"] = round(statistics.median(ms["table"]) / statistics.median(ms["store"]), 4)
        out[f"hop_{hop}"] = leg
    return out


def harness_leg(det, F, repeats, device):
    from dfd_clip_amd import align as AL
    from dfd_clip_amd.harness import infer_raw_video
    k = np.arange(68, dtype=np.float64)
    ref = 127.5 + 95.0 * np.sqrt((k + 1) / 68.0)[:, None] * np.stack([np.cos(2.399963 * k), np.sin(2.399963 * k)], 1)
    lm = ref[None] + np.random.default_rng(3).normal(0, 0.5, (F, 68, 2))
    aligner = AL.FaceAligner(ref, canvas=256, crop=224, border=0)
    frames = torch.randint(0, 256, (F, 256, 256, 3), dtype=torch.uint8, device=device, generator=torch.Generator(device=device).manual_seed(5))
    arms = {"hop_none": lambda: infer_raw_video(det, frames, lm, aligner, batch_size=BATCH, with_logits=True)[2],
            "hop_30": lambda: infer_raw_video(det, frames, lm, aligner, batch_size=BATCH, with_logits=True, hop=T)[2],
            "hop_30_table": lambda: infer_raw_video(det, frames, lm, aligner, batch_size=BATCH, with_logits=True, hop=T, gather="table")[2]}
    first = {n: timed(fn) for n, fn in arms.items()}
    assert first["hop_none"][1].shape == first["hop_30"][1].shape and torch.equal(first["hop_30"][1], first["hop_30_table"][1])
    ms = {n: [] for n in arms}
    for _ in range(repeats):
        for n, fn in arms.items():
            ms[n].append(timed(fn)[0])
            print(f"  infer_raw_video {n}: {ms[n][-1]:.1f} ms", file=sys.stderr, flush=True)
    out = {"frames": F, "windows": int(first["hop_none"][1].shape[0]), "bit_identical_logits": bool(torch.equal(first["hop_none"][1], first["hop_30"][1]))}
    for n in arms:
        out[n] = {"ms_per_video": spread(ms[n], 2), "series_ms": [round(t, 2) for t in ms[n]]}
    out["hop_30_over_hop_none"] = round(statistics.median(ms["hop_30"]) / statistics.median(ms["hop_none"]), 4)
    out["hop_30_table_over_hop_none"] = round(statistics.median(ms["hop_30_table"]) / statistics.median(ms["hop_none"]), 4)
    out["hop_30_table_over_hop_30"] = round(statistics.median(ms["hop_30_table"]) / statistics.median(ms["hop_30"]), 4)
    return out


def kernel_leg(iters, repeats, device):
    from dfd_clip_amd import capi
    L, P, D, n = len(LAYERS), 196, 768, BATCH * T
    cap = n + T
    buf = torch.empty(L, n, P + 1, 3 * D, device=device, dtype=torch.bfloat16).normal_()
    k, v = buf[:, :, 1:, D:2 * D], buf[:, :, 1:, 2 * D:]
    sk, sv = (torch.empty(L, cap, P, D, device=device, dtype=torch.bfloat16).normal_() for _ in range(2))
    dk, dv = (torch.empty(L, n, P, D, device=device, dtype=torch.bfloat16) for _ in range(2))
    slots = torch.as_tensor([(cap - 7 + i) % cap for i in range(n)], dtype=torch.int32)           # a wrap
    wins = torch.as_tensor([(w * 5 + j) % cap for w in range(BATCH) for j in range(T)], dtype=torch.int32)  # hop 5: frames six times
    dslots, dwins = slots.to(device), wins.to(device)
    moved = 2 * 2 * L * n * P * D * 2  # K and V, read + written, bf16
    src = torch.empty(moved // 4, device=device, dtype=torch.bfloat16).normal_()
    dst = torch.empty_like(src)
    calls = {"ingest": lambda: capi.kv_move_frames(k, v, sk, sv, None, dslots, src_once=True, dst_host=slots),
             "gather": lambda: capi.kv_move_frames(sk, sv, dk, dv, dwins, None, src_host=wins),
             "copy": lambda: dst.copy_(src)}

    def series(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / iters

    for n_, fn in calls.items():
        for _ in range(3):
            fn()
        if n_ != "copy":
            assert capi.kv_move_last_path() == capi.KVFRAMES_VEC16
    torch.cuda.synchronize()
    us = {n_: [] for n_ in calls}
    for _ in range(repeats):
        for n_, fn in calls.items():
            us[n_].append(series(fn))
    out = {"frames": n, "layers": L, "rows_per_tensor": L * n * P, "row_bytes": D * 2, "bytes_moved": moved}
    for n_ in calls:
        out[n_] = {"us": spread(us[n_], 2), "gbs": round(moved / statistics.median(us[n_]) / 1e3, 1)}
    for n_ in ("ingest", "gather"):
        out[f"{n_}_over_copy"] = round(statistics.median(us[n_]) / statistics.median(us["copy"]), 3)
    return out


def attention_leg(iters, repeats, device):
    """(c2): one layer's tabled launch beside gather + untabled launch, W = 16 windows, walking round the store's layers"""
    from dfd_clip_amd import capi
    L, P, D, H, W = len(LAYERS), 196, 768, 12, BATCH
    S, cap = T * P, BATCH * T + T
    sk, sv = (torch.empty(L, cap, P, D, device=device, dtype=torch.bfloat16).normal_() for _ in range(2))
    dk, dv = (torch.empty(L, W * T, P, D, device=device, dtype=torch.bfloat16) for _ in range(2))
    q = torch.randn(W, 2 * D, device=device)
    pos = torch.randn(T, D, device=device) * 0.02
    m = torch.ones(W, T, dtype=torch.uint8, device=device)
    splits = max(1, min(S // 64, max(1, 768 // W)))  # Decoder._splits
    ws = torch.empty(capi.decoder_attn_workspace_bytes(W, H, 64, splits) // 4, device=device)
    mix, stats = torch.empty(W, D, device=device), torch.empty(W, H, 2, device=device)
    out = {"windows": W, "layers_walked": L, "splits": splits, "named_bytes": 2 * W * T * P * D * 2}
    for hop in (5, 1):
        wins = torch.as_tensor([(cap - 11 + w * hop + j) % cap for w in range(W) for j in range(T)], dtype=torch.int32)  # a wrap
        dwins = wins.to(device)
        distinct = len(set(wins.tolist()))
        layer = [0]

        def tabled():
            i = layer[0] = (layer[0] + 1) % L
            capi.decoder_attn_fwd_frames(q, sk[i], sv[i], dwins, m, mix, stats, ws, splits, W, T, P, H, pos=pos, table_host=wins)

        def gathered():
            i = layer[0] = (layer[0] + 1) % L
            capi.kv_move_frames(sk[i:i + 1], sv[i:i + 1], dk[i:i + 1], dv[i:i + 1], dwins, None, src_host=wins)
            capi.decoder_attn_fwd(q, dk[i], dv[i], m, mix, stats, ws, splits, W, T, P, H, pos=pos)

        def untabled_alone():
            i = layer[0] = (layer[0] + 1) % L
            capi.decoder_attn_fwd(q, dk[i], dv[i], m, mix, stats, ws, splits, W, T, P, H, pos=pos)

        calls = {"table": tabled, "gather_plus_untabled": gathered, "untabled_alone": untabled_alone}

        def series(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e3 / iters

        for fn in calls.values():
            for _ in range(L):
                fn()
        gathered()
        ref = mix.clone()
        layer[0] -= 1  # the same layer again
        tabled()
        assert torch.isfinite(mix).all() and torch.equal(ref, mix)  # (synchronises)
        us = {n: [] for n in calls}
        for _ in range(repeats):
            for n, fn in calls.items():
                us[n].append(series(fn))
        named, dist = out["named_bytes"], 2 * distinct * P * D * 2
        leg = {"distinct_frames": distinct, "named_frames": W * T, "distinct_bytes": dist}
        for n in calls:
            med = statistics.median(us[n])
            leg[n] = {"us": spread(us[n], 2), "named_gbs": round(named / med / 1e3, 1), "distinct_gbs": round(dist / med / 1e3, 1)}
        leg["table_over_gather_plus_untabled"] = round(statistics.median(us["table"]) / statistics.median(us["gather_plus_untabled"]), 4)
        leg["table_over_untabled_alone"] = round(statistics.median(us["table"]) / statistics.median(us["untabled_alone"]), 4)
        out[f"hop_{hop}"] = leg
    return out


def live_leg(det, crops, pushes):
    from dfd_clip_amd.stream import StreamingVerdict
    out = {}
    for hop in (1, 5, 30):
        leg = {}
        svs = {g: StreamingVerdict(det, hop, gather=g) for g in ("copy", "table")}
        at = 0
        for _ in range(T // hop + 4):  # fill the rings and warm every shape: from here each push completes one window
            for sv in svs.values():
                sv.push(crops[at:at + hop])
            at += hop
        ms = {g: [] for g in svs}
        for _ in range(pushes):
            if at + hop > crops.shape[0]:
                at = 0  # (the content of a frame does not change its cost)
            for g, sv in svs.items():  # alternating
                t, got = timed(lambda: sv.push(crops[at:at + hop]))
                assert len(got) == 1
                ms[g].append(t)
            at += hop
        for g in svs:
            leg[g] = {"ms_push_to_verdict": spread(ms[g], 3)}
        leg.update(pushes=pushes, ring_frames=svs["copy"].store.capacity,
                   table_over_copy=round(statistics.median(ms["table"]) / statistics.median(ms["copy"]), 4))
        out[f"hop_{hop}"] = leg
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=900)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--live", type=int, default=30)
    ap.add_argument("--hops", default="30,15,5,1")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stream needs a GPU: a time taken anywhere else says nothing")
    from dfd_clip_amd import capi
    capi.load_library()
    device = torch.device("cuda", 0)
    det = build(device)
    crops = torch.randint(0, 256, (args.frames, 3, 224, 224), dtype=torch.uint8, device=device,
                          generator=torch.Generator(device=device).manual_seed(1234))
    out = {"tool": "bench_stream", "arch": ARCH, "dtype": "bf16", "T": T, "frames": args.frames, "batch": BATCH, "layers": LAYERS,
           "encode_chunk": BATCH * T, "repeats": args.repeats, "iters": args.iters}
    out["windows"] = windows_leg(det, crops, [int(h) for h in args.hops.split(",")], args.repeats)
    out["harness"] = harness_leg(det, args.frames, args.repeats, device)
    out["kernel"] = kernel_leg(args.iters, args.repeats, device)
    out["attention"] = attention_leg(5 * args.iters, args.repeats, device)  # (a launch is ~0.1 ms: five times the launches per series)
    out["live"] = live_leg(det, crops, args.live)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
