#!/usr/bin/env python3
"""Lab: the c_fc -> c_proj pair alone, fragment-blocked `u` against row-major `u` on the same kernel
(`capi.gemm_pair_set_variant(1)`), at the encoder's shapes.  Bitwise comparison first, then interleaved timed rounds
(device events around ITERS launches of one GEMM; both layouts in every round, so drift hits them alike)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from dfd_clip_amd import blocked, capi  # noqa: E402

ITERS, ROUNDS = 20, 5
capi.load_library()


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(3):
        fn()
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / ITERS


for name, M, D, H, epi in (("ViT-B/16", 480 * 197, 768, 3072, capi.EPI_BIAS_QUICKGELU), ("ViT-L/14", 240 * 257, 1024, 4096, capi.EPI_BIAS_QUICKGELU),
                           ("DINOv2 ViT-B/14", 240 * 257, 768, 3072, capi.EPI_BIAS_GELU)):
    g = torch.Generator(device="cuda").manual_seed(M)
    Mp = blocked.padded_rows(M)
    h = torch.randn(M, D, device="cuda", generator=g).to(torch.bfloat16)
    w_fc = (torch.randn(H, D, device="cuda", generator=g) * D ** -0.5).to(torch.bfloat16)
    b_fc = torch.randn(H, device="cuda", generator=g) * 0.1
    w_pr = (torch.randn(D, H, device="cuda", generator=g) * H ** -0.5).to(torch.bfloat16)
    b_pr = torch.randn(D, device="cuda", generator=g) * 0.1
    idx = blocked.fc_channel_perm(H, device="cuda")
    w_fc_b, b_fc_b = w_fc[idx].contiguous(), b_fc[idx].contiguous()
    u_r = torch.zeros(Mp, H, device="cuda", dtype=torch.bfloat16)
    u_b = torch.zeros(Mp, H, device="cuda", dtype=torch.bfloat16)
    d_r = torch.zeros(M, D, device="cuda", dtype=torch.bfloat16)
    d_b = torch.zeros(M, D, device="cuda", dtype=torch.bfloat16)
    sp = dict(spare_cus=32, spare_if_free=True)  # as the encoder launches c_proj in a forward-only pass

    def fc(blk):
        capi.gemm_pair_set_variant(0 if blk else 1)
        capi.gemm(h, w_fc_b if blk else w_fc, u_b if blk else u_r, b_fc_b if blk else b_fc, epi, m=M, stream_out=True, c_blocked=True)

    def proj(blk, **kw):
        capi.gemm_pair_set_variant(0 if blk else 1)
        capi.gemm(u_b if blk else u_r, w_pr, d_b if blk else d_r, b_pr, capi.EPI_BIAS, m=M, stream_out=True, a_blocked=True, **kw)

    fc(False), fc(True), proj(False), proj(True)
    torch.cuda.synchronize()
    print(f"{name}: M {M} D {D} H {H}: unpack(u blocked) == u row-major: {bool(torch.equal(blocked.unpack(u_b, M), u_r[:M]))}; "
          f"c_proj outputs equal: {bool(torch.equal(d_b, d_r))}; finite: {bool(torch.isfinite(d_b.float()).all())}", flush=True)
    for r in range(ROUNDS):
        t = [timed(lambda: fc(False)), timed(lambda: fc(True)), timed(lambda: proj(False)), timed(lambda: proj(True)),
             timed(lambda: proj(False, **sp)), timed(lambda: proj(True, **sp))]
        print(f"  round {r}: c_fc row-major {t[0]:.4f} ms, blocked {t[1]:.4f} ms | c_proj row-major {t[2]:.4f} ms, blocked {t[3]:.4f} ms | "
              f"c_proj (32 spare CUs if free) row-major {t[4]:.4f} ms, blocked {t[5]:.4f} ms", flush=True)
    capi.gemm_pair_set_variant(0)
    del h, u_r, u_b, d_r, d_b
