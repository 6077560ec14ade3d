"""dfd_stream_policy_set (include/dfdclip_hooks.h): a family's bit changes the cache policy of its read-once loads and
write-once stores and nothing else.  Every kernel that has a non-temporal form runs through the C ABI with the mask at 0
and with its family's bit set, on the same inputs, and every output must be equal bit for bit.  Shapes are the smallest
that reach each kernel's tails, both K/V layouts, and every instantiation the launchers choose between."""
import copy

import numpy as np
import pytest
import torch

from tests.cases import build_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    assert torch.cuda.is_available()
    return c


def rnd(*shape, seed=0, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32) * scale)


def off_and_on(capi, bit, run):
    """run() -> dict of output tensors, once with the mask at 0 and once with `bit`; the mask is put back."""
    old = capi.stream_policy_get()
    try:
        capi.stream_policy_set(0)
        plain = {k: v.clone() for k, v in run().items()}
        capi.stream_policy_set(bit)
        assert capi.stream_policy_get() == bit
        hinted = {k: v.clone() for k, v in run().items()}
        torch.cuda.synchronize()
    finally:
        capi.stream_policy_set(old)
    assert plain.keys() == hinted.keys() and plain
    for name in plain:
        a, b = plain[name], hinted[name]
        if a.element_size() == 1:  # e4m3 bytes
            a, b = a.view(torch.uint8), b.view(torch.uint8)
        assert torch.isfinite(a.float()).all(), name
        assert torch.equal(a, b), f"{name}: differs with stream policy bit {bit}"


# ---- decoder attention: K / V loads, forward and backward ---------------------------------------------------------

@pytest.mark.parametrize("inplace", [False, True], ids=["dense", "inplace"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_decoder_attention_forward_and_backward(capi, dtype, inplace):
    """B 2, T 3, 5 patches, 2 heads (D = 128), one frame masked.  Dense K / V, and K / V read in place out of a
    [frames, 1 + patches, 3 D] activation (row stride 3 D, CLS row skipped) with the positional embedding added on the fly."""
    B, T, P, heads = 2, 3, 5, 2
    D, S = heads * 64, T * P
    q = rnd(B, 2 * D, seed=3).cuda()
    dmix = rnd(B, D, seed=4).cuda()
    m = torch.ones(B, T, dtype=torch.uint8)
    m[1, 2] = 0
    m = m.cuda()
    if inplace:
        qkv = rnd(B * T, P + 1, 3 * D, seed=1).to(dtype).cuda()
        k, v = qkv[:, 1:, D:2 * D], qkv[:, 1:, 2 * D:]
        pos = rnd(T, D, seed=5, scale=0.1).cuda()
    else:
        k, v = rnd(B, S, D, seed=1).to(dtype).cuda(), rnd(B, S, D, seed=2).to(dtype).cuda()
        pos = None
    splits = 2
    ws = torch.empty(capi.decoder_attn_workspace_bytes(B, heads, 64, splits) // 4, device="cuda")
    ws2 = torch.empty(capi.decoder_attn_bwd_workspace_bytes(B, T, heads) // 4, device="cuda")

    def run():
        mix, mix_s, stats = torch.zeros(B, D, device="cuda"), torch.zeros(B, D, device="cuda"), torch.zeros(B, heads, 2, device="cuda")
        capi.decoder_attn_fwd(q, k, v, m, mix, stats, ws, splits, B, T, P, heads, mix_softmax=mix_s, pos=pos)
        dq, dpos = torch.zeros(B, 2 * D, device="cuda"), torch.zeros(T, D, device="cuda")
        dk, dv = torch.zeros(B, S, D, device="cuda"), torch.zeros(B, S, D, device="cuda")
        capi.decoder_attn_bwd(q, k, v, m, dmix, mix_s, stats, dq, dpos, ws2, B, T, P, heads, dk=dk, dv=dv, pos=pos)
        dk16, dv16 = torch.zeros(B, S, D, device="cuda", dtype=torch.bfloat16), torch.zeros(B, S, D, device="cuda", dtype=torch.bfloat16)
        dq2 = torch.zeros_like(dq)
        capi.decoder_attn_bwd(q, k, v, m, dmix, mix_s, stats, dq2, None, ws2, B, T, P, heads, dk=dk16, dv=dv16, pos=pos)
        return dict(mix=mix, mix_s=mix_s, stats=stats, dq=dq, dpos=dpos, dk=dk, dv=dv, dq2=dq2, dk16=dk16, dv16=dv16)
    off_and_on(capi, capi.STREAM_DECODER_KV, run)


# ---- decoder linears: weight loads, dW stores ----------------------------------------------------------------------

@pytest.mark.parametrize("N,K", [(7, 132), (101, 36), (5, 260)])
def test_linear_rows(capi, N, K):
    """3 rows; odd N (a ragged last workgroup of four output columns); K below one 256-column trip of a wave (some lanes
    load nothing) and one lane past it (a second trip for lane 0 alone)."""
    B = 3
    x, w, bias, y0 = rnd(B, K, seed=20).cuda(), rnd(N, K, seed=21, scale=K ** -0.5).cuda(), rnd(N, seed=22, scale=0.1).cuda(), rnd(B, N, seed=23).cuda()

    def run():
        out = {}
        for epi in (capi.EPI_BIAS, capi.EPI_BIAS_QUICKGELU, capi.EPI_BIAS_RESIDUAL):
            y = y0.clone()
            capi.linear_rows(x, w, bias, y, epi)
            out[f"y{epi}"] = y
        return out
    off_and_on(capi, capi.STREAM_DECODER_WEIGHTS, run)


@pytest.mark.parametrize("N,K", [(8, 33), (260, 7), (100, 132)])
def test_linear_rows_t(capi, N, K):
    """3 rows; K odd, below one 8-row step, and with a tail after whole steps; N below and past one 256-column workgroup."""
    B = 3
    x, wt, bias, y0 = rnd(B, K, seed=28).cuda(), rnd(K, N, seed=29, scale=K ** -0.5).cuda(), rnd(N, seed=30, scale=0.1).cuda(), rnd(B, N, seed=31).cuda()
    ws = torch.empty(capi.linear_rows_t_workspace_bytes(B, N, K) // 4, device="cuda")

    def run():
        out = {}
        for epi in (capi.EPI_BIAS, capi.EPI_BIAS_QUICKGELU, capi.EPI_BIAS_RESIDUAL):
            y = y0.clone()
            capi.linear_rows_t(x, wt, bias, y, ws, epi)
            out[f"y{epi}"] = y
        return out
    off_and_on(capi, capi.STREAM_DECODER_WEIGHTS, run)


@pytest.mark.parametrize("with_db", [True, False])
@pytest.mark.parametrize("N,K", [(7, 132), (101, 36), (9, 1028)])
def test_linear_rows_bwd_weight(capi, N, K, with_db):
    """3 rows; N no multiple of the 8 output rows of a workgroup; K below its 1,024-column trip and one thread past it."""
    B = 3
    x, dy = rnd(B, K, seed=5).cuda(), rnd(B, N, seed=7).cuda()

    def run():
        dw = torch.zeros(N, K, device="cuda")
        db = torch.zeros(N, device="cuda") if with_db else None
        capi.linear_rows_bwd_weight(dy, x, dw, db)
        return dict(dw=dw, db=db) if with_db else dict(dw=dw)
    off_and_on(capi, capi.STREAM_DECODER_WEIGHTS, run)


# ---- optimizer ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("adamw", [False, True], ids=["sgd", "adamw"])
def test_optimizer_step(capi, adamw):
    """Parameters of 1, 255, 257 and 4,099 elements (below, around and past a 256-thread trip and a 1,024-element block) and
    one 5 x 7 weight with its transposed mirror; the first step and a later one."""
    shapes = [((1,), False), ((255,), False), ((257,), False), ((4099,), False), ((5, 7), True)]
    n = len(shapes)
    p0 = [rnd(*s, seed=60 + i) for i, (s, _) in enumerate(shapes)]
    gr = [[rnd(*s, seed=70 + 10 * st + i).cuda() for i, (s, _) in enumerate(shapes)] for st in range(2)]

    def run():
        ps = [p.clone().cuda() for p in p0]
        gs = [g.clone() for g in gr[0]]
        ms = [torch.zeros_like(p) for p in ps]
        vs = [torch.zeros_like(p) for p in ps]
        mirs = [torch.zeros(s[1], s[0], device="cuda") if mir else None for s, mir in shapes]
        rows_, first = [], 0
        for i, (s, mir) in enumerate(shapes):
            r, c = (s[0], s[1]) if len(s) == 2 else (0, 0)
            rows_.append([ps[i].data_ptr(), gs[i].data_ptr(), ms[i].data_ptr(), mirs[i].data_ptr() if mir else 0, ps[i].numel(), r | (c << 32), first])
            first += capi.sgd_blocks(ps[i].numel(), r, c, mir)
        table = torch.tensor(rows_, dtype=torch.int64, device="cuda")
        second = torch.tensor([v.data_ptr() for v in vs], dtype=torch.int64, device="cuda")
        out = {}
        for st in range(2):
            for i in range(n):
                gs[i].copy_(gr[st][i])
            extra = capi.adamw_extra(0.9, 0.999, 1e-8, st + 1, second) if adamw else None
            capi.sgd_step(table, n, first, 0.01, 0.95, 0.01, st == 0, extra=extra)
            for i in range(n):
                out[f"p{i}@{st}"], out[f"m{i}@{st}"], out[f"v{i}@{st}"] = ps[i].clone(), ms[i].clone(), vs[i].clone()
            out[f"mirror@{st}"] = mirs[4].clone()
            assert torch.equal(mirs[4], ps[4].t()), "the mirror is the transposed parameter"
        return out
    off_and_on(capi, capi.STREAM_OPTIMIZER, run)


# ---- the encoder's row kernels -------------------------------------------------------------------------------------

def _ln_outputs(kind, rows, cols):
    if kind == "dual":
        return torch.zeros(rows, cols, device="cuda", dtype=torch.bfloat16), torch.zeros(rows, cols, device="cuda", dtype=torch.uint8)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "e4m3": torch.uint8}[kind]
    return torch.zeros(rows, cols, device="cuda", dtype=dt), None


@pytest.mark.parametrize("kind", ["bf16", "e4m3", "f32", "dual"])
@pytest.mark.parametrize("rows", [3, 257])
def test_layernorm_family(capi, rows, kind):
    """Width 768; 3 rows (a ragged last workgroup of four waves) and 257 (many workgroups and a ragged one).  layernorm,
    layernorm2 and add_layernorm with one and two pending deltas (bf16 and f32), `store_x` on and off, into bf16, e4m3, f32
    and the dual bf16 + e4m3 form.  Zero pending deltas is the plain layernorm."""
    cols = 768
    x0 = rnd(rows, cols, seed=40).cuda()
    ga, ba, gb, bb = rnd(cols, seed=41).cuda(), rnd(cols, seed=42, scale=0.1).cuda(), rnd(cols, seed=43).cuda(), rnd(cols, seed=44, scale=0.1).cuda()
    d1, d2 = rnd(rows, cols, seed=45, scale=0.5).cuda(), rnd(rows, cols, seed=46, scale=0.5).cuda()
    inv = 0.5

    def run():
        out = {}
        x = x0.clone()
        y, y8 = _ln_outputs(kind, rows, cols)
        if kind == "dual":
            capi.layernorm_dual(x, ga, ba, y, y8, inv)
        else:
            capi.layernorm(x, ga, ba, y, out_inv_scale=inv if kind == "e4m3" else 0.0)
        out["ln.y"], out["ln.y8"] = y, y8
        x = x0.clone()
        y, y8 = _ln_outputs(kind, rows, cols)
        if kind == "dual":
            capi.layernorm2_dual(x, ga, ba, gb, bb, y, y8, inv)
        else:
            capi.layernorm2(x, ga, ba, gb, bb, y, out_inv_scale=inv if kind == "e4m3" else 0.0)
        out["ln2.x"], out["ln2.y"], out["ln2.y8"] = x, y, y8
        for ddt in (torch.bfloat16, torch.float32):
            for two in (False, True):
                for store_x in (True, False):
                    x = x0.clone()
                    y, y8 = _ln_outputs(kind, rows, cols)
                    a, b = d1.to(ddt), (d2.to(ddt) if two else None)
                    if kind == "dual":
                        capi.add_layernorm_dual(x, a, gb, bb, y, y8, inv, delta2=b, store_x=store_x)
                    else:
                        capi.add_layernorm(x, a, gb, bb, y, delta2=b, store_x=store_x, out_inv_scale=inv if kind == "e4m3" else 0.0)
                    tag = f"aln.{ddt}.{two}.{store_x}"
                    out[tag + ".x"], out[tag + ".y"], out[tag + ".y8"] = x, y, y8
                    if not store_x:
                        assert torch.equal(x, x0), "store_x off leaves x alone"
        return {k: v for k, v in out.items() if v is not None}
    off_and_on(capi, capi.STREAM_ENCODER_ROWS, run)


@pytest.mark.parametrize("res,patch", [(32, 16), (96, 32)])
def test_patchify_strip(capi, res, patch):
    """The strip form (bf16 rows, no K padding): 3 frames, a 2 x 2 and a 3 x 3 grid."""
    frames = rnd(3, 3, res, res, seed=50).cuda()

    def run():
        out = torch.zeros(3 * (res // patch) ** 2, 3 * patch * patch, device="cuda", dtype=torch.bfloat16)
        capi.patchify(frames, out, res, patch)
        return dict(out=out)
    off_and_on(capi, capi.STREAM_ENCODER_ROWS, run)


# ---- a captured decoder train graph keeps the mask of its capture ---------------------------------------------------------

def test_decoder_train_graph_captured_with_the_mask_on(capi):
    """Two copies of one detector train on the same batches: one eagerly with the mask at 0, one with `static_graphs` and
    every bit set while its decoder graph is captured.  The mask goes back to 0 before the replays, which must still
    equal the eager run bit for bit: losses, gradients, parameters."""
    from dfd_clip_amd import decoder as dmod
    from dfd_clip_amd.detector import Detector
    case = build_case("small")
    det_e = Detector(case["cfg"], case["T"], None, precision="bf16")
    det_e.load_state_dict(case["sd"])
    det_e = det_e.to("cuda")
    det_g = copy.deepcopy(det_e)
    det_g.static_graphs = True
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    opt_e, opt_g = det_e.configure_optimizers(0.01), det_g.configure_optimizers(0.01)
    old = capi.stream_policy_get()
    try:
        for step in range(4):
            res = []
            for det, opt, mask in ((det_e, opt_e, 0), (det_g, opt_g, capi.STREAM_ALL if step < 2 else 0)):
                capi.stream_policy_set(mask)
                det.train()
                opt.zero_grad(set_to_none=True)
                losses, logits, other = det(x, [y], m, train=True, single_task=0)
                (losses[0].mean() + sum(other.values())).backward()
                res.append((losses[0].detach().clone(), {n: p.grad.detach().clone() for n, p in det.named_parameters() if p.grad is not None}))
                opt.step()
                torch.cuda.synchronize()
            assert torch.equal(res[0][0], res[1][0]), f"step {step}: losses differ"
            for n in res[0][1]:
                assert torch.equal(res[0][1][n], res[1][1][n]), f"step {step}: gradient of {n} differs"
    finally:
        capi.stream_policy_set(old)
    assert (dmod._GRAPHS.get(det_g.decoder) or {}) and not det_g.decoder._graphs_failed, "the decoder graph was captured and replayed"
    for (n, pe), (_, pg) in zip(det_e.named_parameters(), det_g.named_parameters()):
        assert torch.equal(pe, pg), n
