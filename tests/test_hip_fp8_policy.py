"""The fp8 precision policy on the GPU: the erf-GELU epilogue of `dfd_gemm_fp8` (DINOv2's fc1) against fp64 on the same e4m3
operands; then `set_fp8_policy` end to end — which projections run on e4m3 is exactly what the policy says, layer by
layer, bit for bit against the "all" and the bf16 runs; graph replay, K/V in place and exported, small chunks; the DINOv2
foundation in fp8; and the ViT-L/14 acceptance numbers per preset."""
import copy

import numpy as np
import pytest
import torch

from dfd_clip_amd.encoder import FP8_CONTRACT_POLICY, FP8_PRESETS
from tests.test_hip_fp8 import _auroc, _make, _spearman, assert_close, e4m3

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from dfd_clip_amd import capi as c
    c.load_library()
    return c


# ---- kernel level: the erf-GELU epilogue on e4m3 operands ------------------------------------------------------------

def gelu_f64(u):
    return u * 0.5 * (1 + torch.erf(u / 2 ** 0.5))


def _gelu_operands(M, N, K):
    """The operands of tests/test_hip_fp8.py::test_gemm_fp8_epilogues (same seed, same draws)."""
    g = torch.Generator().manual_seed(N * 3 + K)
    a8, af = e4m3(torch.randn(M, K, generator=g) * 4.0)
    w8, wf = e4m3(torch.randn(N, K, generator=g) * 8.0)
    cs = (torch.rand(N, generator=g) * 0.02 + 0.001).cuda()
    bias = (torch.randn(N, generator=g) * 0.1).cuda()
    return a8, af, w8, wf, cs, bias


def _gelu_runs(capi, a8, w8, cs, bias, M, N, out_scale):
    c = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    capi.gemm_fp8(a8, w8, c, cs, bias, capi.EPI_BIAS_GELU)
    c8 = torch.full((M, N), 0x7f, device="cuda", dtype=torch.uint8)
    capi.gemm_fp8(a8, w8, c8, cs, bias, capi.EPI_BIAS_GELU, out_inv_scale=1.0 / out_scale)
    return c, c8


@pytest.mark.parametrize("M,N,K", [(1024 + 256 * 7 + 77, 768, 768), (1024 + 256 * 7 + 77, 3072, 768), (1024 + 256 * 7 + 77, 3072, 1024),
                                   (1024 + 256 * 7 + 77, 1024, 4096), (1024 + 96, 3072, 768)])  # last: fewer tiles than CUs, ragged panel
def test_gemm_fp8_gelu_epilogue(capi, M, N, K):
    a8, af, w8, wf, cs, bias = _gelu_operands(M, N, K)
    ref = (af @ wf.T) * cs.double() + bias.double()
    AT = 2.0 ** -11 * (af.abs() @ wf.abs().T) * cs.double() + 1e-4  # test_gemm_fp8_epilogues' bound on the accumulator
    want = gelu_f64(ref)
    out_scale = float(want.abs().max()) / 448.0
    c, c8 = _gelu_runs(capi, a8, w8, cs, bias, M, N, out_scale)
    assert_close(c, want, 1.13 * AT, 2 ** -8, "gelu")  # max |gelu'| = 1.129
    dec = c8.view(torch.float8_e4m3fn).double() * out_scale
    assert_close(dec, want, 1.13 * AT + 2.0 ** -10 * out_scale, 2 ** -4, "gelu -> e4m3")
    # the ping-pong kernel and the persistent kernel behind it serve every shape here: the same bits
    capi.gemm_set_variant(1)
    try:
        p, p8 = _gelu_runs(capi, a8, w8, cs, bias, M, N, out_scale)
    finally:
        capi.gemm_set_variant(0)
    assert torch.equal(c, p) and torch.equal(c8, p8)


# ---- end to end on vitb16_cfg1 (B2 x T8, 3,152 rows, 12 layers, taps 6..11) -----------------------------------------------

def _qkv(det, xf):
    """q / k / v of every layer from the reference API (copies: the views alias the workspace)."""
    with torch.no_grad():
        return [{n: d[n].clone() for n in ("q", "k", "v")} for d in det.encoder(xf, with_q=True)]


def _logits(det, x, m):
    with torch.no_grad():
        return det.predict(x, m)[0][0].float().clone()


def _same(a, b):
    return all(torch.equal(a[n], b[n]) for n in ("q", "k", "v"))


@pytest.fixture(scope="module")
def b16():
    """The detectors on `vitb16_cfg1`, each calibrated on the batch it runs, and the "all" / bf16 results shared by the tests."""
    from tests.cases import build_case
    case = build_case("vitb16_cfg1")
    x, m = case["x"].cuda(), case["m"].cuda()
    xf = x.flatten(0, 1).contiguous()
    plain, det, det16 = _make(case, "fp8"), _make(case, "fp8"), _make(case, "bf16")
    plain.calibrate_fp8(x)
    det.calibrate_fp8(x)
    det.set_fp8_policy("all")
    out = dict(case=case, x=x, m=m, xf=xf, plain=plain, det=det, det16=det16)
    out["all"] = (_logits(det, x, m), _qkv(det, xf))
    out["bf16"] = (_logits(det16, x, m), _qkv(det16, xf))
    return out


def test_all_is_the_default_and_a_reset_returns_its_bits(b16):
    x, m, xf, det = b16["x"], b16["m"], b16["xf"], b16["det"]
    l_all, q_all = b16["all"]
    assert torch.equal(_logits(b16["plain"], x, m), l_all)
    for a, b in zip(_qkv(b16["plain"], xf), q_all):
        assert _same(a, b)
    det.set_fp8_policy("proj-bf16")
    assert not torch.equal(_logits(det, x, m), l_all), "the policy changed nothing"
    det.set_fp8_policy("all")
    assert torch.equal(_logits(det, x, m), l_all), "invalidation: back to 'all' must give the same bits"
    assert torch.equal(det.encoder.fp8_calibration(), b16["plain"].encoder.fp8_calibration())


def test_none_is_the_bf16_path(b16):
    x, m, xf, det = b16["x"], b16["m"], b16["xf"], b16["det"]
    det.set_fp8_policy("none")
    try:
        assert torch.equal(_logits(det, x, m), b16["bf16"][0])
        for a, b in zip(_qkv(det, xf), b16["bf16"][1]):
            assert _same(a, b)
    finally:
        det.set_fp8_policy("all")


def test_a_per_layer_change_starts_where_the_policy_says(b16):
    xf, det = b16["xf"], b16["det"]
    det.set_fp8_policy([{} if l != 7 else {"proj": "bf16"} for l in range(12)])
    try:
        got = _qkv(det, xf)
    finally:
        det.set_fp8_policy("all")
    for l in range(8):  # layer 7's c_proj is the first kernel that differs: it feeds layer 8
        assert _same(got[l], b16["all"][1][l]), f"layer {l} changed"
    assert not any(torch.equal(got[8][n], b16["all"][1][8][n]) for n in ("q", "k", "v")), "layer 8 did not change"


@pytest.mark.parametrize("layer,tapped", [(6, "detector"), (0, None)])  # ln_1 behind two deferred residuals / behind ln_pre
def test_kv_bf16_splits_one_projection(b16, layer, tapped):
    """Q third on e4m3 from `h8`, K and V thirds on bf16 from `h`, both written by ONE dual-output LayerNorm pass."""
    xf, det = b16["xf"], b16["det"]
    taps = b16["case"]["layer_indices"] if tapped else None

    def run(qkv):
        det.encoder.set_fp8_policy([{} if l != layer else {"qkv": qkv} for l in range(12)], tapped=taps)
        assert det.encoder.fp8_policy()[layer]["qkv"] == qkv
        return _qkv(det, xf)
    try:
        split, whole = run("kv-bf16"), run("bf16")
    finally:
        det.set_fp8_policy("all")
    assert torch.equal(split[layer]["q"], b16["all"][1][layer]["q"]), "the Q third must be the e4m3 projection's"
    assert torch.equal(split[layer]["k"], whole[layer]["k"]) and torch.equal(split[layer]["v"], whole[layer]["v"])
    assert not torch.equal(split[layer]["k"], b16["all"][1][layer]["k"])
    for l in range(layer):
        assert _same(split[l], b16["all"][1][l])


@pytest.mark.parametrize("preset", FP8_PRESETS)
def test_presets_graph_replay_and_kv_in_place(b16, preset):
    """The policy only changes which kernels `_block` enqueues: the pipelined encoder replayed as one HIP graph gives the
    eager launches' logits bit for bit, with the K/V read in place and exported."""
    x, m, det = b16["x"], b16["m"], b16["det"]
    det.set_fp8_policy(preset)
    try:
        for in_place in (True, False):
            det.kv_in_place = in_place
            want = _logits(det, x, m)
            assert torch.isfinite(want).all()
            g = copy.deepcopy(det)
            assert g.encoder.fp8_policy() == det.encoder.fp8_policy() and g.encoder.fp8_calibration() is not None
            g.pipeline_encoder, g.inputs_ready, g.static_graphs = True, True, True
            torch.cuda.synchronize()
            for i in range(4):  # two K/V sets alternate: each (input, set) pair is captured at its second sighting
                assert torch.equal(_logits(g, x, m), want), f"{preset} in_place={in_place} pass {i}"
            assert g._enc_graphs_failed is None
            assert (len(g._enc_graphs) >= 1) == in_place, "the encoder pass is replayed as a graph exactly when K/V stay in place"
            del g
    finally:
        det.kv_in_place = True
        det.set_fp8_policy("all")


def test_small_chunk_under_a_policy_runs_bf16(b16):
    x, det = b16["x"], b16["det"]
    det.set_fp8_policy("kv+proj-bf16")
    try:
        with torch.no_grad():
            kv8 = det.encoder(x[0, :4].contiguous())    # 4 frames x 197 rows < 1,024
            kv16 = b16["det16"].encoder(x[0, :4].contiguous())
            for a, b in zip(kv8, kv16):
                assert torch.equal(a["k"], b["k"]) and torch.equal(a["v"], b["v"])
    finally:
        det.set_fp8_policy("all")


# ---- the DINOv2 foundation in fp8 --------------------------------------------------------------------------------------

def _dino(arch, B, T, taps, precision, seed=0):
    from dfd_clip_amd.detector import Detector
    from dfd_clip_amd.weights import random_state_dict
    from tests.dinov2_cases import make_config
    cfg = make_config(arch, decode_mode="index", decode_indices=taps)
    sd = random_state_dict(cfg, T, seed=seed)
    g = torch.Generator().manual_seed(5)
    for k in sd:
        if k.endswith("ls1.gamma") or k.endswith("ls2.gamma"):  # not 1: the LayerScale fold must come BEFORE the quantisation
            sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
    dets = []
    for p in precision:
        det = Detector(cfg, T, None, precision=p)
        det.load_state_dict(sd)
        dets.append(det.cuda().eval())
    return dets


def test_dinov2_fp8_close_to_bf16_and_none_is_bf16():
    B, T = 32, 8  # 256 frames x 5 tokens = 1,280 rows
    d16, d8 = _dino("dino_w768", B, T, [0, 1], ("bf16", "fp8"))
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(B, T, 3, 28, 28, device="cuda", generator=g)
    m = torch.ones(B, T, dtype=torch.bool, device="cuda")
    d8.calibrate_fp8(x)
    with torch.no_grad():
        l16, l8 = _logits(d16, x, m), _logits(d8, x, m)
        k16, _ = d16.encoder.extract_kv(x.flatten(0, 1), [0, 1], T, d16.decoder.temporal_pos())
        k8, _ = d8.encoder.extract_kv(x.flatten(0, 1), [0, 1], T, d8.decoder.temporal_pos())
    rel = ((k8.float() - k16.float()).norm() / k16.float().norm()).item()
    dl = (l8 - l16).abs().max().item()
    print(f"dino_w768: fp8 vs bf16 exported K relative error {rel:.3e}; max|dlogit| {dl:.3e}")
    assert torch.isfinite(l8).all()
    assert 0 < rel < 0.08, "exported keys drift more than e4m3 quantisation explains (or the fp8 path did not run)"
    d8.set_fp8_policy("none")
    assert torch.equal(_logits(d8, x, m), l16)
    with torch.no_grad():
        kn, _ = d8.encoder.extract_kv(x.flatten(0, 1), [0, 1], T, d8.decoder.temporal_pos())
    assert torch.equal(kn, k16)


def test_dinov2_vitb14_fp8_properties():
    """The real geometry (width 768, 257 tokens per frame), 4 frames = 1,028 rows: finite, and clips independent."""
    B, T = 2, 2
    (d8,) = _dino("dinov2_vitb14", B, T, [6, 7, 8, 9, 10, 11], ("fp8",))
    g = torch.Generator(device="cuda").manual_seed(4)
    x = torch.randn(B, T, 3, 224, 224, device="cuda", generator=g)
    m = torch.ones(B, T, dtype=torch.bool, device="cuda")
    d8.calibrate_fp8(x)
    base = _logits(d8, x, m)
    assert torch.isfinite(base).all()
    assert torch.equal(_logits(d8, x.flip(0).contiguous(), m), base.flip(0)), "clips are not independent"


# ---- ViT-L/14 acceptance per preset -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def l14():
    """Inputs, labels and calibration subset of tests/test_hip_fp8.py::test_fp8_auroc_parity_vitl14; the bf16 outputs once."""
    from tests.cases import build_case
    case = build_case("vitl14")
    T, res, n_clips = case["T"], case["res"], 256
    rng = np.random.default_rng(4321)
    x = torch.from_numpy(rng.standard_normal((n_clips, T, 3, res, res), dtype=np.float32))
    m = torch.ones(n_clips, T, dtype=torch.bool)
    m[3::7, T - 1:] = False
    y = np.random.default_rng(7).integers(0, 2, n_clips)

    def outputs(det):
        p, lg = [], []
        with torch.no_grad():
            for i in range(0, n_clips, 32):
                logits, _ = det.predict(x[i:i + 32].cuda(), m[i:i + 32].cuda())
                p.append(logits[0].softmax(dim=-1)[:, 1].cpu())
                lg.append(logits[0].float().cpu())
        return torch.cat(p).numpy(), torch.cat(lg)

    det16 = _make(case, "bf16")
    ref = outputs(det16)
    del det16
    torch.cuda.empty_cache()
    det8 = _make(case, "fp8")
    det8.calibrate_fp8(x[:16].cuda())
    return dict(y=y, ref=ref, det8=det8, outputs=outputs, auroc16=_auroc(y, ref[0]))


def _l14_figures(l14, preset):
    l14["det8"].set_fp8_policy(preset)
    p, lg = l14["outputs"](l14["det8"])
    a = _auroc(l14["y"], p)
    d = (lg - l14["ref"][1]).abs()
    fig = dict(auroc=a, dauroc=abs(a - l14["auroc16"]), spearman=_spearman(l14["ref"][0], p), dmax=d.max().item(), dmean=d.mean().item())
    print(f"ViT-L/14 {preset}: AUROC bf16 {l14['auroc16']:.4f} fp8 {a:.4f} |dAUROC| {fig['dauroc']:.2e}  spearman {fig['spearman']:.5f}  "
          f"|dlogit| max {fig['dmax']:.3e} mean {fig['dmean']:.3e}")
    return fig


@pytest.mark.parametrize("preset", FP8_PRESETS)
def test_vitl14_acceptance_per_preset(l14, preset):
    fig = _l14_figures(l14, preset)
    assert fig["spearman"] > 0.99   # the bars of tests/test_hip_fp8.py (FP8_L14_SPEARMAN_BAR, FP8_L14_LOGIT_BAR)
    assert fig["dmax"] < 0.8
    if preset == "none":
        assert fig["dauroc"] == 0 and fig["dmax"] == 0


def test_vitl14_contract_policy_meets_1e_3(l14):
    """|dAUROC| <= 1e-3 against bf16 for the preset `encoder.FP8_CONTRACT_POLICY` names."""
    if FP8_CONTRACT_POLICY is None:
        pytest.skip("encoder.FP8_CONTRACT_POLICY is None: no preset other than 'none' is recorded as meeting the contract")
    assert FP8_CONTRACT_POLICY in FP8_PRESETS and FP8_CONTRACT_POLICY != "none"
    assert _l14_figures(l14, FP8_CONTRACT_POLICY)["dauroc"] <= 1e-3
