"""CPU pins of adapter pre-training (`CompInvEncoder`): the f64 restatement of the pair loss, run on the CPU oracle's
encoder / adapter, reproduces what the reference's own class computed (tests/golden/compinv_*.npz, written by
tools/gen_golden_compinv.py); the model's config, state_dict schema and host-side argument checks."""
import numpy as np
import pytest
import torch

from dfd_clip_amd import capi, default_compinv_config
from oracle import ref_cpu
from tests.compinv_cases import CASES, build_case, load_golden, loss_f64

TOL = 2e-5


def oracle_adapted(case, params=None):
    """Adapted K/V per tapped layer ({"k", "v"} [B, T, P, h, d]) from the CPU oracle; `params` overrides adapter tensors."""
    sd = dict(case["sd"])
    if params:
        sd.update(params)
    B, T = case["B"], case["T"]
    with torch.no_grad():
        enc = ref_cpu.encoder_forward(sd, case["x"].flatten(0, 1), case["heads"], case["patch"])
    kvs = [{s: enc[l][s][:, 1:].unflatten(0, (B, T)) for s in ("k", "v")} for l in case["layer_indices"]]
    return ref_cpu.adapter_forward(sd, kvs, "768-x-768")


@pytest.mark.parametrize("name", list(CASES))
def test_f64_restatement_reproduces_reference_losses_and_gradients(name):
    case = build_case(name)
    g = load_golden(name)
    params = {k: v.clone().requires_grad_(True) for k, v in case["sd"].items() if k.startswith("adapter.")}
    recon, match = loss_f64(oracle_adapted(case, params), len(case["layer_indices"]))
    for mode in (0, 1):
        for tag in ("str", "lab"):
            assert float(g[f"recon_m{mode}_{tag}"]) == 0.0
            np.testing.assert_allclose(match.item(), float(g[f"match_m{mode}_{tag}"]), rtol=TOL, atol=0)
    (recon + match).backward()
    # a tensor whose gradient is all rounding noise (~1e-9) is held to the case's gradient scale, not its own
    scale = max(float(np.abs(g[k]).max()) for k in g.files if k.startswith("grad_m") and not k.endswith(".norm"))
    for mode in (0, 1):
        for pn, p in params.items():
            want = p.grad.float()
            if f"grad_m{mode}.{pn}" in g.files:
                ref = torch.from_numpy(g[f"grad_m{mode}.{pn}"])
                assert (want - ref).abs().max().item() <= TOL * max(ref.abs().max().item(), 1e-2 * scale), (mode, pn, (want - ref).abs().max().item(), ref.abs().max().item())
            else:
                np.testing.assert_allclose(want.norm().item(), float(g[f"grad_m{mode}.{pn}.norm"]), rtol=TOL, atol=1e-2 * scale)
                head = torch.from_numpy(g[f"grad_m{mode}.{pn}.head"])
                assert (want.flatten()[:64] - head).abs().max().item() <= TOL * max(head.abs().max().item(), 1e-2 * scale), (mode, pn)


def test_loss_reinterprets_the_sum_as_p_by_t_not_a_transpose():
    """M[p'] is the mean of T consecutive flat rows of the [T, P, D] sum; a transposed mean gives another number."""
    torch.manual_seed(0)
    B, T, P, h, d = 2, 3, 4, 1, 8
    a = torch.randn(B, T, P, h, d, dtype=torch.float64)
    _, match = loss_f64([{"k": a, "v": a * 0}], 1)
    s = (a[0] - a[1]).abs().reshape(T * P, h * d) / 2
    m = torch.stack([s[r * T:(r + 1) * T].mean(0) for r in range(P)])
    assert torch.allclose(match, m.norm() / P)
    assert not torch.allclose(match, s.view(T, P, -1).mean(0).norm() / P)


def test_default_config_is_the_references():
    C = default_compinv_config()
    assert dict(C) == dict(name="CompInvEncoder", architecture="ViT-B/16", decode_mode="stride", decode_stride=2, decode_indices=[],
                           adapter={}, dropout=0.0, mode=0)


@pytest.fixture(scope="module")
def lib():
    from dfd_clip_amd.build import build
    build()
    return capi.load_library()


@pytest.mark.parametrize("name", list(CASES))
def test_state_dict_schema_is_the_references(lib, name):
    from dfd_clip_amd.compinv import CompInvEncoder
    case = build_case(name)
    g = load_golden(name)
    model = CompInvEncoder(case["cfg"], None, num_frames=case["T"], precision="fp32")
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in g["keys"]]
    assert [",".join(map(str, t.shape)) for t in sd.values()] == [str(s) for s in g["shapes"]]
    assert list(case["sd"]) == list(sd)  # weights.random_compinv_state_dict writes the same schema
    model.load_state_dict(case["sd"])
    assert model.layer_indices == case["layer_indices"] and model.mode == 1
    opt = model.configure_optimizers(1e-3)
    assert isinstance(opt, torch.optim.AdamW)
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in model.adapter.parameters()]


def test_host_side_checks(lib):
    from dfd_clip_amd.compinv import CompInvEncoder
    case = build_case("compinv_tiny")
    with pytest.raises(NotImplementedError):
        CompInvEncoder(case["cfg"], None, num_frames=case["T"], precision="fp8")
    model = CompInvEncoder(case["cfg"], None, num_frames=case["T"], precision="fp32")
    with pytest.raises(ValueError, match="pair"):
        model(case["x"][:1], ["raw"])
    with pytest.raises(ValueError, match="entries"):
        model(case["x"], ["raw", "c23"])
    with pytest.raises(capi.DfdError):  # no CPU path
        model(case["x"], case["comp"])
    assert lib.dfd_compinv_loss_fwd(None, None, capi.F32, 2, 1, 4, 128, 1, None, None, None, None, None) == -1
    assert lib.dfd_compinv_loss_fwd(1 << 12, 1 << 12, capi.F32, 1, 1, 4, 128, 1, 1 << 12, 1 << 12, 1 << 12, None, None) == -1
    assert b"B >= 2" in lib.dfd_last_error()
    assert lib.dfd_compinv_loss_workspace(196, 768) == (196 * 768 + 196 * 3) * 4
