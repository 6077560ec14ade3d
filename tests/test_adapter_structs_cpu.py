"""CPU checks of the CompInvAdapter structs "768-bn", "768-xxx-768" and "linear": the state_dict schema equals the
reference's (recorded in tests/golden/adapter_*.npz), construction-time initialisation and refusals, the seeded state
dicts, and the host-side argument checks of their kernels (no launch, no GPU)."""
import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.build import build
from tests.adapter_struct_cases import CASES, COMPINV_CASES, build_case, build_compinv_case, load_golden
from tests.cases import make_config


def _schema(module):
    sd = module.state_dict()
    return list(sd), [",".join(map(str, t.shape)) for t in sd.values()]


@pytest.mark.parametrize("name", list(CASES))
def test_detector_state_dict_matches_reference_schema(name):
    from dfd_clip_amd.detector import Detector
    c = build_case(name)
    g = load_golden(name)
    det = Detector(c["cfg"], c["T"], None, precision="fp32")
    keys, shapes = _schema(det)
    assert keys == list(g["keys"]) and shapes == list(g["shapes"])
    assert set(c["sd"]) == set(keys)  # weights.random_state_dict covers the same state, buffers included
    res = det.load_state_dict(c["sd"], strict=True)
    assert not res.missing_keys and not res.unexpected_keys


@pytest.mark.parametrize("name", list(COMPINV_CASES))
def test_compinv_state_dict_matches_reference_schema(name):
    from dfd_clip_amd.compinv import CompInvEncoder
    c = build_compinv_case(name)
    g = load_golden(name)
    model = CompInvEncoder(c["cfg"], None, num_frames=c["T"], precision="fp32")
    keys, shapes = _schema(model)
    assert keys == list(g["keys"]) and shapes == list(g["shapes"])
    model.load_state_dict(c["sd"], strict=True)
    bn = model.adapter.l0_k[1]
    assert torch.equal(bn.running_mean, c["sd"]["adapter.l0_k.1.running_mean"])
    assert bn.num_batches_tracked.dtype == torch.int64 and bn.num_batches_tracked.item() >= 1


def test_seeded_batchnorm_statistics_are_not_the_defaults():
    sd = build_case("adapter_vitb32_bn")["sd"]
    for j in ("k", "v"):
        rm, rv = sd[f"adapter.l0_{j}.1.running_mean"], sd[f"adapter.l0_{j}.1.running_var"]
        assert rm.shape == (2,) and (rm != 0).all() and (rv > 0).all() and (rv != 1).all()
        assert sd[f"adapter.l0_{j}.1.num_batches_tracked"].dtype == torch.int64


def test_linear_starts_as_the_identity():
    from dfd_clip_amd.detector import Detector
    det = Detector(make_config("tiny", adapter__type="normal", adapter__struct={"type": "linear", "x": 32}), 4, None,
                   precision="fp32")
    for i in range(len(det.layer_indices)):
        for j in ("k", "v"):
            assert torch.equal(getattr(det.adapter, f"l{i}_{j}")[0].weight, torch.eye(128))
    assert det.adapter.residual is False


def test_batchnorm_refusals():
    from dfd_clip_amd.detector import Detector
    # width 128: the reference hard-codes Linear(768, 768)
    with pytest.raises(NotImplementedError, match="models.py:877-886"):
        Detector(make_config("tiny", adapter__type="normal", adapter__struct={"type": "768-bn", "x": 32}), 4, None)
    # ema_frame collapses the clip to one frame; BatchNorm2d(num_frames) has num_frames channels
    cfg = make_config("ViT-B/32", decode_mode="index", decode_indices=[11], adapter__type="normal",
                      adapter__struct={"type": "768-bn", "x": 32}, op_mode__ema_frame=0.3)
    with pytest.raises(NotImplementedError, match="ema_frame"):
        Detector(cfg, 4, None)
    # the other structs take any width, ViT-L/14's 1024 included
    for st in ("768-xxx-768", "linear"):
        Detector(make_config("ViT-L/14", decode_mode="index", decode_indices=[23], adapter__type="normal",
                             adapter__struct={"type": st, "x": 64}), 2, None)


def test_invalid_arguments_are_reported_not_launched():
    build()
    lib = capi.load_library()
    assert lib.dfd_abi_version() == 17
    rc = lib.dfd_adapter_bn_stats(1 << 12, capi.BF16, 1 << 12, None, None, None, 1 << 12, 6, 49, 768, 4, 1, 0.1, 1e-5, None)
    assert rc == -1 and b"bad shape" in lib.dfd_last_error()  # 6 frames are not whole clips of 4
    rc = lib.dfd_adapter_bn_stats(1 << 12, capi.BF16, 1 << 12, None, None, None, 1 << 12, 4, 49, 768, 2, 2, 0.1, 1e-5, None)
    assert rc == -1 and b"running statistics" in lib.dfd_last_error()
    rc = lib.dfd_adapter_bn_apply((1 << 12) + 4, capi.F32, None, 1 << 12, capi.F32, None, None, None, None, None, 4, 49, 768, 2, None)
    assert rc == -1 and b"aligned" in lib.dfd_last_error()
    rc = lib.dfd_adapter_bn_bwd(1 << 12, 1 << 12, capi.BF16, 1 << 12, capi.F32, 1 << 12, 1 << 12, 1 << 12, 1 << 12, None,
                                1 << 12, 4, 49, 768, 2, 1, None)
    assert rc == -1 and b"dtypes" in lib.dfd_last_error()
    rc = lib.dfd_gelu_erf(1 << 12, capi.F32, 1 << 12, capi.BF16, 12, None, None)
    assert rc == -1 and b"multiple of 8" in lib.dfd_last_error()
    rc = lib.dfd_gelu_erf_bwd(1 << 12, capi.F32, None, capi.F32, 1 << 12, capi.F32, 16, None, None)
    assert rc == -1 and b"null pointer" in lib.dfd_last_error()
    assert lib.dfd_adapter_bn_workspace(16 * 30, 196, 768) == 16 * 30 * 19 * 16
