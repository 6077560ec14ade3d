"""The bf16 gradient fixtures (tests/golden/bf16grad_<case>.npz) meet the conditions their bars rest on, checked from the
files alone: no GPU, no reference.  tests/test_hip_bf16_grad.py holds the HIP gradients to these bars."""
import numpy as np
import pytest

from tests import adapter_struct_cases, cases
from tests import bf16_grad_cases as bc
from tests.cases import load_golden

# the only parameters whose gradient is ill-conditioned under bf16 in the reference itself (|g| ~ 2e-4 .. 7e-4, spread 2.6
# and 6.6): the bias of the LayerNorm behind the GELU, in the first tapped layer's and the second's key adapter
EXCLUDED = {"tiny_adapter_gl": ["adapter.l0_k.2.bias", "adapter.l1_k.2.bias"],
            "tiny_adapter_legacy": ["adapter.l0_k.2.bias", "adapter.l1_k.2.bias"]}


def test_every_case_has_a_fixture():
    assert len(bc.DETECTOR_CASES) == 19 and len(bc.STRUCT_CASES) + len(bc.LEFT_OUT) == 4
    for name in bc.ALL_CASES:
        bc.load_fixture(name)


@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_fixture_conditions(name):
    fx = bc.load_fixture(name)
    bars, sample = bc.bars(fx), int(fx["sample"])
    assert 0 < sample <= bc.SAMPLE
    excluded = [pn for pn, b in bars.items() if b is None]
    assert excluded == EXCLUDED.get(name, [])
    assert len(excluded) <= bc.MAX_EXCLUDED * len(bars)
    for pn, b in bars.items():
        g, numel = fx["g32." + pn], int(fx["numel." + pn])
        assert g.dtype == np.float32 and g.ndim == 1 and np.isfinite(g).all(), pn
        idx = bc.sample_indices(pn, numel, sample)
        assert g.size == (numel if idx is None else sample), pn
        if idx is not None:
            assert idx.size == sample == np.unique(idx).size and 0 <= idx[0] and idx[-1] < numel, pn
        norm, spread = float(fx["norm32." + pn]), float(fx["spread." + pn])
        assert np.isfinite(norm) and np.isfinite(spread) and spread >= 0, pn
        stored_norm = float(np.linalg.norm(g.astype(np.float64)))
        if idx is None:
            assert abs(stored_norm - norm) <= 1e-6 * norm, pn
        else:
            assert stored_norm <= norm * (1 + 1e-6), pn
        if b == 0.0:
            assert norm == 0 and not g.any(), pn
        elif b is not None:
            assert 0 < b <= bc.MAX_BAR, (pn, b)
            assert spread <= bc.MAX_SPREAD, pn


@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_fixture_keys_are_the_trainable_parameters(name):
    import torch
    from dfd_clip_amd.detector import Detector
    table = adapter_struct_cases.CASES if name in adapter_struct_cases.CASES else cases.CASES
    arch, _, T, over = table[name][:4]
    fx = bc.load_fixture(name)
    with torch.device("meta"):  # names and shapes only: no weights are drawn
        det = Detector(cases.make_config(arch, **over), T, None, precision="bf16")
    want = {pn: p.numel() for pn, p in det.named_parameters() if p.requires_grad and not pn.startswith("encoder.")}
    assert sorted(bc.param_names(fx)) == sorted(want)
    assert all(int(fx["numel." + pn]) == n for pn, n in want.items())
    per_param = {"g32.", "norm32.", "spread.", "numel."}
    assert sorted(fx.files) == sorted(["sample"] + [k + pn for pn in want for k in per_param])


@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_fp32_gradients_are_those_of_the_existing_fixture(name):
    """The fp32 side is the gradient the fp32 train-step tests already hold the HIP path to."""
    fx, g = bc.load_fixture(name), load_golden(name)
    sample, seen = int(fx["sample"]), 0
    for pn in bc.param_names(fx):
        if "grad0." + pn in g.files:
            whole = g["grad0." + pn].reshape(-1)
            assert np.array_equal(bc.stored_elements(pn, whole, sample), fx["g32." + pn]), pn
            seen += 1
        elif f"grad0.{pn}.norm" in g.files:
            # that fixture's norm was accumulated in f32 over up to 4M elements, this one's in f64 (the generator compares
            # the f32 norms for equality); the elements both files hold are compared exactly
            assert abs(float(g[f"grad0.{pn}.norm"]) - float(fx["norm32." + pn])) <= 1e-3 * float(fx["norm32." + pn]), pn
            head = g[f"grad0.{pn}.head"]
            idx = bc.sample_indices(pn, int(fx["numel." + pn]), sample)
            assert np.array_equal(fx["g32." + pn][:np.searchsorted(idx, 64)], head[idx[idx < 64]]), pn
            seen += 1
    assert seen == len(bc.param_names(fx))
