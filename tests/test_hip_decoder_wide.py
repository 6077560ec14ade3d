"""The decoder's attention kernels past 16 heads (ViT-g/14's decoder has 24; the shared argument check allows 64 = 4096
channels): the cases, float64 references and bars of tests/test_hip_decoder_edges.py, run by its own test bodies at head
counts whose merge (`decoder_attn_combine_kernel`, one thread per channel of at most 16 heads) takes several workgroups per
clip: 24 = two groups of 12, 18 = two groups of 9 with eight key rows side by side, 64 = four groups of 16 (the bound).
(Some counts stay refused, in words, by the older rule that a workgroup of heads * 8 * R lanes must be whole waves and at
most 1024 lanes: 17 would need 1088, as tests/test_abi_cpu.py pins.)"""
import pytest
import torch

from tests import test_hip_decoder_edges as edges
from tests.test_hip_decoder_edges import capi  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

# (B, T, P, heads)
WIDE = [(2, 3, 20, 24), (3, 2, 9, 18), (2, 2, 5, 64)]


@pytest.mark.parametrize("shape", WIDE, ids=str)
@pytest.mark.parametrize("dtype", edges.DTYPES, ids=["f32", "bf16"])
def test_forward_and_map_past_16_heads(capi, shape, dtype):  # noqa: F811
    edges.test_forward_and_map(capi, shape, dtype)


@pytest.mark.parametrize("shape", WIDE, ids=str)
@pytest.mark.parametrize("dtype", edges.DTYPES, ids=["f32", "bf16"])
def test_backward_past_16_heads(capi, shape, dtype):  # noqa: F811
    edges.test_backward(capi, shape, dtype)


@pytest.mark.parametrize("modes", ["frame+temporal"])
@pytest.mark.parametrize("shape", WIDE[:1], ids=str)
def test_modes_at_24_heads(capi, shape, modes):  # noqa: F811
    edges.test_modes(capi, shape, torch.bfloat16, modes)
