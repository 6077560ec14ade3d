"""bf16 training gradients of the HIP `Detector` (adapter and decoder) against the reference's own fp32 gradients
(tests/golden/bf16grad_<case>.npz, written by tools/gen_golden_bf16_grad.py).

The bar of a parameter comes from the reference alone: `spread` is how far the reference's gradient under bf16 autocast
sits from its fp32 gradient, and the HIP gradient must sit within max(3 spread, 3 median spread of the case) of the fp32
one (relative L2 on the stored elements; for sampled tensors the full norm as well).  Both are bf16 realisations of one
fp32 computation, about one spread from it each; the HIP path rounds a few more stored tensors (the exported K/V, a2,
da1, da2, the masked dOut), at most doubling the roundings on a path, and independent roundings add in quadrature: 3x
covers that and stays far below the 0.3 of a norm that a dropped term, a wrong mask or a wrong transpose moves.
Parameters whose spread exceeds 0.1 are ill-conditioned under bf16 in the reference itself and only checked for
finiteness (tests/test_bf16_grad_cpu.py caps them at 5 % of a case and every applied bar at 0.2).

Largest e / spread per case, measured on MI355X (deterministic kernels, so the values repeat):
    tiny                    0.81  decoder.transformer.resblocks.0.ln_1.bias
    tiny_stride             0.76  decoder.transformer.resblocks.0.attn.out_proj.weight
    tiny_adapter_nln        0.82  adapter.l1_v.1.weight
    tiny_adapter_ln         0.79  adapter.l0_k.1.weight
    tiny_adapter_gl         0.92  adapter.l0_v.2.weight
    tiny_adapter_legacy     0.92  adapter.l0_v.2.weight
    tiny_global             0.46  decoder.transformer.resblocks.1.attn.out_proj.weight
    tiny_attnmode           1.65  decoder.ln_post.bias
    tiny_nopos              0.96  decoder.ln_post.bias
    tiny_augq               0.63  decoder.transformer.resblocks.1.ln_1.weight
    small                   0.71  decoder.transformer.resblocks.1.ln_1.weight
    small14                 0.45  decoder.transformer.resblocks.0.attn.in_proj.weight
    vitb16_cfg1             1.04  decoder.ln_post.bias
    vitl14                  1.29  decoder.ln_post.bias
    vitb16_adapter_gl       0.87  decoder.ln_post.bias
    vitb16_adapter_legacy   0.87  decoder.ln_post.bias
    tiny_ema                0.19  decoder.transformer.resblocks.1.attn.in_proj.weight
    tiny_rank               0.81  decoder.transformer.resblocks.0.ln_1.bias
    tiny_pmask              1.25  decoder.transformer.resblocks.1.ln_1.weight
    adapter_tiny_xxx        0.69  adapter.l0_k.3.weight
    adapter_tiny_linear     0.66  decoder.transformer.resblocks.1.attn.in_proj.weight
    adapter_vitb16_xxx      3.08  decoder.ln_post.bias
(`adapter_vitb16_xxx`: every gradient of the case is 1.0 % short of the fp32 one, |g| / |g32| = 0.989 .. 0.990, which
is what a shift of the bf16 logit does to the slope of the single loss term of this one-clip case; the other cases show
such a common factor too, 1.007 at most.  That 1.0e-2 stands against a bar of 2.1e-2, three times the case's median.)
"""
import numpy as np
import pytest
import torch

from tests import bf16_grad_cases as bc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# fp32 gradient exactly zero in the reference: the temporal ranking loss of `tiny_rank` is flat at its starting point
ZERO_GRADIENT = {"tiny_rank": ["ranking_transform_param"]}


def rel_l2(got, want):
    return float(np.linalg.norm(got.astype(np.float64) - want.astype(np.float64)) / np.linalg.norm(want.astype(np.float64)))


@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_bf16_gradients_within_reference_bf16_spread(name):
    from dfd_clip_amd.detector import Detector
    c, fx = bc.build_case(name), bc.load_fixture(name)
    det = Detector(c["cfg"], c["T"], None, precision="bf16")
    det.load_state_dict(c["sd"], strict=True)
    det = det.to(DEV).train()
    x, m, y = c["x"].to(DEV), c["m"].to(DEV), c["y"].to(DEV)
    comp, speed, np_seed = bc.extras(c)
    np.random.seed(np_seed)
    task_losses, _, other = det(x, [y], m, comp, torch.tensor(speed, device=DEV), train=True, single_task=0)
    (task_losses[0].mean() + sum(other.values())).backward()
    torch.cuda.synchronize()
    params = dict(det.named_parameters())
    bars, sample = bc.bars(fx), int(fx["sample"])
    assert sorted(bars) == sorted(pn for pn, p in params.items() if p.requires_grad and not pn.startswith("encoder."))
    assert [pn for pn, b in bars.items() if b == 0.0] == ZERO_GRADIENT.get(name, [])
    failures, worst = [], (0.0, None)
    for pn, bar in bars.items():
        grad = params[pn].grad
        if bar == 0.0:
            assert grad is None or not grad.any(), pn
            continue
        assert grad is not None and torch.isfinite(grad).all(), pn
        full = grad.detach().float().flatten().cpu().numpy()
        want, spread = fx["g32." + pn], float(fx["spread." + pn])
        e = rel_l2(bc.stored_elements(pn, full, sample), want)
        norm_ratio = float(np.linalg.norm(full.astype(np.float64)) / float(fx["norm32." + pn]))
        print(f"{name} {pn}: e {e:.3e} spread {spread:.3e} e/spread {e / max(spread, 1e-30):.2f} |g|/|g32| {norm_ratio:.4f}"
              + ("  (excluded: spread > 0.1)" if bar is None else f" bar {bar:.3e}"))
        if bar is None:
            continue
        if e / max(spread, 1e-30) > worst[0]:
            worst = (e / max(spread, 1e-30), pn)
        if not (e <= bar and abs(norm_ratio - 1) <= bar):
            failures.append((pn, e, norm_ratio, bar))
    print(f"{name}: largest e/spread {worst[0]:.2f} ({worst[1]})")
    assert not failures, failures
