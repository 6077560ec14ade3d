"""What the bf16 gradient fixtures (tests/golden/bf16grad_<case>.npz) hold and how a test reads them; shared by their
generator (`tools/gen_golden_bf16_grad.py`, which ran the reference's own `Detector` in fp32 and under bf16 autocast) and
by tests/test_bf16_grad_cpu.py / tests/test_hip_bf16_grad.py.

Per trainable parameter `pn` of a case:
  g32.<pn>      the reference's fp32 gradient of training step 0: whole up to `sample` elements, above that the
                elements `sample_indices(pn, numel, sample)` of the flattened tensor (re-derived, never stored)
  norm32.<pn>   the full fp32 gradient's L2 norm
  spread.<pn>   |g_autocast - g32| / |g32| (L2) over the stored elements: how far the reference's own bf16 run sits
                from its fp32 run
and once per file `sample` (4096 unless the file would have passed 1 MB) and `numel.<pn>`.
"""
import os
import zlib

import numpy as np

from tests import adapter_struct_cases, cases

SAMPLE = 4096
MAX_SPREAD = 0.1     # above it the parameter's gradient is ill-conditioned under bf16 in the reference itself
MAX_EXCLUDED = 0.05  # of a case's parameters
FACTOR = 3.0
MAX_BAR = 0.2
DETECTOR_CASES = list(cases.CASES)
# a case that misses a condition of the fixtures is left out, not the condition loosened: the BatchNorm struct's reference
# run under bf16 autocast sits up to 0.09 of a norm from its fp32 run, which would set a bar of 0.27 > MAX_BAR
LEFT_OUT = {"adapter_vitb32_bn": "largest bar 0.270 > 0.2"}
STRUCT_CASES = [n for n in adapter_struct_cases.CASES if n not in LEFT_OUT]
ALL_CASES = DETECTOR_CASES + STRUCT_CASES


def build_case(name):
    return adapter_struct_cases.build_case(name) if name in adapter_struct_cases.CASES else cases.build_case(name)


def extras(case):
    """The `comp` / `speed` inputs of the reference's training run of this case."""
    e = cases.EXTRA_INPUTS
    return e["comp"][:case["B"]], e["speed"][:case["B"]], e["np_seed"]


def sample_indices(pn, numel, sample=SAMPLE):
    """Sorted flat indices of the elements a fixture keeps of parameter `pn`; None: all of them."""
    if numel <= sample:
        return None
    return np.sort(np.random.default_rng(zlib.crc32(pn.encode())).choice(numel, sample, replace=False))


def stored_elements(pn, flat, sample=SAMPLE):
    idx = sample_indices(pn, flat.shape[0], sample)
    return flat if idx is None else flat[idx]


def fixture_path(name):
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"bf16grad_{name}.npz")


def load_fixture(name):
    return np.load(fixture_path(name), allow_pickle=False)


def param_names(fx):
    return [k[len("g32."):] for k in getattr(fx, "files", fx) if k.startswith("g32.")]


def bars(fx):
    """{pn: bar} of a fixture: max(3 spread(pn), 3 median spread of the case); None where the parameter is excluded
    (spread > MAX_SPREAD) and 0.0 where the fp32 gradient itself is zero.  The median runs over every parameter with a
    non-zero fp32 gradient."""
    names = param_names(fx)
    spread = {pn: float(fx["spread." + pn]) for pn in names if float(fx["norm32." + pn]) > 0}
    med = float(np.median(list(spread.values())))
    out = {}
    for pn in names:
        if pn not in spread:
            out[pn] = 0.0
        elif spread[pn] > MAX_SPREAD:
            out[pn] = None
        else:
            out[pn] = max(FACTOR * spread[pn], FACTOR * med)
    return out
