#!/usr/bin/env python3
"""Writes tests/golden/small24.npz by running the reference's own `Detector` (src/models.py around src/clip/model.py) on
the seeded case of tests/anytok_cases.py, in fp32 and under bf16 autocast on the CPU.  Needs the reference checkout, so
it runs only where that exists; the tests read the fixture and never run this.  Nothing of the reference is copied: it
is imported, through oracle/gen_golden.py's loader, and that module's own `run_case` produces the file — the case is
added to its table in this process only, so the stored layout is exactly that of small14.npz ("medium": fp32 logits,
`logits_bf16` under autocast, K / V row slices, losses, gradients, two SGD steps).

usage: python tools/gen_golden_anytok.py [case ...]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import oracle.gen_golden as gg  # noqa: E402
from oracle.gen_golden import REF, load_reference  # noqa: E402,F401
from tests.anytok_cases import CASES, STORE  # noqa: E402

if __name__ == "__main__":
    torch.set_num_threads(8)
    mm, Acc, to_cn = load_reference()
    for case in (sys.argv[1:] or list(CASES)):
        gg.CASES[case] = (*CASES[case], STORE)
        gg.run_case(case, mm, Acc, to_cn)
