"""CPU checks of `bench.py`'s options: a plain run measures the headline alone, and `--dump-outputs` writes float32
arrays within its budget, sampled at the same positions in every run."""
import os
import sys

import numpy as np
import torch

import bench


def _parse(argv, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_plain_run_is_the_headline_alone(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "2"], monkeypatch)
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(["--full", "--dump-outputs", "out"], monkeypatch)
    assert a.full and a.dump_outputs == "out"


class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.big = torch.nn.Parameter(torch.randn(512, 300, generator=g))  # larger than DUMP_SAMPLE: sampled
        self.small = torch.nn.Parameter(torch.randn(16, generator=g))
        self.frozen = torch.nn.Parameter(torch.randn(8, generator=g), requires_grad=False)
        self.big.grad = torch.ones_like(self.big)
        self.small.grad = -torch.ones_like(self.small)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_train(tmp_path):
    det = _Toy()
    out = ([torch.tensor(0.25)], [torch.arange(6.0).view(3, 2).to(torch.bfloat16)])
    runs = []
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), det, out, "train")
        runs.append(_load(str(tmp_path / name)))
    a, b = runs
    assert sorted(a) == ["grad.big", "grad.small", "param.big", "param.small", "task0_logits", "task0_loss"]
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= bench.DUMP_BUDGET_BYTES
    np.testing.assert_array_equal(a["task0_logits"], np.arange(6.0, dtype=np.float32).reshape(3, 2))
    assert a["task0_loss"] == np.float32(0.25)
    np.testing.assert_array_equal(a["param.small"], det.small.detach().numpy())
    assert a["param.big"].shape == (bench.DUMP_SAMPLE,)
    flat = det.big.detach().numpy().reshape(-1)
    assert np.isin(a["param.big"], flat).all()  # a sample of the tensor's own elements ...
    for k in a:  # ... at the same positions in every run
        np.testing.assert_array_equal(a[k], b[k])


def test_dump_outputs_infer(tmp_path):
    logits = [torch.randn(4, 2, generator=torch.Generator().manual_seed(1))]
    bench.dump_outputs(str(tmp_path), _Toy(), logits, "infer")
    got = _load(str(tmp_path))
    assert list(got) == ["task0_logits"]
    np.testing.assert_array_equal(got["task0_logits"], logits[0].numpy())
