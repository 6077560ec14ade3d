"""CPU side of the fused AdamW step (dfd-clip_amd/optim.py: `FusedAdamW`; csrc/optim.hip behind `dfd_sgd_step`'s `extra`): the
ctypes mirror of `dfd_optim_extra` has the header's layout, the entry point rejects bad hyper-parameters on the host before
any launch, and on CPU parameters `FusedAdamW` IS `torch.optim.AdamW` (its fallback), state_dict included."""
import copy
import ctypes
import os
import re

import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# C type -> (size, alignment) under the LP64 ABI the library is built for
_C = {"int32_t": (4, 4), "int64_t": (8, 8), "float": (4, 4), "double": (8, 8)}


def header_layout(struct):
    """[(field, offset)], sizeof of `struct` as a C compiler lays out its declaration in include/dfdclip.h."""
    text = open(os.path.join(ROOT, "include", "dfdclip.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, off, worst = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        if "*" in decl:
            ctype, names = (8, 8), [decl.rsplit("*", 1)[1].replace("const", "").strip()]
        else:
            t, rest = decl.split(None, 1)
            ctype, names = _C[t], [n.strip() for n in rest.split(",")]
        for n in names:
            off = (off + ctype[1] - 1) // ctype[1] * ctype[1]
            fields.append((n, off))
            off += ctype[0]
            worst = max(worst, ctype[1])
    return fields, (off + worst - 1) // worst * worst


def test_optim_extra_mirror_has_the_headers_layout():
    fields, size = header_layout("dfd_optim_extra")
    assert [n for n, _ in fields] == [n for n, _ in capi.OptimExtra._fields_]
    assert [(n, getattr(capi.OptimExtra, n).offset) for n, _ in capi.OptimExtra._fields_] == fields
    assert ctypes.sizeof(capi.OptimExtra) == size == 48
    assert (capi.OPTIM_SGD, capi.OPTIM_ADAMW) == (0, 1)
    text = open(os.path.join(ROOT, "include", "dfdclip.h")).read()
    assert re.search(r"DFD_OPTIM_SGD = 0, DFD_OPTIM_ADAMW = 1", text)


@pytest.fixture(scope="module")
def lib():
    build()
    return capi.load_library()


def _call(lib, extra, table=1 << 12, n=1, blocks=1):
    return lib.dfd_sgd_step(table, n, blocks, 0.01, 0.0, 0.01, 0, None, None if extra is None else ctypes.byref(extra))


@pytest.mark.parametrize("bad,message", [
    (dict(kind=7), b"unknown kind 7"),
    (dict(beta1=1.0), b"betas"),
    (dict(beta2=-0.5), b"betas"),
    (dict(beta1=float("nan")), b"betas"),
    (dict(eps=0.0), b"eps"),
    (dict(step=0), b"step count 0"),
    (dict(exp_avg_sq=None), b"second moments"),
])
def test_bad_adamw_arguments_are_reported_not_launched(lib, bad, message):
    """The table pointer is a made-up address: a call that got as far as a launch would not come back with -1."""
    args = dict(kind=capi.OPTIM_ADAMW, reserved=0, beta1=0.9, beta2=0.999, eps=1e-8, step=1, exp_avg_sq=1 << 12)
    args.update(bad)
    rc = _call(lib, capi.OptimExtra(**args))
    assert rc == -1 and message in lib.dfd_last_error(), lib.dfd_last_error()


def test_empty_table_is_rejected_with_and_without_extra(lib):
    good = capi.OptimExtra(capi.OPTIM_ADAMW, 0, 0.9, 0.999, 1e-8, 1, 1 << 12)
    for extra in (None, good):
        assert _call(lib, extra, table=None) == -1 and b"empty table" in lib.dfd_last_error()
        assert _call(lib, extra, n=0) == -1 and b"empty table" in lib.dfd_last_error()
        assert _call(lib, extra, blocks=0) == -1 and b"total_blocks" in lib.dfd_last_error()


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in [(7, 5), (33,), (1,), (2, 3, 4)]]


def test_on_cpu_parameters_it_is_torch_adamw():
    from dfd_clip_amd.optim import FusedAdamW
    ref, mine = _params(), _params()
    o_ref = torch.optim.AdamW(ref, lr=0.01, weight_decay=0.02)
    o_mine = FusedAdamW(mine, lr=0.01, weight_decay=0.02)
    assert isinstance(o_mine, torch.optim.AdamW)
    assert o_mine.defaults == o_ref.defaults
    g = torch.Generator().manual_seed(1)
    for step in range(3):
        for i, (a, b) in enumerate(zip(ref, mine)):
            if i == 2 and step == 0:  # no gradient: skipped, no state yet
                a.grad = b.grad = None
                continue
            gr = torch.randn(a.shape, generator=g)
            a.grad, b.grad = gr.clone(), gr.clone()
        o_ref.step()
        o_mine.step()
    for a, b in zip(ref, mine):
        assert torch.equal(a, b)
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(o_ref.state[a][k], o_mine.state[b][k]), k
    assert o_mine.state[mine[2]]["step"].item() == 2 and o_mine.state[mine[0]]["step"].item() == 3


@pytest.mark.parametrize("plain_adamw_first", [False, True])
def test_fallback_is_logged_once_and_runs_step_hooks_once(caplog, monkeypatch, plain_adamw_first):
    """torch wraps a class's `step` in its step-hook wrapper the first time the class is instantiated, so what
    `torch.optim.AdamW.step` is depends on whether the process has made a plain AdamW yet: the fallback must run torch's step,
    and the hooks once, in both states."""
    from dfd_clip_amd.optim import FusedAdamW
    unhooked = torch.optim.AdamW.step
    if getattr(unhooked, "hooked", False):
        unhooked = unhooked.__wrapped__
    assert not getattr(unhooked, "hooked", False)
    monkeypatch.setattr(torch.optim.AdamW, "step", unhooked)  # a process that has not made a plain AdamW yet
    if plain_adamw_first:
        torch.optim.AdamW(_params(), lr=0.01)
    assert bool(getattr(torch.optim.AdamW.step, "hooked", False)) == plain_adamw_first
    mine, ref = _params(), _params()
    opt = FusedAdamW(mine, lr=0.01)
    before, after = [], []
    opt.register_step_pre_hook(lambda *a: before.append(1))
    opt.register_step_post_hook(lambda *a: after.append(1))
    with caplog.at_level("WARNING", logger="dfd_clip_amd.optim"):
        for _ in range(3):
            for p in mine:
                p.grad = torch.ones_like(p)
            opt.step()
    assert len(before) == len(after) == 3
    assert len([r for r in caplog.records if "FusedAdamW" in r.getMessage()]) == 1
    o_ref = torch.optim.AdamW(ref, lr=0.01)
    for _ in range(3):
        for p in ref:
            p.grad = torch.ones_like(p)
        o_ref.step()
    for a, b in zip(ref, mine):
        assert torch.equal(a, b) and opt.state[b]["step"].item() == 3


def test_state_dict_loads_into_torch_adamw_and_back():
    from dfd_clip_amd.optim import FusedAdamW
    a, b, c = _params(), _params(), _params()
    o_a = FusedAdamW(a, lr=0.01)
    for p in a:
        p.grad = torch.full_like(p, 0.5)
    o_a.step()
    sd = copy.deepcopy(o_a.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    o_b = torch.optim.AdamW(b, lr=0.5)
    assert set(o_b.state_dict()["param_groups"][0]) == set(sd["param_groups"][0])
    o_b.load_state_dict(sd)
    o_c = FusedAdamW(c, lr=0.5)
    o_c.load_state_dict(copy.deepcopy(o_b.state_dict()))
    for params, opt in ((a, o_a), (b, o_b), (c, o_c)):
        assert opt.param_groups[0]["lr"] == 0.01
        for p, q in zip(params, a):
            p.data.copy_(q.data)
    for params, opt in ((a, o_a), (b, o_b), (c, o_c)):
        for p in params:
            p.grad = torch.full_like(p, -0.25)
        opt.step()
    for pa, pb, pc in zip(a, b, c):
        assert torch.equal(pa, pb) and torch.equal(pa, pc)
        assert o_b.state[pb]["step"].item() == o_c.state[pc]["step"].item() == 2


def test_compinv_encoder_hands_out_the_fused_adamw(lib):
    from dfd_clip_amd.compinv import CompInvEncoder
    from dfd_clip_amd.optim import FusedAdamW, FusedSGD
    from tests.compinv_cases import build_case
    case = build_case("compinv_tiny")
    model = CompInvEncoder(case["cfg"], None, num_frames=case["T"], precision="fp32")
    opt = model.configure_optimizers(1e-3)
    assert isinstance(opt, FusedAdamW) and isinstance(opt, torch.optim.AdamW) and not isinstance(opt, FusedSGD)
    assert opt.defaults["weight_decay"] == 0.01 and opt.defaults["lr"] == 1e-3
