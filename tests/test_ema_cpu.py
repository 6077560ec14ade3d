"""CPU checks of the EMA-teacher update (include/dfdclip_ema.h, `harness.EmaTeacher`): the header against its ctypes table, the
build entries, every host-side refusal of `dfd_ema_step` (none launches, so none needs a GPU), `capi.ema_reference` against the
torch expression of the reference's loop, the rounding fact the shared tower rests on (a self-blend is not the identity in
f32), what `share_encoder`'s deep copy shares, and that `update` leaves aliased pairs alone."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from torch import nn

from dfd_clip_amd import capi
from dfd_clip_amd.harness import EmaTeacher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"const dfd_sgd_param*": ctypes.c_void_p, "void*": ctypes.c_void_p, "int": ctypes.c_int, "int64_t": ctypes.c_int64,
         "float": ctypes.c_float}
RATIOS = [0.0, 0.3, 0.5, 0.95, 0.999, 1.0]


def test_header_matches_the_ctypes_table():
    text = open(os.path.join(ROOT, "include", "dfdclip_ema.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\bint\s+(dfd_\w+)\s*\(([^)]*)\)\s*;", code)
    assert sorted(n for n, _ in protos) == sorted(capi.EMA_SIGNATURES) == ["dfd_ema_step"]
    lib = capi.load_library()
    for name, params in protos:
        res, args = capi.EMA_SIGNATURES[name]
        assert res is ctypes.c_int and getattr(lib, name).argtypes == args
        types = [" ".join(p.split()[:-1]) for p in params.split(",")]
        assert [CTYPE[t] for t in types] == args, name
    assert "DFD_ABI_VERSION" not in code and "typedef" not in code  # the table type is dfdclip.h's own
    assert capi.ABI_VERSION == 17


def test_the_table_is_disjoint_from_every_other():
    others = [capi.SIGNATURES, capi.EXT_SIGNATURES, capi.EXPLAIN_SIGNATURES, capi.AUGMENT_SIGNATURES, capi.ALIGN_SIGNATURES,
              capi.ELASTIC_SIGNATURES, capi.YUV_SIGNATURES, capi.SWIGLU_SIGNATURES, capi.KVGATHER_SIGNATURES, capi.HOOK_SIGNATURES]
    for table in others:
        assert not set(table) & set(capi.EMA_SIGNATURES)
    dfdclip_h = open(os.path.join(ROOT, "include", "dfdclip.h")).read()
    assert "dfd_ema_step" not in dfdclip_h


def test_build_lists_the_header_and_holds_the_kernel_to_zero_scratch():
    from dfd_clip_amd import build
    assert build.NO_SCRATCH["optim.hip"] == "ema_step_kernel"
    src = open(os.path.join(ROOT, "dfd-clip_amd", "csrc", "optim.hip")).read()
    assert "ema_step_kernel" in set(re.findall(r"void (\w+_kernel)\(", src))
    assert "dfdclip_ema.h" in open(build.__file__).read() and "dfdclip_ema.h" in src
    # the blend must not be contracted into a fused multiply-add: the source says so where it is computed
    body = src[src.index("float ema_blend"):src.index("ema_step_kernel")]
    assert "fp contract(off)" in body and "fma" not in body
    # the ISA lint compiles every csrc/*.hip, this one included
    import importlib.util
    spec = importlib.util.spec_from_file_location("isa_lint", os.path.join(ROOT, "tools", "isa_lint.py"))
    lint = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lint)
    assert os.path.samefile(lint.CSRC, build.CSRC) and "optim.hip" in build.sources()
    assert lint.findings(lint.device_asm(os.path.join(build.CSRC, "optim.hip")), "optim.hip") == []


# ---- refusals: all on the host, before any launch --------------------------------------------------------------------

FAKE = 0x10000  # never dereferenced: every call below returns before a launch


@pytest.mark.parametrize("args,word", [
    ((0, 1, 1, 0.5, 0.5), "empty table"), ((FAKE, 0, 1, 0.5, 0.5), "empty table"), ((FAKE, -3, 1, 0.5, 0.5), "empty table"),
    ((FAKE, 1, 0, 0.5, 0.5), "total_blocks"), ((FAKE, 1, -1, 0.5, 0.5), "total_blocks"), ((FAKE, 1, 1 << 31, 0.5, 0.5), "total_blocks"),
    ((FAKE, 1, 1, float("nan"), 0.5), "non-finite"), ((FAKE, 1, 1, 0.5, float("inf")), "non-finite"),
    ((FAKE, 1, 1, float("-inf"), 0.5), "non-finite"),
])
def test_refusals_come_back_with_the_functions_name(args, word):
    lib = capi.load_library()
    rc = lib.dfd_ema_step(*args, None)
    msg = lib.dfd_last_error().decode()
    assert rc == -1 and "dfd_ema_step" in msg and word in msg, (args, rc, msg)


def test_the_binding_refuses_host_tables():
    with pytest.raises(capi.DfdError, match="device tensors"):
        capi.ema_step(torch.zeros(1, 7, dtype=torch.int64), 1, 1, 0.5)


def test_factors_are_the_python_doubles():
    for r in RATIOS:
        keep, take = capi.ema_factors(r)
        assert keep == 1 - r and take == r and isinstance(keep, float)
    assert np.float32(capi.ema_factors(0.999)[0]) != np.float32(1) - np.float32(0.999)  # formed in double, cast once


# ---- ema_reference is the torch expression ----------------------------------------------------------------------------

def operands():
    g = torch.Generator().manual_seed(7)
    t = torch.randn(4096, generator=g)
    s = torch.randn(4096, generator=g) * 3
    tiny = float(np.float32(1e-45))
    special = [0.0, -0.0, tiny, -tiny, 1.1e-38, -5.9e-39, float("inf"), float("-inf"), float("nan"), 1.0, -1.0, 3.4e38, -3.4e38]
    ts = torch.tensor([a for a in special for _ in special], dtype=torch.float32)
    ss = torch.tensor([b for _ in special for b in special], dtype=torch.float32)
    return torch.cat([t, ts]), torch.cat([s, ss])


def same_bits(got, want):
    got, want = torch.as_tensor(got), torch.as_tensor(want)
    assert got.dtype == torch.float32 and want.dtype == torch.float32 and got.shape == want.shape
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), "NaN positions differ"
    assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))


@pytest.mark.parametrize("r", RATIOS)
def test_ema_reference_is_the_torch_expression(r):
    t, s = operands()
    want = (1 - r) * t + r * s  # the reference's loop body on f32 tensors (src/trainer.py:183)
    same_bits(capi.ema_reference(t, s, r), want)
    same_bits(capi.ema_reference(t.numpy(), s.numpy(), r), want)
    assert isinstance(capi.ema_reference(t.numpy(), s.numpy(), r), np.ndarray)


def test_a_fused_multiply_add_would_differ():
    """Why the kernel must not contract: fma(keep, t, take * s) rounds once where torch rounds twice."""
    t, s = operands()
    t, s = t[:4096].double(), s[:4096].double()
    keep, take = np.float32(1 - 0.999), np.float32(0.999)
    fused = (float(keep) * t + (float(take) * s).float().double()).float()  # exact product + rounded product, one rounding
    assert not torch.equal(fused, capi.ema_reference(t.float(), s.float(), 0.999))


def test_self_blend_drifts_except_at_one_half():
    """(1 - r) x + r x != x in f32: the reference's copy of the frozen tower takes a rounding walk; at r = 0.5 it is exact."""
    x = torch.randn(200_000, generator=torch.Generator().manual_seed(1))
    for r, lo, hi in ((0.999, 0.05, 0.30), (0.95, 0.05, 0.30)):
        moved = ((1 - r) * x + r * x != x).float().mean().item()
        assert lo < moved < hi, (r, moved)
        assert torch.equal(capi.ema_reference(x, x, r), (1 - r) * x + r * x)
    assert torch.equal((1 - 0.5) * x + 0.5 * x, x) and torch.equal(capi.ema_reference(x, x, 0.5), x)


# ---- share_encoder: what the copy shares, what update leaves alone ----------------------------------------------------

class Stub(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = nn.Linear(5, 7)
        self.decoder = nn.Sequential(nn.Linear(7, 3), nn.BatchNorm1d(3))


def test_memo_deep_copy_shares_the_towers_parameters_and_nothing_else():
    from dfd_clip_amd.detector import Detector
    from tests.cases import build_case
    case = build_case("tiny_adapter_ln")
    model = Detector(case["cfg"], case["T"], None, precision="fp32")
    model.load_state_dict(case["sd"])
    shared = EmaTeacher(model, 0.999, 0, share_encoder=True)
    private = EmaTeacher(model, 0.999, 0)
    assert shared.module.encoder is model.encoder and private.module.encoder is not model.encoder
    assert shared.module is not model and shared.module.decoder is not model.decoder and shared.module.adapter is not model.adapter
    tower = {id(p) for p in model.encoder.parameters()} | {id(b) for b in model.encoder.buffers()}
    assert tower
    pairs = list(zip(shared.module.named_parameters(), model.named_parameters()))
    assert len(pairs) == len(list(private.module.parameters())) and len(pairs) > len(tower)
    for (n1, p1), (n2, p2) in pairs:
        assert n1 == n2
        if id(p2) in tower:
            assert p1 is p2, n1
        else:
            assert p1 is not p2 and p1.data_ptr() != p2.data_ptr() and torch.equal(p1, p2), n1
    for (n1, b1), (n2, b2) in zip(shared.module.named_buffers(), model.named_buffers()):
        assert n1 == n2 and ((b1 is b2) == (id(b2) in tower)), n1
    sd = shared.module.state_dict()
    assert list(sd) == list(model.state_dict()) and all(torch.equal(sd[k], v) for k, v in model.state_dict().items())
    # runtime state is the copy's own
    assert shared.module._kv_cache is not model._kv_cache and shared.module.decoder._wt_cache is not model.decoder._wt_cache


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("r", [0.999, 0.5])
def test_update_skips_aliased_pairs(fused, r):
    torch.manual_seed(3)
    model = Stub()
    teacher = EmaTeacher(model, r, teach_at=1, share_encoder=True, fused=fused)
    assert teacher.module.encoder is model.encoder and teacher.module.decoder is not model.decoder
    with torch.no_grad():
        for p in model.decoder.parameters():
            p.add_(torch.randn_like(p))
        model.decoder[1].running_mean.add_(1.0)
    tower = [(p, p.data_ptr(), p._version, p.detach().clone()) for p in model.encoder.parameters()]
    before = [p.detach().clone() for p in teacher.module.decoder.parameters()]
    ptrs = [p.data_ptr() for p in teacher.module.decoder.parameters()]
    teacher.update(model)
    assert teacher.steps == 1 and not teacher.teaching
    for p, ptr, version, value in tower:  # not re-seated, not written: the student's own weights
        assert p.data_ptr() == ptr and p._version == version and torch.equal(p, value)
        assert not (r != 0.5 and torch.equal((1 - r) * value + r * value, value)), "the blend would have changed it"
    for p1, p2, old in zip(teacher.module.decoder.parameters(), model.decoder.parameters(), before):
        assert torch.equal(p1, (1 - r) * old + r * p2) and not torch.equal(p1, old)
    if fused:  # in place, whichever kernels did it
        assert [p.data_ptr() for p in teacher.module.decoder.parameters()] == ptrs
    # only parameters are blended (the reference's loop): buffers keep the copy's values
    assert torch.equal(teacher.module.decoder[1].running_mean, torch.zeros(3))
    teacher.update(model)
    assert teacher.teaching


def test_unshared_unfused_update_is_the_reference_loop():
    torch.manual_seed(4)
    model = Stub()
    teacher = EmaTeacher(model, 0.95, teach_at=0)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(torch.randn_like(p))
    before = [p.detach().clone() for p in teacher.module.parameters()]
    teacher.update(model)
    for p1, p2, old in zip(teacher.module.parameters(), model.parameters(), before):
        assert torch.equal(p1, (1 - 0.95) * old + 0.95 * p2)
    assert teacher.teaching
