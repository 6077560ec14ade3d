"""CPU checks of the patch-mask K/V gather (include/dfdclip_kvgather.h): the header against its ctypes table, every host-side
refusal and no-op of `dfd_kv_gather_patches` (none of them launches, so none needs a GPU), `detector.gather_reference`
against the torch sequence the `mask_gather="torch"` arm runs, and the [L, S] index table of the new host code against the
draws of that arm's per-layer loop under the same numpy seed."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.detector import draw_patch_indices, gather_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "const float*": ctypes.c_void_p,
         "int": ctypes.c_int, "int64_t": ctypes.c_int64}


def test_header_matches_the_ctypes_table():
    text = open(os.path.join(ROOT, "include", "dfdclip_kvgather.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\bint\s+(dfd_\w+)\s*\(([^)]*)\)\s*;", code)
    assert sorted(n for n, _ in protos) == sorted(capi.KVGATHER_SIGNATURES) == ["dfd_kv_gather_last_path", "dfd_kv_gather_patches"]
    lib = capi.load_library()
    for name, params in protos:
        res, args = capi.KVGATHER_SIGNATURES[name]
        assert res is ctypes.c_int and getattr(lib, name).argtypes == args
        types = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
        assert len(types) == len(args), name
        assert [CTYPE[t] for t in types] == args, name
    assert "DFD_ABI_VERSION" not in code.replace("WITHOUT a new DFD_ABI_VERSION", "")
    assert (capi.KVGATHER_VEC16, capi.KVGATHER_ELEMENT) == tuple(int(re.search(rf"#define {n} (\d+)", code).group(1))
                                                               for n in ("DFD_KVGATHER_VEC16", "DFD_KVGATHER_ELEMENT"))
    assert capi.ABI_VERSION == 17


def test_the_table_is_disjoint_from_every_other():
    others = [capi.SIGNATURES, capi.EXT_SIGNATURES, capi.EXPLAIN_SIGNATURES, capi.AUGMENT_SIGNATURES, capi.ALIGN_SIGNATURES,
              capi.ELASTIC_SIGNATURES, capi.YUV_SIGNATURES, capi.SWIGLU_SIGNATURES, capi.HOOK_SIGNATURES]
    for table in others:
        assert not set(table) & set(capi.KVGATHER_SIGNATURES)


def test_build_lists_the_header_and_holds_the_kernels_to_zero_scratch():
    from dfd_clip_amd import build
    assert build.NO_SCRATCH["kv_gather.hip"] == "kv_gather_"
    src = open(os.path.join(ROOT, "dfd-clip_amd", "csrc", "kv_gather.hip")).read()
    assert set(re.findall(r"void (\w+_kernel)\(", src)) == {"kv_gather_vec16_kernel", "kv_gather_element_kernel"}
    assert "dfdclip_kvgather.h" in open(build.__file__).read() and "kv_gather.hip" in build.sources()


# ---- refusals and no-ops: all on the host, before any launch -------------------------------------------------------------

FAKE = 0x10000  # never dereferenced: every call below returns before a launch
GOOD = dict(k=FAKE, v=FAKE + 4096, dtype=capi.BF16, sl=4 * 9 * 64, sf=9 * 64, sp=64, index=FAKE + 8192, pos=0, k_out=FAKE + 12288,
            v_out=FAKE + 16384, L=2, frames=4, T=2, P=9, S=5, D=64)


def call(**over):
    a = dict(GOOD, **over)
    lib = capi.load_library()
    rc = lib.dfd_kv_gather_patches(a["k"], a["v"], a["dtype"], a["sl"], a["sf"], a["sp"], a["index"], a["pos"], a["k_out"], a["v_out"],
                                   a["L"], a["frames"], a["T"], a["P"], a["S"], a["D"], None)
    return rc, lib.dfd_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(k=0), "null"), (dict(v=0), "null"), (dict(index=0), "null"), (dict(k_out=0), "null"), (dict(v_out=0), "null"),
    (dict(dtype=capi.FP8), "dtype"), (dict(dtype=7), "dtype"),
    (dict(S=10), "S=10"), (dict(S=-1), "S=-1"), (dict(T=0), "T=0"), (dict(T=-2), "T=-2"), (dict(T=3), "T=3"),
    (dict(sp=63), "stride_patch"), (dict(L=65536), "fit the grid"),
    (dict(frames=1 << 29, T=1, P=8, S=8), "fit the grid"), (dict(frames=1 << 40, T=1), "fit the grid"),
    (dict(L=-1), "negative"), (dict(frames=-2), "negative"), (dict(D=-8, sp=64), "negative"),
])
def test_refusals_come_back_with_the_functions_name(over, word):
    rc, msg = call(**over)
    assert rc == -1 and "dfd_kv_gather_patches" in msg and word in msg, (over, rc, msg)
    assert capi.load_library().dfd_kv_gather_last_path() == 0


@pytest.mark.parametrize("over", [dict(L=0), dict(frames=0), dict(S=0), dict(S=0, P=0), dict(L=0, frames=0, S=0)])
def test_empty_calls_are_successful_no_ops(over):
    rc, msg = call(**over)
    assert rc == 0, (over, msg)
    assert capi.load_library().dfd_kv_gather_last_path() == 0


def test_the_binding_refuses_host_tensors():
    k = torch.zeros(1, 2, 4, 8)
    idx = torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(capi.DfdError, match="device tensors"):
        capi.kv_gather_patches(k, k, idx, None, T=1)


# ---- gather_reference is the torch sequence of the "torch" arm ------------------------------------------------------------

def torch_arm(kr, vr, idx_rows, pos, b, t, P):
    """The sequence of `Detector.predict`'s `mask_gather="torch"` branch on a dense export [L, b*t*P, D], verbatim."""
    num_select = len(idx_rows[0])
    ks, vs = [], []
    for i in range(kr.shape[0]):
        idx = torch.as_tensor(idx_rows[i])
        ks.append(kr[i].view(b * t, P, -1).index_select(1, idx).reshape(b * t * num_select, -1))
        vs.append(vr[i].view(b * t, P, -1).index_select(1, idx).reshape(b * t * num_select, -1))
    kr, vr = torch.stack(ks), torch.stack(vs)
    if pos is not None:
        pp = pos.to(kr.dtype).view(1, 1, t, 1, -1)
        kr = (kr.view(len(ks), b, t, num_select, -1) + pp).view_as(kr)
        vr = (vr.view(len(vs), b, t, num_select, -1) + pp).view_as(vr)
    return kr.contiguous(), vr.contiguous()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("L,b,t,P,S,D", [(2, 2, 3, 9, 5, 72), (1, 1, 1, 4, 4, 8), (3, 2, 4, 4, 2, 128)])
def test_gather_reference_is_the_torch_arm_bit_for_bit(dtype, with_pos, L, b, t, P, S, D):
    g = torch.Generator().manual_seed(L * 1000 + D)
    kr = torch.randn(L, b * t * P, D, generator=g).to(dtype)
    vr = torch.randn(L, b * t * P, D, generator=g).to(dtype)
    pos = (torch.randn(t, D, generator=g) * 1.37) if with_pos else None  # f32 values that bf16 cannot hold: rounded first
    rng = np.random.RandomState(3)
    rows = [rng.permutation(P)[:S] for _ in range(L)]
    index = torch.as_tensor(np.stack(rows), dtype=torch.int32)
    want_k, want_v = torch_arm(kr, vr, rows, pos, b, t, P)
    for src_k, src_v, kw in ((kr, vr, dict(P=P)), (kr.view(L, b * t, P, D), vr.view(L, b * t, P, D), {})):
        got_k, got_v = gather_reference(src_k, src_v, index, pos, t, **kw)
        assert got_k.dtype == dtype and got_k.shape == (L, b * t * S, D) and got_k.is_contiguous()
        assert torch.equal(got_k.view(torch.uint8), want_k.view(torch.uint8)) and torch.equal(got_v.view(torch.uint8), want_v.view(torch.uint8))
    # the same from strided views of a q|k|v buffer whose every other byte is NaN
    buf = torch.full((L, b * t, P + 1, 3 * D), float("nan"), dtype=dtype)
    buf[:, :, 1:, D:2 * D] = kr.view(L, b * t, P, D)
    buf[:, :, 1:, 2 * D:] = vr.view(L, b * t, P, D)
    got_k, got_v = gather_reference(buf[:, :, 1:, D:2 * D], buf[:, :, 1:, 2 * D:], index, pos, t)
    assert torch.equal(got_k.view(torch.uint8), want_k.view(torch.uint8)) and torch.equal(got_v.view(torch.uint8), want_v.view(torch.uint8))


def test_gather_reference_rounds_pos_first():
    """bf16, k = 2^-8, pos = 1 + 2^-8.  pos is a tie between 1 and 1 + 2^-7 and rounds to even, 1; then 2^-8 + 1 is the
    same tie: 1.  One rounding of the f32 sum 1 + 2^-7 would give 1.0078125, which bf16 holds exactly."""
    k = torch.full((1, 1, 1, 1), 2.0 ** -8, dtype=torch.bfloat16)
    pos = torch.tensor([[1.0 + 2.0 ** -8]])
    got, _ = gather_reference(k, k, torch.zeros(1, 1, dtype=torch.int32), pos, 1)
    assert got.float().item() == 1.0  # pos -> 1.0 (tie to even), 1 + 2^-8 -> tie -> 1.0
    assert torch.tensor(2.0 ** -8 + 1.0 + 2.0 ** -8).to(torch.bfloat16).float().item() == 1.0078125  # one rounding would differ


# ---- the [L, S] table is the per-layer loop's draws ----------------------------------------------------------------------

def legacy_draws(kind, P, num_select, layer_indices, guide_v):
    """The draws of the "torch" arm's loop, verbatim but for the device copy."""
    rows, idx = [], None
    for i in range(len(layer_indices)):
        if kind == "guide":
            idx = np.random.choice(range(P), num_select, replace=False, p=guide_v[layer_indices[i]].flatten())
        elif idx is None or kind == "sample":
            idx = np.random.choice(range(P), num_select, replace=False)
        rows.append(np.asarray(idx))
    return np.stack(rows)


@pytest.mark.parametrize("kind", ["batch", "sample", "guide"])
@pytest.mark.parametrize("P,S,layers", [(4, 2, [0, 1]), (196, 49, [1, 3, 5, 7, 9, 11]), (9, 9, [2])])
def test_index_table_equals_the_loops_draws(kind, P, S, layers):
    g = int(round(P ** 0.5))
    v = np.random.RandomState(5).uniform(0.05, 1.0, size=(max(layers) + 1, g, g))
    v = v / v.reshape(len(v), -1).sum(1)[:, None, None]
    for seed in (11, 12):
        np.random.seed(seed)
        want = legacy_draws(kind, P, S, layers, v)
        after_want = np.random.random()
        np.random.seed(seed)
        table = torch.full((len(layers), S), -7, dtype=torch.int32)
        draw_patch_indices(kind, P, S, layers, v, table.numpy())
        after_got = np.random.random()
        assert np.array_equal(table.numpy(), want) and table.dtype == torch.int32
        assert after_got == after_want, "the numpy stream must advance exactly as in the loop"
        if kind == "batch":
            assert (table == table[0]).all()
        elif len(layers) > 1 and P > 4:
            assert not (table == table[0]).all()
