"""CPU side of the decoder attention maps: the float64 restatement against the reference's fixtures, the explain header
against its ctypes table and the library's exports, argument checks that return before any launch, guide files, and the
guide draw of `patch_mask.type: guide`."""
import ast
import os
import re

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi, harness
from tests.attnmap_cases import (ATTNMAP_CASES, GUIDE_CASE, attention_branches, build_guide_case, guide_map,
                                 load_attnmap_golden)
from tests.cases import EXTRA_INPUTS, load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ATTNMAP_CASES)
def test_restatement_matches_the_reference(name):
    """<= 2e-5, the oracle's bar in test_oracle_golden.py, on the (q, k, mask) the reference's blocks received."""
    g = load_attnmap_golden(name)
    modes = ("frame", "temporal") if name == "tiny_attnmode" else ()
    q, k, mask = torch.from_numpy(g["q"]), torch.from_numpy(g["k"]), torch.from_numpy(g["mask"])
    L, B, H, S = g["aff"].shape
    assert g["branches"].shape == (2, L, B, H, S) and q.shape == (L, B, H, 128) and k.shape == (L, B, S, H * 64)
    for i in range(L):
        ws, wc = attention_branches(q[i], k[i], mask, mask.shape[1], modes)
        for nm, got, want in (("softmax", ws, g["branches"][0, i]), ("coda", wc, g["branches"][1, i]), ("aff", 0.5 * (ws + wc), g["aff"][i])):
            err = (got - torch.from_numpy(want).double()).abs().max().item()
            print(f"{name} block {i} {nm}: worst |err| {err:.3e}")
            assert err <= 2e-5, (name, i, nm, err)
    if name == "tiny":  # the padded tail of clip 1 weighs nothing
        pad = ~mask.repeat_interleave(S // mask.shape[1], dim=1)
        assert pad.any() and (g["aff"][:, pad.numpy()[:, None, :].repeat(H, 1)] == 0).all()


def _explain_functions():
    text = open(os.path.join(ROOT, "include", "dfdclip_explain.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", text)))


def test_explain_header_ctypes_table_and_exports_agree():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    fns = _explain_functions()
    assert fns == sorted(capi.EXPLAIN_SIGNATURES) == ["dfd_decoder_attn_map"]
    assert not set(fns) & (set(capi.SIGNATURES) | set(capi.EXT_SIGNATURES) | set(capi.HOOK_SIGNATURES))
    for name in fns:
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes == capi.EXPLAIN_SIGNATURES[name][1]
    assert lib.dfd_abi_version() == capi.ABI_VERSION == 17
    # the declaration has as many parameters as the table
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfdclip_explain.h")).read(), flags=re.S)
    params = re.search(r"dfd_decoder_attn_map\s*\((.*?)\)\s*;", text, flags=re.S).group(1)
    assert len(params.split(",")) == len(capi.EXPLAIN_SIGNATURES["dfd_decoder_attn_map"][1])


def test_every_explain_function_has_a_guarded_test():
    src = open(os.path.join(ROOT, "tests", "test_hip_guarded_attnmap.py")).read()
    tree = ast.parse(src)
    tests = {n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith("test_")}
    table = {}
    for line in ast.get_docstring(tree).splitlines():
        m = re.match(r"\s*(dfd_[a-z0-9_]+)\s+(test_[a-z0-9_, ]+)$", line)
        if m:
            table[m.group(1)] = [t.strip() for t in m.group(2).split(",") if t.strip()]
    assert sorted(table) == _explain_functions()
    for f, ts in table.items():
        assert ts and all(t in tests for t in ts), f
        assert re.search(r"\bcapi\.%s\(" % re.escape(f[len("dfd_"):]), src), f"{f}: no call through capi in the module"


def test_bad_arguments_return_an_error_without_launching():
    from dfd_clip_amd.build import build
    build()
    lib = capi.load_library()
    p = [1 << 12, 1 << 13, 1 << 14, 1 << 15, 1 << 16]  # never dereferenced: every call returns at its checks
    call = lambda q, k, mask, stats, ext, aff, d=64, dt=capi.F32, lay=None: lib.dfd_decoder_attn_map(
        q, k, dt, lay, mask, stats, ext, aff, None, 1, 2, 4, 2, d, None)
    for q, k, aff in ((None, p[1], p[4]), (p[0], None, p[4]), (p[0], p[1], None)):
        assert call(q, k, p[2], p[3], None, aff) == -1 and b"null pointer" in lib.dfd_last_error()
    assert call(p[0], p[1], p[2], None, None, p[4]) == -1 and b"null pointer" in lib.dfd_last_error()  # neither stats nor ext_weights
    assert call(p[0], p[1], p[2], p[3], None, p[4], d=32) == -1 and b"head dim 32" in lib.dfd_last_error()
    assert call(p[0], p[1], p[2], p[3], None, p[4], dt=capi.FP8) == -1 and b"kv_dtype" in lib.dfd_last_error()
    assert call(p[0], p[1] + 4, p[2], p[3], None, p[4]) == -1 and b"16-byte aligned" in lib.dfd_last_error()
    import ctypes
    lay = capi.KvLayoutDesc(3 * 128 + 2, 5 * (3 * 128 + 2), None)  # rows that would not stay 16-byte aligned
    assert call(p[0], p[1], p[2], p[3], None, p[4], lay=ctypes.byref(lay)) == -1 and b"row stride" in lib.dfd_last_error()


# ---- guide files ----------------------------------------------------------------------------------------------------

def test_guide_round_trip_and_refusals(tmp_path):
    v = guide_map(2, 2)
    assert np.allclose(v.reshape(2, -1).sum(1), 1.0) and v.std() > 0.05
    path = tmp_path / "guide.npz"
    harness.save_guide(path, {"v": v})
    back = harness.load_guide(path)
    assert back["v"].dtype == np.float64 and np.array_equal(back["v"], v)
    for bad in (tmp_path / "guide.pkl", tmp_path / "guide.pickle", tmp_path / "guide"):
        with pytest.raises(ValueError, match=r"np\.savez\(path, v=np\.stack"):
            harness.load_guide(bad)
        with pytest.raises(ValueError, match="npz"):
            harness.save_guide(bad, {"v": v})
    with pytest.raises(ValueError, match=r"\[layers, g, g\]"):
        harness.save_guide(path, {"v": np.ones((2, 2, 3))})
    np.savez(tmp_path / "other.npz", w=v)
    with pytest.raises(ValueError, match="no array 'v'"):
        harness.load_guide(tmp_path / "other.npz")


def _detector(tmp_path, v=None, with_path=True):
    from dfd_clip_amd.detector import Detector
    path = tmp_path / "guide.npz"
    if v is not None:
        harness.save_guide(path, {"v": v})
    case = build_guide_case(path)
    if not with_path:
        del case["cfg"].train_mode.patch_mask["path"]
    return case, Detector(case["cfg"], case["T"], None, precision="fp32")


def test_detector_guide_needs_a_path_and_the_right_grid(tmp_path):
    with pytest.raises(ValueError, match="patch_mask.path"):
        _detector(tmp_path, with_path=False)
    with pytest.raises(ValueError, match="this model needs"):
        _detector(tmp_path, v=guide_map(2, 3))       # 3 x 3 where the tiny model has 2 x 2 patches
    with pytest.raises(ValueError, match="this model needs"):
        _detector(tmp_path, v=guide_map(1, 2))       # no map for tapped layer 1
    with pytest.raises(ValueError, match="npz"):
        from dfd_clip_amd.detector import Detector
        case = build_guide_case(tmp_path / "guide.pkl")
        Detector(case["cfg"], case["T"], None, precision="fp32")


def test_guide_draw_is_numpys_own(tmp_path):
    """With a fixed NumPy seed the layers' draws equal np.random.choice(..., p=...) called directly, in the reference's
    order, and equal the indices recorded when the reference's fixture was made."""
    g = load_golden(GUIDE_CASE)
    case, det = _detector(tmp_path, v=g["guide_v"])
    v = det.guide_map["v"]
    assert v.dtype == np.float64 and np.allclose(v, g["guide_v"], rtol=1e-15, atol=0)
    P = v.shape[1] * v.shape[2]
    num_select = int(P * case["cfg"].train_mode.patch_mask.ratio)
    for step in range(2):
        np.random.seed(EXTRA_INPUTS["np_seed"] + step)
        direct = [np.random.choice(range(P), num_select, replace=False, p=v[l].flatten()) for l in det.layer_indices]
        assert np.array_equal(np.asarray(direct), g["patch_indices"][step])
    # a stored map that is only nearly normalised is renormalised in float64, so np.random.choice accepts it
    _, det2 = _detector(tmp_path, v=g["guide_v"].astype(np.float32).astype(np.float64) * 3.0)
    np.random.choice(range(P), num_select, replace=False, p=det2.guide_map["v"][0].flatten())
