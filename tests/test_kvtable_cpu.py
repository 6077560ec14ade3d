"""CPU checks of the decoder attention over a frame store (include/dfdclip_kvtable.h, dfd_clip_amd/stream.py): the header
against its ctypes table, the host-side refusals of the two entry points (none of them launches, so none needs a GPU),
`choose_gather` over every combination, `table_reference` against a plain Python loop, and the four-element form of
`Decoder._unpack`."""
import ctypes
import inspect
import itertools
import os
import re
from types import SimpleNamespace

import pytest
import torch

from dfd_clip_amd import capi, stream
from dfd_clip_amd.stream import choose_gather, table_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "const float*": ctypes.c_void_p,
         "float*": ctypes.c_void_p, "const uint8_t*": ctypes.c_void_p, "const dfd_kv_layout_t*": ctypes.c_void_p, "int": ctypes.c_int}
NAMES = ["dfd_decoder_attn_fwd_frames", "dfd_decoder_attn_map_frames"]
INVALID_ARG = -1  # DFD_ERR_INVALID_ARG of dfdclip.h


def prototypes(header):
    text = open(os.path.join(ROOT, "include", header)).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return text, code, {n: [" ".join(p.split()[:-1]) for p in params.split(",")]
                        for n, params in re.findall(r"\bint\s+(dfd_\w+)\s*\(([^)]*)\)\s*;", code)}


def test_header_matches_the_ctypes_table():
    text, code, protos = prototypes("dfdclip_kvtable.h")
    assert sorted(protos) == sorted(capi.KVTABLE_SIGNATURES) == NAMES
    lib = capi.load_library()
    for name, types in protos.items():
        res, args = capi.KVTABLE_SIGNATURES[name]
        assert res is ctypes.c_int and getattr(lib, name).argtypes == args
        assert [CTYPE[t] for t in types] == args, name
    assert "DFD_ABI_VERSION" not in code and capi.ABI_VERSION == 17 and lib.dfd_abi_version() == 17
    # what the header has to say in words
    flat = " ".join(re.sub(r"^\s*/?\*+\s?", "", line) for line in text.splitlines())
    flat = " ".join(flat.split())
    for phrase in ("clamped to [0, store_frames)", "formed in 64 bits", "Nothing outside mix, mix_softmax (when given), stats and the workspace is written",
                   "Nothing outside aff and branches (when given) is written", "null frame_table, store_frames <= 0"):
        assert phrase in flat, phrase


def test_the_frames_entry_points_take_the_untabled_arguments_plus_two():
    """... in the untabled order, with `frame_table, store_frames` in front of `stream`"""
    _, _, tabled = prototypes("dfdclip_kvtable.h")
    _, _, explain = prototypes("dfdclip_explain.h")
    _, _, abi = prototypes("dfdclip.h")
    for name, plain in (("dfd_decoder_attn_fwd_frames", abi["dfd_decoder_attn_fwd"]), ("dfd_decoder_attn_map_frames", explain["dfd_decoder_attn_map"])):
        assert tabled[name] == plain[:-1] + ["const int32_t*", "int"] + plain[-1:], name
    fwd, fwd_t = capi.SIGNATURES["dfd_decoder_attn_fwd"][1], capi.KVTABLE_SIGNATURES["dfd_decoder_attn_fwd_frames"][1]
    amap, amap_t = capi.EXPLAIN_SIGNATURES["dfd_decoder_attn_map"][1], capi.KVTABLE_SIGNATURES["dfd_decoder_attn_map_frames"][1]
    assert fwd_t == fwd[:-1] + [ctypes.c_void_p, ctypes.c_int] + fwd[-1:] and amap_t == amap[:-1] + [ctypes.c_void_p, ctypes.c_int] + amap[-1:]


def test_the_table_is_loaded_and_shares_no_symbol():
    others = [capi.SIGNATURES, capi.EXT_SIGNATURES, capi.EXPLAIN_SIGNATURES, capi.AUGMENT_SIGNATURES, capi.ALIGN_SIGNATURES,
              capi.ELASTIC_SIGNATURES, capi.YUV_SIGNATURES, capi.SWIGLU_SIGNATURES, capi.KVGATHER_SIGNATURES, capi.KVFRAMES_SIGNATURES,
              capi.EMA_SIGNATURES, capi.HOOK_SIGNATURES]
    for table in others:
        assert not set(table) & set(capi.KVTABLE_SIGNATURES)
    assert "KVTABLE_SIGNATURES" in inspect.getsource(capi.load_library)


def test_build_lists_the_header():
    from dfd_clip_amd import build
    assert "dfdclip_kvtable.h" in open(build.__file__).read()


# ---- refusals of the library: all on the host, before any launch -----------------------------------------------------------

def _fwd_args(**over):
    """arguments of dfd_decoder_attn_fwd_frames that pass every check (the pointers are never followed: B = 0 returns first)"""
    a = dict(q=64, k=64, v=64, dtype=capi._DTYPE[torch.float32], layout=None, mask=64, ext=None, mix=64, mix_s=None, stats=64, ws=64,
             splits=1, B=0, T=2, P=3, H=1, d=64, table=64, frames=5, stream=None)
    a.update(over)
    return list(a.values())


def _map_args(**over):
    a = dict(q=64, k=64, dtype=capi._DTYPE[torch.float32], layout=None, mask=64, stats=64, ext=None, aff=64, branches=None, B=0, T=2, P=3,
             H=1, d=64, table=64, frames=5, stream=None)
    a.update(over)
    return list(a.values())


def test_library_refusals_and_the_empty_batch():
    lib = capi.load_library()
    err = lambda: lib.dfd_last_error().decode()
    for fn, args, name in ((lib.dfd_decoder_attn_fwd_frames, _fwd_args, "dfd_decoder_attn_fwd_frames"),
                           (lib.dfd_decoder_attn_map_frames, _map_args, "dfd_decoder_attn_map_frames")):
        assert fn(*args()) == 0  # B == 0: a successful no-op
        assert fn(*args(table=None)) == INVALID_ARG and err() == f"{name}: null frame table"
        for frames in (0, -1):
            assert fn(*args(frames=frames)) == INVALID_ARG and f"{name}: store_frames={frames}" in err()
        # check_decoder_attn's refusals, in its words under this entry point's name
        assert fn(*args(q=None)) == INVALID_ARG and err() == f"{name}: null pointer"
        assert fn(*args(d=32)) == INVALID_ARG and err() == f"{name}: head dim 32, only 64 is supported"
        assert fn(*args(T=0)) == INVALID_ARG and err() == f"{name}: bad shape"
        assert fn(*args(H=200)) == INVALID_ARG and "bad shape" in err()
        assert fn(*args(dtype=capi.FP8)) == INVALID_ARG and err().startswith(f"{name}: kv_dtype=")
        assert fn(*args(k=68)) == INVALID_ARG and err() == f"{name}: pointers must be 16-byte aligned"
        lay = capi.KvLayoutDesc(63, 192, None)
        assert fn(*args(layout=ctypes.byref(lay))) == INVALID_ARG and f"{name}: key/value layout: row stride 63" in err()
    assert lib.dfd_decoder_attn_fwd_frames(*_fwd_args(splits=0)) == INVALID_ARG and err() == "dfd_decoder_attn_fwd_frames: splits=0"
    assert lib.dfd_decoder_attn_fwd_frames(*_fwd_args(splits=4096, H=16)) == INVALID_ARG and "needs 262144 B of LDS to merge" in err()
    # the untabled entry points keep their own names in the same refusals
    assert lib.dfd_decoder_attn_fwd(*_fwd_args(splits=0)[:-3], None) == INVALID_ARG and err() == "dfd_decoder_attn_fwd: splits=0"
    assert lib.dfd_decoder_attn_map(*_map_args(d=32)[:-3], None) == INVALID_ARG and err() == "dfd_decoder_attn_map: head dim 32, only 64 is supported"


def test_the_binding_refuses_cpu_tensors():
    q, k, t = torch.zeros(1, 128), torch.zeros(3, 2, 64), torch.zeros(2, dtype=torch.int32)
    m, o = torch.ones(1, 2, dtype=torch.uint8), torch.zeros(1, 64)
    with pytest.raises(capi.DfdError, match="device tensors"):
        capi.decoder_attn_fwd_frames(q, k, k, t, m, o, torch.zeros(1, 1, 2), torch.zeros(130), 1, 1, 2, 2, 1)
    with pytest.raises(capi.DfdError, match="device tensors"):
        capi.decoder_attn_map_frames(q, k, t, m, torch.zeros(1, 1, 2), torch.zeros(1, 1, 4), 1, 2, 2, 1)


# ---- choose_gather -----------------------------------------------------------------------------------------------------------

def test_choose_gather_over_every_combination():
    for requested, has_adapter, modes in itertools.product(("copy", "table", "auto"), (False, True), (0, 1, 2, 3)):
        allowed = not has_adapter and modes == 0
        if requested == "copy":
            assert choose_gather(requested, has_adapter, modes) == "copy"
        elif allowed:
            assert choose_gather(requested, has_adapter, modes) == "table"
        elif requested == "auto":
            assert choose_gather(requested, has_adapter, modes) == "copy"
        else:
            # the adapter is named first when both stand in the way
            words = "the model has an adapter.*positional embedding" if has_adapter else "op_mode\\.attn_mode.*reads no frame table"
            with pytest.raises(capi.DfdError, match="gather='table': " + words):
                choose_gather(requested, has_adapter, modes)
    for bad in ("gather", None, "TABLE", 1):
        with pytest.raises(ValueError, match="'copy', 'table' or 'auto'"):
            choose_gather(bad, False, 0)


def test_defaults_do_not_move():
    from dfd_clip_amd import harness
    from dfd_clip_amd.detector import Detector
    for fn in (stream.predict_windows, Detector.predict_windows, stream.StreamingVerdict.__init__, harness.infer_raw_video):
        assert inspect.signature(fn).parameters["gather"].default == "copy", fn
    for fn in (stream.predict_windows, Detector.predict_windows):
        sig = inspect.signature(fn).parameters
        assert sig["with_attention"].default is False and sig["with_video_features"].default is False
        assert list(sig)[-3:] == ["with_video_features", "with_attention", "gather"]


# ---- table_reference is the indexing of the header ---------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("slots", [[0, 1, 2, 3], [4, 4, 4], [3, 0, 4, 1, 1, 2], [-3, 5, 7, 2], []])
def test_table_reference(dtype, slots):
    C, P, D = 5, 3, 8
    g = torch.Generator().manual_seed(5)
    whole = torch.randn(C, P + 1, 3 * D, generator=g).to(dtype)
    k_view, v_view = whole[:, 1:, D:2 * D], whole[:, 1:, 2 * D:]  # the in-place view: row stride 3D, frame stride tokens*3D
    for k, v in ((k_view, v_view), (k_view.contiguous(), v_view.contiguous())):
        rk, rv = table_reference(k, v, torch.tensor(slots, dtype=torch.int32))
        assert rk.shape == rv.shape == (len(slots), P, D) and rk.is_contiguous() and rv.is_contiguous() and rk.dtype == dtype
        for i, s in enumerate(slots):
            c = min(max(s, 0), C - 1)
            for p in range(P):
                assert torch.equal(rk[i, p], whole[c, 1 + p, D:2 * D]) and torch.equal(rv[i, p], whole[c, 1 + p, 2 * D:])
        assert table_reference(k, None, slots)[1] is None and torch.equal(table_reference(k, None, slots)[0], rk)


# ---- Decoder._unpack ---------------------------------------------------------------------------------------------------------

def test_unpack_takes_the_four_form_and_still_wants_device_tensors():
    from dfd_clip_amd.decoder import Decoder
    me = SimpleNamespace(layer_indices=[0, 1], width=128)
    k = torch.zeros(2, 7, 4, 128)
    slots = torch.zeros(8, dtype=torch.int32)
    m = torch.ones(2, 4, dtype=torch.bool)
    for kvs in ((k, k, None, slots), (k, k, torch.zeros(4, 128), slots)):
        with pytest.raises(capi.DfdError, match="HIP kernels only"):
            Decoder._unpack(me, kvs, m)
    with pytest.raises(ValueError):  # five elements are no form
        Decoder._unpack(me, (k, k, None, slots, None), m)
