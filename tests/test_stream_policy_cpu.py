"""The stream-policy switch on the host: include/dfdclip_hooks.h and capi.HOOK_SIGNATURES agree on its two entry points and
its family bits, `get` returns what `set` stored, and the switch is process-wide (another thread sees it).  No GPU."""
import ctypes
import os
import re
import threading

from dfd_clip_amd import capi
from dfd_clip_amd.build import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hooks_header():
    text = open(os.path.join(ROOT, "include", "dfdclip_hooks.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_and_ctypes_table_agree_on_the_hooks():
    text = _hooks_header()
    assert sorted(set(re.findall(r"\b(dfd_[a-z0-9_]+)\s*\(", text))) == sorted(capi.HOOK_SIGNATURES)
    assert re.search(r"unsigned\s+dfd_stream_policy_set\s*\(\s*unsigned\s+mask\s*\)", text)
    assert re.search(r"unsigned\s+dfd_stream_policy_get\s*\(\s*void\s*\)", text)
    assert capi.HOOK_SIGNATURES["dfd_stream_policy_set"] == (ctypes.c_uint, [ctypes.c_uint])
    assert capi.HOOK_SIGNATURES["dfd_stream_policy_get"] == (ctypes.c_uint, [])
    assert not {"dfd_stream_policy_set", "dfd_stream_policy_get"} & set(capi.SIGNATURES)
    bits = dict(re.findall(r"\b(DFD_STREAM_[A-Z_]+)\s*=\s*(\d+)", text))
    assert {k: int(v) for k, v in bits.items()} == {
        "DFD_STREAM_DECODER_KV": capi.STREAM_DECODER_KV, "DFD_STREAM_DECODER_WEIGHTS": capi.STREAM_DECODER_WEIGHTS,
        "DFD_STREAM_OPTIMIZER": capi.STREAM_OPTIMIZER, "DFD_STREAM_ENCODER_ROWS": capi.STREAM_ENCODER_ROWS,
        "DFD_STREAM_ALL": capi.STREAM_ALL}
    assert int(re.search(r"#define\s+DFD_STREAM_DEFAULT\s+(\d+)", text).group(1)) == capi.STREAM_DEFAULT


def test_get_returns_what_set_stored():
    build()
    lib = capi.load_library()
    assert hasattr(lib, "dfd_stream_policy_set") and hasattr(lib, "dfd_stream_policy_get")
    start = capi.stream_policy_get()
    try:
        assert start == capi.STREAM_DEFAULT
        for mask in (0, 1, 2, 4, 8, 5, capi.STREAM_ALL):
            before = capi.stream_policy_get()
            assert capi.stream_policy_set(mask) == before, "set returns the previous mask"
            assert capi.stream_policy_get() == mask
        capi.stream_policy_set(0xF0 | capi.STREAM_OPTIMIZER)
        assert capi.stream_policy_get() == capi.STREAM_OPTIMIZER, "bits that name no family are dropped"
        seen = []
        t = threading.Thread(target=lambda: seen.append(capi.stream_policy_get()))
        t.start()
        t.join()
        assert seen == [capi.STREAM_OPTIMIZER], "process-wide: the autograd thread launches under the same mask"
    finally:
        capi.stream_policy_set(start)
