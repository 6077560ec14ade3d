"""CPU checks of the streaming path (dfd_clip_amd/stream.py, include/dfdclip_kvframes.h): the header against its ctypes table,
every host-side refusal and no-op of `dfd_kv_move_frames` (none of them launches, so none needs a GPU), `move_reference`
against a plain Python loop, `window_table`, and the ring bookkeeping of a frame store (`FrameRing`, which holds no device
memory)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.stream import FrameRing, FrameStore, StreamingVerdict, move_reference, window_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CTYPE = {"const void*": ctypes.c_void_p, "void*": ctypes.c_void_p, "const int32_t*": ctypes.c_void_p, "int": ctypes.c_int,
         "int64_t": ctypes.c_int64}


def test_header_matches_the_ctypes_table():
    text = open(os.path.join(ROOT, "include", "dfdclip_kvframes.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    protos = re.findall(r"\bint\s+(dfd_\w+)\s*\(([^)]*)\)\s*;", code)
    assert sorted(n for n, _ in protos) == sorted(capi.KVFRAMES_SIGNATURES) == ["dfd_kv_move_frames", "dfd_kv_move_last_path"]
    lib = capi.load_library()
    for name, params in protos:
        res, args = capi.KVFRAMES_SIGNATURES[name]
        assert res is ctypes.c_int and getattr(lib, name).argtypes == args
        types = [] if params.strip() == "void" else [" ".join(p.split()[:-1]) for p in params.split(",")]
        assert len(types) == len(args), name
        assert [CTYPE[t] for t in types] == args, name
    assert "DFD_ABI_VERSION" not in code
    defines = {n: int(v) for n, v in re.findall(r"#define (DFD_KVFRAMES_\w+) (\d+)", code)}
    assert defines == {"DFD_KVFRAMES_SRC_ONCE": capi.KVFRAMES_SRC_ONCE, "DFD_KVFRAMES_VEC16": capi.KVFRAMES_VEC16,
                       "DFD_KVFRAMES_ELEMENT": capi.KVFRAMES_ELEMENT}
    assert capi.ABI_VERSION == 17 and lib.dfd_abi_version() == 17


def test_the_table_is_disjoint_from_every_other():
    others = [capi.SIGNATURES, capi.EXT_SIGNATURES, capi.EXPLAIN_SIGNATURES, capi.AUGMENT_SIGNATURES, capi.ALIGN_SIGNATURES,
              capi.ELASTIC_SIGNATURES, capi.YUV_SIGNATURES, capi.SWIGLU_SIGNATURES, capi.KVGATHER_SIGNATURES, capi.EMA_SIGNATURES,
              capi.HOOK_SIGNATURES]
    for table in others:
        assert not set(table) & set(capi.KVFRAMES_SIGNATURES)


def test_build_lists_the_header_and_holds_the_kernels_to_zero_scratch():
    from dfd_clip_amd import build
    assert build.NO_SCRATCH["kv_frames.hip"] == "kv_frames_"
    src = open(os.path.join(ROOT, "dfd-clip_amd", "csrc", "kv_frames.hip")).read()
    names = set(re.findall(r"void (\w+_kernel)\(", src))
    assert names == {"kv_frames_vec16_kernel", "kv_frames_element_kernel"}
    assert all("kv_frames_" in n and "kv_gather_" not in n for n in names)
    assert "dfdclip_kvframes.h" in open(build.__file__).read() and "kv_frames.hip" in build.sources()


# ---- refusals and no-ops: all on the host, before any launch -------------------------------------------------------------

FAKE = 0x10000  # never dereferenced: every call below returns before a launch
GOOD = dict(k=FAKE, v=FAKE + 4096, k_out=FAKE + 8192, v_out=FAKE + 12288, dtype=capi.BF16, ssl=4 * 9 * 64, ssf=9 * 64, ssp=64,
            dsl=6 * 9 * 64, dsf=9 * 64, dsp=64, src=FAKE + 16384, dst=FAKE + 20480, L=2, n=4, Fs=4, Fd=6, P=9, D=64, flags=0)


def call(**over):
    a = dict(GOOD, **over)
    lib = capi.load_library()
    rc = lib.dfd_kv_move_frames(a["k"], a["v"], a["k_out"], a["v_out"], a["dtype"], a["ssl"], a["ssf"], a["ssp"], a["dsl"], a["dsf"],
                                a["dsp"], a["src"], a["dst"], a["L"], a["n"], a["Fs"], a["Fd"], a["P"], a["D"], a["flags"], None)
    return rc, lib.dfd_last_error().decode()


@pytest.mark.parametrize("over,word", [
    (dict(k=0), "null"), (dict(v=0), "null"), (dict(k_out=0), "null"), (dict(v_out=0), "null"),
    (dict(dtype=capi.FP8), "dtype"), (dict(dtype=7), "dtype"),
    (dict(L=-1), "negative"), (dict(n=-2), "negative"), (dict(P=-1), "negative"), (dict(D=-8), "negative"), (dict(Fs=-1), "negative"),
    (dict(Fd=-3), "negative"),
    (dict(ssl=-1), "source strides"), (dict(ssf=-1), "source strides"), (dict(ssp=63), "src_stride_patch"),
    (dict(dsl=-1), "destination strides"), (dict(dsf=-1), "destination strides"), (dict(dsp=63), "dst_stride_patch"),
    (dict(L=65536), "fit the grid"), (dict(n=1 << 29, P=8), "fit the grid"), (dict(n=1 << 40), "fit the grid"),
    (dict(D=1 << 30, ssp=1 << 30, dsp=1 << 30), "fit the grid"),
    (dict(Fs=0), "src_frames=0"), (dict(Fd=0), "dst_frames=0"), (dict(D=0), "D=0"),
    (dict(flags=2), "flag"), (dict(flags=-1), "flag"), (dict(flags=3), "flag"),
    (dict(src=0, n=5), "identity"), (dict(dst=0, n=7), "identity"),
])
def test_refusals_come_back_with_the_functions_name(over, word):
    rc, msg = call(**over)
    assert rc == -1 and "dfd_kv_move_frames" in msg and word in msg, (over, rc, msg)
    assert capi.load_library().dfd_kv_move_last_path() == 0


@pytest.mark.parametrize("over", [dict(L=0), dict(n=0), dict(P=0), dict(n=0, Fs=0, Fd=0), dict(L=0, n=0, P=0, D=0, ssp=0, dsp=0),
                                  dict(n=0, src=0, dst=0), dict(n=0, flags=1)])
def test_empty_calls_are_successful_no_ops(over):
    rc, msg = call(**over)
    assert rc == 0, (over, msg)
    assert capi.load_library().dfd_kv_move_last_path() == 0


def test_the_binding_refuses_host_tensors():
    k = torch.zeros(1, 2, 4, 8)
    with pytest.raises(capi.DfdError, match="device tensors"):
        capi.kv_move_frames(k, k, k.clone(), k.clone())


# ---- move_reference is the loop of the header ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("src,dst,Fs,Fd", [(None, [4, 0, 2], 3, 5), ([2, 2, 0, 1], None, 3, 4), ([1, 0], [0, 3], 2, 4), (None, None, 3, 3)])
def test_move_reference_is_the_plain_loop(dtype, src, dst, Fs, Fd):
    L, P, D = 2, 3, 5
    g = torch.Generator().manual_seed(Fs * 10 + Fd)
    buf = torch.randn(L, Fs, P + 1, 3 * D, generator=g).to(dtype)  # the in-place q|k|v layout
    k, v = buf[:, :, 1:, D:2 * D], buf[:, :, 1:, 2 * D:]
    pad = torch.full((2, L, Fd, P, D + 2), float("nan"), dtype=dtype)  # padded rows: the outputs are views too
    ko, vo = pad[0, ..., :D], pad[1, ..., :D]
    n = len(src) if src is not None else (len(dst) if dst is not None else Fs)
    want = pad.clone()
    for i in range(n):
        for l in range(L):
            for p in range(P):
                s, d = (i if src is None else src[i]), (i if dst is None else dst[i])
                want[0, l, d, p, :D] = k[l, s, p, :]
                want[1, l, d, p, :D] = v[l, s, p, :]
    to = lambda t: None if t is None else torch.tensor(t, dtype=torch.int32)
    got = move_reference(k, v, to(src), to(dst), ko, vo)
    assert got[0] is ko and got[1] is vo
    assert torch.equal(pad.view(torch.uint8), want.view(torch.uint8))  # NaN padding and unnamed frames included, bit for bit


# ---- window_table ----------------------------------------------------------------------------------------------------------

def test_window_table_hops_steps_and_tails():
    T = 4
    t = window_table(0, 11, T, 1)
    assert t.dtype == torch.int64 and tuple(t.shape) == (8, T)
    assert t.tolist() == [[s, s + 1, s + 2, s + 3] for s in range(8)]
    assert window_table(0, 11, T, 3)[:, 0].tolist() == [0, 3, 6]
    assert window_table(0, 11, T, T).tolist() == [[0, 1, 2, 3], [4, 5, 6, 7]]       # the reference's clips, ragged tail dropped
    assert window_table(0, 11, T, T + 2)[:, 0].tolist() == [0, 6]
    assert window_table(5, 16, T, 3)[:, 0].tolist() == [5, 8, 11]                   # a ring whose oldest frame is 5
    assert window_table(0, 11, T, 1, step=2).tolist() == [[s, s + 2, s + 4, s + 6] for s in range(5)]
    assert window_table(0, 11, T, 3, step=2)[:, 0].tolist() == [0, 3]
    # tails: "last" adds the window that ends on the last frame, only where the grid leaves frames uncovered
    assert window_table(0, 11, T, 3, tail="last")[:, 0].tolist() == [0, 3, 6, 7]
    assert window_table(0, 11, T, T, tail="last").tolist() == [[0, 1, 2, 3], [4, 5, 6, 7], [7, 8, 9, 10]]
    assert window_table(0, 12, T, T, tail="last")[:, 0].tolist() == [0, 4, 8]
    assert window_table(0, 10, T, 3, tail="last")[:, 0].tolist() == [0, 3, 6]
    assert window_table(0, 11, T, 3, tail="last", step=2).tolist()[-1] == [4, 6, 8, 10]
    assert window_table(0, 11, T, 1, tail="last").tolist() == t.tolist()
    for tail in ("drop", "last"):
        for count in (0, 1, T - 1):
            e = window_table(0, count, T, 2, tail=tail)
            assert tuple(e.shape) == (0, T) and e.dtype == torch.int64
        assert tuple(window_table(0, 6, T, 1, tail=tail, step=2).shape) == (0, T)  # four frames two apart span seven
    assert window_table(0, T, T, 9).tolist() == [[0, 1, 2, 3]]


@pytest.mark.parametrize("kw", [dict(hop=0), dict(hop=-1), dict(step=0), dict(tail="pad"), dict(tail=None)])
def test_window_table_raises(kw):
    with pytest.raises(ValueError, match="window_table"):
        window_table(0, 10, 4, **dict(dict(hop=1), **kw))


# ---- the ring --------------------------------------------------------------------------------------------------------------

def test_ring_arithmetic_eviction_and_validity():
    ring = FrameRing(capacity=7, num_frames=4, chunk=3)
    assert (ring.first, ring.count) == (0, 0) and not ring.valid.any()
    with pytest.raises(capi.DfdError, match="frame 3 is not pushed yet"):
        ring.check([[0, 1, 2, 3]])
    pushed = []
    for start in range(0, 14, 3):
        n = min(3, 14 - start)
        flags = [(start + i) % 5 != 0 for i in range(n)]
        slots, f = ring.reserve(n, flags)
        assert slots.dtype == np.int32 and slots.tolist() == [(start + i) % 7 for i in range(n)]
        assert (ring.first, ring.count) == (max(0, start - 7), start)  # reserve commits nothing
        got = ring.commit(slots, f)
        assert got == range(start, start + n)
        pushed += flags
        assert ring.count == start + n and ring.first == max(0, ring.count - 7)
        # what is retained carries its own flag, whichever slot it wrapped into
        kept = list(range(ring.first, ring.count))
        assert ring.mask(kept).tolist() == [pushed[a] for a in kept]
        assert ring.slots(kept).tolist() == [a % 7 for a in kept]
        table = window_table(ring.first, ring.count, 4, 1)
        assert ring.check(table).dtype == np.int64 and ring.mask(table).shape == tuple(table.shape)
        if ring.first > 0:
            with pytest.raises(capi.DfdError, match=f"frame {ring.first - 1} is evicted"):
                ring.check(table - 1)
        if table.numel():
            with pytest.raises(capi.DfdError, match=f"frame {ring.count} is not pushed yet"):
                ring.check(table + 1)
    assert (ring.first, ring.count) == (7, 14)
    assert ring.check(torch.zeros(0, 4, dtype=torch.int64)).shape == (0, 4)  # nothing named, nothing wrong


def test_ring_refusals():
    with pytest.raises(ValueError, match="capacity=6 is below num_frames \\+ encode_chunk = 4 \\+ 3"):
        FrameRing(6, 4, 3)
    with pytest.raises(ValueError):
        FrameRing(8, 4, 0)
    ring = FrameRing(7, 4, 3)
    with pytest.raises(ValueError, match="4 frames in one pass"):
        ring.reserve(4)
    with pytest.raises(ValueError, match="2 valid flags for 3 frames"):
        ring.reserve(3, [True, False])
    slots, flags = ring.reserve(2)  # no flags: every frame counts
    assert flags.tolist() == [True, True]
    assert ring.reserve(0)[0].shape == (0,)


class _Model:
    """What FrameStore looks at before it touches a device."""

    def __init__(self, ema, device="cpu"):
        from types import SimpleNamespace
        self.op_mode = type("Cfg", (dict,), {"__getattr__": dict.__getitem__})({"ema_frame": ema} if ema is not None else {})
        self.num_frames, self.layer_indices = 4, [0, 1]
        self.encoder = SimpleNamespace(tokens=5, width=128, act_dtype=torch.float32)
        self._p = torch.nn.Parameter(torch.zeros(1, device=device))

    def parameters(self):
        return iter([self._p])


def test_the_store_refuses_ema_frame_and_a_cpu_model_in_words():
    with pytest.raises(capi.DfdError, match="ema_frame.*depend on its clip"):
        FrameStore(_Model(0.9), 16)
    for ema in (None, 0, False):
        with pytest.raises(capi.DfdError, match="the model is on cpu"):
            FrameStore(_Model(ema), 16)
        with pytest.raises(capi.DfdError, match="the model is on cpu"):
            StreamingVerdict(_Model(ema), hop=2)
    with pytest.raises(ValueError, match="window_table: hop=0"):
        StreamingVerdict(_Model(None), hop=0)


def test_harness_exports_the_streaming_verdict():
    from dfd_clip_amd import harness
    import inspect
    assert harness.StreamingVerdict is StreamingVerdict
    sig = inspect.signature(harness.infer_raw_video).parameters
    assert sig["hop"].default is None and sig["tail"].default == "drop" and sig["encode_chunk"].default is None
    assert "single stream" in StreamingVerdict.__doc__.lower() and "fp8" in StreamingVerdict.__doc__
