"""`gather="table"` of the streaming path on the GPU (dfd_clip_amd/stream.py): the decoder reads the frame ring in place
through the windows' slot table instead of a gathered dense copy.  The setup is tests/test_hip_stream.py's: the `tiny` tower
(P = 4, D = 128, tapped layers [0, 1]), T = 4, seeded weights and frames, fp32 and bf16.

The table arm runs the kernels of the copy arm on the same rows in the same order, so every comparison between the two,
and with `predict` where the copy arm equals `predict`, is BIT FOR BIT: a derived bar."""
import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.stream import FrameStore, StreamingVerdict, window_table
from dfd_clip_amd.weights import synthetic_clips
from tests.test_hip_stream import RES, T, feed, model, same

pytestmark = pytest.mark.gpu

PRECISIONS = ["fp32", "bf16"]


def both(det, store, table):
    """-> {gather: (logits, video, [attention per layer])} of one window batch, cloned"""
    out = {}
    for g in ("copy", "table"):
        lg, ft = det.predict_windows(store, table, with_video_features=True, with_attention=True, gather=g)
        assert sorted(ft) == ["attention", "video"] and len(ft["attention"]) == store.layers
        out[g] = (lg[0].clone(), ft["video"].clone(), [a.clone() for a in ft["attention"]])
    return out


def assert_arms_equal(out, what):
    c, t = out["copy"], out["table"]
    assert same(c[0], t[0]), f"{what}: logits"
    assert same(c[1], t[1]), f"{what}: video features"
    assert all(same(a, b) for a, b in zip(c[2], t[2])), f"{what}: attention"


# ---- 1. aligned windows: both arms are predict, attention included ------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_aligned_windows_equal_predict_bit_for_bit_on_both_arms(precision):
    det = model(precision, False)
    B = 3
    x, m, _ = synthetic_clips(B, T, RES, seed=1234, masked_tail=True)
    x, m = x.cuda(), m.cuda()
    with torch.no_grad():
        want, feats = det.predict(x, m, with_video_features=True, with_attention=True)
    want, want_video, want_att = want[0].clone(), feats["video"].clone(), [a.clone() for a in feats["attention"]]
    store = FrameStore(det, B * T + T, encode_chunk=B * T)
    det.push_frames(store, x.flatten(0, 1), m.flatten())
    table = window_table(store.first, store.count, T, T)
    out = both(det, store, table)
    assert_arms_equal(out, f"{precision} aligned")
    heads, P = det.encoder.heads, store.patches
    for g, (lg, video, att) in out.items():
        assert same(lg, want) and same(video, want_video), g
        assert all(a.shape == (B, heads, T, P) and a.dtype == torch.float32 for a in att)
        assert all(same(a, b) for a, b in zip(att, want_att)), g
    # padded frames weigh exactly nothing
    pad = (~m)[:, None, :, None].expand(B, heads, T, P)
    assert all((a[pad] == 0).all() for a in out["table"][2]) and bool(pad.any())
    # without with_attention the logits are the same bits and nothing else comes back
    lg, ft = det.predict_windows(store, table, gather="table")
    assert ft == {} and same(lg[0], want)


def test_a_table_only_run_never_allocates_the_dense_buffer_and_launches_no_gather():
    det = model("bf16", False)
    N = 11
    frames, valid = feed(N)
    store = FrameStore(det, N + T, encode_chunk=N)
    det.push_frames(store, frames, valid)
    lib = capi.load_library()
    # the mover's last-path hook is per thread: 0 after a no-op call, and only a launch of the mover sets it again
    assert capi.kv_move_last_path() == capi.KVFRAMES_VEC16  # (the ingest above)
    k = store.k
    rc = lib.dfd_kv_move_frames(k.data_ptr(), store.v.data_ptr(), k.data_ptr(), store.v.data_ptr(), capi._DTYPE[k.dtype], k.stride(0), k.stride(1),
                                k.stride(2), k.stride(0), k.stride(1), k.stride(2), None, None, store.layers, 0, store.capacity, store.capacity,
                                store.patches, store.width, 0, capi._stream())
    assert rc == 0 and capi.kv_move_last_path() == 0  # n = 0: the ABI's no-op
    for g in ("table", "auto"):
        lg, ft = det.predict_windows(store, window_table(0, N, T, 1), with_video_features=True, with_attention=True, gather=g)
        assert store._dense is None and capi.kv_move_last_path() == 0, g
    det.predict_windows(store, window_table(0, N, T, 1))
    assert store._dense is not None and capi.kv_move_last_path() == capi.KVFRAMES_VEC16
    assert lib.dfd_abi_version() == 17


# ---- 2. overlapping windows ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_overlapping_windows_at_hop_one(precision):
    det = model(precision, False)
    N = 11
    frames, valid = feed(N)
    store = FrameStore(det, N + T, encode_chunk=N)
    det.push_frames(store, frames, valid)
    table = window_table(0, N, T, 1)
    assert table.shape[0] == 8
    out = both(det, store, table)
    assert_arms_equal(out, f"{precision} N = 11 at hop 1")
    assert not same(out["table"][0][0], out["table"][0][1])  # (windows one frame apart are different windows)
    # the windows in another order: every row follows its window
    flipped = both(det, store, table.flip(0))
    assert_arms_equal(flipped, f"{precision} flipped")


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_ring_of_seven_slots_fed_in_chunks_of_three(precision):
    """windows cross the ring's end: the table arm on the ring of T + 3 slots, the copy arm on it and on a store of 14"""
    det = model(precision, False)
    N, chunk = 14, 3
    frames, valid = feed(N)
    small, big = FrameStore(det, T + chunk, encode_chunk=chunk), FrameStore(det, N, encode_chunk=chunk)
    done, wrapped = 0, 0
    for f0 in range(0, N, chunk):
        for store in (small, big):
            det.push_frames(store, frames[f0:f0 + chunk], valid[f0:f0 + chunk])
        table = window_table(0, small.count, T, 1)[done:]
        if table.shape[0]:
            slots = small.slots(table)
            wrapped += int((np.diff(slots, axis=1) < 0).any(axis=1).sum())
            a, b = both(det, small, table), both(det, big, table)
            assert_arms_equal(a, f"{precision} ring, frames to {small.count}")
            assert_arms_equal(b, f"{precision} store of 14, frames to {small.count}")
            assert_arms_equal({"copy": b["copy"], "table": a["table"]}, f"{precision} ring's table arm against the store's copy arm")
            done += table.shape[0]
    assert done == N - T + 1 and wrapped >= 3
    with pytest.raises(capi.DfdError, match="frame 6 is evicted"):
        det.predict_windows(small, [[6, 7, 8, 9]], gather="table")


# ---- 4. StreamingVerdict and infer_raw_video -----------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_streaming_verdict_yields_the_rows_of_copy_whatever_the_slicing(precision):
    det = model(precision, False)
    N = 14
    frames, valid = feed(N)
    runs = {}
    for g, cuts in (("copy", [N]), ("table", [1] * N), ("table", [5, 9]), ("table", [N]), ("auto", [5, 9])):
        sv = StreamingVerdict(det, hop=2, encode_chunk=2, gather=g)
        assert sv.gather == ("copy" if g == "copy" else "table")
        out, f0 = [], 0
        for c in cuts:
            out += sv.push(frames[f0:f0 + c], valid[f0:f0 + c])
            f0 += c
        assert sv.flush() == []
        if g != "copy":
            assert sv.store._dense is None
        runs[(g, tuple(cuts))] = (out, sv.result(with_logits=True), sv.starts)
    base = runs[("copy", (N,))]
    assert base[2] == [0, 2, 4, 6, 8, 10]
    for key, (out, res, starts) in runs.items():
        assert starts == base[2] and [s for s, _ in out] == starts, key
        assert same(torch.stack([r for _, r in out]), torch.stack([r for _, r in base[0]])), key
        assert all(same(a, b) for a, b in zip(res, base[1])), key


@pytest.mark.parametrize("precision", PRECISIONS)
def test_infer_raw_video_with_the_table_equals_hop_none(precision):
    from dfd_clip_amd import align as AL
    from dfd_clip_amd.harness import infer_raw_video
    from tests import align_cases as C
    det = model(precision, False)
    F, H, Wd = 2 * T + 3, 150, 190
    ref = C.mean_face()
    frames = C.smooth_hwc(F, H, Wd, seed=37)
    lm = np.stack([C.apply_affine(AL.invert_affine(C.centred(1.4 + 0.02 * f, 0.03 * f - 0.1, (H, Wd), shift=(3.0 * f - 10, 6 - f))), ref)
                   for f in range(F)])
    lm[5] = lm[9] = np.nan
    aligner = AL.FaceAligner(ref, border=0)
    dev = torch.from_numpy(frames).cuda()
    for bs in (16, 1):
        base = infer_raw_video(det, dev, lm, aligner, batch_size=bs, with_logits=True)
        tab = infer_raw_video(det, dev, lm, aligner, batch_size=bs, with_logits=True, hop=T, encode_chunk=bs * T, gather="table")
        assert tuple(base[2].shape) == (2, 2) and all(same(a, b) for a, b in zip(base, tab)), bs
    copy1 = infer_raw_video(det, dev, lm, aligner, batch_size=1, with_logits=True, hop=1, encode_chunk=T)
    tab1 = infer_raw_video(det, dev, lm, aligner, batch_size=1, with_logits=True, hop=1, encode_chunk=T, gather="table")
    assert tuple(tab1[2].shape) == (F - T + 1, 2) and all(same(a, b) for a, b in zip(copy1, tab1))


# ---- 5. where the table is not allowed -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,kind", [("fp32", "adapter"), ("bf16", "adapter"), ("fp32", "attn_mode"), ("bf16", "attn_mode")])
def test_table_is_refused_in_words_and_auto_is_copy(precision, kind):
    det = model(precision, True) if kind == "adapter" else model(precision, False, op_mode__attn_mode="frame+temporal")
    words = "gather='table': the model has an adapter" if kind == "adapter" else r"gather='table': op_mode\.attn_mode"
    N = 9
    frames, valid = feed(N)
    store = FrameStore(det, N + T, encode_chunk=N)
    det.push_frames(store, frames, valid)
    table = window_table(0, N, T, 2)
    with pytest.raises(capi.DfdError, match=words):
        det.predict_windows(store, table, gather="table")
    with pytest.raises(capi.DfdError, match=words):
        StreamingVerdict(det, hop=2, gather="table")
    with pytest.raises(ValueError, match="'copy', 'table' or 'auto'"):
        det.predict_windows(store, table, gather="tabled")
    assert store._dense is None
    out = {}
    for g in ("copy", "auto"):
        lg, ft = det.predict_windows(store, table, with_video_features=True, with_attention=True, gather=g)
        out[g] = (lg[0].clone(), ft["video"].clone(), [a.clone() for a in ft["attention"]])
    assert same(out["copy"][0], out["auto"][0]) and same(out["copy"][1], out["auto"][1])
    assert all(same(a, b) for a, b in zip(out["copy"][2], out["auto"][2]))
    W, heads, P = table.shape[0], det.encoder.heads, store.patches
    assert all(a.shape == (W, heads, T, P) and torch.isfinite(a).all() for a in out["copy"][2])
    assert StreamingVerdict(det, hop=2, gather="auto").gather == "copy"
    # the decoder itself refuses a table where it cannot follow one
    slots = torch.from_numpy(store.slots(table).reshape(-1)).cuda()
    m = torch.from_numpy(store.mask(table)).cuda()
    if kind == "attn_mode":
        with pytest.raises(capi.DfdError, match="attn_mode"), torch.no_grad():
            det.decoder.run((store.k, store.v, det.decoder.temporal_pos(), slots), m)


def test_the_autograd_path_refuses_a_table():
    det = model("fp32", False)
    N = 8
    frames, valid = feed(N)
    store = FrameStore(det, N + T, encode_chunk=N)
    det.push_frames(store, frames, valid)
    table = window_table(0, N, T, T)
    slots = torch.from_numpy(store.slots(table).reshape(-1)).cuda()
    m = torch.from_numpy(store.mask(table)).cuda()
    kvs = (store.k, store.v, det.decoder.temporal_pos(), slots)
    assert any(p.requires_grad for p in det.decoder.parameters())
    with pytest.raises(capi.DfdError, match="autograd path"):
        det.decoder.run(kvs, m)
    with torch.no_grad():  # the same call without grad is predict_windows' own
        _, video, logits = det.decoder.run(kvs, m)
    want, ft = det.predict_windows(store, table, with_video_features=True)
    assert same(logits[0], want[0]) and same(video, ft["video"])
