"""The streaming path on the GPU (dfd_clip_amd/stream.py): `Detector.push_frames` / `predict_windows` over a `FrameStore`,
`StreamingVerdict` and `harness.infer_raw_video(hop=)` against `Detector.predict` on the same frames.

The `tiny` tower (P = 4, D = 128, tapped layers [0, 1]), T = 4, seeded weights and frames, fp32 and bf16, without an adapter and
with "768-x-768-z0" (x = 64), eval mode.  Where the new path runs the same kernels on the same rows as `predict` the
results are compared BIT FOR BIT.  Where it cannot (a tower pass over N frames against one over W*T materialised rows) the
bar is what `predict` itself moves by when only the size of its tower passes changes (`encoder.frame_chunk`), measured in
the same process on the same clips; where that is zero, bit identity is demanded.  Every figure is printed before it is held."""
import functools

import numpy as np
import pytest
import torch

from dfd_clip_amd import capi
from dfd_clip_amd.stream import FrameStore, StreamingVerdict, move_reference, window_table
from dfd_clip_amd.weights import ARCHS, random_state_dict, synthetic_clips
from tests.cases import make_config

pytestmark = pytest.mark.gpu

T = 4
RES = ARCHS["tiny"][0]
Z0 = {"type": "768-x-768-z0", "x": 64}
CONFIGS = [(p, a) for p in ("fp32", "bf16") for a in (False, True)]
IDS = [f"{p}-{'z0' if a else 'noadapter'}" for p, a in CONFIGS]


@functools.lru_cache(maxsize=None)
def model(precision, adapter, **extra):
    from dfd_clip_amd.detector import Detector
    over = dict(decode_mode="index", decode_indices=[0, 1], **extra)
    if adapter:
        over.update(adapter__type="normal", adapter__frozen=0, adapter__struct=dict(Z0))
    cfg = make_config("tiny", **over)
    det = Detector(cfg, T, None, precision=precision)
    det.load_state_dict(random_state_dict(cfg, T, seed=0))
    return det.cuda().eval()


@functools.lru_cache(maxsize=None)
def feed(n, seed=77):
    """n seeded frames [n,3,R,R] on the device and their flags (every fifth frame from the third has no face)."""
    x = synthetic_clips(1, n, RES, seed=seed, masked_tail=False)[0][0]
    valid = np.array([i % 5 != 2 for i in range(n)])
    return x.cuda(), valid


def bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.uint8)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a.cpu()), bits(b.cpu()))


def gap(a, b):
    return (a.double() - b.double()).abs().max().item()


def chunk_gap(det, x, m):
    """What `predict` on these clips moves by when only the rows per tower pass change (frame_chunk 0: one pass; T: one per
    clip): -> (logits gap, video-feature gap)."""
    keep = det.encoder.frame_chunk
    try:
        outs = []
        for fc in (0, T):
            det.encoder.frame_chunk = fc
            with torch.no_grad():
                lg, ft = det.predict(x, m, with_video_features=True)
            outs.append((lg[0].clone(), ft["video"].clone()))
    finally:
        det.encoder.frame_chunk = keep
    return gap(outs[0][0], outs[1][0]), gap(outs[0][1], outs[1][1])


def hold(name, got, want, bar):
    g = gap(got, want)
    print(f"{name}: max |d| {g:.3e}, bar {bar:.3e}")
    if bar == 0.0:
        assert same(got, want), f"{name}: bit identity demanded (the bar is zero), max |d| {g:.3e}"
    else:
        assert g <= bar, (name, g, bar)


# ---- 1. aligned windows are predict ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,adapter", CONFIGS, ids=IDS)
def test_aligned_windows_equal_predict_bit_for_bit(precision, adapter):
    """The B*T frames of three clips (clip 1 with a masked tail) pushed in one call, read back through the hop = T table: the
    tower pass has predict's row count, the stored rows are its rows, the adapter and decoder calls are its calls."""
    det = model(precision, adapter)
    B = 3
    x, m, _ = synthetic_clips(B, T, RES, seed=1234, masked_tail=True)
    x, m = x.cuda(), m.cuda()
    with torch.no_grad():
        want, feats = det.predict(x, m, with_video_features=True)
    want, want_video = want[0].clone(), feats["video"].clone()
    store = FrameStore(det, B * T + T, encode_chunk=B * T)
    got_range = det.push_frames(store, x.flatten(0, 1), m.flatten())
    assert got_range == range(0, B * T) and (store.first, store.count) == (0, B * T)
    assert capi.kv_move_last_path() == capi.KVFRAMES_VEC16
    table = window_table(store.first, store.count, T, T)
    assert tuple(table.shape) == (B, T)
    got, feats = det.predict_windows(store, table, with_video_features=True)
    assert capi.kv_move_last_path() == capi.KVFRAMES_VEC16
    print(f"logits gap {gap(got[0], want):.3e}, video gap {gap(feats['video'], want_video):.3e}")
    if not adapter:  # the stored rows are the rows of predict's in-place pass (its persistent set is still there)
        kv = det._kv_static[1][0]
        D = store.width
        assert same(store.k[:, :B * T], kv[:, :, 1:, D:2 * D]) and same(store.v[:, :B * T], kv[:, :, 1:, 2 * D:])
    assert same(got[0], want) and same(feats["video"], want_video)
    assert det.predict_windows(store, table)[1] == {}
    # the same logits from the windows in another order, one at a time (the mask travels with the frame)
    again = det.predict_windows(store, table.flip(0))[0][0]
    assert gap(again.flip(0), want) <= (1e-3 if precision == "fp32" else 5e-2)


# ---- 2. overlapping windows --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,adapter", CONFIGS, ids=IDS)
def test_overlapping_windows(precision, adapter):
    det = model(precision, adapter)
    N = 11
    frames, valid = feed(N)
    store = FrameStore(det, N + T, encode_chunk=N)
    det.push_frames(store, frames, valid)
    table = window_table(0, N, T, 1)
    W = table.shape[0]
    assert W == 8
    got, feats = det.predict_windows(store, table, with_video_features=True)
    got, got_video = got[0].clone(), feats["video"].clone()
    # (a) the decoder (after the adapter) on move_reference's rows of the same store, same W: bit for bit
    L, P, D = store.layers, store.patches, store.width
    rk, rv = (torch.full((L, W * T, P, D), float("nan"), device="cuda", dtype=store.dtype) for _ in range(2))
    move_reference(store.k, store.v, torch.from_numpy(store.slots(table).reshape(-1)), None, rk, rv)
    m = torch.from_numpy(valid[table.numpy()]).cuda()
    pos = det.decoder.temporal_pos()
    with torch.no_grad():
        kv = (rk, rv, pos) if not adapter else det.adapter.run(rk.view(L, W * T * P, D), rv.view(L, W * T * P, D), T, pos, None)
        _, ref_video, ref = det.decoder.run(kv, m, None)
    assert same(got, ref[0]) and same(got_video, ref_video)
    # (b) predict on the materialised windows: the tower over W*T rows instead of N
    x = frames[table.cuda()]
    assert tuple(x.shape) == (W, T, 3, RES, RES)
    bar_logits, bar_video = chunk_gap(det, x, m)
    with torch.no_grad():
        want, feats = det.predict(x, m, with_video_features=True)
    hold(f"{precision} {'z0' if adapter else 'noadapter'} logits vs predict(frames[table])", got, want[0], bar_logits)
    hold(f"{precision} {'z0' if adapter else 'noadapter'} video vs predict(frames[table])", got_video, feats["video"], bar_video)
    assert not same(got[0], got[1])  # (windows one frame apart are different windows)


# ---- 3. the ring ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,adapter", [("fp32", False), ("bf16", True)], ids=["fp32-noadapter", "bf16-z0"])
def test_a_ring_of_seven_slots_decodes_what_a_store_of_fourteen_does(precision, adapter):
    det = model(precision, adapter)
    N, chunk = 14, 3
    frames, valid = feed(N)
    small, big = FrameStore(det, T + chunk, encode_chunk=chunk), FrameStore(det, N, encode_chunk=chunk)
    done = 0
    for f0 in range(0, N, chunk):
        for store in (small, big):
            got = det.push_frames(store, frames[f0:f0 + chunk], valid[f0:f0 + chunk])
            assert got == range(f0, min(N, f0 + chunk))
        assert small.first == max(0, small.count - (T + chunk)) and big.first == 0
        table = window_table(0, small.count, T, 1)[done:]  # every window this pass completed, decoded at once
        if table.shape[0]:
            a = det.predict_windows(small, table, with_video_features=True)
            a = (a[0][0].clone(), a[1]["video"].clone())
            b = det.predict_windows(big, table, with_video_features=True)
            assert same(a[0], b[0][0]) and same(a[1], b[1]["video"]), (f0, table[:, 0].tolist())
            done += table.shape[0]
    assert done == N - T + 1 and (small.first, small.count) == (N - T - chunk, N)
    assert same(small.k[:, torch.from_numpy(small.slots(range(7, 14))).long().cuda()], big.k[:, 7:14])
    with pytest.raises(capi.DfdError, match="frame 6 is evicted"):
        det.predict_windows(small, [[6, 7, 8, 9]])
    with pytest.raises(capi.DfdError, match="frame 14 is not pushed yet"):
        det.predict_windows(small, [[11, 12, 13, 14]])
    assert det.predict_windows(big, [[6, 7, 8, 9]])[0][0].shape == (1, 2)


# ---- 4. push granularity --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision,adapter", [("fp32", True), ("bf16", False)], ids=["fp32-z0", "bf16-noadapter"])
def test_the_verdict_does_not_depend_on_how_pushes_are_sliced(precision, adapter):
    det = model(precision, adapter)
    N = 14
    frames, valid = feed(N)
    runs = []
    for cuts in ([1] * N, [5, 9], [N]):
        sv = StreamingVerdict(det, hop=2, encode_chunk=2)
        out, f0 = [], 0
        for c in cuts:
            out += sv.push(frames[f0:f0 + c], valid[f0:f0 + c])
            f0 += c
        assert sv.flush() == [] and sv.store.count == N  # 14 frames are seven passes of two: nothing is pending
        runs.append((out, sv.result(with_logits=True), sv.starts))
    starts = [0, 2, 4, 6, 8, 10]
    for out, res, st in runs:
        assert [s for s, _ in out] == starts == st
        assert all(row.device.type == "cpu" and row.shape == (2,) for _, row in out)
        assert same(torch.stack([r for _, r in out]), torch.stack([r for _, r in runs[0][0]]))
        assert all(same(a, b) for a, b in zip(res, runs[0][1]))
        assert same(res[2], torch.stack([r for _, r in out])) and same(res[1], res[2].softmax(dim=-1)) and same(res[0], res[1].mean(dim=0)[1])
    # tails on 13 frames: the grid ends on frame 11.  "drop" never encodes frame 12; "last" adds exactly the window 9..12
    for tail in ("drop", "last"):
        sv = StreamingVerdict(det, hop=2, encode_chunk=2, tail=tail)
        out = sv.push(frames[:13], valid[:13])
        assert [s for s, _ in out] == [0, 2, 4, 6, 8] and sv.store.count == 12
        assert same(torch.stack([r for _, r in out]), torch.stack([r for _, r in runs[0][0][:5]]))
        extra = sv.flush()
        if tail == "drop":
            assert extra == [] and sv.store.count == 12
        else:
            assert [s for s, _ in extra] == [9] and sv.store.count == 13 and sv.starts == [0, 2, 4, 6, 8, 9]
            want = det.predict_windows(sv.store, [[9, 10, 11, 12]])[0][0][0].cpu()
            assert same(extra[0][1], want)
        assert sv.flush() == []
        with pytest.raises(capi.DfdError, match="closed"):
            sv.push(frames[:1])
    with pytest.raises(ValueError, match="no window"):
        StreamingVerdict(det, hop=2).result()


# ---- 5. infer_raw_video ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_infer_raw_video_with_a_hop(precision):
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
    for bs in (16, 1):  # one tower pass for the video; one per clip
        base = infer_raw_video(det, dev, lm, aligner, batch_size=bs, with_logits=True)
        hopT = infer_raw_video(det, dev, lm, aligner, batch_size=bs, with_logits=True, hop=T, encode_chunk=bs * T)
        assert tuple(base[2].shape) == (2, 2)
        assert all(same(a, b) for a, b in zip(base, hopT)), (bs, gap(base[2], hopT[2]))
        assert all(same(a, b) for a, b in zip(hopT, infer_raw_video(det, dev, lm, aligner, batch_size=bs, with_logits=True, hop=T)))
    # hop = 1 at batch_size 1 and passes of T frames: windows 0 and T read the rows of predict's own per-clip passes and are
    # decoded alone, as predict decodes its clips there
    base = infer_raw_video(det, dev, lm, aligner, batch_size=1, with_logits=True)
    hop1 = infer_raw_video(det, dev, lm, aligner, batch_size=1, with_logits=True, hop=1, encode_chunk=T)
    assert tuple(hop1[2].shape) == (F - T + 1, 2) and same(hop1[1], hop1[2].softmax(dim=-1)) and same(hop1[0], hop1[1].mean(dim=0)[1])
    plan = aligner.plan(lm)
    crops = aligner.apply(dev, plan)
    x = crops[:2 * T].view(2, T, *crops.shape[1:])
    m = torch.from_numpy(plan.valid[:2 * T].copy()).view(2, T).cuda()
    assert m.tolist() == [[True] * 4, [True, False, True, True]]
    bar, _ = chunk_gap(det, x, m)
    hold(f"{precision} hop=1 rows 0 and {T} vs hop=None", hop1[2][::T], base[2], bar)
    # tail="last" at hop 3: starts 0, 3, 6 and 7; the same passes (4 + 4 + 3 frames) and the same decoder batch as hop = 1
    last = infer_raw_video(det, dev, lm, aligner, batch_size=1, with_logits=True, hop=3, tail="last", encode_chunk=T)[2]
    assert tuple(last.shape) == (4, 2) and same(last, hop1[2][[0, 3, 6, 7]])
    with pytest.raises(ValueError, match="do not fill one clip"):
        infer_raw_video(det, dev[:3], lm[:3], aligner, hop=1)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------

def test_refusals():
    ema = model("fp32", False, op_mode__ema_frame=0.3, op_mode__temporal_position=0)
    with pytest.raises(capi.DfdError, match="ema_frame"):
        FrameStore(ema, 16)
    with pytest.raises(capi.DfdError, match="ema_frame"):
        StreamingVerdict(ema, hop=1)
    det = model("fp32", False)
    with pytest.raises(ValueError, match="capacity=6 is below num_frames \\+ encode_chunk = 4 \\+ 3"):
        FrameStore(det, 6, encode_chunk=3)
    with pytest.raises(ValueError, match="capacity"):
        FrameStore(det, T)
    with pytest.raises(ValueError, match="capacity"):
        StreamingVerdict(det, hop=2, capacity=5)
    store = FrameStore(det, 8)
    assert store.chunk == 4 and store.k.shape == (2, 8, 4, 128) and store.k.is_contiguous() and store.staging.shape == (2, 4, 5, 384)
    frames, valid = feed(11)
    with pytest.raises(capi.DfdError, match="device tensor"):
        det.push_frames(store, frames[:2].cpu())
    with pytest.raises(capi.DfdError, match="device tensor"):
        det.push_frames(store, frames[:2].cpu().numpy())
    with pytest.raises(ValueError, match="5 frames in one pass"):
        det.push_frames(store, frames[:5])
    with pytest.raises(ValueError, match="valid flags"):
        det.push_frames(store, frames[:3], valid[:2])
    with pytest.raises(capi.DfdError, match="another geometry"):
        model("bf16", False).push_frames(store, frames[:2])
    assert (store.first, store.count) == (0, 0)  # nothing of the above stored a frame
    assert det.push_frames(store, frames[:0]) == range(0, 0)
    assert det.push_frames(store, frames[:3], valid[:3]) == range(0, 3) and det.push_frames(store, frames[3:7]) == range(3, 7)
    for bad in ([[0, 1, 2]], [[0, 1, 2, 3, 4]], [0, 1, 2, 3]):
        with pytest.raises(capi.DfdError, match="num_frames = 4"):
            det.predict_windows(store, bad)
    with pytest.raises(capi.DfdError, match="no window"):
        det.predict_windows(store, torch.zeros(0, T, dtype=torch.int64))
    det.train()
    try:
        with pytest.raises(capi.DfdError, match="eval"):
            det.predict_windows(store, [[0, 1, 2, 3]])
    finally:
        det.eval()
    logits, feats = det.predict_windows(store, [[3, 4, 5, 6], [0, 1, 2, 3]])
    assert logits[0].shape == (2, 2) and torch.isfinite(logits[0]).all() and not logits[0].requires_grad and feats == {}
