"""Overlapping-window and live verdicts over a per-frame K/V store.

The frozen tower is per frame: the raw K/V rows of a frame depend on nothing but that frame.  What binds a frame to a window
of `num_frames` comes after the tower and is cheap: the temporal positional embedding, the adapter and the decoder.  So a
frame goes through the tower ONCE (`Detector.push_frames`), its raw rows land in a ring (`FrameStore`), and any number of
windows read them (`Detector.predict_windows`): one `dfd_kv_move_frames` launch gathers the frames of W windows into a dense
[L, W*T, P, D] tensor, which the adapter and the decoder take exactly as `predict` hands them its own.  The decoder, the
adapter and the encoder kernels are the ones `predict` runs; with overlap `T / hop` the tower, ~95 % of a forward, does
`hop / T` of the work of re-encoding every window.  With `gather="table"` there is no gather and no dense tensor: the decoder
reads the ring in place through the windows' slot table (`capi.decoder_attn_fwd_frames`), bit for bit the same verdicts.

  window_table      which frames each window names (pure host)
  FrameRing         the ring's bookkeeping: slots, eviction, validity (pure host)
  FrameStore        FrameRing + the device buffers
  move_reference    `capi.kv_move_frames` restated with torch indexing (the yardstick of the kernel's tests)
  table_reference   the dense operand a slot table stands for (the yardstick of the tabled decoder attention's tests)
  choose_gather     "copy" or "table" for a model (pure host)
  push_frames / predict_windows   what the two `Detector` methods run
  StreamingVerdict  frames in, (window start, logits) out: live feeds, and `harness.infer_raw_video(hop=)`

fp8.  Under `precision="fp8"` a tower pass below `capi.FP8_MIN_ROWS` rows runs the bf16 arithmetic (the encoder's rule), so
there the rows of a frame, and with them the verdict, depend on how many frames share its pass: `encode_chunk` is that knob
(`encode_chunk * tokens >= FP8_MIN_ROWS` for the e4m3 kernels).  No bitwise claim is made for fp8 across chunk sizes."""
import numpy as np
import torch

from . import capi


def window_table(first, count, T, hop, tail="drop", step=1):
    """int64 [W, T] absolute frame indices of the windows over the frames [first, count): window w starts at
    `first + w*hop` and names T frames `step` apart.  `tail="drop"` (the reference's rule: a ragged tail is dropped) keeps
    the windows of that grid that fit; `tail="last"` adds one window that ends on frame `count - 1` when the grid leaves
    frames uncovered.  Fewer frames than one window spans give an empty [0, T] table."""
    first, count, T, hop, step = int(first), int(count), int(T), int(hop), int(step)
    if hop < 1:
        raise ValueError(f"window_table: hop={hop}: windows advance by at least one frame")
    if step < 1:
        raise ValueError(f"window_table: step={step}: frames of a window are at least one apart")
    if tail not in ("drop", "last"):
        raise ValueError(f"window_table: tail={tail!r}: 'drop' or 'last'")
    if T < 1:
        raise ValueError(f"window_table: T={T}: a window names at least one frame")
    extent = (T - 1) * step + 1
    span = count - first
    starts = list(range(first, count - extent + 1, hop)) if span >= extent else []
    if tail == "last" and starts and starts[-1] + extent < count:
        starts.append(count - extent)
    offs = torch.arange(T, dtype=torch.int64) * step
    return torch.tensor(starts, dtype=torch.int64).view(-1, 1) + offs.view(1, T)


def move_reference(k, v, src_frame, dst_frame, k_out, v_out):
    """What `capi.kv_move_frames` computes, in plain torch on any device (the yardstick of its tests):
    k_out[l, dst_frame[i], p, :] = k[l, src_frame[i], p, :] for every layer and patch row, the same for v; a table that is
    None is the identity i.  k, v [L, src_frames, P, D] and k_out, v_out [L, dst_frames, P, D] may be any strided views;
    bits are copied, nothing else of the outputs is touched.  Returns (k_out, v_out)."""
    n = len(src_frame) if src_frame is not None else (len(dst_frame) if dst_frame is not None else k.shape[1])
    ident = torch.arange(n, device=k.device)
    s = ident if src_frame is None else src_frame.to(device=k.device, dtype=torch.int64)
    d = ident if dst_frame is None else dst_frame.to(device=k.device, dtype=torch.int64)
    assert len(s) == len(d) == n, (len(s), len(d), n)
    k_out[:, d] = k[:, s]
    v_out[:, d] = v[:, s]
    return k_out, v_out


def table_reference(k_layer, v_layer, slots):
    """What `capi.decoder_attn_fwd_frames` / `decoder_attn_map_frames` read through a slot table, in plain torch on any device
    (the yardstick of their tests): the rows `k_layer[slots.clamp(0, C - 1)]` of one store layer [C, P, D] (any strided
    view) as the dense [B*T, P, D] operand of the untabled entry points; entries outside [0, C) are clamped as the kernel
    clamps them.  `v_layer` may be None.  Returns (k, v)."""
    idx = torch.as_tensor(slots).to(device=k_layer.device, dtype=torch.int64).reshape(-1).clamp(0, k_layer.shape[0] - 1)
    return k_layer[idx].contiguous(), (None if v_layer is None else v_layer[idx].contiguous())


GATHERS = ("copy", "table", "auto")


def choose_gather(requested, has_adapter, attn_modes):
    """How `predict_windows` hands a window batch to the decoder: "copy" (one `dfd_kv_move_frames` launch into the store's
    dense buffer) or "table" (the decoder reads the ring in place through the slot table).  `requested`: "copy", "table", or
    "auto" = "table" where it is allowed.  It is not allowed with an adapter (it needs the window's rows with the window's
    positional embedding, as one dense operand) nor with `op_mode.attn_mode` (the grouped-softmax pass scores its keys
    through a kernel that reads no table): "table" then raises `DfdError` naming the reason, "auto" is "copy"."""
    if requested not in GATHERS:
        raise ValueError(f"gather={requested!r}: 'copy', 'table' or 'auto'")
    if requested == "copy":
        return "copy"
    reason = None
    if has_adapter:
        reason = "the model has an adapter, which needs the window's rows with the window's positional embedding as one dense tensor"
    elif attn_modes:
        reason = "op_mode.attn_mode scores the keys in a grouped-softmax pass that reads no frame table"
    if reason is None:
        return "table"
    if requested == "table":
        raise capi.DfdError(f"gather='table': {reason}; use gather='copy' or 'auto'")
    return "copy"


def _gather_for(model, requested):
    return "copy" if requested == "copy" else choose_gather(requested, model.adapter is not None, model.decoder.attn_modes)


class FrameRing:
    """The bookkeeping of a frame store, on the host alone.  Frames carry absolute indices 0, 1, 2, ... in push order;
    frame `a` lives in slot `a % capacity`.  `count` is the index of the next frame, `first` that of the oldest frame
    still retained (`count - first <= capacity`), `valid[slot]` the caller's per-frame flag (a frame with a face)."""

    def __init__(self, capacity, num_frames, chunk):
        capacity, num_frames, chunk = int(capacity), int(num_frames), int(chunk)
        if num_frames < 1 or chunk < 1:
            raise ValueError(f"FrameRing: num_frames={num_frames}, chunk={chunk}: both at least 1")
        if capacity < num_frames + chunk:
            raise ValueError(f"FrameRing: capacity={capacity} is below num_frames + encode_chunk = {num_frames} + {chunk}: a pass "
                             "of new frames would evict frames of the window that it completes")
        self.capacity, self.num_frames, self.chunk = capacity, num_frames, chunk
        self.valid = np.zeros(capacity, dtype=bool)
        self.first = self.count = 0

    def slots(self, frames):
        """int32 slots of absolute frame indices (any shape)."""
        return (np.asarray(frames, dtype=np.int64) % self.capacity).astype(np.int32)

    def reserve(self, n, valid=None):
        """The slots the next n frames go to, and their flags, WITHOUT committing: -> (int32 [n] slots, bool [n])."""
        n = int(n)
        if n < 0 or n > self.chunk:
            raise ValueError(f"frame store: {n} frames in one pass, the store was built for passes of at most {self.chunk}")
        flags = np.ones(n, dtype=bool) if valid is None else np.asarray(torch.as_tensor(valid).cpu(), dtype=bool).reshape(-1)
        if flags.shape[0] != n:
            raise ValueError(f"frame store: {flags.shape[0]} valid flags for {n} frames")
        return self.slots(np.arange(self.count, self.count + n)), flags

    def commit(self, slots, flags):
        """The frames reserved are stored: -> range of their absolute indices.  Frames that fall out of the ring are evicted."""
        n = len(slots)
        self.valid[slots] = flags
        start = self.count
        self.count += n
        self.first = max(self.first, self.count - self.capacity)
        return range(start, self.count)

    def check(self, table):
        """Raises, naming the frame, when `table` names one that is evicted or not pushed yet: -> the table as int64 numpy."""
        table = np.asarray(torch.as_tensor(table).cpu(), dtype=np.int64)
        if table.size:
            lo, hi = int(table.min()), int(table.max())
            if lo < self.first:
                raise capi.DfdError(f"frame store: frame {lo} is evicted (the ring of {self.capacity} slots retains frames "
                                    f"{self.first} to {self.count - 1})")
            if hi >= self.count:
                raise capi.DfdError(f"frame store: frame {hi} is not pushed yet (the next frame is {self.count})")
        return table

    def mask(self, table):
        """bool numpy array, shaped as `table`: the flags of its frames."""
        return self.valid[self.slots(table)]


class FrameStore(FrameRing):
    """A ring of the tower's raw K/V per frame (no positional embedding, before any adapter) for `model`:
    `k`, `v` contiguous [L, capacity, P, D] in the tower's activation dtype on the model's device, a private in-place
    staging buffer [L, encode_chunk, tokens, 3D] that a tower pass writes its q|k|v into, and a dense buffer that grows to
    the largest window batch gathered.  `capacity >= num_frames + encode_chunk` (the default `encode_chunk` is what
    `capacity` leaves: `capacity - num_frames`).  A pass of `Detector.push_frames` holds at most `encode_chunk` frames."""

    def __init__(self, model, capacity, encode_chunk=None):
        if "ema_frame" in model.op_mode and model.op_mode.ema_frame:
            raise capi.DfdError("FrameStore: op_mode.ema_frame blends the frames of a clip into the tower's input, so a frame's K/V "
                                "depend on its clip and cannot be shared between windows")
        device = next(model.parameters()).device
        if device.type != "cuda":
            raise capi.DfdError(f"FrameStore: the model is on {device}: the store lives beside the HIP kernels, move the model to the GPU first")
        T = int(model.num_frames)
        chunk = int(encode_chunk) if encode_chunk is not None else max(1, int(capacity) - T)
        super().__init__(capacity, T, chunk)
        enc = model.encoder
        self.device, self.dtype = device, enc.act_dtype
        self.layers, self.tokens, self.width = len(model.layer_indices), int(enc.tokens), int(enc.width)
        self.patches = self.tokens - 1
        shape = (self.layers, self.capacity, self.patches, self.width)
        # (uninitialised: `check` lets no window name a slot before a frame was moved into it)
        self.k = torch.empty(shape, device=device, dtype=self.dtype)
        self.v = torch.empty(shape, device=device, dtype=self.dtype)
        self.staging = torch.empty(self.layers, self.chunk, self.tokens, 3 * self.width, device=device, dtype=self.dtype)
        self._dense = None

    def staging_for(self, n):
        """The staging buffer as the contiguous [L, n, tokens, 3D] a pass of n <= encode_chunk frames writes in place."""
        if n == self.chunk:
            return self.staging
        size = self.layers * n * self.tokens * 3 * self.width
        return self.staging.view(-1)[:size].view(self.layers, n, self.tokens, 3 * self.width)

    def dense(self, frames):
        """Two persistent contiguous [L, frames, P, D] tensors (views of buffers that grow to the largest request)."""
        size = self.layers * frames * self.patches * self.width
        if self._dense is None or self._dense[0].numel() < size:
            self._dense = (torch.empty(size, device=self.device, dtype=self.dtype), torch.empty(size, device=self.device, dtype=self.dtype))
        shape = (self.layers, frames, self.patches, self.width)
        return self._dense[0][:size].view(shape), self._dense[1][:size].view(shape)


def _own(model, store):
    if not isinstance(store, FrameStore):
        raise capi.DfdError(f"a FrameStore is needed, got {type(store).__name__}")
    enc = model.encoder
    if (store.layers, store.tokens, store.width, store.dtype, store.num_frames) != (len(model.layer_indices), enc.tokens, enc.width,
                                                                                     enc.act_dtype, model.num_frames):
        raise capi.DfdError("the FrameStore was built for a model of another geometry")


@torch.no_grad()
def push_frames(model, store, frames, valid=None):
    """`Detector.push_frames`: see there."""
    _own(model, store)
    if not torch.is_tensor(frames) or not frames.is_cuda:
        raise capi.DfdError("push_frames: frames must be a device tensor, f32 [N,3,R,R] or uint8 [N,3,H,W] (the tower runs on HIP kernels only)")
    if frames.dim() != 4 or frames.shape[1] != 3:
        raise capi.DfdError(f"push_frames: frames [N,3,H,W], got {tuple(frames.shape)}")
    n = frames.shape[0]
    slots, flags = store.reserve(n, valid)
    if n == 0:
        return store.commit(slots, flags)
    k, v = model.encoder.extract_kv(frames, model.layer_indices, 1, None, in_place=store.staging_for(n))
    capi.kv_move_frames(k, v, store.k, store.v, None, torch.from_numpy(slots).to(store.device), src_once=True, dst_host=slots)
    return store.commit(slots, flags)


@torch.no_grad()
def predict_windows(model, store, table, with_video_features=False, with_attention=False, gather="copy"):
    """`Detector.predict_windows`: see there."""
    _own(model, store)
    gather = _gather_for(model, gather)
    if model.training:
        raise capi.DfdError("predict_windows is inference only (no dropout, no batch statistics): call model.eval() first")
    table = store.check(table)
    T = int(model.num_frames)
    if table.ndim != 2 or table.shape[1] != T:
        raise capi.DfdError(f"predict_windows: the table is {tuple(table.shape)}, windows of this model name num_frames = {T} frames: [W, {T}]")
    W = table.shape[0]
    if W == 0:
        raise capi.DfdError("predict_windows: the table names no window")
    slots = store.slots(table).reshape(-1)
    slots_dev = torch.from_numpy(slots).to(store.device)
    m = torch.from_numpy(store.mask(table)).to(store.device)
    pos = model.decoder.temporal_pos()
    model.decoder.use_graphs = False
    if gather == "table":  # no gather launch, no dense buffer: the decoder reads the ring through the slots
        kv = (store.k, store.v, pos, slots_dev)
    else:
        k4, v4 = store.dense(W * T)
        capi.kv_move_frames(store.k, store.v, k4, v4, slots_dev, None, src_host=slots)
        if model.adapter is None:
            kv = (k4, v4, pos)
        else:
            model.adapter.use_graphs = False
            rows = W * T * store.patches
            kv = model.adapter.run(k4.view(store.layers, rows, store.width), v4.view(store.layers, rows, store.width), T, pos, None)
    heads = model.encoder.heads
    attention = torch.empty(store.layers, W, heads, T * store.patches, device=store.device, dtype=torch.float32) if with_attention else None
    _, video_features, task_logits = model.decoder.run(kv, m, None, attention=attention,
                                                       slots_host=torch.from_numpy(slots) if gather == "table" else None)
    features = {}
    if with_attention:
        features["attention"] = [attention[i].view(W, heads, T, -1) for i in range(store.layers)]
    if with_video_features:
        features["video"] = video_features
    return task_logits, features


class StreamingVerdict:
    """Frames in, verdicts out: every frame goes through the tower once, every window of `model.num_frames` consecutive
    frames that starts on a multiple of `hop` is decoded as soon as its last frame is stored.

    `push(frames, valid=None)` appends device frames (f32 [N,3,R,R] or uint8 [N,3,H,W]) to a pending buffer; the tower
    runs in passes of exactly `encode_chunk` frames (default `hop`), so what comes out does not depend on how the caller
    slices its pushes; the windows completed by a pass are decoded in batches of at most `batch_size`.  It returns the new
    verdicts as a list of (start frame, logits row of task `task_index` on the host).  `flush()` encodes what is pending
    in one last, shorter pass and applies `tail` (`window_table`): "drop" leaves the frames behind the last whole window
    out of the tower altogether, "last" adds the window that ends on the last frame.  `result()` is the verdict of
    everything decoded so far, as `harness.infer_raw_video` returns it.  The ring holds `capacity` frames (default
    `num_frames + encode_chunk`, the least that never evicts a frame of a window still to come), whatever the length of
    the feed.

    Single stream: every launch goes to the stream that is current when `push` / `flush` is called, and the store, the
    staging and the dense buffer are ordered by it alone.  Call one object from one stream (and one thread); `push` returns
    after copying the new logits to the host, which waits for that stream.

    `gather` is `predict_windows`'s: "copy" gathers every window batch into the store's dense buffer, "table" lets the
    decoder read the ring in place (refused, in words, for a model with an adapter or an attn_mode), "auto" is "table" where
    that is allowed.  The verdicts are the same bits either way.

    Under `precision="fp8"` the verdict depends on `encode_chunk` (see the module's note)."""

    def __init__(self, model, hop, encode_chunk=None, capacity=None, batch_size=16, task_index=0, tail="drop", gather="copy"):
        self.hop = int(hop)
        self.T = int(model.num_frames)
        window_table(0, 0, self.T, self.hop, tail)  # its raises
        if int(batch_size) < 1:
            raise ValueError(f"StreamingVerdict: batch_size={batch_size}")
        self.chunk = int(encode_chunk) if encode_chunk is not None else self.hop
        self.model, self.batch_size, self.task_index, self.tail = model, int(batch_size), int(task_index), tail
        self.gather = _gather_for(model, gather)  # its raises, before any buffer
        self.store = FrameStore(model, int(capacity) if capacity is not None else self.T + self.chunk, self.chunk)
        self._pending, self._pending_valid, self._npending = [], [], 0
        self._next_start = 0
        self._rows = []
        self._closed = False

    def push(self, frames, valid=None):
        if self._closed:
            raise capi.DfdError("StreamingVerdict: flush() closed this feed; start a new object for the next one")
        if not torch.is_tensor(frames) or not frames.is_cuda:
            raise capi.DfdError("StreamingVerdict.push: frames must be a device tensor, f32 [N,3,R,R] or uint8 [N,3,H,W]")
        n = frames.shape[0]
        flags = np.ones(n, dtype=bool) if valid is None else np.asarray(torch.as_tensor(valid).cpu(), dtype=bool).reshape(-1)
        if flags.shape[0] != n:
            raise ValueError(f"StreamingVerdict.push: {flags.shape[0]} valid flags for {n} frames")
        self._pending.append(frames)
        self._pending_valid.append(flags)
        self._npending += n
        out = []
        if self._npending >= self.chunk:
            buf, flags = self._take_pending()
            off = 0
            while self._npending - off >= self.chunk:
                out += self._ingest(buf[off:off + self.chunk], flags[off:off + self.chunk])
                off += self.chunk
            self._keep_pending(buf[off:], flags[off:])
        return out

    def flush(self):
        """Encode the pending remainder, decode what it completes, apply `tail`: -> the new (start, logits row) pairs."""
        if self._closed:
            return []
        self._closed = True
        out = []
        total = self.store.count + self._npending
        table = window_table(0, total, self.T, self.hop, self.tail)
        need = int(table.max()) + 1 if table.numel() else 0  # frames behind the last window go through no tower pass
        keep = min(self._npending, max(0, need - self.store.count))
        if keep:
            buf, flags = self._take_pending()
            out += self._ingest(buf[:keep], flags[:keep])
        self._keep_pending(None, None)
        if table.shape[0] > window_table(0, total, self.T, self.hop, "drop").shape[0]:  # tail="last": the one window off the grid
            out += self._decode(table[-1:])
        return out

    def result(self, with_logits=False):
        """(mean softmax probability of class 1, per-window probabilities [W, classes]) of the windows decoded so far,
        on the host; `with_logits` appends the logits [W, classes].  `starts` holds their first frames."""
        if not self._rows:
            raise ValueError(f"no window of {self.T} frames is complete yet")
        logits = torch.stack([row for _, row in self._rows])
        p = logits.softmax(dim=-1)
        res = (p.mean(dim=0)[1], p)
        return res + (logits,) if with_logits else res

    @property
    def starts(self):
        return [s for s, _ in self._rows]

    def _take_pending(self):
        buf = self._pending[0] if len(self._pending) == 1 else torch.cat(self._pending)
        return buf, np.concatenate(self._pending_valid)

    def _keep_pending(self, buf, flags):
        if buf is None or buf.shape[0] == 0:
            self._pending, self._pending_valid, self._npending = [], [], 0
        else:
            self._pending, self._pending_valid, self._npending = [buf], [flags], buf.shape[0]

    def _ingest(self, frames, flags):
        self.model.push_frames(self.store, frames, flags)
        starts = list(range(self._next_start, self.store.count - self.T + 1, self.hop))
        out = []
        for i in range(0, len(starts), self.batch_size):
            s = torch.tensor(starts[i:i + self.batch_size], dtype=torch.int64)
            out += self._decode(s.view(-1, 1) + torch.arange(self.T, dtype=torch.int64).view(1, -1))
        return out

    def _decode(self, table):
        logits = self.model.predict_windows(self.store, table, gather=self.gather)[0][self.task_index].detach().to("cpu")
        new = [(int(table[i, 0]), logits[i]) for i in range(table.shape[0])]
        self._rows += new
        self._next_start = max(self._next_start, int(table[-1, 0]) + self.hop)
        return new
