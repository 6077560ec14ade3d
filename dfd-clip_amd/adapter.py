"""CompInvAdapter on HIP kernels (reference `src/models.py:783-940`).

Per selected layer and per tensor (k, v): a residual bottleneck
    kv <- kv + Linear_{x->D}( GELU( LayerNorm( Linear_{D->x}(kv) ) ) )        structs 768-x-768-{nln, ln, z0}
    kv <- kv + Linear_{x->D}( LayerNorm( GELU( Linear_{D->x}(kv) ) ) )        structs 768-x-768, legacy-768-x-768
applied to the exported K/V (CLS row dropped) BEFORE the decoder adds its temporal positional
embedding.  Parameter names follow the reference's `nn.Sequential` indices
(`l{i}_{k|v}.0.weight`, `.1.weight`, `.1.bias`, `.4.weight`), so reference checkpoints load.

Kernel sequence per (layer, tensor) on the packed export `[N*P, D]`:
    dfd_gemm(BIAS, bias = NULL)                    a1 = kv · W0ᵀ           [N*P, x]
    dfd_adapter_norm_gelu                          a2 = GELU(LN(a1))        "nln": stats over (P, x); "ln"/"z0": over x
    dfd_gemm(RESIDUAL_POS)                         kv += a2 · W4ᵀ + pos[frame % T]   (in place, one rounding)
In `train()` mode with `config.dropout` > 0 the reference's two nn.Dropout layers act as there: p/10 (p/5 for
`768-x-768`, none for `legacy-`) on a2, and p on a2 · W4ᵀ before the residual add (the GEMM epilogue draws the
mask); masks are counter-based and regenerated in the backward (csrc/dropout.hpp).

Training (`run`, with grad enabled and trainable parameters) goes through `_AdapterFn`: the forward is
out of place and keeps a1; the backward takes dK/dV from the decoder's attention backward and runs
    a2  = GELU(LN(a1))                      (recomputed)            dfd_adapter_norm_gelu
    dW4 = dOutᵀ · a2                        [D, x]                  dfd_gemm_at_b   (split-K over B·T·P rows)
    dA2 = dOut · W4                         [rows, x]               dfd_gemm
    da1, dγ, dβ = LN/GELU backward                                  dfd_adapter_norm_gelu_bwd
    dW0 = da1ᵀ · X                          [x, D]                  dfd_gemm_at_b
The encoder output X needs no gradient (frozen encoder, reference models.py:440).

The structs without a LayerNorm (models.py:877-922; csrc/adapter_structs.hip), per (layer, tensor):
    "768-bn"       kv <- kv + Dropout_p(BatchNorm2d(T)(kv · W0ᵀ))   channel = frame index t, statistics over (b, p, 768)
        dfd_gemm(BIAS)                 y = kv · W0ᵀ                       [N*P, 768]
        dfd_adapter_bn_stats           (mean, invstd)[t]; train mode: batch statistics, running ones advanced on the device
        dfd_adapter_bn_apply           kv = kv + drop(γ_t (y - μ_t) invstd_t + β_t) + pos[frame % T]   (in place)
      backward: dfd_adapter_bn_bwd (Σdz, Σdz·ŷ per channel, then dy), dfd_gemm_at_b (dW0 = dyᵀ · X)
    "768-xxx-768"  kv <- kv + Dropout_p(W6 · drop_{p/5}(GELU(W3 · drop_{p/5}(GELU(W0 · kv)))))   GELU = exact erf form
        dfd_gemm(BIAS), dfd_gelu_erf, dfd_gemm(BIAS), dfd_gelu_erf, dfd_gemm(RESIDUAL_POS)
      backward: dfd_gemm_at_b / dfd_gemm per Linear, dfd_gelu_erf_bwd (from the saved pre-activations) per GELU
    "linear"       kv <- Dropout_p(kv · W0ᵀ)                        no residual; W0 starts as the identity
        dfd_gemm(BIAS) into an f32 scratch, dfd_adapter_bn_apply without statistics (drop + pos, one rounding)
      backward: dfd_dropout, dfd_gemm_at_b
BatchNorm follows the module's own `training` flag, as nn.BatchNorm2d does (not `Detector.forward(train=...)`): in
train mode a forward normalises with the batch's statistics and advances the running ones, with or without autograd and
for a frozen adapter too; the backward never touches them.  With several ranks the statistics are per rank (DDP
without SyncBatchNorm); the buffers travel with `dist.broadcast_parameters`.
"""
import collections
import logging
import weakref

import torch
from torch import nn

from . import capi
from .encoder import RuntimeStateMixin

# captured forward / backward kernel sequences per adapter instance and input signature (as the decoder's: decoder.py)
_GRAPHS = weakref.WeakKeyDictionary()

# struct -> (index of the LayerNorm and of the output Linear inside the reference's nn.Sequential, kernel mode:
# 0 = GELU(LN_row(a)), 1 = GELU(LN_joint(a)), 2 = LN_row(GELU(a)))   (reference models.py:795-875)
_STRUCTS = {"768-x-768-nln": (1, 4, 1), "768-x-768-ln": (1, 4, 0), "768-x-768-z0": (1, 4, 0),
            "768-x-768": (2, 4, 2), "legacy-768-x-768": (2, 3, 2)}
# the structs without a LayerNorm (models.py:877-922): struct -> names of their parameters inside the nn.Sequential
_PLAIN_STRUCTS = {"768-bn": ("0.weight", "1.weight", "1.bias"), "768-xxx-768": ("0.weight", "3.weight", "6.weight"),
                  "linear": ("0.weight",)}
_SUPPORTED = tuple(_STRUCTS) + tuple(_PLAIN_STRUCTS)


class CompInvAdapter(RuntimeStateMixin, nn.Module):
    _RUNTIME_STATE = {"_prep": None, "_after_backward": None, "_graphs_failed": None}
    max_graphs = 4

    def invalidate_caches(self):
        self._prep = None
        _GRAPHS.pop(self, None)

    def __init__(self, config, detector, num_frames=50):
        super().__init__()
        enc = detector.encoder
        width = enc.width
        self.patches = (enc.input_resolution // enc.patch_size) ** 2
        self.struct = config.adapter.struct.type
        if self.struct not in _SUPPORTED:
            raise NotImplementedError(f"adapter struct {self.struct} is not built (supported: {_SUPPORTED})")
        self.plain = self.struct in _PLAIN_STRUCTS
        if self.struct == "768-bn":
            if width != 768:
                raise NotImplementedError(f"adapter struct 768-bn at width {width}: the reference hard-codes Linear(768, 768) "
                                          "(src/models.py:877-886) and fails at its first forward on this tower")
            op = config.op_mode if "op_mode" in config else {}
            if "ema_frame" in op and op.ema_frame:
                raise NotImplementedError("adapter struct 768-bn with op_mode.ema_frame: the clip collapses to one frame but "
                                          "BatchNorm2d(num_frames) has num_frames channels (src/models.py:572-578, :877-886)")
        self.ln_idx, self.out_idx, self.mode = _STRUCTS[self.struct] if not self.plain else (None, None, None)
        self.inner = int(config.adapter.struct.x) if "x" in config.adapter.struct else 0
        self.width = width
        self.num_frames = num_frames
        p = float(config.dropout) if "dropout" in config else 0.0
        self.drop_outer = p  # every struct ends in nn.Dropout(p) (models.py:807, :820, :836, :852, :864, :884, :904, :913)
        self.drop_inner = 0.0 if self.struct in ("legacy-768-x-768", "768-bn", "linear") else (
            p / 5 if self.struct in ("768-x-768", "768-xxx-768") else p / 10)
        self.residual = self.struct != "linear"  # models.py:908
        self.n_layers = len(detector.layer_indices)
        for i in range(self.n_layers):
            for j in ("k", "v"):
                ln_shape = (self.patches, self.inner) if self.struct.endswith("nln") else self.inner
                if self.struct == "768-bn":
                    seq = nn.Sequential(nn.Linear(768, 768, bias=False), nn.BatchNorm2d(num_frames), nn.Dropout(p))
                elif self.struct == "768-xxx-768":
                    seq = nn.Sequential(nn.Linear(width, self.inner, bias=False), nn.GELU(), nn.Dropout(p / 5),
                                        nn.Linear(self.inner, self.inner, bias=False), nn.GELU(), nn.Dropout(p / 5),
                                        nn.Linear(self.inner, width, bias=False), nn.Dropout(p))
                elif self.struct == "linear":  # starts as the identity map (models.py:916-917)
                    seq = nn.Sequential(nn.Linear(width, width, bias=False), nn.Dropout(p))
                    seq[0].weight.data = torch.eye(width)
                elif self.struct == "768-x-768":
                    seq = nn.Sequential(nn.Linear(width, self.inner, bias=False), nn.GELU(), nn.LayerNorm(self.inner),
                                        nn.Dropout(config.dropout / 5), nn.Linear(self.inner, width, bias=False),
                                        nn.Dropout(config.dropout))
                elif self.struct == "legacy-768-x-768":
                    seq = nn.Sequential(nn.Linear(width, self.inner, bias=False), nn.GELU(), nn.LayerNorm(self.inner),
                                        nn.Linear(self.inner, width, bias=False), nn.Dropout(config.dropout))
                else:
                    seq = nn.Sequential(nn.Linear(width, self.inner, bias=False), nn.LayerNorm(ln_shape), nn.GELU(),
                                        nn.Dropout(config.dropout / 10), nn.Linear(self.inner, width, bias=False),
                                        nn.Dropout(config.dropout))
                if self.struct.endswith("z0"):  # starts as the identity map (models.py:867-869)
                    seq[1].weight.data.zero_()
                    seq[4].weight.data.zero_()
                setattr(self, f"l{i}_{j}", seq)
        self._prep = None
        self._after_backward = None  # one-shot callback for the next autograd node (Detector's encoder pipelining)
        # training: replay the forward / backward kernel sequences as HIP graphs (`Detector.static_graphs`).  The ~170
        # launches and ~100 small tensor ops of an adapter step then cost the host two graph launches; the outputs
        # (k, v) = adapter(raw) + pos live in the graph's static buffers — what a call returned is overwritten by the
        # next call with the same input buffers, and the decoder's own graphs find them at fixed addresses
        self.use_graphs = False
        self._graphs_failed = None

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._prep = None
        return out

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self._prep = None
        return out

    def _weights(self, act):
        # (the address too: `p.data = new` — the unfused EMA teacher's update — re-seats a parameter without moving its version)
        key = (act, tuple((p._version, p.data_ptr()) for p in self.parameters()))
        if self._prep is None or self._prep[0] != key:
            w = {}
            for i in range(self.n_layers):
                for j in ("k", "v"):
                    seq = getattr(self, f"l{i}_{j}")
                    if self.plain:  # Linear weights in the activation dtype, BatchNorm affine in f32
                        sd = {n: t.detach() for n, t in seq.named_parameters()}
                        w[(i, j)] = tuple(_staged(sd[n], act) for n in _PLAIN_STRUCTS[self.struct])
                        continue
                    ln, out = seq[self.ln_idx], seq[self.out_idx]
                    w[(i, j)] = (seq[0].weight.detach().to(act).contiguous(), ln.weight.detach().float().contiguous(),
                                 ln.bias.detach().float().contiguous(), out.weight.detach().to(act).contiguous())
            self._prep = (key, w)
        return self._prep[1]

    def run(self, k_raw, v_raw, num_frames, temporal_pos, drop_rng=None):
        """(k, v) = adapter(raw export) + pos.  In place without autograd; out of place through
        `_AdapterFn` when gradients can flow to the adapter's parameters.  `drop_rng`: this step's
        dropout state (device int64 {seed, step}) in train mode, None = no dropout."""
        names = [n for n, p in self.named_parameters()]
        params = [p for n, p in self.named_parameters()]
        if torch.is_grad_enabled() and any(p.requires_grad for p in params):
            return _AdapterFn.apply(self, k_raw, v_raw, num_frames, temporal_pos, names, drop_rng, *params)
        return self.apply_packed(k_raw, v_raw, num_frames, temporal_pos, drop_rng)

    def _drops(self, drop_rng, i, jj):
        """(inner, outer) dropout descriptors of layer i, tensor jj (0 = k, 1 = v); None where inactive."""
        if drop_rng is None:
            return None, None
        base = 1000 + 4 * (2 * i + jj)
        inner = capi.Dropout(drop_rng, base, self.drop_inner) if self.drop_inner > 0 else None
        outer = capi.Dropout(drop_rng, base + 1, self.drop_outer) if self.drop_outer > 0 else None
        return inner, outer

    def _drop_second(self, drop_rng, i, jj):
        """768-xxx-768's second inner dropout (after the second GELU): site base + 2 of the four per (layer, tensor)."""
        if drop_rng is None or self.drop_inner <= 0:
            return None
        return capi.Dropout(drop_rng, 1000 + 4 * (2 * i + jj) + 2, self.drop_inner)

    def _bn_mode(self, update_running):
        if not self.training:
            return capi.BN_EVAL
        return capi.BN_TRAIN_UPDATE if update_running else capi.BN_TRAIN

    def _plain_fwd(self, wts, src, dst, i, j, jj, num_frames, pos, drop_rng, bufs, update_running):
        """One (layer, tensor) of a struct without LayerNorm: dst = adapter(src) + pos; dst may be src (in place).  `bufs`
        holds this tensor's intermediates (kept for the backward, or scratch)."""
        P = self.patches
        frames = src.shape[0] // P
        inner, outer = self._drops(drop_rng, i, jj)
        if self.struct == "768-bn":
            w0, gamma, beta = wts
            if num_frames != self.num_frames:
                raise RuntimeError(f"768-bn adapter built for {self.num_frames} frames got clips of {num_frames}")
            bn = getattr(self, f"l{i}_{j}")[1]
            capi.gemm(src, w0, bufs["y"], None, capi.EPI_BIAS)
            capi.adapter_bn_stats(bufs["y"], bufs["stats"], bufs["ws"], frames, P, num_frames, self._bn_mode(update_running),
                                  bn.running_mean, bn.running_var, bn.num_batches_tracked, momentum=bn.momentum, eps=bn.eps)
            capi.adapter_bn_apply(bufs["y"], dst, frames, P, num_frames, bufs["stats"], gamma, beta, residual=src, pos=pos,
                                  drop=outer)
        elif self.struct == "768-xxx-768":
            w0, w3, w6 = wts
            capi.gemm(src, w0, bufs["a1"], None, capi.EPI_BIAS)
            capi.gelu_erf(bufs["a1"], bufs["h1"], inner)
            capi.gemm(bufs["h1"], w3, bufs["a2"], None, capi.EPI_BIAS)
            capi.gelu_erf(bufs["a2"], bufs["h2"], self._drop_second(drop_rng, i, jj))
            capi.gemm(bufs["h2"], w6, dst, None, capi.EPI_RESIDUAL_POS, pos=pos, tokens=P + 1, frames_per_clip=num_frames,
                      residual=None if dst is src else src, drop=outer)
        else:  # linear: the GEMM cannot write over its own A operand, so it goes through an f32 scratch
            (w0,) = wts
            capi.gemm(src, w0, bufs["o"], None, capi.EPI_BIAS)
            capi.adapter_bn_apply(bufs["o"], dst, frames, P, max(num_frames, 1), pos=pos, drop=outer)

    def _plain_bufs(self, rows, act, dev, L=None):
        """Intermediates of `_plain_fwd`: one set (L None: scratch shared by every tensor) or [L][2] sets to keep."""
        P, T, x = self.patches, self.num_frames, self.inner
        frames = rows // P

        def one(share=None):
            if self.struct == "768-bn":
                ws = share["ws"] if share else torch.empty(capi.adapter_bn_workspace_bytes(frames, P, 768) // 4 + 4,
                                                           device=dev, dtype=torch.float32)
                return dict(y=torch.empty(rows, 768, device=dev, dtype=act), stats=torch.empty(2, T, device=dev, dtype=torch.float32),
                            ws=ws)
            if self.struct == "768-xxx-768":
                if L is None:  # in place: h = GELU(a) over a, two buffers suffice
                    a, b = torch.empty(rows, x, device=dev, dtype=act), torch.empty(rows, x, device=dev, dtype=act)
                    return dict(a1=a, h1=a, a2=b, h2=b)
                return {k: torch.empty(rows, x, device=dev, dtype=act) for k in ("a1", "h1", "a2", "h2")}
            return dict(o=share["o"] if share else torch.empty(rows, self.width, device=dev, dtype=torch.float32))

        if L is None:
            return one()
        first = one()
        return [[first if (i, jj) == (0, 0) else one(first) for jj in range(2)] for i in range(L)]

    def _stage_weights(self, w, act):
        out = {}
        for i in range(self.n_layers):
            for j in ("k", "v"):
                pre = f"l{i}_{j}."
                if self.plain:
                    out[(i, j)] = tuple(_staged(w[pre + n], act) for n in _PLAIN_STRUCTS[self.struct])
                    continue
                out[(i, j)] = (w[pre + "0.weight"].to(act).contiguous(), w[pre + f"{self.ln_idx}.weight"].float().contiguous(),
                               w[pre + f"{self.ln_idx}.bias"].float().contiguous(),
                               w[pre + f"{self.out_idx}.weight"].to(act).contiguous())
        return out

    def _forward_train(self, w, k_raw, v_raw, num_frames, temporal_pos, drop_rng=None, update_running=True):
        act = k_raw.dtype
        sw = self._stage_weights(w, act)
        L, rows, D = k_raw.shape
        if self.plain:
            k_out, v_out = torch.empty_like(k_raw), torch.empty_like(v_raw)
            bufs = self._plain_bufs(rows, act, k_raw.device, L)
            for i in range(L):
                for jj, (j, src, dst) in enumerate((("k", k_raw, k_out), ("v", v_raw, v_out))):
                    self._plain_fwd(sw[(i, j)], src[i], dst[i], i, j, jj, num_frames, temporal_pos, drop_rng, bufs[i][jj],
                                    update_running)
            return k_out, v_out, (bufs, self.training)
        P, x = self.patches, self.inner
        frames = rows // P
        joint = self.mode
        k_out, v_out = torch.empty_like(k_raw), torch.empty_like(v_raw)
        # GELU-first structs keep the projection output in f32 (LayerNorm after the non-linearity amplifies
        # the rounding of its input ~4x more than the other order)
        a1_all = torch.empty(L, 2, rows, x, device=k_raw.device, dtype=torch.float32 if self.mode == 2 else act)
        # the second Linear's input (after the inner dropout) is kept as well: 48 MB per (layer, tensor) at B16xT30 buys the
        # backward one normalisation pass less each
        a2_all = torch.empty(L, 2, rows, x, device=k_raw.device, dtype=act)
        for i in range(L):
            for jj, (j, src, dst) in enumerate((("k", k_raw, k_out), ("v", v_raw, v_out))):
                w0, lw, lb, w4 = sw[(i, j)]
                inner, outer = self._drops(drop_rng, i, jj)
                a2 = a2_all[i, jj]
                capi.gemm(src[i], w0, a1_all[i, jj], None, capi.EPI_BIAS)
                capi.adapter_norm_gelu(a1_all[i, jj], a2, lw, lb, frames, P, x, joint)
                if inner is not None:
                    capi.dropout(a2, a2, inner)
                capi.gemm(a2, w4, dst[i], None, capi.EPI_RESIDUAL_POS, pos=temporal_pos, tokens=P + 1, frames_per_clip=num_frames,
                          residual=src[i], drop=outer)
        return k_out, v_out, (a1_all, a2_all)

    def _backward_train(self, w, k_raw, v_raw, saved, dk, dv, drop_rng=None):
        if self.plain:
            return self._plain_backward(w, k_raw, v_raw, saved, dk, dv, drop_rng)
        a1_all, a2_all = saved
        act = k_raw.dtype
        sw = self._stage_weights(w, act)
        L, rows, D = k_raw.shape
        P, x = self.patches, self.inner
        frames = rows // P
        joint = self.mode
        dev = k_raw.device
        f32 = dict(device=dev, dtype=torch.float32)
        da2 = torch.empty(rows, x, device=dev, dtype=act)
        da1 = torch.empty(rows, x, device=dev, dtype=act)
        nb = max(capi.gemm_at_b_workspace_bytes(rows, D, x, act), capi.gemm_at_b_workspace_bytes(rows, x, D, act))
        ws_ab = torch.empty(nb // 4 + 64, **f32)
        ws_ln = torch.empty(capi.adapter_norm_gelu_bwd_workspace_bytes(frames, P, x, joint) // 4 + 4, **f32)
        grads = {}
        d_masked = None
        for i in range(L):
            for jj, (j, src, dout) in enumerate((("k", k_raw, dk), ("v", v_raw, dv))):
                pre = f"l{i}_{j}."
                w0, lw, lb, w4 = sw[(i, j)]
                inner, outer = self._drops(drop_rng, i, jj)
                if outer is not None:  # gradient entering the dropped a2 · W4ᵀ: same mask, same scale
                    if d_masked is None:
                        d_masked = torch.empty(rows, D, device=dev, dtype=act)
                    d_o = capi.dropout(dout[i], d_masked, outer)
                else:
                    d_o = dout[i].to(act) if dout.dtype != act else dout[i]
                a1, a2 = a1_all[i, jj], a2_all[i, jj]
                dw4 = torch.empty(D, x, **f32)
                capi.gemm_at_b(d_o, a2, dw4, ws_ab)
                w4t = w[pre + f"{self.out_idx}.weight"].float().t().contiguous().to(act)  # [x, D]: dA2 = dOut @ W4 as A @ (W4^T)^T
                capi.gemm(d_o, w4t, da2, None, capi.EPI_BIAS)
                if inner is not None:
                    capi.dropout(da2, da2, inner)
                dlw, dlb = torch.empty_like(lw), torch.empty_like(lb)
                capi.adapter_norm_gelu_bwd(a1, da2, da1, lw, lb, dlw, dlb, ws_ln, frames, P, x, joint)
                dw0 = torch.empty(x, D, **f32)
                capi.gemm_at_b(da1, src[i], dw0, ws_ab)
                grads[pre + "0.weight"], grads[pre + f"{self.out_idx}.weight"] = dw0, dw4
                grads[pre + f"{self.ln_idx}.weight"], grads[pre + f"{self.ln_idx}.bias"] = dlw, dlb
        return grads

    def _plain_backward(self, w, k_raw, v_raw, saved, dk, dv, drop_rng=None):
        bufs, trained = saved
        act = k_raw.dtype
        sw = self._stage_weights(w, act)
        L, rows, D = k_raw.shape
        P, x, T = self.patches, self.inner, self.num_frames
        frames = rows // P
        dev = k_raw.device
        f32 = dict(device=dev, dtype=torch.float32)
        shapes = {"768-bn": [(rows, 768, D)], "768-xxx-768": [(rows, D, x), (rows, x, x), (rows, x, D)],
                  "linear": [(rows, D, D)]}[self.struct]
        ws_ab = torch.empty(max(capi.gemm_at_b_workspace_bytes(*s, act) for s in shapes) // 4 + 64, **f32)
        grads = {}
        d_masked = dy = dh = None
        for i in range(L):
            for jj, (j, src, dout) in enumerate((("k", k_raw, dk), ("v", v_raw, dv))):
                pre = f"l{i}_{j}."
                b = bufs[i][jj]
                inner, outer = self._drops(drop_rng, i, jj)
                if self.struct == "768-bn":  # the dropout mask is applied inside the BatchNorm backward
                    _, gamma, _ = sw[(i, j)]
                    if dy is None:
                        dy = torch.empty(rows, 768, device=dev, dtype=act)
                    d_in = dout[i] if dout.dtype in (act, torch.float32) else dout[i].to(act)
                    dg, db = torch.empty(T, **f32), torch.empty(T, **f32)
                    capi.adapter_bn_bwd(b["y"], d_in, dy, b["stats"], gamma, dg, db, b["ws"], frames, P, T, trained, drop=outer)
                    dw0 = torch.empty(768, D, **f32)
                    capi.gemm_at_b(dy, src[i], dw0, ws_ab)
                    grads[pre + "0.weight"], grads[pre + "1.weight"], grads[pre + "1.bias"] = dw0, dg, db
                    continue
                if outer is not None:  # gradient entering the dropped output: same mask, same scale
                    if d_masked is None:
                        d_masked = torch.empty(rows, D, device=dev, dtype=act)
                    d_o = capi.dropout(dout[i], d_masked, outer)
                else:
                    d_o = dout[i].to(act) if dout.dtype != act else dout[i]
                if self.struct == "linear":
                    dw0 = torch.empty(D, D, **f32)
                    grads[pre + "0.weight"] = capi.gemm_at_b(d_o, src[i], dw0, ws_ab)
                    continue
                if dh is None:
                    dh = torch.empty(rows, x, device=dev, dtype=act)
                    dh1 = torch.empty(rows, x, device=dev, dtype=act)
                dw6, dw3, dw0 = torch.empty(D, x, **f32), torch.empty(x, x, **f32), torch.empty(x, D, **f32)
                capi.gemm_at_b(d_o, b["h2"], dw6, ws_ab)
                w6t = w[pre + "6.weight"].float().t().contiguous().to(act)  # [x, D]: dH2 = dOut @ W6 as A @ (W6^T)^T
                capi.gemm(d_o, w6t, dh, None, capi.EPI_BIAS)
                capi.gelu_erf_bwd(b["a2"], dh, dh, self._drop_second(drop_rng, i, jj))
                capi.gemm_at_b(dh, b["h1"], dw3, ws_ab)
                w3t = w[pre + "3.weight"].float().t().contiguous().to(act)
                capi.gemm(dh, w3t, dh1, None, capi.EPI_BIAS)
                capi.gelu_erf_bwd(b["a1"], dh1, dh1, inner)
                capi.gemm_at_b(dh1, src[i], dw0, ws_ab)
                grads[pre + "0.weight"], grads[pre + "3.weight"], grads[pre + "6.weight"] = dw0, dw3, dw6
        return grads

    @torch.no_grad()
    def apply_packed(self, k_all, v_all, num_frames, temporal_pos, drop_rng=None):
        """In place on the packed exports [L, N*P, D] (raw encoder K/V, no positional embedding yet):
        afterwards they hold adapter(kv) + pos, i.e. exactly what the decoder attends to."""
        if not k_all.is_cuda:
            raise capi.DfdError("the adapter runs on HIP kernels only: pass device tensors")
        act = k_all.dtype
        w = self._weights(act)
        L, rows, D = k_all.shape
        if self.plain:
            bufs = self._plain_bufs(rows, act, k_all.device)
            for i in range(L):
                for jj, (j, t) in enumerate((("k", k_all), ("v", v_all))):
                    self._plain_fwd(w[(i, j)], t[i], t[i], i, j, jj, num_frames, temporal_pos, drop_rng, bufs, True)
            return k_all, v_all
        P, x = self.patches, self.inner
        frames = rows // P
        a1 = torch.empty(rows, x, device=k_all.device, dtype=torch.float32 if self.mode == 2 else act)
        a2 = torch.empty(rows, x, device=k_all.device, dtype=act) if self.mode == 2 else a1
        joint = self.mode
        for i in range(L):
            for jj, (j, t) in enumerate((("k", k_all), ("v", v_all))):
                w0, lw, lb, w4 = w[(i, j)]
                inner, outer = self._drops(drop_rng, i, jj)
                capi.gemm(t[i], w0, a1, None, capi.EPI_BIAS)
                capi.adapter_norm_gelu(a1, a2, lw, lb, frames, P, x, joint)
                if inner is not None:
                    capi.dropout(a2, a2, inner)
                capi.gemm(a2, w4, t[i], None, capi.EPI_RESIDUAL_POS, pos=temporal_pos, tokens=P + 1, frames_per_clip=num_frames,
                          drop=outer)
        return k_all, v_all


    # ---- HIP-graph replay ------------------------------------------------------------------------------------------
    def _graph_forward(self, w, k_raw, v_raw, num_frames, temporal_pos, drop_rng, params):
        if self._graphs_failed:
            return None
        key = (k_raw.data_ptr(), v_raw.data_ptr(), tuple(k_raw.shape), str(k_raw.dtype), num_frames,
               None if temporal_pos is None else tuple(temporal_pos.shape),
               tuple(p.data_ptr() for p in params), drop_rng is not None, self.drop_inner, self.drop_outer, self.patches,
               self.training, tuple(b.data_ptr() for b in self.buffers()))
        graphs = _GRAPHS.setdefault(self, collections.OrderedDict())
        ent = graphs.get(key)
        if ent is not None:
            graphs.move_to_end(key)
        else:
            while len(graphs) >= self.max_graphs:
                torch.cuda.synchronize()
                graphs.popitem(last=False)
            # `temporal_pos` is a fresh f32 copy of the parameter on every call: the graph reads a static copy of it,
            # refreshed before each replay (as the dropout state)
            ent = dict(bwd={}, rng=None if drop_rng is None else drop_rng.clone(),
                       pos=None if temporal_pos is None else temporal_pos.clone())
            # eager once: lazy initialisations (the BatchNorm running statistics advance only in the captured forward)
            self._forward_train(w, k_raw, v_raw, num_frames, ent["pos"], ent["rng"], update_running=False)
            torch.cuda.synchronize()
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    k_out, v_out, a1_all = self._forward_train(w, k_raw, v_raw, num_frames, ent["pos"], ent["rng"])
            except Exception as e:  # capture is an optimisation: a runtime that refuses it leaves the eager launches
                self._graphs_failed = f"{type(e).__name__}: {e}"
                logging.warning("adapter: HIP graph capture failed, staying on eager launches (%s)", self._graphs_failed)
                torch.cuda.synchronize()
                return None
            ent.update(fwd=g, k_out=k_out, v_out=v_out, a1_all=a1_all)
            graphs[key] = ent
        if drop_rng is not None:
            ent["rng"].copy_(drop_rng)
        if temporal_pos is not None:
            ent["pos"].copy_(temporal_pos)
        ent["fwd"].replay()
        return ent

    def _graph_backward(self, ent, w, k_raw, v_raw, dk, dv):
        sig = (dk.data_ptr(), dv.data_ptr(), str(dk.dtype))
        b = ent["bwd"].get(sig)
        if b is None:
            if len(ent["bwd"]) >= 2:  # gradient buffers keep moving (the decoder is not replaying graphs): copy into a static pair
                sig = "static"
                b = ent["bwd"].get(sig)
        if b is None:
            static = sig == "static"
            b = dict(dk=dk.clone() if static else dk, dv=dv.clone() if static else dv, static=static)
            self._backward_train(w, k_raw, v_raw, ent["a1_all"], b["dk"], b["dv"], ent["rng"])  # eager once
            torch.cuda.synchronize()
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    grads = self._backward_train(w, k_raw, v_raw, ent["a1_all"], b["dk"], b["dv"], ent["rng"])
            except Exception as e:
                self._graphs_failed = f"{type(e).__name__}: {e}"
                logging.warning("adapter: HIP graph capture of the backward failed, staying on eager launches (%s)", self._graphs_failed)
                torch.cuda.synchronize()
                return self._backward_train(w, k_raw, v_raw, ent["a1_all"], dk, dv, ent["rng"])
            b.update(graph=g, grads=grads)
            ent["bwd"][sig] = b
        if b["static"]:
            b["dk"].copy_(dk)
            b["dv"].copy_(dv)
        b["graph"].replay()
        names = list(b["grads"])
        src = [b["grads"][k] for k in names]
        dst = [torch.empty_like(t) for t in src]  # autograd may keep or accumulate into what it is handed
        torch._foreach_copy_(dst, src)
        return dict(zip(names, dst))


def _staged(t, act):
    """A parameter as the kernels read it: Linear weights in the activation dtype, 1-d (BatchNorm affine) in f32."""
    return (t.to(act) if t.dim() == 2 else t.float()).contiguous()


class _AdapterFn(torch.autograd.Function):
    """autograd node around the adapter's HIP forward / backward.  Outputs (k, v) = adapter(raw) + pos."""

    @staticmethod
    def forward(ctx, adapter, k_raw, v_raw, num_frames, temporal_pos, names, drop_rng, *params):
        w = {n: p.detach() for n, p in zip(names, params)}
        ent = adapter._graph_forward(w, k_raw, v_raw, num_frames, temporal_pos, drop_rng, params) if adapter.use_graphs else None
        if ent is not None:
            k_out, v_out, a1_all = ent["k_out"], ent["v_out"], ent["a1_all"]
        else:
            k_out, v_out, a1_all = adapter._forward_train(w, k_raw, v_raw, num_frames, temporal_pos, drop_rng)
        ctx.graph_entry = ent
        ctx.adapter, ctx.w, ctx.names, ctx.drop_rng = adapter, w, names, drop_rng
        ctx.after_backward, adapter._after_backward = adapter._after_backward, None
        ctx.saved = (k_raw, v_raw, a1_all)
        ctx.req = [p.requires_grad for p in params]
        return k_out, v_out

    @staticmethod
    def backward(ctx, dk, dv):
        k_raw, v_raw, a1_all = ctx.saved
        if ctx.graph_entry is not None:
            grads = ctx.adapter._graph_backward(ctx.graph_entry, ctx.w, k_raw, v_raw, dk.contiguous(), dv.contiguous())
        else:
            grads = ctx.adapter._backward_train(ctx.w, k_raw, v_raw, a1_all, dk.contiguous(), dv.contiguous(), ctx.drop_rng)
        out = [grads.get(nm) if rq else None for nm, rq in zip(ctx.names, ctx.req)]
        if ctx.after_backward is not None:
            ctx.after_backward()
        return (None, None, None, None, None, None, None, *out)
