"""`CompInvEncoder`: stage 1 of DFD-CLIP, pre-training the K/V adapter (reference `src/models.py:943-1059`).

    CompInvEncoder(config, accelerator=None, num_frames=50, precision="bf16" | "fp32")

Same constructor arguments, attributes (`encoder`, `layer_indices`, `mode`, `adapter`, `transform`), `predict` /
`forward` / `configure_optimizers` contracts and state_dict names as the reference class, so `CompInvTrainer` /
`CompInvEvaluator` drive it unchanged and its checkpoint loads into `Detector` with `adapter.type: pretrain`.

    frames --extract_kv--> raw K/V [L, B*T*P, D] --CompInvAdapter (no positional embedding)--> A
           --dfd_compinv_loss_fwd--> (recon = 0, match = ||M||_F / P)

The frozen encoder, the adapter and the pair loss run on HIP kernels; the loss's backward
(`dfd_compinv_loss_bwd`) hands dK / dV straight to the adapter's own autograd node.

What the reference computes, reproduced here on purpose ("Adapter pre-training"):
  * its `predict` returns `(kvs, _kvs)` as one list object, and the adapter rebinds entries of the dicts it was
    given, so both losses compare ADAPTED keys / values: `recon_loss` is identically 0 (gradient 0), `mode` 0 and 1
    give the same `match_loss`, and the loss is symmetric within a pair, so `comp` does not change the numbers;
  * `match_loss = ||S.view(P, T, D).mean(1)||_F / P` reinterprets the [T, P, D] sum (no transpose).
One divergence: fewer than two clips is a `ValueError` here (the reference divides by zero pairs).
"""
import contextlib

import torch
from torch import nn

from . import capi
from .adapter import CompInvAdapter
from .config import default_compinv_config
from .detector import ClipTransform, disable_gradients, load_clip_visual
from .encoder import RuntimeStateMixin
from .weights import resolve_layer_indices


class _CompInvLossFn(torch.autograd.Function):
    """(recon, match) of the adapted packed K/V.  recon is the constant 0 (its gradient is 0); match's backward
    writes dK / dV in the K/V dtype and layout, reading the incoming gradient and ||M|| on the device."""

    @staticmethod
    def forward(ctx, k, v, B, T, P):
        f32 = dict(device=k.device, dtype=torch.float32)
        ws = torch.empty(-(-capi.compinv_loss_workspace_bytes(P, k.shape[-1]) // 4), **f32)
        recon, match, norm = torch.empty((), **f32), torch.empty((), **f32), torch.empty((), **f32)
        capi.compinv_loss_fwd(k, v, B, T, P, ws, match, norm, recon)
        ctx.save_for_backward(k, v)
        ctx.ws, ctx.norm, ctx.shape = ws, norm, (B, T, P)
        return recon, match

    @staticmethod
    def backward(ctx, d_recon, d_match):
        if d_match is None:
            return None, None, None, None, None
        k, v = ctx.saved_tensors
        B, T, P = ctx.shape
        g = d_match.detach().to(torch.float32).reshape(1).contiguous()
        dk, dv = torch.empty_like(k), torch.empty_like(v)
        capi.compinv_loss_bwd(k, v, B, T, P, ctx.ws, ctx.norm, g, dk, dv)
        return dk, dv, None, None, None


class CompInvEncoder(RuntimeStateMixin, nn.Module):
    _RUNTIME_STATE = {"_drop_master": None, "_kv_static": {}}

    @staticmethod
    def get_default_config():
        return default_compinv_config()

    def __init__(self, config, accelerator=None, num_frames=50, precision="bf16", *args, **kargs):
        super().__init__()
        assert config.decode_mode in ["stride", "index"]
        if precision not in ("fp32", "bf16"):
            raise NotImplementedError(f"CompInvEncoder precision {precision!r}: fp32 and bf16 are built (fp8 is not)")
        capi.load_library()  # fail at construction, not at first forward, when the kernels are missing
        self.config = config
        self.precision = precision
        self.num_frames = num_frames
        ctx = accelerator.main_process_first() if accelerator is not None else contextlib.nullcontext()
        with ctx:
            self.encoder = disable_gradients(load_clip_visual(config.architecture, precision))
        self.decode_mode = config.decode_mode
        self.layer_indices = resolve_layer_indices(config, len(self.encoder.transformer.resblocks))
        self.mode = int(config.mode)
        self.dropout_p = float(config.dropout) if "dropout" in config else 0.0
        self.adapter = CompInvAdapter(config, self, num_frames=num_frames)
        self.transform = ClipTransform(self.encoder.input_resolution)
        # opt-in: replay the adapter's training kernels as HIP graphs (fixed batch shape).  The raw K/V export then
        # goes to static buffers, and what `predict` / `forward` return lives in the graph's buffers until the next call
        self.use_graphs = False
        self._kv_static = {}
        self._drop_seed = None
        self._drop_master = None

    def invalidate_caches(self):
        self.encoder.invalidate()
        self.adapter.invalidate_caches()
        self._kv_static = {}

    def seed_dropout(self, seed):
        """As `Detector.seed_dropout`: fixes the stream of the adapter's dropout masks (train mode, dropout > 0)."""
        self._drop_seed = int(seed)
        self._drop_master = None

    def _next_drop_rng(self, device):
        if not self.training or self.dropout_p <= 0:
            return None
        if self._drop_master is None or self._drop_master.device != device:
            from . import dist as ddist
            seed = (self._drop_seed if self._drop_seed is not None else torch.initial_seed()) + 0x9E3779B97F4A7C15 * ddist.rank()
            self._drop_master = torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64, device=device)
        snap = self._drop_master.clone()
        self._drop_master[1] += 1
        return snap

    def _adapted(self, x):
        """x [B, T, 3, R, R] -> adapted packed K/V [L, B*T*P, D] (adapter(kv), no positional embedding)."""
        b, t = x.shape[:2]
        graphs = bool(self.use_graphs and torch.is_grad_enabled() and any(p.requires_grad for p in self.adapter.parameters()))
        out = None
        if graphs:  # fixed input addresses: the captured adapter graph is keyed on them
            key = (tuple(x.shape), x.device)
            out = self._kv_static.get(key)
            if out is None:
                P, D, L = self.adapter.patches, self.encoder.width, len(self.layer_indices)
                k = torch.empty(L, b * t * P, D, device=x.device, dtype=self.encoder.act_dtype)
                out = self._kv_static[key] = (k, torch.empty_like(k))
        with torch.no_grad():  # the encoder is frozen (reference models.py:992)
            kr, vr = self.encoder.extract_kv(x.flatten(0, 1), self.layer_indices, t, None, out=out)
        self.adapter.use_graphs = graphs
        drop_rng = self._next_drop_rng(x.device)
        return self.adapter.run(kr, vr, t, None, drop_rng)

    def predict(self, x):
        """x [B, T, 3, R, R] -> (kvs, kvs): per tapped layer {"k", "v"} views [B, T, P, heads, D/heads] of the adapted
        keys / values.  Both members are the same list, as in the reference (its `_kvs` aliases the adapted dicts)."""
        b, t = x.shape[:2]
        k, v = self._adapted(x)
        hh = self.encoder.heads
        P, D = self.adapter.patches, k.shape[-1]
        kvs = [{"k": k[i].view(b, t, P, hh, D // hh), "v": v[i].view(b, t, P, hh, D // hh)} for i in range(k.shape[0])]
        return kvs, kvs

    def forward(self, x, comp, *args, **kargs):
        """-> (recon_loss, match_loss), 0-dim f32 device tensors.  `comp`: per-clip compression tags (strings) or the
        labels tensor `CompInvTrainer` passes; one entry per clip.  The loss is symmetric within a pair, so its values
        do not change the result."""
        b, t = x.shape[:2]
        if b < 2:
            raise ValueError(f"CompInvEncoder.forward needs at least one (raw, c23) pair of clips, got a batch of {b} "
                             "(the reference divides by zero pairs here)")
        if len(comp) != b:
            raise ValueError(f"comp has {len(comp)} entries for a batch of {b} clips")
        k, v = self._adapted(x)
        return _CompInvLossFn.apply(k, v, b, t, self.adapter.patches)

    def configure_optimizers(self, lr):
        """AdamW over the adapter's parameters (reference `src/models.py:1053-1057`; torch's default weight decay 0.01): a
        `torch.optim.AdamW` whose step is one HIP launch (optim.py; CPU parameters are stepped by torch's own code)."""
        from .optim import FusedAdamW
        return FusedAdamW(self.adapter.parameters(), lr=lr)
