"""`configure_optimizers`' optimizers as ONE HIP launch per step: `FusedSGD` (reference `src/models.py:740-754`:
torch.optim.SGD, momentum 0.95, weight decay, over the trainable parameters; stepped once per batch by
`src/trainer.py:157-177` under a OneCycleLR that moves BOTH `lr` and `momentum` of the parameter group every step) and
`FusedAdamW` (the Detector's `optimizer: adamw`, `src/models.py:748-753`, and the only optimizer of adapter pre-training,
`src/models.py:1053-1057`; OneCycleLR moves `lr` and `betas[0]`).

`FusedSGD` is a `torch.optim.Optimizer`: `param_groups[0]["lr"]` / `["momentum"]` are read at every step, `state[p]
["momentum_buffer"]` holds the velocity (a view into one flat buffer), `state_dict()` / `load_state_dict()` work as for
`torch.optim.SGD`, parameters without a gradient are skipped, a parameter's first step initialises its velocity with the
gradient — torch's semantics and torch's rounding order (csrc/optim.hip).  What differs is the mechanics: gradients are
packed into a persistent flat buffer by one multi-tensor copy, then `dfd_sgd_step` updates every parameter in one launch;
for the decoder's Linear weights that launch also rewrites the transposed f32 copy the decoder's row-streaming linears
read (`Decoder.weight_mirrors`), so no transpose kernel runs after an update.

`FusedAdamW` is a `torch.optim.AdamW` with the same mechanics: `state[p]` = {"step": CPU f32 tensor, "exp_avg",
"exp_avg_sq"} as torch lays it out (the moments are views into two flat buffers), so its `state_dict()` loads into a
`torch.optim.AdamW` and back; the arithmetic is `_multi_tensor_adam`'s, op for op.  Parameters that share a step count
share a launch: one launch in steady state.  What the kernel does not cover (amsgrad, maximize, capturable, a parameter
that is not contiguous f32 on the GPU) is stepped by `torch.optim.AdamW.step` itself and logged once.
"""
import logging

import torch

from . import capi

_log = logging.getLogger(__name__)


class _TablePlans:
    """What the fused optimizers share: per parameter group, the packed gradients, one flat buffer per state tensor named
    in `_STATE` (the parameters' `state[p][name]` are views into it) and the device tables `dfd_sgd_step` walks."""
    _STATE = ()

    def _init_plans(self, mirrors):
        # mirrors: None, or an object with `mirror_for(param) -> tensor [cols, rows] or None`, `current_mirror(param)` and
        # `mirrors_written(pairs)` (the Decoder): the transposed copies this optimizer keeps in step with the weights
        self._mirrors = mirrors
        self._plans = {}

    @staticmethod
    def _fusable(p):
        return p.dtype == torch.float32 and p.is_cuda and p.is_contiguous()

    def _plan(self, gi, active):
        """Flat buffers and device tables of group `gi` for the parameters that have a gradient this step."""
        key = tuple((p.data_ptr(), tuple(p.shape)) for p in active)
        plan = self._plans.get(gi)
        if plan is not None and plan["key"] == key and all(
                e["mirror"] is None or self._mirrors.current_mirror(e["p"]) is e["mirror"] for e in plan["entries"]):
            return plan  # same parameters, and the decoder still reads the transposed copies this plan writes
        dev = active[0].device
        for p in active:
            if not self._fusable(p):
                raise capi.DfdError(f"{type(self).__name__} updates contiguous f32 parameters on the GPU")
        old = plan
        total = sum(p.numel() for p in active)
        gflat = torch.empty(total, device=dev, dtype=torch.float32)
        flats = {name: torch.zeros(total, device=dev, dtype=torch.float32) for name in self._STATE}
        entries, off = [], 0
        gviews = []
        for p in active:
            n = p.numel()
            gv = gflat[off:off + n].view_as(p)
            st = self.state[p]
            seasoned = st.get(self._STATE[0]) is not None
            views = {}
            for name, flat in flats.items():
                views[name] = flat[off:off + n].view_as(p)
                if st.get(name) is not None:
                    views[name].copy_(st[name])  # carried over from the previous plan / a loaded state_dict
                st[name] = views[name]
            mirror = self._mirrors.mirror_for(p) if (self._mirrors is not None and p.dim() == 2) else None
            rows, cols = (p.shape if mirror is not None else (0, 0))
            entries.append(dict(p=p, g=gv, buf=views[self._STATE[0]], state=views, mirror=mirror, numel=n, rows=rows, cols=cols,
                                fresh=not seasoned))
            gviews.append(gv)
            off += n
        plan = dict(key=key, gflat=gflat, flats=flats, entries=entries, gviews=gviews, tables={}, old=None)
        self._plans[gi] = plan
        del old
        return plan

    @staticmethod
    def _table(entries, dev):
        rows, first = [], 0
        for e in entries:
            m = e["mirror"]
            rows.append([e["p"].data_ptr(), e["g"].data_ptr(), e["buf"].data_ptr(), 0 if m is None else m.data_ptr(), e["numel"],
                         int(e["rows"]) | (int(e["cols"]) << 32), first])
            first += capi.sgd_blocks(e["numel"], e["rows"], e["cols"], m is not None)
        return torch.tensor(rows, dtype=torch.int64).to(dev), first

    def _written(self, plan):
        """After the launches of a step: the kernel wrote through raw pointers."""
        # caches keyed on a parameter's version counter must see the update
        # (the call takes an ITERABLE of tensors; handed one tensor it would iterate over its rows)
        torch._C._increment_version([e["p"] for e in plan["entries"]])
        written = []
        for e in plan["entries"]:
            e["fresh"] = False
            if e["mirror"] is not None:
                written.append((e["p"], e["mirror"]))
        if written:
            self._mirrors.mirrors_written(written)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plans.clear()  # the loaded state tensors are not views of the flat buffers: the next step packs them again


class FusedSGD(_TablePlans, torch.optim.Optimizer):
    _STATE = ("momentum_buffer",)

    def __init__(self, params, lr, momentum=0.95, weight_decay=0.0, mirrors=None):
        if lr < 0 or momentum < 0 or weight_decay < 0:
            raise ValueError("lr, momentum and weight_decay must be non-negative")
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay, dampening=0, nesterov=False))
        self._init_plans(mirrors)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for gi, group in enumerate(self.param_groups):
            if group.get("nesterov") or group.get("dampening", 0) != 0:
                raise capi.DfdError("FusedSGD: plain momentum only (the reference's optimizer)")
            active = [p for p in group["params"] if p.grad is not None]
            if not active:
                continue
            plan = self._plan(gi, active)
            torch._foreach_copy_(plan["gviews"], [p.grad for p in active])
            # a parameter's first step copies the gradient into its velocity (torch.optim.SGD); all later ones blend
            fresh = [e for e in plan["entries"] if e["fresh"]]
            seasoned = [e for e in plan["entries"] if not e["fresh"]]
            for first, part in ((True, fresh), (False, seasoned)):
                if not part:
                    continue
                tkey = (first, tuple(id(e["p"]) for e in part))
                tab = plan["tables"].get(tkey)
                if tab is None:
                    tab = plan["tables"][tkey] = self._table(part, active[0].device)
                capi.sgd_step(tab[0], len(part), tab[1], group["lr"], group["momentum"], group["weight_decay"], first)
            self._written(plan)
        return loss


class FusedAdamW(_TablePlans, torch.optim.AdamW):
    _STATE = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, mirrors=None, **kwargs):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, **kwargs)
        self._init_plans(mirrors)
        self._told = set()

    def _unfused(self, work):
        """Why this step is torch's and not the kernel's, or None.  `work`: (group index, group, active parameters)."""
        for gi, group, active in work:
            for flag in ("amsgrad", "maximize", "capturable", "differentiable", "fused"):
                if group.get(flag):
                    return f"{flag}=True"
            if isinstance(group["lr"], torch.Tensor):
                return "lr is a tensor"
            for p in active:  # every step: a gradient can turn sparse or change device between two steps
                if not self._fusable(p):
                    return "a parameter that is not contiguous f32 on the GPU"
                if p.grad.is_sparse or p.grad.device != p.device:
                    return "a gradient that is sparse or not on its parameter's device"
        return None

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for gi, group in enumerate(self.param_groups):
            active = [p for p in group["params"] if p.grad is not None]
            work.append((gi, group, active))
        why = self._unfused(work)
        if why is not None:
            if why not in self._told:
                self._told.add(why)
                _log.warning("FusedAdamW: %s: stepping with torch.optim.AdamW's own kernels", why)
            # torch's step without the step-hook wrapper torch puts round a class's `step` the first time the class is
            # instantiated (marked `hooked`): this step already runs inside that wrapper, the hooks must not run twice
            torch_step = torch.optim.AdamW.step
            if getattr(torch_step, "hooked", False):
                torch_step = torch_step.__wrapped__
            torch_step(self)
            return loss
        for gi, group, active in work:
            if not active:
                continue
            plan = self._plan(gi, active)
            torch._foreach_copy_(plan["gviews"], [p.grad for p in active])
            # the bias corrections depend on a parameter's own step count: parameters that share it share a launch
            by_step = {}
            for e in plan["entries"]:
                st = self.state[e["p"]]
                if st.get("step") is None:
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                st["step"] += 1
                by_step.setdefault(int(st["step"].item()), []).append(e)
            beta1, beta2 = group["betas"]
            for count, part in by_step.items():
                tkey = tuple(id(e["p"]) for e in part)
                tab = plan["tables"].get(tkey)
                if tab is None:
                    dev = active[0].device
                    second = torch.tensor([e["state"]["exp_avg_sq"].data_ptr() for e in part], dtype=torch.int64).to(dev)
                    tab = plan["tables"][tkey] = (*self._table(part, dev), second)
                capi.sgd_step(tab[0], len(part), tab[1], group["lr"], 0.0, group["weight_decay"], False,
                              extra=capi.adamw_extra(beta1, beta2, group["eps"], count, tab[2]))
            self._written(plan)
        return loss
