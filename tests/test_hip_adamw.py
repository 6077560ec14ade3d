"""`FusedAdamW` (dfd-clip_amd/optim.py; the AdamW form of `dfd_sgd_step`, csrc/optim.hip): the AdamW of
`Detector.configure_optimizers` (reference src/models.py:748-753) and of adapter pre-training (src/models.py:1053-1057) as
one HIP launch that also keeps the decoder's transposed weight copies current — against `torch.optim.AdamW(foreach=True)`
on the same tensors, between guard bands through the C ABI, and through the two models."""
import copy

import pytest
import torch

from tests.cases import build_case
from tests.test_hip_guarded import both, capi, rnd, verify  # noqa: F401  (capi: the module's fixture)
from tests.test_hip_optim import _Mirrors

pytestmark = pytest.mark.gpu

SHAPES = [(768, 768), (3072, 768), (768,), (30, 1, 12, 64), (1,), (2, 768), (1537, 33), (5,), (1025,), (33, 1537)]


def _bar(ref):
    return 1e-6 * max(1.0, ref.abs().max().item())


def _count_launches():
    from dfd_clip_amd import capi as c
    calls, real = [], c.sgd_step

    def counting(*a, **k):
        calls.append(k.get("extra"))
        return real(*a, **k)

    c.sgd_step = counting
    return calls, lambda: setattr(c, "sgd_step", real)


def test_fused_adamw_equals_torch_adamw_step_by_step():
    """The bar is 1e-6 * max(1, |ref|max) for parameters and both moments after every step; the worst error / bar over the
    five steps is printed before the last assertions (DESIGN §2 records what an MI355X run gave, once one is recorded)."""
    from dfd_clip_amd.optim import FusedAdamW
    g = torch.Generator(device="cuda").manual_seed(5)
    ref = [torch.nn.Parameter(torch.randn(*s, device="cuda", generator=g)) for s in SHAPES]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    mirrors = _Mirrors()
    o_ref = torch.optim.AdamW(ref, lr=0.01, weight_decay=0.01, foreach=True)
    o_mine = FusedAdamW(mine, lr=0.01, weight_decay=0.01, mirrors=mirrors)
    sched_r = torch.optim.lr_scheduler.OneCycleLR(o_ref, max_lr=0.01, total_steps=6)  # cycles betas[0] 0.95 <-> 0.85 as well
    sched_m = torch.optim.lr_scheduler.OneCycleLR(o_mine, max_lr=0.01, total_steps=6)
    calls, restore = _count_launches()
    worst = {"p": 0.0, "exp_avg": 0.0, "exp_avg_sq": 0.0}
    try:
        for step in range(5):
            for i, (a, b) in enumerate(zip(ref, mine)):
                if i == 4 and step < 2:      # a parameter that gets its first gradient late: its own step count from then on
                    a.grad = b.grad = None
                    continue
                if i == 7 and step == 3:     # ... and one that misses a step: skipped, moments and step count kept
                    a.grad = b.grad = None
                    continue
                gr = torch.randn(a.shape, device="cuda", generator=g)
                a.grad, b.grad = gr.clone(), gr.clone()
            v_before = [p._version for p in mine]
            n0 = len(calls)
            o_ref.step()
            o_mine.step()
            # one launch per distinct step count among the parameters with a gradient
            distinct = {o_ref.state[a]["step"].item() for a in ref if a.grad is not None}
            assert len(calls) - n0 == len(distinct) == {0: 1, 1: 1, 2: 2, 3: 2, 4: 3}[step]
            assert o_mine.param_groups[0]["betas"][0] == o_ref.param_groups[0]["betas"][0]
            sched_r.step()
            sched_m.step()
            for i, (a, b) in enumerate(zip(ref, mine)):
                worst["p"] = max(worst["p"], (a - b).abs().max().item() / _bar(a))
                torch.testing.assert_close(b, a, rtol=0, atol=_bar(a), msg=f"step {step} param {i}")
                if b.grad is not None:
                    assert b._version > v_before[i], "caches keyed on the version counter must see the update"
                if b.dim() == 2:
                    assert torch.equal(mirrors.t[id(b)], b.detach().t()), f"step {step}: transposed copy of param {i} is stale"
                sa, sb = o_ref.state[a], o_mine.state[b]
                assert set(sa) == set(sb)
                if sa:
                    assert sb["step"].item() == sa["step"].item() and not sb["step"].is_cuda and sb["step"].dtype == torch.float32
                    for k in ("exp_avg", "exp_avg_sq"):
                        worst[k] = max(worst[k], (sa[k] - sb[k]).abs().max().item() / _bar(sa[k]))
                        torch.testing.assert_close(sb[k], sa[k], rtol=0, atol=_bar(sa[k]), msg=f"step {step} param {i} {k}")
        print("FusedAdamW vs torch.optim.AdamW(foreach=True), worst error / bar over 5 steps:", worst)
        assert mirrors.written > 0
        assert o_mine.param_groups[0]["lr"] == pytest.approx(o_ref.param_groups[0]["lr"])

        # state_dict round trip: a resumed optimizer continues bit-identically (moments, step counts, hyper-parameters)
        sd = copy.deepcopy(o_mine.state_dict())
        resumed_p = [torch.nn.Parameter(p.detach().clone()) for p in mine]
        o_res = FusedAdamW(resumed_p, lr=0.5, weight_decay=0.5)
        o_res.load_state_dict(sd)
        for a, b, c in zip(ref, mine, resumed_p):
            gr = torch.randn(a.shape, device="cuda", generator=g)
            a.grad, b.grad, c.grad = gr.clone(), gr.clone(), gr.clone()
        o_ref.step(), o_mine.step(), o_res.step()
        for a, b, c in zip(ref, mine, resumed_p):
            assert torch.equal(b, c), "resumed from state_dict"
            assert torch.equal(o_mine.state[b]["exp_avg_sq"], o_res.state[c]["exp_avg_sq"])
            torch.testing.assert_close(b, a, rtol=0, atol=_bar(a))

        # ... and that state is torch's: a torch.optim.AdamW takes it and steps to the same place
        plain_p = [torch.nn.Parameter(p.detach().clone()) for p in mine]
        o_plain = torch.optim.AdamW(plain_p, lr=0.5, foreach=True)
        o_plain.load_state_dict(copy.deepcopy(o_mine.state_dict()))
        for b, c in zip(mine, plain_p):
            gr = torch.randn(b.shape, device="cuda", generator=g)
            b.grad, c.grad = gr.clone(), gr.clone()
        n0 = len(calls)
        o_mine.step(), o_plain.step()
        assert len(calls) - n0 == 3  # still three step counts: parameters 4 and 7 keep their own
        for i, (b, c) in enumerate(zip(mine, plain_p)):
            torch.testing.assert_close(b, c, rtol=0, atol=_bar(c), msg=f"param {i} after a torch step from the fused state")
            assert o_mine.state[b]["step"].item() == o_plain.state[c]["step"].item()
        assert all(e is not None and e.kind == 1 for e in calls)
    finally:
        restore()


def test_one_launch_per_steady_state_step_and_no_weight_decay():
    from dfd_clip_amd.optim import FusedAdamW
    g = torch.Generator(device="cuda").manual_seed(6)
    ref = [torch.nn.Parameter(torch.randn(*s, device="cuda", generator=g)) for s in [(33, 65), (1025,), (1,)]]
    mine = [torch.nn.Parameter(p.detach().clone()) for p in ref]
    o_ref = torch.optim.AdamW(ref, lr=0.01, weight_decay=0.0, foreach=True)
    o_mine = FusedAdamW(mine, lr=0.01, weight_decay=0.0, mirrors=_Mirrors())
    calls, restore = _count_launches()
    try:
        for step in range(3):
            for a, b in zip(ref, mine):
                gr = torch.randn(a.shape, device="cuda", generator=g)
                a.grad, b.grad = gr.clone(), gr.clone()
            o_ref.step(), o_mine.step()
            assert len(calls) == step + 1
            for a, b in zip(ref, mine):
                torch.testing.assert_close(b, a, rtol=0, atol=_bar(a), msg=f"weight_decay 0, step {step}")
    finally:
        restore()


def _adamw_f64(p, m, v, g, step, lr, wd, b1, b2, eps):
    p = p * (1 - lr * wd)
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    den = v.sqrt() / (1 - b2 ** step) ** 0.5 + eps
    return p - (lr / (1 - b1 ** step)) * (m / den), m, v


def test_adamw_step_between_guards(capi):
    """Params, grads, both moments and mirrors each between guards; the shapes of test_hip_guarded.py::test_sgd_step (a
    mirrored [1537, 33] weight, ragged for the transposing tiles; 1 and 5 elements); two AdamW calls with step counts 1 and
    2, then one call with extra = NULL on the same table, which must still be an SGD step (exp_avg its velocity).
    Reference: the arithmetic in f64; tolerance 1e-6 * max(1, |ref|) as that test."""
    shapes = [((1537, 33), True), ((1,), False), ((5,), False), ((8, 7), True), ((2, 768), False)]
    lr, wd, b1, b2, eps, mom = 0.01, 0.01, 0.9, 0.999, 1e-8, 0.95
    n = len(shapes)
    p0 = [rnd(*s, seed=60 + i) for i, (s, _) in enumerate(shapes)]
    gr = [[rnd(*s, seed=70 + 10 * st + i) for i, (s, _) in enumerate(shapes)] for st in range(3)]
    pr = [p.double() for p in p0]
    mr, vr = [torch.zeros_like(p) for p in pr], [torch.zeros_like(p) for p in pr]
    for i in range(n):
        for st in (1, 2):
            pr[i], mr[i], vr[i] = _adamw_f64(pr[i], mr[i], vr[i], gr[st - 1][i].double(), st, lr, wd, b1, b2, eps)
    after_adamw = [p.clone() for p in pr]
    for i in range(n):  # the third call: plain SGD, not a first step
        gg = gr[2][i].double() + wd * pr[i]
        mr[i] = mom * mr[i] + gg
        pr[i] = pr[i] - lr * mr[i]

    def op(b):
        ps = [b.out((1, p.numel()), init=p, name=f"p{i}") for i, p in enumerate(p0)]
        gs = [b.out((1, p.numel()), init=gr[0][i], name=f"g{i}") for i, p in enumerate(p0)]
        ms = [b.out((1, p.numel()), init=torch.zeros_like(p), name=f"m{i}") for i, p in enumerate(p0)]
        vs = [b.out((1, p.numel()), init=torch.zeros_like(p), name=f"v{i}") for i, p in enumerate(p0)]
        mirs = [b.out((s[1], s[0]), name=f"mirror{i}") if mir else None for i, (s, mir) in enumerate(shapes)]
        rows_, first = [], 0
        for i, (s, mir) in enumerate(shapes):
            r, c = (s[0], s[1]) if len(s) == 2 else (0, 0)
            rows_.append([ps[i].data_ptr(), gs[i].data_ptr(), ms[i].data_ptr(), mirs[i].data_ptr() if mir else 0, p0[i].numel(), r | (c << 32), first])
            first += capi.sgd_blocks(p0[i].numel(), r, c, mir)
        table = torch.tensor(rows_, dtype=torch.int64, device="cuda")
        second = torch.tensor([v.data_ptr() for v in vs], dtype=torch.int64, device="cuda")
        mid = None
        for st in range(3):
            if st:
                if b.guard:  # the gradients are inputs: nothing of them may change; then load the next step's
                    torch.cuda.synchronize()
                    for g_, _ in b.items:
                        if g_.name.startswith("g"):
                            g_.assert_untouched(view_too=True)
                for i in range(n):
                    gs[i].copy_(gr[st][i].reshape(1, -1))
                if b.guard:
                    for g_, _ in b.items:
                        if g_.name.startswith("g"):
                            g_._snap = g_.flat.clone()
            if st < 2:
                capi.sgd_step(table, n, first, lr, 0.5, wd, True, extra=capi.adamw_extra(b1, b2, eps, st + 1, second))
            else:
                mid = [p.clone() for p in ps]
                vmid = [v.clone() for v in vs]
                capi.sgd_step(table, n, first, lr, mom, wd, False, extra=None)
        out = {f"p{i}": ps[i] for i in range(n)}
        out.update({f"m{i}": ms[i] for i in range(n)})
        out.update({f"v{i}": vs[i] for i in range(n)})
        out.update({f"adamw_p{i}": mid[i] for i in range(n)})
        out.update({f"mirror{i}": mirs[i] for i, (_, mir) in enumerate(shapes) if mir})
        for i in range(n):
            assert torch.equal(vs[i], vmid[i]), "the SGD form does not touch the second moments"
        if b.guard:
            for g_, _ in b.items:
                if g_.name.startswith("g"):
                    g_.assert_untouched(view_too=True)
        return out
    d, g = both(op)
    refs = {}
    for i in range(n):
        refs[f"p{i}"] = (pr[i], 1e-6 * max(1.0, pr[i].abs().max().item()), 0.0)
        refs[f"m{i}"] = (mr[i], 1e-6 * max(1.0, mr[i].abs().max().item()), 0.0)
        refs[f"v{i}"] = (vr[i], 1e-6 * max(1.0, vr[i].abs().max().item()), 0.0)
        refs[f"adamw_p{i}"] = (after_adamw[i], 1e-6 * max(1.0, after_adamw[i].abs().max().item()), 0.0)
    verify(d, g, refs, msg="adamw_step")
    for r_ in (d, g):
        for i, (s, mir) in enumerate(shapes):
            if mir:
                assert torch.equal(r_[f"mirror{i}"], r_[f"p{i}"].view(s).t()), f"mirror {i} is not the transpose of the updated weight"


@pytest.mark.parametrize("graphs", [False, True])
def test_detector_training_with_fused_adamw_keeps_the_decoders_transposes_current(graphs):
    """Through `Detector.configure_optimizers` with `optimizer: adamw`, as test_hip_optim.py does for SGD: the optimizer is
    the fused one, the decoder launches no transpose after step 0, the parameters follow a twin stepped by
    torch.optim.AdamW, and a plain torch optimizer afterwards is caught up with.  lr = 1e-3: the reference trainer's
    default learning rate (src/trainer.py:29)."""
    from dfd_clip_amd import capi
    from dfd_clip_amd.optim import FusedAdamW
    from tests.test_hip_detector import make_detector
    case = build_case("small")
    case["cfg"].optimizer = "adamw"
    det = make_detector(case, "bf16").train()
    twin = copy.deepcopy(det)
    det.static_graphs = twin.static_graphs = graphs
    x, m, y = case["x"].cuda(), case["m"].cuda(), case["y"].cuda()
    lr = 1e-3
    opt = det.configure_optimizers(lr)
    assert isinstance(opt, FusedAdamW) and isinstance(opt, torch.optim.AdamW)
    assert opt.defaults["weight_decay"] == det.weight_decay
    opt_t = torch.optim.AdamW([p for p in twin.parameters() if p.requires_grad], lr=lr, weight_decay=twin.weight_decay)
    calls = {"n": 0}
    real = capi.transpose
    launches, restore = _count_launches()

    def counting(src, dst):
        calls["n"] += 1
        return real(src, dst)

    capi.transpose = counting
    try:
        for step in range(4):
            for d, o in ((det, opt), (twin, opt_t)):
                o.zero_grad(set_to_none=True)
                c0 = calls["n"]
                losses, logits, other = d(x, [y], m, train=True, single_task=0)
                (losses[0].mean() + sum(other.values())).backward()
                o.step()
                if d is det:
                    mine = calls["n"] - c0  # transposes launched by this model's forward / backward / optimizer
            assert len(launches) == step + 1, "one optimizer launch per step"
            if step == 0:
                assert mine > 0  # the copies are created once
            else:
                assert mine == 0, "the fused optimizer keeps the copies current: no transpose after step 0"
        worst = ("", 0.0)
        for (n, a), (_, b) in zip(det.named_parameters(), twin.named_parameters()):
            if a.requires_grad:
                worst = max(worst, (n, (a - b).abs().max().item() / (2e-5 * max(1.0, b.abs().max().item()))), key=lambda t: t[1])
        print(f"graphs={graphs}: worst parameter error / bar after 4 AdamW steps: {worst}")
        for (n, a), (_, b) in zip(det.named_parameters(), twin.named_parameters()):
            if a.requires_grad:
                torch.testing.assert_close(a, b, rtol=0, atol=2e-5 * max(1.0, b.abs().max().item()), msg=n)
        # hand the model to a plain torch optimizer: the decoder must notice that its copies went stale
        plain = torch.optim.SGD([p for p in det.parameters() if p.requires_grad], lr=0.05)
        for d, o in ((det, plain), (twin, torch.optim.SGD([p for p in twin.parameters() if p.requires_grad], lr=0.05))):
            o.zero_grad(set_to_none=True)
            losses, logits, other = d(x, [y], m, train=True, single_task=0)
            (losses[0].mean() + sum(other.values())).backward()
            o.step()
        det.eval(), twin.eval()
        with torch.no_grad():
            la = det(x, [y], m, single_task=0)[1][0]
            lb = twin(x, [y], m, single_task=0)[1][0]
        assert (la - lb).abs().max().item() < 1e-3
    finally:
        capi.transpose = real
        restore()


def test_compinv_encoder_on_the_device_hands_out_the_fused_adamw():
    from dfd_clip_amd.compinv import CompInvEncoder
    from dfd_clip_amd.optim import FusedAdamW
    from tests.compinv_cases import build_case as build_compinv_case
    case = build_compinv_case("compinv_tiny")
    model = CompInvEncoder(case["cfg"], None, num_frames=case["T"], precision="bf16")
    model.load_state_dict(case["sd"])
    model = model.to("cuda")
    opt = model.configure_optimizers(4e-4)
    assert isinstance(opt, FusedAdamW) and isinstance(opt, torch.optim.AdamW)
    assert opt.defaults["weight_decay"] == 0.01
    # one step on the device is the kernel's, not torch's: a single launch for the whole adapter
    launches, restore = _count_launches()
    try:
        before = [p.detach().clone() for p in model.adapter.parameters()]
        for p in model.adapter.parameters():
            p.grad = torch.ones_like(p)
        opt.step()
        assert len(launches) == 1
        for p, q in zip(model.adapter.parameters(), before):  # the first AdamW step moves every element by lr (1 - wd lr p)
            torch.testing.assert_close(p.detach(), q * (1 - 4e-4 * 0.01) - 4e-4, rtol=0, atol=1e-6)
    finally:
        restore()
