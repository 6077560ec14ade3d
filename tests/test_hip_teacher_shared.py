"""EMA-teacher training on the fast path (`harness.EmaTeacher(share_encoder=True, fused=True)`, `Detector.encode_clips`): the
teacher reads the student's encoder pass instead of running the shared frozen tower again, and its update is one
`dfd_ema_step` launch.  Tiny geometries of tests/cases.py (`tiny`, `tiny_pmask`, `tiny_adapter_ln`, the last also patch-masked),
two tasks, fp32 and bf16, dropout 0.5 from fixed seeds.  Everything is held bit for bit: a consumer of a handle runs the
kernels it would run on its own pass, on the same K/V."""
import functools

import numpy as np
import pytest
import torch

from tests.cases import CASES, make_config

pytestmark = pytest.mark.gpu

B, T, NP_SEED = 2, 4, 11
GEOMETRIES = {"tiny": ("tiny", {}), "tiny_pmask": ("tiny_pmask", {}), "tiny_adapter_ln": ("tiny_adapter_ln", {}),
              "tiny_adapter_ln_pmask": ("tiny_adapter_ln", dict(train_mode__patch_mask={"type": "batch", "ratio": 0.5}))}
CONFIGS = [(g, p) for g in GEOMETRIES for p in ("fp32", "bf16")]
IDS = [f"{g}-{p}" for g, p in CONFIGS]


@functools.lru_cache(maxsize=None)
def case(geometry):
    from dfd_clip_amd.weights import random_state_dict, synthetic_clips
    name, extra = GEOMETRIES[geometry]
    cfg = make_config("tiny", **dict(CASES[name][3], dropout=0.5, **extra))
    cfg.out_dim = [2, 3]
    cfg.losses = ["auc_roc", "auc_roc"]
    x, m, y = synthetic_clips(B, T, 32, seed=5)
    return dict(cfg=cfg, sd=random_state_dict(cfg, T, seed=0), x=x.cuda(), m=m.cuda(), y=y.cuda())


def make_model(geometry, precision, fast=False):
    from dfd_clip_amd.detector import Detector
    c = case(geometry)
    model = Detector(c["cfg"], T, None, precision=precision)
    model.load_state_dict(c["sd"])
    model = model.cuda().train()
    if fast:
        model.static_graphs = model.pipeline_encoder = model.inputs_ready = True
    return model


def make_teacher(model, share, fused, ratio=0.5, noise=True):
    from dfd_clip_amd.harness import EmaTeacher
    teacher = EmaTeacher(model, ema_ratio=ratio, teach_at=0, share_encoder=share, fused=fused)
    if noise:  # a teacher that differs from its student in everything it owns
        g = torch.Generator(device="cuda").manual_seed(9)
        tower = {id(p) for p in teacher.module.encoder.parameters()}  # (shared: the student's own; private: an equal copy)
        with torch.no_grad():
            for p in teacher.module.parameters():
                if id(p) not in tower:
                    p.add_(0.02 * torch.randn(p.shape, device=p.device, generator=g))
    return teacher


def bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


@pytest.mark.parametrize("geometry,precision", CONFIGS, ids=IDS)
def test_teacher_logits_from_the_students_pass_are_its_own(geometry, precision):
    c = case(geometry)
    model = make_model(geometry, precision)
    teacher = make_teacher(model, share=True, fused=False)
    assert teacher.module.encoder is model.encoder
    x, m = c["x"], c["m"]
    teacher.module.seed_dropout(5)
    with torch.no_grad():
        _, own = teacher.module(x, [None, None], m, single_task=-1)
    own = [t.clone() for t in own]
    teacher.module.seed_dropout(5)
    np.random.seed(NP_SEED)
    enc = model.encode_clips(x, train=True)
    assert enc.tower is model.encoder and (enc.b, enc.t) == (B, T) and not enc.consumed
    assert enc.layout == ("dense" if "adapter" in geometry and "pmask" not in geometry else "in_place")
    source = [t.clone() for t in enc.kv[:2]]
    with torch.no_grad():
        _, shared = teacher.module(x, [None, None], m, single_task=-1, encoded=enc)
    assert not enc.consumed, "only the producer consumes"
    assert bits(source[0], enc.kv[0]) and bits(source[1], enc.kv[1]), "a consumer left the producer's K/V as it was"
    enc.release()
    assert enc.consumed and model._enc_open is None
    for a, b in zip(own, shared):
        assert torch.isfinite(a).all() and bits(a, b), (a, b)
    # and the labels the harness hands out are those logits' softmax
    teacher.module.seed_dropout(5)
    enc = model.encode_clips(x, train=True)
    labels = teacher.labels(x, m, c["y"], 0, 2, encoded=enc)
    enc.release()
    assert labels[0] is c["y"] and bits(labels[1], own[1].softmax(dim=-1))


def student_step(model, c, use_handle):
    model.seed_dropout(7)
    np.random.seed(NP_SEED)
    model.zero_grad()
    soft = torch.tensor([[0.2, 0.5, 0.3], [0.6, 0.1, 0.3]], device="cuda")
    y = [c["y"], soft]
    if use_handle:
        enc = model.encode_clips(c["x"], train=True)
        losses, logits, other = model(c["x"], y, c["m"], train=True, single_task=None, encoded=enc)
        assert enc.consumed and model._enc_open is None
    else:
        losses, logits, other = model(c["x"], y, c["m"], train=True, single_task=None)
    (sum(l.mean() for l in losses) + sum(other.values())).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return [l.detach().clone() for l in losses], [l.detach().clone() for l in logits], grads


@pytest.mark.parametrize("geometry,precision", CONFIGS, ids=IDS)
def test_student_forward_and_gradients_with_a_handle_are_those_without(geometry, precision):
    c = case(geometry)
    model = make_model(geometry, precision)
    plain = student_step(model, c, False)
    drop0 = int(model._drop_master[1])
    held = student_step(model, c, True)
    assert int(model._drop_master[1]) == drop0, "the dropout counter advances once per predict, handle or not"
    assert len(plain[2]) > 20 and plain[2].keys() == held[2].keys()
    for a, b in zip(plain[0] + plain[1], held[0] + held[1]):
        assert torch.isfinite(a).all() and bits(a, b)
    for n in plain[2]:
        assert bits(plain[2][n], held[2][n]), n


def run_steps(geometry, precision, share, fused, fast, steps=3):
    from dfd_clip_amd.harness import train_step
    c = case(geometry)
    model = make_model(geometry, precision, fast=fast)
    teacher = make_teacher(model, share, fused, ratio=0.5, noise=False)
    opt = model.configure_optimizers(0.05)
    model.seed_dropout(7)
    teacher.module.seed_dropout(5)
    np.random.seed(NP_SEED)
    outs = []
    for _ in range(steps):
        outs.append(train_step(model, opt, [(c["x"], c["y"], c["m"], None, None, 0)], teacher=teacher))
    torch.cuda.synchronize()
    assert teacher.teaching and teacher.steps == steps
    return model, teacher, outs


def compare_arms(geometry, precision, fast):
    m0, t0, o0 = run_steps(geometry, precision, False, False, fast)
    m1, t1, o1 = run_steps(geometry, precision, True, True, fast)
    assert t1.module.encoder is m1.encoder and t0.module.encoder is not m0.encoder
    for a, b in zip(o0, o1):
        assert bits(a["losses"][0], b["losses"][0]) and bits(a["logits"][0], b["logits"][0])
    moved = 0
    for (n, p0), (_, p1) in zip(m0.named_parameters(), m1.named_parameters()):
        assert bits(p0, p1), f"student {n}"
    for (n, p0), (_, p1), (_, s1) in zip(t0.module.named_parameters(), t1.module.named_parameters(), m1.named_parameters()):
        assert bits(p0, p1), f"teacher {n}"
        moved += int(not n.startswith("encoder.") and not torch.equal(p1, s1))
    assert moved >= 4 * len(t1.module.decoder.transformer.resblocks), "the teacher trails the student (at least in every Linear weight)"
    dec0, dec1 = t0.module.decoder, t1.module.decoder
    mirrored = 0
    for (n, p0), (_, p1) in zip(dec0.named_parameters(), dec1.named_parameters()):
        cur = dec1.current_mirror(p1)
        if cur is None:
            continue
        mirrored += 1
        assert bits(cur, p0.detach().t().contiguous()), f"teacher mirror {n}"
        assert bits(cur, dec0.mirror_for(p0))
    assert mirrored == 4 * len(dec1.transformer.resblocks)


@pytest.mark.parametrize("geometry,precision", CONFIGS, ids=IDS)
def test_three_train_steps_private_unfused_against_shared_fused(geometry, precision):
    compare_arms(geometry, precision, fast=False)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_three_train_steps_with_graphs_and_the_pipelined_encoder(precision):
    compare_arms("tiny", precision, fast=True)


def test_fused_update_is_one_launch_in_place_and_no_transpose_follows(monkeypatch):
    from dfd_clip_amd import capi
    from dfd_clip_amd.harness import train_step
    c = case("tiny_adapter_ln")
    model = make_model("tiny_adapter_ln", "bf16")
    teacher = make_teacher(model, True, True, noise=False)
    opt = model.configure_optimizers(0.05)
    calls = {"ema": 0, "transpose": 0}
    real_ema, real_transpose = capi.ema_step, capi.transpose

    def ema(*a, **k):
        calls["ema"] += 1
        return real_ema(*a, **k)

    def transpose(*a, **k):
        calls["transpose"] += 1
        return real_transpose(*a, **k)

    monkeypatch.setattr(capi, "ema_step", ema)
    monkeypatch.setattr(capi, "transpose", transpose)
    batch = [(c["x"], c["y"], c["m"], None, None, 0)]
    ptrs = [p.data_ptr() for p in teacher.module.parameters()]
    versions = [p._version for p in teacher.module.parameters()]
    train_step(model, opt, batch, teacher=teacher)  # (not teaching yet: the first update plans the table and its mirrors)
    assert calls["ema"] == 1 and teacher.teaching
    first = calls["transpose"]
    for step in (2, 3):
        train_step(model, opt, batch, teacher=teacher)
        assert calls["ema"] == step
    assert calls["transpose"] == first, "the teacher's (and the student's) transposed copies are kept by the update launches"
    assert [p.data_ptr() for p in teacher.module.parameters()] == ptrs
    tower = {id(p) for p in model.encoder.parameters()}
    for p, v in zip(teacher.module.parameters(), versions):
        assert (p._version == v) == (id(p) in tower), "every blended parameter's version moved, the shared tower's did not"
    assert len(teacher._plan["entries"]) == len([p for p in teacher.module.parameters() if id(p) not in tower]) and not teacher._plan["rest"]


def test_one_tower_in_memory():
    c = case("tiny")
    model = make_model("tiny", "bf16")
    with torch.no_grad():
        model.predict(c["x"], c["m"])  # the student's tower is staged (bf16 operands, workspace) before anything is measured
    torch.cuda.synchronize()
    tower_bytes = sum(p.numel() * p.element_size() for p in model.encoder.parameters())

    def cost(share):
        """Bytes a teacher adds: (at construction, after its first forward of its own)."""
        base = torch.cuda.memory_allocated()
        teacher = make_teacher(model, share, False, noise=False)
        built = torch.cuda.memory_allocated() - base
        with torch.no_grad():
            teacher.module.predict(c["x"], c["m"])
        torch.cuda.synchronize()
        return teacher, built, torch.cuda.memory_allocated() - base

    private, built_private, run_private = cost(False)
    del private
    shared, built_shared, run_shared = cost(True)
    assert shared.module.encoder is model.encoder
    # the parameters at construction; after a forward the private tower's staged operands come on top
    assert tower_bytes > 0 and built_private - built_shared >= tower_bytes, (built_private, built_shared, tower_bytes)
    assert run_private - run_shared > built_private - built_shared, (run_private, run_shared, built_private, built_shared)
    assert len(shared.module.state_dict()) == len(model.state_dict())


def test_the_raises():
    from dfd_clip_amd.capi import DfdError
    c = case("tiny")
    x, m = c["x"], c["m"]
    model = make_model("tiny", "bf16").eval()
    teacher = make_teacher(model, True, False)
    stranger = make_teacher(model, False, False)
    with torch.no_grad():
        enc = model.encode_clips(x)
        with pytest.raises(DfdError, match="still open"):
            model.encode_clips(x)
        with pytest.raises(DfdError, match="still open"):
            model.predict(x, m)
        with pytest.raises(DfdError, match="another tower"):
            stranger.module.predict(x, m, encoded=enc)
        with pytest.raises(DfdError, match="shape"):
            teacher.module.predict(x[:1], m[:1], encoded=enc)
        with pytest.raises(DfdError, match="frame mask"):
            teacher.module.predict(x, m[:1], encoded=enc)
        with pytest.raises(DfdError, match="same mode"):
            model.predict(x, m, train=True, encoded=enc)
        first, _ = teacher.module.predict(x, m, encoded=enc)
        own, _ = model.predict(x, m, encoded=enc)
        assert enc.consumed
        with pytest.raises(DfdError, match="consumed or released"):
            teacher.module.predict(x, m, encoded=enc)
        enc2 = model.encode_clips(x)
        with pytest.raises(DfdError, match="stale"):
            teacher.module.predict(x, m, encoded=enc)
        with pytest.raises(DfdError, match="stale"):
            model.predict(x, m, encoded=enc)
        again, _ = model.predict(x, m, encoded=enc2)
        assert bits(own[0], again[0]) and not bits(own[0], first[0])
        model.kv_in_place = False
        with pytest.raises(DfdError, match="kv_in_place"):
            model.encode_clips(x)
        model.kv_in_place = True
        model.encode_clips(x).release()
        model.predict(x, m)
