"""Reference-shaped callers of the model boundary: train step, evaluation pass, per-video inference.

These restate the CONTRACTS of the reference's host loops in this repo's own
code, so that a reference user finds the same step semantics on top of `Detector`:

  train_step      `Trainer.run`'s loop body (`src/trainer.py:108-177`): zero_grad -> for each training
                  set: forward(train=True, single_task=idx) -> backward(task_loss[idx].mean() + Σ other)
                  -> [gradient all-reduce] -> optimizer.step -> lr_scheduler.step.  `augment=`: the datasets'
                  colour / JPEG / flip augmentation (`src/datasets.py:288-399`) applied to each batch's uint8 device
                  clips first (`augment.ClipAugment`); `ssl_fake=`: the self-supervised fakes (`:401-418`, `:667-669`)
                  made from the batch's real clips after that (`elastic.SslFake`).
  make_one_cycle  the OneCycleLR the trainer builds (`src/trainer.py:51-60`): initial lr = max/25 and
                  `total_steps = max_steps * num_processes` because Accelerate steps a prepared
                  scheduler once per process per optimizer step; `step_scheduler` mirrors that.
  EmaTeacher      the trainer's "teacher" mode (`src/trainer.py:66-69`, `:124-137`, `:179-190`): a deep copy of
                  the model updated as an exponential moving average after every optimizer step; once
                  `teach_at` steps have passed it supplies soft labels for the tasks a batch has no labels for.
  evaluate        `Evaluator.run` (`src/evaluator.py:50-97`) + the metric callbacks
                  (`src/callbacks/metrics.py:86-155`): no_grad, eval(), model(x, y_list, m, single_task)
                  -> softmax -> gather over ranks -> accuracy / AUROC on p[:, 1].
  compinv_train_step / compinv_evaluate
                  `CompInvTrainer.run` / `CompInvEvaluator.run` (`src/trainer.py:263-303`, `src/evaluator.py:138-172`):
                  the adapter pre-training step (forward -> backward(recon + match) per batch, one optimizer
                  step) and its no_grad evaluation pass.
  infer_videos    `inference.py:105-162`: per video, chunks of `batch_size` clips -> predict -> softmax ->
                  clip- or video-level (mean over clips) probabilities -> gather -> accuracy / AUROC with
                  the dummy [0, 1] pair the reference appends before computing.
  infer_raw_video `pipeline.py:114-182` + `:328-351`: decoded frames (RGB tensors, or the decoder's 4:2:0 surfaces as a
                  `yuv.Yuv420`) + landmarks -> face-aligned crops on the device (`align.FaceAligner`) -> clips of num_frames, ragged tail dropped -> predict in chunks -> softmax ->
                  mean over clips -> probability of class 1.  `hop=`: overlapping windows over a per-frame K/V store
                  (`stream.StreamingVerdict`, exported here too) instead of disjoint clips.
"""
import copy
import logging

import torch
from torch.optim.lr_scheduler import OneCycleLR

from . import capi
from . import dist as ddist
from .stream import StreamingVerdict

_log = logging.getLogger(__name__)


def make_one_cycle(optimizer, learning_rate, max_steps, num_processes=None):
    n = num_processes or ddist.world_size()
    return OneCycleLR(optimizer=optimizer, max_lr=learning_rate, total_steps=max_steps * n)


def step_scheduler(scheduler, num_processes=None):
    for _ in range(num_processes or ddist.world_size()):
        scheduler.step()


class EmaTeacher:
    """EMA copy of the model that labels the tasks a batch does not cover (reference
    `src/trainer.py:66-69` deep copy, `:179-185` update p_t <- (1-r) p_t + r p, `:188-190` teaching
    starts once `teach_at < steps`, `:124-137` pseudo labels = softmax of the teacher's logits).

    Two opt-in switches take the mode onto the fast path; with both off this is the reference's loop, op for op.

    `share_encoder`: the copy keeps the model's frozen tower instead of duplicating it (`teacher.module.encoder is
    model.encoder`: one set of tower parameters, staged operands and fp8 scales), `update` leaves the shared parameters
    alone, and `train_step` runs ONE encoder pass per batch that teacher and student both read (`Detector.encode_clips`).
    The reference blends its copy of the tower with the tower it was copied from every step; in f32 that self-blend is
    not the identity ((1 - r) x + r x != x for about one element in six at r = 0.999, exact at r = 0.5), so its teacher's tower
    drifts from the frozen weights by rounding.  Here the teacher reads the frozen tower itself: the one deliberate deviation.

    `fused`: `update` is one `dfd_ema_step` launch over every parameter pair that is contiguous f32 on the GPU, in place —
    the teacher's parameters keep their addresses, its decoder's transposed weight copies are rewritten by the same launch
    (no transpose runs afterwards) and version-keyed caches see the change.  The arithmetic is the torch expression's, bit
    for bit.  Pairs the kernel does not cover are blended by the torch expression (in place) and logged once."""

    def __init__(self, model, ema_ratio, teach_at, share_encoder=False, fused=False):
        self.share_encoder = bool(share_encoder)
        self.fused = bool(fused)
        if self.share_encoder:
            tower = model.encoder
            self.module = copy.deepcopy(model, memo={id(tower): tower})
        else:
            self.module = copy.deepcopy(model)
        self.ema_ratio = float(ema_ratio)
        self.teach_at = int(teach_at)
        self.steps = 0
        self.teaching = False
        self._pairs = None   # fused: (student model, [(teacher parameter, student parameter), ...] without aliased pairs)
        self._plan = None
        self._told = False

    @torch.no_grad()
    def update(self, model):
        r = self.ema_ratio
        if self.fused:
            self._update_fused(model, r)
        else:
            for p1, p2 in zip(self.module.parameters(), model.parameters()):
                if p1 is p2:
                    continue  # share_encoder: the tower is the student's own; re-seating its .data would re-seat the student's
                p1.data = (1 - r) * p1.data + r * p2.data
        self.steps += 1
        if not self.teaching and self.teach_at < self.steps:
            self.teaching = True

    # ---- fused update: one dfd_ema_step launch ------------------------------------------------------------------------
    @staticmethod
    def _fusable(p1, p2):
        return all(p.dtype == torch.float32 and p.is_cuda and p.is_contiguous() for p in (p1, p2)) and p1.shape == p2.shape \
            and p1.device == p2.device and p1.data_ptr() != p2.data_ptr() and p1.numel() > 0

    def _ema_plan(self, pairs):
        """Device table of the pairs the kernel covers (+ the pairs it does not), planned once and again when a parameter's
        address or a transposed copy changed — `optim._TablePlans._plan`'s rule."""
        mirrors = getattr(self.module, "decoder", None)
        if not hasattr(mirrors, "mirror_for"):
            mirrors = None
        key = tuple((p1.data_ptr(), p2.data_ptr(), tuple(p1.shape)) for p1, p2 in pairs)
        plan = self._plan
        if plan is not None and plan["key"] == key and all(
                e[2] is None or mirrors.current_mirror(e[0]) is e[2] for e in plan["entries"]):
            return plan
        entries, rest, rows, first = [], [], [], 0
        for p1, p2 in pairs:
            if not self._fusable(p1, p2) or (entries and p1.device != entries[0][0].device):
                rest.append((p1, p2))
                continue
            m = mirrors.mirror_for(p1) if (mirrors is not None and p1.dim() == 2) else None
            nr, nc = p1.shape if m is not None else (0, 0)
            entries.append((p1, p2, m))
            rows.append([p1.data_ptr(), p2.data_ptr(), 0, 0 if m is None else m.data_ptr(), p1.numel(), int(nr) | (int(nc) << 32), first])
            first += capi.sgd_blocks(p1.numel(), nr, nc, m is not None)
        host = torch.tensor(rows, dtype=torch.int64).view(-1, 7)
        plan = dict(key=key, entries=entries, rest=rest, host=host, table=host.to(entries[0][0].device) if entries else None,
                    blocks=first, params=[e[0] for e in entries], written=[(e[0], e[2]) for e in entries if e[2] is not None],
                    mirrors=mirrors)
        self._plan = plan
        return plan

    def _update_fused(self, model, r):
        if self._pairs is None or self._pairs[0] is not model:  # the module trees are static: walk them once
            self._pairs = (model, [(p1, p2) for p1, p2 in zip(self.module.parameters(), model.parameters()) if p1 is not p2])
        plan = self._ema_plan(self._pairs[1])
        if plan["entries"]:
            capi.ema_step(plan["table"], len(plan["entries"]), plan["blocks"], r, table_host=plan["host"])
            # the kernel wrote through raw pointers: caches keyed on a parameter's version counter must see the update
            # (the call takes an ITERABLE of tensors), and the transposed copies it rewrote are current
            torch._C._increment_version(plan["params"])
            if plan["written"]:
                plan["mirrors"].mirrors_written(plan["written"])
        if plan["rest"]:
            if not self._told:
                self._told = True
                _log.warning("EmaTeacher(fused=True): %d parameter pair(s) are not contiguous f32 on one GPU: blended with torch's "
                             "own kernels", len(plan["rest"]))
            for p1, p2 in plan["rest"]:
                p1.data.copy_((1 - r) * p1.data + r * p2.data)

    @torch.no_grad()
    def labels(self, frames, mask, labels, task_index, total_tasks, encoded=None):
        """Per-task label list: the batch's own labels for its task, the teacher's class probabilities
        for every other task (the model's losses accept probability targets).  `encoded`: the student's
        `Detector.encode_clips` handle of these frames — the teacher then runs no encoder pass of its own (`share_encoder`)."""
        extra = {} if encoded is None else {"encoded": encoded}
        _, teacher_logits = self.module(frames, [None] * total_tasks, mask, single_task=-1, **extra)
        return [labels if i == task_index else teacher_logits[i].softmax(dim=-1) for i in range(total_tasks)]


def _augmented(frames, augment):
    """The batch's frames through `augment` (an `augment.ClipAugment`): uint8 device clips only, since the augmentation
    is defined on 8-bit samples and runs on the GPU."""
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8):
        raise TypeError("augment= needs uint8 device frames [B,T,3,H,W]; got "
                        f"{getattr(frames, 'dtype', type(frames))} on {getattr(frames, 'device', 'the host')}")
    return augment(frames)


def _ssl_faked(frames, labels, ssl_fake):
    """The batch through `ssl_fake` (an `elastic.SslFake`): (frames, labels) with the chosen real clips warped and relabelled;
    uint8 device clips only, as for `augment`."""
    if not (torch.is_tensor(frames) and frames.is_cuda and frames.dtype == torch.uint8):
        raise TypeError("ssl_fake= needs uint8 device frames [B,T,3,H,W]; got "
                        f"{getattr(frames, 'dtype', type(frames))} on {getattr(frames, 'device', 'the host')}")
    return ssl_fake(frames, labels)


def train_step(model, optimizer, batches, scheduler=None, total_tasks=None, teacher=None, augment=None, ssl_fake=None):
    """One optimizer step over `batches`: list of (frames, labels, mask, comps, speed, task_index)
    — one entry per training set, as the reference draws one batch per set per step.
    With an `EmaTeacher` that has started teaching, every task contributes a loss (the other tasks
    against the teacher's soft labels); the teacher is updated after the optimizer step.  A teaching teacher built with
    `share_encoder` labels each batch from the student's own encoder pass (`Detector.encode_clips` -> `teacher.labels(...,
    encoded=)` -> `model(..., encoded=)`): one pass through the frozen tower per batch instead of two.
    `augment`: an `augment.ClipAugment`; each batch's uint8 device frames go through it (one fresh draw per batch) before
    the model and the teacher see them, as the reference's datasets augment before collation.
    `ssl_fake`: an `elastic.SslFake`; after `augment` (the reference's order, `src/datasets.py:665-668`) each batch's real
    clips whose coin fired are warped elastically and labelled fake, on the device and without a sync.
    Returns {"losses": [...per batch mean task loss...], "logits": [...]}."""
    total_tasks = total_tasks or len(model.out_dim)
    model.zero_grad()
    model.train()
    out = {"losses": [], "logits": []}
    teaching = teacher is not None and teacher.teaching
    shared = teaching and bool(getattr(teacher, "share_encoder", False))
    for frames, labels, mask, comps, speed, task_index in batches:
        if augment is not None:
            frames = _augmented(frames, augment)
        if ssl_fake is not None:
            frames, labels = _ssl_faked(frames, labels, ssl_fake)
        if shared:
            # one encoder pass, two consumers: the teacher reads the student's K/V first, then the student consumes it
            # (which is what lets the next pass into that K/V set start)
            enc = model.encode_clips(frames, train=True)
            try:
                y_list = teacher.labels(frames, mask, labels, task_index, total_tasks, encoded=enc)
                task_losses, task_logits, other = model(frames, y_list, mask, comps, speed, train=True, single_task=None, encoded=enc)
            finally:
                enc.release()  # (nothing to do after the student's forward; after an error it frees the model for the next pass)
        else:
            if teaching:
                y_list = teacher.labels(frames, mask, labels, task_index, total_tasks)
            else:
                y_list = [labels if i == task_index else None for i in range(total_tasks)]
            task_losses, task_logits, other = model(frames, y_list, mask, comps, speed, train=True,
                                                    single_task=None if teaching else task_index)
        if teaching:
            loss = sum(l.mean() for l in task_losses) + sum(other[k].mean() for k in other)
        else:
            loss = task_losses[task_index].mean() + sum(other[k].mean() for k in other)
        loss.backward()
        out["losses"].append(task_losses[task_index].detach())
        out["logits"].append(task_logits[task_index].detach())
    ddist.allreduce_gradients([p for p in model.parameters() if p.requires_grad])
    optimizer.step()
    if scheduler is not None:
        step_scheduler(scheduler)
    model.zero_grad()
    if teacher is not None:
        teacher.update(model)
    return out


def compinv_train_step(model, optimizer, batches, scheduler=None, augment=None):
    """One `CompInvTrainer` step for a `CompInvEncoder`: `batches` = list of (frames, comp), one per training set;
    `augment` as for `train_step`.
    Returns {"recon": [...], "match": [...]}, detached 0-dim device tensors per batch."""
    model.zero_grad()
    model.train()
    out = {"recon": [], "match": []}
    for frames, comp in batches:
        if augment is not None:
            frames = _augmented(frames, augment)
        recon, match = model(frames, comp)
        (recon + match).backward()
        out["recon"].append(recon.detach())
        out["match"].append(match.detach())
    ddist.allreduce_gradients([p for p in model.parameters() if p.requires_grad])
    optimizer.step()
    if scheduler is not None:
        step_scheduler(scheduler)
    model.zero_grad()
    return out


@torch.no_grad()
def compinv_evaluate(model, batches):
    """`CompInvEvaluator.run`: eval(), no_grad, model(frames, comp) per batch -> {"recon": [...], "match": [...]}."""
    model.eval()
    out = {"recon": [], "match": []}
    for frames, comp in batches:
        recon, match = model(frames, comp)
        out["recon"].append(recon)
        out["match"].append(match)
    return out


def binary_auroc(labels, scores):
    """Area under the ROC curve of `scores` for the positive class 1 (ties get the average rank);
    what sklearn.metrics.roc_auc_score — the backend of the reference's `roc_auc` metric — returns."""
    labels = torch.as_tensor(labels).flatten().to(torch.float64)
    scores = torch.as_tensor(scores).flatten().to(torch.float64)
    n_pos = labels.sum().item()
    n_neg = labels.numel() - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("AUROC needs both classes")
    order = torch.argsort(scores)
    s = scores[order]
    ranks = torch.empty_like(s)
    i, n = 0, s.numel()
    while i < n:  # average ranks over ties
        j = i
        while j + 1 < n and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = (i + j) / 2.0 + 1.0
        i = j + 1
    r = torch.empty_like(ranks)
    r[order] = ranks
    return ((r[labels == 1].sum().item() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


@torch.no_grad()
def evaluate(model, batches, total_tasks=None):
    """batches: iterable of (frames, labels, mask, task_index[, valid]) for this rank; `valid` = number
    of real samples when the last batch was padded to a common size across ranks.
    Returns dict(accuracy, roc_auc, loss, labels, probs) over ALL ranks' samples."""
    total_tasks = total_tasks or len(model.out_dim)
    model.eval()
    all_labels, all_probs, all_losses = [], [], []
    for batch in batches:
        frames, labels, mask, task_index = batch[:4]
        valid = batch[4] if len(batch) > 4 else None
        y_list = [labels if i == task_index else None for i in range(total_tasks)]
        task_losses, task_logits = model(frames, y_list, mask, single_task=task_index)
        probs = task_logits[task_index].detach().softmax(dim=-1)
        lab, pr, ls = ddist.gather_for_metrics((labels, probs, task_losses[task_index].detach()), valid=valid)
        all_labels.append(lab.cpu())
        all_probs.append(pr.cpu())
        all_losses.append(ls.cpu())
    labels, probs, losses = torch.cat(all_labels), torch.cat(all_probs), torch.cat(all_losses)
    res = dict(accuracy=(probs.argmax(dim=-1) == labels).float().mean().item(), loss=losses.mean().item(), labels=labels,
               probs=probs)
    try:
        res["roc_auc"] = binary_auroc(labels, probs[:, 1])
    except ValueError:
        res["roc_auc"] = float("nan")
    return res


@torch.no_grad()
def infer_videos(model, videos, batch_size=30, modality="video", task_index=0, device=None):
    """videos: iterable of (clips list of [T,3,R,R], label(s), masks list of [T]) for this rank; a video
    without clips is skipped, as the reference does.  Returns dict(accuracy, roc_auc, labels, probs)."""
    model.eval()
    device = device or next(model.parameters()).device
    labels_all, probs_all = [], []
    for clips, label, masks in videos:
        if len(clips) == 0:
            continue
        logits = []
        for i in range(0, len(clips), batch_size):  # last chunk ragged
            x = torch.stack(clips[i:i + batch_size]).to(device)
            m = torch.stack(masks[i:i + batch_size]).to(device)
            logits.append(model.predict(x, m)[0][task_index].detach().to("cpu"))
        p = torch.cat(logits).softmax(dim=-1)
        if modality == "clip":
            pred_prob, lab = p, torch.as_tensor(label).reshape(-1)
        elif modality == "video":
            pred_prob = p.mean(dim=0).unsqueeze(0)
            lab = torch.as_tensor(label).reshape(-1)[:1]
        else:
            raise NotImplementedError()
        n = ddist.world_size()
        if n > 1:  # ranks hold different numbers of rows per video in clip mode: pad to the maximum
            cnt = torch.tensor([pred_prob.shape[0]], dtype=torch.int64, device=device)
            mx = cnt.clone()
            torch.distributed.all_reduce(mx, op=torch.distributed.ReduceOp.MAX)
            pad = int(mx.item()) - pred_prob.shape[0]
            pp = torch.cat([pred_prob, pred_prob.new_zeros(pad, pred_prob.shape[1])]).to(device)
            ll = torch.cat([lab, lab.new_zeros(pad)]).to(device)
            ll, pp = ddist.gather_for_metrics((ll, pp), valid=pred_prob.shape[0])
            lab, pred_prob = ll.cpu(), pp.cpu()
        labels_all.append(lab)
        probs_all.append(pred_prob)
    labels, probs = torch.cat(labels_all), torch.cat(probs_all)
    # the reference appends one dummy sample of each class before computing (inference.py:159-160)
    lab2 = torch.cat([labels, torch.tensor([0, 1])])
    sc2 = torch.cat([probs[:, 1], torch.tensor([0.0, 1.0])])
    pred2 = torch.cat([probs.argmax(dim=-1), torch.tensor([0, 1])])
    return dict(accuracy=round((pred2 == lab2).float().mean().item(), 3), roc_auc=round(binary_auroc(lab2, sc2), 3),
                labels=labels, probs=probs)


@torch.no_grad()
def infer_raw_video(model, frames, landmarks, aligner, batch_size=16, task_index=0, layout="hwc", swap_rb=False, with_logits=False,
                    matrix=None, hop=None, tail="drop", encode_chunk=None, gather="copy"):
    """One decoded video to a verdict, as `pipeline.get_result` does after its file handling (`pipeline.py:328-351`), with
    the face alignment it reads from a pre-cropped file done here on the device (`align.FaceAligner`).

    frames: uint8 device frames [F,H,W,3] (`layout="hwc"`) or [F,3,H,W]; landmarks [F,68,2]; `aligner.plan` /
    `aligner.apply` turn them into [F,3,crop,crop] crops.  A `yuv.Yuv420` (the decoder's NV12 / I420 surfaces on the device)
    goes through `aligner.apply_yuv` with `matrix` (`yuv.matrix(...)`, default BT.601 limited range) instead; `layout` and
    `swap_rb` do not apply to it (NV21 is `Yuv420.nv12(..., swap_uv=True)`).  The frames are cut into clips of `model.num_frames`
    consecutive frames, a ragged last clip is dropped (`pipeline.py:334-336`), `predict` runs on uint8 clips in chunks of
    `batch_size` with `plan.valid` (frames with a face) as the mask, and the softmax is averaged over clips.
    Returns (probability of class 1, per-clip probabilities [clips, classes]) on the host; `with_logits` appends the
    per-clip logits.

    `hop` (an integer; None is the path above, untouched): overlapping windows of `model.num_frames` frames every `hop`
    frames, through a `stream.StreamingVerdict` fed with the crops in passes of `encode_chunk` frames (default
    `batch_size * num_frames`, the tower pass of the path above): every frame goes through the tower once, the K/V ring
    holds `num_frames + encode_chunk` frames whatever the length of the video, and "clips" above reads "windows".
    `tail` is `stream.window_table`'s: "drop" as above, "last" adds the window that ends on the last frame.  `gather` is
    `StreamingVerdict`'s ("copy", "table" or "auto": whether the decoder reads a gathered copy of the windows' frames or the
    ring in place; the same bits).  Under
    `precision="fp8"` the verdict depends on `encode_chunk` (`stream`'s note)."""
    model.eval()
    plan = aligner.plan(landmarks)
    from .yuv import Yuv420
    if isinstance(frames, Yuv420):
        if swap_rb:
            raise ValueError("swap_rb is for interleaved BGR tensors; a Yuv420 source names its own u and v planes")
        crops = aligner.apply_yuv(frames, plan, matrix=matrix)
    else:
        if matrix is not None:
            raise ValueError("matrix= converts a yuv.Yuv420 source; RGB tensors take none")
        crops = aligner.apply(frames, plan, layout=layout, swap_rb=swap_rb)
    T = int(model.num_frames)
    n = crops.shape[0] // T
    if n == 0:
        raise ValueError(f"{crops.shape[0]} frames do not fill one clip of {T}")
    if hop is not None:
        chunk = int(encode_chunk) if encode_chunk is not None else batch_size * T
        sv = StreamingVerdict(model, hop, encode_chunk=chunk, batch_size=batch_size, task_index=task_index, tail=tail, gather=gather)
        for i in range(0, crops.shape[0], chunk):
            sv.push(crops[i:i + chunk], plan.valid[i:i + chunk])
        sv.flush()
        return sv.result(with_logits=with_logits)
    clips = crops[:n * T].view(n, T, *crops.shape[1:])
    mask = torch.from_numpy(plan.valid[:n * T].copy()).view(n, T).to(crops.device)
    logits = []
    for i in range(0, n, batch_size):
        logits.append(model.predict(clips[i:i + batch_size], mask[i:i + batch_size])[0][task_index].detach().to("cpu"))
    logits = torch.cat(logits)
    p = logits.softmax(dim=-1)
    res = (p.mean(dim=0)[1], p)
    return res + (logits,) if with_logits else res


# ---- patch saliency guides (train_mode.patch_mask.type: guide) -----------------------------------------------------

@torch.no_grad()
def saliency_guide(model, batches):
    """The map `patch_mask.type: guide` samples from (reference models.py:533-539: `guide_map['v'][layer]`), measured on
    this model: |aff| of `predict(with_attention=True)` averaged over clips, unpadded frames and heads, per tapped layer,
    accumulated on the device.  `batches`: an iterable of (frames [B,T,3,R,R], mask [B,T]).
    -> {"v": float64 ndarray [tower layers, g, g]}; each tapped layer's map sums to 1, untapped layers are uniform."""
    import numpy as np
    m = getattr(model, "module", model)
    acc, frames = None, 0
    for x, mask in batches:
        _, features = m.predict(x, mask, with_attention=True)
        a = torch.stack(features["attention"]).abs().to(torch.float64)  # [L, B, heads, T, P]; padded frames are 0
        part = a.sum(dim=(1, 3)).mean(dim=1)                             # [L, P]
        acc = part if acc is None else acc + part
        frames += int(mask.sum())
    if acc is None or frames == 0:
        raise ValueError("saliency_guide: no unpadded frame in `batches`")
    acc = (acc / frames).cpu().numpy()
    patches = acc.shape[1]
    g = int(round(patches ** 0.5))
    if g * g != patches:
        raise ValueError(f"{patches} patches are not a square grid")
    layers = len(m.encoder.transformer.resblocks) if hasattr(m.encoder, "transformer") else max(m.layer_indices) + 1
    v = np.full((layers, g, g), 1.0 / patches, dtype=np.float64)
    for i, l in enumerate(m.layer_indices):
        tot = acc[i].sum()
        if not np.isfinite(tot) or tot <= 0:
            raise ValueError(f"saliency_guide: layer {l} has no finite attention mass")
        v[l] = (acc[i] / tot).reshape(g, g)
    return {"v": v}


_GUIDE_HINT = ("guide maps are read and written as .npz only (no unpickling of foreign files); convert the reference's pickle "
               "once, where you trust it: np.savez(path, v=np.stack([guide_map['v'][l] for l in range(layers)]))")


def save_guide(path, guide):
    """Writes {"v": [layers, g, g]} as an .npz (float64)."""
    import numpy as np
    if not str(path).endswith(".npz"):
        raise ValueError(f"{path}: {_GUIDE_HINT}")
    v = np.asarray(guide["v"], dtype=np.float64)
    if v.ndim != 3 or v.shape[1] != v.shape[2]:
        raise ValueError(f"guide 'v' must be [layers, g, g], got {v.shape}")
    np.savez(path, v=v)


def load_guide(path):
    """-> {"v": float64 ndarray [layers, g, g]} from an .npz written by `save_guide` (allow_pickle=False)."""
    import numpy as np
    if not str(path).endswith(".npz"):
        raise ValueError(f"{path}: {_GUIDE_HINT}")
    with np.load(path, allow_pickle=False) as z:
        if "v" not in z.files:
            raise ValueError(f"{path}: no array 'v' ({_GUIDE_HINT})")
        v = np.asarray(z["v"], dtype=np.float64)
    if v.ndim != 3 or v.shape[1] != v.shape[2]:
        raise ValueError(f"{path}: 'v' must be [layers, g, g], got {v.shape}")
    return {"v": v}
