"""Self-training of the two-domain step (train.py): everything ``train_kwargs["lambda_pl"]`` switches on, in one policy object."""
import contextlib
from typing import NamedTuple

import torch

from . import gradsink, pselab
from .losses import cross_entropy_pair, cross_entropy_soft_pair
from .stepopts import POSITIVE, StepOption, number


class Target(NamedTuple):
    """What one head's target rows learn from.  Hard: ``value`` = int64 labels [n].  Soft: ``value`` = the teacher's logits [n, C],
    ``other`` = the other modality's for "ensemble", ``threshold`` = None, a float, or the head's [C] row of adaptive thresholds."""
    value: torch.Tensor
    other: torch.Tensor = None
    threshold: object = None


@contextlib.contextmanager
def _as_teacher(model, ema):
    """The model computes with the teacher's weights in eval mode - no dropout mask is drawn, no running statistic updated - and
    claims no gradient sink (no backward follows these forwards); every module's mode is put back as it was.  ``applied()`` marks the
    packed 16-bit weights stale twice (conv2d.PARAM_EPOCH): the eager eval trunk repacks on first use, the student's graphs repack as
    their first node anyway."""
    modes = [(m, m.training) for m in model.modules()]
    try:
        with ema.applied(), gradsink.suspended():
            model.eval()
            yield
    finally:
        for m, was in modes:
            m.training = was


class SelfTraining(StepOption):
    """Self-training (the second round: pselab.export_pseudo_labels -> the loaders' ``pselab_paths=`` -> here): with
    ``lambda_pl`` > 0 each main head also learns from the pseudo labels of the TARGET batch, loss_2d += lambda_pl * pl2d and
    loss_3d += lambda_pl * pl3d, logged as ``{stage}/pl_loss_tgt_2d`` / ``_3d``.  pl* = unweighted cross entropy of the head's
    target rows, ignore_index -100 (a refined-away point), mean over the counted rows.  The class weights are left out on
    purpose: they describe the SOURCE label distribution.  A target batch whose pseudo labels are all -100 contributes loss 0
    and a zero gradient (losses.cross_entropy_pair), not torch's 0/0.  ``pseudo_labels``: "own" = the 2D head learns from
    ``pseudo_label_2d`` and the 3D head from ``pseudo_label_3d``; "ensemble" = both from ``pseudo_label_ensemble``.
    0.0 (default): the step is exactly the step without the option - pseudo-label keys of the batch are ignored.
    ``pseudo_label_source``: where the pseudo labels come from (consulted only with ``lambda_pl`` > 0).  "batch" (default): the batch's
    ``pseudo_label_*`` keys, as above.  "teacher": the mean teacher labels the target batch inside the step - before the
    student's forward the model computes the target rows in eval mode with the teacher's weights (``ema.applied()``, no_grad)
    and ONE launch turns the two logit matrices into the int64 labels of both heads (pselab.teacher_labels; "own" / "ensemble"
    as above); after the step the teacher follows the student as always.  ``pseudo_label_*`` keys of the batch are ignored.
    ``pl_threshold`` (teacher source only): None keeps every label, a float in (0, 1] refuses labels whose confidence is
    below it, "median" applies the loaders' refinement rule over this batch's target rows (per class min(lower median, 0.9),
    mm_pselab_refine per output).  What was used: ``last_teacher`` = dict(label_2d, label_3d, kept) and the logged
    ``train/pl_kept_2d`` / ``_3d`` (kept share of the target rows), all device tensors.
    "adaptive" (teacher source only; hard and soft targets, "own" and "ensemble"): FreeMatch's self-adaptive per-class
    thresholds (pselab.AdaptiveThreshold, mm_pl_adapt).  Per output a running confidence level tau and a running class mass
    pt[c] - EMAs with ``pl_threshold_momentum`` (default 0.999; ``pl_threshold_warmup``: min(momentum, (1 + t) / (10 + t)),
    as ``ema_warmup``) over the target batches - give thr[c] = pt[c] / max(pt) * tau; every target batch updates them
    first and is then judged by them, a row by the threshold of its own class.  The state lives on the device and no host
    read is added.  The update is NOT gated by the loss-scale skip or by the data-parallel reducer's flag: the teacher's
    predictions are valid whether or not the student's step is taken.  KNOWN GAP: under data parallelism the state is per
    rank (each rank sees its own target batches) and is not reduced.  ``pl_adaptive``: the object, built with the first
    teacher pass (the class count is known then), None without the option or with ``lambda_pl`` 0; ``last_teacher`` gains
    "threshold" (float32 [2, C], this step's), the logs ``train/pl_tau_2d`` / ``_3d``, the checkpoint "pl_adaptive".
    ``pl_targets``: what the target rows learn from (consulted only with ``lambda_pl`` > 0).  "hard" (default): int64 pseudo labels, as
    above, launch for launch the step without the option.  "soft": the teacher's DISTRIBUTION - each head's target rows take
    losses.cross_entropy_soft_pair against softmax(teacher logits / ``pl_temperature``) ("own": the 2D head the teacher's 2D
    logits, the 3D head its 3D logits; "ensemble": both heads the average of the two softmaxes), rows kept by their
    confidence at temperature 1 against ``pl_threshold`` (None or a float; "median" works on labels and is refused), mean
    over the kept rows, no T^2 factor.  Source "teacher": the teacher pass runs as above without the label launch, and
    ``last_teacher`` = dict(logit_2d, logit_3d, kept); source "batch": the target batch carries ``teacher_logit_2d`` /
    ``teacher_logit_3d`` [n, C] (a frozen teacher of the caller's own).  Both log ``train/pl_kept_2d`` / ``_3d``.
    ``pl_agreement`` (consulted only with ``lambda_pl`` > 0): None (default) = the step is launch for launch the step without the
    option.  A finite number > 0 = ``beta``: every target row's pseudo-label term, in both heads, is scaled by
    w = exp(-beta * D), D = half the Jeffreys divergence between the 2D and the 3D prediction of the row
    (pselab.agreement_weights, mm_pl_agree) - the second signal next to the confidence: two sensors that contradict each other
    at high confidence pull less, two that agree keep their full weight.  The thresholds decide which rows are counted or kept
    exactly as without the option and ``pl_kept_*`` is unchanged; the weights scale the rows that remain and are not in the
    losses' denominators (losses.cross_entropy_pair ``row_weight_tail``, cross_entropy_soft_pair ``row_weight``); they carry no
    gradient.  Works with every source / targets / "own" - "ensemble" / threshold combination.  The two logit matrices: source
    "teacher": the teacher's (one extra call in the teacher pass); source "batch" with soft targets: the batch's
    ``teacher_logit_2d`` / ``_3d``; source "batch" with hard labels (the file-based round): the student's own main-head target
    rows of this step, detached.  No state: nothing to checkpoint or to reduce.  ``last_agreement`` = dict(weight [n],
    mean_weight, mean_div), logged as ``train/pl_agree_w`` / ``train/pl_agree_div``; device tensors all."""

    FORWARDED = ("lambda_pl", "pseudo_labels", "pseudo_label_source", "pl_threshold", "pl_threshold_momentum", "pl_threshold_warmup",
                 "pl_targets", "pl_temperature", "pl_adaptive", "last_teacher", "pl_agreement",
                 "last_agreement")

    def __init__(self, train_kwargs, ema_decay=None, overlap_metadata=False, overlap_branches=0):
        def option(name, default, ok, must):
            v = train_kwargs.get(name, default)
            if not ok(v):
                raise ValueError(f"train_kwargs['{name}'] must be {must}, not {v!r}")
            return v

        self.lambda_pl = float(option("lambda_pl", 0.0, lambda v: float(v) >= 0.0, ">= 0"))
        self.pseudo_labels = option("pseudo_labels", "own", lambda v: v in ("own", "ensemble"), "'own' or 'ensemble'")
        self.pseudo_label_source = option("pseudo_label_source", "batch", lambda v: v in ("batch", "teacher"), "'batch' or 'teacher'")
        self.pl_threshold = thr = option("pl_threshold", None, lambda v: v is None or (isinstance(v, str) and v in ("median", "adaptive"))
                                         or (isinstance(v, (int, float)) and not isinstance(v, bool) and 0.0 < v <= 1.0),
                                         "None, 'median', 'adaptive' or a number in (0, 1]")
        if isinstance(thr, str) and thr == "adaptive" and self.pseudo_label_source != "teacher":
            raise ValueError("train_kwargs['pl_threshold'] = 'adaptive' needs pseudo_label_source='teacher': the thresholds follow "
                             "the teacher's predictions of every target batch")
        self.pl_threshold_momentum = number(train_kwargs, "pl_threshold_momentum", 0.999, lambda v: 0.0 <= v < 1.0, "a number in [0, 1)")
        self.pl_threshold_warmup = bool(train_kwargs.get("pl_threshold_warmup", False))
        self.pl_targets = option("pl_targets", "hard", lambda v: v in ("hard", "soft"), "'hard' or 'soft'")
        self.pl_temperature = number(train_kwargs, "pl_temperature", 1.0, *POSITIVE)
        if self.pl_targets == "hard" and self.pl_temperature != 1.0:
            raise ValueError(f"train_kwargs['pl_temperature'] = {train_kwargs['pl_temperature']!r} with pl_targets='hard': an arg-max has no temperature "
                             "(it would be silently meaningless); use pl_targets='soft'")
        if self.pl_targets == "soft" and thr == "median":
            raise ValueError("train_kwargs['pl_threshold'] = 'median' is refused with pl_targets='soft': the refinement works on "
                             "labels; give a number in (0, 1] or None")
        self.pl_agreement = number(train_kwargs, "pl_agreement", None, POSITIVE[0], "None or a finite number > 0 (beta of w = exp(-beta * D))")
        # checked whatever lambda_pl is: a schedule that starts at 0 must not hide a configuration that cannot run later
        why = ("ema_decay is None (the teacher is the EMA of the weights)" if ema_decay is None else
               "overlap_metadata is on" if overlap_metadata else f"overlap_branches is {overlap_branches}" if overlap_branches != 0 else None)
        if self.pseudo_label_source == "teacher" and why is not None:
            raise ValueError(f"train_kwargs['pseudo_label_source'] = 'teacher' is refused: {why}; the teacher pass runs on the "
                             "step's one stream (the side-stream modes are experimental and not extended to it)")
        self.pl_adaptive = self.last_teacher = self.last_agreement = None
        self._kept = None  # this step's kept rows: the share [2] of the teacher's labels, or the counts of the two soft loss calls
        self._agree = None  # this step's pselab.agreement_weights (pl_agreement): the teacher pass or losses() fills it

    def _soft(self, l2, l3, thr):
        """Per head the soft targets ("own": the head's own modality, "ensemble": both) and its row of a [2, C] threshold tensor."""
        pairs = [(l2, l3), (l2, l3)] if self.pseudo_labels == "ensemble" else [(l2, None), (l3, None)]
        return [Target(*p, thr[o] if torch.is_tensor(thr) else thr) for o, p in enumerate(pairs)]

    def batch_targets(self, trg):
        """Source "batch": the two heads' :class:`Target` from the target batch's ``pseudo_label_*`` keys (hard) or its
        ``teacher_logit_*`` keys (soft), checked on the host before anything is queued."""
        soft, n = self.pl_targets == "soft", int(trg["x"][0].shape[0])
        if soft:
            keys, want = ("teacher_logit_2d", "teacher_logit_3d"), f"float logits [{n}, C]"
            hint = "give the teacher's logits [n, C] of the target rows, or train with pseudo_label_source='teacher'"
        else:
            keys = ("pseudo_label_ensemble",) * 2 if self.pseudo_labels == "ensemble" else ("pseudo_label_2d", "pseudo_label_3d")
            want, hint = f"labels [{n}]", "build the target dataset with pselab_paths= (the file pselab.export_pseudo_labels writes)"
        for k in keys:
            if k not in trg:
                raise KeyError(f"lambda_pl > 0 with pl_targets={self.pl_targets!r} but the target batch has no '{k}': {hint}")
            v = trg[k]
            if k == "pseudo_label_3d" and isinstance(v, (list, tuple)) and len(v) == 0:
                raise ValueError(f"the pseudo-label file has no 3D entries ('{k}' is empty): train with pseudo_labels=\"ensemble\"")
            if not torch.is_tensor(v) or v.dim() != 1 + soft or int(v.shape[0]) != n or (soft and not v.is_floating_point()):
                raise ValueError(f"'{k}' holds {(tuple(v.shape), v.dtype) if torch.is_tensor(v) else type(v).__name__}, the target "
                                 f"batch has {n} point rows: {want} are expected")
        a, b = trg[keys[0]], trg[keys[1]]
        if a.shape != b.shape:
            raise ValueError(f"'{keys[0]}' is {tuple(a.shape)} and '{keys[1]}' is {tuple(b.shape)}")
        return self._soft(a, b, self.pl_threshold) if soft else [Target(a), Target(b)]

    @torch.no_grad()
    def teacher_targets(self, trainer, batch_2d, batch_3d, first_row=0):
        """Source "teacher": the two heads' :class:`Target` of the target rows, computed by ``trainer``'s teacher before the student's
        forward is queued.  ``batch_2d``: the target images; ``batch_3d``: a dict the 3D net may write to (Net3DSeg.forward replaces
        ``x[1]`` by the gated features) whose point rows ``[first_row:]`` are the target's - in the joined step the [source | target]
        tensors, whose coordinate tensor carries the step's sparse metadata: nothing is built a second time and no host read is added.
        ``pl_threshold="adaptive"``: the pass first takes the batch into ``pl_adaptive`` (built here once the class count is known),
        then labels under the new per-class thresholds (hard targets) or hands each head's loss call its row of them (soft targets)."""
        if trainer.ema is None:
            raise RuntimeError("pseudo_label_source='teacher': the teacher is built with the optimisers (fit_step does it; before a "
                               "bare training_step call configure_optimizers() first)")
        ens, soft, thr = self.pseudo_labels == "ensemble", self.pl_targets == "soft", self.pl_threshold
        adaptive, median = thr == "adaptive", thr == "median"
        with _as_teacher(trainer.model, trainer.ema):
            l2 = trainer(batch_2d, model_name=trainer.modules_name[0])[0]["seg_logit"]
            l3 = trainer(batch_3d, model_name=trainer.modules_name[1])[0]["seg_logit"][first_row:]
            C = int(l2.shape[1])
            if self.pl_agreement is not None:  # the two matrices are at hand here: both heads' loss calls read the one vector
                self._agree = pselab.agreement_weights(l2, l3, self.pl_agreement)
            if adaptive:  # the state takes this batch in, then judges it
                if self.pl_adaptive is None:
                    self.pl_adaptive = pselab.AdaptiveThreshold(C, self.pl_threshold_momentum, self.pl_threshold_warmup, device=l2.device)
                thr = self.pl_adaptive.update(l2, l3, ensemble=ens)
            if soft:
                # no label launch: the loss calls read the logits themselves.  They now outlive the student's forward and
                # backward; both are tensors of their own (lifting's and the linear head's torch.empty outputs, l3 a row
                # slice of one) - neither a workspace nor a static graph buffer (eval forwards are eager): no copy is needed
                targets, seen = self._soft(l2, l3, thr), {"logit_2d": l2, "logit_3d": l3, "kept": None}  # "kept": filled by log()
            else:
                # "median": threshold 0 refuses exactly the rows without a confidence (non-finite logits give NaN, or the
                # ensemble's -1): mm_pselab_refine wants finite probabilities, and passes -100 through without reading them
                out = pselab.teacher_labels(l2, l3, ensemble=ens, threshold=0.0 if median else thr, with_probs=median)
                y2, y3, kept = out["label_2d"], out["label_3d"], out["kept"]
                if median:  # the loaders' refinement over this batch: an exact radix select per output (mm_pselab_refine)
                    y2 = pselab.refine_pseudo_labels(out["prob_2d"], y2, num_classes=C, device=l2.device)
                    y3 = y2 if ens else pselab.refine_pseudo_labels(out["prob_3d"], y3, num_classes=C, device=l2.device)
                    kept = torch.stack([(y2 != -100).sum(), (y3 != -100).sum()])
                targets, seen = [Target(y2), Target(y3)], {"label_2d": y2, "label_3d": y3, "kept": kept}
        self.last_teacher = dict(seen, threshold=thr) if adaptive else seen
        self._kept = None if soft else kept.to(torch.float32) / max(int(l2.shape[0]), 1)
        return targets

    def losses(self, logits_2d, logits_3d, split, targets, gt_head=None, weight_head=None):
        """``(seg2d, seg3d, pl2d, pl3d)``, one pass per head: rows ``[0, split)`` against ``gt_head`` with the class weights, rows
        ``[split, N)`` against the head's target.  ``gt_head=None``: unlabelled head rows; the first two results are to be ignored."""
        rw = None
        if self.pl_agreement is not None:
            if self.pseudo_label_source == "batch":
                if self.pl_targets == "soft":  # the batch's teacher_logit_2d / _3d ("own": one per head; "ensemble": both in each)
                    a, b = targets[0].value, targets[1].value if targets[0].other is None else targets[0].other
                    a, b = a.to(logits_2d.device), b.to(logits_2d.device)
                else:  # file-based labels: the student's own main-head target rows of this step
                    a, b = logits_2d[split:].detach(), logits_3d[split:].detach()
                self._agree = pselab.agreement_weights(a, b, self.pl_agreement)
            rw = self._agree["weight"]

        def pair(logits, t):
            if self.pl_targets == "soft":
                return cross_entropy_soft_pair(logits, split, gt_head, t.value, t.other, weight_head=weight_head,
                                               temperature=self.pl_temperature, threshold=t.threshold, row_weight=rw)
            return (*cross_entropy_pair(logits, split, gt_head, t.value, weight_head=weight_head, row_weight_tail=rw), None)

        (seg2d, pl2d, k2), (seg3d, pl3d, k3) = pair(logits_2d, targets[0]), pair(logits_3d, targets[1])
        if self.pl_targets == "soft":  # the rows the two loss calls kept: counted in their forward launches
            self._kept = (k2, k3)
        return seg2d, seg3d, pl2d, pl3d

    def log(self, logs, stage, pl2d, pl3d, target_rows):
        """Adds ``pl_loss_tgt_*``, ``pl_kept_*`` and ``pl_tau_*`` of ``stage`` to ``logs``; soft targets complete ``last_teacher["kept"]``."""
        logs[f"{stage}/pl_loss_tgt_2d"], logs[f"{stage}/pl_loss_tgt_3d"] = pl2d, pl3d
        teacher, kept = self.pseudo_label_source == "teacher", self._kept
        if self.pl_targets == "soft":
            counts = torch.stack(kept)
            kept = counts.to(torch.float32) / max(int(target_rows), 1)
            if teacher:
                self.last_teacher["kept"] = counts
        if kept is not None:
            logs[f"{stage}/pl_kept_2d"], logs[f"{stage}/pl_kept_3d"] = kept[0], kept[1]
        if self.pl_agreement is not None:
            ag = self._agree
            self.last_agreement = {k: ag[k] for k in ("weight", "mean_weight", "mean_div")}
            logs[f"{stage}/pl_agree_w"], logs[f"{stage}/pl_agree_div"] = ag["mean_weight"], ag["mean_div"]
        if teacher and self.pl_adaptive is not None:  # this step's confidence levels, a copy: the state moves on with the next batch
            tau = self.pl_adaptive.state[:, 0].to(torch.float32)
            logs[f"{stage}/pl_tau_2d"], logs[f"{stage}/pl_tau_3d"] = tau[0], tau[1]

    def state_dict(self):  # the checkpoint's entry: the adaptive thresholds' running state of both outputs, once built
        return {"pl_adaptive": self.pl_adaptive.state_dict()} if self.pl_adaptive is not None else {}

    def load_state_dict(self, ckpt, device=None):
        if not (self.pl_threshold == "adaptive" and self.lambda_pl > 0):
            return
        sd = ckpt.get("pl_adaptive")
        if sd is not None:
            if self.pl_adaptive is None:  # a resume before the first teacher pass: the checkpoint knows the class count
                self.pl_adaptive = pselab.AdaptiveThreshold(sd["num_classes"], self.pl_threshold_momentum, self.pl_threshold_warmup,
                                                            device=device if device is not None else sd["state"].device)
            self.pl_adaptive.load_state_dict(sd)
        elif self.pl_adaptive is not None:
            self.pl_adaptive.reset()  # a checkpoint without the thresholds: they start over
