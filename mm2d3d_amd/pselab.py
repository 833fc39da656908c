"""Pseudo labels: the producer side of the self-training round (csrc/pselab.hip).

The reference's second training round reads ``pselab_paths=`` files (lib/dataset/nuscenes_dataloader.py:96-162,
semantic_kitti.py:143-205): a pickled object array with one dict per scene, ``probs_2d / pseudo_label_2d / probs_3d /
pseudo_label_3d / probs_ensemble / pseudo_label_ensemble``, each ``[n_points]`` - the largest softmax probability (fp32) and
its class (uint8) of the 2D network, of the 3D network and of their average (train.py:297-339).  This module writes them:

    predict(logits_2d, logits_3d)            the six per-point tensors of one batch, one kernel (mm_pselab_predict)
    teacher_labels(logits_2d, logits_3d)     the same per-point expression as int64 training labels of both heads, with an
                                             optional confidence threshold (mm_teacher_labels): what a mean teacher gives the
                                             target batch inside the training step (selftrain.py pseudo_label_source="teacher")
    AdaptiveThreshold(num_classes)           self-adaptive per-class thresholds for those labels (mm_pl_adapt): running state
                                             on the device, ``update`` / ``labels`` per target batch
                                             (selftrain.py pl_threshold="adaptive")
    agreement_weights(logits_2d, logits_3d, beta)  per row exp(-beta * half the Jeffreys divergence of the two softmaxes): the
                                             row weights of the pseudo-label losses (mm_pl_agree; selftrain.py pl_agreement)
    PseudoLabelWriter(path)                  collects scenes, ``close()`` writes the file
    export_pseudo_labels(trainer, dataset, path)   walks a dataset through ``TrainModel.predict_step`` into a writer
    refine_pseudo_labels(probs, labels)      lib/utils/refine_pseudo_labels.py on the GPU (mm_pselab_refine), exact: what the
                                             loaders run three times over every point of a split at construction

``radix_select_medians`` restates the kernel's selection in numpy; only tests use it.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, stream

KEYS = ("probs_2d", "pseudo_label_2d", "probs_3d", "pseudo_label_3d", "probs_ensemble", "pseudo_label_ensemble")
MAX_CLASSES = 32  # csrc/pointpred.h MM_PRED_MAXC


# ---------------------------------------------------------------------------------------------------- prediction
def _logits(t, name, who="predict"):
    """The checked fp32 ``[N, C]`` tensor the kernels read, and its row pitch."""
    _lib.require_cuda(t, name)
    t = t.detach()
    if t.dim() != 2:
        raise ValueError(f"pselab.{who}: {name} must be [N, C]")
    return _lib.row_pitched(t)  # a row-pitched view (stride(1) == 1) is read in place


@torch.no_grad()
def predict(logits_2d, logits_3d=None):
    """Per point the confidence and the class of the 2D logits, the 3D logits and the softmax average, as device tensors under
    the keys of the pseudo-label file (fp32 probabilities, uint8 labels).  ``logits_3d=None``: a 2D-only prediction, the
    3D and ensemble entries are ``None``."""
    a, ld_a = _logits(logits_2d, "logits_2d")
    b, ld_b = (None, 0) if logits_3d is None else _logits(logits_3d, "logits_3d")
    if b is not None and (b.shape != a.shape or b.device != a.device):
        raise ValueError("pselab.predict: logits_2d and logits_3d must have the same shape and device")
    N, C = a.shape
    n_out = 1 if b is None else 3
    probs = torch.empty((n_out, N), dtype=torch.float32, device=a.device)
    labels = torch.empty((n_out, N), dtype=torch.uint8, device=a.device)
    with torch.cuda.device(a.device):
        check(_lib.lib().mm_pselab_predict(ptr(a), ld_a, ptr(b), ld_b, N, C, ptr(probs[0]), ptr(labels[0]),
                                           ptr(probs[1]) if b is not None else None, ptr(labels[1]) if b is not None else None,
                                           ptr(probs[2]) if b is not None else None, ptr(labels[2]) if b is not None else None,
                                           stream()), "pselab_predict")
    out = dict.fromkeys(KEYS)
    out["probs_2d"], out["pseudo_label_2d"] = probs[0], labels[0]
    if b is not None:
        out["probs_3d"], out["pseudo_label_3d"] = probs[1], labels[1]
        out["probs_ensemble"], out["pseudo_label_ensemble"] = probs[2], labels[2]
    return out


@torch.no_grad()
def teacher_labels(logits_2d, logits_3d, ensemble=False, threshold=None, ignore_label=-100, with_probs=False):
    """The int64 training labels a teacher's logits give both heads, in one launch (mm_teacher_labels): per row the expression
    of :func:`predict`, so ``label_2d`` / ``label_3d`` are ``pseudo_label_2d`` / ``pseudo_label_3d`` of an export, or with
    ``ensemble`` both ``pseudo_label_ensemble``.  ``threshold``: a label whose confidence is not ``>= threshold`` (float32)
    becomes ``ignore_label``; ``None`` keeps all; a float32 ``[2, C]`` device tensor (row 0: 2D, row 1: 3D; read on the device) judges
    a row by the threshold of its own class (mm_teacher_labels_cls, :class:`AdaptiveThreshold`).  Returns ``dict(label_2d, label_3d,
    kept)``, ``kept`` an int64 ``[2]`` device tensor with the labels kept per output; ``with_probs`` adds ``prob_2d`` / ``prob_3d``,
    the confidences the labels were judged by.  Row-pitched views are read in place."""
    cls = torch.is_tensor(threshold)
    if cls:  # checked from the arguments as they come, before anything else looks at them
        if (threshold.dtype, tuple(threshold.shape), threshold.device) != (torch.float32, (2, logits_2d.shape[-1]), logits_2d.device):
            raise ValueError(f"pselab.teacher_labels: a threshold tensor must be float32 [2, {logits_2d.shape[-1]}] on "
                             f"{logits_2d.device}, not {threshold.dtype} {tuple(threshold.shape)} on {threshold.device}")
        threshold = threshold.detach().contiguous()
    (a, ld_a), (b, ld_b) = _logits(logits_2d, "logits_2d", "teacher_labels"), _logits(logits_3d, "logits_3d", "teacher_labels")
    if b.shape != a.shape or b.device != a.device:
        raise ValueError("pselab.teacher_labels: logits_2d and logits_3d must have the same shape and device")
    N, C = a.shape
    labels = torch.empty((2, N), dtype=torch.int64, device=a.device)
    probs = torch.empty((2, N), dtype=torch.float32, device=a.device) if with_probs else None
    kept = torch.zeros(2, dtype=torch.int64, device=a.device) if N == 0 else torch.empty(2, dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        fn = _lib.lib().mm_teacher_labels_cls if cls else _lib.lib().mm_teacher_labels
        check(fn(ptr(a), ld_a, ptr(b), ld_b, N, C, int(bool(ensemble)),
                 ptr(threshold) if cls else -1.0 if threshold is None else float(threshold), int(ignore_label), ptr(labels[0]),
                 ptr(labels[1]), ptr(probs[0]) if with_probs else None, ptr(probs[1]) if with_probs else None, ptr(kept), stream()),
              "teacher_labels_cls" if cls else "teacher_labels")
    out = {"label_2d": labels[0], "label_3d": labels[1], "kept": kept}
    return dict(out, prob_2d=probs[0], prob_3d=probs[1]) if with_probs else out


def agreement_beta(beta, who="pselab.agreement_weights"):
    """``beta`` as a float, or ``ValueError``: a finite number > 0 (a bool is not a number here)."""
    if isinstance(beta, bool) or not isinstance(beta, (int, float)) or not 0.0 < float(beta) < float("inf"):
        raise ValueError(f"{who}: beta must be a finite number > 0, not {beta!r}")
    return float(beta)


@torch.no_grad()
def agreement_weights(logits_2d, logits_3d, beta):
    """Row weights from the agreement of the two modalities (mm_pl_agree; the definition is in include/mm2d3d.h): per row
    ``D`` = half the Jeffreys divergence of ``softmax(logits_2d)`` and ``softmax(logits_3d)`` and ``w = exp(-beta * D)``, 1 where
    the two predictions agree and towards 0 where they contradict each other; a row with a non-finite logit gets 0.  Returns
    ``dict(weight, mean_weight, mean_div, finite)``: float32 ``[N]``, the mean of ``w`` over all rows, the mean of ``D`` over the
    finite rows (float32 scalars) and their number (int64 scalar) - device tensors all, no host read; detached.  Row-pitched views
    (``stride(1) == 1``) are read in place.  Two launches, bit-stable run to run."""
    who = "agreement_weights"
    beta = agreement_beta(beta)
    (a, ld_a), (b, ld_b) = _logits(logits_2d, "logits_2d", who), _logits(logits_3d, "logits_3d", who)
    if b.shape != a.shape or b.device != a.device:
        raise ValueError(f"pselab.{who}: logits_2d and logits_3d must have the same shape and device")
    N, C = a.shape
    if not 2 <= C <= MAX_CLASSES:
        raise ValueError(f"pselab.{who}: {C} classes, the row kernels take 2 to {MAX_CLASSES}")
    w = torch.empty(N, dtype=torch.float32, device=a.device)
    stats = torch.empty(2, dtype=torch.float32, device=a.device)
    finite = torch.empty((), dtype=torch.int64, device=a.device)
    L = _lib.lib()
    with torch.cuda.device(a.device):
        ws = _lib.workspace.get(int(L.mm_pl_agree_ws_bytes()), a.device, "pselab")
        check(L.mm_pl_agree(ptr(a), ld_a, ptr(b), ld_b, N, C, beta, ptr(w), ptr(stats), ptr(finite), ptr(ws), ws.numel(), stream()),
              "pl_agree")
    return {"weight": w, "mean_weight": stats[0], "mean_div": stats[1], "finite": finite}


# ---------------------------------------------------------------------------------------------------- adaptive thresholds
class AdaptiveThreshold:
    """Self-adaptive per-class thresholds for a mean teacher's pseudo labels (FreeMatch, Wang et al., ICLR 2023; the definition
    the kernels follow is in include/mm2d3d.h at mm_pl_adapt).  Per output (0: 2D, 1: 3D) a running confidence level ``tau`` and a
    running class mass ``pt[c]``, both an exponential moving average over the target batches, give
    ``thr[c] = (pt[c] / max(pt)) * tau``: classes the teacher rarely predicts get a lower bar, and the bar moves with the
    teacher's confidence.  A row is kept iff its confidence is ``>= thr[its class]`` (float32, the project's ``>=``).

    ``state``: fp64 ``[2, 1 + C]`` = (tau, pt) per output, all ``1 / C`` at the start; ``count``: int64 ``[2]``, the updates
    taken.  Both live on the device and are updated there (two launches, no atomics, no host read: bit-stable run to run).  Rows
    whose confidence is not ``>= 0`` (non-finite logits) are not counted; a batch without counted rows leaves an output's state
    and count alone.  ``warmup``: momentum_t = min(momentum, (1 + t) / (10 + t)) over the updates t taken so far, the form of
    ``ema_warmup``.  With momentum 0.999 and no warm-up the thresholds start near ``1 / C``, which no confidence is below: every
    row is kept until the state has moved.

    Every ``update`` / ``labels`` call counts: the trainer's update is not gated by the loss-scale skip or by the data-parallel
    reducer's flag (the teacher's predictions are valid whether or not the student's step is taken).  Under data parallelism every
    rank keeps its own state from its own target batches; it is not reduced (a known gap)."""

    def __init__(self, num_classes, momentum=0.999, warmup=False, device="cuda"):
        C = int(num_classes)
        if not 1 <= C <= MAX_CLASSES:
            raise ValueError(f"pselab.AdaptiveThreshold: {num_classes!r} classes, the row kernels take 1 to {MAX_CLASSES}")
        if isinstance(momentum, bool) or not isinstance(momentum, (int, float)) or not 0.0 <= momentum < 1.0:
            raise ValueError(f"pselab.AdaptiveThreshold: momentum must be a number in [0, 1), not {momentum!r}")
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("pselab.AdaptiveThreshold keeps its state on a GPU")
        self.num_classes, self.momentum, self.warmup = C, float(momentum), bool(warmup)
        self.state = torch.empty((2, 1 + C), dtype=torch.float64, device=dev)
        self.count = torch.empty(2, dtype=torch.int64, device=dev)
        self.reset()

    def reset(self):
        """Back to the initial state: tau = pt[c] = 1 / C, no update taken."""
        self.state.fill_(1.0 / self.num_classes)
        self.count.zero_()

    def state_dict(self):
        return {"num_classes": self.num_classes, "state": self.state.clone(), "count": self.count.clone()}

    def load_state_dict(self, sd):
        if int(sd["num_classes"]) != self.num_classes or tuple(sd["state"].shape) != tuple(self.state.shape):
            raise ValueError(f"pselab.AdaptiveThreshold: the state is of {int(sd['num_classes'])} classes, this object has {self.num_classes}")
        self.state.copy_(sd["state"].to(torch.float64))
        self.count.copy_(sd["count"].to(torch.int64))

    def _update(self, logits_2d, logits_3d, ensemble, who):
        (a, ld_a), (b, ld_b) = _logits(logits_2d, "logits_2d", who), _logits(logits_3d, "logits_3d", who)
        if b.shape != a.shape or b.device != a.device:
            raise ValueError(f"pselab.{who}: logits_2d and logits_3d must have the same shape and device")
        if a.shape[1] != self.num_classes or a.device != self.state.device:
            raise ValueError(f"pselab.{who}: logits [N, {a.shape[1]}] on {a.device}, the state is of {self.num_classes} classes on "
                             f"{self.state.device}")
        N, C = a.shape
        thr = torch.empty((2, C), dtype=torch.float32, device=a.device)
        L = _lib.lib()
        with torch.cuda.device(a.device):
            ws = _lib.workspace.get(int(L.mm_pl_adapt_ws_bytes()), a.device, "pselab")
            check(L.mm_pl_adapt(ptr(a), ld_a, ptr(b), ld_b, N, C, int(bool(ensemble)), self.momentum, int(self.warmup),
                                ptr(self.state), ptr(self.count), ptr(thr), ptr(ws), ws.numel(), stream()), "pl_adapt")
        return a, b, thr

    @torch.no_grad()
    def update(self, logits_2d, logits_3d, ensemble=False):
        """Takes the batch into the state and returns this step's thresholds, a fresh float32 ``[2, C]`` device tensor (row 0 the
        2D output's, row 1 the 3D output's): updated first, then to be applied to the same batch.  ``ensemble``: both outputs
        follow the softmax average.  Row-pitched views are read in place."""
        return self._update(logits_2d, logits_3d, ensemble, "AdaptiveThreshold.update")[2]

    @torch.no_grad()
    def labels(self, logits_2d, logits_3d, ensemble=False, ignore_label=-100, with_probs=False):
        """:meth:`update`, then the labels of :func:`teacher_labels` under the new thresholds (mm_teacher_labels_cls): its dict
        plus ``"threshold"``, the ``[2, C]`` tensor the rows were judged by."""
        a, b, thr = self._update(logits_2d, logits_3d, ensemble, "AdaptiveThreshold.labels")
        return dict(teacher_labels(a, b, ensemble, thr, ignore_label, with_probs), threshold=thr)


# ---------------------------------------------------------------------------------------------------- refinement
def refine_pseudo_labels(probs, labels, ignore_label=-100, num_classes=None, device="cuda"):
    """``datasets.refine_pseudo_labels`` on the GPU: the same labels, exactly.  ``probs`` / ``labels``: numpy arrays or tensors
    ``[N]``; they are uploaded (if they are not on ``device`` already), refined by mm_pselab_refine and returned in the input's
    kind, dtype and shape.  ``num_classes``: classes are ``[0, num_classes)`` (default: largest label + 1); labels outside
    (``-100`` from an earlier refinement, say) pass through.  float32 probabilities only - the selection works on their bit
    patterns; every other dtype raises ``TypeError``: use ``mm2d3d_amd.datasets.refine_pseudo_labels`` for those."""
    as_numpy = not torch.is_tensor(labels)
    p = probs if torch.is_tensor(probs) else torch.from_numpy(np.ascontiguousarray(probs))
    y = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    if p.dtype != torch.float32:
        raise TypeError(f"pselab.refine_pseudo_labels takes float32 probabilities, not {p.dtype}: the host function "
                        "mm2d3d_amd.datasets.refine_pseudo_labels handles other dtypes")
    if y.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8):
        raise TypeError(f"pselab.refine_pseudo_labels takes signed integer labels (ignore_label must fit), not {y.dtype}")
    if p.shape != y.shape:
        raise ValueError("pselab.refine_pseudo_labels: probs and labels must have the same shape")
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("pselab.refine_pseudo_labels runs on a GPU; the host function is mm2d3d_amd.datasets.refine_pseudo_labels")
    if num_classes is None:
        num_classes = int(y.max()) + 1 if y.numel() else 0
    out_dev = y.device
    if y.numel() == 0 or num_classes <= 0:
        res = y.clone()
    else:
        pd = p.reshape(-1).to(dev).contiguous()
        yd = y.reshape(-1).to(dev, torch.int64).contiguous()
        od = torch.empty_like(yd)
        L = _lib.lib()
        with torch.cuda.device(pd.device):
            ws = _lib.workspace.get(int(L.mm_pselab_refine_ws_bytes(int(num_classes))), pd.device, "pselab")
            check(L.mm_pselab_refine(ptr(pd), ptr(yd), yd.numel(), int(num_classes), int(ignore_label), ptr(od), ptr(ws), ws.numel(),
                                     stream()), "pselab_refine")
        res = od.to(out_dev).to(y.dtype).reshape(y.shape)
    return res.numpy() if as_numpy else res


def float_keys(p):
    """The order-preserving uint32 image of float32 values (csrc/pselab.hip f2key)."""
    u = np.ascontiguousarray(p, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def radix_select_medians(probs, labels, num_classes):
    """Numpy restatement of the kernel chain's selection (tests only): per class of ``[0, num_classes)`` the element of rank
    ``(n - 1) // 2`` among its probabilities, by four most-significant-digit passes of 256-bucket counts.  Returns
    ``(medians float32 [num_classes], present bool [num_classes])``."""
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    labels = np.asarray(labels)
    keys = float_keys(probs)
    med, present = np.zeros(num_classes, np.float32), np.zeros(num_classes, bool)
    for c in range(num_classes):
        k = keys[labels == c]
        if not len(k):
            continue
        present[c] = True
        rank, prefix = (len(k) - 1) // 2, 0
        for p in range(4):
            shift = 24 - 8 * p
            if p:
                k = k[(k >> np.uint32(shift + 8)) == prefix]
            counts = np.bincount((k >> np.uint32(shift)) & np.uint32(255), minlength=256)
            incl = np.cumsum(counts)
            b = int(np.searchsorted(incl, rank, side="right"))  # first bucket with incl > rank
            rank -= int(incl[b] - counts[b])
            prefix = (prefix << 8) | b
        key = np.uint32(prefix)
        bits = key & np.uint32(0x7FFFFFFF) if key & np.uint32(0x80000000) else ~key
        med[c] = np.array([bits], dtype=np.uint32).view(np.float32)[0]
    return med, present


def refine_with_medians(probs, labels, medians, present, ignore_label=-100):
    """The threshold rule of the refinement on given medians: ``thr = min(median, float32(0.9))``, compared in float32."""
    probs = np.ascontiguousarray(probs, dtype=np.float32)
    out = np.array(labels, copy=True)
    for c in np.nonzero(present)[0]:
        thr = np.minimum(np.float32(medians[c]), np.float32(0.9))
        out[(out == c) & (probs < thr)] = ignore_label
    return out


# ---------------------------------------------------------------------------------------------------- the file
class PseudoLabelWriter:
    """Collects per-scene pseudo labels and writes the file the loaders' ``pselab_paths=`` reads: ``close()`` saves
    ``np.array(list_of_dicts, dtype=object)`` with the six ``KEYS`` per scene, float32 probabilities and uint8 labels.
    ``with_3d=False``: the two 3D entries are ``None`` (a 2D-only round; the loaders accept it)."""

    def __init__(self, path, with_3d=True):
        self.path, self.with_3d, self.scenes, self.closed = path, with_3d, [], False

    @staticmethod
    def _host(x, dtype, n=None, what=""):
        if torch.is_tensor(x):
            x = x.detach().cpu().numpy()
        x = np.array(x, dtype=dtype, copy=True).reshape(-1)  # a copy: callers reuse their staging buffers
        if n is not None and len(x) != n:
            raise ValueError(f"PseudoLabelWriter: {what} has {len(x)} entries, probs_2d has {n}")
        return x

    def add_scene(self, probs_2d, label_2d, probs_3d, label_3d, probs_ensemble, label_ensemble):
        if self.closed:
            raise RuntimeError("PseudoLabelWriter: already closed")
        if probs_ensemble is None or label_ensemble is None:
            raise ValueError("PseudoLabelWriter: the ensemble entries are required (the loaders refine them unconditionally)")
        if self.with_3d and (probs_3d is None or label_3d is None):
            raise ValueError("PseudoLabelWriter: with_3d=True needs probs_3d and label_3d")
        d = {"probs_2d": self._host(probs_2d, np.float32)}
        n = len(d["probs_2d"])
        d["pseudo_label_2d"] = self._host(label_2d, np.uint8, n, "label_2d")
        d["probs_3d"] = self._host(probs_3d, np.float32, n, "probs_3d") if self.with_3d else None
        d["pseudo_label_3d"] = self._host(label_3d, np.uint8, n, "label_3d") if self.with_3d else None
        d["probs_ensemble"] = self._host(probs_ensemble, np.float32, n, "probs_ensemble")
        d["pseudo_label_ensemble"] = self._host(label_ensemble, np.uint8, n, "label_ensemble")
        self.scenes.append(d)

    def close(self):
        if self.closed:
            return self.path
        arr = np.empty(len(self.scenes), dtype=object)  # = np.array(self.scenes, dtype=object), 1-D also for an empty list
        for i, d in enumerate(self.scenes):
            arr[i] = d
        with open(self.path, "wb") as f:  # np.save appends ".npy" to a name; a file object keeps the caller's path
            np.save(f, arr, allow_pickle=True)
        self.closed = True
        return self.path


class _HostCopy:
    """One batch's outputs on their way to the host: asynchronous copies into pinned buffers on the current stream, then an
    event (the pattern of scn/metadata._Readback); ``wait()`` blocks only if the GPU has not got there yet.  The pinned
    buffers belong to a slot of the exporter and are reused by the batch after next."""

    def __init__(self, slot, tensors):
        self.views, self._keep = {}, tensors
        dev = next(t.device for t in tensors.values() if t is not None)
        for k, t in tensors.items():
            if t is None:
                self.views[k] = None
                continue
            buf = slot.get(k)
            if buf is None or buf.numel() < t.numel() or buf.dtype != t.dtype:
                buf = slot[k] = torch.empty(max(int(t.numel() * 1.25), 1024), dtype=t.dtype).pin_memory()
            buf[: t.numel()].copy_(t.reshape(-1), non_blocking=True)
            self.views[k] = buf[: t.numel()].numpy()
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(dev))

    def wait(self):
        self.event.synchronize()
        self._keep = None
        return self.views


def export_pseudo_labels(trainer, dataset, path, batch_size=8, device="cuda", **gpu_batch_kwargs):
    """Pseudo labels of every scene of ``dataset`` under ``trainer``'s current weights, written to ``path`` in the format
    ``pselab_paths=`` reads.  Scenes are walked in index order, ``batch_size`` at a time (the last batch may be short):
    ``dataset.gpu_batch`` -> ``trainer.predict_step`` -> per-scene slices -> pinned host buffers (one batch's copies in flight while
    the next batch is computed) -> :class:`PseudoLabelWriter`.

    The file's rows must line up with the scenes' points as the loader will see them, so the dataset must be built with
    ``output_orig=True`` and without augmentation that drops points; a scene of which a point fell outside the voxel range,
    or whose exported length differs from the length the loader checks (a cropping or down-sampling configuration), raises
    ``ValueError`` naming the scene, and no file is written.  ``predict_step`` leaves the trainer's model in eval mode and nothing
    here undoes that: call ``trainer.model.train()`` before training goes on.  Returns ``dict(path, scenes, points, num_classes, hist_2d,
    hist_3d, hist_ensemble)`` with the per-class label counts."""
    name = type(dataset).__name__
    if not getattr(dataset, "has_pselab", False):
        raise ValueError(f"export_pseudo_labels: {name} is a source-only dataset (has_pselab = False): its loader reads no pseudo labels "
                         "(refused before scene 0)")
    if not getattr(dataset, "output_orig", False):
        raise ValueError(f"export_pseudo_labels: this {name} was not built with output_orig=True, so the per-scene range masks cannot be "
                         "checked (refused before scene 0)")
    length_key = getattr(dataset, "pselab_length_key", None)
    if length_key is None:
        raise ValueError(f"export_pseudo_labels: {name} does not say which per-scene array its pseudo labels line up with "
                         "(refused before scene 0)")
    writer = PseudoLabelWriter(path, with_3d=True)
    hist = np.zeros((3, 256), dtype=np.int64)
    slots, pending, points = [{}, {}], None, 0

    def drain(job):
        nonlocal points
        copy, counts = job
        host = copy.wait()
        left = 0
        for n in counts:
            cut = [host[k][left : left + n] for k in KEYS]
            writer.add_scene(*cut)
            for j, k in enumerate(("pseudo_label_2d", "pseudo_label_3d", "pseudo_label_ensemble")):
                hist[j] += np.bincount(host[k][left : left + n], minlength=256)
            left += n
            points += n

    n_scenes = len(dataset)
    for k, start in enumerate(range(0, n_scenes, batch_size)):
        indices = list(range(start, min(start + batch_size, n_scenes)))
        batch = dataset.gpu_batch(indices, device=device, **gpu_batch_kwargs)
        counts = [int(t.shape[0]) for t in batch["img_indices"]]
        for b, i in enumerate(indices):
            mask = np.asarray(batch["orig_points_idx"][b])
            if not mask.all():
                raise ValueError(f"export_pseudo_labels: scene {i}: {int((~mask).sum())} of {len(mask)} points fall outside the voxel range "
                                 f"(full_scale={dataset.full_scale}): the file's rows would not line up with the scene's points")
            want = len(dataset.data[i][length_key])
            if counts[b] != want:
                raise ValueError(f"export_pseudo_labels: scene {i}: {counts[b]} points reach the networks but the loader checks "
                                 f"len(data[{i}][{length_key!r}]) = {want}: export without cropping or down-sampling")
        out = trainer.predict_step(batch)
        if out["probs_3d"] is None:
            raise ValueError("export_pseudo_labels: predict_step returned no 3D prediction")
        if sum(counts) != out["probs_2d"].shape[0]:
            raise ValueError(f"export_pseudo_labels: scene {indices[0]}: the batch has {sum(counts)} points, the prediction {out['probs_2d'].shape[0]}")
        job = (_HostCopy(slots[k % 2], {key: out[key] for key in KEYS}), counts)
        if pending is not None:
            drain(pending)  # the previous batch, while this one's kernels and copies run
        pending = job
    if pending is not None:
        drain(pending)
    writer.close()
    used = np.nonzero(hist.sum(0))[0]
    C = max(int(getattr(trainer, "num_classes", None) or 0), int(used[-1]) + 1 if len(used) else 0)
    return dict(path=os.fspath(path), scenes=n_scenes, points=points, num_classes=C, hist_2d=hist[0, :C].copy(), hist_3d=hist[1, :C].copy(),
                hist_ensemble=hist[2, :C].copy())
