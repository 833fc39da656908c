"""Loss registry with the reference's API (lib/losses.py:81-153) over fused HIP row kernels (csrc/loss.hip).

``Loss(cfg)``; ``loss("segmentation", pred=, gt=)``; ``split_by_target()``; ``update_loss_params()`` behave as
in the reference; ``cross_entropy`` (weighted, ignore_index -100, weighted-mean reduction = torch's
``F.cross_entropy`` default) and the cross-modal KL of train.py:157-184 run as single fused kernels; ``lovasz_softmax`` sorts its
errors per class with the segmented radix sort of csrc/lovasz.hip; ``target_entropy`` (entropy minimisation and its diversity guard on
unlabelled rows) runs on the row kernels of csrc/infomax.hip; ``coral`` (Deep CORAL / LogCORAL alignment of the source and the target
rows' covariances) on those of csrc/coral.hip; ``adversarial`` (a point discriminator on the softmax or self-information of the
source and the target rows, AdaptSegNet / AdvEnt) on those of csrc/adv.hip; ``cross_modal_dense`` (the cross-modal KL pair against
the best pixel of a window round each point's own, the sparse-to-dense matching of DsCML) on the window search of csrc/xmdense.hip;
``cross_entropy_pair`` / ``cross_entropy_soft_pair`` take a weight per
tail row (``pselab.agreement_weights``) through a compile-time flag of the same kernels.
"""
from __future__ import annotations

from copy import deepcopy

import torch

from . import _lib
from ._lib import check, ptr, stream

F32 = torch.float32


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index):
        _lib.require_cuda(logits, "pred")
        L = _lib.lib()
        logits = logits.to(F32).contiguous()
        labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
        N, C = logits.shape
        stats = torch.empty(2, dtype=F32, device=logits.device)
        ws = _lib.workspace.get(int(L.mm_loss_ws_bytes()), logits.device)
        check(L.mm_ce_fwd(ptr(logits), C, ptr(labels), ptr(weight), N, C, ignore_index, ptr(stats), ptr(ws), ws.numel(),
                          stream()), "ce_fwd")
        ctx.save_for_backward(logits, labels, weight, stats)
        ctx.ignore_index = ignore_index
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        logits, labels, weight, stats = ctx.saved_tensors
        N, C = logits.shape
        d = torch.empty_like(logits)
        g = g.to(F32).contiguous()
        check(L.mm_ce_bwd(ptr(logits), C, ptr(labels), ptr(weight), N, C, ctx.ignore_index, ptr(stats), ptr(g), ptr(d), C,
                          stream()), "ce_bwd")
        return d, None, None, None


_UPLOADED = {"weight": {}, "prior": {}}  # kind -> {(values, device): device tensor}


def _uploaded(kind, values, device, upload):
    """A host sequence of numbers on ``device``, uploaded ONCE per device.  torch.tensor(list, device=cuda) is a pageable
    host-to-device copy - the host waits until the stream has reached it, i.e. for the whole forward pass queued before the loss:
    3.3 ms per call in the host profile of round 5, twice per step."""
    cache, key = _UPLOADED[kind], (values, device)
    hit = cache.get(key)
    if hit is None:
        if len(cache) > 64:
            cache.clear()
        hit = cache[key] = upload()
    return hit


def _device_weight(weight, device):
    if isinstance(weight, (list, tuple)):  # the class weights of a config come as a Python list (config.yaml:45)
        weight = _uploaded("weight", tuple(float(v) for v in weight), device, lambda: torch.tensor(weight, dtype=F32, device=device))
    elif weight is not None:
        weight = weight.to(device=device, dtype=F32).contiguous()
    return weight


def cross_entropy(pred, gt, weight=None, ignore_index=-100):
    return _CrossEntropyFn.apply(pred, gt, _device_weight(weight, pred.device), ignore_index)


def _grad_rows(logits, in_dtype, launch):
    """The gradient of a row loss: ``launch(d)`` has a backward kernel write the fp32 [N, C] buffer ``d`` (row pitch C), which goes
    back in the dtype the logits came in."""
    d = torch.empty(tuple(logits.shape), dtype=F32, device=logits.device)
    launch(d)
    return d if in_dtype == F32 else d.to(in_dtype)


def _labels(gt, n, device, ignore_index, who, which):
    """int64 labels of a segment of ``n`` rows on ``device``; ``None`` = unlabelled."""
    if gt is None:
        return None
    gt = gt.to(device=device, dtype=torch.int64).contiguous()
    if gt.dim() != 1 or gt.shape[0] != n:
        raise ValueError(f"{who}: {which} has shape {tuple(gt.shape)}, its segment has {n} rows")
    # an empty tensor has no address, and no address means "unlabelled" to the library: a labelled segment without rows
    # (0/0 unless zero_if_empty) passes one label that no row reads
    return gt if n else gt.new_full((1,), ignore_index)


def _class_weights(w, C, device, who, which):
    w = _device_weight(w, device)
    if w is not None and w.numel() != C:
        raise ValueError(f"{who}: {which} has {w.numel()} entries for {C} classes")
    return w


class _CrossEntropyPairFn(torch.autograd.Function):
    """Rows [0, split) of ``logits`` against (labels0, weight0), rows [split, N) against (labels1, weight1): one forward call,
    and ONE backward launch that writes the whole gradient from both upstream gradients (csrc/loss.hip k_ce_*<2>).  ``row_w``
    (float32 [N - split], a constant of the gradient, or None): the tail's row weights, through mm_ce2_*_w."""

    @staticmethod
    def forward(ctx, logits, split, labels0, weight0, labels1, weight1, ignore_index, zero_bits, row_w=None):
        _lib.require_cuda(logits, "pred")
        L = _lib.lib()
        ctx.in_dtype = logits.dtype
        logits, ld = _lib.row_pitched(logits)
        N, C = logits.shape
        stats = torch.empty(4, dtype=F32, device=logits.device)
        ws = _lib.workspace.get(int(L.mm_ce2_ws_bytes()), logits.device)
        if row_w is None:
            check(L.mm_ce2_fwd(ptr(logits), ld, N, split, C, ptr(labels0), ptr(weight0), ptr(labels1), ptr(weight1), ignore_index,
                               zero_bits, ptr(stats), ptr(ws), ws.numel(), stream()), "ce2_fwd")
        else:
            check(L.mm_ce2_fwd_w(ptr(logits), ld, N, split, C, ptr(labels0), ptr(weight0), ptr(labels1), ptr(weight1), ignore_index,
                                 zero_bits, ptr(row_w), ptr(stats), ptr(ws), ws.numel(), stream()), "ce2_fwd_w")
        ctx.save_for_backward(logits, labels0, weight0, labels1, weight1, stats, row_w)
        ctx.args = (ld, split, ignore_index)
        return stats[0], stats[2]

    @staticmethod
    def backward(ctx, g0, g1):
        L = _lib.lib()
        logits, labels0, weight0, labels1, weight1, stats, row_w = ctx.saved_tensors
        ld, split, ignore_index = ctx.args
        N, C = logits.shape
        g = torch.stack((g0, g1)).to(F32)  # the two upstream scalars side by side: the kernel's grad_out[2]
        if row_w is None:
            launch = lambda d: check(
                L.mm_ce2_bwd(ptr(logits), ld, N, split, C, ptr(labels0), ptr(weight0), ptr(labels1), ptr(weight1), ignore_index,
                             ptr(stats), ptr(g), ptr(d), C, stream()), "ce2_bwd")
        else:
            launch = lambda d: check(
                L.mm_ce2_bwd_w(ptr(logits), ld, N, split, C, ptr(labels0), ptr(weight0), ptr(labels1), ptr(weight1), ignore_index,
                               ptr(row_w), ptr(stats), ptr(g), ptr(d), C, stream()), "ce2_bwd_w")
        return _grad_rows(logits, ctx.in_dtype, launch), None, None, None, None, None, None, None, None


def _row_weight(w, n, device, who, which):
    """The checked row weights of a segment of ``n`` rows: a float32 ``[n]`` tensor on ``device`` that does not require grad (the
    weights are constants of the gradient), contiguous; ``None`` stays ``None``."""
    if w is None:
        return None
    if not torch.is_tensor(w) or w.dtype != F32 or tuple(w.shape) != (n,):
        got = f"{w.dtype} {tuple(w.shape)}" if torch.is_tensor(w) else type(w).__name__
        raise ValueError(f"{who}: {which} must be a float32 tensor [{n}] (one weight per tail row), not {got}")
    if w.requires_grad:
        raise ValueError(f"{who}: {which} requires grad, but the row weights are not differentiated: detach it")
    if w.device != device:
        raise ValueError(f"{who}: {which} lives on {w.device}, pred on {device}")
    return w.contiguous()


def cross_entropy_pair(pred, split, gt_head=None, gt_tail=None, weight_head=None, weight_tail=None, ignore_index=-100,
                       zero_if_empty=(False, True), row_weight_tail=None):
    """``(loss_head, loss_tail)``: the cross entropy of rows ``[0, split)`` of ``pred`` [N, C] against ``gt_head`` and of rows
    ``[split, N)`` against ``gt_tail`` - each ``cross_entropy``'s weighted mean over its own counted rows - from one pass over
    ``pred`` per direction (the joined [source | target] step: supervised loss on the source rows, pseudo-label loss on the target
    rows, ``train_kwargs["lambda_pl"]``).  ``pred`` may be a row-pitched view (``stride(1) == 1``).

    ``gt_* = None``: that segment is unlabelled - loss 0, zero gradient rows.  ``split`` may be 0 or N.  Labels outside
    ``[0, C)`` are skipped like ``ignore_index``.

    ``zero_if_empty[s]``: a segment in which nothing is counted (every label ignored, or no rows) gives loss ``0.0`` and a zero
    gradient.  This DEVIATES from ``F.cross_entropy`` (and from ``cross_entropy``), which return nan = 0/0: a target batch whose
    pseudo labels were all refined away must not poison the step, so the tail's default is True; the head keeps torch's nan.

    ``row_weight_tail`` (float32 device tensor ``[N - split]``, e.g. ``pselab.agreement_weights``; not differentiated, a tensor
    that requires grad is refused): ``loss_tail`` = ``sum_i row_w_i * w[y_i] * ce_i / sum_i w[y_i]`` over the counted tail rows -
    the weights scale the rows' terms and gradient rows and are NOT in the denominator, so an uncertain batch pulls less.  A row
    of weight 0 is still counted.  ``None``: the call is launch for launch the call without the option."""
    if pred.dim() != 2:
        raise ValueError("cross_entropy_pair: pred must be [N, C]")
    N, split = int(pred.shape[0]), int(split)
    if not 0 <= split <= N:
        raise ValueError(f"cross_entropy_pair: split {split} outside [0, {N}]")
    who, dev, C = "cross_entropy_pair", pred.device, int(pred.shape[1])
    row_weight_tail = _row_weight(row_weight_tail, N - split, dev, who, "row_weight_tail")
    gt_head = _labels(gt_head, split, dev, ignore_index, who, "gt_head")
    gt_tail = _labels(gt_tail, N - split, dev, ignore_index, who, "gt_tail")
    weight_head = _class_weights(weight_head, C, dev, who, "weight_head")
    weight_tail = _class_weights(weight_tail, C, dev, who, "weight_tail")
    bits = (1 if zero_if_empty[0] else 0) | (2 if zero_if_empty[1] else 0)
    return _CrossEntropyPairFn.apply(pred, split, gt_head, weight_head, gt_tail, weight_tail, int(ignore_index), bits, row_weight_tail)


class _CrossEntropySoftPairFn(torch.autograd.Function):
    """Rows [0, split) of ``logits`` against (labels0, weight0), rows [split, N) against the softened distribution of the teacher
    logits: one forward call, and ONE backward launch that writes the whole gradient, recomputing the teacher's distribution
    (csrc/loss.hip k_ce2s_*).  ``row_w`` (float32 [N - split], a constant of the gradient, or None): the tail's row weights, through
    mm_ce2s_*_w."""

    @staticmethod
    def forward(ctx, logits, split, labels0, weight0, ta, tb, temperature, thr, ignore_index, row_w=None):
        _lib.require_cuda(logits, "pred")
        L = _lib.lib()
        ctx.in_dtype = logits.dtype
        logits, ld = _lib.row_pitched(logits)
        ta, ld_a = _lib.row_pitched(ta)
        tb, ld_b = _lib.row_pitched(tb) if tb is not None else (None, 0)
        N, C = logits.shape
        stats = torch.empty(4, dtype=F32, device=logits.device)
        kept = torch.empty((), dtype=torch.int64, device=logits.device)
        ws = _lib.workspace.get(int(L.mm_ce2s_ws_bytes()), logits.device)
        cls = torch.is_tensor(thr)  # float32 [C] on the device: one threshold per class (mm_ce2s_*_cls)
        if row_w is None:
            fwd = L.mm_ce2s_fwd_cls if cls else L.mm_ce2s_fwd
            check(fwd(ptr(logits), ld, N, split, C, ptr(labels0), ptr(weight0), ignore_index, ptr(ta), ld_a, ptr(tb), ld_b,
                      temperature, ptr(thr) if cls else thr, ptr(stats), ptr(kept), ptr(ws), ws.numel(), stream()), "ce2s_fwd")
        else:  # one entry point for both kinds of threshold: a non-NULL thr_cls wins
            check(L.mm_ce2s_fwd_w(ptr(logits), ld, N, split, C, ptr(labels0), ptr(weight0), ignore_index, ptr(ta), ld_a, ptr(tb), ld_b,
                                  temperature, 0.0 if cls else thr, ptr(thr) if cls else None, ptr(row_w), ptr(stats), ptr(kept),
                                  ptr(ws), ws.numel(), stream()), "ce2s_fwd_w")
        ctx.save_for_backward(logits, labels0, weight0, ta, tb, stats, thr if cls else None, row_w)
        ctx.args = (ld, ld_a, ld_b, split, temperature, None if cls else thr, ignore_index)
        ctx.mark_non_differentiable(kept)
        return stats[0], stats[2], kept

    @staticmethod
    def backward(ctx, g0, g1, _):
        L = _lib.lib()
        logits, labels0, weight0, ta, tb, stats, thr_cls, row_w = ctx.saved_tensors
        ld, ld_a, ld_b, split, temperature, thr, ignore_index = ctx.args
        N, C = logits.shape
        g = torch.stack((g0, g1)).to(F32)  # the two upstream scalars side by side: the kernel's grad_out[2]
        if row_w is None:
            bwd = L.mm_ce2s_bwd if thr_cls is None else L.mm_ce2s_bwd_cls
            launch = lambda d: check(
                bwd(ptr(logits), ld, N, split, C, ptr(labels0), ptr(weight0), ignore_index, ptr(ta), ld_a, ptr(tb), ld_b,
                    temperature, thr if thr_cls is None else ptr(thr_cls), ptr(stats), ptr(g), ptr(d), C, stream()), "ce2s_bwd")
        else:
            launch = lambda d: check(
                L.mm_ce2s_bwd_w(ptr(logits), ld, N, split, C, ptr(labels0), ptr(weight0), ignore_index, ptr(ta), ld_a, ptr(tb), ld_b,
                                temperature, 0.0 if thr is None else thr, ptr(thr_cls), ptr(row_w), ptr(stats), ptr(g), ptr(d), C,
                                stream()), "ce2s_bwd_w")
        return _grad_rows(logits, ctx.in_dtype, launch), None, None, None, None, None, None, None, None, None


def cross_entropy_soft_pair(pred, split, gt_head, teacher, teacher_other=None, weight_head=None, temperature=1.0, threshold=None,
                            ignore_index=-100, row_weight=None):
    """``(loss_head, loss_tail, kept)``: rows ``[0, split)`` of ``pred`` [N, C] against the labels ``gt_head`` exactly as in
    :func:`cross_entropy_pair` (``None`` = unlabelled: loss 0, zero gradient rows), rows ``[split, N)`` against a teacher's
    DISTRIBUTION - the consistency loss of mean-teacher training, of which hard pseudo labels are the limit.

    ``teacher`` [N - split, C]: teacher logits, detached here.  The target is ``q = softmax(teacher / temperature)``, or with
    ``teacher_other`` (same shape) the ensemble ``0.5 * (softmax(teacher / T) + softmax(teacher_other / T))``.  A row's confidence
    is the largest probability of that target at temperature 1 - the float32 value ``pselab.teacher_labels`` judges the row by,
    bit for bit - and with ``threshold`` in (0, 1] only rows whose confidence is ``>= threshold`` are kept; ``None`` keeps every
    row whose teacher logits are finite; a float32 device tensor ``[C]`` gives every class its own threshold, a row being judged
    by that of its arg-max class (``pselab.AdaptiveThreshold``; the values are read on the device).  ``loss_tail`` = mean over the kept rows of ``sum_c q_c * (logsumexp(x) - x_c)``, i.e.
    KL(q || softmax(x)) plus the entropy of q; there is no ``T^2`` factor.  Nothing kept: loss 0 and a zero gradient.  ``kept``:
    the number of kept rows, an int64 device scalar.

    ``row_weight`` (float32 device tensor ``[N - split]``, e.g. ``pselab.agreement_weights``; not differentiated, a tensor that
    requires grad is refused): ``loss_tail`` = ``(1 / K) * sum over the K kept rows of row_w_i * sum_c q_c * (logsumexp(x) - x_c)``.
    The thresholds decide which rows are kept, the weights scale those that remain; ``kept`` ignores the weights.  ``None``: the
    call is launch for launch the call without the option.

    One autograd node and one backward launch write the whole gradient of ``pred``; all three matrices may be row-pitched views
    (``stride(1) == 1``) and are read in place."""
    who = "cross_entropy_soft_pair"
    if pred.dim() != 2:
        raise ValueError(f"{who}: pred must be [N, C]")
    N, C, split = int(pred.shape[0]), int(pred.shape[1]), int(split)
    if not 0 <= split <= N:
        raise ValueError(f"{who}: split {split} outside [0, {N}]")
    if C > 32:
        raise ValueError(f"{who}: {C} classes, the row kernels take at most 32")
    row_weight = _row_weight(row_weight, N - split, pred.device, who, "row_weight")
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not 0.0 < float(temperature) < float("inf"):
        raise ValueError(f"{who}: temperature must be a finite number > 0, not {temperature!r}")
    if torch.is_tensor(threshold):  # one threshold per class (pselab.AdaptiveThreshold's rows); the values stay on the device
        if threshold.dtype != F32 or tuple(threshold.shape) != (C,) or threshold.device != pred.device:
            raise ValueError(f"{who}: a threshold tensor must be float32 [{C}] on {pred.device}, not {threshold.dtype} "
                             f"{tuple(threshold.shape)} on {threshold.device}")
        threshold = threshold.detach().contiguous()
    elif threshold is not None and (isinstance(threshold, bool) or not isinstance(threshold, (int, float)) or not 0.0 < threshold <= 1.0):
        raise ValueError(f"{who}: threshold must be None, a number in (0, 1] or a float32 device tensor [C], not {threshold!r}")

    def logits(t, which):
        if not torch.is_tensor(t) or tuple(t.shape) != (N - split, C):
            got = tuple(t.shape) if torch.is_tensor(t) else type(t).__name__
            raise ValueError(f"{who}: {which} is {got}, the tail has [{N - split}, {C}] logits")
        t = t.detach().to(device=pred.device)
        # an empty tensor has no address: an empty tail passes one row that no row of pred reads (as cross_entropy_pair's labels)
        return t if N - split else t.new_zeros((1, C))

    teacher = logits(teacher, "teacher")
    if teacher_other is not None:
        teacher_other = logits(teacher_other, "teacher_other")
    gt_head = _labels(gt_head, split, pred.device, ignore_index, who, "gt_head")  # a labelled head without rows: 0/0
    weight_head = _class_weights(weight_head, C, pred.device, who, "weight_head")
    return _CrossEntropySoftPairFn.apply(pred, split, gt_head, weight_head, teacher, teacher_other, float(temperature),
                                         threshold if torch.is_tensor(threshold) else 0.0 if threshold is None else float(threshold),
                                         int(ignore_index), row_weight)


class _LovaszFn(torch.autograd.Function):
    """Lovasz-softmax of ``logits`` [N, C] against ``labels`` (csrc/lovasz.hip): the forward sorts every class's errors and leaves
    the signed, scaled Jaccard increments ``coef`` [C, N]; the backward is one row kernel over ``logits`` and ``coef``."""

    @staticmethod
    def forward(ctx, logits, labels, classes_all, ignore_index):
        _lib.require_cuda(logits, "pred")
        L = _lib.lib()
        ctx.in_dtype = logits.dtype
        logits, ld = _lib.row_pitched(logits)
        N, C = logits.shape
        err = torch.empty((C, N), dtype=F32, device=logits.device)  # needed by nobody after the call: freed on return
        coef = torch.empty((C, N), dtype=F32, device=logits.device)
        stats = torch.empty(3, dtype=F32, device=logits.device)
        ws = _lib.workspace.get(int(L.mm_lovasz_ws_bytes(N, C)), logits.device)
        check(L.mm_lovasz_fwd(ptr(logits), ld, N, C, ptr(labels), ignore_index, classes_all, ptr(err), ptr(coef), ptr(stats), ptr(ws),
                              ws.numel(), stream()), "lovasz_fwd")
        ctx.save_for_backward(logits, coef)
        ctx.ld = ld
        return stats[0]

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        logits, coef = ctx.saved_tensors
        N, C = logits.shape
        g = g.to(F32).contiguous()
        d = _grad_rows(logits, ctx.in_dtype, lambda d: check(
            L.mm_lovasz_bwd(ptr(logits), ctx.ld, N, C, ptr(coef), ptr(g), ptr(d), C, stream()), "lovasz_bwd"))
        return d, None, None, None


def lovasz_softmax(pred, gt, classes="present", ignore_index=-100):
    """Lovasz-softmax loss (Berman et al., CVPR 2018) of ``pred`` [N, C] against the labels ``gt`` [N]: the mean over the included
    classes of the Lovasz extension of the Jaccard loss of the class's errors ``|[y == c] - softmax(pred)_c|``.  Rows are counted as
    in :func:`cross_entropy_pair` (``gt != ignore_index`` and ``0 <= gt < C``).  ``classes="present"``: the classes that label a
    counted row; ``"all"``: every class.  Nothing counted: loss ``0.0`` and a zero gradient.  The Jaccard increments are constants
    of the gradient, as in the paper's implementation; there is no ``per_image``.  ``pred`` may be fp16, bf16 or a row-pitched
    view (``stride(1) == 1``), which is read in place.  One autograd node; bit-stable run to run."""
    who = "lovasz_softmax"
    if not isinstance(classes, str) or classes not in ("present", "all"):
        raise ValueError(f'{who}: classes must be "present" or "all", not {classes!r}')
    if not torch.is_tensor(pred) or pred.dim() != 2:
        raise ValueError(f"{who}: pred must be [N, C]")
    N, C = int(pred.shape[0]), int(pred.shape[1])
    if not 1 <= C <= 32:
        raise ValueError(f"{who}: {C} classes, the row kernels take 1 to 32")
    if N > 1 << 24:
        raise ValueError(f"{who}: {N} rows, the sort takes at most 2^24")
    if not torch.is_tensor(gt) or gt.dim() != 1 or gt.shape[0] != N:
        got = tuple(gt.shape) if torch.is_tensor(gt) else type(gt).__name__
        raise ValueError(f"{who}: gt is {got}, pred has {N} rows")
    gt = gt.to(device=pred.device, dtype=torch.int64).contiguous()
    return _LovaszFn.apply(pred, gt, 1 if classes == "all" else 0, int(ignore_index))


def _check_rows(who, x, name, first_row, width, columns):
    """What the two-segment row losses ask of ``x`` [N, ``width``] (2 to 32 ``columns``, N * width < 2^31) and ``first_row``; the width."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{who}: {name} must be [N, {width}]")
    N, C = int(x.shape[0]), int(x.shape[1])
    if not 2 <= C <= 32:
        raise ValueError(f"{who}: {C} {columns}, the row kernels take 2 to 32")
    if isinstance(first_row, bool) or not isinstance(first_row, int) or not 0 <= first_row <= N:
        raise ValueError(f"{who}: first_row {first_row!r} outside [0, {N}]")
    if N * C >= 1 << 31:
        raise ValueError(f"{who}: {N} rows of {C} {columns}, N * {width} must stay below 2^31")
    return C


class _TargetEntropyFn(torch.autograd.Function):
    """Entropy and diversity of rows [first_row, N) of ``logits`` (csrc/infomax.hip): two forward launches leave both scalars, the
    class mass, the row count and ``aux`` (ln(mass / prior) per class, 1 / (n ln C)); ONE backward launch writes the whole gradient
    from both upstream gradients and ``aux``."""

    @staticmethod
    def forward(ctx, logits, first_row, prior):
        _lib.require_cuda(logits, "pred")
        L = _lib.lib()
        ctx.in_dtype = logits.dtype
        logits, ld = _lib.row_pitched(logits)
        N, C = logits.shape
        dev = logits.device
        stats, mass, aux = (torch.empty(k, dtype=F32, device=dev) for k in (2, C, C + 1))
        count = torch.empty((), dtype=torch.int64, device=dev)
        ws = _lib.workspace.get(int(L.mm_im_ws_bytes()), dev)
        check(L.mm_im_fwd(ptr(logits), ld, N, first_row, C, ptr(prior), ptr(stats), ptr(mass), ptr(count), ptr(aux), ptr(ws), ws.numel(),
                          stream()), "im_fwd")
        ctx.save_for_backward(logits, aux)
        ctx.args = (ld, first_row)
        ctx.mark_non_differentiable(mass, count)
        ctx.set_materialize_grads(False)  # else every backward fills a zero gradient for ``mass`` and for ``count``: two launches
        return stats[0], stats[1], mass, count

    @staticmethod
    def backward(ctx, g0, g1, _mass, _count):
        if g0 is None and g1 is None:
            return None, None, None
        if g0 is None or g1 is None:  # one of the two scalars did not enter the loss
            g0, g1 = (torch.zeros_like(g1), g1) if g0 is None else (g0, torch.zeros_like(g0))
        L = _lib.lib()
        logits, aux = ctx.saved_tensors
        ld, first_row = ctx.args
        N, C = logits.shape
        g = torch.stack((g0, g1)).to(F32)  # the two upstream scalars side by side: the kernel's grad_out[2]
        d = _grad_rows(logits, ctx.in_dtype, lambda d: check(
            L.mm_im_bwd(ptr(logits), ld, N, first_row, C, ptr(aux), ptr(g), ptr(d), C, stream()), "im_bwd"))
        return d, None, None


def class_prior(prior, who="target_entropy"):
    """``prior`` (None, a sequence or a 1-D tensor of positive finite numbers) as a tuple of floats that sums to 1, or None."""
    if prior is None:
        return None
    vals = prior.detach().tolist() if torch.is_tensor(prior) and prior.dim() == 1 else prior
    ok = isinstance(vals, (list, tuple)) and len(vals) > 0 and all(
        isinstance(v, (int, float)) and not isinstance(v, bool) and 0.0 < float(v) < float("inf") for v in vals)
    if not ok:
        raise ValueError(f"{who}: the prior must be None or a sequence / 1-D tensor of positive finite numbers, not {prior!r}")
    total = sum(float(v) for v in vals)
    return tuple(float(v) / total for v in vals)


def _device_prior(prior, device):
    """A normalised prior (``class_prior``) on ``device``: uploaded once per device, rounded from float64."""
    if prior is None:
        return None
    return _uploaded("prior", prior, device, lambda: torch.tensor(prior, dtype=torch.float64).to(F32).to(device))


def target_entropy(pred, first_row=0, prior=None):
    """``(ent, div, mass, count)`` of the rows ``[first_row, N)`` of ``pred`` [N, C] - the unlabelled target rows of a joined
    [source | target] pass, or with ``first_row=0`` all rows.  Counted are the rows whose logits are all finite, ``count`` of them
    (int64 device scalar).  ``ent``: the mean over them of the softmax entropy divided by ln C, in [0, 1] - entropy minimisation
    (MinEnt, Vu et al., CVPR 2019).  ``mass`` (fp32 [C]): their mean softmax.  ``div`` = KL(mass || prior) / ln C >= 0, the
    diversity term of information maximisation (SHOT, Liang et al., ICML 2020), which keeps ``ent`` from collapsing onto the
    majority class; ``prior``: None = uniform, or C positive finite numbers (a sequence or a tensor; normalised to sum 1 on the
    host and cached per device - pass a sequence in a training loop, a device tensor is read back on every call).  Nothing counted:
    both losses 0, ``mass`` 0, a zero gradient.

    ``ent`` and ``div`` are differentiable, one autograd node and one backward launch write the whole gradient of ``pred`` (zero
    rows before ``first_row``); ``mass`` and ``count`` are detached.  ``mass`` is the mean over THIS call's rows: under data
    parallelism each rank's own batch mean, as batch-norm statistics are, not reduced over ranks.  ``pred`` may be fp16, bf16 or a
    row-pitched view (``stride(1) == 1``), which is read in place.  Bit-stable run to run."""
    who = "target_entropy"
    C = _check_rows(who, pred, "pred", first_row, "C", "classes")
    prior = class_prior(prior, who)
    if prior is not None and len(prior) != C:
        raise ValueError(f"{who}: the prior has {len(prior)} entries for C = {C} classes")
    _lib.require_cuda(pred, "pred")
    return _TargetEntropyFn.apply(pred, first_row, _device_prior(prior, pred.device))


CORAL_MODES = {"plain": 0, "log": 1}  # the ``mode`` of mm_coral_fwd


class _CoralFn(torch.autograd.Function):
    """Correlation alignment of the rows [0, first_row) and [first_row, N) of ``x`` (csrc/coral.hip): two forward launches leave the
    loss, the two row counts, means and covariances and ``aux`` (the means as fp32 pairs and the two matrices 2 / (n_a - 1) * G_a); ONE backward
    launch writes the whole gradient from the upstream gradient and ``aux``."""

    @staticmethod
    def forward(ctx, x, first_row, mode, eps):
        _lib.require_cuda(x, "x")
        L = _lib.lib()
        ctx.in_dtype = x.dtype
        x, ld = _lib.row_pitched(x)
        N, d = x.shape
        dev = x.device
        loss = torch.empty((), dtype=F32, device=dev)
        mean, cov, aux = (torch.empty(s, dtype=F32, device=dev) for s in ((2, d), (2, d, d), (4 * d + 2 * d * d,)))
        count = torch.empty(2, dtype=torch.int64, device=dev)
        ws = _lib.workspace.get(int(L.mm_coral_ws_bytes(d)), dev)
        check(L.mm_coral_fwd(ptr(x), ld, N, first_row, d, mode, eps, ptr(loss), ptr(count), ptr(mean), ptr(cov), ptr(aux), ptr(ws),
                             ws.numel(), stream()), "coral_fwd")
        ctx.save_for_backward(x, aux)
        ctx.args = (ld, first_row)
        ctx.mark_non_differentiable(count, mean, cov)
        ctx.set_materialize_grads(False)  # else every backward fills zero gradients for the three detached outputs
        return loss, count, mean, cov

    @staticmethod
    def backward(ctx, g, _count, _mean, _cov):
        if g is None:
            return None, None, None, None
        L = _lib.lib()
        x, aux = ctx.saved_tensors
        ld, first_row = ctx.args
        N, d = x.shape
        g = g.to(F32).contiguous()
        dx = _grad_rows(x, ctx.in_dtype, lambda dx: check(
            L.mm_coral_bwd(ptr(x), ld, N, first_row, d, ptr(aux), ptr(g), ptr(dx), d, stream()), "coral_bwd"))
        return dx, None, None, None


def coral(x, first_row, mode="log", eps=1e-4):
    """Correlation alignment of two row segments of ``x`` [N, d]: rows ``[0, first_row)`` (source) against rows ``[first_row, N)``
    (target) of a joined [source | target] pass.  Returns ``dict(loss, count, mean, cov)``, all device tensors.  Counted are the
    rows whose values are all finite, ``count`` (int64 [2]) of them per segment; ``mean`` [2, d] and ``cov`` [2, d, d] (fp32) are
    their means and unbiased covariances C_s, C_t.  ``mode="plain"``: Deep CORAL (Sun & Saenko, ECCV-W 2016), ``loss`` =
    ||C_s - C_t||_F^2 / (4 d^2).  ``mode="log"`` (default): Deep LogCORAL (Morerio et al., ICLR 2018; the uni-modal baseline of the
    xMUDA comparison), ``loss`` = ||log(C_s + eps I) - log(C_t + eps I)||_F^2 / d^2 with the matrix logarithm of the symmetric
    eigendecomposition, which the kernel computes itself (cyclic Jacobi in fp64); the ridge ``eps`` > 0 keeps a singular covariance (fewer
    counted rows than d, a constant column) finite.  A segment with fewer than two counted rows: loss 0, a zero gradient.

    ``loss`` is differentiable with respect to BOTH segments' rows; one autograd node, two forward launches and one backward
    launch, no host read; ``count``, ``mean`` and ``cov`` are detached.  The statistics are those of THIS call's rows: under
    data parallelism each rank's own batch's, as batch-norm statistics are, not reduced over ranks.  Generic in d (2 to 32): the
    class logits of a head, or a feature matrix such as the 3D branch's 16-channel ``feats``.  ``x`` may be fp16, bf16 or a
    row-pitched view (``stride(1) == 1``), which is read in place.  Bit-stable run to run."""
    who = "coral"
    if not isinstance(mode, str) or mode not in CORAL_MODES:
        raise ValueError(f'{who}: mode must be "log" or "plain", not {mode!r}')
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 < float(eps) < float("inf"):
        raise ValueError(f"{who}: eps must be a finite number > 0, not {eps!r}")
    _check_rows(who, x, "x", first_row, "d", "columns")
    _lib.require_cuda(x, "x")
    loss, count, mean, cov = _CoralFn.apply(x, first_row, CORAL_MODES[mode], float(eps))
    return dict(loss=loss, count=count, mean=mean, cov=cov)


ADV_MODES = {"softmax": 0, "selfinfo": 1}  # the ``mode`` of mm_adv_fwd
ADV_HIDDEN = (16, 32, 64)


def adversarial_param_count(C, hidden):
    """The length of the discriminator's flat parameter buffer: W1 [H][C], b1 [H], W2 [H][H], b2 [H], w3 [H], b3."""
    return hidden * C + hidden * hidden + 3 * hidden + 1


class _AdversarialFn(torch.autograd.Function):
    """The point discriminator on the rows [0, first_row) (source) and [first_row, N) (target) of ``x`` (csrc/adv.hip): the forward
    leaves both losses, the counts, the discriminator's parameter gradient and ``gx`` = dloss_G / dx; ONE backward launch scales the
    saved ``gx`` by the upstream gradient.  ``params`` gets no gradient from autograd: the caller steps it with ``grad_params``."""

    @staticmethod
    def forward(ctx, x, first_row, params, mode, hidden):
        _lib.require_cuda(x, "x")
        L = _lib.lib()
        ctx.in_dtype = x.dtype
        x, ld = _lib.row_pitched(x)
        N, C = x.shape
        dev = x.device
        stats = torch.empty(2, dtype=F32, device=dev)
        count, correct = (torch.empty(2, dtype=torch.int64, device=dev) for _ in range(2))
        dparams = torch.empty(params.numel(), dtype=F32, device=dev)
        gx = torch.empty((N, C), dtype=F32, device=dev)
        ws = _lib.workspace.get(int(L.mm_adv_ws_bytes(C, hidden)), dev)
        check(L.mm_adv_fwd(ptr(x), ld, N, first_row, C, hidden, mode, ptr(params), ptr(stats), ptr(count), ptr(correct), ptr(dparams),
                           ptr(gx), C, ptr(ws), ws.numel(), stream()), "adv_fwd")
        ctx.save_for_backward(gx)
        loss_g, loss_d = stats[1], stats[0]
        ctx.mark_non_differentiable(loss_d, dparams, count, correct)
        ctx.set_materialize_grads(False)  # else every backward fills zero gradients for the four detached outputs
        return loss_g, loss_d, dparams, count, correct

    @staticmethod
    def backward(ctx, g, _d, _p, _n, _c):
        if g is None:
            return None, None, None, None, None
        L = _lib.lib()
        (gx,) = ctx.saved_tensors
        N, C = gx.shape
        g = g.to(F32).contiguous()
        dx = _grad_rows(gx, ctx.in_dtype, lambda dx: check(L.mm_adv_bwd(ptr(gx), C, N, C, ptr(g), ptr(dx), C, stream()), "adv_bwd"))
        return dx, None, None, None, None


def adversarial(x, first_row, params, mode="selfinfo", hidden=64):
    """Adversarial alignment in the output space: a point-wise discriminator D on the rows of ``x`` [N, C], rows ``[0, first_row)``
    source (domain 0) and ``[first_row, N)`` target (domain 1) of a joined [source | target] pass.  D reads ``u`` = softmax(x_i)
    (``mode="softmax"``, AdaptSegNet, Tsai et al., CVPR 2018) or the weighted self-information -p ln p / ln C
    (``mode="selfinfo"``, default; AdvEnt, Vu et al., CVPR 2019) and is the MLP ``a = w3 . lrelu(W2 lrelu(W1 u + b1) + b2) + b3``
    with slope 0.2 and ``hidden`` = 16, 32 or 64 units per layer.  ``params``: its weights as ONE flat fp32 device tensor of
    ``adversarial_param_count(C, hidden)`` elements in the order W1 [H][C], b1, W2 [H][H], b2, w3, b3.

    Returns ``dict(loss_g, loss_d, grad_params, count, correct)``, all device tensors.  Counted are the rows whose logits are all
    finite, ``count`` (int64 [2]) per domain.  ``loss_d`` = 0.5 mean_src softplus(a) + 0.5 mean_trg softplus(-a), the
    discriminator's binary cross entropy, and ``grad_params`` its gradient with respect to ``params``, for the caller to step D
    with; ``loss_g`` = mean_trg softplus(a), the target rows called "source" - the term the segmentation network minimises.
    ``correct`` (int64 [2]): source rows with a <= 0 and target rows with a > 0.  Only ``loss_g`` is differentiable, and only with
    respect to ``x``: its gradient was formed in the forward with the weights D had THEN, so ``params`` may be stepped before the
    backward runs, and autograd never sees ``params``.  One autograd node, three forward launches and one backward launch, no host
    read.  The statistics are those of THIS call's rows.  ``x`` may be fp16, bf16 or a row-pitched view (``stride(1) == 1``),
    which is read in place.  Bit-stable run to run."""
    who = "adversarial"
    if not isinstance(mode, str) or mode not in ADV_MODES:
        raise ValueError(f'{who}: mode must be "selfinfo" or "softmax", not {mode!r}')
    if isinstance(hidden, bool) or not isinstance(hidden, int) or hidden not in ADV_HIDDEN:
        raise ValueError(f"{who}: hidden must be 16, 32 or 64, not {hidden!r}")
    C = _check_rows(who, x, "x", first_row, "C", "classes")
    need = adversarial_param_count(C, hidden)
    if not torch.is_tensor(params) or params.dtype != F32 or params.dim() != 1 or params.numel() != need or not params.is_contiguous():
        raise ValueError(f"{who}: params must be a flat contiguous float32 tensor of {need} elements for C = {C}, hidden = {hidden}")
    _lib.require_cuda(x, "x")
    _lib.require_cuda(params, "params")
    loss_g, loss_d, dparams, count, correct = _AdversarialFn.apply(x, first_row, params.detach(), ADV_MODES[mode], hidden)
    return dict(loss_g=loss_g, loss_d=loss_d, grad_params=dparams, count=count, correct=correct)


class _KLFn(torch.autograd.Function):
    """mean_i sum_c softmax(t)_ic * (log_softmax(t)_ic - log_softmax(p)_ic); gradient flows to p only (t is detached)."""

    @staticmethod
    def forward(ctx, pred, target):
        _lib.require_cuda(pred, "pred")
        L = _lib.lib()
        pred = pred.to(F32).contiguous()
        target = target.detach().to(F32).contiguous()
        N, C = pred.shape
        out = torch.empty(1, dtype=F32, device=pred.device)
        ws = _lib.workspace.get(int(L.mm_loss_ws_bytes()), pred.device)
        check(L.mm_kl_fwd(ptr(pred), C, ptr(target), C, N, C, ptr(out), ptr(ws), ws.numel(), stream()), "kl_fwd")
        ctx.save_for_backward(pred, target)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        L = _lib.lib()
        pred, target = ctx.saved_tensors
        N, C = pred.shape
        d = torch.empty_like(pred)
        g = g.to(F32).contiguous()
        check(L.mm_kl_bwd(ptr(pred), C, ptr(target), C, N, C, ptr(g), ptr(d), C, stream()), "kl_bwd")
        return d, None


def kl_to_detached(pred, target):
    return _KLFn.apply(pred, target)


def cross_modal_loss(gt_for_2d, prediction_avg, gt_for_3d, prediction_3d):
    """train.py:157-184: each branch's aux head mimics the other branch's detached main head."""
    return kl_to_detached(prediction_avg, gt_for_2d), kl_to_detached(prediction_3d, gt_for_3d)


XM_WINDOW_MAX = 3  # the largest window radius of mm_xm_search: 7 x 7 pixels


def _window_search(seg, index, rows, radius, split, direction, counts):
    """``(sel, klmin)`` of one ``mm_xm_search`` call over the detached map ``seg`` [B, C, H, W] (any strides) and ``rows`` [N, C]."""
    L = _lib.lib()
    seg = seg.detach()
    if seg.dtype != F32:
        seg = seg.float()
    rows, ld = _lib.row_pitched(rows.detach())
    B, C, H, W = seg.shape
    sel = torch.empty(max(index.n, 1), dtype=torch.int32, device=seg.device)
    klmin = torch.empty(index.n, dtype=F32, device=seg.device)
    ws = _lib.workspace.get(int(L.mm_xm_search_ws_bytes()), seg.device)
    check(L.mm_xm_search(ptr(seg), seg.stride(0), seg.stride(2), seg.stride(3), seg.stride(1), B, H, W, C, ptr(index.key), ptr(rows), ld,
                         index.n, split, radius, direction, ptr(sel), ptr(klmin), ptr(counts), ptr(ws), ws.numel(), stream()), "xm_search")
    return sel, klmin


def cross_modal_dense(gt_for_2d, map_avg, map_main, prediction_3d, index, radius, split=None):
    """The cross-modal KL pair of :func:`cross_modal_loss` with each point matched against the DENSE 2D prediction in the
    ``(2 radius + 1)^2`` pixel window round its own pixel instead of against that one pixel (the sparse-to-dense matching of DsCML,
    Peng et al., ICCV 2021, as a hard minimum).  ``gt_for_2d`` [N, C]: the 3D main head's rows (teacher of the 2D term);
    ``map_avg`` / ``map_main`` [B, C, H, W]: the dense logits of the 2D aux and main head (``seg_logit_avg_2d``, ``seg_logit_2d``;
    any strides, e.g. the halves of one NHWC buffer); ``prediction_3d`` [N, C]: the 3D aux head's rows; ``index``: the batch's
    ``lifting.PixelIndex``.  The candidates of point i are the pixels of its window inside its own image, the centre first, then
    row-major.  ``j*(i) = argmin_j KL(softmax(gt_for_2d_i) || softmax(map_avg_j))`` and
    ``k*(i) = argmin_j KL(softmax(map_main_j) || softmax(prediction_3d_i))``: the smallest value, the earliest among equal ones, a
    NaN is skipped, nothing left keeps the centre.  The selection is a constant of the gradient (the sub-gradient of a minimum).

    Returns ``(pairs, info)``.  ``pairs``: one ``(loss_avg, loss_3d)`` per row range - ``split=None``: all rows; ``split=P``: rows
    ``[0, P)``, then rows ``[P, N)`` - with ``loss_avg = kl_to_detached(map_avg[j*], gt_for_2d)`` and ``loss_3d =
    kl_to_detached(prediction_3d, map_main[k*])`` over the range's rows; an empty range gives 0 and no gradient.  ``map_avg`` is
    lifted ONCE for all ranges (``lifting.lift_at``: its backward stores into the gradient slot the plain ``lift`` of that map would
    fill - do not also back-propagate through that one).  ``info``: ``sel_2d`` / ``sel_3d`` (int32 [N] pixel keys), ``klmin_2d`` /
    ``klmin_3d`` (fp32 [N], the matched rows' KL), ``moved`` / ``shift`` (int64 [2, 2]: per term 2D / 3D and per range, the rows
    whose match left the centre and the sum of their Chebyshev displacements), all on the device.  ``radius`` 0 is the plain pair.
    Two launches per search, no host read; bit-stable run to run."""
    from . import lifting

    who = "cross_modal_dense"
    if isinstance(radius, bool) or not isinstance(radius, int) or not 0 <= radius <= XM_WINDOW_MAX:
        raise ValueError(f"{who}: radius must be an integer in [0, {XM_WINDOW_MAX}], not {radius!r}")
    N = index.n
    for name, t in (("gt_for_2d", gt_for_2d), ("prediction_3d", prediction_3d)):
        if not torch.is_tensor(t) or t.dim() != 2 or t.shape[0] != N or t.shape[1] != map_avg.shape[1]:
            raise ValueError(f"{who}: {name} must be [{N}, {map_avg.shape[1]}] (a row per point of the index, a column per class)")
    if tuple(map_avg.shape) != tuple(map_main.shape) or tuple(map_avg.shape[2:]) != (index.H, index.W):
        raise ValueError(f"{who}: the maps are {tuple(map_avg.shape)} and {tuple(map_main.shape)}, the index has {index.H} x {index.W} pixels")
    if split is not None and (isinstance(split, bool) or not isinstance(split, int) or not 0 <= split <= N):
        raise ValueError(f"{who}: split {split!r} outside [0, {N}]")
    _lib.require_cuda(map_avg, "map_avg")
    P = N if split is None else split
    counts = torch.empty((2, 4), dtype=torch.int64, device=map_avg.device)
    sel_2d, kl_2d = _window_search(map_avg, index, gt_for_2d, radius, P, 0, counts[0])
    sel_3d, kl_3d = _window_search(map_main, index, prediction_3d, radius, P, 1, counts[1])
    matched_avg = lifting.lift_at(map_avg, index, sel_2d)
    matched_main = lifting.lift_at(map_main.detach(), index, sel_3d)
    pairs = []
    for lo, hi in ((0, N),) if split is None else ((0, P), (P, N)):
        if hi == lo:
            zero = torch.zeros((), dtype=F32, device=map_avg.device)
            pairs.append((zero, zero))
        else:
            pairs.append((kl_to_detached(matched_avg[lo:hi], gt_for_2d[lo:hi]), kl_to_detached(prediction_3d[lo:hi], matched_main[lo:hi])))
    return pairs, dict(sel_2d=sel_2d[:N], sel_3d=sel_3d[:N], klmin_2d=kl_2d, klmin_3d=kl_3d, moved=counts[:, :2], shift=counts[:, 2:])


# ---------------------------------------------------------------------------------------------- registry (reference API)
class _GenericLoss:
    def __init__(self, **args):
        self.other_args = args

    def __repr__(self):
        r = self.name
        if self.other_args:
            r += "[" + ",".join(f"{n}={v}" for n, v in self.other_args.items()) + "]"
        return r


class L1(_GenericLoss):
    name, default_target = "l1", "depth"

    def __call__(self, pred, gt, **kw):
        mask = gt > 0
        return torch.mean(torch.abs(pred[mask] - gt[mask]))


class L2(_GenericLoss):
    name, default_target = "l2", "depth"

    def __call__(self, pred, gt, **kw):
        mask = gt > 0
        return torch.mean(torch.square(pred[mask] - gt[mask]))


class CrossEntropy(_GenericLoss):
    name, default_target = "cross_entropy", "segmentation"

    def __call__(self, pred, gt, weight=None, **kw):
        return cross_entropy(pred, gt, weight)


class LovaszSoftmax(_GenericLoss):
    name, default_target = "lovasz_softmax", "segmentation"

    def __call__(self, pred, gt, classes="present", **kw):
        return lovasz_softmax(pred, gt, classes)


_LOSSES = {"l1": L1, "l2": L2, "cross_entropy": CrossEntropy, "lovasz_softmax": LovaszSoftmax}


class Loss:
    def __init__(self, cfg):
        if isinstance(cfg, str):
            fn = _LOSSES[cfg]()
            self._losses = [(1.0, fn.default_target, fn)]
        elif isinstance(cfg, (list, tuple)):
            self._losses = []
            for item in cfg:
                if isinstance(item, str):
                    fn = _LOSSES[item]()
                    self._losses.append((1.0, fn.default_target, fn))
                else:
                    cls = _LOSSES[item["name"]]
                    self._losses.append((item.get("weight", 1.0), item.get("target", cls.default_target),
                                         cls(**dict(item.get("args", {}) or {}))))
        else:
            raise ValueError(f"not recognized cfg {cfg}")

    def update_loss_params(self, loss_name, loss_target, **kwargs):
        for _, target, loss in self._losses:
            if loss.name == loss_name and target == loss_target:
                loss.other_args.update(**kwargs)

    def __call__(self, target, image=None, pred=None, gt=None):
        sel = [(w, l) for w, t, l in self._losses if t == target]
        if not sel:
            raise RuntimeError(f"no losses for loss target {target}")
        out = 0.0
        for w, l in sel:
            out = out + w * l(image=image, pred=pred, gt=gt, **l.other_args)
        return out

    def __repr__(self):
        if len(self._losses) == 1:
            w, _, l = self._losses[0]
            return (str(w) if w != 1.0 else "") + str(l)
        return "+".join(f"{w if w != 1.0 else ''}{l}" for w, _, l in self._losses)

    def split_by_target(self):
        out = {}
        for t in {t for _, t, _ in self._losses}:
            c = deepcopy(self)
            c._losses = [deepcopy(l) for l in self._losses if l[1] == t]
            out[t] = c
        return out
