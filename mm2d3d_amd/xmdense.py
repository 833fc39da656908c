"""Sparse-to-dense cross-modal matching in the two-domain step (train.py): everything ``train_kwargs["xm_window"]`` switches on, in
one policy object."""
import torch

from .losses import XM_WINDOW_MAX, cross_modal_dense
from .stepopts import StepOption


class DenseMatching(StepOption):
    """With ``xm_window`` = r >= 1 the cross-modal KL terms no longer couple a point to the one pixel it projects to: each point is
    matched against the dense 2D prediction in the (2r + 1)^2 window round its pixel and learns from (or teaches) the best match
    (``losses.cross_modal_dense``; the sparse-to-dense idea of DsCML, Peng et al., ICCV 2021, without its discriminators and
    multi-scale patches).  The terms keep their log keys ``xm_loss_{src,tgt}_{2d,3d}``, their separate means over source and target
    rows and their weights ``lambda_xm_src`` / ``lambda_xm_trg``; the centre is always a candidate, so every row's matched KL is <=
    its plain KL.  Logged besides: ``{stage}/xm_moved_2d`` / ``_3d``, the share of the step's rows whose match left the centre, and
    ``{stage}/xm_shift_2d`` / ``_3d``, the mean Chebyshev displacement of those rows (0 when none moved).  ``last_match``:
    ``{"sel_2d", "sel_3d", "klmin_2d", "klmin_3d", "moved", "shift", "split"}`` of the last step - device tensors over the step's
    [source | target] rows (``cross_modal_dense``'s ``info``; ``moved`` / ``shift`` int64 [2, 2]: term x domain) and the number of
    source rows; in the two-call pass (``joint_domains=False``) the keys of each domain count the pixels of its own call's maps.
    A pure loss: nothing to checkpoint, nothing reduced over ranks.  Validation, test, ``predict_step`` and the teacher pass never
    match.  Independent of every other option of the step and composes with all of them.  ``xm_window`` 0 (default): nothing is
    called or allocated, no log key appears, the step is launch for launch the step without the option."""

    FORWARDED = ("xm_window", "last_match")

    def __init__(self, train_kwargs):
        r = train_kwargs.get("xm_window", 0)
        if isinstance(r, bool) or not isinstance(r, int) or not 0 <= r <= XM_WINDOW_MAX:
            raise ValueError(f"train_kwargs['xm_window'] must be an integer in [0, {XM_WINDOW_MAX}], not {r!r}")
        self.xm_window = r
        self.last_match = None
        self._calls = []
        self._plain = None  # the trainer's ``cross_modal_loss`` hook, which forms the terms while the window is 0

    @property
    def active(self):
        return self.xm_window > 0

    def begin_step(self, trainer):
        self._calls, self._plain = [], trainer.cross_modal_loss

    def terms(self, gt_for_2d, prediction_3d, aux2d, p2d, batch, split=None):
        """The matched ``(loss_avg, loss_3d)`` pairs of one pass of the 2D network over ``batch`` (``aux2d`` / ``p2d``: its aux and
        main outputs): one pair with ``split=None``, else one for the rows ``[0, split)`` and one for ``[split, N)``.  With the window
        0 the plain pairs of the trainer's ``cross_modal_loss`` over the same rows."""
        if not self.active:
            a2d, l2d = aux2d["seg_logit_avg"], p2d["seg_logit"]
            if split is None:
                return (self._plain(gt_for_2d, a2d, l2d, prediction_3d),)
            return tuple(self._plain(gt_for_2d[r], a2d[r], l2d[r], prediction_3d[r]) for r in (slice(0, split), slice(split, None)))
        pairs, info = cross_modal_dense(gt_for_2d, aux2d["seg_logit_avg_2d"], p2d["seg_logit_2d"], prediction_3d, batch["_pixel_index"],
                                        self.xm_window, split)
        self._calls.append((info, int(gt_for_2d.shape[0]) if split is None else split))
        return pairs

    def log(self, logs, stage):
        """Files ``last_match`` and the four log entries of the step from the calls since ``begin_step``: one joined call, or the
        source's call followed by the target's.  Nothing with the window 0."""
        if not self.active:
            return
        if len(self._calls) == 1:
            info, split = self._calls[0]
            m = dict(info)
        else:
            (src, split), (trg, _) = self._calls
            m = {k: torch.cat((src[k], trg[k])) for k in ("sel_2d", "sel_3d", "klmin_2d", "klmin_3d")}
            for k in ("moved", "shift"):  # each call counted its rows as range 0
                m[k] = torch.stack((src[k][:, 0], trg[k][:, 0]), 1)
        m["split"] = split
        self.last_match, self._calls = m, []
        n = max(int(m["sel_2d"].shape[0]), 1)
        moved, shift = m["moved"].sum(1), m["shift"].sum(1)
        share, mean = moved.to(torch.float32) / n, shift.to(torch.float32) / moved.clamp(min=1).to(torch.float32)
        for i, d in enumerate(("2d", "3d")):
            logs[f"{stage}/xm_moved_{d}"], logs[f"{stage}/xm_shift_{d}"] = share[i], mean[i]
