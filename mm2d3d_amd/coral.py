"""Correlation alignment of the source and the target batch in the two-domain step (train.py): everything
``train_kwargs["lambda_coral"]``, ``["coral"]`` and ``["coral_eps"]`` switch on, in one policy object."""
from .losses import CORAL_MODES, coral
from .stepopts import NON_NEGATIVE, POSITIVE, LogitTerm, number


class DomainAlignment(LogitTerm):
    """With ``lambda_coral`` > 0 each main head also aligns the second-order statistics of its logits on the SOURCE rows with
    those on the TARGET rows - no extra forward, one ``losses.coral`` call per head on the [source | target] logits the step
    already holds: loss_2d += lambda_coral * coral(l2d, P), the same for 3D.  ``coral``: "log" (default; Deep LogCORAL, Morerio et
    al., ICLR 2018, the uni-modal baseline of the xMUDA comparison beside MinEnt and pseudo labels) or "plain" (Deep CORAL, Sun &
    Saenko, ECCV-W 2016, which applies the loss to the classifier layer's outputs as here).  ``coral_eps``: the ridge of the log
    mode, finite and > 0 (default 1e-4).  Rows with a non-finite logit are not counted; a domain with fewer than two counted rows
    gives 0.  The terms are logged as ``{stage}/coral_2d`` / ``_3d``; ``last_coral``: ``{"cov_2d", "cov_3d", "count"}`` - fp32
    [2, C, C] device tensors, the source's and the target's covariance of each head's logits, and the int64 [2] counted rows of
    the 2D head.  Under data parallelism each rank aligns its OWN batch's covariances, as batch-norm statistics are the rank's
    own: nothing is reduced over ranks.  Independent of ``lambda_pl``, of the teacher, of MinEnt and of the loss registry's
    entries and composes with all of them; validation, test and ``predict_step`` do not evaluate it.  ``lambda_coral`` 0.0
    (default): nothing is called or allocated, no log key appears, the step is launch for launch the step without the option."""

    FORWARDED = ("lambda_coral", "coral", "coral_eps", "last_coral")
    READS_SOURCE = True

    def __init__(self, train_kwargs):
        self.lambda_coral = number(train_kwargs, "lambda_coral", 0.0, *NON_NEGATIVE)
        self.coral = train_kwargs.get("coral", "log")
        if not isinstance(self.coral, str) or self.coral not in CORAL_MODES:
            raise ValueError(f"train_kwargs['coral'] must be \"log\" or \"plain\", not {self.coral!r}")
        self.coral_eps = number(train_kwargs, "coral_eps", 1e-4, *POSITIVE)
        self.last_coral = None

    @property
    def active(self):
        return self.lambda_coral > 0.0

    def terms(self, logits_2d, logits_3d, first_row):
        """``(coral2d, coral3d)`` of the two main heads' logits, rows ``[0, first_row)`` against ``[first_row, N)``; None with the
        weight 0."""
        if not self.active:
            return None
        c2 = coral(logits_2d, first_row, self.coral, self.coral_eps)
        c3 = coral(logits_3d, first_row, self.coral, self.coral_eps)
        self.last_coral = {"cov_2d": c2["cov"], "cov_3d": c3["cov"], "count": c2["count"]}
        return c2["loss"], c3["loss"]

    def add(self, logs, stage, loss_2d, loss_3d, terms):
        """Logs the two terms of ``stage`` and returns the two branch losses with them added."""
        c2, c3 = terms
        logs[f"{stage}/coral_2d"], logs[f"{stage}/coral_3d"] = c2, c3
        return loss_2d + self.lambda_coral * c2, loss_3d + self.lambda_coral * c3
