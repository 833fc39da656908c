"""Target-domain entropy and diversity terms of the two-domain step (train.py): everything ``train_kwargs["lambda_minent"]`` and
``["lambda_div"]`` switch on, in one policy object."""
import torch

from .losses import class_prior, target_entropy
from .stepopts import NON_NEGATIVE, LogitTerm, number


class TargetEntropy(LogitTerm):
    """With ``lambda_minent`` > 0 or ``lambda_div`` > 0 each main head also learns from its own predictions of the unlabelled TARGET
    rows - no teacher pass, no extra forward, one ``losses.target_entropy`` call per head: loss_2d += lambda_minent * ent2d +
    lambda_div * div2d, the same for 3D.  ``ent``: the mean softmax entropy of the target rows over ln C (entropy minimisation,
    MinEnt: one of xMUDA's uda baselines).  ``div``: KL(batch-mean target prediction || ``div_prior``) / ln C, the diversity term
    of information maximisation (SHOT), the guard against MinEnt's collapse onto the majority class.  ``div_prior``: None =
    uniform, or C positive finite numbers (normalised to sum 1); values are checked here, the length at the first step.  Rows with
    a non-finite logit are not counted.  Both terms are logged as ``{stage}/minent_tgt_2d`` / ``_3d`` and ``{stage}/div_tgt_2d``
    / ``_3d`` even when one weight is 0; ``last_target_mass``: fp32 [2, C] device tensor, the batch-mean target prediction of the
    2D and the 3D head.  Under data parallelism that mean is the rank's own batch's, as batch-norm statistics are: it is NOT
    reduced over ranks.  The terms are independent of ``lambda_pl``, of the teacher and of the loss registry's entries and compose
    with all of them; validation, test and ``predict_step`` do not evaluate them.  Both weights 0.0 (default): nothing is called
    or allocated, no log key appears, the step is launch for launch the step without the options."""

    FORWARDED = ("lambda_minent", "lambda_div", "div_prior", "last_target_mass")

    def __init__(self, train_kwargs):
        self.lambda_minent = number(train_kwargs, "lambda_minent", 0.0, *NON_NEGATIVE)
        self.lambda_div = number(train_kwargs, "lambda_div", 0.0, *NON_NEGATIVE)
        # normalised here once; a tuple, so that the loss call finds its device copy without a host read
        self.div_prior = class_prior(train_kwargs.get("div_prior"), "train_kwargs['div_prior']")
        self.last_target_mass = None
        self._classes = None  # the class count the prior's length was checked against

    @property
    def active(self):
        return self.lambda_minent > 0.0 or self.lambda_div > 0.0

    @staticmethod
    def _head_classes(net):
        """The class count of a network's main head where it can be read off the module (Net2DSeg.con1_1_avg, Net3DSeg.linear, or a bare
        head)."""
        for m in (getattr(net, "con1_1_avg", None), getattr(net, "linear", None), net):
            C = getattr(m, "out_channels", None) or getattr(m, "out_features", None)
            if C:
                return int(C)
        return None

    def begin_step(self, trainer):
        """Before anything of the step is queued: a ``div_prior`` whose length is not the class count is refused.  The count is
        ``trainer.num_classes`` or read off the heads; a plugin network that shows neither is checked by the loss call itself."""
        if not self.active or self.div_prior is None or self._classes is not None:
            return
        C = trainer.num_classes or next((c for c in map(self._head_classes, trainer.model.values()) if c), None)
        if C is not None:
            self._check(int(C))

    def _check(self, C):
        if self.div_prior is not None and len(self.div_prior) != C:
            raise ValueError(f"train_kwargs['div_prior'] has {len(self.div_prior)} entries, the heads have C = {C} classes")
        self._classes = C

    def terms(self, logits_2d, logits_3d, first_row):
        """``(ent2d, div2d, ent3d, div3d)`` of the rows ``[first_row, N)`` of the two main heads' logits, or None with both weights 0."""
        if not self.active:
            return None
        self._check(int(logits_2d.shape[1]))
        e2, d2, m2, _ = target_entropy(logits_2d, first_row, self.div_prior)
        e3, d3, m3, _ = target_entropy(logits_3d, first_row, self.div_prior)
        self.last_target_mass = torch.stack((m2, m3))
        return e2, d2, e3, d3

    def add(self, logs, stage, loss_2d, loss_3d, terms):
        """Logs the four terms of ``stage`` and returns the two branch losses with them added."""
        e2, d2, e3, d3 = terms
        logs[f"{stage}/minent_tgt_2d"], logs[f"{stage}/minent_tgt_3d"] = e2, e3
        logs[f"{stage}/div_tgt_2d"], logs[f"{stage}/div_tgt_3d"] = d2, d3
        return (loss_2d + self.lambda_minent * e2 + self.lambda_div * d2, loss_3d + self.lambda_minent * e3 + self.lambda_div * d3)
