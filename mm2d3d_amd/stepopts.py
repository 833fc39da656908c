"""What the two-domain step (train.py) asks of an optional term: the protocol of the policy objects in ``train.OPTIONS`` and the one
check of their numeric ``train_kwargs`` values."""
import math

NON_NEGATIVE = (lambda v: 0.0 <= v < math.inf, "a finite number >= 0")  # the ``ok, what`` of ``number``, as most options want them
POSITIVE = (lambda v: 0.0 < v < math.inf, "a finite number > 0")


def number(train_kwargs, name, default, ok, what):
    """``train_kwargs[name]`` (or ``default``) as a float: an int or a float, no bool, for which ``ok(float(v))`` holds.  With the
    default None, None is a value too (the option is off) and comes back as it is."""
    v = train_kwargs.get(name, default)
    if v is None and default is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not ok(float(v)):
        raise ValueError(f"train_kwargs['{name}'] must be {what}, not {v!r}")
    return float(v)


class StepOption:
    """One optional part of the step, built from ``train_kwargs``.  The trainer forwards the names in ``FORWARDED`` to the object as
    properties and calls every hook below on every option, in table order; an option overrides what it needs."""

    FORWARDED = ()  # the options and the state the trainer forwards by name
    active = False

    def begin_step(self, trainer):
        """Before anything of the step is queued."""

    def check_reducer(self, reducer):
        """``configure_optimizers``: raise here if the option cannot run under this data-parallel reducer."""

    def state_dict(self):
        """The option's entries of the checkpoint."""
        return {}

    def load_state_dict(self, ckpt, device):
        """Takes the option's entries out of the checkpoint ``ckpt``; ``device``: the model's GPU, or None."""


class LogitTerm(StepOption):
    """A term on the two main heads' logits.  Once the cross-modal terms are formed the step calls ``terms(logits_2d, logits_3d,
    first_row)`` of every active one, in table order, then ``add(logs, stage, loss_2d, loss_3d, terms)`` of those that returned
    something: it logs them under ``stage`` and returns the two branch losses with them added."""

    # True: ``terms`` gets the [source | target] rows and the number of source rows; False: in the two-call pass the target call's
    # logits alone, with ``first_row`` 0
    READS_SOURCE = False

    def terms(self, logits_2d, logits_3d, first_row):
        return None

    def add(self, logs, stage, loss_2d, loss_3d, terms):
        return loss_2d, loss_3d
