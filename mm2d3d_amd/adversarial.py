"""Adversarial alignment in the output space of the two-domain step (train.py): everything ``train_kwargs["lambda_adv"]`` and
``["adv_*"]`` switch on, in one policy object that also owns the two discriminators and their optimisers."""
import math

import torch

from .losses import ADV_HIDDEN, ADV_MODES, adversarial, adversarial_param_count
from .stepopts import NON_NEGATIVE, LogitTerm, number


def initial_parameters(C, hidden, generator):
    """One discriminator's flat fp32 parameters (W1 [H][C], b1, W2 [H][H], b2, w3, b3) by torch's ``nn.Linear`` rule - weights and
    biases uniform in +-1 / sqrt(fan_in) - drawn on the CPU from ``generator`` alone: the global random stream, and with it the
    dropout masks of the step, is what it is without the option."""
    parts = []
    for fan_in, fan_out in ((C, hidden), (hidden, hidden), (hidden, 1)):
        k = 1.0 / math.sqrt(fan_in)
        for n in (fan_out * fan_in, fan_out):  # the weight, then the bias
            parts.append((torch.rand(n, generator=generator, dtype=torch.float64) * 2.0 - 1.0) * k)
    flat = torch.cat(parts).to(torch.float32)
    assert flat.numel() == adversarial_param_count(C, hidden)
    return flat


class OutputAdversary(LogitTerm):
    """With ``lambda_adv`` > 0 each main head gets a discriminator D on its per-point logits - a point-wise MLP (two hidden layers
    of ``adv_hidden`` = 16, 32 or 64 units, LeakyReLU 0.2) that tells source rows from target rows - and the head learns to fool
    it: loss_2d += lambda_adv * loss_g(l2d), the same for 3D, loss_g = the target rows' binary cross entropy against the label
    "source".  ``adv_input``: what D reads, "selfinfo" (default; AdvEnt, Vu et al., CVPR 2019: the weighted self-information
    -p ln p / ln C) or "softmax" (AdaptSegNet, Tsai et al., CVPR 2018).  One ``losses.adversarial`` call per head on the [source |
    target] logits the step already holds produces both losses, D's parameter gradient and the head's gradient (csrc/adv.hip); no
    extra forward of either network.

    D lives outside the two networks.  Each D is ONE flat ``nn.Parameter`` under its own ``FlatAdam`` (``adv_lr``, default 1e-4;
    ``adv_betas``, default (0.9, 0.99), AdaptSegNet's), built at the first call, when C is known, from a private
    ``torch.Generator`` seeded with ``adv_seed``.  ``terms`` steps D AT ONCE with the gradient the kernel reports: the head's
    gradient was formed in the same launch with the weights D had then, so the student's backward does not depend on D's weights
    any more.  D's update goes through neither autograd nor the GradScaler, the reducer, the clip or the EMA, and it is NOT gated by
    the loss-scale skip: D's gradient comes from the forward's logits, which are valid whether or not the student's step is taken
    (the stance ``pl_threshold="adaptive"`` takes for its running statistics).  D is not reduced over ranks: with an active
    data-parallel reducer ``configure_optimizers`` raises, because un-reduced discriminators would diverge across ranks.

    Logged: ``{stage}/adv_g_2d`` / ``_3d`` (loss_g), ``adv_d_2d`` / ``_3d`` (D's loss before its step), ``adv_acc_2d`` / ``_3d``
    (D's accuracy over both domains).  ``last_adversary``: ``{"loss_d", "loss_g", "count", "correct"}``, [2] device tensors, 2D head
    first (count / correct: the counted and the correctly told rows of both domains).  The checkpoint gains "adversary" once D is
    built; loading a checkpoint without it resets D.  Validation, test, ``predict_step`` and the teacher pass never call it.
    ``lambda_adv`` 0.0 (default): nothing is built, called or allocated, no log key appears, the step is launch for launch the
    step without the option.  The other options are validated whatever the weight is."""

    FORWARDED = ("lambda_adv", "adv_input", "adv_hidden", "adv_lr", "adv_betas", "adv_seed", "last_adversary")
    READS_SOURCE = True

    def __init__(self, train_kwargs):
        self.lambda_adv = number(train_kwargs, "lambda_adv", 0.0, *NON_NEGATIVE)
        self.adv_input = train_kwargs.get("adv_input", "selfinfo")
        if not isinstance(self.adv_input, str) or self.adv_input not in ADV_MODES:
            raise ValueError(f"train_kwargs['adv_input'] must be \"selfinfo\" or \"softmax\", not {self.adv_input!r}")
        self.adv_hidden = train_kwargs.get("adv_hidden", 64)
        if isinstance(self.adv_hidden, bool) or not isinstance(self.adv_hidden, int) or self.adv_hidden not in ADV_HIDDEN:
            raise ValueError(f"train_kwargs['adv_hidden'] must be 16, 32 or 64, not {self.adv_hidden!r}")
        self.adv_lr = number(train_kwargs, "adv_lr", 1e-4, *NON_NEGATIVE)
        b = train_kwargs.get("adv_betas", (0.9, 0.99))
        if not isinstance(b, (tuple, list)) or len(b) != 2 or any(
                isinstance(v, bool) or not isinstance(v, (int, float)) or not 0.0 <= float(v) < 1.0 for v in b):
            raise ValueError(f"train_kwargs['adv_betas'] must be two numbers in [0, 1), not {b!r}")
        self.adv_betas = (float(b[0]), float(b[1]))
        self.adv_seed = train_kwargs.get("adv_seed", 0)
        if isinstance(self.adv_seed, bool) or not isinstance(self.adv_seed, int):
            raise ValueError(f"train_kwargs['adv_seed'] must be an integer, not {self.adv_seed!r}")
        self.last_adversary = None
        self.params, self.optimizers, self.classes = None, None, None  # built at the first call

    @property
    def active(self):
        return self.lambda_adv > 0.0

    @property
    def built(self):
        return self.params is not None

    def check_reducer(self, reducer):
        """``configure_optimizers``: the discriminators are not reduced over ranks (known gap)."""
        if self.active and reducer is not None and reducer.active:
            raise RuntimeError("train_kwargs['lambda_adv'] > 0 under an active data-parallel reducer: the discriminators are stepped "
                               "per rank and not reduced, they would diverge across ranks")

    def _build(self, C, device):
        from .optimizers import FlatAdam

        gen = torch.Generator().manual_seed(int(self.adv_seed))
        self.params = [torch.nn.Parameter(initial_parameters(C, self.adv_hidden, gen).to(device)) for _ in range(2)]  # 2D head first
        self.optimizers = [FlatAdam([p], lr=self.adv_lr, betas=self.adv_betas) for p in self.params]
        self.classes = C

    def reset(self):
        self.params, self.optimizers, self.classes = None, None, None

    def step_discriminator(self, i, grad_params):
        """One ``FlatAdam`` step of discriminator ``i`` on ``grad_params``.  The packed 16-bit weight copies of the 2D network are
        keyed to conv2d.PARAM_EPOCH, which every flat step advances; D has no such copy, so the epoch is put back."""
        from . import conv2d as _c2d

        opt = self.optimizers[i]
        opt.grad_arenas()[0].copy_(grad_params)
        opt.mark_all_touched()
        epoch = _c2d.PARAM_EPOCH[0]
        opt.step()
        _c2d.PARAM_EPOCH[0] = epoch

    def terms(self, logits_2d, logits_3d, first_row):
        """``(g2d, g3d)``, loss_g of the two main heads' logits, rows ``[0, first_row)`` source and ``[first_row, N)`` target, and
        one step of each discriminator; None with the weight 0 or outside a train step with gradients enabled."""
        if not self.active or not torch.is_grad_enabled():
            return None
        C = int(logits_2d.shape[1])
        if not self.built:
            self._build(C, logits_2d.device)
        elif C != self.classes:
            raise ValueError(f"adversary: built for {self.classes} classes, the logits have {C}")
        outs = []
        for i, x in enumerate((logits_2d, logits_3d)):
            o = adversarial(x, first_row, self.params[i].data, self.adv_input, self.adv_hidden)
            self.step_discriminator(i, o["grad_params"])  # gx is saved: the student's backward no longer reads D's weights
            outs.append(o)
        self.last_adversary = {"loss_d": torch.stack([o["loss_d"] for o in outs]),
                               "loss_g": torch.stack([o["loss_g"].detach() for o in outs]),
                               "count": torch.stack([o["count"].sum() for o in outs]),
                               "correct": torch.stack([o["correct"].sum() for o in outs])}
        return outs[0]["loss_g"], outs[1]["loss_g"]

    def add(self, logs, stage, loss_2d, loss_3d, terms):
        """Logs the terms of ``stage`` and returns the two branch losses with ``lambda_adv * loss_g`` added."""
        g2, g3 = terms
        last = self.last_adversary
        acc = last["correct"] / last["count"].clamp_min(1)
        logs[f"{stage}/adv_g_2d"], logs[f"{stage}/adv_g_3d"] = g2, g3
        logs[f"{stage}/adv_d_2d"], logs[f"{stage}/adv_d_3d"] = last["loss_d"][0], last["loss_d"][1]
        logs[f"{stage}/adv_acc_2d"], logs[f"{stage}/adv_acc_3d"] = acc[0], acc[1]
        return loss_2d + self.lambda_adv * g2, loss_3d + self.lambda_adv * g3

    # ------------------------------------------------------------------ checkpoints
    def state_dict(self):
        """``{"adversary": ...}`` once the discriminators are built, else nothing."""
        if not self.built:
            return {}
        return {"adversary": {"params": [p.detach().clone() for p in self.params],
                              "optimizers": [o.state_dict() for o in self.optimizers],
                              "C": self.classes, "H": self.adv_hidden, "mode": self.adv_input}}

    def load_state_dict(self, ckpt, device):
        sd = ckpt.get("adversary")
        if sd is None:
            self.reset()  # a checkpoint without discriminators: they start again from the seed
            return
        if sd["H"] != self.adv_hidden or sd["mode"] != self.adv_input:
            raise ValueError(f"checkpoint holds discriminators with hidden = {sd['H']}, input = {sd['mode']!r}; the trainer has "
                             f"{self.adv_hidden}, {self.adv_input!r}")
        self._build(int(sd["C"]), device if device is not None else sd["params"][0].device)
        with torch.no_grad():
            for p, o, v, osd in zip(self.params, self.optimizers, sd["params"], sd["optimizers"]):
                p.copy_(v)
                o.load_state_dict(osd)
