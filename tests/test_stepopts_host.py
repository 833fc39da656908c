"""Host checks of the option protocol of the training step (mm2d3d_amd/stepopts.py) and of the table that drives it
(train.OPTIONS): property forwarding, the checkpoint's keys, the do-nothing defaults and the shared number check.  No GPU."""
import pytest
import torch

ORDER = ["selftrain", "target_entropy", "alignment", "adversary", "input_style", "dense_xm"]
# what checkpoint() of a trainer without options, optimisers, teacher and loss scale returns, in this order
DEFAULT_CHECKPOINT_KEYS = ["state_dict", "optimizer_states", "lr_schedulers", "global_step", "best_source_iou", "best_target_iou",
                           "best_source_iou_3d", "best_target_iou_3d", "best_source_iou_avg", "best_target_iou_avg"]


def _trainer(**kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, None, Loss("cross_entropy"), dict(gc_freeze=False, **kw))


def test_the_table_builds_the_options_in_order():
    from mm2d3d_amd.stepopts import LogitTerm, StepOption
    from mm2d3d_amd.train import OPTIONS

    tm = _trainer()
    assert [name for name, _ in OPTIONS] == ORDER
    assert [type(o) for o in tm._options] == [cls for _, cls in OPTIONS] and all(isinstance(o, StepOption) for o in tm._options)
    assert all(getattr(tm, name) is o for (name, _), o in zip(OPTIONS, tm._options))
    assert tm._logit_terms == [tm.target_entropy, tm.alignment, tm.adversary] and all(isinstance(o, LogitTerm) for o in tm._logit_terms)
    # who sees the source rows: the alignment and the adversary compare the domains, the entropy terms are the target's alone
    assert [o.READS_SOURCE for o in tm._logit_terms] == [False, True, True]
    assert not any(o.active for o in tm._options)


def test_every_forwarded_name_reads_and_assigns_through_the_trainer():
    from mm2d3d_amd.train import OPTIONS

    tm = _trainer()
    for owner, cls in OPTIONS:
        option = getattr(tm, owner)
        assert cls.FORWARDED, owner
        for name in cls.FORWARDED:
            assert name in vars(option) and name not in vars(tm), (owner, name)
            assert getattr(tm, name) is getattr(option, name), (owner, name)
            token = object()
            setattr(tm, name, token)
            assert getattr(option, name) is token and getattr(tm, name) is token and name not in vars(tm), (owner, name)


def test_no_name_is_claimed_by_two_options():
    from mm2d3d_amd.train import OPTIONS

    names = [name for _, cls in OPTIONS for name in cls.FORWARDED]
    assert len(names) == len(set(names))
    assert not set(names) & set(vars(_trainer())) and not set(names) & set(ORDER)


def test_the_default_checkpoint_has_the_keys_it_always_had():
    assert list(_trainer().checkpoint()) == DEFAULT_CHECKPOINT_KEYS
    # options that are on but have built no state yet add nothing either
    on = _trainer(ema_decay=0.9, lambda_pl=1.0, pseudo_label_source="teacher", pl_threshold="adaptive", lambda_adv=0.5)
    assert list(on.checkpoint()) == DEFAULT_CHECKPOINT_KEYS
    on.load_checkpoint(on.checkpoint())
    assert on.pl_adaptive is None and not on.adversary.built


def test_an_option_that_overrides_nothing_is_inert():
    from mm2d3d_amd.stepopts import LogitTerm, StepOption

    class Nothing(StepOption):
        pass

    class NoTerm(LogitTerm):
        pass

    tm = _trainer()
    for option in (Nothing(), NoTerm()):
        assert option.FORWARDED == () and not option.active and option.state_dict() == {}
        assert option.begin_step(tm) is None and option.check_reducer(None) is None and option.load_state_dict({"x": 1}, None) is None
        assert vars(option) == {}
    a, b, logs = torch.tensor(1.0), torch.tensor(2.0), {}
    term = NoTerm()
    assert not term.READS_SOURCE and term.terms(None, None, 0) is None
    out = term.add(logs, "train", a, b, None)
    assert out[0] is a and out[1] is b and logs == {}


def test_the_number_check():
    from mm2d3d_amd.stepopts import NON_NEGATIVE, POSITIVE, number

    assert number({}, "w", 0.0, *NON_NEGATIVE) == 0.0 and number({"w": 2}, "w", 0.0, *NON_NEGATIVE) == 2.0
    assert isinstance(number({"w": 2}, "w", 0.0, *NON_NEGATIVE), float)
    assert number({}, "w", None, *POSITIVE) is None and number({"w": None}, "w", None, *POSITIVE) is None  # None by default: "off"
    for bad in (True, "1", -0.5, float("nan"), float("inf"), [1.0], None):
        with pytest.raises(ValueError, match=r"train_kwargs\['w'\] must be a finite number >= 0, not "):
            number({"w": bad}, "w", 0.0, *NON_NEGATIVE)
    with pytest.raises(ValueError, match=r"train_kwargs\['w'\] must be a finite number > 0, not 0"):
        number({"w": 0}, "w", 1.0, *POSITIVE)
    with pytest.raises(ValueError, match=r"train_kwargs\['w'\] must be below one, not 1.5"):
        number({"w": 1.5}, "w", None, lambda v: v < 1.0, "below one")
