"""Host checks of the mean-teacher weights (mm2d3d_amd/ema.py WeightEMA, train_kwargs["ema_decay"]) and of the C ABI of their
kernels (include/mm2d3d.h mm_ema_*).  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(3, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 2))


def _trainer(**kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, None, Loss("cross_entropy"), dict(gc_freeze=False, **kw))


def test_constructor_refuses_a_bad_decay_and_a_non_flat_optimiser():
    from mm2d3d_amd.ema import WeightEMA
    from mm2d3d_amd.optimizers import FlatSGD

    m = _model()
    flat = FlatSGD(m.parameters(), lr=0.1)
    for bad in (1.0, -0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            WeightEMA([flat], m, bad)
    with pytest.raises(TypeError, match="flat optimiser"):
        WeightEMA([torch.optim.SGD(_model().parameters(), lr=0.1)], m, 0.9)
    with pytest.raises(TypeError, match="flat optimiser"):
        WeightEMA([flat, torch.optim.SGD(_model().parameters(), lr=0.1)], m, 0.9)
    ema = WeightEMA([flat], m, 0.0, warmup=True)  # both ends of the range that is allowed
    assert ema.decay == 0.0 and ema.warmup is True
    assert WeightEMA([flat], m, 0.9999).warmup is False
    # the kernels are HIP only: CPU arenas are refused, not averaged on the host
    with pytest.raises(RuntimeError, match="GPU"):
        ema.update()
    with pytest.raises(RuntimeError, match="GPU"):
        ema.swap()


def test_state_dict_keys_and_what_is_tracked():
    from mm2d3d_amd.ema import WeightEMA
    from mm2d3d_amd.optimizers import FlatAdam, FlatSGD

    m = _model()
    m[2].bias.requires_grad_(False)  # frozen: outside the arenas, shared with the student
    o1, o2 = FlatSGD(m[0].parameters(), lr=0.1), FlatAdam(m[2].parameters(), lr=0.1)
    ema = WeightEMA([o1, o2], m, 0.99, warmup=True)
    sd = ema.state_dict()
    assert set(sd) == {"decay", "warmup", "arenas", "buffers"}
    assert sd["decay"] == 0.99 and sd["warmup"] is True
    assert [t.numel() for t in sd["arenas"]] == [3 * 5 + 5, 5 * 2]
    assert set(sd["buffers"]) == {"1.running_mean", "1.running_var"}  # num_batches_tracked is an integer: shared
    assert torch.equal(sd["arenas"][0], o1._arenas[0]["p"]) and sd["arenas"][0].data_ptr() != o1._arenas[0]["p"].data_ptr()
    t = ema.teacher_state_dict()
    assert list(t) == list(m.state_dict())
    assert all(torch.equal(t[k], v) and t[k].data_ptr() != v.data_ptr() for k, v in m.state_dict().items())
    # a round trip through another instance; a teacher of another shape is refused
    sd["arenas"][0] = sd["arenas"][0] + 1.0
    sd["decay"] = 0.5
    other = WeightEMA([o1, o2], m, 0.9)
    other.load_state_dict(sd)
    assert other.decay == 0.5 and other.warmup is True
    assert torch.equal(other.teacher_state_dict()["0.weight"], m[0].weight + 1.0)
    assert torch.equal(other.teacher_state_dict()["2.bias"], m[2].bias)
    with pytest.raises(ValueError, match="arenas"):
        other.load_state_dict(dict(sd, arenas=sd["arenas"][:1]))
    # a dict of modules prefixes the keys as nn.ModuleDict does
    named = WeightEMA([o1, o2], {"a": m[0], "b": m[1]}, 0.9)
    assert set(named.state_dict()["buffers"]) == {"b.running_mean", "b.running_var"}
    assert set(named.teacher_state_dict()) == {"a.weight", "a.bias", "b.weight", "b.bias", "b.running_mean", "b.running_var", "b.num_batches_tracked"}


def test_the_accessors_of_a_flat_optimiser_before_any_step():
    from mm2d3d_amd.optimizers import FlatAdamW

    o = FlatAdamW(_model().parameters())
    assert o.gate_coef() is None and o.step_counter() == 0
    o.load_state_dict(dict(o.state_dict(), step=7))
    assert o.gate_coef() is None and o.step_counter() == 7


def test_trainer_options():
    tm = _trainer()
    assert tm.ema is None and tm.ema_decay is None and tm.ema_warmup is False and tm.ema_eval is False
    tm = _trainer(ema_decay=None, ema_warmup=True, ema_eval=True)
    assert tm.ema is None
    assert "ema" not in tm.checkpoint() and "ema_state_dict" not in tm.checkpoint()
    tm = _trainer(ema_decay=0.999, ema_warmup=True, ema_eval=True)
    assert tm.ema is None and tm.ema_decay == 0.999 and tm.ema_warmup and tm.ema_eval  # built with the optimisers
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError, match="ema_decay"):
            _trainer(ema_decay=bad)


def test_trainer_builds_the_teacher_with_the_optimisers_and_checkpoints_it():
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    def make(**kw):
        torch.manual_seed(1)
        return TrainModel({"2d_net": _model(), "3d_net": _model()}, {"2d_net": Optimizer("sgd", lr=0.1), "3d_net": Optimizer("adamw", lr=0.1)},
                          Loss("cross_entropy"), dict(gc_freeze=False, **kw))

    plain = make()
    plain.configure_optimizers()
    assert plain.ema is None
    tm = make(ema_decay=0.9, ema_warmup=True)
    tm.configure_optimizers()
    assert tm.ema is not None and tm.ema.decay == 0.9 and tm.ema.warmup and tm.ema.optimizers == tm.optimizers
    ck = tm.checkpoint()
    assert set(ck["ema"]) == {"decay", "warmup", "arenas", "buffers"}
    assert set(ck["ema_state_dict"]) == set(ck["state_dict"]) and "model.2d_net.model.0.weight" in ck["ema_state_dict"]
    assert all(torch.equal(ck["ema_state_dict"][k], v) for k, v in ck["state_dict"].items())
    # "ema" restores the teacher; a checkpoint without it starts the teacher from the loaded weights
    moved = {k: v + 1.0 if v.dtype.is_floating_point else v for k, v in ck["state_dict"].items()}
    other = make(ema_decay=0.9)
    other.load_checkpoint(dict(ck, state_dict=moved))
    assert all(torch.equal(v, ck["state_dict"][k]) for k, v in other.checkpoint()["ema_state_dict"].items())
    assert other.ema.warmup is True
    bare = {k: v for k, v in ck.items() if k not in ("ema", "ema_state_dict")}
    other.load_checkpoint(dict(bare, state_dict=moved))
    assert all(torch.equal(v, moved[k]) for k, v in other.checkpoint()["ema_state_dict"].items())


def test_header_declares_and_the_binding_matches_the_three_symbols():
    from mm2d3d_amd import _lib

    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const void*": _lib.vp, "const int64_t*": _lib.vp, "const int*": _lib.vp, "mm_stream_t": _lib.vp, "int": _lib.i32,
             "int64_t": _lib.i64, "double": _lib.f64}
    want = {"mm_ema_row_bytes": 0, "mm_ema_update": 11, "mm_ema_swap": 4}
    for name, n_args in want.items():
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [] if m.group(1).strip() == "void" else [" ".join(p.split()[:-1]) for p in m.group(1).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is _lib.i32 and len(args) == len(params) == n_args, name
        assert args == [ctype[p] for p in params], (name, params)
    L = _lib.lib()
    assert int(L.mm_ema_row_bytes()) == 32
    # argument errors are reported before anything is launched; an empty table is no error and launches nothing
    assert L.mm_ema_update(None, 0, 0, 0.9, 0, 0, None, None, None, 0, None) == 0
    assert L.mm_ema_swap(None, 0, 0, None) == 0
    assert L.mm_ema_update(None, 1, 1, 0.9, 0, 0, None, None, None, 0, None) == -1 and b"ema" in L.mm_last_error()
    assert L.mm_ema_update(None, 0, 1, 0.9, 0, 0, None, None, None, 0, None) == -1
    assert L.mm_ema_update(None, -1, 0, 0.9, 0, 0, None, None, None, 0, None) == -1
    assert L.mm_ema_update(None, 0, 1 << 31, 0.9, 0, 0, None, None, None, 0, None) == -1
    for decay in (1.0, -0.1, float("nan")):
        assert L.mm_ema_update(None, 0, 0, decay, 0, 0, None, None, None, 0, None) == -1 and b"decay" in L.mm_last_error()
    assert L.mm_ema_update(None, 0, 0, 0.9, 1, -1, None, None, None, 0, None) == -1
    assert L.mm_ema_update(None, 0, 0, 0.9, 0, 0, None, None, None, 1, None) == -1 and b"skip" in L.mm_last_error()
    assert L.mm_ema_update(None, 0, 0, 0.9, 0, 0, None, None, None, 17, None) == -1
    assert L.mm_ema_swap(None, 1, 1, None) == -1 and L.mm_ema_swap(None, 0, -1, None) == -1
