"""Host checks of the self-training options (train_kwargs["lambda_pl"], ["pseudo_labels"]) and of the C ABI of the two-segment
cross entropy (include/mm2d3d.h mm_ce2_*).  The options live in mm2d3d_amd/selftrain.py; the trainer forwards them.  No GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _trainer(**kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": torch.nn.Linear(2, 2), "3d_net": torch.nn.Linear(2, 2)}, None, Loss("cross_entropy"), dict(gc_freeze=False, **kw))


def test_constructor_checks_the_two_options():
    tm = _trainer()
    assert tm.lambda_pl == 0.0 and tm.pseudo_labels == "own"
    tm = _trainer(lambda_pl=0.25, pseudo_labels="ensemble")
    assert tm.lambda_pl == 0.25 and tm.pseudo_labels == "ensemble"
    with pytest.raises(ValueError, match="lambda_pl"):
        _trainer(lambda_pl=-0.1)
    with pytest.raises(ValueError, match="lambda_pl"):
        _trainer(lambda_pl=float("nan"))
    with pytest.raises(ValueError, match="pseudo_labels"):
        _trainer(pseudo_labels="3d")
    with pytest.raises(ValueError, match="pseudo_labels"):
        _trainer(lambda_pl=1.0, pseudo_labels=None)


def test_pseudo_label_refusals_are_host_checks():
    """Raised from the batch dict alone, before a forward pass: no device is involved."""
    st = _trainer(lambda_pl=1.0).selftrain
    x = [torch.zeros(5, 4, dtype=torch.int64), torch.zeros(5, 3)]
    y = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(KeyError, match="pselab_paths="):
        st.batch_targets({"x": x})
    with pytest.raises(ValueError, match='pseudo_labels="ensemble"'):
        st.batch_targets({"x": x, "pseudo_label_2d": y, "pseudo_label_3d": [], "pseudo_label_ensemble": y})
    with pytest.raises(ValueError, match="5 point rows"):
        st.batch_targets({"x": x, "pseudo_label_2d": y[:4], "pseudo_label_3d": y, "pseudo_label_ensemble": y})
    a, b = st.batch_targets({"x": x, "pseudo_label_2d": y, "pseudo_label_3d": y + 1, "pseudo_label_ensemble": y + 2})
    assert a.value is y and int(b.value[0]) == 1 and a[1:] == b[1:] == (None, None)  # labels alone: no second matrix, no threshold
    ens = _trainer(lambda_pl=1.0, pseudo_labels="ensemble").selftrain
    a, b = ens.batch_targets({"x": x, "pseudo_label_2d": y, "pseudo_label_3d": [], "pseudo_label_ensemble": y + 2})
    assert int(a.value[0]) == 2 and a.value is b.value


def test_the_single_cross_entropy_entry_is_recognised():
    from mm2d3d_amd.losses import Loss

    tm = _trainer()
    assert tm._single_cross_entropy() == (1.0, None)
    w = [1.0, 2.0]
    tm.loss = Loss([{"name": "cross_entropy", "weight": 0.5, "target": "segmentation", "args": {"weight": w}}, {"name": "l1", "target": "depth"}])
    assert tm._single_cross_entropy() == (0.5, w)
    tm.loss = Loss(["cross_entropy", "cross_entropy"])
    assert tm._single_cross_entropy() is None
    tm.loss = Loss([{"name": "l1", "target": "segmentation"}])
    assert tm._single_cross_entropy() is None


def test_header_declares_and_the_binding_matches_the_three_symbols():
    from mm2d3d_amd import _lib

    txt = open(os.path.join(ROOT, "include", "mm2d3d.h")).read()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    ctype = {"const float*": _lib.vp, "float*": _lib.vp, "const int64_t*": _lib.vp, "void*": _lib.vp, "mm_stream_t": _lib.vp, "int": _lib.i32,
             "int64_t": _lib.i64, "size_t": _lib.sz}
    want = {"mm_ce2_ws_bytes": 0, "mm_ce2_fwd": 15, "mm_ce2_bwd": 15}
    for name, n_args in want.items():
        assert hasattr(lib, name), f"{name} is not exported"
        m = re.search(r"\b(int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert m, f"{name} is not declared in include/mm2d3d.h"
        params = [] if m.group(2).strip() == "void" else [" ".join(p.split()[:-1]) for p in m.group(2).split(",")]
        res, args = _lib._PROTOS[name]
        assert res is ctype[m.group(1)] and len(args) == len(params) == n_args, name
        assert args == [ctype[p] for p in params], (name, params)
    L = _lib.lib()
    assert int(L.mm_ce2_ws_bytes()) >= 1024 * 4 * 8
    # argument errors are reported before anything is launched: class count above the limit, split outside [0, N], workspace
    assert L.mm_ce2_fwd(None, 33, 10, 5, 33, None, None, None, None, -100, 2, None, None, 0, None) == -1 and b"ce2" in L.mm_last_error()
    assert L.mm_ce2_fwd(None, 6, 10, 11, 6, None, None, None, None, -100, 2, None, None, 1 << 20, None) == -1 and b"split" in L.mm_last_error()
    assert L.mm_ce2_fwd(None, 6, 10, 5, 6, None, None, None, None, -100, 2, None, None, 16, None) != 0 and b"workspace" in L.mm_last_error()
    assert L.mm_ce2_bwd(None, 6, 10, -1, 6, None, None, None, None, -100, None, None, None, 6, None) == -1 and b"split" in L.mm_last_error()
    assert L.mm_ce2_bwd(None, 6, 10, 5, 6, None, None, None, None, -100, None, None, None, 5, None) == -1
