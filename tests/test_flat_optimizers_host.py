"""Host side of the flat optimisers (mm2d3d_amd/optimizers.py): what ``sgd`` / ``adam`` / ``rmsprop`` / ``adamw`` of the
reference's registry build, their torch-shaped ``param_groups``, schedulers, checkpoints, and the data-parallel reducer on gloo."""
import os
import socket
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn

TORCH = {"sgd": torch.optim.SGD, "adam": torch.optim.Adam, "rmsprop": torch.optim.RMSprop, "adamw": torch.optim.AdamW}
KW = {"sgd": dict(lr=0.02, momentum=0.9, weight_decay=0.05, nesterov=True), "adam": dict(lr=2e-3, betas=(0.8, 0.99), amsgrad=True),
      "rmsprop": dict(lr=3e-3, alpha=0.9, momentum=0.5, centered=True)}


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [nn.Parameter(torch.randn(s, generator=g)) for s in [(3, 2), (5,), (1,), (4, 4)]]


@pytest.mark.parametrize("name", ["sgd", "adam", "rmsprop"])
def test_registry_names_build_flat_optimisers_with_torch_param_groups(name):
    from mm2d3d_amd import optimizers
    from mm2d3d_amd.optimizers import Optimizer

    ps = _params()
    before = [p.detach().clone() for p in ps]
    o, s = Optimizer(name, **KW[name]).build(ps)
    assert s is None
    assert type(o) is {"sgd": optimizers.FlatSGD, "adam": optimizers.FlatAdam, "rmsprop": optimizers.FlatRMSprop}[name]
    (g,) = o.grad_arenas()
    a = o._arenas[0]
    assert g is a["g"] and g.numel() == sum(p.numel() for p in ps) and {"params", "p", "g", "spans", "touched"} <= set(a)
    for p, b, (lo, hi) in zip(ps, before, a["spans"]):
        assert torch.equal(p.detach(), b)
        assert p.data_ptr() == a["p"].data_ptr() + 4 * lo and hi - lo == p.numel()  # a view into the arena
        assert p._mm_sink.data_ptr() == g.data_ptr() + 4 * lo and p._mm_sink.shape == p.shape and p._mm_pending == 0
    ref = TORCH[name](_params(), **KW[name])
    mine, theirs = dict(o.param_groups[0]), dict(ref.param_groups[0])
    mine.pop("params"), theirs.pop("params")
    assert mine == theirs
    assert {k: v for k, v in o.defaults.items()} == {k: v for k, v in ref.defaults.items()}
    # state arenas: only what the hyper-parameters need
    assert a["state"] == {"sgd": ("buf",), "adam": ("m", "v", "vmax"), "rmsprop": ("sq", "gavg", "buf")}[name]
    bare, _ = Optimizer(name).build(_params())
    assert bare._arenas[0]["state"] == {"sgd": (), "adam": ("m", "v"), "rmsprop": ("sq",)}[name]
    with pytest.raises(RuntimeError, match="GPU"):
        o.step()  # the update is a HIP kernel: no CPU fallback


@pytest.mark.parametrize("sched,skw", [("one_cycle", dict(max_lr=0.05, total_steps=10)),
                                       ("cyclic", dict(base_lr=0.001, max_lr=0.01, step_size_up=3)),
                                       ("multi_step_lr", dict(milestones=[2, 5], gamma=0.3))])
@pytest.mark.parametrize("name", ["sgd", "adam", "rmsprop", "adamw"])
def test_torch_schedulers_cycle_lr_and_momentum_as_on_the_torch_class(name, sched, skw):
    from mm2d3d_amd.optimizers import Optimizer

    kw = {"sgd": dict(lr=0.01, momentum=0.9), "adam": dict(lr=0.01), "rmsprop": dict(lr=0.01, momentum=0.8), "adamw": dict(lr=0.01)}[name]
    o, s = Optimizer(name, **kw).set_scheduler(sched, **skw).build(_params())
    r = TORCH[name](_params(), **kw)
    rs = type(s)(r, **skw)
    mom = (lambda grp: grp["betas"][0]) if name in ("adam", "adamw") else (lambda grp: grp["momentum"])
    o._opt_called = True  # (step() is HIP-only: tell the schedulers the optimiser stepped)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for i in range(8):
            assert abs(o.param_groups[0]["lr"] - r.param_groups[0]["lr"]) < 1e-12, i
            assert abs(mom(o.param_groups[0]) - mom(r.param_groups[0])) < 1e-12, i
            s.step(), rs.step()
    if sched != "multi_step_lr":
        assert mom(o.param_groups[0]) != mom(o.defaults) or o.param_groups[0]["lr"] != kw["lr"]  # something did cycle


def test_arguments_that_do_not_apply_raise_and_their_off_values_are_accepted():
    from mm2d3d_amd.optimizers import FlatAdam, FlatAdamW, FlatRMSprop, FlatSGD, Optimizer

    for name in ("sgd", "adam", "rmsprop", "adamw"):
        with pytest.raises(NotImplementedError):
            Optimizer(name, maximize=True).build(_params())
    for name in ("sgd", "adam", "adamw"):
        with pytest.raises(NotImplementedError):
            Optimizer(name, fused=True).build(_params())
    for cls, flag in [(FlatSGD, "foreach"), (FlatSGD, "differentiable"), (FlatAdam, "capturable"), (FlatAdam, "foreach"),
                      (FlatAdamW, "differentiable"), (FlatRMSprop, "capturable"), (FlatRMSprop, "foreach")]:
        with pytest.raises(NotImplementedError):
            cls(_params(), **{flag: True})
    FlatSGD(_params(), foreach=None, fused=None, differentiable=False, maximize=False)
    FlatAdam(_params(), foreach=False, fused=False, capturable=False, differentiable=False)
    FlatRMSprop(_params(), foreach=None, capturable=False, differentiable=False)
    with pytest.raises(ValueError):
        FlatSGD(_params(), nesterov=True)  # torch's rule: Nesterov needs a momentum and zero dampening


def test_flat_adamw_with_amsgrad_builds():
    from mm2d3d_amd.optimizers import FlatAdamW

    o = FlatAdamW(_params(), amsgrad=True)
    assert o._arenas[0]["state"] == ("m", "v", "vmax") and o._arenas[0]["vmax"].shape == o._arenas[0]["p"].shape
    assert FlatAdamW(_params())._arenas[0]["state"] == ("m", "v")
    assert set(FlatAdamW(_params()).state_dict()["flat"][0]) == {"m", "v"}


@pytest.mark.parametrize("name,kw", [("sgd", KW["sgd"]), ("adam", KW["adam"]), ("rmsprop", KW["rmsprop"]),
                                     ("adamw", dict(amsgrad=True)), ("adamw", {})])
def test_state_dict_round_trip_restores_every_state_arena_and_the_step(name, kw):
    from mm2d3d_amd.optimizers import Optimizer

    o, _ = Optimizer(name, **kw).build(_params())
    g = torch.Generator().manual_seed(5)
    a = o._arenas[0]
    assert a["state"]
    for n in a["state"]:
        a[n].copy_(torch.randn(a[n].shape, generator=g))
    o._step = 7
    sd = o.state_dict()
    assert sd["step"] == 7 and set(sd["flat"][0]) == set(a["state"])
    fresh, _ = Optimizer(name, **kw).build(_params(1))
    fresh.load_state_dict(sd)
    assert fresh._step == 7 and fresh._arenas[0]["state"] == a["state"]
    for n in a["state"]:
        assert torch.equal(fresh._arenas[0][n], a[n]) and fresh._arenas[0][n] is not sd["flat"][0][n]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from mm2d3d_amd.ddp import GradAllReducer
        from mm2d3d_amd.optimizers import FlatSGD

        torch.manual_seed(0)  # identical init on every rank
        net = nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))
        opt = FlatSGD(net.parameters(), lr=0.1, momentum=0.9)
        with warnings.catch_warnings():
            warnings.simplefilter("error")  # a flat optimiser does not warn
            red = GradAllReducer([opt], bucket_bytes=300, overlap=False, tail_bytes=100)
        assert len(red.buckets) >= 2
        spans = sorted((b.lo, b.hi) for b in red.buckets)
        assert spans[0][0] == 0 and spans[-1][1] == opt.grad_arenas()[0].numel()
        assert all(spans[i][1] == spans[i + 1][0] for i in range(len(spans) - 1))
        torch.manual_seed(100 + rank)  # different data per rank
        x = torch.randn(5, 8)
        for _ in range(2):
            opt.zero_grad()
            (net(x) ** 2).sum().backward()
            local = opt.grad_arenas()[0].clone()
            red.finish()
            gathered = [torch.zeros_like(local) for _ in range(world)]
            dist.all_gather(gathered, local)
            assert torch.allclose(opt.grad_arenas()[0], sum(gathered), atol=1e-6)
            # ... and averaged by the update kernel's grad_scale
            assert torch.allclose(opt.grad_arenas()[0] * red.grad_scale, sum(gathered) / world, atol=1e-6)
        # a foreign optimiser stays usable, but the reducer says that nothing of it is reduced
        other = nn.Linear(4, 4)
        with pytest.warns(RuntimeWarning, match="NOT all-reduced"):
            red2 = GradAllReducer([torch.optim.SGD(other.parameters(), lr=0.1)], overlap=False)
        assert red2.buckets == []
        q.put((rank, "ok"))
    except BaseException as e:  # pragma: no cover
        import traceback

        q.put((rank, "".join(traceback.format_exception(type(e), e, e.__traceback__))))
    finally:
        dist.destroy_process_group()


def test_flat_sgd_gradients_are_bucketed_and_a_foreign_optimiser_warns_world2_gloo():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=30)
    for rank, msg in res:
        assert msg == "ok", f"rank {rank}: {msg}"
