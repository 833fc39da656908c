"""Mean-teacher weights on the GPU: the kernels of csrc/optim.hip through the C ABI (mm_ema_update / mm_ema_swap), their gating by
the device-side decision of the optimiser step, mm2d3d_amd/ema.py WeightEMA and train_kwargs["ema_decay"] / ["ema_eval"].

Error bound of every comparison with the float64 recurrence  e <- decay_t * e + (1 - decay_t) * p : ``8 * K * 2**-24 * M`` after K
updates, M = the largest magnitude among all p and the initial e.  An update rounds at most three times in fp32 (d = p - e, w * d,
the sum), each on a magnitude <= 2 M, i.e. by <= 2**-24 M each; w = (float)(1 - decay_t) is off by <= 2**-25 relative, on |d| <= 2 M;
decay_t < 1 never amplifies what earlier updates left.  That is 4 * 2**-24 * M per update, 8 with slack for contraction."""
import copy

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = [4099, 1, 3, 0, 4, 5, 64, 1023, 1025, 0]  # per row; the first stands alone in the nrows = 1 case
UNALIGNED = 8  # this row's two tensors start one float past a 16-byte boundary: the element-by-element path, over two workgroups
GUARD = 8  # floats after every row that no kernel may touch


def _dev():
    import mm2d3d_amd  # noqa: F401

    return torch.device("cuda:0")


def _bound(K, *arrays):
    M = max(float(np.abs(np.asarray(a, dtype=np.float64)).max()) for a in arrays if np.asarray(a).size)
    return 8 * K * 2.0 ** -24 * M


def _bits(t):
    t = t.detach().contiguous().reshape(-1)
    return (t.view(torch.int32) if t.dtype == torch.float32 else t).cpu()


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


class _Rows:
    """Two flat buffers (teacher, live) with the rows of LENGTHS at 16-byte aligned offsets (one of them one float past), guard
    words between them, and the device table of include/mm2d3d.h."""

    def __init__(self, dev, seed=0):
        from mm2d3d_amd import _lib

        self.L = _lib.lib()
        assert int(self.L.mm_ema_row_bytes()) == 32
        g = torch.Generator().manual_seed(seed)
        self.g = g
        offs, off = [], 0
        for i, n in enumerate(LENGTHS):
            off = (off + 3) // 4 * 4 + (1 if i == UNALIGNED else 0)
            offs.append(off)
            off += n + GUARD
        self.offs, total = offs, off
        self.e = torch.randn(total, generator=g).to(dev)
        self.p = torch.randn(total, generator=g).to(dev)
        assert self.e.data_ptr() % 16 == 0 and self.p.data_ptr() % 16 == 0
        self.inside = torch.zeros(total, dtype=torch.bool)
        rows, first = np.zeros((len(LENGTHS), 4), dtype=np.int64), 0
        for i, (o, n) in enumerate(zip(offs, LENGTHS)):
            self.inside[o : o + n] = True
            rows[i] = (self.e.data_ptr() + 4 * o, self.p.data_ptr() + 4 * o, n, first)
            first += -(-n // 1024)
        assert rows[UNALIGNED, 0] % 16 == 4 and rows[UNALIGNED, 1] % 16 == 4 and all(rows[i, 0] % 16 == 0 for i in range(len(LENGTHS)) if i != UNALIGNED)
        self.rows = rows
        self.table = torch.from_numpy(rows.view(np.uint8).reshape(-1).copy()).to(dev)
        self.dev = dev

    def blocks(self, nrows):
        return int(sum(-(-n // 1024) for n in LENGTHS[:nrows]))

    def covered(self, nrows):
        m = torch.zeros_like(self.inside)
        for o, n in list(zip(self.offs, LENGTHS))[:nrows]:
            m[o : o + n] = True
        return m

    def new_p(self):
        self.p.copy_(torch.randn(self.p.numel(), generator=self.g))

    def update(self, nrows, decay, warmup=0, t_host=0, step=None, coef=None, skip=None):
        from mm2d3d_amd._lib import check, ptr, stream

        check(self.L.mm_ema_update(ptr(self.table), nrows, self.blocks(nrows), decay, warmup, t_host, ptr(step), ptr(coef), ptr(skip),
                                   0 if skip is None else skip.numel(), stream()), "ema_update")

    def swap(self, nrows):
        from mm2d3d_amd._lib import check, ptr, stream

        check(self.L.mm_ema_swap(ptr(self.table), nrows, self.blocks(nrows), stream()), "ema_swap")


@pytest.mark.parametrize("nrows", [1, len(LENGTHS)], ids=["one_row", "all_rows"])
def test_kernel_follows_the_float64_recurrence_and_stays_inside_its_rows(nrows):
    K, decay = 5, 0.9
    r = _Rows(_dev())
    e0 = r.e.clone()
    ref = e0.cpu().double().numpy()
    cov = r.covered(nrows).numpy()
    seen = [e0.cpu().numpy()]
    for _ in range(K):
        r.new_p()
        p_before = r.p.clone()
        r.update(nrows, decay)
        assert _same_bits(r.p, p_before)  # the live side is read only
        p = r.p.cpu().double().numpy()
        seen.append(p)
        ref[cov] = decay * ref[cov] + (1.0 - decay) * p[cov]
    got = r.e.cpu().double().numpy()
    bound = _bound(K, *seen)
    err = np.abs(got - ref)[cov].max()
    print(f"nrows {nrows}: max |e - float64 recurrence| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    for o, n in list(zip(r.offs, LENGTHS))[:nrows]:
        assert n == 0 or not torch.equal(r.e[o : o + n], e0[o : o + n]), (o, n)
    # guard words, and with nrows = 1 every other row: bit-identical
    assert _same_bits(r.e[~torch.from_numpy(cov)], e0[~torch.from_numpy(cov)])


def test_kernel_is_exact_at_both_ends():
    r = _Rows(_dev(), seed=1)
    n = len(LENGTHS)
    # p == e leaves e bit-identical
    r.p.copy_(r.e)
    e0 = r.e.clone()
    r.update(n, 0.9)
    r.update(n, 0.3)  # w >= 0.5: the other branch of lerp
    assert _same_bits(r.e, e0)
    # decay = 0 makes e the bits of p, inside the rows only
    r.new_p()
    r.update(n, 0.0)
    inside = r.inside
    assert _same_bits(r.e[inside], r.p[inside]) and _same_bits(r.e[~inside], e0[~inside])
    # ... and with warm-up the decay is min(decay, (1 + t) / (10 + t)): still 0
    r.new_p()
    r.update(n, 0.0, warmup=1, t_host=5)
    assert _same_bits(r.e[inside], r.p[inside]) and _same_bits(r.e[~inside], e0[~inside])


def test_kernel_warmup_reads_the_host_or_the_device_counter():
    dev = _dev()
    n = len(LENGTHS)
    res = []
    for step in (None, torch.tensor([3], dtype=torch.int64, device=dev)):
        r = _Rows(dev, seed=2)
        e0 = r.e.cpu().double().numpy()
        r.update(n, 0.999, warmup=1, t_host=3 if step is None else 1000, step=step)  # the device counter wins when given
        ref = e0 + (1.0 - 4.0 / 13.0) * (r.p.cpu().double().numpy() - e0)
        m = r.inside.numpy()
        assert np.abs(r.e.cpu().double().numpy() - ref)[m].max() <= _bound(1, e0, r.p.cpu().numpy())
        res.append(r.e.clone())
    assert _same_bits(*res)
    # t large: the decay itself
    r = _Rows(dev, seed=2)
    e0 = r.e.cpu().double().numpy()
    r.update(n, 0.5, warmup=1, t_host=1000)
    ref = e0 + 0.5 * (r.p.cpu().double().numpy() - e0)
    assert np.abs(r.e.cpu().double().numpy() - ref)[r.inside.numpy()].max() <= _bound(1, e0, r.p.cpu().numpy())


def test_kernel_skip_words_and_a_skip_coefficient_row_write_nothing():
    from mm2d3d_amd import _lib

    dev = _dev()
    r = _Rows(dev, seed=3)
    n = len(LENGTHS)
    e0 = r.e.clone()
    r.update(n, 0.9, skip=torch.tensor([0, 0, 7], dtype=torch.int32, device=dev))
    assert _same_bits(r.e, e0)
    nb = int(_lib.lib().mm_optim_coef_bytes())
    coef = torch.zeros(nb // 4, dtype=torch.int32, device=dev)
    coef[8] = 1  # OptCoef::skip (eight floats before it)
    r.update(n, 0.9, coef=coef.view(torch.uint8))
    assert _same_bits(r.e, e0)
    coef[8] = 0
    r.update(n, 0.9, coef=coef.view(torch.uint8), skip=torch.zeros(16, dtype=torch.int32, device=dev))
    assert not torch.equal(r.e[r.inside], e0[r.inside]) and _same_bits(r.e[~r.inside], e0[~r.inside])


def test_kernel_swap_exchanges_contents_inside_the_rows():
    r = _Rows(_dev(), seed=4)
    e0, p0 = r.e.clone(), r.p.clone()
    for nrows in (1, len(LENGTHS)):
        cov = r.covered(nrows)
        r.swap(nrows)
        assert _same_bits(r.e[cov], p0[cov]) and _same_bits(r.p[cov], e0[cov])
        assert _same_bits(r.e[~cov], e0[~cov]) and _same_bits(r.p[~cov], p0[~cov])
        r.swap(nrows)
        assert _same_bits(r.e, e0) and _same_bits(r.p, p0)


# ---------------------------------------------------------------------------------------------- WeightEMA over small optimisers
SHAPES = [(6,), (3, 1), (1,), (1037,), (16, 6), (5000,)]


def _small(dev, seed=11, **kw):
    """A FlatSGD and a FlatAdam over a few parameters each, a batch norm for its buffers, and their teacher."""
    from mm2d3d_amd.ema import WeightEMA
    from mm2d3d_amd.optimizers import FlatAdam, FlatSGD

    g = torch.Generator().manual_seed(seed)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in SHAPES]
    pa = [torch.nn.Parameter(torch.randn(s, generator=g).to(dev)) for s in SHAPES]
    bn = torch.nn.BatchNorm1d(7).to(dev)
    bn.running_mean.copy_(torch.randn(7, generator=g))
    for q in bn.parameters():
        q.requires_grad_(False)  # frozen: in no arena, shared with the student
    osgd, oadam = FlatSGD(ps, lr=0.01, momentum=0.9), FlatAdam(pa, lr=0.01)
    return g, ps, pa, bn, osgd, oadam, WeightEMA([osgd, oadam], bn, **kw)


def _backward(g, params, opts, dev, scale=None):
    for o in opts:
        o.zero_grad()
    loss = sum((p * torch.randn(p.shape, generator=g).to(dev)).sum() for p in params)
    (loss if scale is None else scale(loss)).backward()


def _teacher(ema):
    return [e.clone() for _, _, e in ema._arenas] + [c.clone() for _, _, c in ema._buffers]


def _student(ema):
    return [a["p"].clone() for _, a, _ in ema._arenas] + [b.clone() for _, b, _ in ema._buffers]


def _frozen(ema, snap):
    return all(_same_bits(a, b) for a, b in zip(_teacher(ema), snap))


def test_teacher_is_a_copy_with_its_own_memory():
    _, ps, pa, bn, osgd, oadam, ema = _small(_dev(), decay=0.9)
    assert len(ema._arenas) == 2 and [k for k, _, _ in ema._buffers] == ["running_mean", "running_var"]
    assert ema._nrows == 4 and ema._table.numel() == 4 * 32
    for t, s in zip(_teacher(ema), _student(ema)):
        assert _same_bits(t, s)
    own = {e.data_ptr() for _, _, e in ema._arenas} | {c.data_ptr() for _, _, c in ema._buffers}
    assert not own & ({a["p"].data_ptr() for _, a, _ in ema._arenas} | {b.data_ptr() for _, b, _ in ema._buffers})
    t = ema.teacher_state_dict()
    assert t["weight"].data_ptr() != bn.weight.data_ptr() and torch.equal(t["weight"], bn.weight)
    assert t["num_batches_tracked"].dtype == torch.int64


def test_a_nonzero_skip_word_leaves_every_teacher_tensor_as_it_is():
    dev = _dev()
    g, ps, pa, bn, osgd, oadam, ema = _small(dev, decay=0.9)
    for a in (osgd._arenas[0], oadam._arenas[0]):
        a["p"].add_(1.0)
    bn.running_mean.add_(1.0), bn.running_var.add_(1.0)
    snap = _teacher(ema)
    ema.update(skip_words=torch.tensor([0, 3], dtype=torch.int32, device=dev))
    assert _frozen(ema, snap)
    ema.update(skip_words=torch.zeros(2, dtype=torch.int32, device=dev))
    for t, s0 in zip(_teacher(ema), snap):
        assert not torch.equal(t, s0)
        assert torch.allclose(t, s0 + 0.1, rtol=0, atol=1e-5)


def test_an_overflow_skips_the_teacher_too_and_the_next_taken_step_is_step_one():
    from mm2d3d_amd.amp import GradScaler

    dev = _dev()
    g, ps, pa, bn, osgd, oadam, ema = _small(dev, decay=0.999, warmup=True)
    sc = GradScaler(dev, init_scale=1024.0)
    _backward(g, ps + pa, [osgd, oadam], dev, sc.scale)
    oadam.grad_arenas()[0][1500] = float("inf")
    bn.running_mean.add_(0.5)  # the forward pass of a skipped step moves the buffers all the same
    snap, before = _teacher(ema), _student(ema)
    sc.step_all([osgd, oadam])
    sc.update()
    ema.update()
    assert sc.steps_taken(osgd) == 0 and osgd.gate_coef() is not None and torch.is_tensor(osgd.step_counter())
    assert all(_same_bits(a, b) for a, b in zip(_student(ema), before))  # the step itself was skipped
    assert _frozen(ema, snap)
    _backward(g, ps + pa, [osgd, oadam], dev, sc.scale)
    sc.step_all([osgd, oadam])
    sc.update()
    ema.update()
    assert sc.steps_taken(osgd) == 1 and sc.steps_taken(oadam) == 1
    # t = 1: decay_t = min(0.999, 2 / 11)
    for t, e0, p in zip(_teacher(ema), snap, _student(ema)):
        e0, p = e0.cpu().double().numpy(), p.cpu().double().numpy()
        ref = (2.0 / 11.0) * e0 + (9.0 / 11.0) * p
        assert np.abs(t.cpu().double().numpy() - ref).max() <= _bound(1, e0, p)
    assert not _same_bits(ema._arenas[0][2], snap[0])


@pytest.mark.parametrize("how", ["loss_scaled", "skip_words"])
def test_warmup_counts_the_steps_that_were_taken(how):
    """Four steps of which the second is skipped on the device: the float64 recurrence with (1 + t) / (10 + t) for t = 1, 2, 3
    over the three taken ones.  A host-side count would use t = 1 .. 4 and average the skipped step in."""
    from mm2d3d_amd.amp import GradScaler

    dev = _dev()
    g, ps, pa, bn, osgd, oadam, ema = _small(dev, seed=5, decay=0.999, warmup=True)
    sc = GradScaler(dev, init_scale=1024.0) if how == "loss_scaled" else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ref = [t.cpu().double().numpy() for t in _teacher(ema)]
    seen = [r.copy() for r in ref]
    t = 0
    for i in range(4):
        skipped = i == 1
        _backward(g, ps + pa, [osgd, oadam], dev, sc.scale if sc else None)
        bn.running_mean.add_(0.25), bn.running_var.mul_(1.5)
        if sc:
            if skipped:
                osgd.grad_arenas()[0][3] = float("nan")
            sc.step_all([osgd, oadam])
            sc.update()
            ema.update()
        else:
            flag.fill_(int(skipped))
            osgd.step(skip_words=flag), oadam.step(skip_words=flag)
            ema.update(skip_words=flag)
        if skipped:
            continue
        t += 1
        d = min(0.999, (1.0 + t) / (10.0 + t))
        for r, s in zip(ref, _student(ema)):
            s = s.cpu().double().numpy()
            seen.append(s)
            r[...] = d * r + (1.0 - d) * s
    assert t == 3 and int(osgd.step_counter().item()) == 3
    bound = _bound(3, *seen)
    for r, got in zip(ref, _teacher(ema)):
        err = np.abs(got.cpu().double().numpy() - r).max()
        print(f"{how}: max |teacher - float64 recurrence| = {err:.3e}, bound {bound:.3e}")
        assert err <= bound


def test_plain_steps_use_the_host_counter():
    dev = _dev()
    g, ps, pa, bn, osgd, oadam, ema = _small(dev, seed=6, decay=0.999, warmup=True)
    e0 = [t.cpu().double().numpy() for t in _teacher(ema)]
    _backward(g, ps + pa, [osgd, oadam], dev)
    osgd.step(), oadam.step()
    assert osgd.gate_coef() is None and osgd.step_counter() == 1
    ema.update()
    for t, e, p in zip(_teacher(ema), e0, _student(ema)):
        p = p.cpu().double().numpy()
        assert np.abs(t.cpu().double().numpy() - ((2.0 / 11.0) * e + (9.0 / 11.0) * p)).max() <= _bound(1, e, p)


def test_swap_exchanges_contents_and_never_pointers():
    from mm2d3d_amd import conv2d

    dev = _dev()
    g, ps, pa, bn, osgd, oadam, ema = _small(dev, decay=0.9)
    for _, _, e in ema._arenas:
        e.copy_(torch.randn(e.numel(), generator=g))
    for _, _, c in ema._buffers:
        c.copy_(torch.randn(c.numel(), generator=g))
    teacher, student = _teacher(ema), _student(ema)
    ptrs = [q.data_ptr() for q in ps + pa] + [b.data_ptr() for b in bn.buffers()]
    values = [q.detach().clone() for q in ps + pa]
    epoch = conv2d.PARAM_EPOCH[0]
    ema.swap()
    assert conv2d.PARAM_EPOCH[0] == epoch + 1
    assert all(_same_bits(a, b) for a, b in zip(_student(ema), teacher))  # p holds the old teacher bits
    assert all(_same_bits(a, b) for a, b in zip(_teacher(ema), student))  # and the teacher's arrays the old weights
    assert [q.data_ptr() for q in ps + pa] + [b.data_ptr() for b in bn.buffers()] == ptrs
    assert _same_bits(ps[3], teacher[0][10:1047].view(1037))  # a parameter is a view: it sees the teacher's values
    ema.swap()
    assert conv2d.PARAM_EPOCH[0] == epoch + 2
    assert all(_same_bits(a, b) for a, b in zip(_student(ema), student)) and all(_same_bits(a, b) for a, b in zip(_teacher(ema), teacher))
    assert all(_same_bits(q, v) for q, v in zip(ps + pa, values))
    # applied(): the teacher inside, the student back afterwards - also when the body raises
    with ema.applied():
        assert all(_same_bits(a, b) for a, b in zip(_student(ema), teacher))
    assert all(_same_bits(a, b) for a, b in zip(_student(ema), student))
    with pytest.raises(ZeroDivisionError):
        with ema.applied():
            assert _same_bits(bn.running_mean, teacher[2])
            with ema.applied():  # re-entrant: the inner context does not swap the student back in
                assert all(_same_bits(a, b) for a, b in zip(_student(ema), teacher))
            assert all(_same_bits(a, b) for a, b in zip(_student(ema), teacher))
            1 / 0
    assert all(_same_bits(a, b) for a, b in zip(_student(ema), student)) and all(_same_bits(a, b) for a, b in zip(_teacher(ema), teacher))
    assert conv2d.PARAM_EPOCH[0] == epoch + 6 and [q.data_ptr() for q in ps + pa] == ptrs[: len(ps + pa)]


# ---------------------------------------------------------------------------------------------- the trainer
W = [1.9241476, 1.0, 2.16763851, 2.78254323, 1.54875664, 1.85686537]
NET3D = dict(in_channels=3, m=16, full_scale=4096, num_planes=7)
CE = [{"name": "cross_entropy", "target": "segmentation", "args": {"weight": W}}]
STEPS, DECAY = 3, 0.9


def _nets(dev=None, seed=0):
    from mm2d3d_amd.net2d import Net2DSeg
    from mm2d3d_amd.net3d import Net3DSeg

    torch.manual_seed(seed)
    n2, n3 = Net2DSeg(6, pretrained=False), Net3DSeg(6, True, NET3D)
    for m in n2.modules():  # dropout is random: off, for parity between the sides
        if isinstance(m, torch.nn.Dropout):
            m.p = 0.0
    return (n2, n3) if dev is None else (n2.to(dev), n3.to(dev))


def _batch(dev):
    """1 + 1 scenes with 48x64 images."""
    from mm2d3d_amd.synthetic import make_batch

    return {"source": make_batch(5, 1, "nuscenes", (48, 64), device=dev), "target": make_batch(6, 1, "nuscenes", (48, 64), device=dev)}


def _trainer(n2, n3, cfg=CE, **kw):
    from mm2d3d_amd.losses import Loss
    from mm2d3d_amd.optimizers import Optimizer
    from mm2d3d_amd.train import TrainModel

    return TrainModel({"2d_net": n2, "3d_net": n3}, {k: Optimizer("adamw", lr=1e-3) for k in ("2d_net", "3d_net")}, Loss(cfg),
                      dict(lambda_xm_src=1.0, lambda_xm_trg=0.1, gc_freeze=False, precision="fp16", **kw))


def _state(tm):
    return {k: v.detach().clone() for k, v in tm.model.state_dict().items()}


def _logs(tm):
    return {k: float(v.detach()) for k, v in tm.last_logs.items()}


@pytest.fixture(scope="module")
def runs():
    """Three fit_steps of a trainer with a teacher and of one without, same seed, default fp16 precision: computed once."""
    from mm2d3d_amd import nn2d, scn

    dev = _dev()
    try:
        n2, n3 = _nets(dev)
        fresh = (copy.deepcopy(n2), copy.deepcopy(n3)), (copy.deepcopy(n2), copy.deepcopy(n3)), (copy.deepcopy(n2), copy.deepcopy(n3))
        plain_nets = copy.deepcopy(n2), copy.deepcopy(n3)
        tm = _trainer(n2, n3, ema_decay=DECAY, ema_eval=True)
        assert tm.ema is None
        tm.configure_optimizers()
        out = dict(dev=dev, tm=tm, fresh=fresh, start=_state(tm), teacher0={k: v.clone() for k, v in tm.ema.teacher_state_dict().items()},
                   snaps=[], taken=[], logs=[], losses=[])
        for _ in range(STEPS):
            out["losses"].append(float(tm.fit_step(_batch(dev)).detach()))
            out["logs"].append(_logs(tm))
            out["snaps"].append(_state(tm))
            out["taken"].append(int(tm.optimizers[0].step_counter().item()))
        out["teacher"] = tm.ema.teacher_state_dict()
        plain = _trainer(*plain_nets)
        out["plain_losses"], out["plain_logs"] = [], []
        for _ in range(STEPS):
            out["plain_losses"].append(float(plain.fit_step(_batch(dev)).detach()))
            out["plain_logs"].append(_logs(plain))
        out["plain"], out["plain_state"] = plain, _state(plain)
        torch.cuda.synchronize()
        yield out
    finally:
        nn2d.set_precision(nn2d.DEFAULT_PRECISION)
        scn.set_activation_dtype(torch.float32)


def test_trainer_teacher_follows_the_recurrence_over_the_taken_steps(runs):
    tm = runs["tm"]
    assert tm.ema is not None and tm.ema.decay == DECAY and not tm.ema.warmup
    assert tm.scaler is not None  # fp16: the loss scale decides on the device which steps happen
    for k, v in runs["teacher0"].items():
        assert _same_bits(v, runs["start"][k]), k  # the teacher starts as a copy
    ref = {k: v.cpu().double().numpy() for k, v in runs["teacher0"].items() if v.dtype.is_floating_point}
    seen = {k: [float(np.abs(v).max()) if v.size else 0.0] for k, v in ref.items()}
    tracked = {k for k, v in tm.model.state_dict(keep_vars=True).items() if v.dtype.is_floating_point}
    done = 0
    for snap, taken in zip(runs["snaps"], runs["taken"]):
        if taken == done:
            continue  # skipped on the device: not averaged in
        assert taken == done + 1
        done = taken
        for k in ref:
            s = snap[k].cpu().double().numpy()
            seen[k].append(float(np.abs(s).max()) if s.size else 0.0)
            ref[k] = DECAY * ref[k] + (1.0 - DECAY) * s
    print(f"steps taken: {runs['taken']}")
    assert done >= 1 and set(ref) == tracked
    M = max(max(v) for v in seen.values())
    bound = 8 * done * 2.0 ** -24 * M
    worst, moved = 0.0, 0
    for k, r in ref.items():
        got = runs["teacher"][k].cpu().double().numpy()
        if r.size:
            worst = max(worst, float(np.abs(got - r).max()))
            moved += int(not np.array_equal(got, runs["teacher0"][k].cpu().double().numpy()))
    print(f"max |teacher - float64 recurrence| = {worst:.3e}, bound {bound:.3e} (M = {M:.3f}); tensors that moved: {moved} of {len(ref)}")
    assert worst <= bound
    assert moved > len(ref) // 2
    # and it is not the student: the last snapshot differs from the teacher
    last = runs["snaps"][-1]
    assert sum(int(not torch.equal(runs["teacher"][k], last[k])) for k in ref) > len(ref) // 2
    # integer buffers are the student's
    for k, v in runs["teacher"].items():
        if not v.dtype.is_floating_point:
            assert torch.equal(v, last[k]), k


def test_trainer_training_is_unchanged_by_the_teacher(runs):
    assert runs["plain"].ema is None
    assert runs["losses"] == runs["plain_losses"]
    assert runs["logs"] == runs["plain_logs"] and len(runs["logs"][0]) >= 6
    last = runs["snaps"][-1]
    assert list(last) == list(runs["plain_state"])
    for k, v in runs["plain_state"].items():
        assert _same_bits(v, last[k]) if v.dtype.is_floating_point else torch.equal(v, last[k]), k
    assert int(runs["plain"].optimizers[0].state_dict()["step"]) == runs["taken"][-1]


def test_trainer_ema_eval_predicts_with_the_teacher_and_gives_the_student_back(runs):
    dev, tm = runs["dev"], runs["tm"]
    batch = lambda: _batch(dev)["target"]  # seeded: the same scenes every time (the 3D net gates the features in place)
    before = _state(tm)
    ptrs = [p.data_ptr() for p in tm.model.parameters()]
    got = tm.predict_step(batch())
    after = _state(tm)
    tm.model.train()
    assert list(before) == list(after) and [p.data_ptr() for p in tm.model.parameters()] == ptrs
    for k, v in before.items():
        assert _same_bits(v, after[k]) if v.dtype.is_floating_point else torch.equal(v, after[k]), k
    ck = tm.checkpoint()
    assert set(ck["ema_state_dict"]) == set(ck["state_dict"]) and all(k.startswith("model.") and ".model." in k for k in ck["ema_state_dict"])
    loaded = _trainer(*runs["fresh"][0])
    loaded.load_checkpoint({"state_dict": ck["ema_state_dict"]})
    want = loaded.predict_step(batch())
    student = _trainer(*runs["fresh"][1])
    student.load_checkpoint({"state_dict": ck["state_dict"]})
    other = student.predict_step(batch())
    torch.cuda.synchronize()
    assert list(got) == list(want) and len(got) == 6
    for k in got:
        assert _same_bits(got[k], want[k]) if got[k].dtype.is_floating_point else torch.equal(got[k], want[k]), k
    # the teacher is not the student: the probabilities differ somewhere
    assert any(k.startswith("probs") and not torch.equal(got[k], other[k]) for k in got)
    # validation runs under the teacher too and leaves the student alone
    tm.validation_step(_batch(dev)["source"])
    tm.model.train()
    for k, v in before.items():
        assert torch.equal(v, _state(tm)[k]), k


def test_trainer_checkpoint_round_trip_and_a_checkpoint_without_a_teacher(runs):
    dev, tm = runs["dev"], runs["tm"]
    ck = tm.checkpoint()
    assert set(ck["ema"]) == {"decay", "warmup", "arenas", "buffers"}
    other = _trainer(*runs["fresh"][2], ema_decay=0.5, ema_warmup=True)
    other.load_checkpoint(ck)
    assert other.ema.decay == DECAY and other.ema.warmup is False
    for (k, a), (_, b) in zip(tm.ema.teacher_state_dict().items(), other.ema.teacher_state_dict().items()):
        assert torch.equal(a, b), k
    la, lb = float(tm.fit_step(_batch(dev)).detach()), float(other.fit_step(_batch(dev)).detach())
    torch.cuda.synchronize()
    assert la == lb
    ta, tb = tm.ema.teacher_state_dict(), other.ema.teacher_state_dict()
    assert list(ta) == list(tb)
    for k in ta:
        assert _same_bits(ta[k], tb[k]) if ta[k].dtype.is_floating_point else torch.equal(ta[k], tb[k]), k
    assert any(not torch.equal(ta[k], v) for k, v in runs["teacher"].items())  # the step moved the teacher
    # a checkpoint without "ema": the teacher restarts from the loaded weights
    bare = {k: v for k, v in ck.items() if k not in ("ema", "ema_state_dict")}
    other.load_checkpoint(bare)
    strip = lambda k: k[len("model."):].replace(".model.", ".", 1)
    loaded = {strip(k): v for k, v in bare["state_dict"].items()}
    t = other.ema.teacher_state_dict()
    assert set(t) == set(loaded)
    for k, v in loaded.items():
        assert torch.equal(t[k], v), k
