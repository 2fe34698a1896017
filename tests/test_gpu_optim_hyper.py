"""Hyper-parameters that change while captured steps keep replaying: the optimizer entry that reads them on the device
(cgnn_adam_step_dev) against the by-value entry and against torch, optim.Adam / optim.AdamW under replay with a
schedule, and the Trainer's rule for optimizers whose captured launches freeze their values."""
import copy
import functools
import warnings

import pytest
import torch

from connectome_gnn_amd import _lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPES = [(64, 5), (64,), (64, 64), (1,), (300, 7), (2, 32)]          # test_gpu_kernels.test_optim_adam_matches_torch_adam's


# ------------------------------------------------------------------------------------------- 1. the two entries
def _jobs(ps, gs, ms, vs):
    out = []
    for lo in range(0, len(ps), _lib.ADAM_MAX_JOBS):
        jb = _lib.CgnnAdamJobs()
        jb.n = len(ps[lo:lo + _lib.ADAM_MAX_JOBS])
        for i in range(jb.n):
            p, g, m, v = ps[lo + i], gs[lo + i], ms[lo + i], vs[lo + i]
            jb.numel[i] = p.numel()
            jb.param[i], jb.grad[i], jb.exp_avg[i], jb.exp_avg_sq[i] = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr()
        out.append(jb)
    return out


@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("shapes", [[(64, 5), (64,), (1,), (300, 7), (1025,)], [(7,)] * 20 + [(3, 5)] * 13],
                         ids=["five", "thirty-three"])
def test_the_two_entries_give_the_same_bits(shapes, wd):
    """cgnn_adam_step and cgnn_adam_step_dev(decoupled=0) on cloned states: torch.equal parameters and moments after
    each of 5 steps; (1025,) crosses the 1024-element workgroup boundary by one element; 33 parameters are more than
    ADAM_MAX_JOBS, i.e. two launches of which only the last advances the shared counter."""
    torch.manual_seed(0)
    lr, b1, b2, eps = 1e-2, 0.9, 0.999, 1e-8
    ps = [torch.randn(*s, device=DEV) for s in shapes]
    gs = [torch.empty_like(p) for p in ps]
    side = {}
    for name in ("value", "device"):
        st = dict(p=[p.clone() for p in ps], m=[torch.zeros_like(p) for p in ps], v=[torch.zeros_like(p) for p in ps],
                  step=torch.zeros((), device=DEV), arrivals=torch.zeros(1, dtype=torch.int32, device=DEV))
        st["jobs"] = _jobs(st["p"], gs, st["m"], st["v"])
        side[name] = st
    launches = len(side["value"]["jobs"])
    assert launches == (2 if len(shapes) > _lib.ADAM_MAX_JOBS else 1)
    hyper = torch.zeros(_lib.ADAM_HYPER_STRIDE, dtype=torch.float64)
    hyper[:5] = torch.tensor([lr, b1, b2, eps, wd], dtype=torch.float64)
    hyper = hyper.to(DEV)
    for it in range(5):
        for g in gs:
            g.copy_(torch.randn_like(g) * (1.0 + it))
        a, b = side["value"], side["device"]
        for i in range(launches):
            last = int(i == launches - 1)
            _lib.call("cgnn_adam_step", a["jobs"][i], a["step"], a["arrivals"], last, lr, b1, b2, eps, wd)
            _lib.call("cgnn_adam_step_dev", b["jobs"][i], b["step"], b["arrivals"], last, hyper, 0)
        torch.cuda.synchronize()
        assert float(a["step"]) == float(b["step"]) == it + 1.0
        assert int(a["arrivals"]) == int(b["arrivals"]) == 0
        for k in ("p", "m", "v"):
            for x, y in zip(a[k], b[k]):
                assert torch.equal(x, y), (it, k, tuple(x.shape))
    assert not torch.equal(side["value"]["p"][0], ps[0])               # (they did move)


# ------------------------------------------------------------------------------------------- 2. changes under replay
def _replayed(edits: bool):
    """optim.Adam with its step captured once, an eager torch.optim.Adam(capturable=False) beside it on the same
    gradients; with ``edits``, both see StepLR(1, 0.5) for two replays, then weight_decay 0 -> 1e-2, betas
    (0.8, 0.99) and eps 1e-6 by hand, one replay each (torch always sees them).  1 eager + 5 replayed steps."""
    from connectome_gnn_amd.optim import Adam
    torch.manual_seed(0)
    ps_a = [torch.randn(*s, device=DEV).requires_grad_(True) for s in SHAPES]
    ps_b = [p.detach().clone().requires_grad_(True) for p in ps_a]
    for p, q in zip(ps_a, ps_b):
        p.grad, q.grad = torch.zeros_like(p), torch.zeros_like(q)
    oa = Adam(ps_a, lr=1e-2)
    ob = torch.optim.Adam(ps_b, lr=1e-2, capturable=False)
    sa = torch.optim.lr_scheduler.StepLR(oa, step_size=1, gamma=0.5)
    sb = torch.optim.lr_scheduler.StepLR(ob, step_size=1, gamma=0.5)
    it = [0]

    def grads():
        for p, q in zip(ps_a, ps_b):
            g = torch.randn_like(p) * (1.0 + it[0])
            p.grad.copy_(g)
            q.grad.copy_(g)
        it[0] += 1

    grads()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step()
    torch.cuda.current_stream().wait_stream(side)
    ob.step()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        oa.step()
    uploads = 0

    def edit(fn):
        fn(ob)
        if edits:
            fn(oa)

    def by_hand(key, value):
        return lambda opt: opt.param_groups[0].__setitem__(key, value)

    changes = [lambda opt: (sa if opt is oa else sb).step(), lambda opt: (sa if opt is oa else sb).step(),
               by_hand("weight_decay", 1e-2), by_hand("betas", (0.8, 0.99)), by_hand("eps", 1e-6)]
    for change in changes:
        edit(change)
        grads()
        uploads += int(oa.refresh_hyper())          # every replay goes through refresh_hyper()
        g.replay()
        ob.step()
    torch.cuda.synchronize()
    assert float(oa.state[ps_a[0]]["step"]) == 6.0
    assert uploads == (5 if edits else 0)           # one copy per change, nothing when nothing changed
    if edits:
        assert oa.param_groups[0]["lr"] == ob.param_groups[0]["lr"] == 2.5e-3
    return ps_a, ps_b


def test_changes_under_replay_are_followed():
    """Tolerance: test_optim_adam_matches_torch_adam's for 11 steps (this one takes 6).  Without the device table the
    replays keep lr = 1e-2, weight_decay = 0, betas = (0.9, 0.999), eps = 1e-8 and this fails; that the pass is not
    vacuous shows in the run whose optimizer never sees the edits: it ends more than 100 tolerances from torch."""
    ps_a, ps_b = _replayed(edits=True)
    for p, q in zip(ps_a, ps_b):
        torch.testing.assert_close(p, q, rtol=5e-6, atol=1e-7)
    ps_a, ps_b = _replayed(edits=False)
    for p, q in zip(ps_a, ps_b):
        assert bool(((p - q).abs() > 100 * (1e-7 + 5e-6 * q.abs())).any()), tuple(p.shape)


# ------------------------------------------------------------------------------------------- 3. stale table in capture
def test_a_stale_table_during_capture_is_refused():
    from connectome_gnn_amd.optim import Adam
    torch.manual_seed(1)
    ps_a = [torch.randn(*s, device=DEV).requires_grad_(True) for s in SHAPES[:3]]
    ps_b = [p.detach().clone().requires_grad_(True) for p in ps_a]
    for p, q in zip(ps_a, ps_b):
        p.grad = torch.randn_like(p)
        q.grad = p.grad.clone()
    oa, ob = Adam(ps_a, lr=1e-2), torch.optim.Adam(ps_b, lr=1e-2)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        oa.step()
    torch.cuda.current_stream().wait_stream(side)
    ob.step()
    oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 3e-3            # ... and no refresh_hyper()
    before = [p.detach().clone() for p in ps_a]
    g = torch.cuda.CUDAGraph()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                                    # (torch: "The CUDA Graph is empty")
        with pytest.raises(RuntimeError, match="stale while a stream is capturing"):
            with torch.cuda.graph(g):
                oa.step()
    assert not torch.cuda.is_current_stream_capturing()
    torch.cuda.synchronize()
    assert float(oa.state[ps_a[0]]["step"]) == 1.0 and all(torch.equal(p, b) for p, b in zip(ps_a, before))
    oa.step()                                                              # eager: refreshes, then steps with 3e-3
    ob.step()
    torch.cuda.synchronize()
    assert float(oa.state[ps_a[0]]["step"]) == 2.0
    for p, q in zip(ps_a, ps_b):
        torch.testing.assert_close(p, q, rtol=2e-6, atol=1e-7)
    g2 = torch.cuda.CUDAGraph()                                            # and with a fresh table a capture is fine
    with torch.cuda.graph(g2):
        oa.step()
    g2.replay()
    ob.step()
    torch.cuda.synchronize()
    for p, q in zip(ps_a, ps_b):
        torch.testing.assert_close(p, q, rtol=2e-6, atol=1e-7)


def test_which_entry_a_step_goes_through(monkeypatch):
    """A launch that is recorded reads the table (cgnn_adam_step_dev); an eager Adam step carries the same values by
    value (cgnn_adam_step, the shorter launch); AdamW, which only the table entry implements, always reads the table."""
    from connectome_gnn_amd import optim
    names, real = [], _lib.call

    def call(name, *a, **kw):
        names.append(name)
        return real(name, *a, **kw)

    monkeypatch.setattr(_lib, "call", call)
    for cls, eager in ((optim.Adam, "cgnn_adam_step"), (optim.AdamW, "cgnn_adam_step_dev")):
        p = torch.randn(300, 7, device=DEV).requires_grad_(True)
        p.grad = torch.randn_like(p)
        opt = cls([p], lr=1e-2)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            opt.step()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            opt.step()
        g.replay()
        opt.step()
        torch.cuda.synchronize()
        assert names == [eager, "cgnn_adam_step_dev", eager] and float(opt.state[p]["step"]) == 3.0
        del names[:]


# ------------------------------------------------------------------------------------------- 4. AdamW
@pytest.mark.parametrize("wd", [1e-2, 0.0])
def test_optim_adamw_matches_torch_adamw(wd):
    """connectome_gnn_amd.optim.AdamW against torch.optim.AdamW(foreach=False, capturable=False) step for step, with
    test_optim_adam_matches_torch_adam's gradients, tolerances (7 steps: 2e-6 / 1e-7; 11 steps: 5e-6 / 1e-7) and
    checkpoint round trip through torch's format, both ways; three captured replays follow torch."""
    from connectome_gnn_amd.optim import AdamW
    torch.manual_seed(0)
    ps_a = [torch.randn(*s, device=DEV).requires_grad_(True) for s in SHAPES]
    ps_b = [p.detach().clone().requires_grad_(True) for p in ps_a]
    oa = AdamW(ps_a, lr=1e-2, weight_decay=wd)
    ob = torch.optim.AdamW(ps_b, lr=1e-2, weight_decay=wd, foreach=False, capturable=False)
    ps_c, ob2 = None, None
    for it in range(7):
        gs = [torch.randn_like(p) * (1.0 + it) for p in ps_a]
        for p, q, g in zip(ps_a, ps_b, gs):
            p.grad, q.grad = g.clone(), g.clone()
        if ob2 is not None:
            for r, g in zip(ps_c, gs):
                r.grad = g.clone()
            ob2.step()                   # a stock torch AdamW that resumed from OUR checkpoint
        oa.step()
        ob.step()
        if it == 3:
            sd = oa.state_dict()
            steps = [st["step"] for st in sd["state"].values()]
            assert len({t.data_ptr() for t in steps}) == len(steps), "exported step tensors are aliased"
            ps_c = [q.detach().clone().requires_grad_(True) for q in ps_b]
            ob2 = torch.optim.AdamW(ps_c, lr=1e-2, weight_decay=wd)
            ob2.load_state_dict(copy.deepcopy(sd))
            assert float(ob2.state[ps_c[0]]["step"]) == 4.0
            oa.load_state_dict(copy.deepcopy(ob.state_dict()))
    for p, q in zip(ps_a, ps_b):
        torch.testing.assert_close(p, q, rtol=2e-6, atol=1e-7)
    assert all(float(ob2.state[r]["step"]) == 7.0 for r in ps_c)
    for r, q in zip(ps_c, ps_b):         # (it resumed from OUR moments: rounding-level differences)
        torch.testing.assert_close(r, q, rtol=1e-4, atol=1e-6)
    assert float(oa.state[ps_a[0]]["step"]) == 7.0
    if wd:                               # decoupled, not L2: an Adam of the same weight_decay is somewhere else
        assert oa.param_groups[0]["decoupled_weight_decay"] is True
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    fixed = [torch.randn_like(p) for p in ps_a]
    for p, q, f in zip(ps_a, ps_b, fixed):
        p.grad.copy_(f)
        q.grad = f.clone()
    with torch.cuda.stream(side):
        oa.step()
    torch.cuda.current_stream().wait_stream(side)
    ob.step()
    with torch.cuda.graph(g):
        oa.step()
    for _ in range(3):
        g.replay()
        ob.step()
    torch.cuda.synchronize()
    assert float(oa.state[ps_a[0]]["step"]) == 11.0
    for p, q in zip(ps_a, ps_b):
        torch.testing.assert_close(p, q, rtol=5e-6, atol=1e-7)


def test_adamw_decays_where_adam_adds_to_the_gradient():
    """One step from zero moments with weight_decay 0.5 on a parameter whose gradient is zero: Adam's L2 term moves it
    by lr (the normalised step), AdamW only shrinks it by 1 - lr * wd."""
    from connectome_gnn_amd.optim import Adam, AdamW
    out = {}
    for cls in (Adam, AdamW):
        p = torch.full((1025,), 2.0, device=DEV).requires_grad_(True)
        p.grad = torch.zeros_like(p)
        cls([p], lr=1e-2, weight_decay=0.5).step()
        out[cls] = p.detach()
    torch.cuda.synchronize()
    assert torch.equal(out[AdamW], torch.full_like(out[AdamW], 2.0 * float(torch.tensor(1.0 - 1e-2 * 0.5, dtype=torch.float32))))
    torch.testing.assert_close(out[Adam], torch.full_like(out[Adam], 2.0 - 1e-2), rtol=1e-6, atol=0)


# ------------------------------------------------------------------------------------------- 5-8. the Trainer
RTOL, ATOL = 2e-4, 2e-6       # test_the_unchanged_reference_script_is_served_from_the_device's, for the same pair of paths


def _trainer_run(make_opt, host: bool, gamma, epochs: int):
    """``epochs`` calls of train_epoch over 40 graphs in batches of 16 (16, 16, 8), StepLR(1, gamma) stepped after
    each (gamma None: no scheduler) -> trainer, train losses, final parameters, tr._graphs after every epoch."""
    import connectome_gnn_amd as C
    graphs = _dataset()
    torch.manual_seed(3)
    m = C.GCNConnectome(5, 64, dropout=0.0)
    opt = make_opt(m.parameters())
    tr = C.Trainer(m, opt, device="cuda", **({"resident": False, "graph": False} if host else {}))
    ld = C.ConnectomeDataLoader(graphs, batch_size=16, shuffle=True)
    sched = torch.optim.lr_scheduler.StepLR(opt, 1, gamma=gamma) if gamma is not None else None
    losses, kept = [], []
    for _ in range(epochs):
        losses.append(tr.train_epoch(ld))
        kept.append(dict(tr._graphs))
        if sched is not None:
            sched.step()
    torch.cuda.synchronize()
    assert len(m.convs) == len(m.batch_norms) == 3            # (every conv's bias feeds a BatchNorm: CANCELLED below)
    return tr, losses, {k: p.detach().clone() for k, p in m.named_parameters()}, kept


@functools.lru_cache(maxsize=None)
def _dataset():
    import connectome_gnn_amd as C
    return C.generate_dataset(40, 84, 8, seed=5)


@functools.lru_cache(maxsize=None)
def _host_run(gamma, epochs):
    """The reference semantics: eager steps from the host loader with torch.optim.Adam (computed once, never changed)
    -> losses, parameters by name, and the largest |gradient| of each parameter at the last step."""
    tr, losses, params, _ = _trainer_run(lambda ps: torch.optim.Adam(ps, lr=1e-2), True, gamma, epochs)
    grads = {k: float(p.grad.abs().max()) for k, p in tr.model.named_parameters()}
    return losses, params, grads


def _cancelled(name: str) -> bool:
    """A GCN layer's bias: BatchNorm follows it, and in training mode BatchNorm's output does not change when a
    constant is added to a channel -- the exact gradient of such a bias is zero."""
    import re
    return re.fullmatch(r"convs\.\d+\.bias", name) is not None


def _assert_follows_host(losses, params, gamma, epochs):
    """The train_loss history and the final parameters against the host run's, rtol 2e-4 / atol 2e-6 -- every
    parameter but the three biases that BatchNorm cancels.  What is computed for those is the rounding residue of a
    sum that is zero in exact arithmetic, and Adam divides a gradient by its own running magnitude: residue comes
    out as steps of about +-lr, a random walk that no two execution paths share (nor two optimizers: the host run
    repeated with optim.Adam in place of torch.optim.Adam leaves every other parameter within 1.2e-7 of this one and
    these biases 1.1e-2 / 1.2e-3 / 1.1e-3 away, their whole magnitude).  They are exempt on that ground alone, and
    the ground is asserted on the host run's own numbers: their gradient is below 1e-4 of their layer's weight
    gradient.  (The residue of an fp32 sum over 16 x 84 rows is about 2^-24 sqrt(1344) = 2e-6 of its terms: 1e-4
    leaves a factor of 50; a bias that mattered would have a gradient of the order of the weight's.)"""
    want_losses, want_params, want_grads = _host_run(gamma, epochs)
    torch.testing.assert_close(torch.tensor(losses), torch.tensor(want_losses), rtol=RTOL, atol=ATOL)
    assert list(params) == list(want_params) and sum(_cancelled(k) for k in params) == 3
    for k, q in want_params.items():
        if _cancelled(k):
            weight = k.replace(".bias", ".linear.weight")
            assert want_grads[k] <= 1e-4 * want_grads[weight], (k, want_grads[k], want_grads[weight])
        else:
            torch.testing.assert_close(params[k], q, rtol=RTOL, atol=ATOL, msg=lambda s: f"{k}: {s}")


def test_trainer_follows_a_schedule_with_a_torch_optimizer():
    """The unchanged reference script with StepLR(1, 0.1): the captured steps of torch's Adam freeze lr, so each epoch's
    change releases them and they are captured again; the trajectory is the host run's.  (Without that, the replays of
    epochs 2 and 3 keep lr = 1e-2: the third run below, which has no scheduler, is what they would compute.)"""
    tr, losses, params, _ = _trainer_run(lambda ps: torch.optim.Adam(ps, lr=1e-2), False, 0.1, 3)
    assert tr.graph and sorted(k[2] for k in tr._graphs if k[0] == "resident") == [8, 16]
    _assert_follows_host(losses, params, 0.1, 3)
    assert tr.hyper_recaptures > 0
    want_losses, want_params, _ = _host_run(0.1, 3)
    _, flat_losses, flat_params, _ = _trainer_run(lambda ps: torch.optim.Adam(ps, lr=1e-2), False, None, 3)
    a, b = torch.tensor(flat_losses), torch.tensor(want_losses)
    assert bool(((a - b).abs() > 10 * (ATOL + RTOL * b.abs())).any())
    assert all(bool(((flat_params[k] - q).abs() > 10 * (ATOL + RTOL * q.abs())).any())
               for k, q in want_params.items() if not _cancelled(k))


def test_trainer_follows_a_schedule_with_our_optimizer_without_recapture():
    from connectome_gnn_amd.optim import Adam
    tr, losses, params, kept = _trainer_run(lambda ps: Adam(ps, lr=1e-2), False, 0.1, 3)
    assert tr.graph and sorted(k[2] for k in tr._graphs if k[0] == "resident") == [8, 16]
    _assert_follows_host(losses, params, 0.1, 3)
    assert tr.hyper_recaptures == 0
    assert kept[0].keys() == kept[-1].keys() and all(kept[-1][k] is kept[0][k] for k in kept[0])
    assert tr.optimizer.param_groups[0]["lr"] == pytest.approx(1e-5)


def test_a_foreign_optimizer_outside_the_trainer_is_refused_once_stale():
    import connectome_gnn_amd as C
    from connectome_gnn_amd.graphed import GraphedTrainStep
    torch.manual_seed(2)
    b = C.collate_graphs(C.generate_dataset(8, 84, 8, seed=2)).to(DEV)
    m = C.GCNConnectome(5, 64, dropout=0.0).to(DEV).train()
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, capturable=True)
    step = GraphedTrainStep(m, opt, b, warmup=1)
    step()
    assert step.hyper_current()
    opt.param_groups[0]["lr"] = 1e-4
    assert not step.hyper_current()
    before = [p.detach().clone() for p in m.parameters()]
    with pytest.raises(RuntimeError, match=r"param_groups\[0\]\['lr'\] has changed"):
        step()
    torch.cuda.synchronize()
    assert all(torch.equal(p, q) for p, q in zip(m.parameters(), before))       # refused before any launch
    opt.param_groups[0]["lr"] = 1e-3
    step()
    torch.cuda.synchronize()
    assert not all(torch.equal(p, q) for p, q in zip(m.parameters(), before))


def test_the_remainder_batch_goes_eager():
    """The batch of 8 comes once per epoch; with lr changed after every epoch its captured step is stale each time it
    is met and never replays: after the third stale capture that key stays eager, with one warning, while the batches
    of 16 (replayed once per epoch) keep being captured again.  The trajectory is still the host run's."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        tr, losses, params, kept = _trainer_run(lambda ps: torch.optim.Adam(ps, lr=1e-2), False, 0.5, 4)
    stale = [w for w in caught if "went stale" in str(w.message)]
    assert len(stale) == 1, [str(w.message) for w in caught]
    assert "connectome_gnn_amd.optim.Adam" in str(stale[0].message) and "AdamW" in str(stale[0].message)
    assert "batches of 8 graphs" in str(stale[0].message)
    assert [k[2] for k in tr._eager_keys] == [8]
    assert sorted(k[2] for k in kept[2] if k[0] == "resident") == [8, 16]      # epochs 1-3: captured (again)
    assert sorted(k[2] for k in kept[3] if k[0] == "resident") == [16]         # epoch 4: the remainder ran eagerly
    assert tr.hyper_recaptures == 6                                            # two keys, stale at epochs 2, 3 and 4
    _assert_follows_host(losses, params, 0.5, 4)
