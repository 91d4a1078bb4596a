"""Fused optimisation step against the reference's torch calls (oracle/optim_ref.py)."""
import numpy as np
import pytest
import torch


SCHED = dict(max_lr=3e-4, total_steps=40, pct_start=0.3, div_factor=10, final_div_factor=1000)


@pytest.mark.parametrize("three_phase,anneal", [(False, "cos"), (True, "cos"), (False, "linear")])
def test_onecycle_mirror_matches_torch_scheduler(three_phase, anneal):
    """CPU: the host-side schedule reproduces OneCycleLR's lr and beta1 cycling at every step."""
    from gaviko_amd.optim import OneCycle
    from oracle import optim_ref
    p = [torch.nn.Parameter(torch.zeros(3))]
    opt, sch = optim_ref.make(p, lr=1e-3, eps=1e-8, anneal_strategy=anneal, three_phase=three_phase, **SCHED)
    mine = OneCycle(anneal_strategy=anneal, three_phase=three_phase, **SCHED)
    for t in range(SCHED["total_steps"]):
        lr, b1 = mine.at(t)
        assert abs(lr - opt.param_groups[0]["lr"]) <= 1e-12 + 1e-9 * lr
        assert abs(b1 - opt.param_groups[0]["betas"][0]) <= 1e-12
        p[0].grad = torch.ones(3)
        opt.step()
        if t + 1 < SCHED["total_steps"]:
            sch.step()


@pytest.mark.gpu
def test_fused_clip_adam_onecycle_matches_reference_step(dev):
    """GPU: 12 steps of gvk_sumsq + gvk_adam_step on 7 ragged tensors against clip_grad_norm_ + Adam + OneCycleLR on the CPU.
    Gradients alternate between large (clipped) and tiny (unclipped) so both branches run."""
    from gaviko_amd.optim import FusedAdamOneCycle
    from oracle import optim_ref
    g = torch.Generator().manual_seed(7)
    shapes = [(5,), (20, 768), (768, 20), (1,), (1025,), (3, 341), (64, 20)]
    ref = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    mine = [p.detach().clone().to(dev) for p in ref]
    total = sum(p.numel() for p in ref)
    flat = torch.zeros(total, device=dev)
    opt, sch = optim_ref.make(ref, lr=1e-3, eps=1e-8, **SCHED)
    fused = FusedAdamOneCycle(mine, lr=1e-3, eps=1e-8, max_norm=1.0, flat_grad=flat, **SCHED)
    for t in range(12):
        scale = 1.0 if t % 2 == 0 else 1e-4
        grads = [torch.randn(s, generator=g) * scale for s in shapes]
        for p, gr in zip(ref, grads):
            p.grad = gr.clone()
        flat.copy_(torch.cat([gr.reshape(-1) for gr in grads]).to(dev))
        n_ref = optim_ref.step(ref, opt, sch, 1.0)
        fused.step()
        torch.cuda.synchronize()
        assert abs(fused.grad_norm().item() - n_ref.item()) <= 1e-5 * n_ref.item()
        for p, q in zip(ref, mine):
            assert torch.allclose(q.cpu(), p.detach(), atol=1e-7, rtol=2e-6), t
        off = 0                                              # the stored gradients are the clipped ones, as torch leaves them
        for p in ref:
            assert torch.allclose(flat[off: off + p.numel()].cpu(), p.grad.reshape(-1), atol=1e-9, rtol=1e-5)
            off += p.numel()


@pytest.mark.gpu
def test_fused_optimizer_drives_a_model(dev):
    """GPU: the optimizer binds to a gaviko_amd model (flat gradient buffer + trainable tensors) and the loss goes down."""
    import test_model_gpu as tm
    from gaviko_amd.optim import FusedAdamOneCycle
    from gaviko_amd.utils import synth
    m, cfg = tm.build("gaviko", "vit-t16", dict(tm.GAVIKO), dev)
    opt = FusedAdamOneCycle(m, lr=1e-3, eps=1e-8, **SCHED)
    x = torch.from_numpy(synth.volumes(0, 2)).to(dev)
    y = torch.from_numpy(synth.labels(0, 2)).to(dev)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        loss = torch.nn.functional.cross_entropy(m(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert losses[-1] < losses[0], losses
    frozen = [p for n, p in m.named_parameters() if not p.requires_grad]
    assert all(p.grad is None for p in frozen)


@pytest.mark.gpu
def test_adam_moments_follow_names_when_the_flat_layout_moves(dev):
    """exp_avg / exp_avg_sq are positional in the flat gradient layout, and that layout is regrouped by make_reducer(mode=...)
    / set_bucket_layers; a same-size buffer used to be kept as is -- Adam state silently permuted against the parameters.  Step, change
    the layout, step again: every parameter must equal torch.optim.Adam's fed with the same gradients; the state dict carries the names
    and a state saved under one layout loads under another."""
    import test_model_gpu as tm
    from gaviko_amd.optim import FusedAdamOneCycle
    from gaviko_amd.utils import synth
    m, cfg = tm.build("gaviko", "vit-t16", dict(tm.GAVIKO), dev)
    named = dict(m.named_parameters())
    eng = m._engine()
    tr = eng.trainable_names()
    ref_p = {n: torch.nn.Parameter(named[n].detach().clone()) for n in tr}
    ref = torch.optim.Adam(list(ref_p.values()), lr=2e-3, eps=1e-8)
    opt = FusedAdamOneCycle(m, lr=2e-3, eps=1e-8, max_norm=None)
    x = torch.from_numpy(synth.volumes(0, 2)).to(dev)
    y = torch.from_numpy(synth.labels(0, 2)).to(dev)

    def one():
        opt.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()
        for n in tr:
            ref_p[n].grad = named[n].grad.detach().clone()
        ref.step()
        opt.step()
        torch.cuda.synchronize()

    def check(tag):
        for n in tr:
            assert torch.allclose(named[n].detach(), ref_p[n].detach(), rtol=2e-5, atol=2e-7), (tag, n)

    one(); one()
    check("before")
    order0 = list(eng.flat_names())
    sd = opt.state_dict()
    assert sd["names"] == order0 and sum(sd["numels"]) == sd["exp_avg"].numel()
    eng.set_bucket_layers(1)                                            # what make_reducer(layers_per_bucket=1) does to the layout
    assert list(eng.flat_names()) != order0
    one(); one()
    check("after the layout moved")
    # a state saved under the first layout, loaded into a fresh optimizer that binds under the second
    opt2 = FusedAdamOneCycle(m, lr=2e-3, eps=1e-8, max_norm=None)
    opt2.load_state_dict(sd)
    opt2._bind()
    off_new = {}
    o = 0
    for n in eng.flat_names():
        off_new[n] = o
        o += named[n].numel()
    o = 0
    for n, k in zip(sd["names"], sd["numels"]):
        assert torch.equal(opt2.m[off_new[n]: off_new[n] + k], sd["exp_avg"][o: o + k]), n
        o += k
    # a state that covers other tensors than the model trains is an error, not a silent reuse
    bad = dict(sd, names=["nope"] + sd["names"][1:])
    opt3 = FusedAdamOneCycle(m, lr=2e-3, eps=1e-8, max_norm=None)
    opt3.load_state_dict(bad)
    with pytest.raises(Exception, match="covers other tensors"):
        opt3._bind()


# ---------------------------------------------------------------------------------------------------------------------------------
# the whole schedule, the plain configurations, non-finite gradients, state round trips, legacy (name-less) states

SHAPES3 = [(5,), (1025,), (3, 341)]
KW = dict(lr=1e-3, eps=1e-8)


def _pair(shapes, dev, seed):
    """-> (generator, torch reference parameters on the CPU, the same values on the device, their flat gradient buffer)."""
    g = torch.Generator().manual_seed(seed)
    ref = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in shapes]
    mine = [p.detach().clone().to(dev) for p in ref]
    return g, ref, mine, torch.zeros(sum(p.numel() for p in ref), device=dev)


def _feed(ref, flat, grads):
    for p, gr in zip(ref, grads):
        p.grad = gr.clone()
    flat[: sum(gr.numel() for gr in grads)].copy_(torch.cat([gr.reshape(-1) for gr in grads]))


def _moments(opt, ref):
    """torch.optim.Adam's exp_avg / exp_avg_sq in the flat layout."""
    return tuple(torch.cat([opt.state[p][k].reshape(-1) for p in ref]) for k in ("exp_avg", "exp_avg_sq"))


def _moments_close(fused, opt, ref, gmax, steps):
    """exp_avg / exp_avg_sq against torch's after `steps` steps on the same gradients.  Both sides run the same fp32 recurrences; what
    differs is the clip factor (the two norms are asserted to agree within 1e-5 relative) and <= 8 roundings per step and side.  m is a
    weighted mean of the clipped gradients with weights summing to < 1 and may cancel, so its error is bounded by the largest gradient
    magnitude the element saw (gmax), not by |m|; v sums non-negative terms in g^2, so twice that, relative to v."""
    m_ref, v_ref = _moments(opt, ref)
    m, v = fused.m.cpu(), fused.v.cpu()
    assert torch.equal(torch.isnan(m), torch.isnan(m_ref)) and torch.equal(torch.isnan(v), torch.isnan(v_ref))
    ok = ~torch.isnan(m_ref)
    tol = 1e-5 + 8 * steps * 2.0 ** -24
    assert ((m - m_ref).abs()[ok] <= tol * gmax[ok]).all()
    assert ((v - v_ref).abs()[ok] <= 2 * tol * v_ref[ok]).all()


def _same(mine, ref, tag):
    for q, p in zip(mine, ref):
        assert torch.allclose(q.cpu(), p.detach(), atol=1e-7, rtol=2e-6), tag


@pytest.mark.gpu
@pytest.mark.parametrize("three_phase,anneal", [(False, "cos"), (True, "cos"), (False, "linear")])
def test_fused_step_follows_the_whole_schedule(dev, three_phase, anneal):
    """GPU: all 40 steps of the 40-step schedule -- warm-up, the descending anneal(s), the last steps where the bias corrections approach 1
    and lr reaches max_lr / div / final_div -- against clip_grad_norm_ + Adam + OneCycleLR on the CPU, with the assertions of
    test_fused_clip_adam_onecycle_matches_reference_step at every step and no re-synchronisation of the two runs.  A 41st step() raises
    the schedule's ValueError and leaves the step count, the parameters and the moments alone."""
    from gaviko_amd.optim import FusedAdamOneCycle
    from oracle import optim_ref
    shapes = [(5,), (20, 768), (768, 20), (1,), (1025,), (3, 341), (64, 20)]
    g, ref, mine, flat = _pair(shapes, dev, 7)
    opt, sch = optim_ref.make(ref, anneal_strategy=anneal, three_phase=three_phase, **KW, **SCHED)
    fused = FusedAdamOneCycle(mine, max_norm=1.0, flat_grad=flat, anneal_strategy=anneal, three_phase=three_phase, **KW, **SCHED)
    steps = SCHED["total_steps"]
    for t in range(steps):
        scale = 1.0 if t % 2 == 0 else 1e-4
        _feed(ref, flat, [torch.randn(s, generator=g) * scale for s in shapes])
        assert abs(fused.get_last_lr()[0] - opt.param_groups[0]["lr"]) <= 1e-9 * opt.param_groups[0]["lr"]
        if t + 1 < steps:
            n_ref = optim_ref.step(ref, opt, sch, 1.0)
        else:                                                # OneCycleLR itself refuses the scheduler step after the last optimizer step
            n_ref = torch.nn.utils.clip_grad_norm_(ref, 1.0)
            opt.step()
        fused.step()
        torch.cuda.synchronize()
        assert abs(fused.grad_norm().item() - n_ref.item()) <= 1e-5 * n_ref.item()
        _same(mine, ref, t)
        off = 0
        for p in ref:
            assert torch.allclose(flat[off: off + p.numel()].cpu(), p.grad.reshape(-1), atol=1e-9, rtol=1e-5)
            off += p.numel()
    lr_min = SCHED["max_lr"] / SCHED["div_factor"] / SCHED["final_div_factor"]
    assert abs(opt.param_groups[0]["lr"] - lr_min) <= 1e-9 * lr_min and abs(fused.schedule.at(steps - 1)[0] - lr_min) <= 1e-9 * lr_min
    before = [t.clone() for t in mine + [fused.m, fused.v]]
    with pytest.raises(ValueError, match="beyond total_steps"):
        fused.step()
    torch.cuda.synchronize()
    assert fused.t == steps
    assert all(torch.equal(a, b) for a, b in zip(mine + [fused.m, fused.v], before))


@pytest.mark.gpu
@pytest.mark.parametrize("max_norm", [1.0, None])
def test_fused_step_without_schedule_matches_plain_adam(dev, max_norm):
    """GPU: max_lr=None is a constant lr and beta1 -- torch.optim.Adam with no scheduler, 6 steps on an explicit (params, flat_grad) pair.
    max_norm=None launches no gvk_sumsq and hands the kernel no norm: the gradient buffer keeps its bits."""
    from gaviko_amd.optim import FusedAdamOneCycle
    g, ref, mine, flat = _pair(SHAPES3, dev, 8)
    opt = torch.optim.Adam(ref, **KW)
    fused = FusedAdamOneCycle(mine, max_norm=max_norm, flat_grad=flat, **KW)
    gmax = torch.zeros(flat.numel())
    for t in range(6):
        _feed(ref, flat, [torch.randn(s, generator=g) * (3.0 if t % 2 == 0 else 1e-4) for s in SHAPES3])
        kept = flat.clone()
        gmax = torch.maximum(gmax, kept.cpu().abs())
        assert fused.current() == (1e-3, 0.9) and fused.get_last_lr() == [1e-3]
        if max_norm is not None:
            n_ref = torch.nn.utils.clip_grad_norm_(ref, max_norm)
        opt.step()
        fused.step()
        torch.cuda.synchronize()
        _same(mine, ref, t)
        if max_norm is None:
            assert torch.equal(flat.view(torch.int32), kept.view(torch.int32))
        else:
            assert abs(fused.grad_norm().item() - n_ref.item()) <= 1e-5 * n_ref.item()
            assert torch.allclose(flat.cpu(), torch.cat([p.grad.reshape(-1) for p in ref]), atol=1e-9, rtol=1e-5)
    _moments_close(fused, opt, ref, gmax, 6)


@pytest.mark.gpu
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_non_finite_gradients_behave_as_in_torch(dev, bad):
    """GPU: one ordinary step, then a step with ONE non-finite gradient element, against clip_grad_norm_ + Adam (oracle/optim_ref.step).
    NaN: the norm and with it clip are NaN, so every gradient, moment and parameter turns NaN (a min() that drops the NaN would poison
    that one element only).  +inf: the norm is inf and clip 0, the inf element turns NaN (inf * 0) and every other gradient 0.  These are
    values in buffers: the launches finish normally."""
    from gaviko_amd.optim import FusedAdamOneCycle
    from oracle import optim_ref
    g, ref, mine, flat = _pair(SHAPES3, dev, 9)
    opt, sch = optim_ref.make(ref, **KW, **SCHED)
    fused = FusedAdamOneCycle(mine, max_norm=1.0, flat_grad=flat, **KW, **SCHED)
    where = SHAPES3[0][0] + 700                               # inside the second tensor
    gmax = torch.zeros(flat.numel())
    for t in range(2):
        grads = [torch.randn(s, generator=g) for s in SHAPES3]
        if t == 1:
            grads[1][700] = bad
        _feed(ref, flat, grads)
        gmax = torch.maximum(gmax, flat.cpu().abs())
        n_ref = optim_ref.step(ref, opt, sch, 1.0)
        fused.step()
        torch.cuda.synchronize()
    n, n_ref = fused.grad_norm().cpu().reshape(()), n_ref.reshape(())
    assert torch.equal(torch.isnan(n), torch.isnan(n_ref)) and torch.equal(torch.isinf(n), torch.isinf(n_ref))
    assert bool(torch.isnan(n)) if bad != bad else bool(torch.isinf(n))
    m_ref, v_ref = _moments(opt, ref)
    _moments_close(fused, opt, ref, gmax, 2)
    got = dict(p=torch.cat([q.reshape(-1) for q in mine]), g=flat, m=fused.m, v=fused.v)
    want = dict(p=torch.cat([p.detach().reshape(-1) for p in ref]), g=torch.cat([p.grad.reshape(-1) for p in ref]), m=m_ref, v=v_ref)
    for k in got:
        a, b = got[k].cpu(), want[k]
        assert torch.equal(torch.isnan(a), torch.isnan(b)), k
        assert not torch.isinf(a).any() and not torch.isinf(b).any(), k
        if k in "pg":                                        # the bounds of the finite runs; m and v: _moments_close above
            assert torch.allclose(a, b, equal_nan=True, **(dict(atol=1e-7, rtol=2e-6) if k == "p" else dict(atol=1e-9, rtol=1e-5))), k
        if bad != bad:
            assert torch.isnan(a).all(), k
        else:
            assert torch.isnan(a).nonzero().reshape(-1).tolist() == [where], k
    if bad == bad:
        others = torch.ones(flat.numel(), dtype=torch.bool)
        others[where] = False
        assert not got["g"].cpu()[others].any()


@pytest.mark.gpu
def test_resumed_optimizer_continues_bit_for_bit(dev):
    """GPU: 5 steps, state_dict(), a fresh optimizer over clones of the parameters loads it, and both take 5 more steps on the same
    gradients mid-schedule: parameters, moments and get_last_lr() are identical at every step."""
    from gaviko_amd.optim import FusedAdamOneCycle
    g, _, mine, flat = _pair(SHAPES3, dev, 10)
    a = FusedAdamOneCycle(mine, max_norm=1.0, flat_grad=flat, **KW, **SCHED)
    draw = lambda t: torch.cat([torch.randn(s, generator=g).reshape(-1) for s in SHAPES3]).to(dev) * (1.0 if t % 2 == 0 else 1e-4)
    for t in range(5):
        flat.copy_(draw(t))
        a.step()
    sd = a.state_dict()
    assert sd["t"] == 5 and sd["names"] == ["#0", "#1", "#2"] and sd["numels"] == [5, 1025, 1023]
    clones, flat_b = [p.clone() for p in mine], torch.zeros_like(flat)
    b = FusedAdamOneCycle(clones, max_norm=1.0, flat_grad=flat_b, **KW, **SCHED)
    b.load_state_dict(sd)
    assert b.get_last_lr() == a.get_last_lr() and b.get_last_lr() != FusedAdamOneCycle(clones, flat_grad=flat_b, **KW, **SCHED).get_last_lr()
    for t in range(5, 10):
        gr = draw(t)
        flat.copy_(gr)
        flat_b.copy_(gr)
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert a.t == b.t == t + 1 and a.get_last_lr() == b.get_last_lr()
        assert all(torch.equal(p, q) for p, q in zip(mine, clones)), t
        assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and torch.equal(a.grad_norm(), b.grad_norm()), t
    assert sd["t"] == 5 and not torch.equal(sd["exp_avg"], a.m)          # the state dict is a copy, not a view of the live moments


@pytest.mark.gpu
def test_a_moved_parameter_is_rebound_and_keeps_its_moments(dev):
    """GPU: after 2 steps one parameter's storage moves (p.data = p.data.clone()).  The next step() rebuilds its tables (the pointer
    signature changed), keeps the moments, matches torch, and does not write the old storage."""
    from gaviko_amd.optim import FusedAdamOneCycle
    from oracle import optim_ref
    g, ref, mine, flat = _pair(SHAPES3, dev, 12)
    opt, sch = optim_ref.make(ref, **KW, **SCHED)
    fused = FusedAdamOneCycle(mine, max_norm=1.0, flat_grad=flat, **KW, **SCHED)

    gmax = torch.zeros(flat.numel())

    def steps(k, tag):
        nonlocal gmax
        for t in range(k):
            _feed(ref, flat, [torch.randn(s, generator=g) for s in SHAPES3])
            gmax = torch.maximum(gmax, flat.cpu().abs())
            optim_ref.step(ref, opt, sch, 1.0)
            fused.step()
            torch.cuda.synchronize()
            _same(mine, ref, (tag, t))

    steps(2, "before")
    old = mine[1].data                                        # shares the storage the tables point to
    old_bits, m_before = old.clone(), fused.m.clone()
    mine[1].data = mine[1].data.clone()
    assert mine[1].data_ptr() != old.data_ptr()
    steps(2, "after")
    assert torch.equal(old.view(torch.int32), old_bits.view(torch.int32)), "the old storage was written"
    assert not torch.equal(mine[1], old_bits)
    assert m_before.abs().max() > 0
    _moments_close(fused, opt, ref, gmax, 4)


@pytest.mark.gpu
def test_grad_norm_before_a_step_and_a_never_stepped_state(dev):
    """GPU: grad_norm() before any step is a GavikoHipError that says so.  A state dict taken before any step (no moments yet) loads into
    an optimizer that has already stepped and resets it: with the parameters put back, its next steps equal a fresh optimizer's."""
    from gaviko_amd.lib import GavikoHipError
    from gaviko_amd.optim import FusedAdamOneCycle
    g, _, mine, flat = _pair(SHAPES3, dev, 13)
    start = [p.clone() for p in mine]
    a = FusedAdamOneCycle(mine, max_norm=1.0, flat_grad=flat, **KW, **SCHED)
    with pytest.raises(GavikoHipError, match="no step has run"):
        a.grad_norm()
    sd0 = a.state_dict()
    assert sd0["t"] == 0 and sd0["exp_avg"] is None and sd0["exp_avg_sq"] is None
    grads = [torch.cat([torch.randn(s, generator=g).reshape(-1) for s in SHAPES3]).to(dev) for _ in range(4)]
    for gr in grads[:2]:
        flat.copy_(gr)
        a.step()
    a.load_state_dict(sd0)
    assert a.t == 0 and a.m is None and a.v is None
    with pytest.raises(GavikoHipError, match="no step has run"):
        a.grad_norm()
    for p, s in zip(mine, start):
        p.copy_(s)
    fresh_p, flat_b = [s.clone() for s in start], torch.zeros_like(flat)
    b = FusedAdamOneCycle(fresh_p, max_norm=1.0, flat_grad=flat_b, **KW, **SCHED)
    for gr in grads[2:]:
        flat.copy_(gr)
        flat_b.copy_(gr)
        a.step()
        b.step()
        torch.cuda.synchronize()
        assert all(torch.equal(p, q) for p, q in zip(mine, fresh_p))
        assert torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


class _StubEngine:
    """What load_state_dict reads of an engine: the trainable tensors in named_parameters() order, the model kind and its config."""
    kind = "gaviko"

    def __init__(self, numels, share_factor=1):
        self.p = {n: torch.nn.Parameter(torch.zeros(k)) for n, k in numels.items()}
        self.cfg = dict(share_factor=share_factor)

    def trainable_names(self):
        return list(self.p)


class _StubModel:
    def __init__(self, eng):
        self._eng = eng

    def _engine(self):
        return self._eng


def test_nameless_state_is_loaded_only_when_its_layout_is_known():
    """CPU: a model-bound state without `names` is in trainable_names() order or in flat_order(.., 4) order, and its size cannot tell
    which.  Where the two differ the load is refused unless legacy_order= picks one (legacy_layers_per_bucket= for a reducer that did
    not group by 4 layers); where they coincide it is accepted; a size that contradicts the layout is the numel error; a refused load
    changes nothing; the explicit-params form stays positional."""
    from gaviko_amd.distributed import flat_order
    from gaviko_amd.lib import GavikoHipError
    from gaviko_amd.optim import FusedAdamOneCycle
    numels = {"prompt_embeddings": 3, "transformer.layers.0.a.weight": 5, "transformer.layers.2.a.weight": 7,
              "transformer.layers.5.a.weight": 11, "mlp_head.head.weight": 2}
    named = list(numels)
    flat4 = ["transformer.layers.5.a.weight", "transformer.layers.0.a.weight", "transformer.layers.2.a.weight", "prompt_embeddings",
             "mlp_head.head.weight"]
    flat1 = ["transformer.layers.5.a.weight", "transformer.layers.2.a.weight", "transformer.layers.0.a.weight", "prompt_embeddings",
             "mlp_head.head.weight"]
    assert flat_order(named, 1, 4) == flat4 and flat_order(named, 1, 1) == flat1 and flat4 != named
    total = sum(numels.values())
    sd = dict(t=2, exp_avg=torch.arange(total, dtype=torch.float32), exp_avg_sq=torch.arange(total, dtype=torch.float32) + 100)
    layout = lambda order: [(n, numels[n]) for n in order]

    opt = FusedAdamOneCycle(_StubModel(_StubEngine(numels)))
    with pytest.raises(GavikoHipError, match="legacy_order='named'.*legacy_order='flat'"):
        opt.load_state_dict(sd)
    assert opt.t == 0 and opt.m is None and opt.v is None and opt._layout is None
    for kw, order in ((dict(legacy_order="flat"), flat4), (dict(legacy_order="named"), named),
                      (dict(legacy_order="flat", legacy_layers_per_bucket=1), flat1)):
        opt = FusedAdamOneCycle(_StubModel(_StubEngine(numels)))
        opt.load_state_dict(sd, **kw)
        assert opt._layout == layout(order) and opt.t == 2
        assert torch.equal(opt.m, sd["exp_avg"]) and torch.equal(opt.v, sd["exp_avg_sq"]) and opt.m is not sd["exp_avg"]
        # and the bind-time re-ordering carries every stretch to its tensor's place in another layout
        moved = FusedAdamOneCycle._relayout(opt.m, opt._layout, layout(named))
        at = {n: o for n, o in zip(order, np.cumsum([0] + [numels[n] for n in order]))}
        assert torch.equal(moved, torch.cat([sd["exp_avg"][at[n]: at[n] + numels[n]] for n in named]))
    with pytest.raises(GavikoHipError, match="legacy_order must be"):
        opt.load_state_dict(sd, legacy_order="bucketed")
    for order in ("flat", "named"):
        with pytest.raises(GavikoHipError, match="do not have the size"):
            opt.load_state_dict(dict(sd, exp_avg=sd["exp_avg"][:-1], exp_avg_sq=sd["exp_avg_sq"][:-1]), legacy_order=order)
    assert opt.t == 2 and opt.m.numel() == total
    # names recorded: the keyword is not consulted
    opt.load_state_dict(dict(sd, names=flat1, numels=[numels[n] for n in flat1]))
    assert opt._layout == layout(flat1)
    # no layer-indexed tensor: both candidates are the same list, nothing to choose
    plain = {"prompt_embeddings": 3, "mlp_head.head.weight": 2}
    opt = FusedAdamOneCycle(_StubModel(_StubEngine(plain)))
    opt.load_state_dict(dict(t=1, exp_avg=torch.zeros(5), exp_avg_sq=torch.zeros(5)))
    assert opt._layout == list(plain.items())
    # explicit params: positional
    ps = [torch.zeros(4), torch.zeros(6)]
    opt = FusedAdamOneCycle(ps, flat_grad=torch.zeros(10))
    opt.load_state_dict(dict(t=3, exp_avg=torch.zeros(10), exp_avg_sq=torch.zeros(10)))
    assert opt._layout == [("#0", 4), ("#1", 6)]
    with pytest.raises(GavikoHipError, match="do not have the size"):
        opt.load_state_dict(dict(t=3, exp_avg=torch.zeros(9), exp_avg_sq=torch.zeros(9)))


@pytest.mark.gpu
def test_nameless_state_lands_on_its_tensors_in_a_model(dev):
    """GPU, ADVICE round 5: a state saved without names used to be taken as trainable_names() order although the revisions that grouped
    the flat buffer stored flat_names() order -- same size, so every moment was silently paired with another parameter.  Two steps of
    the tiny GAViKO model, then the same moments as a name-less state in either order: with the matching legacy_order= every tensor's
    moments sit at that tensor's current offset (under a layout that differs from both), and one more step equals torch.optim.Adam
    continued from those moments; with no keyword the load is refused, and a state of another size is the numel error."""
    import test_model_gpu as tm
    from gaviko_amd.distributed import flat_order
    from gaviko_amd.lib import GavikoHipError
    from gaviko_amd.optim import FusedAdamOneCycle
    from gaviko_amd.utils import synth
    m, cfg = tm.build("gaviko", "vit-t16", dict(tm.GAVIKO), dev)
    named = dict(m.named_parameters())
    eng = m._engine()
    tr = list(eng.trainable_names())
    opt = FusedAdamOneCycle(m, lr=2e-3, eps=1e-8, max_norm=None)
    x = torch.from_numpy(synth.volumes(0, 2)).to(dev)
    y = torch.from_numpy(synth.labels(0, 2)).to(dev)

    def backward(o):
        o.zero_grad()
        torch.nn.functional.cross_entropy(m(x), y).backward()

    for _ in range(2):
        backward(opt)
        opt.step()
    torch.cuda.synchronize()
    sd = opt.state_dict()
    mom, o = {}, 0
    for n, k in zip(sd["names"], sd["numels"]):
        mom[n] = (sd["exp_avg"][o: o + k].clone(), sd["exp_avg_sq"][o: o + k].clone())
        o += k
    flat4 = flat_order(tr, 1, 4)
    assert flat4 != tr and sorted(flat4) == sorted(tr)       # the two candidate layouts differ for this model: nothing below is vacuous
    state = lambda order: dict(t=sd["t"], exp_avg=torch.cat([mom[n][0] for n in order]), exp_avg_sq=torch.cat([mom[n][1] for n in order]))
    eng.set_bucket_layers(1)                                  # bind under a third layout, so that both loads have to move every group
    assert list(eng.flat_names()) not in (flat4, tr)

    for kw, order in ((dict(legacy_order="flat"), flat4), (dict(legacy_order="named"), tr)):
        o2 = FusedAdamOneCycle(m, lr=2e-3, eps=1e-8, max_norm=None)
        o2.load_state_dict(state(order), **kw)
        backward(o2)
        o2._bind()
        off = 0
        for n in eng.flat_names():
            k = named[n].numel()
            assert torch.equal(o2.m[off: off + k], mom[n][0]) and torch.equal(o2.v[off: off + k], mom[n][1]), (kw, n)
            off += k
        ref_p = {n: torch.nn.Parameter(named[n].detach().clone()) for n in tr}
        ref = torch.optim.Adam(list(ref_p.values()), lr=2e-3, eps=1e-8)
        for n in tr:
            ref_p[n].grad = named[n].grad.detach().clone()
            ref.state[ref_p[n]] = dict(step=torch.tensor(float(sd["t"])), exp_avg=mom[n][0].clone().view_as(ref_p[n]),
                                       exp_avg_sq=mom[n][1].clone().view_as(ref_p[n]))
        ref.step()
        o2.step()
        torch.cuda.synchronize()
        assert o2.t == sd["t"] + 1
        for n in tr:
            assert torch.allclose(named[n].detach(), ref_p[n].detach(), rtol=2e-5, atol=2e-7), (kw, n)

    o3 = FusedAdamOneCycle(m, lr=2e-3, eps=1e-8, max_norm=None)
    with pytest.raises(GavikoHipError, match="legacy_order"):
        o3.load_state_dict(state(flat4))
    assert o3.t == 0 and o3.m is None
    short = state(flat4)
    short = dict(short, exp_avg=short["exp_avg"][:-1], exp_avg_sq=short["exp_avg_sq"][:-1])
    with pytest.raises(GavikoHipError, match="do not have the size"):
        o3.load_state_dict(short, legacy_order="flat")
